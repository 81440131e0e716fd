"""TEST INFRASTRUCTURE ONLY -- numpy restatement of the indexed plan sampler (neurodiffeq_amd/csrc/ndq_sample.h:
sample_plan_indexed_kernel; include/ndq.h: ndq_sample_plan_indexed): ResampleGenerator / BatchGenerator directly above a plan.

Output point i of draw t is element r of inner draw k (``window``); r is mapped to the plan point j (``index_map``: identity,
uniform indices with replacement, or the swap-or-not shuffle); the values are those of tests/sampler_plan_ref.sample_plan for
draw k, gathered at j.  All of it is integer work on Philox words, so kernel and restatement agree bit for bit on the indices."""
import numpy as np

from oracle import philox_ref as P
from tests import sampler_plan_ref as R

GOLDEN = 0x9E3779B97F4A7C15
U32 = np.uint32


def plan_index_seed(seed):
    """The key of the index map: the leaves of a plan own the multipliers 0..7 (sampler_plan_ref.leaf_seed)."""
    return (seed + 8 * GOLDEN) % 2 ** 64


def window(t, bs, m, size):
    """(k, r) of the output points 0 .. size - 1 of draw t, in exact (python) integers: without a batch (bs == 0) inner draw t
    itself, else elements [t * bs, (t + 1) * bs) of the concatenated stream of inner draws of m points each."""
    if not bs:
        return [t] * size, list(range(size))
    g = [t * bs + i for i in range(size)]
    return [x // m for x in g], [x % m for x in g]


def window_k0r0(t, bs, m, size):
    """The launcher's form of ``window``: k0 / r0 of output point 0 in 64 bits, then 32-bit arithmetic per point."""
    g0 = (t * bs) % 2 ** 64
    k0, r0 = (g0 // m, g0 % m) if bs else (t, 0)
    u = (np.uint32(r0) + np.arange(size, dtype=U32)).astype(U32)
    assert r0 + size - 1 < 2 ** 32
    return [(k0 + int(q)) % 2 ** 64 for q in u // U32(m)], [int(x) for x in u % U32(m)]


def rounds(n):
    return 2 * int(n - 1).bit_length() + 8


def fmix32(h):
    """murmur3's 32-bit finaliser on uint32 arrays (the products wrap)."""
    h = h.astype(U32)
    h = h ^ (h >> U32(16))
    h = h * U32(0x85EBCA6B)
    h = h ^ (h >> U32(13))
    h = h * U32(0xC2B2AE35)
    return h ^ (h >> U32(16))


def _umulhi(w, n):
    return ((w.astype(np.uint64) * np.uint64(n)) >> np.uint64(32)).astype(U32)


def _counter(word0, ks, stream_id):
    """Philox counters (word0[a], k_lo[b], k_hi[b], stream_id) for every (a, b), flattened a-major."""
    a, b = len(word0), len(ks)
    lo = np.array([k & 0xFFFFFFFF for k in ks], dtype=np.uint64)
    hi = np.array([(k >> 32) & 0xFFFFFFFF for k in ks], dtype=np.uint64)
    return [np.repeat(np.asarray(word0, dtype=np.uint64), b), np.tile(lo, a), np.tile(hi, a), np.full(a * b, stream_id, np.uint64)]


def round_keys(n, ks, seed, stream_id=0):
    """(K, S), each [rounds][len(ks)] uint32: round q of inner draw k shuffles with K_q = umulhi(B.x, n), S_q = B.y,
    B = Philox4x32-10(counter (q | 2^31, k_lo, k_hi, stream_id), key plan_index_seed(seed))."""
    s = plan_index_seed(seed)
    nr = rounds(n)
    q = np.arange(nr, dtype=np.uint64) | np.uint64(0x80000000)
    b = P.philox4x32_10(_counter(q, ks, stream_id), (s & 0xFFFFFFFF, s >> 32))
    return _umulhi(b[0], n).reshape(nr, len(ks)), b[1].reshape(nr, len(ks))


def index_map(mode, n, m, k, seed, stream_id=0):
    """j(r) for r = 0 .. m - 1 of inner draw ``k`` (int64 [m]); ``k`` may be a sequence of draws: [len(k)][m]."""
    ks = [int(k)] if np.isscalar(k) else [int(x) for x in k]
    r = np.arange(m, dtype=U32)
    if mode == "none":
        assert m == n
        j = np.broadcast_to(r, (len(ks), m))
    elif mode == "replace":
        s = plan_index_seed(seed)
        w = P.philox4x32_10(_counter(r, ks, stream_id), (s & 0xFFFFFFFF, s >> 32))[0]
        j = _umulhi(w, n).reshape(m, len(ks)).T
    else:
        assert mode == "permute" and m <= n
        K, S = round_keys(n, ks, seed, stream_id)
        x = np.broadcast_to(r, (len(ks), m)).copy()
        for q in range(rounds(n)):
            Kq, Sq = K[q][:, None], S[q][:, None]
            p = np.where(Kq >= x, Kq - x, Kq + U32(n) - x).astype(U32)         # (K - x) mod n; K + n < 2^32
            coin = fmix32(np.maximum(x, p) ^ Sq) >> U32(31)
            x = np.where(coin == 1, p, x)
        j = x
    j = j.astype(np.int64)
    return j[0] if np.isscalar(k) else j


def gather_indexed(plan, seed, t, stream_id, rows_of):
    """[d][plan.size]: ``rows_of(k)`` ([d][n], the plan's rows of inner draw k) gathered through window and index map of draw t."""
    ix = plan.index
    ks, rs = window(t, ix.batch, ix.m, plan.size)
    ks, rs = np.array(ks, dtype=object), np.array(rs)
    out = None
    for k in sorted(set(ks)):
        sel = np.nonzero(ks == k)[0]
        rows = np.asarray(rows_of(int(k)))
        assert rows.shape == (plan.d, ix.n)
        if out is None:
            out = np.empty((plan.d, plan.size), dtype=rows.dtype)
        j = index_map(ix.mode, ix.n, ix.m, int(k), seed, stream_id)
        out[:, sel] = rows[:, j[rs[sel]]]
    return out


def sample_plan_indexed(plan, seed, t, stream_id=0):
    """``plan``: a ``generators.PlanSpec`` with ``index`` set -> [d][plan.size] fp32, what ndq_sample_plan_indexed writes for
    draw ``t``: per inner draw k the un-indexed restatement (tests/sampler_plan_ref.sample_plan), gathered."""
    return gather_indexed(plan, seed, t, stream_id, lambda k: R.sample_plan(plan, seed, k, stream_id))
