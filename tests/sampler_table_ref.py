"""TEST INFRASTRUCTURE ONLY -- numpy restatement of the table sampler (neurodiffeq_amd/csrc/ndq_sample.h:
sample_table_kernel; include/ndq.h: ndq_sample_table) on top of the pinned Philox restatement of oracle/philox_ref.py.

Per point i: block A = Philox counter (i, draw_lo, draw_hi, stream) -- ``philox_ref.words`` -- gives the normals of axes
0..2 exactly as ``philox_ref.sample_grid`` derives them; block B, counter word 0 = i | 0x80000000, gives those of axes
3..5 the same way.  Integer work is bit-exact with the kernel, the float transforms agree to a few ulp (libm against the
device's fast log / sin / cos)."""
import numpy as np

from oracle import philox_ref as P
from oracle.philox_ref import words, u01, u01_open

NORMAL, CHEB2_NOISY = 0, 1          # NDQ_AXIS_* of include/ndq.h
F = np.float32


def words_b(n, seed, draw, stream_id):
    """Block B of every point: ``philox_ref.words`` with the top bit of counter word 0 set."""
    i = np.arange(n, dtype=np.uint64) | np.uint64(0x80000000)
    ctr = [i, np.full(n, draw & 0xFFFFFFFF, np.uint64), np.full(n, (draw >> 32) & 0xFFFFFFFF, np.uint64),
           np.full(n, stream_id, np.uint64)]
    return P.philox4x32_10(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))


def normals3(w):
    """Three of the four Box-Muller normals of one block: the lines of ``philox_ref.sample_grid``."""
    two_pi = F(6.283185307179586)
    r0, t0 = np.sqrt(F(-2.0) * np.log(u01_open(w[0]))), two_pi * u01(w[1])
    r1, t1 = np.sqrt(F(-2.0) * np.log(u01_open(w[2]))), two_pi * u01(w[3])
    return [(r0 * np.cos(t0)).astype(F), (r0 * np.sin(t0)).astype(F), (r1 * np.cos(t1)).astype(F)]


def normals(total, d, seed, draw, stream_id=0):
    """z_0 .. z_{d-1} of every point; block B only when d > 3."""
    z = normals3(words(total, seed, draw, stream_id))
    if d > 3:
        z += normals3(words_b(total, seed, draw, stream_id))
    return z[:d]


def sample_table(spec, seed, draw, stream_id=0):
    """``spec``: a ``generators.TableSpec`` -> [d][total] fp32, what ndq_sample_table writes."""
    total = int(np.prod(spec.n))
    if spec.law[0] == CHEB2_NOISY:                      # generators.py: _chebyshev_second_noisy, in fp32 like torch
        w = words(total, seed, draw, stream_id)
        t = (np.arange(total).astype(F) + (F(2.0) * u01(w[0]) - F(1.0))) / F(spec.n[0] - 1) * F(np.pi)
        lo, hi = F(spec.lo[0]), F(spec.hi[0])
        return (((lo + hi) + (hi - lo) * np.cos(t)) / F(2.0)).astype(F)[None]
    z = normals(total, spec.d, seed, draw, stream_id)
    idx = np.unravel_index(np.arange(total), spec.n)   # ij order, last axis fastest
    out = []
    for c in range(spec.d):
        v = spec.mean[c][idx[c]]
        if spec.std[c] is not None:
            w = spec.std[c][idx[c]]
            v = np.where(w != 0, v + w * z[c], v)
        out.append((np.abs(v) if spec.abs_value else v).astype(F))
    return np.stack(out)
