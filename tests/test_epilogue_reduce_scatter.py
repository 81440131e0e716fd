"""Host model of the closure kernel's reduce-scatter epilogue (csrc/ndq_mlp.h: reduce_scatter, rs_swizzle,
block_reduce_store_rs) against what it replaces.

* point_sum() adds the 16 lanes of a DPP row by row_ror 8, 4, 2, 1 and leaves every lane with the total.
  reduce_scatter() runs the same pairings on 16 values at once and leaves lane p with the total of value p.  Both
  networks of adds are modelled lane by lane in fp32, driven by the DPP controls the header itself names, and compared
  bit for bit: no sum may be re-associated.
* rs_swizzle() moves the entries of a layer's 32 x 32 block inside that block: an involution and a bijection of
  [0, 1024); the deposits of a wave then fall on distinct banks and the final pass's reads stay conflict-free.
* the per-unit totals, one per lane after the reduce-scatter, are deposited at exactly the places the unit-by-unit stores
  wrote.
"""
import os
import re

import numpy as np
import pytest

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "neurodiffeq_amd", "csrc", "ndq_mlp.h")


def _source():
    with open(HEADER) as fh:
        return fh.read()


def dpp(v, ctrl):
    """What __builtin_amdgcn_update_dpp(0, v, ctrl, 0xf, 0xf, false) hands each of the 16 lanes of a row (v: [16, ...]);
    a lane whose source lies outside the row keeps `old`, i.e. 0."""
    out = np.zeros_like(v)
    for i in range(16):
        if ctrl < 0x100:                                      # quad_perm: two bits per lane of the quad
            src = (i & ~3) + ((ctrl >> (2 * (i & 3))) & 3)
        elif 0x101 <= ctrl <= 0x10f:                          # row_shl:n -- lane i reads lane i + n
            src = i + (ctrl & 15)
        elif 0x111 <= ctrl <= 0x11f:                          # row_shr:n -- lane i reads lane i - n
            src = i - (ctrl & 15)
        elif 0x121 <= ctrl <= 0x12f:                          # row_ror:n -- lane i reads lane (i - n) mod 16
            src = (i - (ctrl & 15)) % 16
        else:
            raise AssertionError(hex(ctrl))
        if 0 <= src < 16:
            out[i] = v[src]
    return out


def point_sum_model(v, ctrls):
    for c in ctrls:
        v = v + dpp(v, c)
    return v


def reduce_scatter_model(x, levels, plain8):
    """x: [16 lanes, N values] -> [16 lanes]; levels: (LO, HI, H2) of the rs_level calls; plain8: the N = 8 variant, whose
    distance-8 step is point_sum's own."""
    p = np.arange(16)
    x = x.copy()
    if plain8:
        x = x + dpp(x, 0x128)
        levels = levels[1:]
    for lo_c, hi_c, h in levels:
        assert x.shape[1] >= 2 * h
        lo = x[:, :h] + dpp(x[:, :h], lo_c)
        hi = x[:, h:2 * h] + dpp(x[:, h:2 * h], hi_c)
        up = (p & h) != 0
        x = np.where(up[:, None], hi, lo)
    return x[:, 0]


def _controls():
    src = _source()
    ps = src[src.index("real point_sum(real v)"):]
    point = [int(c, 16) for c in re.findall(r"dpp_add<(0x[0-9a-f]+)>", ps[:ps.index("return v;")])]
    rs = src[src.index("float reduce_scatter(float (&x)[N], int p)"):]
    rs = rs[:rs.index("return x[0];")]
    levels = [(int(a, 16), int(b, 16), int(h)) for a, b, h in re.findall(r"rs_level<(0x[0-9a-f]+), (0x[0-9a-f]+), (\d+)>", rs)]
    masks = [int(m) for m in re.findall(r"\(p & (\d+)\) != 0", rs)]
    return point, levels, masks


def _values(rng, n):
    """[16 lanes, n values] of fp32: many exponents, both signs, signed zeros, exact cancellations."""
    v = (rng.standard_normal((16, n)) * np.exp2(rng.integers(-60, 60, (16, n)))).astype(np.float32)
    v[rng.random((16, n)) < 0.1] = 0.0
    v[rng.random((16, n)) < 0.1] = -0.0
    for k in range(0, n, 7):                                 # partners that cancel at every distance
        d = (1, 2, 4, 8)[(k // 7) % 4]
        i = int(rng.integers(0, 16))
        v[i ^ d, k] = -v[i, k]
    return v


def test_header_controls_are_the_xor_butterfly():
    point, levels, masks = _controls()
    assert point == [0x128, 0x124, 0x122, 0x121]
    assert [h for _, _, h in levels] == [8, 4, 2, 1] and masks == [8, 4, 2, 1]
    lane = np.arange(16, dtype=np.float32)
    for lo_c, hi_c, h in levels:                             # the lanes that keep the lower / upper half read lane i ^ h
        lo, hi = dpp(lane, lo_c), dpp(lane, hi_c)
        for i in range(16):
            assert (hi if i & h else lo)[i] == (i ^ h), (hex(lo_c), hex(hi_c), i)


@pytest.mark.parametrize("seed", range(4))
def test_reduce_scatter_adds_in_point_sums_tree_bit_for_bit(seed):
    point, levels, _ = _controls()
    rng = np.random.default_rng(seed)
    x = _values(rng, 16 * 64)
    want = point_sum_model(x, point)                         # [16 lanes, values]: every lane the total
    assert (want.view(np.uint32) == want.view(np.uint32)[:1]).all(), "point_sum leaves the lanes with different bits"
    for g in range(0, x.shape[1], 16):
        got = reduce_scatter_model(x[:, g:g + 16], levels, False)
        assert (got.view(np.uint32) == want[0, g:g + 16].view(np.uint32)).all(), (g, got, want[0, g:g + 16])
        got8 = reduce_scatter_model(x[:, g:g + 8], levels, True)
        assert (got8.view(np.uint32) == want[0, np.arange(16) % 8 + g].view(np.uint32)).all(), g
    with np.errstate(invalid="ignore", over="ignore"):
        naive = x.sum(axis=0, dtype=np.float32)              # the yardstick has teeth: another order, other bits
    assert (naive.view(np.uint32) != want[0].view(np.uint32)).any()


def swizzle(e):
    return e ^ (((e >> 8) & 1) << 5) ^ (((e >> 7) & 1) << 4)


def test_swizzle_is_the_headers_and_an_involution_and_a_bijection():
    assert "return e ^ (((e >> 8) & 1) << 5) ^ (((e >> 7) & 1) << 4);" in _source()
    e = np.arange(1024)
    s = swizzle(e)
    assert sorted(s) == list(e) and (swizzle(s) == e).all()
    assert (s >> 9 == e >> 9).all() and ((s >> 6) & 7 == (e >> 6) & 7).all()      # only row bit 0 and the column half move


def _deposit_addresses(jb, kb, r):
    """Region offsets (in floats, relative to the layer's block) of the 64 lanes' store of accumulator entry
    (j, k) = (16 jb + 4 q + r, 16 kb + p), as block_reduce_store_rs forms them."""
    lane = np.arange(64)
    p, q = lane & 15, lane >> 4
    at = (4 * q + ((r & 1) ^ (q >> 1))) * 32 + 16 * (kb ^ (q & 1)) + p
    return 512 * jb + 32 * (r & 2) + at, (16 * jb + 4 * q + r) * 32 + 16 * kb + p


def test_matrix_deposits_hit_distinct_banks_at_the_swizzled_places():
    src = _source()
    assert "at[rb][kb] = (4 * q + (rb ^ (q >> 1))) * 32 + 16 * (kb ^ (q & 1)) + p;" in src
    assert "512 * jb + 32 * (r & 2) + at[r & 1][kb]" in src
    seen = []
    for base in (0, 96, 1188 + 96, 7 * 1188 + 96):           # a constant offset (region, layer) only rotates the banks
        for jb in range(2):
            for kb in range(2):
                for r in range(4):
                    addr, e = _deposit_addresses(jb, kb, r)
                    assert (addr == swizzle(e)).all()
                    assert len(set((base + addr) % 64)) == 64            # 64 banks x 4 B: no two lanes of the wave on one
                    for half in (addr[:32], addr[32:]):                  # ds_write_b32: two groups of 32 lanes, 32 banks
                        assert len(set((base + half) % 32)) == 32
                    plain = e                                            # the parent's places: 4 lanes per bank
                    assert len(set(plain % 64)) == 16
                    if base == 0:
                        seen.extend(addr)
    assert sorted(seen) == list(range(1024))                 # every place of the block written exactly once


def test_final_pass_reads_stay_conflict_free():
    """Thread i of the final pass reads entry i through the swizzle; the blocks start on multiples of 32 floats, so 32
    consecutive threads read one row: 32 distinct banks (ds_read_b32: two groups of 32 lanes), and 64 consecutive threads
    two runs of 32 in different halves of 64 banks."""
    for off in (96, 96 + 1056):
        assert off % 32 == 0
        for i0 in range(off, off + 1024, 64):
            i = np.arange(i0, i0 + 64)
            at = off + swizzle(i - off)
            for half in (at[:32], at[32:]):
                assert len(set(half % 32)) == 32 and half.max() - half.min() == 31
            assert len(set(at % 64)) == 64


@pytest.mark.parametrize("nin,layers", [(2, 2), (1, 2), (3, 1), (2, 3)])
def test_dense_deposits_write_every_per_unit_sum_once(nin, layers):
    """Octets (W1 column by column, b1, b_2 .. b_L, Wout) are reduced in pairs; lane (q, p) of pair g then holds octet
    2 g + (p >> 3), unit 16 b + 4 q + r with (b, r) = ((p >> 2) & 1, p & 3).  An odd last octet is held twice (p, p ^ 8)
    and stored by p < 8."""
    off_w1, off_b1 = 0, 32 * nin
    off_w = lambda l: 32 * nin + 32 + (l - 2) * (1024 + 32)          # noqa: E731
    off_b = lambda l: off_w(l) + 1024                                  # noqa: E731
    n_oct = nin + layers + 1
    off = [off_w1 + o for o in range(nin)] + [off_b1] + [off_b(l) for l in range(2, layers + 1)] + [off_w(layers + 1)]
    stride = [nin] * nin + [1] * (layers + 1)
    assert len(off) == n_oct
    want = {}
    for j in range(32):                                              # block_reduce_store's unit-by-unit places
        for d in range(nin):
            want[off_w1 + j * nin + d] = ("w1", d, j)
        want[off_b1 + j] = ("b1", j)
        for l in range(2, layers + 1):
            want[off_b(l) + j] = ("b", l, j)
        want[off_w(layers + 1) + j] = ("wout", j)
    names = [("w1", d) for d in range(nin)] + [("b1",)] + [("b", l) for l in range(2, layers + 1)] + [("wout",)]
    got = {}
    for g in range((n_oct + 1) // 2):
        for q in range(4):
            for p in range(16):
                unit = 16 * ((p >> 2) & 1) + 4 * q + (p & 3)
                if 2 * g + 1 < n_oct:
                    o = 2 * g + (p >> 3)
                elif p < 8:
                    o = 2 * g
                else:
                    continue
                place = off[o] + unit * stride[o]
                assert place not in got
                got[place] = names[o] + (unit,)
    assert got == want
