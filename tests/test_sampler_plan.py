"""Plan route of the device sampler (csrc/ndq_sample.h: sample_plan_kernel, include/ndq.h: ndq_sample_plan,
generators.plan_spec / DeviceGenerator): g1 + g2, g1 * g2, g1 ^ g2, Static / Predefined generators drawn on the MI355X in one
launch.  On the CPU: the normal form and its refusals, the numpy restatement (tests/sampler_plan_ref.py) -- leaf seeds,
independence of the leaves, mesh marginals --, descriptor validation.  On the GPU: the kernel against the composition of
per-leaf DeviceGenerator draws and against the restatement, exactness, reproducibility, fp64 hand-out, a solver training on
composed batches, live changes."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

from oracle import philox_ref as P
from tests import sampler_plan_ref as R
from tests import sampler_table_ref as T
from neurodiffeq_amd import _lib
from neurodiffeq_amd import generators as G
from neurodiffeq_amd.generators import (BaseGenerator, BatchGenerator, ConcatGenerator, DeviceGenerator, EnsembleGenerator,
                                        FilterGenerator, Generator1D, Generator2D, Generator3D, GeneratorND,
                                        GeneratorSpherical, MeshGenerator, PredefinedGenerator, ResampleGenerator,
                                        SamplerGenerator, StaticGenerator, TransformGenerator, device_source, table_spec)


def _np(t):
    return t.detach().cpu().numpy().reshape(-1)


def _shape(p):
    return [(f.kind, f.row0, f.rows, f.size) for f in p.leaves]


# ---------------------------------------------------------------------------------------------------------- host side
def test_plan_spec_accepted_shapes():
    torch.manual_seed(0)
    a, b, c = Generator1D(5), Generator1D(6, 0.1, 2.0, "log-spaced-noisy"), Generator1D(7, method="equally-spaced")
    # a lone leaf: a plan of one segment
    p = G.plan_spec(a)
    assert (p.d, p.size, p.segments, _shape(p)) == (1, 5, [("leaf", 0, 1, 0, 5)], [("simple", 0, 1, 5)]) and p.leaves[0].gen is a
    # (a + b) + c: flattened, leaves depth-first
    p = G.plan_spec((a + b) + c)
    assert (p.d, p.size) == (1, 18) and [f.gen for f in p.leaves] == [a, b, c]
    assert p.segments == [("leaf", 0, 1, 0, 5), ("leaf", 1, 1, 5, 6), ("leaf", 2, 1, 11, 7)]
    assert _shape(p) == [("simple", 0, 1, 5), ("table", 0, 1, 6), ("simple", 0, 1, 7)] and len(p.wrappers) == 2
    # (a * b) * c: one ensemble, rows in leaf order
    e1, e2, e3 = Generator1D(9), Generator2D((3, 3)), Generator1D(9, 0.1, 2.0, "chebyshev2-noisy")
    p = G.plan_spec((e1 * e2) * e3)
    assert (p.d, p.size, p.segments) == (4, 9, [("ensemble", 0, 3, 0, 9)]) and [f.gen for f in p.leaves] == [e1, e2, e3]
    assert _shape(p) == [("simple", 0, 1, 9), ("simple", 1, 2, 9), ("table", 3, 1, 9)]
    # a three-factor mesh
    p = G.plan_spec(a ^ b ^ c)
    assert (p.d, p.size, p.segments) == (3, 210, [("mesh", 0, 3, 0, 210)])
    assert _shape(p) == [("simple", 0, 1, 5), ("table", 1, 1, 6), ("simple", 2, 1, 7)]
    # a concat of {leaf, ensemble, mesh} with equal d
    p = G.plan_spec(Generator2D((4, 4)) + Generator1D(9) * Generator1D(9) + (Generator1D(3) ^ Generator1D(5)))
    assert (p.d, p.size) == (2, 40)
    assert p.segments == [("leaf", 0, 1, 0, 16), ("ensemble", 1, 2, 16, 9), ("mesh", 3, 2, 25, 15)]
    assert _shape(p) == [("simple", 0, 2, 16), ("simple", 0, 1, 9), ("simple", 1, 1, 9), ("simple", 0, 1, 3), ("simple", 1, 1, 5)]
    # a 6-row ensemble; a GeneratorND leaf counts its table size (`cut` shortens the draw, not `size`)
    nd = GeneratorND((4, 3, 2, 2), (0.0,) * 4, (1.0,) * 4, ("equally-spaced",) * 4, cut=((None, -1), (None, None), (None, None), (None, None)))
    assert nd.size == 48
    ens = BaseGenerator.__new__(EnsembleGenerator)
    ens.generators, ens.size = (nd, Generator1D(36), Generator1D(36)), 36
    p = G.plan_spec(ens)
    assert (p.d, p.size, p.segments) == (6, 36, [("ensemble", 0, 3, 0, 36)])
    assert _shape(p) == [("table", 0, 4, 36), ("simple", 4, 1, 36), ("simple", 5, 1, 36)]
    # 8 leaves
    g = lambda n: Generator1D(n)
    p = G.plan_spec(g(2) * g(2) + (g(2) ^ g(3)) + g(4) * g(4) + (g(1) ^ g(5)))
    assert (p.d, p.size, len(p.leaves)) == (2, 17, 8)
    assert p.segments == [("ensemble", 0, 2, 0, 2), ("mesh", 2, 2, 2, 6), ("ensemble", 4, 2, 8, 4), ("mesh", 6, 2, 12, 5)]
    assert [f.row0 for f in p.leaves] == [0, 1] * 4


def test_plan_spec_data_leaves_are_the_generators_own_tensors():
    torch.manual_seed(1)
    inner = Generator2D((6, 5), (0, -1), (1, 1))
    st = StaticGenerator(inner)
    p = G.plan_spec(st)
    assert (p.d, p.size, p.segments, _shape(p)) == (2, 30, [("leaf", 0, 1, 0, 30)], [("data", 0, 2, 30)])
    for row, ex in zip(p.leaves[0].data, st.examples):
        assert row.dtype == np.float32 and np.array_equal(row.view(np.uint32), _np(ex).view(np.uint32))
    # a StaticGenerator is DATA whatever it wraps: a latin-hypercube draw, a wrapper
    for wrapped in (Generator1D(8, method="latin-hypercube"), Generator1D(4) ^ Generator1D(3), Generator1D(8) + Generator1D(3)):
        st = StaticGenerator(wrapped)
        p = G.plan_spec(st)
        ex = [st.examples] if isinstance(st.examples, torch.Tensor) else list(st.examples)
        assert _shape(p) == [("data", 0, len(ex), ex[0].numel())]
        assert all(np.array_equal(row.view(np.uint32), _np(e).view(np.uint32)) for row, e in zip(p.leaves[0].data, ex))
    pre = PredefinedGenerator([0.5, 1.5, 2.5], [1.0, 2.0, 3.0], [-1.0, 0.0, 1.0])
    p = G.plan_spec(GeneratorSpherical(10) + pre)
    assert (p.d, p.size, _shape(p)) == (3, 13, [("simple", 0, 3, 10), ("data", 0, 3, 3)])
    assert all(np.array_equal(row, _np(x)) for row, x in zip(p.leaves[1].data, pre.xs))
    one = PredefinedGenerator([0.25, 0.75])
    p = G.plan_spec(one ^ Generator1D(3))
    assert _shape(p) == [("data", 0, 1, 2), ("simple", 1, 1, 3)] and np.array_equal(p.leaves[0].data[0], _np(one.xs))


def test_plan_spec_refusals_name_the_node():
    a, b = Generator1D(4), Generator1D(4)
    g2 = Generator2D((2, 2))

    def forced(cls, *gens):                     # what the constructors would not build, or what a callback could leave behind
        w = BaseGenerator.__new__(cls)
        w.generators, w.size = tuple(gens), gens[0].size
        return w

    lh = Generator1D(8, method="latin-hypercube")
    refused = {
        "Concat inside Mesh": ((a + b) ^ Generator1D(3), "ConcatGenerator inside MeshGenerator"),
        "Concat inside Ensemble": ((a + b) * Generator1D(8), "ConcatGenerator inside EnsembleGenerator"),
        "Mesh inside Ensemble": ((Generator1D(2) ^ Generator1D(2)) * a, "MeshGenerator inside EnsembleGenerator"),
        "Ensemble inside Mesh": ((a * b) ^ a, "EnsembleGenerator inside MeshGenerator"),
        "multi-row mesh factor": (g2 ^ a, "Generator2D"),
        "different row counts": (a + g2, "Generator2D"),
        "more than 6 rows": (forced(EnsembleGenerator, Generator3D((2, 2, 1)), Generator3D((2, 2, 1)), a), "7 rows"),
        "more than 8 leaves": (ConcatGenerator(*[Generator1D(4) for _ in range(9)]), "9 leaves"),
        "latin-hypercube": (lh, "latin-hypercube"),
        "latin-hypercube inside a wrapper": (a + lh + b, "latin-hypercube"),
        "ensemble members of different sizes": (forced(EnsembleGenerator, a, Generator1D(5)), r"\[4, 5\]"),
        "Transform": (a + TransformGenerator(b, transform=lambda x: x), "TransformGenerator"),
        "Filter": (FilterGenerator(a, lambda x: x > 0), "FilterGenerator"),
        "Resample": (ResampleGenerator(a) * b, "ResampleGenerator"),
        "Batch": (BatchGenerator(a, 2) ^ b, "BatchGenerator"),
        "Sampler": (SamplerGenerator(a) + b, "SamplerGenerator"),
    }
    for what, (g, match) in refused.items():
        with pytest.raises(ValueError, match=match):
            G.plan_spec(g)
    # the single-leaf descriptions keep refusing wrappers
    with pytest.raises(ValueError):
        table_spec(a + b)
    with pytest.raises(ValueError):
        DeviceGenerator.describe(a * b)
    with pytest.raises(ValueError):
        DeviceGenerator.describe(GeneratorND((4, 4)))


def test_leaf_seeds_of_the_restatement():
    assert R.leaf_seed(77, 0) == 77 == G.plan_leaf_seed(77, 0)
    assert R.leaf_seed(77, 3) == G.plan_leaf_seed(77, 3) == (77 + 3 * 0x9E3779B97F4A7C15) % 2 ** 64
    assert G.plan_leaf_seed(2 ** 64 - 1, 1) == 0x9E3779B97F4A7C15 - 1                      # mod 2^64
    assert len({G.plan_leaf_seed(5, l) for l in range(8)}) == 8
    torch.manual_seed(0)
    g1 = Generator1D(33, 0.1, 12.0, "log-spaced-noisy")
    g2 = Generator2D((11, 3), (0, -1), (1, 1))
    g3 = Generator1D(33, 0.0, 2.0, "uniform")
    plan = G.plan_spec(g2 * g1 * g3)
    for seed, draw, stream in ((7, 0, 0), (2 ** 64 - 5, 2 ** 32 + 1, 3)):
        got = R.sample_plan(plan, seed, draw, stream)
        # leaf 0: the existing restatement under `seed` itself; leaf l: under seed_l
        assert np.array_equal(got[0:2], P.sample_grid((11, 3), (0, -1), (1, 1), [g2.noise_xstd, g2.noise_ystd], seed, draw, stream))
        assert np.array_equal(got[2:3], T.sample_table(table_spec(g1), R.leaf_seed(seed, 1), draw, stream))
        assert np.array_equal(got[3:4], P.sample_uniform(33, [0.0], [2.0], R.leaf_seed(seed, 2), draw, stream))
        # ... in a concat and in a mesh as well: the leaf-local index is counter word 0
        cat = R.sample_plan(G.plan_spec(g3 + g1), seed, draw, stream)
        assert np.array_equal(cat[0, :33], P.sample_uniform(33, [0.0], [2.0], seed, draw, stream)[0])
        assert np.array_equal(cat[0, 33:], T.sample_table(table_spec(g1), R.leaf_seed(seed, 1), draw, stream)[0])
        mesh = R.sample_plan(G.plan_spec(g3 ^ g1), seed, draw, stream).reshape(2, 33, 33)
        assert np.array_equal(mesh[0, :, 0], P.sample_uniform(33, [0.0], [2.0], seed, draw, stream)[0])
        assert np.array_equal(mesh[1, 0, :], T.sample_table(table_spec(g1), R.leaf_seed(seed, 1), draw, stream)[0])


def test_leaves_of_a_plan_are_independent():
    """n = 4 096 points per leaf: the jitters of two noisy leaves at equal local indices are uncorrelated (|r| < 5 / sqrt(n)),
    and so are those of the SAME leaf used twice in a mesh (the reference draws g ^ g as two independent draws)."""
    n = 4096
    bound = 5.0 / np.sqrt(n)
    a, b = Generator1D(n, 0.0, 1.0, "equally-spaced-noisy"), Generator1D(n, 0.1, 12.0, "log-spaced-noisy")
    jitter = lambda g, row: (row.astype(np.float64) - _np(g.examples)) / g.noise_std
    for draw in (0, 1):
        rows = R.sample_plan(G.plan_spec(a * b), 11, draw)
        ja, jb = jitter(a, rows[0]), jitter(b, rows[1])
        assert 0.9 < ja.std() < 1.1 and 0.9 < jb.std() < 1.1
        r = np.corrcoef(ja, jb)[0, 1]
        print(f"draw {draw}: two leaves r = {r:.4f} (bound {bound:.4f})")
        assert abs(r) < bound
        plan = G.plan_spec(a ^ a)                       # (the spec of a 4 096 x 4 096 mesh: nothing of that size is built)
        assert plan.size == n * n and plan.leaves[0].gen is plan.leaves[1].gen
        first, second = R.leaf_draws(plan, 11, draw)
        r = np.corrcoef(jitter(a, first[0]), jitter(a, second[0]))[0, 1]
        print(f"draw {draw}: one leaf twice r = {r:.4f} (bound {bound:.4f})")
        assert abs(r) < bound and not np.array_equal(first, second)


def test_mesh_marginals_are_constant_across_partner_nodes():
    torch.manual_seed(0)
    f0, f1, f2 = Generator1D(5, method="equally-spaced-noisy"), Generator1D(4, 0.1, 3.0, "chebyshev2-noisy"), Generator1D(6)
    plan = G.plan_spec(f0 ^ f1 ^ f2)
    rows = R.sample_plan(plan, 3, 1, 2).reshape(3, 5, 4, 6)
    leaves = R.leaf_draws(plan, 3, 1, 2)
    assert np.array_equal(rows[0], np.broadcast_to(leaves[0][0][:, None, None], (5, 4, 6)))
    assert np.array_equal(rows[1], np.broadcast_to(leaves[1][0][None, :, None], (5, 4, 6)))
    assert np.array_equal(rows[2], np.broadcast_to(leaves[2][0][None, None, :], (5, 4, 6)))
    assert len(set(leaves[0][0])) == 5 and len(set(leaves[2][0])) == 6


# ------------------------------------------------------------------------------------------------- descriptor validation
def _simple(n, kind=R.GRID, d=1):
    s = _lib.SamplerDesc()
    s.kind, s.d = kind, d
    for c in range(d):
        s.n[c], s.lo[c], s.hi[c] = n, 0.0, 1.0
    return s


def _leaf(desc, l, kind, row0, rows, n=0, simple=None, table=None, data=None):
    f = desc.leaf[l]
    f.kind, f.row0, f.rows, f.n = kind, row0, rows, n
    if simple is not None:
        f.u.simple = simple
    if table is not None:
        f.u.table = table
    for c, ptr in enumerate(data or ()):
        f.u.data[c] = ptr


def _table(n, mean):
    t = _lib.TableSamplerDesc()
    t.d, t.n[0], t.law[0], t.mean[0] = 1, n, T.NORMAL, mean
    return t


def _valid(ptr):
    """16 points of 2 rows: an ensemble of a 1-D grid and a 1-D table (8 points), then a mesh of DATA (2) x uniform (4)."""
    d = _lib.PlanSamplerDesc()
    d.d, d.n_leaves, d.n_segments = 2, 4, 2
    _leaf(d, 0, _lib.NDQ_LEAF_SIMPLE, 0, 1, simple=_simple(8))
    _leaf(d, 1, _lib.NDQ_LEAF_TABLE, 1, 1, table=_table(8, ptr))
    _leaf(d, 2, _lib.NDQ_LEAF_DATA, 0, 1, n=2, data=[ptr])
    _leaf(d, 3, _lib.NDQ_LEAF_SIMPLE, 1, 1, simple=_simple(4, R.UNIFORM))
    for k, seg in enumerate(((_lib.NDQ_SEG_ENSEMBLE, 0, 2, 0, 8), (_lib.NDQ_SEG_MESH, 2, 2, 8, 8))):
        d.seg[k].mode, d.seg[k].first, d.seg[k].count, d.seg[k].offset, d.seg[k].size = seg
    return d


def _invalid_plans(ptr):
    out = {}

    def case(what, ldc=64):
        d = _valid(ptr)
        out[what] = (d, ldc)
        return d
    case("d = 0").d = 0
    case("d = 7").d = 7
    case("no leaves").n_leaves = 0
    case("9 leaves").n_leaves = 9
    case("no segments").n_segments = 0
    case("more segments than leaves").n_segments = 5
    case("leaves left over").n_leaves = 5
    case("a segment that does not start at the next leaf").seg[1].first = 1
    case("a segment without leaves").seg[1].count = 0
    case("unknown mode").seg[0].mode = 3
    case("a LEAF segment of two leaves").seg[0].mode = _lib.NDQ_SEG_LEAF
    case("unknown leaf kind").leaf[0].kind = 3
    case("ensemble leaf sizes disagree").leaf[0].u.simple.n[0] = 9
    case("ensemble size is not the leaves'").seg[0].size = 9
    d = case("a multi-row mesh factor")
    d.d = 3
    _leaf(d, 0, _lib.NDQ_LEAF_SIMPLE, 0, 2, simple=_simple(8, R.UNIFORM, 2))
    d.leaf[1].row0 = 2
    _leaf(d, 2, _lib.NDQ_LEAF_DATA, 0, 2, n=2, data=[ptr, ptr])
    d.leaf[3].row0 = 2
    case("mesh product is not the segment's size").leaf[2].n = 3
    case("a row written twice").leaf[1].row0 = 0
    case("a row never written").d = 3
    case("a row outside the block").leaf[3].row0 = 2
    case("a negative row").leaf[0].row0 = -1
    case("rows other than the law's d").leaf[0].rows = 2
    case("offset is not the sum of the earlier sizes").seg[1].offset = 9
    case("ldc < total", ldc=15)
    d = case("more than 2^31 - 1 points", ldc=2 ** 31 - 1)
    d.d, d.n_leaves, d.n_segments = 1, 2, 2
    for k in range(2):
        _leaf(d, k, _lib.NDQ_LEAF_SIMPLE, 0, 1, simple=_simple(2 ** 30, R.UNIFORM))
        d.seg[k].mode, d.seg[k].first, d.seg[k].count, d.seg[k].offset, d.seg[k].size = _lib.NDQ_SEG_LEAF, k, 1, k * 2 ** 30, 2 ** 30
    # a leaf its own entry point would refuse
    case("simple leaf: unknown law").leaf[0].u.simple.kind = 7
    case("simple leaf: n = 0").leaf[3].u.simple.n[0] = 0
    case("table leaf: no mean table").leaf[1].u.table.mean[0] = None
    case("table leaf: unknown law").leaf[1].u.table.law[0] = 2
    d = case("table leaf: CHEB2_NOISY with n = 1")
    d.leaf[1].u.table.law[0], d.leaf[1].u.table.n[0] = T.CHEB2_NOISY, 1
    case("DATA leaf: a null row").leaf[2].u.data[0] = None
    case("DATA leaf: n = 0").leaf[2].n = 0
    case("DATA leaf: 7 rows").leaf[2].rows = 7
    return out


def _assert_all_refused(coords_ptr, table_ptr, stream=None):
    L = _lib.lib()
    for what, (desc, ldc) in _invalid_plans(table_ptr).items():
        assert L.ndq_sample_plan(ctypes.byref(desc), 1, 0, 0, coords_ptr, ldc, stream) == -2, what       # NDQ_EINVAL
    assert L.ndq_sample_plan(None, 1, 0, 0, coords_ptr, 64, stream) == -2
    assert L.ndq_sample_plan(ctypes.byref(_valid(table_ptr)), 1, 0, 0, None, 64, stream) == -2


def test_invalid_plan_descriptors_are_refused_on_the_host():
    """Argument validation precedes any launch, so it is reachable without a GPU (the pointers are never followed)."""
    _assert_all_refused(0x2000, 0x1000)
    assert ctypes.sizeof(_lib.PlanSamplerDesc) == 16 + 8 * (16 + 200) + 8 * 20          # the layout of include/ndq.h


# ---------------------------------------------------------------------------------------------------- on the MI355X
def _close(got, want, scale):                   # tests/test_sampler_table.py: kernel against restatement
    return np.abs(got - want).max() <= 4e-6 * scale


def _rows(dg):
    return [_np(v).copy() for v in dg.get_examples()]


def _nd4():
    return GeneratorND((2, 3, 2, 2), (0.0, 0.5, 0.0, 1.0), (1.0, 2.0, 1.0, 3.0), ("equally-spaced", "log-spaced", "chebyshev2", "equally-spaced"))


def _eight():
    g = lambda n, m="equally-spaced-noisy": Generator1D(n, 0.0, 2.0, m)
    return g(5) * g(5, "uniform") + (g(3) ^ g(4)) + g(7, "equally-spaced") * g(7) + (g(1) ^ g(6, "uniform"))


# name: (generator, per leaf: the scale of each of its rows).  `scale` is the magnitude of the row's box, as in
# tests/test_sampler_table.py, and every jitter width is <= scale / 8.
PLAN_CASES = {
    "concat-37-100-7": (lambda: Generator1D(37, 0.0, 1.0, "equally-spaced-noisy") + Generator1D(100, 0.1, 12.0, "log-spaced-noisy")
                        + Generator1D(7, -2.0, 3.0, "uniform"), [(1.0,), (12.0,), (5.0,)]),
    "concat-300": (lambda: Generator1D(130, 0.0, 1.0, "equally-spaced-noisy") + Generator1D(170, -1.0, 3.0, "chebyshev2-noisy"),
                   [(1.0,), (3.0,)]),
    "mesh-5-1-7": (lambda: Generator1D(5, 0.0, 1.0, "equally-spaced") ^ Generator1D(1, 1.0, 1.0, "equally-spaced")
                   ^ Generator1D(7, 0.0, 2.0, "equally-spaced-noisy"), [(1.0,), (1.0,), (2.0,)]),
    "mesh-three-laws": (lambda: Generator1D(6, -2.0, 3.0, "uniform") ^ Generator1D(5, -1.0, 3.0, "chebyshev2-noisy")
                        ^ Generator1D(4, 0.1, 12.0, "log-spaced"), [(5.0,), (3.0,), (12.0,)]),
    "ensemble-2d-1d": (lambda: Generator2D((3, 5), (0, -1), (1, 1), "equally-spaced-noisy") * Generator1D(15, 0.0, 2.0),
                       [(1.0, 1.0), (2.0,)]),
    "concat-of-all": (lambda: Generator2D((4, 4)) + Generator1D(9) * Generator1D(9) + (Generator1D(3) ^ Generator1D(5)),
                      [(1.0, 1.0), (1.0,), (1.0,), (1.0,), (1.0,)]),
    "six-rows": (lambda: _nd4() * Generator1D(24, 0.0, 2.0) * Generator1D(24, 0.0, 1.0, "equally-spaced-noisy"),
                 [(1.0, 2.0, 1.0, 3.0), (2.0,), (1.0,)]),
    "eight-leaves": (_eight, [(2.0,)] * 8),
    "spherical+predefined": (lambda: GeneratorSpherical(50, 0.1, 3.0) + PredefinedGenerator(
        *[np.linspace(0.1, hi, 11).astype(np.float32) for hi in (3.0, np.pi, 2 * np.pi)]), [(3.0, np.pi, 2 * np.pi)] * 2),
}


def _leaf_kernel_rows(plan, seed, stream, draw):
    """What a DeviceGenerator of each leaf alone hands out under the leaf's seed (DATA leaves: their host tensors)."""
    out = []
    for l, f in enumerate(plan.leaves):
        if f.kind == "data":
            out.append(np.stack(f.data))
            continue
        dg = DeviceGenerator(f.gen, seed=G.plan_leaf_seed(seed, l), stream_id=stream)
        assert dg.plan is None
        dg.draw = draw
        out.append(np.stack(_rows(dg)))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PLAN_CASES))
def test_plan_kernel_matches_the_composition_of_leaf_draws(name):
    torch.manual_seed(123)
    make, scales = PLAN_CASES[name]
    g = make()
    plan = G.plan_spec(g)
    assert len(scales) == len(plan.leaves) and all(len(s) == f.rows for s, f in zip(scales, plan.leaves))
    ones = lambda f, values: np.stack([np.full(f.size, v) for v in values])
    scale = R.compose(plan, [ones(f, s) for f, s in zip(plan.leaves, scales)])
    exact = R.compose(plan, [ones(f, R.leaf_exact_rows(f)) for f in plan.leaves]).astype(bool)
    bit_equal = True
    for stream in (0, 3):
        dg = DeviceGenerator(g, seed=99, stream_id=stream)
        assert dg.plan is not None and dg.size == plan.size and len(dg.blocks) == 1 and dg.block.shape == (plan.d, (plan.size + 63) // 64 * 64)
        for k, draw in enumerate((0, 1, 2 ** 32 + 1)):       # the last one: the high word of the draw counter
            dg.block.fill_(-7.0)
            dg.draw = draw
            got = np.stack(_rows(dg))
            assert got.shape == (plan.d, plan.size) and dg.launches == k + 1            # one launch, whatever the number of leaves
            assert bool((dg.block[:, plan.size:] == -7.0).all())                         # the padding of every row is not written
            leafwise = R.compose(plan, _leaf_kernel_rows(plan, 99, stream, draw))
            restated = R.sample_plan(plan, 99, draw, stream)
            for what, want in (("per-leaf kernels", leafwise), ("restatement", restated)):
                assert np.array_equal(got[exact].view(np.uint32), want[exact].astype(np.float32).view(np.uint32)), (name, what, draw, stream)
                err = np.abs(got - want) / scale
                print(f"{name} stream {stream} draw {draw} vs {what}: max |got - want| / scale = {err.max():.3g} (bound 4e-6)")
                assert err.max() <= 4e-6, (name, what, draw, stream, err.max())
            bit_equal &= np.array_equal(got.view(np.uint32), leafwise.astype(np.float32).view(np.uint32))
    print(f"{name}: jittered rows bit-equal to the per-leaf kernels: {bit_equal}")


@pytest.mark.gpu
def test_data_leaves_and_exact_grids_are_the_host_generators_numbers():
    torch.manual_seed(1)
    st = StaticGenerator(Generator2D((6, 5), (0, -1), (1, 1)))
    dg = DeviceGenerator(st)
    for _ in range(2):
        got = [v.reshape(-1).cpu() for v in dg.get_examples()]
        assert len(got) == 2 and all(torch.equal(a, b.detach()) for a, b in zip(got, st.get_examples()))
    g = Generator2D((8, 8), (0, 0), (1, 2), "equally-spaced") + PredefinedGenerator(torch.rand(13), torch.rand(13) * 2)
    dg = DeviceGenerator(g, seed=3)
    got = [v.reshape(-1).cpu() for v in dg.get_examples()]
    assert dg.size == 77 and all(torch.equal(a, b.detach()) for a, b in zip(got, g.get_examples())) and dg.launches == 1


@pytest.mark.gpu
def test_plan_draws_are_reproducible_from_seed_draw_and_stream():
    make = PLAN_CASES["eight-leaves"][0]
    plan = G.plan_spec(make())
    jittered = ~R.compose(plan, [np.stack([np.full(f.size, e) for e in R.leaf_exact_rows(f)]) for f in plan.leaves]).astype(bool)
    base = np.stack(_rows(DeviceGenerator(make(), seed=5, stream_id=1)))
    dg = DeviceGenerator(make(), seed=5, stream_id=1)
    again, nxt = np.stack(_rows(dg)), np.stack(_rows(dg))
    other_stream = np.stack(_rows(DeviceGenerator(make(), seed=5, stream_id=2)))
    assert np.array_equal(base, again) and dg.launches == 2 == dg.draw and jittered.sum() > 20
    for other in (nxt, other_stream):
        assert (base[jittered] != other[jittered]).mean() > 0.9
        assert np.array_equal(base[~jittered], other[~jittered])
    with pytest.raises(ValueError, match="prefetch"):
        DeviceGenerator(make(), prefetch=True)            # the epoch tail's prefetch speaks ndq_sampler_desc only
    with pytest.raises(ValueError, match="latin-hypercube"):
        DeviceGenerator(Generator1D(8) + Generator1D(8, method="latin-hypercube"))


@pytest.mark.gpu
def test_invalid_plan_descriptors_launch_nothing():
    block, table = torch.full((6, 128), -7.0, device="cuda"), torch.zeros(2048, device="cuda")
    _assert_all_refused(block.data_ptr(), table.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert bool((block == -7.0).all())


@pytest.mark.gpu
def test_plan_draws_in_double_are_the_exact_images_of_the_fp32_draws():
    make = PLAN_CASES["concat-of-all"][0]
    a = DeviceGenerator(make(), seed=4)
    b = DeviceGenerator(make(), seed=4, dtype=torch.float64)
    for _ in range(2):
        xa, xb = a.get_examples(), b.get_examples()
        assert all(y.dtype == torch.float64 and y.shape == (40, 1) and torch.equal(x.double(), y) for x, y in zip(xa, xb))


class _Replay(BaseGenerator):
    """Serves prepared host batches in order."""

    def __init__(self, batches):
        super().__init__()
        self.batches, self.k, self.size = batches, 0, batches[0].shape[1]

    def get_examples(self):
        self.k += 1
        return tuple(torch.from_numpy(row.copy()) for row in self.batches[self.k - 1])


def _laplace_solver(gen):
    from neurodiffeq_amd.solvers import Solver2D
    from tests import configs
    torch.manual_seed(0)
    cfg = configs.make("c2", 8)
    s = Solver2D(cfg["pde"], cfg["conds"], xy_min=(0, 0), xy_max=(1, 1), nets=cfg["nets"], train_generator=gen,
                 valid_generator=Generator2D((4, 4), method="equally-spaced"), n_batches_valid=0)
    s.fused = "require"
    return s


@pytest.mark.gpu
def test_solver_trains_on_plan_drawn_batches():
    """fit() on DeviceGenerator(interior + edge): every epoch's block is drawn in place by ONE plan launch and read in place by
    the closure kernel; the losses are those of a solver that is fed the restated batches from the host."""
    make = lambda: Generator2D((8, 8)) + Generator1D(16) * Generator1D(16)
    gen = DeviceGenerator(make(), seed=42)
    solver = _laplace_solver(gen)
    solver.fit(3, tqdm_file=None)
    assert solver.fused_active and gen.plan is not None and gen.draw == 3 and gen.launches == 3 and gen.size == 80
    assert solver._batch["train"] is gen._views and len(gen._views) == 2 and device_source(gen._views) is gen
    assert solver._fused_sys.resident_ptr(gen._views) == (gen.block.data_ptr(), gen.block.shape[1])
    plan = G.plan_spec(make())
    batches = [R.sample_plan(plan, 42, k) for k in range(3)]
    assert _close(_np(gen._views[1]), batches[2][1], 1.0)
    again = _laplace_solver(_Replay(batches))
    again.fit(3, tqdm_file=None)
    hist, want = solver.metrics_history["train_loss"], again.metrics_history["train_loss"]
    print(f"losses {hist} replayed {want} max rel {np.max(np.abs(np.array(hist) / np.array(want) - 1)):.3g}")
    assert again.fused_active and np.allclose(hist, want, rtol=2e-5), (hist, want)


@pytest.mark.gpu
def test_plan_route_switches_to_the_host_draw_when_the_tree_changes():
    """Any change anywhere in the tree -- a leaf's grid tensor replaced, a wrapper's `generators` tuple replaced -- cannot be
    followed by the uploaded tables: the wrapped generator's own host draw takes over (RuntimeWarning).  No change: no warning."""
    def host_from_now_on(dg, g, change):
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            first, second = _rows(dg), _rows(dg)
        assert not any("host draw" in str(m.message) for m in w)              # no change: no warning
        assert dg.launches == 2 and not dg._on_host and not np.array_equal(first, second)
        change()
        torch.manual_seed(7)
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            x = [v.clone() for v in dg.get_examples()]
        assert dg._on_host and any(issubclass(m.category, RuntimeWarning) and "host draw" in str(m.message) for m in w)
        y = [v.clone() for v in dg.get_examples()]
        torch.manual_seed(7)
        for have in (x, y):                             # from then on: the wrapped generator's own host draws
            want = g.get_examples()
            want = [want] if isinstance(want, torch.Tensor) else list(want)
            assert len(have) == len(want) and all(torch.equal(a.reshape(-1).cpu(), b.detach()) for a, b in zip(have, want))
        assert dg.launches == 2

    a, b = Generator1D(32, 0.0, 1.0, "equally-spaced-noisy"), Generator1D(32, 0.1, 2.0, "log-spaced-noisy")
    g = a * b
    host_from_now_on(DeviceGenerator(g, seed=3), g, lambda: setattr(a, "examples", torch.linspace(2.0, 3.0, 32)))
    a, b, c = Generator1D(20), Generator1D(12, method="equally-spaced-noisy"), Generator1D(12, 5.0, 6.0)
    g = a + b
    host_from_now_on(DeviceGenerator(g, seed=3), g, lambda: setattr(g, "generators", (a, c)))
    # an in-place edit of a DATA leaf's tensor is seen as well (version counter)
    pre = PredefinedGenerator(torch.rand(9))
    g = Generator1D(7) + pre
    dg = DeviceGenerator(g, seed=3)
    dg.get_examples()
    with torch.no_grad():
        pre.xs.mul_(2.0)
    with pytest.warns(RuntimeWarning, match="host draw"):
        got = dg.get_examples()[0].reshape(-1).cpu()
    assert dg._on_host and torch.equal(got[7:], pre.xs.detach())
