"""Indexed plan route of the device sampler (csrc/ndq_sample.h: sample_plan_indexed_kernel, include/ndq.h:
ndq_sample_plan_indexed, generators.plan_spec / DeviceGenerator): ResampleGenerator and BatchGenerator at the root of a plan,
drawn on the MI355X in the plan's own single launch.  On the CPU: the normal form and its refusals, the numpy restatement
(tests/sampler_index_ref.py) -- the swap-or-not shuffle is a bijection and passes chi-square tests of uniformity, the window is
the reference's FIFO cache --, descriptor validation.  On the GPU: the kernel against the restatement, epoch coverage,
reproducibility, fp64 hand-out, live changes, a solver training on mini-batches, the un-indexed path unchanged."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

from tests import sampler_index_ref as X
from tests import sampler_plan_ref as R
from tests import test_sampler_plan as TP
from neurodiffeq_amd import _lib
from neurodiffeq_amd import generators as G
from neurodiffeq_amd.generators import (BatchGenerator, DeviceGenerator, Generator1D, Generator2D, GeneratorND,
                                        PredefinedGenerator, ResampleGenerator, device_source)

Resample, Batch = ResampleGenerator, BatchGenerator


def _np(t):
    return t.detach().cpu().numpy().reshape(-1)


def _index(p):
    return (p.index.mode, p.index.n, p.index.m, p.index.batch, p.size)


# ---------------------------------------------------------------------------------------------------------- host side
def test_plan_spec_accepts_resample_and_batch_at_the_root():
    torch.manual_seed(0)
    leaf = Generator1D(67, method="equally-spaced")
    a, b = Generator1D(5), Generator1D(6, 0.1, 2.0, "log-spaced-noisy")
    # a plain plan: exactly what it was
    p = G.plan_spec(a + b)
    assert p.index is None and p.size == 11 and len(p.wrappers) == 1
    # Resample[leaf]
    rs = Resample(leaf, size=40)
    p = G.plan_spec(rs)
    assert _index(p) == ("permute", 67, 40, 0, 40) and p.d == 1 and p.segments == [("leaf", 0, 1, 0, 67)]
    assert p.wrappers == [rs] and p.leaves[0].gen is leaf
    assert _index(G.plan_spec(Resample(leaf))) == ("permute", 67, 67, 0, 67)
    assert _index(G.plan_spec(Resample(leaf, size=100, replacement=True))) == ("replace", 67, 100, 0, 100)
    # Resample[a + b]
    cat = a + b
    rs = Resample(cat, size=9)
    p = G.plan_spec(rs)
    assert _index(p) == ("permute", 11, 9, 0, 9) and p.wrappers == [rs, cat]
    assert p.segments == [("leaf", 0, 1, 0, 5), ("leaf", 1, 1, 5, 6)] and [f.gen for f in p.leaves] == [a, b]
    # Batch[leaf]
    bt = Batch(Generator1D(10, method="uniform"), 7)
    p = G.plan_spec(bt)
    assert _index(p) == ("none", 10, 10, 7, 7) and p.wrappers == [bt]
    assert _index(G.plan_spec(Batch(Generator1D(10), 25))) == ("none", 10, 10, 25, 25)            # a batch larger than a draw
    # Batch[Resample[a ^ b]]
    mesh = Generator1D(64, method="equally-spaced") ^ Generator1D(5, method="equally-spaced")
    rs = Resample(mesh)
    bt = Batch(rs, 48)
    p = G.plan_spec(bt)
    assert _index(p) == ("permute", 320, 320, 48, 48) and p.d == 2 and p.wrappers == [bt, rs, mesh]
    assert p.segments == [("mesh", 0, 2, 0, 320)]
    assert _index(G.plan_spec(Batch(Resample(mesh, size=30, replacement=True), 25))) == ("replace", 320, 30, 25, 25)
    # the key of the index map: no leaf's
    assert G.plan_index_seed(77) == X.plan_index_seed(77) == (77 + 8 * 0x9E3779B97F4A7C15) % 2 ** 64
    assert G.plan_index_seed(2 ** 64 - 1) == (8 * 0x9E3779B97F4A7C15 - 1) % 2 ** 64
    assert G.plan_index_seed(5) not in {G.plan_leaf_seed(5, l) for l in range(G.PLAN_MAX_LEAVES)}


def test_plan_spec_refusals_of_resample_and_batch_name_the_node():
    a, b = Generator1D(8), Generator1D(8)
    nd_cut = GeneratorND((4, 4), (0.0, 0.0), (1.0, 1.0), ("equally-spaced",) * 2, cut=((None, -1), (None, None)))
    small = Resample(a)
    small.size = 0
    none = Batch(a, 2)
    none.size = 0
    refused = {
        "Resample[Batch]": (Resample(Batch(a, 2)), "BatchGenerator inside ResampleGenerator"),
        "Resample[Resample]": (Resample(Resample(a)), "ResampleGenerator inside ResampleGenerator"),
        "Batch[Batch]": (Batch(Batch(a, 4), 2), "BatchGenerator inside BatchGenerator"),
        "Batch[Resample[Batch]]": (Batch(Resample(Batch(a, 4)), 2), "BatchGenerator inside ResampleGenerator"),
        "Batch[Resample[Resample]]": (Batch(Resample(Resample(a)), 2), "ResampleGenerator inside ResampleGenerator"),
        "more points than the generator has, without replacement": (Resample(a, size=9), "ResampleGenerator.*not size = 9"),
        "... below a Batch": (Batch(Resample(a, size=9), 4), "ResampleGenerator.*not size = 9"),
        "size < 1": (small, "ResampleGenerator.*size 0"),
        "batch_size < 1": (none, "BatchGenerator.*batch size 0"),
        "generator.size is not the plan's": (Resample(nd_cut), "ResampleGenerator.*generator.size = 16"),
        # below the root: as before
        "Resample inside Concat": (Resample(a) + b, "ResampleGenerator"),
        "Batch inside Ensemble": (Batch(a, 8) * b, "BatchGenerator"),
        "Resample inside Mesh below a Batch": (Batch(Resample(a) ^ b, 4), "ResampleGenerator"),
        "Transform below a Resample": (Resample(G.TransformGenerator(a, transform=lambda x: x)), "TransformGenerator"),
        "latin-hypercube below a Batch": (Batch(Generator1D(8, method="latin-hypercube"), 4), "latin-hypercube"),
    }
    for what, (g, match) in refused.items():
        with pytest.raises(ValueError, match=match):
            G.plan_spec(g)
    # with replacement any size is a fixed size
    assert G.plan_spec(Resample(a, size=9, replacement=True)).size == 9


def test_the_shuffle_is_a_bijection_keyed_by_draw_seed_and_stream():
    for n in (1, 2, 3, 7, 64, 1000, 4099):
        assert X.rounds(n) == 2 * int(n - 1).bit_length() + 8 <= 70
        for k in range(3):
            j = X.index_map("permute", n, n, k, 1234)
            assert j.shape == (n,) and np.array_equal(np.sort(j), np.arange(n)), (n, k)
            # a resample of m <= n points reads the head of the same permutation
            m = (n + 1) // 2
            assert np.array_equal(X.index_map("permute", n, m, k, 1234), j[:m])
    assert (X.rounds(1), X.rounds(2), X.rounds(3), X.rounds(64), X.rounds(65), X.rounds(2 ** 31 - 1)) == (8, 10, 12, 20, 22, 70)
    base = X.index_map("permute", 64, 64, 0, 5, 0)
    assert np.array_equal(base, X.index_map("permute", 64, 64, 0, 5, 0))
    for other in (X.index_map("permute", 64, 64, 1, 5, 0), X.index_map("permute", 64, 64, 2 ** 32, 5, 0),
                  X.index_map("permute", 64, 64, 0, 6, 0), X.index_map("permute", 64, 64, 0, 5, 1)):
        assert not np.array_equal(base, other)
    # several draws at once: the rows of the one-draw form
    many = X.index_map("permute", 64, 64, [0, 1, 2 ** 32], 5)
    assert np.array_equal(many[0], base) and np.array_equal(many[2], X.index_map("permute", 64, 64, 2 ** 32, 5))


def _chi2(counts, expected):
    return float(((counts - expected) ** 2 / expected).sum())


def _bound(df):
    return df + 5.0 * np.sqrt(2.0 * df)


@pytest.mark.parametrize("n", [10, 100, 1000])
def test_the_shuffle_is_uniform_by_chi_square(n):
    """seed 77, draws 0..3999: where positions 0, n/2, n-1 land (df n - 1) and (j(1) - j(0)) mod n over its n - 1 possible values
    (df n - 2) are uniform -- chi-square below df + 5 sqrt(2 df), five standard deviations above its mean --, and a draw has one
    fixed point on average (a uniform permutation: mean 1, variance 1; 4 000 draws: sd 0.016)."""
    D = 4000
    J = X.index_map("permute", n, n, range(D), 77)
    assert J.shape == (D, n)
    for pos in (0, n // 2, n - 1):
        chi = _chi2(np.bincount(J[:, pos], minlength=n), D / n)
        print(f"n {n}: position {pos} chi2 {chi:.1f} (df {n - 1}, bound {_bound(n - 1):.1f})")
        assert chi < _bound(n - 1)
    diff = np.bincount((J[:, 1] - J[:, 0]) % n, minlength=n)
    assert diff[0] == 0
    chi = _chi2(diff[1:], D / (n - 1))
    print(f"n {n}: (j(1) - j(0)) mod n chi2 {chi:.1f} (df {n - 2}, bound {_bound(n - 2):.1f})")
    assert chi < _bound(n - 2)
    fixed = (J == np.arange(n)).sum() / D
    print(f"n {n}: fixed points per draw {fixed:.3f}")
    assert 0.9 < fixed < 1.1


def test_indices_with_replacement_are_uniform():
    n, m, D = 36, 50, 4000
    J = X.index_map("replace", n, m, range(D), 77)
    assert J.shape == (D, m) and J.min() >= 0 and J.max() < n
    chi = _chi2(np.bincount(J.reshape(-1), minlength=n), D * m / n)
    print(f"replace n {n} m {m}: chi2 {chi:.1f} (df {n - 1}, bound {_bound(n - 1):.1f})")
    assert chi < _bound(n - 1)
    assert not np.array_equal(J[0], J[1]) and len(set(J[0])) < m             # (50 draws from 36: repeats)
    for n in (1, 2, 7, 2 ** 31 - 1):
        j = X.index_map("replace", n, 9, 3, 1)
        assert j.min() >= 0 and j.max() < n


def test_the_window_is_the_fifo_cache_of_the_reference():
    m, bs = 10, 7                                       # tests/generator_specs.py "batch"
    pairs = []
    for t in range(10):
        k, r = X.window(t, bs, m, bs)
        pairs += list(zip(k, r))
    assert pairs == [(k, r) for k in range(7) for r in range(10)]
    # without a batch: inner draw t itself
    assert X.window(5, 0, 10, 10) == ([5] * 10, list(range(10)))
    # a batch larger than a draw spans three inner draws
    k, r = X.window(0, 25, 10, 25)
    assert k == [0] * 10 + [1] * 10 + [2] * 5 and r == list(range(10)) * 2 + list(range(5))
    k, r = X.window(1, 25, 10, 25)
    assert k == [2] * 5 + [3] * 10 + [4] * 10 and r == list(range(5, 10)) + list(range(10)) * 2
    # the launcher's form (k0 / r0 in 64 bits, 32-bit arithmetic per point) is the same map
    for bs, m, size in ((7, 10, 7), (25, 10, 25), (257, 300, 257), (48, 320, 48), (65536, 65536, 65536), (1, 1, 1), (3, 1, 3)):
        for t in (0, 1, 2, 5, 6, 2 ** 31, 2 ** 32 + 1, 2 ** 40 - 1, 2 ** 40):
            assert X.window_k0r0(t, bs, m, size) == X.window(t, bs, m, size), (bs, m, t)
    assert X.window_k0r0(2 ** 40, 0, 10, 10) == X.window(2 ** 40, 0, 10, 10)
    # the host generators do just that: a BatchGenerator over a static grid serves the concatenated stream
    torch.manual_seed(0)
    g = Generator1D(10, method="equally-spaced")
    host = Batch(g, 7)
    nodes = _np(g.examples)
    for t in range(4):
        k, r = X.window(t, 7, 10, 7)
        assert np.array_equal(_np(host.get_examples()), nodes[r])


# ------------------------------------------------------------------------------------------------- descriptor validation
def _ix(mode, m, batch=0):
    d = _lib.PlanIndexDesc()
    d.mode, d.m, d.batch = mode, m, batch
    return d


def _invalid_indexed(ptr):
    """(plan descriptor, index descriptor, ldc); the valid plan of tests/test_sampler_plan.py has n = 16 points."""
    NONE, PERMUTE, REPLACE = _lib.NDQ_INDEX_NONE, _lib.NDQ_INDEX_PERMUTE, _lib.NDQ_INDEX_REPLACE
    bad_plan = TP._valid(ptr)
    bad_plan.d = 0
    return {
        "m = 0, PERMUTE": (TP._valid(ptr), _ix(PERMUTE, 0), 64),
        "m = 0, REPLACE": (TP._valid(ptr), _ix(REPLACE, 0), 64),
        "m = -1": (TP._valid(ptr), _ix(REPLACE, -1), 64),
        "m > n under PERMUTE": (TP._valid(ptr), _ix(PERMUTE, 17), 64),
        "m > n under PERMUTE below a batch": (TP._valid(ptr), _ix(PERMUTE, 17, 4), 64),
        "m < n under NONE": (TP._valid(ptr), _ix(NONE, 15), 64),
        "m > n under NONE": (TP._valid(ptr), _ix(NONE, 17), 64),
        "batch < 0": (TP._valid(ptr), _ix(PERMUTE, 16, -1), 64),
        "unknown mode 3": (TP._valid(ptr), _ix(3, 16), 64),
        "unknown mode -1": (TP._valid(ptr), _ix(-1, 16), 64),
        "ldc < m": (TP._valid(ptr), _ix(PERMUTE, 16), 15),
        "ldc < m under REPLACE": (TP._valid(ptr), _ix(REPLACE, 40), 39),
        "ldc < batch": (TP._valid(ptr), _ix(NONE, 16, 32), 31),
        "a plan ndq_sample_plan refuses": (bad_plan, _ix(PERMUTE, 16), 64),
    }


def _assert_all_refused(coords_ptr, table_ptr, stream=None):
    L = _lib.lib()
    for what, (desc, ix, ldc) in _invalid_indexed(table_ptr).items():
        assert L.ndq_sample_plan_indexed(ctypes.byref(desc), ctypes.byref(ix), 1, 0, 0, coords_ptr, ldc, stream) == -2, what
    # ... and every plan descriptor ndq_sample_plan refuses, under a valid index
    for what, (desc, ldc) in TP._invalid_plans(table_ptr).items():
        if what == "ldc < total":                                       # (the block holds the OUTPUT points, 8 here)
            continue
        ix = _ix(_lib.NDQ_INDEX_REPLACE, 8)
        assert L.ndq_sample_plan_indexed(ctypes.byref(desc), ctypes.byref(ix), 1, 0, 0, coords_ptr, ldc, stream) == -2, what
    valid, ix = TP._valid(table_ptr), _ix(_lib.NDQ_INDEX_PERMUTE, 16)
    assert L.ndq_sample_plan_indexed(ctypes.byref(valid), None, 1, 0, 0, coords_ptr, 64, stream) == -2
    assert L.ndq_sample_plan_indexed(None, ctypes.byref(ix), 1, 0, 0, coords_ptr, 64, stream) == -2
    assert L.ndq_sample_plan_indexed(ctypes.byref(valid), ctypes.byref(ix), 1, 0, 0, None, 64, stream) == -2


def test_invalid_index_descriptors_are_refused_on_the_host():
    """Argument validation precedes any launch, so it is reachable without a GPU (the pointers are never followed)."""
    _assert_all_refused(0x2000, 0x1000)
    assert ctypes.sizeof(_lib.PlanIndexDesc) == 16                       # the layout of include/ndq.h
    assert (_lib.NDQ_INDEX_NONE, _lib.NDQ_INDEX_PERMUTE, _lib.NDQ_INDEX_REPLACE) == (0, 1, 2)


# ---------------------------------------------------------------------------------------------------- on the MI355X
def _rows(dg):
    return [_np(v).copy() for v in dg.get_examples()]


def _nd4():
    return GeneratorND((4, 3, 2, 2), (0.0,) * 4, (1.0,) * 4, ("equally-spaced",) * 4)


def _four_rows_of_nine():
    return PredefinedGenerator(*[np.linspace(0.05 * c, 1.0, 9).astype(np.float32) for c in range(4)])


# Every coordinate box is [0, 1] (scale 1 in the tolerance of tests/test_sampler_plan.py).  Sizes: 40 of 67 and 50 of 36 end inside
# a wave; 257 of 300 needs a second workgroup and straddles inner draws inside the first; 48 of 320 and 25 of 30 straddle inside a
# wave at draws 6 and 1; 25 of 10 spans three inner draws; n = 1: the 8-round shuffle of one point.
INDEX_CASES = {
    "resample-40-of-67": lambda: Resample(Generator1D(67, method="equally-spaced"), size=40),
    "replace-50-of-6x6": lambda: Resample(Generator2D((6, 6)), size=50, replacement=True),
    "batch-7-of-10": lambda: Batch(Generator1D(10, method="uniform"), 7),
    "batch-257-of-300": lambda: Batch(Generator1D(300, method="equally-spaced-noisy"), 257),
    "batch-48-resample-mesh-64x5": lambda: Batch(Resample(Generator1D(64, method="equally-spaced") ^ Generator1D(5, method="equally-spaced")), 48),
    "batch-25-resample-30-of-nd+predefined": lambda: Batch(Resample(_nd4() + _four_rows_of_nine(), size=30), 25),
    "batch-25-of-10": lambda: Batch(Generator1D(10, method="equally-spaced-noisy"), 25),
    "resample-1-of-1": lambda: Resample(Generator1D(1, method="uniform"), size=1),
    "batch-3-resample-1-of-1": lambda: Batch(Resample(Generator1D(1, method="equally-spaced-noisy")), 3),
    "batch-300-resample-700": lambda: Batch(Resample(Generator1D(700, method="equally-spaced-noisy")), 300),
}
DRAWS = (0, 1, 2, 5, 6, 2 ** 32 + 1)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(INDEX_CASES))
def test_indexed_kernel_matches_the_restatement(name):
    torch.manual_seed(123)
    g = INDEX_CASES[name]()
    plan = G.plan_spec(g)
    exact_rows = R.compose(plan, [np.stack([np.full(f.size, e) for e in R.leaf_exact_rows(f)]) for f in plan.leaves]).astype(bool)
    for stream in (0, 3):
        dg = DeviceGenerator(g, seed=99, stream_id=stream)
        assert dg.plan is not None and dg.size == plan.size == g.size and len(dg.blocks) == 1
        assert dg.block.shape == (plan.d, (plan.size + 63) // 64 * 64)
        for n_draw, draw in enumerate(DRAWS):
            dg.block.fill_(-7.0)
            dg.draw = draw
            got = np.stack(_rows(dg))
            assert got.shape == (plan.d, plan.size) and dg.launches == n_draw + 1         # one launch per draw
            assert bool((dg.block[:, plan.size:] == -7.0).all())                          # the padding is not written
            want = X.sample_plan_indexed(plan, 99, draw, stream)
            exact = X.gather_indexed(plan, 99, draw, stream, lambda k: exact_rows)
            assert np.array_equal(got[exact].view(np.uint32), want[exact].view(np.uint32)), (name, draw, stream)
            err = np.abs(got - want).max()
            print(f"{name} stream {stream} draw {draw}: exact entries {int(exact.sum())} of {exact.size}, max |got - want| = {err:.3g} (bound 4e-6)")
            assert err <= 4e-6, (name, draw, stream, err)


def _epoch_generator():
    return Batch(Resample(Generator1D(64, method="equally-spaced")), 16)


@pytest.mark.gpu
def test_four_batches_are_one_shuffled_epoch():
    torch.manual_seed(0)
    g = _epoch_generator()
    nodes = _np(g.generator.generator.examples)
    dg = DeviceGenerator(g, seed=11)
    epochs = []
    for e in range(3):
        epoch = np.concatenate([_rows(dg)[0] for _ in range(4)])
        assert epoch.shape == (64,) and np.array_equal(np.sort(epoch).view(np.uint32), nodes.view(np.uint32)), e
        assert not np.array_equal(epoch, nodes)                       # shuffled
        epochs.append(epoch)
    assert dg.draw == 12 == dg.launches
    assert not np.array_equal(epochs[0], epochs[1]) and not np.array_equal(epochs[1], epochs[2])
    # a batch that straddles two epochs holds the tail of one and the head of the next
    dg = DeviceGenerator(Batch(Resample(Generator1D(64, method="equally-spaced")), 24), seed=11)
    stream = np.concatenate([_rows(dg)[0] for _ in range(8)])
    assert np.array_equal(stream[:64], epochs[0]) and np.array_equal(stream[64:128], epochs[1]) and np.array_equal(stream[128:], epochs[2])


@pytest.mark.gpu
def test_indexed_draws_are_reproducible_from_seed_draw_and_stream():
    make = INDEX_CASES["batch-25-resample-30-of-nd+predefined"]
    torch.manual_seed(3)
    running = DeviceGenerator(make(), seed=5, stream_id=1)
    draws = [np.stack(_rows(running)) for _ in range(4)]
    torch.manual_seed(3)
    again = DeviceGenerator(make(), seed=5, stream_id=1)
    assert all(np.array_equal(np.stack(_rows(again)), d) for d in draws)
    for t in (3, 1):
        torch.manual_seed(3)
        fresh = DeviceGenerator(make(), seed=5, stream_id=1)
        fresh.draw = t
        assert np.array_equal(np.stack(_rows(fresh)), draws[t]) and fresh.launches == 1
    torch.manual_seed(3)
    other_stream = np.stack(_rows(DeviceGenerator(make(), seed=5, stream_id=2)))
    torch.manual_seed(3)
    other_seed = np.stack(_rows(DeviceGenerator(make(), seed=6, stream_id=1)))
    for other in (draws[1], other_stream, other_seed):
        assert not np.array_equal(draws[0], other)
    with pytest.raises(ValueError, match="prefetch"):
        DeviceGenerator(make(), prefetch=True)


@pytest.mark.gpu
def test_indexed_draws_in_double_are_the_exact_images_of_the_fp32_draws():
    make = INDEX_CASES["batch-257-of-300"]
    a = DeviceGenerator(make(), seed=4)
    b = DeviceGenerator(make(), seed=4, dtype=torch.float64)
    for _ in range(3):
        xa, xb = a.get_examples(), b.get_examples()
        assert all(y.dtype == torch.float64 and y.shape == (257, 1) and torch.equal(x.double(), y) for x, y in zip(xa, xb))


@pytest.mark.gpu
def test_invalid_index_descriptors_launch_nothing():
    block, table = torch.full((6, 128), -7.0, device="cuda"), torch.zeros(2048, device="cuda")
    _assert_all_refused(block.data_ptr(), table.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert bool((block == -7.0).all())


@pytest.mark.gpu
def test_indexed_route_switches_to_the_host_draw_when_a_size_changes():
    torch.manual_seed(0)
    for change in ("resample", "batch"):
        g = _epoch_generator()
        nodes = set(_np(g.generator.generator.examples).tolist())
        dg = DeviceGenerator(g, seed=3)
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            first, second = _rows(dg), _rows(dg)
        assert not any("host draw" in str(m.message) for m in w)              # no change: no warning
        assert dg.launches == 2 and not dg._on_host and not np.array_equal(first, second)
        if change == "resample":
            g.generator.size = 32
        else:
            g.size = 8
        with pytest.warns(RuntimeWarning, match="host draw"):
            got = dg.get_examples()
        size = 16 if change == "resample" else 8
        assert dg._on_host and dg.launches == 2 and len(got) == 1 and got[0].shape == (size, 1)
        assert set(_np(got[0]).tolist()) <= nodes and len(set(_np(got[0]).tolist())) == size


@pytest.mark.gpu
def test_solver_trains_on_device_drawn_mini_batches():
    """Solver1D on DeviceGenerator(BatchGenerator(ResampleGenerator(64-point grid), 16)): every epoch's 16 points are drawn in
    place by ONE indexed plan launch and read in place by the closure kernel; ten shuffled passes over the grid."""
    from neurodiffeq_amd import diff
    from neurodiffeq_amd.conditions import IVP
    from neurodiffeq_amd.solvers import Solver1D
    torch.manual_seed(0)
    gen = DeviceGenerator(_epoch_generator(), seed=42)
    solver = Solver1D(lambda u, t: [diff(u, t) + u], [IVP(0.0, 1.0)], t_min=0.0, t_max=1.0, train_generator=gen,
                      valid_generator=Generator1D(32, method="equally-spaced"), n_batches_valid=0)
    solver.fused = "require"
    epochs = 40
    solver.fit(epochs, tqdm_file=None)
    assert solver.fused_active and gen.plan.index is not None and gen.size == 16
    assert gen.launches == epochs == gen.draw and not gen._on_host
    assert solver._batch["train"] is gen._views and device_source(gen._views) is gen
    plan = G.plan_spec(_epoch_generator())
    assert np.array_equal(_np(gen._views[0]), X.sample_plan_indexed(plan, 42, epochs - 1)[0])
    hist = solver.metrics_history["train_loss"]
    print(f"train loss: first pass {np.mean(hist[:4]):.4g}, last pass {np.mean(hist[-4:]):.4g}")
    assert len(hist) == epochs and np.mean(hist[-4:]) < np.mean(hist[:4])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["concat-37-100-7", "six-rows"])
def test_the_identity_index_writes_what_the_plain_plan_draw_writes(name):
    torch.manual_seed(123)
    dg = DeviceGenerator(TP.PLAN_CASES[name][0](), seed=99, stream_id=3)
    L, n, ld = _lib.lib(), dg.size, dg.block.shape[1]
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for draw in (0, 2 ** 32 + 1):
        plain, indexed = torch.full_like(dg.block, -7.0), torch.full_like(dg.block, -7.0)
        assert L.ndq_sample_plan(ctypes.byref(dg.desc), 99, draw, 3, plain.data_ptr(), ld, stream) == 0
        ix = _ix(_lib.NDQ_INDEX_NONE, n)
        assert L.ndq_sample_plan_indexed(ctypes.byref(dg.desc), ctypes.byref(ix), 99, draw, 3, indexed.data_ptr(), ld, stream) == 0
        torch.cuda.synchronize()
        assert bool((plain[:, :n] != -7.0).all()) and torch.equal(plain.view(torch.int32), indexed.view(torch.int32))
