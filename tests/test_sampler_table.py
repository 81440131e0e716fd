"""Table route of the device sampler (csrc/ndq_sample.h: sample_table_kernel, include/ndq.h: ndq_sample_table,
generators.table_spec / DeviceGenerator): GeneratorND and the node-table laws of Generator1D drawn on the MI355X.  On the
CPU: the host-side table mapping, the numpy restatement (tests/sampler_table_ref.py) against the pinned oracle and
against the host generators' distributions, descriptor validation.  On the GPU: the kernel against the restatement, the
exact laws, reproducibility, fp64 hand-out, solvers training on table-drawn batches, live changes."""
import ctypes
import warnings

import numpy as np
import pytest
import torch
from scipy import stats

from oracle import philox_ref as P
from tests import sampler_table_ref as T
from tests.sampler_table_problems import bundle_problem
from neurodiffeq_amd import _lib
from neurodiffeq_amd.generators import (BaseGenerator, DeviceGenerator, Generator1D, GeneratorND, device_source,
                                        table_spec)


def _np(t):
    return t.detach().cpu().numpy().reshape(-1)


def _mixed_nd(**kw):
    return GeneratorND((5, 4, 6, 3, 4), (0.0, 0.1, 0.0, -1.0, 2.0), (1.0, 2.0, 3.0, 1.0, 5.0),
                       ("equally-spaced", "log-spaced", "exp-spaced", "chebyshev2", "uniform"), base=(10, 10, 2, 10, 10),
                       cut=((None, None), (1, None), (None, -2), (None, None), (None, None)), **kw)


# ---------------------------------------------------------------------------------------------------------- host side
def test_table_spec_of_generator_nd():
    torch.manual_seed(0)
    g = _mixed_nd(abs_value=True)
    s = table_spec(g)
    assert (s.d, s.n, s.law, s.abs_value) == (5, [5, 3, 4, 3, 4], [T.NORMAL] * 5, True)
    assert g.size == 5 * 4 * 6 * 3 * 4 and len(g.grid_r[0]) == 5 * 3 * 4 * 3 * 4            # `cut` shortens the draw, not `size`
    # exact tables: the generator's own tensors, and through the ij-meshgrid its flattened grids
    idx = np.unravel_index(np.arange(int(np.prod(s.n))), s.n)
    for c in range(5):
        assert s.mean[c].dtype == np.float32 and s.std[c].dtype == np.float32
        assert np.array_equal(s.mean[c], _np(g.axis_r[c])) and np.array_equal(s.std[c], _np(g.axis_std[c]))
        assert np.array_equal(s.mean[c][idx[c]], _np(g.grid_r[c])) and np.array_equal(s.std[c][idx[c]], _np(g.grid_std[c]))
    assert np.array_equal(s.mean[1], torch.logspace(np.log10(0.1), np.log10(2.0), 4)[1:].numpy())
    assert not s.std[4].any() and s.std[0].all()                   # 'uniform' nodes are not jittered
    # noisy=False: exact nodes, no fold (the reference folds inside the noisy getter only); one axis given as numbers
    s = table_spec(_mixed_nd(noisy=False, abs_value=True))
    assert s.std == [None] * 5 and not s.abs_value
    s = table_spec(GeneratorND(7, 0.0, 1.0, "chebyshev", abs_value=True, r_noise_std=0.3))
    assert (s.d, s.n, s.abs_value) == (1, [7], True) and np.array_equal(s.std[0], np.full(7, 0.3, np.float32))
    assert table_spec(GeneratorND((2,) * 6, (0,) * 6, (1,) * 6, ("equally-spaced",) * 6)).d == 6
    with pytest.raises(ValueError):
        table_spec(GeneratorND((2,) * 7, (0,) * 7, (1,) * 7, ("equally-spaced",) * 7))


def test_table_spec_refuses_a_generator_nd_whose_grids_left_its_axis_tables():
    """The host getter draws from grid_r / grid_std, the tables come from the per-axis tensors: a generator whose grids were
    replaced or edited before it is wrapped would be drawn under another law on the device."""
    make = lambda **kw: GeneratorND((5, 4), (0.0, 0.1), (1.0, 2.0), ("equally-spaced", "log-spaced"), **kw)
    g = make()
    g.grid_std[0] = torch.full_like(g.grid_std[0], 0.5)
    with pytest.raises(ValueError, match="grid_std"):
        table_spec(g)
    g = make()
    with torch.no_grad():
        g.grid_r[1].mul_(2.0)
    with pytest.raises(ValueError, match="grid_r"):
        table_spec(g)
    g = make()
    del g.grid_r[1]
    with pytest.raises(ValueError, match="grid_r"):
        table_spec(g)
    g = make(noisy=False)                      # the exact getter never reads grid_std
    g.grid_std[0] = torch.full_like(g.grid_std[0], 0.5)
    assert table_spec(g).std == [None, None]
    # the equally spaced grids of Generator1D are the first sampler's (describe), not table laws
    for method in ("equally-spaced", "equally-spaced-noisy", "uniform"):
        with pytest.raises(ValueError):
            table_spec(Generator1D(8, method=method))


def test_table_spec_of_generator_1d_and_refusals():
    for method in ("log-spaced", "log-spaced-noisy", "chebyshev", "chebyshev1", "chebyshev2"):
        g = Generator1D(33, 0.1, 12.0, method)
        s = table_spec(g)
        assert (s.d, s.n, s.law, s.abs_value) == (1, [33], [T.NORMAL], False)
        assert np.array_equal(s.mean[0], _np(g.examples))
        if method.endswith("-noisy"):
            assert np.array_equal(s.std[0], np.full(33, g.noise_std, np.float32))
        else:
            assert s.std[0] is None
    s = table_spec(Generator1D(33, -1.0, 3.0, "chebyshev2-noisy"))
    assert (s.n, s.law, s.mean, s.std, s.lo, s.hi) == ([33], [T.CHEB2_NOISY], [None], [None], [-1.0], [3.0])
    for bad in (Generator1D(8, method="latin-hypercube"), Generator1D(8) + Generator1D(8),
                Generator1D(8) ^ Generator1D(8), Generator1D(8) * Generator1D(8)):
        with pytest.raises(ValueError):
            table_spec(bad)
    # DeviceGenerator.describe keeps speaking ndq_sampler_desc only
    with pytest.raises(ValueError):
        DeviceGenerator.describe(GeneratorND((4, 4)))


def test_restatement_equals_the_pinned_grid_oracle():
    """<= 3 'equally-spaced' axes: the same jitter as NDQ_SAMPLE_GRID under the same (seed, draw, stream), bit for bit."""
    g = GeneratorND((7, 5), (0.0, -1.0), (1.0, 2.0), ("equally-spaced", "equally-spaced"))
    std = [(1.0 / 7) / 4.0, (3.0 / 5) / 4.0]
    for draw, stream in ((0, 0), (2, 1), (2 ** 32 + 1, 3)):
        assert np.array_equal(T.sample_table(table_spec(g), 7, draw, stream), P.sample_grid((7, 5), (0.0, -1.0), (1.0, 2.0), std, 7, draw, stream))
    # block B: other words than block A's, the same on every call; untouched (and not computed) for d <= 3
    a, b = P.words(1000, 1, 0, 0), T.words_b(1000, 1, 0, 0)
    assert (a != b).mean() > 0.99 and np.array_equal(b, T.words_b(1000, 1, 0, 0))
    z3, z6 = T.normals(1000, 3, 1, 0), T.normals(1000, 6, 1, 0)
    assert all(np.array_equal(x, y) for x, y in zip(z3, z6)) and len(z6) == 6
    assert np.abs(np.corrcoef(np.stack(z6)) - np.eye(6)).max() < 0.12


def test_restated_table_distributions_match_the_host_generators():
    torch.manual_seed(0)
    # log-spaced GeneratorND (3 072 points): jitter / per-node width ~ N(0, 1) on every axis, and as the host generator draws it
    g = GeneratorND((64, 48), (0.1, 0.5), (10.0, 2.0), ("log-spaced", "log-spaced"))
    pts = T.sample_table(table_spec(g), seed=11, draw=0)
    host = g.get_examples()
    j = []
    for c in range(2):
        node, width = _np(g.grid_r[c]), _np(g.grid_std[c])
        j.append((pts[c] - node) / width)
        assert stats.kstest(j[c], "norm").pvalue > 1e-3
        assert stats.ks_2samp(j[c], (_np(host[c]) - node) / width).pvalue > 1e-3
    assert abs(np.corrcoef(j[0], j[1])[0, 1]) < 0.06
    g1 = Generator1D(4000, 0.1, 12.0, "log-spaced-noisy")
    node = _np(g1.examples)
    j1 = (T.sample_table(table_spec(g1), seed=5, draw=0)[0] - node) / np.float32(g1.noise_std)
    assert stats.kstest(j1, "norm").pvalue > 1e-3
    assert stats.ks_2samp(j1, (_np(g1.get_examples()) - node) / np.float32(g1.noise_std)).pvalue > 1e-3
    # 'chebyshev2-noisy' (two-sample only): the points, and the jitter in units of the node index
    g2 = Generator1D(4000, -1.0, 3.0, "chebyshev2-noisy")
    got, want = T.sample_table(table_spec(g2), seed=5, draw=0)[0], _np(g2.get_examples())
    assert got.min() >= -1.0 and got.max() <= 3.0 and stats.ks_2samp(got, want).pvalue > 1e-3
    jit = lambda x: (np.arccos(np.clip((2 * x.astype(np.float64) - 2.0) / 4.0, -1, 1)) / np.pi * 3999 - np.arange(4000))[5:-5]
    assert stats.ks_2samp(jit(got), jit(want)).pvalue > 1e-3


def _desc(d=1, n=(8,), law=None, mean=None, std=None, **kw):
    """A descriptor for the validation tests: the table pointers are never read by the host-side checks."""
    s = _lib.TableSamplerDesc()
    s.d = d
    for c in range(min(d, 6) if d > 0 else 0):
        s.n[c], s.law[c] = n[c % len(n)], (law[c % len(law)] if law else T.NORMAL)
        s.mean[c], s.std[c] = mean, std
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _invalid_descriptors(mean):
    big = _desc(3, (2048, 2048, 512), mean=mean)           # 2^31 points: one more than the cap
    return {"d = 0": (_desc(0), 64), "d = 7": (_desc(7, mean=mean), 64), "n = 0": (_desc(2, (8, 0), mean=mean), 64),
            "n < 0": (_desc(1, (-3,), mean=mean), 64), "more than 2^31 - 1 points": (big, 2 ** 31 - 1),
            "ldc < total": (_desc(2, (8, 9), mean=mean), 71),
            "NORMAL without a mean table": (_desc(2, (4, 4), mean=None), 64),
            "CHEB2_NOISY with d = 2": (_desc(2, (4, 4), law=(T.CHEB2_NOISY, T.NORMAL), mean=mean), 64),
            "CHEB2_NOISY on a later axis": (_desc(2, (4, 4), law=(T.NORMAL, T.CHEB2_NOISY), mean=mean), 64),
            "CHEB2_NOISY with n = 1": (_desc(1, (1,), law=(T.CHEB2_NOISY,), mean=mean), 64),
            "unknown law": (_desc(1, (8,), law=(2,), mean=mean), 64)}


def _assert_all_refused(coords_ptr, mean_ptr, stream=None):
    L = _lib.lib()
    for what, (desc, ldc) in _invalid_descriptors(mean_ptr).items():
        assert L.ndq_sample_table(ctypes.byref(desc), 1, 0, 0, coords_ptr, ldc, stream) == -2, what       # NDQ_EINVAL
    assert L.ndq_sample_table(None, 1, 0, 0, coords_ptr, 64, stream) == -2
    assert L.ndq_sample_table(ctypes.byref(_desc(mean=mean_ptr)), 1, 0, 0, None, 64, stream) == -2


def test_invalid_table_descriptors_are_refused_on_the_host():
    """Argument validation precedes any launch, so it is reachable without a GPU (the pointers are never followed)."""
    _assert_all_refused(0x2000, 0x1000)


# ---------------------------------------------------------------------------------------------------- on the MI355X
def _close(got, want, scale):
    return np.abs(got - want).max() <= 4e-6 * scale


def _rows(dg):
    return [_np(v).copy() for v in dg.get_examples()]


# name: (generator, scale per axis).  `scale` is what it is in tests/test_sampler.py: the magnitude of the axis' box.  The kernel's
# normals come from the fast log / sin / cos (absolute error of a normal: up to ~1e-5 at |z| ~ 5), the restatement's from libm,
# so a coordinate may differ by (jitter width) x 1e-5 plus its own rounding: every box below keeps the widths <= scale / 8
# (the axis of one node sits at 1.0 and the folded axis spans [-1, 1] for that reason: scale is the box's magnitude there too).
KERNEL_CASES = {
    "grid-7x5x3": (lambda: GeneratorND((7, 5, 3), (0.0, 0.1, -1.0), (1.0, 2.0, 1.0), ("equally-spaced", "log-spaced", "chebyshev1"),
                                       cut=((None, None), (1, -1), (None, None))), (1.0, 2.0, 1.0)),
    "six-axes": (lambda: GeneratorND((3, 2, 2, 3, 2, 2), (0.0, 0.5, 0.0, 1.0, 1.0, 0.5), (1.0, 2.0, 1.0, 3.0, 2.0, 2.0),
                                     ("equally-spaced", "log-spaced", "chebyshev2", "equally-spaced", "exp-spaced", "equally-spaced"),
                                     base=(10, 10, 10, 10, 2, 10)), (1.0, 2.0, 1.0, 3.0, 2.0, 2.0)),
    "1d-ragged": (lambda: GeneratorND(4099, -2.0, 3.0, "equally-spaced"), (5.0,)),
    "axis-of-one": (lambda: GeneratorND((5, 1, 4), (0.0, 1.0, 0.0), (1.0, 1.0, 2.0), ("equally-spaced",) * 3, r_noise_std=(0.05, 0.1, 0.05)),
                    (1.0, 1.0, 2.0)),
    "abs-around-zero": (lambda: GeneratorND((33, 9), (-1.0, -1.0), (1.0, 1.0), ("equally-spaced", "chebyshev"), abs_value=True,
                                            r_noise_std=(0.05, 0.1)), (1.0, 1.0)),
    "1d-log-noisy": (lambda: Generator1D(1000, 0.1, 12.0, "log-spaced-noisy"), (12.0,)),
    "1d-cheb2-noisy": (lambda: Generator1D(257, -1.0, 3.0, "chebyshev2-noisy"), (3.0,)),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(KERNEL_CASES))
def test_table_kernel_matches_the_restatement(name):
    torch.manual_seed(123)
    make, scale = KERNEL_CASES[name]
    g = make()
    dg = DeviceGenerator(g, seed=99, stream_id=3)
    assert dg.table is not None and len(dg.blocks) == 1
    spec = table_spec(g)
    for draw in (0, 1, 2, 2 ** 32 + 1):                   # the last one: the high word of the draw counter
        dg.draw = draw
        got, want = _rows(dg), T.sample_table(spec, 99, draw, 3)
        assert len(got) == len(want) == spec.d and got[0].shape == want[0].shape
        for c in range(spec.d):
            err = np.abs(got[c] - want[c]).max()
            print(f"{name} draw {draw} axis {c}: max|got - want| = {err:.3g} (bound {4e-6 * scale[c]:.3g})")
            assert _close(got[c], want[c], scale[c]), (name, draw, c, err)
    if name == "abs-around-zero":                         # the nodes straddle zero, the samples are folded
        assert spec.abs_value and spec.mean[0].min() < 0 and spec.mean[1].min() < 0 and min(r.min() for r in got) >= 0.0
    assert dg.launches == 4 and dg.draw == 2 ** 32 + 2


@pytest.mark.gpu
def test_exact_table_laws_are_the_host_generators_tensors():
    torch.manual_seed(1)
    nd = _mixed_nd(noisy=False, abs_value=True)
    got = [v.reshape(-1).cpu() for v in DeviceGenerator(nd).get_examples()]
    assert len(got) == 5 and all(torch.equal(a, b.detach()) for a, b in zip(got, nd.get_examples()))
    for method in ("log-spaced", "chebyshev2", "chebyshev"):
        g = Generator1D(1000, 0.1, 12.0, method)
        assert torch.equal(DeviceGenerator(g).get_examples()[0].reshape(-1).cpu(), g.get_examples().detach())
    # 'uniform' nodes of a noisy GeneratorND carry no jitter either
    g = GeneratorND((6, 5), (0.0, 0.0), (1.0, 2.0), ("uniform", "equally-spaced"))
    assert torch.equal(DeviceGenerator(g, seed=2).get_examples()[0].reshape(-1).cpu(), g.grid_r[0].detach())


@pytest.mark.gpu
def test_table_draws_are_reproducible_from_seed_draw_and_stream():
    make = KERNEL_CASES["six-axes"][0]
    torch.manual_seed(0)
    base = _rows(DeviceGenerator(make(), seed=5, stream_id=1))
    torch.manual_seed(0)
    dg = DeviceGenerator(make(), seed=5, stream_id=1)
    again, nxt = _rows(dg), _rows(dg)
    torch.manual_seed(0)
    other_stream = _rows(DeviceGenerator(make(), seed=5, stream_id=2))
    assert all(np.array_equal(a, b) for a, b in zip(base, again))
    for other in (nxt, other_stream):
        assert all((a != b).mean() > 0.9 for a, b in zip(base, other))
    with pytest.raises(ValueError):
        DeviceGenerator(make(), prefetch=True)            # the epoch tail's prefetch speaks ndq_sampler_desc only
    with pytest.raises(ValueError):
        DeviceGenerator(Generator1D(8, method="latin-hypercube"))


@pytest.mark.gpu
def test_invalid_table_descriptors_launch_nothing():
    block, table = torch.full((2, 128), -7.0, device="cuda"), torch.zeros(2048, device="cuda")
    _assert_all_refused(block.data_ptr(), table.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert bool((block == -7.0).all())


@pytest.mark.gpu
def test_table_draws_in_double_are_the_exact_images_of_the_fp32_draws():
    make = KERNEL_CASES["grid-7x5x3"][0]
    torch.manual_seed(0)
    a = DeviceGenerator(make(), seed=4)
    torch.manual_seed(0)
    b = DeviceGenerator(make(), seed=4, dtype=torch.float64)
    for _ in range(2):
        xa, xb = a.get_examples(), b.get_examples()
        assert all(y.dtype == torch.float64 and y.shape == (63, 1) and torch.equal(x.double(), y) for x, y in zip(xa, xb))


class _Replay(BaseGenerator):
    """Serves prepared host batches in order."""

    def __init__(self, batches):
        super().__init__()
        self.batches, self.k, self.size = batches, 0, batches[0].shape[1]

    def get_examples(self):
        self.k += 1
        return tuple(torch.from_numpy(row.copy()) for row in self.batches[self.k - 1])


def _bundle_solver(axes, wrap):
    from neurodiffeq_amd.solvers import BundleSolver1D
    torch.manual_seed(0)
    p = bundle_problem(axes)
    gen = wrap(p["gen"])
    valid = GeneratorND((4,) * axes, (0.1,) * axes, (1.0,) * axes, ("equally-spaced",) * axes, noisy=False)
    s = BundleSolver1D(p["ode"], p["conds"], nets=p["nets"], train_generator=gen, valid_generator=valid, n_batches_valid=0,
                       eq_param_index=p["eq_param_index"])
    s.fused = "require"
    return s, gen


@pytest.mark.gpu
@pytest.mark.parametrize("axes", [2, 4])
def test_solver_trains_on_table_drawn_batches(axes):
    """fit() on a DeviceGenerator(GeneratorND): every epoch's block is drawn in place by the table kernel and read in place by
    the closure kernel (four rows as well as two); the losses are those of a solver that is fed the restated batches."""
    solver, gen = _bundle_solver(axes, lambda g: DeviceGenerator(g, seed=42))
    solver.fit(3, tqdm_file=None)
    assert solver.fused_active and gen.table is not None and gen.draw == 3 and gen.launches == 3
    # the batch the solver trained on is the generator's own list of views: rows of ONE block the engine reads in place
    assert solver._batch["train"] is gen._views and len(gen._views) == axes and device_source(gen._views) is gen
    assert solver._fused_sys.resident_ptr(gen._views) == (gen.block.data_ptr(), gen.block.shape[1])
    spec = table_spec(bundle_problem(axes)["gen"])
    batches = [T.sample_table(spec, 42, k) for k in range(3)]
    assert _close(_np(gen._views[axes - 1]), batches[2][axes - 1], 2.0)
    again, _ = _bundle_solver(axes, lambda g: _Replay(batches))
    again.fit(3, tqdm_file=None)
    hist, want = solver.metrics_history["train_loss"], again.metrics_history["train_loss"]
    print(f"axes {axes}: losses {hist} replayed {want} max rel {np.max(np.abs(np.array(hist) / np.array(want) - 1)):.3g}")
    assert again.fused_active and np.allclose(hist, want, rtol=2e-5), (hist, want)


@pytest.mark.gpu
def test_table_route_follows_what_a_callback_changes_on_the_wrapped_generator():
    """The wrapped generator's tensors are read when IT draws: a replaced width tensor cannot be followed by the tables, so the
    wrapped generator's own host draw takes over (RuntimeWarning); a new noise_std number on a Generator1D rebuilds the table."""
    torch.manual_seed(0)
    g = GeneratorND((16, 8), (0.0, 0.1), (1.0, 2.0), ("equally-spaced", "log-spaced"))
    dg = DeviceGenerator(g, seed=3)
    first = _rows(dg)
    assert _close(first[0], T.sample_table(table_spec(g), 3, 0)[0], 1.0) and dg.launches == 1
    g.grid_std[0] = torch.full_like(g.grid_std[0], 0.5)                 # a callback after the first epoch
    torch.manual_seed(7)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        x = [v.clone() for v in dg.get_examples()]
    assert dg._on_host and any(issubclass(m.category, RuntimeWarning) and "host draw" in str(m.message) for m in w)
    y = [v.clone() for v in dg.get_examples()]
    torch.manual_seed(7)
    for have in (x, y):                                                 # from then on: the wrapped generator's host draws
        want = g.get_examples()
        assert all(torch.equal(a.reshape(-1).cpu(), b.detach()) for a, b in zip(have, want))
    assert dg.launches == 1 and dg.draw == 3 and float((x[0].reshape(-1).cpu() - g.grid_r[0].detach()).std()) > 0.3
    # an in-place edit of a node tensor is seen as well (version counter)
    g2 = GeneratorND((16, 8), (0.0, 0.1), (1.0, 2.0), ("equally-spaced", "log-spaced"))
    d2 = DeviceGenerator(g2, seed=3)
    d2.get_examples()
    with torch.no_grad():
        g2.grid_r[1].mul_(2.0)
    with pytest.warns(RuntimeWarning, match="host draw"):
        d2.get_examples()
    assert d2._on_host
    # Generator1D: a widened noise_std number -> a new width table, still on the device
    g1 = Generator1D(4096, 0.1, 12.0, "log-spaced-noisy")
    d1 = DeviceGenerator(g1, seed=3)
    node = g1.examples.detach()
    spread = lambda: float((d1.get_examples()[0].reshape(-1).cpu() - node).std())
    assert abs(spread() / g1.noise_std - 1.0) < 0.1
    g1.noise_std = 20.0 * g1.noise_std
    assert abs(spread() / g1.noise_std - 1.0) < 0.1 and not d1._on_host and d1.launches == 2
    assert _close(_np(d1._views[0]), T.sample_table(table_spec(g1), 3, 1)[0], 12.0)
