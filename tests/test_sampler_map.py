"""Map / filter route of the device sampler (generators.plan_spec `stages`, generators.trace_stages, codegen.SamplerMapProgram,
csrc/ndq_sample_map.h): TransformGenerator / FilterGenerator above a plan, drawn on the MI355X.  On the CPU: the normal form and its
refusals, the host build of ``ndq_map_point`` against the callables themselves in torch, the state watch, the restated compaction.
On the GPU: the kernels against the restatement (tests/sampler_map_ref.py) and against ``x[mask]`` of the unfiltered device draw,
launch / readback counts, reproducibility, fp64 hand-out, live changes, solvers that train on filtered / transformed batches."""
import ctypes
import itertools
import math
import warnings

import numpy as np
import pytest
import torch

from tests import sampler_map_cases as C
from tests import sampler_map_ref as M
from tests import sampler_plan_ref as R
from tests import test_sampler_plan as TP
from neurodiffeq_amd import _lib, codegen
from neurodiffeq_amd import generators as G
from neurodiffeq_amd.generators import (BatchGenerator, DeviceGenerator, FilterGenerator, Generator1D, Generator2D, ResampleGenerator,
                                        TransformGenerator, device_source)

Transform, Filter, Resample, Batch = TransformGenerator, FilterGenerator, ResampleGenerator, BatchGenerator


def _np(t):
    return t.detach().cpu().numpy().reshape(-1)


def _program(g):
    plan = G.plan_spec(g)
    return plan, codegen.SamplerMapProgram(*plan.trace, plan.d)


# ---------------------------------------------------------------------------------------------------------- host side
def test_plan_spec_accepts_stages_in_the_root_chain():
    torch.manual_seed(0)
    leaf = Generator2D((4, 5))
    # a plan without stages: exactly what it was
    p = G.plan_spec(leaf)
    assert p.stages == [] and p.d_out == p.d == 2 and p.wrappers == [] and p.trace is None and p.watch is None and not p.filtered
    bt = Batch(Resample(leaf), 7)
    p = G.plan_spec(bt)
    assert p.stages == [] and p.d_out == 2 and p.wrappers == [bt, bt.generator] and p.size == 7
    # one transform, rows 2 -> 2
    t = Transform(leaf, transform=C.polar)
    p = G.plan_spec(t)
    assert p.stages == [("map", C.polar)] and p.stage_nodes == [t] and (p.d, p.d_out, p.size) == (2, 2, 20)
    assert p.wrappers == [t] and p.index is None and not p.filtered and p.watch.complete and not p.watch.dirty()
    # rows may change: 1 -> 3, 3 -> 2, a tuple of one, a tensor
    assert G.plan_spec(Transform(Generator1D(9), transform=C.one_to_three)).d_out == 3
    assert G.plan_spec(Transform(C.nd3(), transform=C.three_to_two)).d_out == 2
    assert G.plan_spec(Transform(leaf, transform=lambda x, y: (x * y,))).d_out == 1
    assert G.plan_spec(Transform(leaf, transform=lambda x, y: x - y)).d_out == 1
    assert G.plan_spec(Transform(Generator1D(9), transform=lambda t: tuple(t * float(k) for k in range(1, 7)))).d_out == 6
    # column-wise, with None
    tl = Transform(leaf, transforms=[None, torch.exp])
    p = G.plan_spec(tl)
    assert p.stages == [("map", tl.trans)] and p.d_out == 2
    # above and between Batch / Resample; nested transforms compose in nesting order (inner first)
    rs = Resample(leaf, size=12)
    above, between = Transform(Batch(rs, 5), transform=C.affine2), Batch(Transform(rs, transform=C.affine2), 5)
    pa, pb = G.plan_spec(above), G.plan_spec(between)
    for p in (pa, pb):
        assert p.stages == [("map", C.affine2)] and (p.index.mode, p.index.n, p.index.m, p.index.batch, p.size) == ("permute", 20, 12, 5, 5)
    assert pa.wrappers == [above, above.generator, rs] and pb.wrappers == [between, between.generator, rs]
    inner = Transform(leaf, transform=C.affine2)
    outer = Transform(inner, transform=C.rotate)
    p = G.plan_spec(outer)
    assert p.stages == [("map", C.affine2), ("map", C.rotate)] and p.stage_nodes == [inner, outer] and p.wrappers == [outer, inner]
    # a filter above every Batch / Resample, stages above it
    disk = C.Disk(0.9)
    f = Filter(Batch(rs, 5), disk)
    top = Transform(Filter(Transform(f, transform=C.centred), C.disk_small), transform=C.rotate)
    p = G.plan_spec(top)
    assert p.stages == [("filter", disk), ("map", C.centred), ("filter", C.disk_small), ("map", C.rotate)]
    assert p.filtered and p.d_out == 2 and p.size == 5 and p.trace[2] is not None and len(p.wrappers) == 6
    assert G.plan_spec(f).filtered and G.plan_spec(f).d_out == 2


def test_stage_refusals_name_the_node():
    torch.manual_seed(0)
    a, b, g2 = Generator1D(8), Generator1D(8), Generator2D((4, 4))
    wrong = Filter(g2, C.Disk(0.9), size=9)
    keeps = Filter(g2, C.Disk(0.9), update_size=False)
    it = iter(range(100))
    refused = {
        "Transform inside Concat": (a + Transform(b, transform=lambda x: x), "TransformGenerator inside ConcatGenerator"),
        "Filter inside Ensemble": (a * Filter(b, C.above_half), "FilterGenerator inside EnsembleGenerator"),
        "Transform inside Mesh": (a ^ Transform(b, transform=lambda x: x), "TransformGenerator inside MeshGenerator"),
        "Filter below Resample": (Resample(Filter(g2, C.Disk(0.9))), "FilterGenerator below ResampleGenerator"),
        "Filter below Batch": (Batch(Filter(g2, C.Disk(0.9)), 4), "FilterGenerator below BatchGenerator"),
        "seven rows": (Transform(a, transform=lambda t: tuple(t + float(k) for k in range(7))), "TransformGenerator.*7 rows"),
        "size disagrees": (wrong, "FilterGenerator.*size = 9.*16 points"),
        "update_size=False": (keeps, "FilterGenerator.*update_size=False"),
        # tracing fails closed
        "an untraceable operation": (Transform(a, transform=lambda t: torch.cumsum(t, 0)), "TransformGenerator.*cannot be traced.*cumsum"),
        "control flow on values": (Filter(a, lambda xs: xs[0] > 0.5 if xs[0].max() > 1 else xs[0] < 0.5), "FilterGenerator.*cannot be traced"),
        "not a per-point column": (Transform(a, transform=lambda t: (t, 1.0)), "TransformGenerator.*per-point column.*float"),
        "a constant tensor": (Transform(a, transform=lambda t: (t, torch.zeros(8))), "TransformGenerator.*per-point column"),
        "batch size in arithmetic": (Transform(a, transform=lambda t: t / t.shape[0]), "TransformGenerator.*batch size"),
        "a map that returns a mask": (Transform(a, transform=lambda t: t > 0.5), "TransformGenerator.*boolean mask"),
        "a filter that returns a column": (Filter(a, lambda xs: xs[0] * 2.0), "FilterGenerator.*boolean mask"),
        "state that cannot be watched": (Filter(a, lambda xs: xs[0] > next(it) * 0.0), "cannot be watched"),
    }
    for what, (g, match) in refused.items():
        with pytest.raises(ValueError, match=match):
            G.plan_spec(g)


# the host build of ndq_map_point against the callable itself, in torch fp32, on 1 000 random rows
_ARITHMETIC = {
    "affine": (2, lambda x, y: (2.0 * x - 1.0, 0.5 * y + 0.25 * x), None),
    "box mask": (2, None, lambda xs: (xs[0] > 0.2) & (xs[1] < 0.7)),
    "disk mask": (2, None, lambda xs: xs[0] * xs[0] + xs[1] * xs[1] < 0.81),
    "where": (2, lambda x, y: (torch.where(x > y, x - y, y / (x + 2.0)), x * y), None),
}
_TRANSCENDENTAL = {
    "polar": (2, lambda r, th: (r * torch.cos(6.2831853 * th), r * torch.sin(6.2831853 * th))),
    "log-time": (1, lambda t: torch.exp(3.0 * t - 1.0)),
    "normalise": (2, lambda x, y: (torch.log(x + 1.5), torch.sqrt(x * x + y * y + 0.1))),
}


def _random_rows(d, n=1000):
    return np.random.default_rng(7).uniform(-1.0, 1.0, size=(d, n)).astype(np.float32)


def _host_build_vs_torch(d, transform, filter_fn):
    g = Generator1D(16) if d == 1 else Generator2D((4, 4))
    stages = []
    if transform is not None:
        g = Transform(g, transform=transform)
        stages.append(("map", transform))
    if filter_fn is not None:
        g = Filter(g, filter_fn)
        stages.append(("filter", filter_fn))
    plan, prog = _program(g)
    rows = _random_rows(d)
    got, keep = codegen.run_sampler_map_cpu(prog, rows)
    want, mask = C.apply_stages(rows, stages)
    return got, keep, want, mask, plan


@pytest.mark.parametrize("name", list(_ARITHMETIC))
def test_host_build_of_arithmetic_stages_is_torch_bit_for_bit(name):
    got, keep, want, mask, plan = _host_build_vs_torch(*_ARITHMETIC[name])
    assert 0 < mask.sum() and np.array_equal(keep, mask)
    assert np.array_equal(got[:, keep].view(np.uint32), want.view(np.uint32))
    # ... and so is the numpy restatement of the DAG
    out, k = M.eval_stages(plan.trace, _random_rows(plan.d))
    assert np.array_equal(k, mask) and np.array_equal(out[:, k].view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("name", list(_TRANSCENDENTAL))
def test_host_build_of_transcendental_stages_matches_torch(name):
    d, f = _TRANSCENDENTAL[name]
    got, keep, want, mask, plan = _host_build_vs_torch(d, f, None)
    assert keep.all() and mask.all()
    rel = float((np.abs(got.astype(np.float64) - want) / np.maximum(np.abs(want.astype(np.float64)), 1e-30)).max())
    print(f"{name}: worst relative error of the host build against torch fp32 over 1 000 rows = {rel:.3g}")
    # measured (worst of the three cases, libm's sinf / cosf / expf / logf / sqrtf against torch's vectorised ones): 1.45e-7 -- about
    # one fp32 ulp; bound = twice that, rounded up to one significant digit
    assert rel <= 3e-7, (name, rel)


def test_the_state_watch_sees_a_captured_number_move():
    disk = C.Disk(0.9)
    plan = G.plan_spec(Filter(Generator2D((4, 4)), disk))
    assert plan.watch.complete and not plan.watch.dirty()
    disk.radius = 0.5
    assert plan.watch.dirty()
    disk.radius = 0.9
    assert not plan.watch.dirty()
    scale = {"a": 2.0}
    plan = G.plan_spec(Transform(Generator1D(8), transform=lambda t: scale["a"] * t))
    assert not plan.watch.dirty()
    scale["a"] = 3.0
    assert plan.watch.dirty()
    it = itertools.count()
    with pytest.raises(ValueError, match="cannot be watched"):
        G.plan_spec(Transform(Generator1D(8), transform=lambda t: t + float(next(it))))


@pytest.mark.parametrize("blocks", [1, 2, 256, 257])
def test_the_restated_compaction_is_plain_masking(blocks):
    rng = np.random.default_rng(blocks)
    for n in (blocks * 256, blocks * 256 - 37 if blocks > 1 else 1):
        rows = rng.standard_normal((2, n)).astype(np.float32)
        for keep in (rng.random(n) < 0.5, np.ones(n, bool), np.zeros(n, bool), rng.random(n) < 0.01):
            out, kept = M.compact(rows, keep)
            assert kept == keep.sum() and np.array_equal(out, rows[:, keep])


def test_invalid_map_arguments_are_refused_on_the_host():
    """Argument validation precedes any launch, so it is reachable without a GPU (the pointers are never followed)."""
    _assert_map_refusals(0x2000, 0x1000, 0x3000)


def _assert_map_refusals(coords_ptr, table_ptr, work_ptr, stream=None):
    torch.manual_seed(0)
    # the valid plan of tests/test_sampler_plan.py: 16 points, two rows
    valid = TP._valid(table_ptr)
    assert valid.d == 2
    mp = codegen.load_sampler_map(_program(Transform(Generator2D((4, 4)), transform=C.affine2))[1])
    fl = codegen.load_sampler_map(_program(Filter(Generator2D((4, 4)), C.Disk(0.9)))[1])
    assert (mp.rows_in, mp.rows_out, mp.filters, fl.filters) == (2, 2, False, True)
    P = ctypes.byref

    def launch(k, desc, ix, ldc, rows, work, work_len, coords=coords_ptr):
        return k.launch(ctypes.cast(desc, ctypes.c_void_p) if desc is not None else None,
                        ctypes.cast(ix, ctypes.c_void_p) if ix is not None else None, 1, 0, 0, coords, ldc, rows, work, work_len, stream)
    for k in (mp, fl):
        w = (work_ptr, 2) if k.filters else (None, 0)
        assert launch(k, None, None, 64, 2, *w) == -2
        assert launch(k, P(valid), None, 64, 2, *w, coords=None) == -2
        assert launch(k, P(valid), None, 15, 2, *w) == -2                       # ldc < points
        assert launch(k, P(valid), None, 64, 1, *w) == -2                       # fewer rows than the stages hand out
        for what, (desc, ldc) in TP._invalid_plans(table_ptr).items():         # whatever ndq_sample_plan refuses
            assert launch(k, P(desc), None, ldc, 2, *w) == -2, what
        ix = _lib.PlanIndexDesc()
        ix.mode, ix.m, ix.batch = _lib.NDQ_INDEX_PERMUTE, 17, 0                  # m > n without replacement
        assert launch(k, P(valid), P(ix), 64, 2, *w) == -2
        ix.mode, ix.m = 7, 16
        assert launch(k, P(valid), P(ix), 64, 2, *w) == -2
    three = TP._valid(table_ptr)
    three.d = 3                                                                  # a plan of another row count than the trace's
    assert launch(mp, P(three), None, 64, 3, None, 0) == -2
    assert launch(fl, P(valid), None, 64, 2, None, 2) == -2                      # no work buffer
    assert launch(fl, P(valid), None, 64, 2, work_ptr, 1) == -2                  # work buffer without room for one workgroup's count
    assert launch(fl, P(valid), None, 64, 2, work_ptr, 0) == -2


# ---------------------------------------------------------------------------------------------------- on the MI355X
DRAWS = (0, 1, 2 ** 32 + 5)


def _rows(dg):
    return np.stack([_np(v).copy() for v in dg.get_examples()])


def _exact_rows(plan, seed, draw, stream):
    """[d][size] bool: entries of the plan's rows (before the stages) that carry no jitter."""
    from tests import sampler_index_ref as X
    per_leaf = [np.stack([np.full(f.size, e) for e in R.leaf_exact_rows(f)]) for f in plan.leaves]
    exact = R.compose(plan, per_leaf).astype(bool)
    return X.gather_indexed(plan, seed, draw, stream, lambda k: exact) if plan.index is not None else exact


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(C.MAP_CASES))
def test_map_kernel_matches_the_restatement(name):
    torch.manual_seed(123)
    g, base, stages = C.MAP_CASES[name]()
    plan = G.plan_spec(g)
    rows_block = max(plan.d, plan.d_out)
    for stream in (0, 3):
        dg = DeviceGenerator(g, seed=99, stream_id=stream)
        assert dg.plan is not None and dg.size == plan.size and len(dg.blocks) == 1 and not plan.filtered
        assert dg.block.shape == (rows_block, (plan.size + 63) // 64 * 64)
        for n_draw, draw in enumerate(DRAWS):
            dg.block.fill_(-7.0)
            dg.draw = draw
            views = dg.get_examples()
            got = np.stack([_np(v) for v in views])
            assert got.shape == (plan.d_out, plan.size) and dg.launches == n_draw + 1 and dg.readbacks == 0     # one launch per draw
            assert all(v.shape == (plan.size, 1) for v in views) and device_source(views) is dg
            assert bool((dg.block[:, plan.size:] == -7.0).all())                  # the padding is not written
            assert bool((dg.block[plan.d_out:] == -7.0).all())                    # nor the rows beyond d_out
            want = M.sample_plan_map(plan, 99, draw, stream)
            err = float(np.abs(got - want).max())
            if _exact_rows(plan, 99, draw, stream).all() and name != "polar-16x16-noisy":
                # exact leaves, + - * / and abs only: bit for bit
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, draw, stream)
            else:
                # polar over a jittered grid on [0, 1]^2: the leaves are within 4e-6 of the restatement (tests/test_sampler_plan.py);
                # (r, th) -> r cos(2 pi th), r sin(2 pi th) has |d/dr| <= 1 and |d/dth| <= 2 pi r, r <= 1 + jitter: a Lipschitz
                # factor 1 + 2 pi = 7.3, taken as 8 -- the rest (3e-6) covers the rounding of 2 pi th (half an ulp of 6.3 = 2.4e-7,
                # times r) and the ulp-level differences between the device's sinf / cosf and numpy's
                assert name == "polar-16x16-noisy" and err <= 8 * 4e-6, (name, draw, stream, err)
            print(f"{name} stream {stream} draw {draw}: max |got - want| = {err:.3g}")


@pytest.mark.gpu
def test_the_spellings_of_a_transform_around_batch_hand_out_the_same_numbers():
    torch.manual_seed(5)
    above = DeviceGenerator(C.MAP_CASES["above-batch-resample"]()[0], seed=7)
    between = DeviceGenerator(C.MAP_CASES["between-batch-and-resample"]()[0], seed=7)
    for _ in range(8):                                        # (48 of 320: draws 6 and 7 straddle two shuffled epochs)
        a, b = _rows(above), _rows(between)
        assert a.shape == (2, 48) and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # (a TransformGenerator BELOW a ResampleGenerator stays refused: tests/test_sampler_index.py pins that refusal)
    with pytest.raises(ValueError, match="TransformGenerator"):
        DeviceGenerator(Batch(Resample(Transform(C.mesh_64x5(), transform=C.affine2)), 48))


def _check_filtered(make, seed, stream, draws, near=None):
    """Filtered device draw == rows of the unfiltered device draw (a second DeviceGenerator, same seed / draw / stream) at the
    positions where the user's callables, run in torch on the CPU, keep the point -- in order."""
    torch.manual_seed(11)
    g, base, stages = make()
    plan = G.plan_spec(g)
    dg = DeviceGenerator(g, seed=seed, stream_id=stream)
    raw = DeviceGenerator(base, seed=seed, stream_id=stream)
    outer = [n for n in plan.stage_nodes if isinstance(n, FilterGenerator)][-1]
    assert plan.filtered and dg.size == plan.size == raw.size
    for n_draw, draw in enumerate(draws):
        dg.block.fill_(-7.0)
        dg.draw = raw.draw = draw
        views = dg.get_examples()
        got = np.stack([_np(v) for v in views])
        rows = _rows(raw)
        want, mask = C.apply_stages(rows, stages)
        assert dg.launches == 3 * (n_draw + 1) and dg.readbacks == n_draw + 1      # three launches and one readback per draw
        if near is not None:
            # decisions within 1e-5 (relative) of the threshold may go either way: compare with those points left out
            doubt = near(rows)
            assert doubt.mean() <= 0.005
            if doubt.any():
                sure_want = C.apply_stages(rows[:, ~doubt], stages)[0]
                kept_set = {tuple(c) for c in got.T.view(np.uint32).tolist()} - {tuple(c) for c in rows[:, doubt].T.view(np.uint32).tolist()}
                got_sure = np.stack([c for c in got.T if tuple(c.view(np.uint32).tolist()) in kept_set], axis=1)
                assert np.array_equal(got_sure.view(np.uint32), sure_want.view(np.uint32))
                continue
        kept = int(mask.sum())
        assert got.shape == (plan.d_out, kept), (got.shape, kept, draw)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (draw, stream)
        assert dg.size == kept == outer.size and all(v.shape == (kept, 1) for v in views)
        assert device_source(views) is dg and len(dg._source_ids) == 1
        assert bool((dg.block[:plan.d_out, kept:] == -7.0).all()) and bool((dg.block[plan.d_out:] == -7.0).all())
    return dg


@pytest.mark.gpu
@pytest.mark.parametrize("n", C.FILTER_SIZES)
def test_filter_kernels_keep_the_masked_rows_in_order(n):
    registry = len(G._DEVICE_SOURCES)
    for kind in ("all", "none", "grid"):
        dg = _check_filtered(lambda: C.filter_1d(kind, n), 99, 0, DRAWS)
        if kind == "all":
            assert dg.size == n
        elif kind == "none":
            assert dg.size == 0 and dg._views[0].shape == (0, 1)
        else:                                                 # the nodes are torch.linspace's own: the count is known exactly
            assert dg.size == int((torch.linspace(0.0, 1.0, n) > 0.5).sum())
        del dg
    import gc
    gc.collect()
    assert len(G._DEVICE_SOURCES) <= registry                 # the registry does not grow with the draws


def _near_the_circle(radius):
    def near(rows):
        q = rows[0].astype(np.float64) ** 2 + rows[1].astype(np.float64) ** 2
        return np.abs(q - radius * radius) <= 1e-5 * radius * radius
    return near


def test_few_uniform_points_lie_within_1e_5_of_the_circle():
    """The share of points the disk comparison may leave out (0.5 %) against what uniform points leave out: of the order 1e-5."""
    pts = np.random.default_rng(11).uniform(-1.0, 1.0, size=(2, 1_000_000)).astype(np.float32)
    share = float(_near_the_circle(0.9)(pts).mean())
    print(f"share of 1e6 uniform points within 1e-5 (relative) of r^2 = 0.81: {share:.3g}")
    assert share <= 1e-4


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(C.FILTER_CASES))
def test_filtered_draws_of_composed_stages(name):
    near = _near_the_circle(0.9) if name.startswith("disk") and "jittered" in name else None
    for stream in (0, 3):
        _check_filtered(C.FILTER_CASES[name], 99, stream, DRAWS, near)


@pytest.mark.gpu
def test_staged_draws_are_reproducible_and_exact_in_double():
    make = C.FILTER_CASES["transform-filter-transform"]
    torch.manual_seed(3)
    running = DeviceGenerator(make()[0], seed=5, stream_id=1)
    draws = [_rows(running) for _ in range(4)]
    for t in (3, 1):
        torch.manual_seed(3)
        fresh = DeviceGenerator(make()[0], seed=5, stream_id=1)
        fresh.draw = t
        assert np.array_equal(_rows(fresh), draws[t]) and fresh.launches == 3
    torch.manual_seed(3)
    other_stream, other_seed = _rows(DeviceGenerator(make()[0], seed=5, stream_id=2)), _rows(DeviceGenerator(make()[0], seed=6, stream_id=1))
    for other in (draws[1], other_stream, other_seed):
        assert other.shape != draws[0].shape or not np.array_equal(draws[0], other)
    with pytest.raises(ValueError, match="prefetch"):
        DeviceGenerator(make()[0], prefetch=True)
    for make in (C.FILTER_CASES["disk-32x32-jittered"], C.MAP_CASES["polar-16x16-noisy"]):
        torch.manual_seed(3)
        a = DeviceGenerator(make()[0], seed=4)
        b = DeviceGenerator(make()[0], seed=4, dtype=torch.float64)
        for _ in range(3):
            xa, xb = a.get_examples(), b.get_examples()
            assert all(y.dtype == torch.float64 and y.shape == x.shape and torch.equal(x.double(), y) for x, y in zip(xa, xb))
            assert a.size == b.size == xa[0].shape[0]


@pytest.mark.gpu
def test_changed_stages_are_followed_by_a_rebuild_then_by_the_host_draw():
    torch.manual_seed(0)
    disk = C.Disk(0.9)
    g = Filter(C.square(), disk)
    dg = DeviceGenerator(g, seed=3)
    raw = DeviceGenerator(g.generator, seed=3)

    def check(stages):
        raw.draw = dg.draw
        want = C.apply_stages(_rows(raw), stages)[0]
        got = _rows(dg)
        assert got.shape == want.shape and np.array_equal(got, want) and not dg._on_host
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        check([("filter", disk)])
        check([("filter", disk)])
        assert dg.launches == 6
        disk.radius = 0.5                                     # 1: a captured radius moves -- the watch is dirty, re-trace, rebuild
        check([("filter", disk)])
        g.filter_fn = C.disk_small                            # 2: another filter_fn
        check([("filter", C.disk_small)])
        disk.radius = 0.9
        g.filter_fn = disk                                    # 3: ... and back
        check([("filter", disk)])
        assert dg.launches == 15 and dg._rebuilds == 3
    assert not any("host draw" in str(m.message) for m in w)
    disk.radius = 0.5                                         # the fourth change: the wrapped generator's own host draw
    with pytest.warns(RuntimeWarning, match="host draw"):
        got = dg.get_examples()
    assert dg._on_host and dg.launches == 15 and len(got) == 2 and got[0].shape == (g.size, 1) == (dg.size, 1)
    assert bool((got[0] ** 2 + got[1] ** 2 < 0.25).all())
    # a transform: `trans` replaced
    t = Transform(Generator2D((16, 16)), transform=C.polar)
    dt = DeviceGenerator(t, seed=3)
    first = _rows(dt)
    t.trans = C.affine2
    dt.draw = 0
    raw = DeviceGenerator(t.generator, seed=3)
    assert np.array_equal(_rows(dt), C.apply_stages(_rows(raw), [("map", C.affine2)])[0]) and not dt._on_host and dt._rebuilds == 1
    assert not np.array_equal(first, _rows(dt))


@pytest.mark.gpu
def test_invalid_map_arguments_launch_nothing():
    block, table = torch.full((6, 128), -7.0, device="cuda"), torch.zeros(2048, device="cuda")
    work = torch.full((8,), -7, dtype=torch.int32, device="cuda")
    _assert_map_refusals(block.data_ptr(), table.data_ptr(), work.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert bool((block == -7.0).all()) and bool((work == -7).all())


def _laplace(u, x, y):
    from neurodiffeq_amd import diff
    return [diff(u, x, order=2) + diff(u, y, order=2) - u]


@pytest.mark.gpu
def test_solver_trains_on_a_device_filtered_disk():
    """Solver2D on DeviceGenerator(FilterGenerator(jittered 32 x 32 grid on [-1, 1]^2, disk)): every epoch's batch has another
    length; the closure kernel reads it in place, the batch size is a kernel argument -- no rebuild, no composite epoch."""
    from neurodiffeq_amd.conditions import NoCondition
    from neurodiffeq_amd.solvers import Solver2D
    torch.manual_seed(0)
    disk = C.Disk(0.9)
    g = Filter(C.square(), disk)
    gen = DeviceGenerator(g, seed=42)
    solver = Solver2D(_laplace, [NoCondition()], xy_min=(-1, -1), xy_max=(1, 1), train_generator=gen,
                      valid_generator=Generator2D((8, 8), (-1, -1), (1, 1), method="equally-spaced"), n_batches_valid=0)
    solver.fused = "require"
    epochs = 30
    sizes = []
    solver.fit(epochs, tqdm_file=None, callbacks=[lambda s: sizes.append(gen.size)])
    system = solver._fused_sys
    assert solver.fused_active and not gen._on_host and gen.draw == epochs
    assert gen.launches == 3 * epochs and gen.readbacks == epochs
    assert len(set(sizes)) > 5 and len(system._bufs) <= system.MAX_BUFFER_SETS           # the size changed, the buffer sets are capped
    assert solver._batch["train"] is gen._views and device_source(gen._views) is gen and len(gen._source_ids) == 1
    plan = G.plan_spec(Filter(C.square(), C.Disk(0.9)))
    want = M.sample_plan_map(plan, 42, epochs - 1)
    got = np.stack([_np(v) for v in gen._views])
    assert abs(got.shape[1] - want.shape[1]) <= 2 and g.size == gen.size == got.shape[1]
    if got.shape == want.shape:                                # (a point within an ulp of the circle may differ from numpy's jitter)
        assert np.abs(got - want).max() <= 4e-6
    hist = solver.metrics_history["train_loss"]
    print(f"disk: sizes {min(sizes)} .. {max(sizes)}, train loss first 5 {np.mean(hist[:5]):.4g}, last 5 {np.mean(hist[-5:]):.4g}")
    assert len(hist) == epochs and np.mean(hist[-5:]) < np.mean(hist[:5])


@pytest.mark.gpu
def test_solver_trains_on_a_device_transformed_polar_grid():
    from neurodiffeq_amd.conditions import NoCondition
    from neurodiffeq_amd.solvers import Solver2D
    torch.manual_seed(0)
    gen = DeviceGenerator(Transform(Generator2D((16, 16)), transform=C.polar), seed=42)
    solver = Solver2D(_laplace, [NoCondition()], xy_min=(-1, -1), xy_max=(1, 1), train_generator=gen,
                      valid_generator=Generator2D((8, 8), (-1, -1), (1, 1), method="equally-spaced"), n_batches_valid=0)
    solver.fused = "require"
    epochs = 20
    solver.fit(epochs, tqdm_file=None)
    assert solver.fused_active and not gen._on_host and gen.launches == epochs == gen.draw and gen.readbacks == 0
    assert solver._batch["train"] is gen._views and device_source(gen._views) is gen
    hist = solver.metrics_history["train_loss"]
    assert len(hist) == epochs and np.mean(hist[-5:]) < np.mean(hist[:5])
