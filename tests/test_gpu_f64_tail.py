"""The fp64 sums + tail launch (csrc/ndq_api64.hip: reduce_tail64_kernel) and the solver route through it
(NDQ_F64_FUSED_TAIL=1: engine.fast_train_epoch_nets -> ndq64_fused_step_run) on the GPU.

Everything here is held to EQUAL BITS against the route the switch replaces -- ndq64_reduce_partials per network, the loss sum
(len = 1, scale = seed), ndq64_epoch_tail per network -- because summation orders are part of the contract (csrc/ndq_tail.h):
a training run must not depend on which route served an epoch.  The one comparison with a tolerance is the reference's own
float64 trajectory (tests/golden/c1_f64.npz), at the bound tests/test_gpu_f64_multi_closure.py puts on it."""
import ctypes
import os
import warnings

import numpy as np
import pytest
import torch

from neurodiffeq_amd import _lib
from oracle import autograd_ref as R
from tests import f64_multi_problems as FP
from tests import f64_tail_problems as TP

pytestmark = pytest.mark.gpu
TOL_GOLDEN = 1e-9
SWITCH = "NDQ_F64_FUSED_TAIL"

# ---------------------------------------------------------------------------------------------- the kernel alone
NPARTS = [1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1024]
PS = [1, 13, 63, 64, 65, 1153]
NETS = [1, 2, 4]


def _kernel_cases():
    """Every nparts twice (two different P each, so every P occurs at least three times), n_nets cycling through 1 / 2 / 4, and
    the variations -- Adam step 1 / 1 000, weight decay 0 / 0.01, snapshot buffer or none, a best loss that improves or not,
    both parities -- spread over the cases by the bits of the case number; then two networks of different P, and a NaN loss
    partial with either parity."""
    cases = []
    for i, nparts in enumerate(NPARTS):
        for j in (0, 1):
            c = 2 * i + j
            P = PS[(i + 3 * j + (i // 6)) % 6]
            cases.append(dict(nparts=nparts, Ps=[P] * NETS[c % 3], adam_step=1000 if c & 1 else 1, wd=0.01 if c & 2 else 0.0,
                              track=c % 5 != 4, improve=bool(c & 4) != bool(c & 1), parity=(c >> 3) & 1, nan=False))
    cases.append(dict(nparts=17, Ps=[13, 130], adam_step=1, wd=0.0, track=True, improve=True, parity=0, nan=False))
    cases.append(dict(nparts=257, Ps=[130, 13], adam_step=1000, wd=0.01, track=True, improve=False, parity=1, nan=False))
    cases.append(dict(nparts=65, Ps=[65], adam_step=1, wd=0.0, track=True, improve=True, parity=0, nan=True))
    cases.append(dict(nparts=256, Ps=[13, 13], adam_step=1000, wd=0.01, track=True, improve=True, parity=1, nan=True))
    return cases


KERNEL_CASES = _kernel_cases()


def _case_id(c):
    return (f"r{c['nparts']}-p{'x'.join(map(str, c['Ps']))}-t{c['adam_step']}-wd{c['wd']}-{'snap' if c['track'] else 'nosnap'}-"
            f"{'better' if c['improve'] else 'worse'}-par{c['parity']}{'-nan' if c['nan'] else ''}")


def test_the_thinned_product_keeps_every_size_and_variation():
    assert {c["nparts"] for c in KERNEL_CASES} == set(NPARTS) and len(KERNEL_CASES) <= 48
    assert {p for c in KERNEL_CASES for p in c["Ps"]} >= set(PS)
    assert {len(c["Ps"]) for c in KERNEL_CASES} == {1, 2, 4}
    for key, values in (("adam_step", {1, 1000}), ("wd", {0.0, 0.01}), ("track", {True, False}), ("improve", {True, False}),
                        ("parity", {0, 1}), ("nan", {True, False})):
        assert {c[key] for c in KERNEL_CASES} == values, key
    assert any(c["track"] and c["improve"] for c in KERNEL_CASES) and any(c["track"] and not c["improve"] for c in KERNEL_CASES)


def _state(c):
    """Inputs of one case on the device: per network partial rows, parameters, moments, gradient / snapshot buffers (filled with
    a sentinel), and the shared loss partials, history ring, best-loss pair, loss slot."""
    g = torch.Generator().manual_seed(1000 * c["nparts"] + sum(c["Ps"]))
    rnd = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float64)
    nets = []
    for P in c["Ps"]:
        nets.append(dict(part=rnd(c["nparts"], P), p=rnd(P), m=0.1 * rnd(P), v=0.01 * rnd(P) ** 2, grad=torch.full((P,), -7.0).double(),
                         best=torch.full((P,), -9.0).double()))
    lpart = rnd(c["nparts"]) ** 2
    if c["nan"]:
        lpart[c["nparts"] // 2] = float("nan")
    seed = 1.0 / (16.0 * c["nparts"])
    loss = float(lpart.sum() * seed)
    best = torch.full((2,), -5.0).double()
    best[c["parity"]] = 10.0 * loss if c["improve"] else 0.1 * loss
    if c["nan"]:
        best[c["parity"]] = 1.0
    shared = dict(lpart=lpart, hist=torch.full((8,), -3.0).double(), best_loss=best, slot=torch.full((4,), -2.0).double())
    dev = lambda d: {k: t.cuda() for k, t in d.items()}
    return [dev(n) for n in nets], dev(shared), seed


ADAM = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)
HIST_INDEX = 5


def _run_new(c, nets, sh, seed):
    arr = (_lib.FusedStep64 * len(nets))()
    for st, n in zip(arr, nets):
        st.n, st.ldc, st.ldj, st.blocks, st.n_params = 0, 0, 0, c["nparts"], n["p"].numel()
        st.seed = seed
        st.params, st.partials, st.loss_partials = n["p"].data_ptr(), n["part"].data_ptr(), sh["lpart"].data_ptr()
        st.grad, st.loss_slot, st.adam_m, st.adam_v = n["grad"].data_ptr(), sh["slot"].data_ptr(), n["m"].data_ptr(), n["v"].data_ptr()
        st.lr, st.beta1, st.beta2, st.eps, st.weight_decay = ADAM["lr"], ADAM["beta1"], ADAM["beta2"], ADAM["eps"], c["wd"]
        st.loss_hist, st.best_loss = sh["hist"].data_ptr(), sh["best_loss"].data_ptr()
        st.best_flat = n["best"].data_ptr() if c["track"] else None
    stream = torch.cuda.current_stream().cuda_stream
    rc = _lib.lib64().ndq64_reduce_tail(arr, len(nets), c["adam_step"], HIST_INDEX, c["parity"], ctypes.c_void_p(stream))
    assert rc == 0


def _run_parent(c, nets, sh, seed):
    L = _lib.lib64()
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for n in nets:
        assert L.ndq64_reduce_partials(vp(n["part"]), c["nparts"], n["p"].numel(), vp(n["grad"]), 0, 1.0, stream) == 0
    assert L.ndq64_reduce_partials(vp(sh["lpart"]), c["nparts"], 1, vp(sh["slot"]), 0, seed, stream) == 0
    for k, n in enumerate(nets):
        rc = L.ndq64_epoch_tail(vp(n["p"]), vp(n["grad"]), vp(n["m"]), vp(n["v"]), n["p"].numel(), ADAM["lr"], ADAM["beta1"],
                                ADAM["beta2"], ADAM["eps"], c["wd"], c["adam_step"], vp(sh["slot"]), 1, vp(sh["hist"]), HIST_INDEX,
                                vp(sh["best_loss"]), c["parity"], vp(n["best"]) if c["track"] else None, 1 if k == 0 else 0, stream)
        assert rc == 0


def _same(a, b):
    """torch.equal with NaN == NaN (a NaN loss must land in the history of both routes)."""
    return a.shape == b.shape and bool(torch.all((a == b) | (torch.isnan(a) & torch.isnan(b))))


@pytest.mark.parametrize("c", KERNEL_CASES, ids=_case_id)
def test_one_launch_leaves_what_the_parents_launches_leave(c):
    got, sh_got, seed = _state(c)
    want, sh_want, _ = _state(c)
    _run_new(c, got, sh_got, seed)
    _run_parent(c, want, sh_want, seed)
    torch.cuda.synchronize()
    start = _state(c)[0]
    for k, (a, b) in enumerate(zip(got, want)):
        for name in ("p", "m", "v", "grad", "best", "part"):
            assert torch.equal(a[name], b[name]), (k, name)
        # (what the case is meant to exercise did happen, on the parent's side)
        assert not torch.equal(b["p"], start[k]["p"])
        snapped = not bool(torch.all(b["best"] == -9.0))
        assert snapped == (c["track"] and c["improve"] and not c["nan"]), (k, snapped)
    for name in ("hist", "best_loss", "slot", "lpart"):
        assert _same(sh_got[name], sh_want[name]), (name, sh_got[name], sh_want[name])
    assert bool(torch.isnan(sh_want["hist"][HIST_INDEX])) == c["nan"]
    assert float(sh_want["hist"][(HIST_INDEX + 1) % 8]) == -3.0 and float(sh_want["slot"][1]) == -2.0


# ---------------------------------------------------------------------------------------------- the solver route
def _make_solver(name, n, **kw):
    """A solver of system ``name`` in double whose training generator serves the same ``n`` points every epoch."""
    from neurodiffeq_amd.generators import Generator1D, Generator2D
    from neurodiffeq_amd.solvers import Solver1D, Solver2D
    from tests import configs
    torch.manual_seed(0)
    if name == "c2":
        cfg = configs.make("c2", 8)
        nets, conds, eqs, d = [net.double() for net in cfg["nets"]], cfg["conds"], cfg["pde"], 2
    elif name == "ramp":
        nets, conds, eqs, d, _ = TP.ramp_system(kw.pop("state"))
    else:
        nets, conds, eqs, d, _ = FP.make(name)
    kw.setdefault("n_batches_valid", 0)
    if d == 1:
        gen = Generator1D(n, 0.0, 1.0)
        s = Solver1D(eqs, conds, t_min=0.0, t_max=1.0, nets=nets, train_generator=gen, valid_generator=Generator1D(n, 0.0, 1.0), **kw)
    else:
        gen = Generator2D((n, 1), (0, 0), (1, 1))
        s = Solver2D(eqs, conds, xy_min=(0, 0), xy_max=(1, 1), nets=nets, train_generator=gen,
                     valid_generator=Generator2D((n, 1), (0, 0), (1, 1)), **kw)
    cols = [c.reshape(-1, 1) for c in TP.batch(d, n, 300 + n)]
    s.generator["train"].get_examples = lambda: cols
    vcols = [c.reshape(-1, 1) for c in TP.batch(d, n, 700 + n)]
    s.generator["valid"].get_examples = lambda: vcols
    s.fused = "require"
    return s, nets


def _result(s, nets):
    torch.cuda.synchronize()
    fs = s._fused_sys
    return dict(hist=np.array(s.metrics_history["train_loss"]), valid=np.array(s.metrics_history["valid_loss"]),
                params=R.get_flat(nets).cpu().numpy(), moments=[(m.cpu().numpy().copy(), v.cpu().numpy().copy()) for _, m, v, _ in s.optimizer._bound],
                loss_buf=fs.loss_buf[:1].cpu().numpy().copy(), launches=fs.launches_per_step(), closure=fs.fusedk is not None,
                K=len(fs.flat), ready=fs.f64_tail_ready(), f64=fs.f64)


def _train(monkeypatch, switch, name, n, epochs=5, run=None, **kw):
    if switch:
        monkeypatch.setenv(SWITCH, "1")
    else:
        monkeypatch.delenv(SWITCH, raising=False)
    s, nets = _make_solver(name, n, **kw)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)       # a rejected closure must not pass on the pipeline
        if run is None:
            for _ in range(epochs):
                s.run_train_epoch()
        else:
            run(s)
    assert s.fused_active
    return s, _result(s, nets)


def _assert_same_run(a, b):
    assert a["hist"].dtype == np.float64 and len(a["hist"]) == len(b["hist"]) > 0
    assert np.array_equal(a["hist"], b["hist"]), (a["hist"], b["hist"])
    assert np.array_equal(a["valid"], b["valid"])
    assert np.array_equal(a["params"], b["params"])
    assert len(a["moments"]) == len(b["moments"]) == a["K"]
    for (ma, va), (mb, vb) in zip(a["moments"], b["moments"]):
        assert np.array_equal(ma, mb) and np.array_equal(va, vb)
    assert np.array_equal(a["loss_buf"], b["loss_buf"])


@pytest.mark.parametrize("name,n", [("c2", 17), ("c2", 1024), ("lv_tanh", 17), ("lv_tanh", 1040), ("uvp16", 17), ("uvp16", 1040),
                                    (FP.OVER_NAME, 17), (FP.OVER_NAME, 1040)])
def test_five_epochs_on_the_new_route_equal_the_parents(monkeypatch, name, n):
    _, new = _train(monkeypatch, True, name, n)
    _, old = _train(monkeypatch, False, name, n)
    assert new["f64"] and old["f64"] and new["closure"] and old["closure"]
    assert new["ready"] and not old["ready"]
    assert new["launches"] == 2 and old["launches"] == 2 + 2 * old["K"]
    assert old["K"] == {"c2": 1, "lv_tanh": 2, "uvp16": 3, FP.OVER_NAME: 4}[name]
    _assert_same_run(new, old)
    assert len(new["hist"]) == 5 and np.all(np.isfinite(new["hist"]))


def test_two_runs_of_the_new_route_are_equal(monkeypatch):
    _, a = _train(monkeypatch, True, "lv_tanh", 1040)
    _, b = _train(monkeypatch, True, "lv_tanh", 1040)
    assert a["ready"] and b["ready"]
    _assert_same_run(a, b)


def test_best_network_tracking_equals_the_parents(monkeypatch):
    """Solver1D.fit, 25 Adam epochs of C1 in double, no validation batches: the snapshot follows the training loss."""
    from tests import configs

    def run(switch):
        if switch:
            monkeypatch.setenv(SWITCH, "1")
        else:
            monkeypatch.delenv(SWITCH, raising=False)
        torch.manual_seed(0)
        s, cfg = configs.make_solver("c1", 64)
        for net in cfg["nets"]:
            net.double()
        s.fused = "require"
        torch.manual_seed(7)
        with warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)
            s.fit(25, tqdm_file=None)
        assert s.fused_active and s._fused_sys.f64 and s._fused_sys.fusedk is not None
        return s, cfg
    (a, ca), (b, cb) = run(True), run(False)
    assert a._fused_sys.launches_per_step() == 2 and b._fused_sys.launches_per_step() == 6
    for key in a.metrics_history:
        assert np.array_equal(np.array(a.metrics_history[key]), np.array(b.metrics_history[key])), key
    assert len(a.metrics_history["train_loss"]) == 25 and a.lowest_loss == b.lowest_loss
    best_a, best_b = R.get_flat(a.best_nets).cpu().numpy(), R.get_flat(b.best_nets).cpu().numpy()
    assert best_a.dtype == np.float64 and np.array_equal(best_a, best_b)
    assert np.array_equal(R.get_flat(ca["nets"]).cpu().numpy(), R.get_flat(cb["nets"]).cpu().numpy())
    # the snapshot is a network the run passed through, not its end
    assert not np.array_equal(best_a, R.get_flat(ca["nets"]).cpu().numpy())


def test_three_epochs_on_the_new_route_follow_the_reference(golden_dir, monkeypatch):
    """tests/test_gpu_f64_multi_closure.py::test_three_epochs_follow_the_reference_under_its_float64_defaults with the switch
    set: C1 at 64 points the way an unchanged reference script runs it, bound 1e-9.  The route computes the parent's bits, so
    the distance from the fixture is the closure's there: loss 1.39e-16, parameters 2.43e-17 (printed below)."""
    from tests import configs
    from neurodiffeq_amd.utils import set_tensor_type
    gold = np.load(os.path.join(golden_dir, "c1_f64.npz"))
    monkeypatch.setenv(SWITCH, "1")
    set_tensor_type(device="cpu", float_bits=64)          # (cpu default device: the host generator's numbers, bit for bit)
    try:
        torch.manual_seed(int(gold["seed"]))
        solver, cfg = configs.make_solver("c1", 64)
        assert np.array_equal(R.get_flat(cfg["nets"]).cpu().numpy(), gold["params0"])
        solver.fused = "require"
        torch.manual_seed(int(gold["seed"]) + 2)
        with warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)
            for _ in range(3):
                solver.run_train_epoch()
        fs = solver._fused_sys
        assert solver.fused_active and fs.f64 and fs.fusedk is not None and fs.f64_tail_ready() and fs.launches_per_step() == 2
        hist = np.array(solver.metrics_history["train_loss"])
        params = R.get_flat(cfg["nets"]).cpu().numpy()
        errs = dict(loss=float(np.max(np.abs(hist - gold["traj_loss"]) / np.abs(gold["traj_loss"]))),
                    params=float(np.linalg.norm(params - gold["traj_params"]) / np.linalg.norm(gold["traj_params"])))
    finally:
        set_tensor_type(device="cpu", float_bits=32)
    print("fused tail", errs)
    assert errs["loss"] < TOL_GOLDEN and errs["params"] < TOL_GOLDEN, errs


# ---------------------------------------------------------------------------------------------- routes that must not take it
@pytest.fixture
def native_calls(monkeypatch):
    """Counts the epochs that went through engine.fast_train_epoch_nets."""
    from neurodiffeq_amd.engine import FusedSystem
    calls = []
    inner = FusedSystem.fast_train_epoch_nets

    def counted(self, *args, **kw):
        calls.append(self)
        return inner(self, *args, **kw)
    monkeypatch.setattr(FusedSystem, "fast_train_epoch_nets", counted)
    return calls


def test_validation_epochs_keep_the_parents_sequence(monkeypatch, native_calls):
    def run(s):
        for _ in range(3):
            s.run_train_epoch()
            s.run_valid_epoch()
    _, new = _train(monkeypatch, True, "lv_tanh", 17, run=run, n_batches_valid=1)
    assert len(native_calls) == 3                         # the training epochs, and nothing else
    _, old = _train(monkeypatch, False, "lv_tanh", 17, run=run, n_batches_valid=1)
    assert len(native_calls) == 3 and len(new["valid"]) == 3
    _assert_same_run(new, old)


def test_two_batches_keep_the_parents_sequence(monkeypatch, native_calls):
    _, new = _train(monkeypatch, True, "lv_tanh", 17, epochs=3, n_batches_train=2)
    _, old = _train(monkeypatch, False, "lv_tanh", 17, epochs=3, n_batches_train=2)
    assert not native_calls and new["ready"]
    _assert_same_run(new, old)


def test_without_a_closure_kernel_nothing_changes(monkeypatch, native_calls):
    monkeypatch.setenv("NDQ_F64_CLOSURE", "0")
    _, new = _train(monkeypatch, True, "lv_tanh", 17, epochs=3)
    _, old = _train(monkeypatch, False, "lv_tanh", 17, epochs=3)
    assert not native_calls and not new["closure"] and not old["closure"] and not new["ready"]
    assert new["launches"] == old["launches"] > 6
    _assert_same_run(new, old)


def test_a_ramped_coefficient_keeps_the_parents_results(monkeypatch, native_calls):
    """A Python float inside the equations, changed by a callback between epochs.  fp32 systems turn it into a kernel argument
    (n_theta > 0); the fp64 engine has no scalar arguments (engine.trace_system: a changed value is a re-trace with the number
    baked in, and FusedSystem refuses n_theta > 0 in double), so ``f64_tail_ready``'s ``n_theta`` clause cannot be reached
    from a solver today: every system of this run has n_theta == 0 and is served by the new route -- with the parent's bits."""
    def run_with(state, systems):
        def run(s):
            def ramp(solver):
                state["a"] = TP.RAMP_VALUES[1]
                systems.append(solver._fused_sys)
            s.fit(max_epochs=4, callbacks=[ramp], tqdm_file=None)
            systems.append(s._fused_sys)
        return run
    sa, sb, sys_a, sys_b = {"a": TP.RAMP_VALUES[0]}, {"a": TP.RAMP_VALUES[0]}, [], []
    _, new = _train(monkeypatch, True, "ramp", 17, run=run_with(sa, sys_a), state=sa)
    assert len(native_calls) == 4
    _, old = _train(monkeypatch, False, "ramp", 17, run=run_with(sb, sys_b), state=sb)
    assert len(native_calls) == 4 and sa["a"] == sb["a"] == TP.RAMP_VALUES[1]
    assert len({id(x) for x in sys_a}) == len({id(x) for x in sys_b}) == 2          # the new value rebuilt the system
    for fs in sys_a + sys_b:
        assert fs.f64 and fs.n_theta == 0 and fs.fusedk is not None
        assert fs.launches_per_step() == (2 if fs.f64_tail_ready() else 6)
    assert all(fs.f64_tail_ready() for fs in sys_a) and not any(fs.f64_tail_ready() for fs in sys_b)
    _assert_same_run(new, old)
