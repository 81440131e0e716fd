"""Inverse problems: the training epoch ends on the device.  The sums + tail launch of an epoch carries one more row that
reduces the scalars' block partials in ndq_reduce_partials' order and applies Adam to them (include/ndq.h: ndq_theta_step);
FusedAdam owns the scalars' moments, the system's device vector their values."""
import copy
import ctypes
import itertools
import os

import numpy as np
import pytest
import torch

from neurodiffeq_amd import _lib
from oracle import autograd_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
vp = ctypes.c_void_p


def _stream():
    return vp(torch.cuda.current_stream().cuda_stream)


@_lib.FUSED_LAUNCH_FN
def _no_closure(*_):
    """A closure launcher that launches nothing: the partial rows are the test's own."""
    return 0


class TailOnly:
    """ndq_fused_theta_multi_step_run around a one-parameter dummy network and the test's own theta_partials: the sums + tail
    launch alone."""

    def __init__(self, part, theta, m, v, frozen=0):
        blocks, nt = part.shape
        f = lambda *s: torch.zeros(*s, dtype=torch.float32, device=DEV)
        self.keep = dict(params=f(1), partials=f(blocks, 1), lparts=f(blocks), grad=f(2), m=f(1), v=f(1), hist=f(8),
                         best=torch.full((2,), float("inf"), device=DEV), coords=f(64), gtheta=f(nt))
        k = self.keep
        st = (_lib.FusedStep * 1)()
        s = st[0]
        s.n, s.ldc, s.ldj, s.blocks, s.n_params, s.seed = 1, 64, 64, blocks, 1, 1.0
        s.params, s.partials, s.loss_partials = k["params"].data_ptr(), k["partials"].data_ptr(), k["lparts"].data_ptr()
        s.grad, s.loss_slot = k["grad"].data_ptr(), k["grad"].data_ptr() + 4
        s.adam_m, s.adam_v, s.lr, s.beta1, s.beta2, s.eps = k["m"].data_ptr(), k["v"].data_ptr(), 1e-3, 0.9, 0.999, 1e-8
        s.loss_hist, s.best_loss = k["hist"].data_ptr(), k["best"].data_ptr()
        th = _lib.ThetaStep()
        th.n_theta, th.frozen = nt, frozen
        th.theta, th.partials, th.gtheta = theta.data_ptr(), part.data_ptr(), k["gtheta"].data_ptr()
        th.adam_m, th.adam_v = m.data_ptr(), v.data_ptr()
        self.st, self.th = st, th

    def set(self, j, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, step=1):
        th = self.th
        th.lr[j], (th.beta1[j], th.beta2[j]), th.eps[j], th.weight_decay[j], th.step[j] = lr, betas, eps, weight_decay, step

    def run(self):
        rc = _lib.lib().ndq_fused_theta_multi_step_run(self.st, 1, ctypes.cast(_no_closure, vp), ctypes.byref(self.th),
                                                       vp(self.keep["coords"].data_ptr()), 1, 0, 0, _stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        return self.keep["gtheta"]


def _reduce(part):
    out = torch.empty(part.shape[1], dtype=torch.float32, device=DEV)
    rc = _lib.lib().ndq_reduce_partials(vp(part.data_ptr()), part.shape[0], part.shape[1], vp(out.data_ptr()), 0, 1.0, _stream())
    assert rc == 0
    torch.cuda.synchronize()
    return out


# ---------------------------------------------------------------------------------------------- 1. sums
def test_sums_have_the_bits_of_reduce_partials():
    """gtheta of the new launch against ndq_reduce_partials on the same rows, bit for bit: every row count around the four
    interleaved chains, one and many workgroups' worth of closure rows, both sides of the LDS staging limit (2048 floats),
    and rows that cancel (+x, -x, tiny), where the order of the additions decides the result."""
    g = torch.Generator().manual_seed(0)
    shapes = list(itertools.product((1, 2, 16, 17, 64, 65, 257), (1, 2, 5))) + [(1024, 2), (1025, 2), (513, 5)]
    for blocks, nt in shapes:
        for kind in ("random", "cancel"):
            part = torch.randn(blocks, nt, generator=g)
            if kind == "cancel" and blocks >= 2:
                x = torch.randn(nt, generator=g) * 1e4
                part[0::3], part[1::3] = x, -x
                part[2::3] = 1e-4 * torch.randn(part[2::3].shape, generator=g)
                if blocks % 3 == 1:
                    part[-1] = 3e-5
            part = part.to(DEV)
            theta, m, v = (torch.zeros(nt, device=DEV) for _ in range(3))
            t = TailOnly(part, theta, m, v)
            for j in range(nt):
                t.set(j)
            got, want = t.run(), _reduce(part)
            assert torch.equal(got, want), (blocks, nt, kind, got, want)


# ---------------------------------------------------------------------------------------------- 2. Adam
GROUPS = {"one": [dict()] * 5,
          "two": [dict(), dict(), dict(lr=1e-2, betas=(0.8, 0.9), eps=1e-6), dict(lr=1e-2, betas=(0.8, 0.9), eps=1e-6), dict()],
          "decay": [dict(weight_decay=0.01)] * 5}


@pytest.mark.parametrize("step", [1, 2, 1000])
@pytest.mark.parametrize("groups", sorted(GROUPS))
def test_adam_has_the_bits_of_adam_step(groups, step):
    """Values and moments after the launch against ndq_adam_step on the same [NT] vectors, group by group; entry 1 is frozen:
    its value stays and its moment slots are not written."""
    g = torch.Generator().manual_seed(step)
    nt, blocks, frozen = 5, 3, 1
    part = torch.randn(blocks, nt, generator=g).to(DEV)
    theta0 = torch.randn(nt, generator=g).to(DEV)
    m0 = (0.1 * torch.randn(nt, generator=g)).to(DEV) if step > 1 else torch.zeros(nt, device=DEV)
    v0 = (0.01 * torch.rand(nt, generator=g)).to(DEV) if step > 1 else torch.zeros(nt, device=DEV)
    m0[frozen], v0[frozen] = 7.0, 9.0                    # sentinels
    theta, m, v = theta0.clone(), m0.clone(), v0.clone()
    t = TailOnly(part, theta, m, v, frozen=1 << frozen)
    full = [dict(dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0), **d) for d in GROUPS[groups]]
    for j, d in enumerate(full):
        if j != frozen:
            t.set(j, step=step, **d)
    gtheta = t.run()
    want_g = _reduce(part)
    assert torch.equal(gtheta, want_g)
    wt, wm, wv = theta0.clone(), m0.clone(), v0.clone()
    for j, d in enumerate(full):
        if j == frozen:
            continue
        rc = _lib.lib().ndq_adam_step(vp(wt[j:].data_ptr()), vp(want_g[j:].data_ptr()), vp(wm[j:].data_ptr()), vp(wv[j:].data_ptr()), 1,
                                      d["lr"], d["betas"][0], d["betas"][1], d["eps"], d["weight_decay"], step, _stream())
        assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(theta, wt) and torch.equal(m, wm) and torch.equal(v, wv), (theta, wt, m, wm, v, wv)
    assert theta[frozen] == theta0[frozen] and m[frozen] == 7.0 and v[frozen] == 9.0
    assert not torch.equal(theta, theta0)


# ---------------------------------------------------------------------------------------------- 3. one epoch, both routes
def _system(name, n):
    """(nets, conds, eqs, n_coords, scalars, batch) of a closure family's smallest system with trainable scalars."""
    from tests import configs, site_problems, theta_tail_problems, wide_multi_problems
    g = torch.Generator().manual_seed(7)
    if name in ("inv1", "inv2"):
        cfg = configs.make_inverse(name, size=n if name == "inv2" else None)
        if name == "inv1":
            batch = [2 * torch.rand(n, generator=g) - 1, torch.rand(n, generator=g)]
        else:
            batch = [torch.linspace(0.0, 1.0, n)]
        for col in cfg["data"]:                              # (a data column lives where the scalars it meets live)
            col.data = col.data.to(DEV)
        return cfg["nets"], cfg["conds"], cfg["pde"], len(batch), cfg["theta"], batch
    if name == "lvtheta":
        nets, conds, eqs, nc = wide_multi_problems.make("lvtheta", 128)
        return nets, conds, eqs, nc, eqs.theta, wide_multi_problems.batch("lvtheta", n, 7)
    if name == "heat-theta":
        nets, conds, eqs, nc = site_problems.make("heat-theta")
        return nets, conds, eqs, nc, eqs.theta, site_problems.batch("heat-theta", n, 7)
    nets, conds, eqs, nc, scalars = theta_tail_problems.narrow_pair()
    return nets, conds, eqs, nc, scalars, [2 * torch.rand(n, generator=g)]


def _build(name, n):
    from neurodiffeq_amd.engine import FusedSystem
    torch.manual_seed(11)
    nets, conds, eqs, nc, scalars, batch = _system(name, n)
    for net in nets:
        net.to(DEV)
    for p in scalars:
        p.data = p.data.to(DEV)
    system = FusedSystem(nets, conds, eqs, nc, DEV)
    assert system.fusedk is not None and system.n_theta == len(scalars) and not system.theta_frozen
    return system, scalars, batch


LR_THETA = 1e-2


def _epochs_composed(name, n, epochs):
    """The existing entry points one after the other: closure ``step`` (with reduce_theta), per-network sums
    (ndq_reduce_grad_loss), ndq_epoch_tail per network, ndq_adam_step on the scalars."""
    L = _lib.lib()
    system, scalars, batch = _build(name, n)
    fs = system.fast_state()
    moments = [(torch.zeros_like(fp.grad), torch.zeros_like(fp.grad)) for fp in system.flat]
    tm, tv = torch.zeros(len(scalars), device=DEV), torch.zeros(len(scalars), device=DEV)
    group = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
    for e in range(epochs):
        b, _ = system.step(batch, train=True, slot=0)
        seed = 1.0 / (float(n) * system.loss_norm)
        for k, fp in enumerate(system.flat):
            rc = L.ndq_reduce_grad_loss(vp(b["fused_partials_all"][k].data_ptr()), b["fused_blocks"], fp.numel, vp(fp.grad.data_ptr()), 0,
                                        vp(b["fused_loss_partials"].data_ptr()), b["fused_blocks"], vp(system.loss_buf.data_ptr()),
                                        seed, _stream())
            assert rc == 0
        system.epoch_tail("train", 1, True, [(m, v, group, e + 1) for m, v in moments])
        rc = L.ndq_adam_step(vp(system.theta_buf.data_ptr()), vp(system.gtheta.data_ptr()), vp(tm.data_ptr()), vp(tv.data_ptr()),
                             len(scalars), LR_THETA, 0.9, 0.999, 1e-8, 0.0, e + 1, _stream())
        assert rc == 0
        with torch.no_grad():
            for j, p in enumerate(system.theta_params):      # (this route uploads the scalars from their tensors every step)
                p.data.copy_(system.theta_buf[j])
    torch.cuda.synchronize()
    return dict(params=[fp.flat.clone() for fp in system.flat], m=[m for m, _ in moments], v=[v for _, v in moments],
                grad=[fp.grad.clone() for fp in system.flat], gtheta=system.gtheta.clone(), loss=system.loss_buf[0].clone(),
                hist=fs["loss_hist"][:epochs].clone(), best=fs["best_loss"].clone(), best_flat=[t.clone() for t in fs["best_flat"]],
                theta=system.theta_buf.clone(), tm=tm, tv=tv, parity=fs["parity"])


def _epochs_new(name, n, epochs):
    from neurodiffeq_amd.optim import FusedAdam
    system, scalars, batch = _build(name, n)
    opt = FusedAdam([dict(params=[p for net in system.nets for p in net.parameters()]), dict(params=scalars, lr=LR_THETA)])
    assert system.theta_tail_ready(opt) and system.launches_per_step() == 2
    opt.bind(system.flat)
    fs = system.fast_state()
    for _ in range(epochs):
        system.fast_train_epoch_theta(batch, opt, [opt.fast_slot(fp) for fp in system.flat], True)
    torch.cuda.synchronize()
    assert [p.item() for p in system.theta_params] == system.theta_buf.tolist()          # (the system's order: first use in the equations)
    return dict(params=[fp.flat.clone() for fp in system.flat], m=[opt._bound[k][1].clone() for k in range(len(system.flat))],
                v=[opt._bound[k][2].clone() for k in range(len(system.flat))],
                grad=[fp.grad.clone() for fp in system.flat], gtheta=system.gtheta.clone(),
                loss=system.flat[0].grad_loss[system.flat[0].numel].clone(), hist=fs["loss_hist"][:epochs].clone(),
                best=fs["best_loss"].clone(), best_flat=[t.clone() for t in fs["best_flat"]], theta=system.theta_buf.clone(),
                tm=opt._theta["m"], tv=opt._theta["v"], parity=fs["parity"])


@pytest.mark.parametrize("name,n", [("inv1", 64), ("inv1", 1000), ("inv2", 64), ("inv2", 1000), ("lvtheta", 64), ("heat-theta", 64),
                                     ("narrow-pair", 64)])
def test_one_epoch_and_the_next_equal_the_composition_of_the_existing_entry_points(name, n):
    """Two epochs (the second starts from non-zero moments and the other best-loss slot): network parameters, both moments,
    gradients, gtheta, loss slot, history, best-loss ping-pong, best snapshot, the scalars and their moments -- all bit-equal."""
    old, new = _epochs_composed(name, n, 2), _epochs_new(name, n, 2)
    assert old["parity"] == new["parity"]
    for key in ("params", "m", "v", "grad", "best_flat"):
        for k, (a, b) in enumerate(zip(old[key], new[key])):
            assert torch.equal(a, b), (key, k, (a - b).abs().max())
    for key in ("gtheta", "loss", "hist", "best", "theta", "tm", "tv"):
        assert torch.equal(old[key], new[key]), (key, old[key], new[key])
    assert torch.isfinite(new["hist"]).all() and new["gtheta"].abs().min() > 0


# ---------------------------------------------------------------------------------------------- solver level
def _solver(name, how="fused", valid=False, cpu_scalars=False, seed=None, **kw):
    """configs.make_inverse_solver(name) with the scalars on the device and the optimiser of the route under test."""
    from neurodiffeq_amd.optim import FusedAdam
    from tests import configs
    if seed is not None:
        torch.manual_seed(seed)
    if valid:
        kw["n_batches_valid"] = 1
    solver, cfg = configs.make_inverse_solver(name, **kw)
    solver.fused = "require"
    for net in cfg["nets"]:
        net.to(DEV)
    if not cpu_scalars:
        for p in cfg["theta"] + cfg["data"]:                 # (a data column lives where the scalars it meets live)
            p.data = p.data.to(DEV)
    net_params = [p for net in cfg["nets"] for p in net.parameters()]
    if how == "torch":
        solver.optimizer = torch.optim.Adam(net_params + cfg["theta"], lr=1e-3)
    elif how == "missing":
        solver.optimizer = FusedAdam(net_params + cfg["theta"][:1], lr=1e-3)
    elif how == "amsgrad":
        solver.optimizer = FusedAdam(net_params, lr=1e-3)
        solver.optimizer.add_param_group(dict(params=cfg["theta"], amsgrad=True))
    else:
        solver.optimizer = FusedAdam(itertools.chain(net_params, cfg["theta"]), lr=1e-3)
    return solver, cfg


@pytest.fixture
def native_calls(monkeypatch):
    """Counts the epochs that went through engine.fast_train_epoch_theta."""
    from neurodiffeq_amd.engine import FusedSystem
    calls = []
    inner = FusedSystem.fast_train_epoch_theta

    def counted(self, *args, **kw):
        calls.append(self)
        return inner(self, *args, **kw)
    monkeypatch.setattr(FusedSystem, "fast_train_epoch_theta", counted)
    return calls


@pytest.fixture
def host_reads(monkeypatch):
    """Counts the synchronising reads of device tensors (item / tolist / cpu / numpy / float()) and device synchronisations."""
    reads = []
    for attr in ("item", "tolist", "cpu", "numpy", "__float__", "__int__", "__bool__"):
        inner = getattr(torch.Tensor, attr)

        def counted(self, *a, _inner=inner, _attr=attr, **kw):
            if self.is_cuda:
                reads.append(_attr)
            return _inner(self, *a, **kw)
        monkeypatch.setattr(torch.Tensor, attr, counted)
    inner_sync = torch.cuda.synchronize
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **kw: (reads.append("synchronize"), inner_sync(*a, **kw))[1])
    return reads


@pytest.mark.parametrize("name", ["inv1", "inv2"])
def test_solver_trajectory_matches_reference_golden_on_the_device_route(golden_dir, name, native_calls, host_reads):
    """Three epochs of the reference's own run (tests/golden/inv1.npz, inv2.npz) with the FusedAdam owning networks and scalars:
    three native calls of two launches, no synchronising read inside run_train_epoch() once the closure kernel has proved itself
    (the first epoch's self-check against the three-kernel pipeline reads back, as on every native path)."""
    gold = np.load(os.path.join(golden_dir, f"{name}.npz"))
    solver, cfg = _solver(name, seed=int(gold["seed"]))
    torch.manual_seed(int(gold["seed"]) + 2)
    solver.run_train_epoch()
    del host_reads[:]
    solver.run_train_epoch()
    solver.run_train_epoch()
    assert host_reads == [], host_reads
    system = solver._fused_sys
    assert solver.fused_active and system.n_theta == 2
    assert system.theta_tail_ready(solver.optimizer) and system.launches_per_step() == 2 and len(native_calls) == 3
    assert np.allclose(solver.metrics_history["train_loss"], gold["traj_loss"], rtol=2e-5)      # (flushed lazily, here)
    params = R.get_flat(cfg["nets"]).cpu().numpy()
    assert np.linalg.norm(params - gold["traj_params"]) <= 1e-5 * np.linalg.norm(gold["traj_params"])
    assert np.allclose([p.item() for p in cfg["theta"]], gold["traj_theta"], rtol=1e-5)


def _state(solver, cfg):
    return (np.array(solver.metrics_history["train_loss"]), np.array(solver.metrics_history["valid_loss"]),
            R.get_flat(cfg["nets"]).cpu().numpy(), np.array([p.item() for p in cfg["theta"]], dtype=np.float32))


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------- 5. ownership
def test_the_device_vector_owns_the_values(monkeypatch):
    runs = {}
    for route in ("new", "old"):
        monkeypatch.setenv("NDQ_NO_THETA_TAIL", "1" if route == "old" else "0")
        solver, cfg = _solver("inv1", seed=0)
        torch.manual_seed(1)
        solver.run_train_epoch()
        nu = cfg["theta"][0]
        with torch.no_grad():
            nu.data.fill_(0.5)                             # an in-place edit between epochs
        solver.run_train_epoch()
        system = solver._fused_sys
        assert system.theta_tail_ready(solver.optimizer) == (route == "new")
        if route == "new":
            torch.cuda.synchronize()
            theta = system.theta_params                    # (the system's order: first use in the equations)
            assert {id(p) for p in theta} == {id(p) for p in cfg["theta"]}
            assert [p.item() for p in theta] == system.theta_buf.tolist()
            assert all(p.grad.item() == system.gtheta[j].item() for j, p in enumerate(theta))
            kept = [p.grad.clone() for p in cfg["theta"]]
            solver.run_train_epoch()
            torch.cuda.synchronize()
            assert [k.item() for k in kept] != [p.grad.item() for p in cfg["theta"]]            # the view follows the new epoch ...
            assert all(p.grad.item() == system.gtheta[j].item() for j, p in enumerate(theta))
        else:
            solver.run_train_epoch()
        runs[route] = _state(solver, cfg)
    assert runs["new"][0][1] != runs["new"][0][0]
    # the edit changed the second epoch's loss exactly as on the old route (losses: the same closure launch, the tail's sum against
    # the general path's: compared as the golden test compares them)
    assert np.allclose(runs["new"][0], runs["old"][0], rtol=2e-5), (runs["new"][0], runs["old"][0])
    solver0, cfg0 = _solver("inv1", seed=0)
    torch.manual_seed(1)
    solver0.run_train_epoch()
    solver0.run_train_epoch()
    assert abs(solver0.metrics_history["train_loss"][1] - runs["new"][0][1]) > 1e-3 * runs["new"][0][1]      # ... and it mattered


# ---------------------------------------------------------------------------------------------- 6. checkpointing
@pytest.mark.parametrize("how", ["state_dict", "deepcopy"])
def test_a_checkpoint_continues_bit_for_bit(how):
    solver, cfg = _solver("inv1", seed=0)
    torch.manual_seed(1)
    for _ in range(4):
        solver.run_train_epoch()
    want = _state(solver, cfg)
    first, fcfg = _solver("inv1", seed=0)
    torch.manual_seed(1)
    first.run_train_epoch()
    first.run_train_epoch()
    rng = torch.get_rng_state()
    first._flush_device_history()
    sd = first.optimizer.state_dict() if how == "state_dict" else copy.deepcopy(first.optimizer).state_dict()
    assert all(float(s["step"]) == 2.0 for s in sd["state"].values())
    nets_sd = [net.state_dict() for net in fcfg["nets"]]
    values = [p.detach().clone() for p in fcfg["theta"]]
    second, scfg = _solver("inv1", seed=5)
    for net, s in zip(scfg["nets"], nets_sd):
        net.load_state_dict(s)
    with torch.no_grad():
        for p, val in zip(scfg["theta"], values):
            p.copy_(val)
    second.optimizer.load_state_dict(sd)
    torch.set_rng_state(rng)
    second.run_train_epoch()
    second.run_train_epoch()
    got = _state(second, scfg)
    assert np.array_equal(got[0], want[0][2:]) and np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])


# ---------------------------------------------------------------------------------------------- 7. frozen + trainable
def test_a_ramped_number_is_followed_while_the_trainable_scalar_steps_on_the_device(native_calls):
    from neurodiffeq_amd.generators import Generator1D
    from neurodiffeq_amd.optim import FusedAdam
    from neurodiffeq_amd.solvers import Solver1D
    from tests import theta_tail_problems as TP

    def run(ramp):
        torch.manual_seed(0)
        nets, conds, eqs, nc, scalars, state = TP.ramped()
        nets[0].to(DEV)
        scalars[0].data = scalars[0].data.to(DEV)
        gen = Generator1D(64, 0.0, 2.0, "equally-spaced")
        solver = Solver1D(eqs, conds, t_min=0.0, t_max=2.0, nets=nets, train_generator=gen, valid_generator=gen, n_batches_valid=0,
                          optimizer=FusedAdam(list(nets[0].parameters()) + scalars, lr=1e-3))
        solver.fused = "require"
        for value in ramp:
            state["nu"] = value
            solver.run_train_epoch()
        return solver, scalars

    solver, scalars = run(TP.RAMP)
    system = solver._fused_sys
    assert system.n_theta == 2 and len(system.theta_frozen) == 1 and len(system._theta_trainable) == 1
    assert system.theta_tail_ready(solver.optimizer) and len(native_calls) == len(TP.RAMP)
    torch.cuda.synchronize()
    frozen, live = system.theta_frozen[0], system._theta_trainable[0]
    assert system.theta_buf[frozen].item() == np.float32(TP.RAMP[-1])                # the ramp's last value, never stepped
    assert scalars[0].item() == system.theta_buf[live].item() != 2.0
    m = solver.optimizer._theta["m"]
    assert m[frozen] == 0 and m[live] != 0
    still, _ = run([TP.RAMP[0]] * len(TP.RAMP))                                       # the ramp is part of the equation
    assert solver.metrics_history["train_loss"][0] == still.metrics_history["train_loss"][0]
    assert solver.metrics_history["train_loss"][-1] != still.metrics_history["train_loss"][-1]


# ---------------------------------------------------------------------------------------------- 8. fallbacks
@pytest.mark.parametrize("how", ["torch", "cpu", "missing", "amsgrad", "switch"])
def test_fallbacks_keep_the_general_path(monkeypatch, how, native_calls):
    """Not eligible: the predicate is false, nothing goes through the new call, and three epochs equal, bit for bit, the same run
    with NDQ_NO_THETA_TAIL=1 -- the route every such run took before."""
    runs = {}
    for switch in ("0", "1"):
        monkeypatch.setenv("NDQ_NO_THETA_TAIL", "1" if how == "switch" else switch)
        solver, cfg = _solver("inv1", how={"cpu": "fused", "switch": "fused"}.get(how, how), cpu_scalars=(how == "cpu"), seed=0)
        torch.manual_seed(1)
        for _ in range(3):
            solver.run_train_epoch()
        assert solver.fused_active and not solver._fused_sys.theta_tail_ready(solver.optimizer)
        runs[switch] = _state(solver, cfg)
    assert not native_calls and _same(runs["0"], runs["1"])
    assert runs["0"][3][0] != np.float32(0.05)               # the scalars were trained all the same


# ---------------------------------------------------------------------------------------------- 9. fit
def test_fit_equals_single_epochs(native_calls):
    runs = {}
    for how in ("fit", "single"):
        solver, cfg = _solver("inv1", valid=True, seed=0)
        torch.manual_seed(1)
        if how == "fit":
            solver.fit(4, tqdm_file=None)
        else:
            for _ in range(4):
                solver.run_train_epoch()
                solver.run_valid_epoch()
        runs[how] = _state(solver, cfg)
    assert len(native_calls) == 8 and len(runs["fit"][1]) == 4
    assert _same(runs["fit"], runs["single"])
