"""Systems of 2 .. 4 one-hidden-layer networks of 65 .. 512 units behind ONE closure launch (csrc/ndq_wide.h:
wide_multi_closure_kernel / wide_multi_closure_tv_kernel) on the GPU: against the three-kernel pipeline of the same
FusedSystem, the fp64 autograd oracle and the goldens the unmodified reference produced (wm1, wm2).

The matrix (tests/wide_multi_problems.py: GPU_CASES) runs every lane layout of WideCfg (16 / 32 / 64 unit lanes, ragged last
unit rows), K = 2, 3 and 4, both ways of keeping the activation states (KEEP_ALL and the second forward pass), third-order and
mixed second-order streams, tanh / sin / sigmoid / swish / GELU, trainable scalars in the equations, and batch sizes at which a
wave's tile loop takes a second and a third trip (more than 16 384 points: 256 workgroups of four 16-point tiles).

Bounds: tests/test_gpu_wide.py's for the one-network wide closure -- 1e-5 (rel-L2 / relative) against the fp64 oracle and
the reference's goldens, 2e-6 between the two launch modes; trajectories 2e-5 (loss) / 1e-5 (parameters)."""
import json
import os
import warnings

import numpy as np
import pytest
import torch

from oracle import autograd_ref as R
from tests import wide_multi_problems as WM

pytestmark = pytest.mark.gpu
TOL = 1e-5            # closure vs fp64 oracle / reference golden (tests/test_gpu_wide.py: TOL)
TOL_MODES = 2e-6      # single launch vs three-kernel pipeline (tests/test_gpu_wide.py: the README network, "1k" vs "3k")
DIAG = os.environ.get("NDQ_TEST_DIAG")      # a directory: every case's measured errors as JSON (profiles/wide_multi_coverage.md)
# one lane | one point past a tile | a ragged last tile | several workgroups, a ragged last one (257 tiles: still ONE tile per wave)
SIZES = [1, 17, 1000, 4097]
# a workgroup's four waves take one 16-point tile each and the grid stops at 256 workgroups, so the tile loop goes round again
# only past 1 024 tiles: 16 400 points are 1 025 tiles (exactly one wave takes a second trip), 33 000 points 2 063 tiles with a
# ragged last one (two and three trips per wave)
TILE_LOOP_SIZES = [16400, 33000]
MAX_BLOCKS, WAVES = 256, 4

FUSED_CASES = [c for c in WM.GPU_CASES if c not in WM.OVER_LDS]
ALL_SIZES = [("lv", 80), ("lv", 128), ("uvp", 80), ("uvp", 128),      # the 16-unit-lane layout ...
             ("lv", 65), ("lv", 200), ("four", 512)]                  # ... and one case per lane layout: 16 / 32 / 64 unit lanes
TILE_LOOP = [("lv", 128), ("uvp", 128), ("uvp", 200), ("four", 72)]


def _matrix():
    out = []
    for case in FUSED_CASES:
        sizes = (SIZES if case in ALL_SIZES else [17, 1000]) + (TILE_LOOP_SIZES if case in TILE_LOOP else [])
        out += [pytest.param(case, n, id=f"{WM.case_id(case)}-{n}") for n in sizes]
    return out


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def _grad(nets, flats):
    where = {}
    for fp in flats:
        for prm, off in zip(fp.params, fp._offsets):
            where[id(prm)] = fp.grad[off:off + prm.numel()]
    return torch.cat([where[id(prm)].reshape(-1) for net in nets for prm in net.parameters()]).cpu().numpy()


def _blocks(case):
    """(name, lo, hi) of a network's parameter blocks in torch's order: W1 | b1 | Wout | bout."""
    d, w = WM.SYSTEMS[case[0]][2], case[1]
    return (("W1", 0, d * w), ("b1", d * w, d * w + w), ("Wout", d * w + w, d * w + 2 * w), ("bout", d * w + 2 * w, d * w + 2 * w + 1))


_SYSTEMS = {}


def _system(case):
    """(nets, closure FusedSystem, pipeline FusedSystem, initial flat parameters, equations), built once per case; only the case
    at hand is kept (the tests walk the matrix case by case: two FusedSystems with their buffer sets at a time)."""
    from neurodiffeq_amd.engine import FusedSystem
    if case not in _SYSTEMS:
        _SYSTEMS.clear()
        _ORACLE.clear()
        torch.manual_seed(0)
        nets, conds, eqs, nc = WM.make(*case)
        flat0 = R.get_flat(nets).clone()
        for net in nets:
            net.to("cuda")
        one = FusedSystem(nets, conds, eqs, nc, "cuda", single_kernel=True)
        three = FusedSystem(nets, conds, eqs, nc, "cuda", single_kernel=False)
        _SYSTEMS[case] = (nets, one, three, flat0, eqs)
    return _SYSTEMS[case]


_ORACLE = {}


def _oracle(case, n, seed, flat0, backward=True):
    """fp64 closure of the batch ``WM.batch(name, n, seed)``: loss, flat gradient, function values and residuals [row][point],
    gradient of the equations' scalars (computed once per case and batch, never modified)."""
    key = (case, n, seed, backward)
    if key not in _ORACLE:
        nets, enf, eqs = WM.make_oracle(*case)
        R.set_flat(nets, flat0.double())
        out = R.closure(nets, enf, eqs, [c.double() for c in WM.batch(case[0], n, seed)], backward=backward)
        _ORACLE[key] = dict(loss=out["loss"].item(), grad=R.get_flat_grad(nets).numpy().copy() if backward else None,
                            funcs=out["funcs"].numpy().T.copy(), resid=out["residuals"].numpy().T.copy(),
                            theta=np.array([p.grad.item() for p in eqs.theta]) if backward else None)
    return _ORACLE[key]


def _step(fs, nets, eqs, coords, n):
    """One training step with function values and residuals: what the launch mode at hand leaves."""
    b, m = fs.step(coords, train=True, slot=0, want_funcs=True, want_resid=True)
    fs.attach_theta_grads()
    torch.cuda.synchronize()
    assert m == n
    return b, dict(loss=fs.loss_buf[0].item(), grad=_grad(nets, fs.flat), funcs=b["funcs"][:fs.n_user_funcs, :n].cpu().numpy(),
                   resid=b["resid"][:fs.n_eq, :n].cpu().numpy(), theta=np.array([p.grad.item() for p in eqs.theta]))


def _compare(case, got, want, tag, errs):
    """Relative errors of one evaluation against another into ``errs``: loss, gradient (whole, per network, per parameter block
    of every network -- each block over that network's whole gradient norm, as tests/test_gpu_wide.py does, so that a wrong last
    unit row, one bias or one output weight shows), every function's values and every residual row over the batch's points,
    the equations' scalars (each over the norm of their gradient)."""
    K = WM.SYSTEMS[case[0]][1]
    errs[f"loss_vs_{tag}"] = abs(got["loss"] - want["loss"]) / abs(want["loss"])
    errs[f"grad_vs_{tag}"] = rel_l2(got["grad"], want["grad"])
    P = got["grad"].size // K
    assert P * K == want["grad"].size and P == _blocks(case)[-1][2]
    for k in range(K):
        g, w = got["grad"][k * P:(k + 1) * P], want["grad"][k * P:(k + 1) * P]
        errs[f"grad{k}_vs_{tag}"] = rel_l2(g, w)
        for name, lo, hi in _blocks(case):
            errs[f"grad{k}_{name}_vs_{tag}"] = float(np.linalg.norm(g[lo:hi].astype(np.float64) - w[lo:hi]) / np.linalg.norm(w))
    assert got["funcs"].shape == want["funcs"].shape and got["resid"].shape == want["resid"].shape
    for k in range(got["funcs"].shape[0]):
        errs[f"funcs{k}_vs_{tag}"] = rel_l2(got["funcs"][k], want["funcs"][k])
    for e in range(got["resid"].shape[0]):
        errs[f"resid{e}_vs_{tag}"] = rel_l2(got["resid"][e], want["resid"][e])
    for j in range(len(want["theta"])):
        errs[f"theta{j}_vs_{tag}"] = float(abs(got["theta"][j] - want["theta"][j]) / np.linalg.norm(want["theta"]))


def _record(test, case, n, errs):
    if not DIAG:
        return
    os.makedirs(DIAG, exist_ok=True)
    with open(os.path.join(DIAG, f"wide_multi_{test}_{WM.case_id(case)}_{n}.json"), "w") as fh:
        json.dump(errs, fh, indent=1)


def _assert_tile_loop(fk, n):
    """The sizes meant to send waves round the tile loop again do: the grid has stopped growing and there are more tiles than
    waves."""
    assert fk.blocks(n) == MAX_BLOCKS and -(-n // 16) > WAVES * MAX_BLOCKS, (n, fk.blocks(n))


@pytest.mark.parametrize("case,n", _matrix())
def test_closure_launch_matches_pipeline_and_oracle(case, n):
    from neurodiffeq_amd import codegen
    name, K = case[0], WM.SYSTEMS[case[0]][1]
    with warnings.catch_warnings():
        # a closure kernel its first-batch self-check rejects would pass everything below on the pipeline: an error here
        warnings.simplefilter("error", RuntimeWarning)
        nets, one, three, flat0, eqs = _system(case)
        assert one.fusedk is not None and three.fusedk is None
        assert codegen.fuse_mode(one.program, one.descs) == "wide_multi" and one.fusedk.n_nets == K
        assert one.n_theta == len(eqs.theta) == (2 if name == "lvtheta" else 0)
        # (3) one closure launch + one sums / tail launch; the pipeline's count is what it was before this mode existed
        assert one.launches_per_step() == 2 and one.launches_per_step() < three.launches_per_step()
        if n in TILE_LOOP_SIZES:
            _assert_tile_loop(one.fusedk, n)
        else:
            assert -(-n // 16) <= WAVES * one.fusedk.blocks(n)          # (one tile per wave at the most)
        R.set_flat(nets, flat0)
        coords = WM.batch(name, n, 100 + n)
        want = _oracle(case, n, 100 + n, flat0)
        # (1) closure launch vs pipeline vs fp64 oracle
        got = {}
        for tag, fs in (("closure", one), ("pipeline", three)):
            b, got[tag] = _step(fs, nets, eqs, coords, n)
            assert (b["fusedk"] is not None) == (tag == "closure")
    assert one.fusedk is not None, getattr(one, "fused_check", None)      # (the first-batch self-check kept the build)
    errs = {}
    _compare(case, got["closure"], want, "oracle", errs)
    _compare(case, got["closure"], got["pipeline"], "pipeline", errs)
    _compare(case, got["pipeline"], want, "pipeline-oracle", errs)        # (recorded, not asserted: which side is off if one is)
    print(WM.case_id(case), n, errs)
    _record("closure", case, n, errs)
    # everything against the oracle at TOL; loss and every piece of the gradient between the launch modes at TOL_MODES (function
    # values and residuals of the two modes are two fp32 evaluations the oracle bounds one by one: recorded)
    held = {k: v for k, v in errs.items() if k.endswith("_vs_oracle") or (k.endswith("_vs_pipeline") and not k.startswith(("funcs", "resid")))}
    assert all(v < (TOL if k.endswith("_vs_oracle") else TOL_MODES) for k, v in held.items()), {k: v for k, v in held.items() if v >= TOL_MODES}
    # (2) a second launch on the same inputs: the same bits everywhere
    b, _ = one.step(coords, train=True, slot=0)
    torch.cuda.synchronize()
    first = ([t.clone() for t in b["fused_partials_all"]], b["fused_loss_partials"].clone(), one.loss_buf[:1].clone(),
             [fp.grad.clone() for fp in one.flat], one.gtheta.clone() if one.n_theta else None)
    b2, _ = one.step(coords, train=True, slot=0)
    torch.cuda.synchronize()
    assert b2 is b
    assert all(torch.equal(x, y) for x, y in zip(first[0], b["fused_partials_all"])) and torch.equal(first[1], b["fused_loss_partials"])
    assert torch.equal(first[2], one.loss_buf[:1]) and all(torch.equal(x, fp.grad) for x, fp in zip(first[3], one.flat))
    assert one.n_theta == 0 or torch.equal(first[4], one.gtheta)
    assert np.array_equal(_grad(nets, one.flat), got["closure"]["grad"]) and one.loss_buf[0].item() == got["closure"]["loss"]


@pytest.mark.parametrize("case,n", _matrix())
def test_train_and_validation_launch_matches_the_separate_launches(case, n):
    """wide_multi_closure_tv_kernel: its training workgroups leave the partial rows of the training launch bit for bit, its
    validation workgroups the loss of the forward-only launch (held to the launch-mode tolerance; the oracle bounds the value)."""
    from neurodiffeq_amd.engine import _c_vp, _ptr
    name = case[0]
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        nets, one, three, flat0, eqs = _system(case)
        R.set_flat(nets, flat0)
        coords = WM.batch(name, n, 100 + n)
        nv = n + 5                                            # (another batch, another buffer set)
        vcoords = WM.batch(name, nv, 900 + n)
        b, _ = one.step(coords, train=True, slot=0)           # training launch
        torch.cuda.synchronize()
        want_parts = [t.clone() for t in b["fused_partials_all"]]
        want_lp = b["fused_loss_partials"].clone()
        vb, _ = one.step(vcoords, train=False, slot=1)        # forward-only launch
        torch.cuda.synchronize()
    want_vloss = one.loss_buf[1].item()
    want_vp = vb["fused_loss_partials"].clone()
    fk, stream = b["fusedk"], one._stream()
    assert fk is not None and vb["fusedk"] is fk
    # the combined launch gives the training batch the first blocks(n) workgroups and the validation batch the next blocks(nv),
    # each half walking its tiles with its own workgroup count (csrc/ndq_closure_host.h: launch_tv)
    tb, vblocks = fk.blocks(n), fk.blocks(nv)
    assert tb == b["fused_blocks"] == want_lp.numel() and vblocks == vb["fused_blocks"] == want_vp.numel()
    if n in TILE_LOOP_SIZES:
        _assert_tile_loop(fk, n)
        _assert_tile_loop(fk, nv)
        assert -(-nv // 16) > WAVES * vblocks                 # the validation half's share of the grid goes round again as well
    params_pp = (_c_vp * len(one.flat))(*[fp.flat.data_ptr() for fp in one.flat])
    parts = [torch.full_like(t, float("nan")) for t in want_parts]
    lp, vp = torch.full_like(want_lp, float("nan")), torch.full_like(want_vp, float("nan"))
    parts_pp = (_c_vp * len(parts))(*[t.data_ptr() for t in parts])
    seed = 1.0 / (float(n) * one.loss_norm)
    if one.n_theta:                                           # the scalars' block sums of the training half: the training batch's rows
        assert b["theta_partials"].shape[0] >= tb
        want_tp = b["theta_partials"][:tb].clone()
        b["theta_partials"][:tb].fill_(float("nan"))
        one._bind_theta(b, fk.lib, True)
    rc = fk.lib.ndq_fused_launch_tv(one._coord_ptr(b, 0), b["ld"], n, params_pp, parts_pp, _ptr(lp), seed,
                                    one._coord_ptr(vb, 0), vb["ld"], nv, _ptr(vp), None, stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(lp, want_lp) and all(torch.equal(a, w) for a, w in zip(parts, want_parts))     # loss and gradient rows
    assert not one.n_theta or torch.equal(b["theta_partials"][:tb], want_tp)
    vloss = float(vp.double().sum().item()) / (nv * one.loss_norm)
    oracle = _oracle(case, nv, 900 + n, flat0, backward=False)["loss"]
    errs = dict(vloss_vs_forward_launch=abs(vloss - want_vloss) / abs(want_vloss), vloss_vs_oracle=abs(vloss - oracle) / abs(oracle))
    print(WM.case_id(case), n, errs)
    _record("tv", case, n, errs)
    assert errs["vloss_vs_forward_launch"] < TOL_MODES, (vloss, want_vloss)
    assert errs["vloss_vs_oracle"] < TOL, (vloss, oracle)


@pytest.mark.parametrize("case", WM.OVER_LDS, ids=WM.case_id)
def test_system_over_the_lds_budget_stays_on_the_pipeline_and_is_right(case):
    """Four 512-unit networks of two inputs with six streams: inside the family, but K unit images + staging are more than one
    workgroup's 160 KiB.  engine.FusedSystem drops the module without a word and the pipeline computes the closure."""
    from neurodiffeq_amd import codegen
    from neurodiffeq_amd.engine import FusedSystem
    name, n = case[0], 1000
    torch.manual_seed(0)
    nets, conds, eqs, nc = WM.make(*case)
    flat0 = R.get_flat(nets).clone()
    for net in nets:
        net.to("cuda")
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        fs = FusedSystem(nets, conds, eqs, nc, "cuda", single_kernel=True)
        assert codegen.fuse_mode(fs.program, fs.descs) == "wide_multi" and codegen.can_fuse(fs.program, fs.descs)
        assert fs.fusedk is None and fs.launches_per_step() > 2
        b, got = _step(fs, nets, eqs, WM.batch(name, n, 100 + n), n)
        assert b["fusedk"] is None and fs.fusedk is None
    assert not seen, [str(w.message) for w in seen]
    errs = {}
    _compare(case, got, _oracle(case, n, 100 + n, flat0), "oracle", errs)
    print(WM.case_id(case), n, errs)
    _record("pipeline", case, n, errs)
    _ORACLE.clear()
    assert max(errs.values()) < TOL, errs


@pytest.mark.parametrize("gname", list(WM.GOLDEN))
def test_reference_goldens(golden_dir, gname):
    """One closure and three Adam epochs against what the unmodified reference produced (wm1 / wm2: 256 points), at the tolerance
    the w17 - w20 goldens are held to in tests/test_gpu_wide.py."""
    import warnings
    from neurodiffeq_amd.engine import FusedSystem
    name, width = WM.GOLDEN[gname]
    gold = np.load(os.path.join(golden_dir, f"{gname}.npz"))
    torch.manual_seed(0)
    nets, conds, eqs, nc = WM.make(name, width)
    for net in nets:
        net.to("cuda")
    fs = FusedSystem(nets, conds, eqs, nc, "cuda")
    assert fs.fusedk is not None and fs.fusedk.n_nets == len(nets)
    R.set_flat(nets, torch.from_numpy(gold["params0"]))
    b, n = fs.step([torch.from_numpy(c) for c in gold["coords"]], train=True, slot=0, want_funcs=True, want_resid=True)
    torch.cuda.synchronize()
    assert fs.fusedk is not None and n == 256
    errs = dict(funcs=rel_l2(b["funcs"][:, :n].T.cpu().numpy(), gold["funcs_f64"]),
                residuals=rel_l2(b["resid"][:, :n].T.cpu().numpy()[:, :gold["residuals_f64"].shape[1]], gold["residuals_f64"]),
                loss=abs(fs.loss_buf[0].item() - float(gold["loss_f64"])) / abs(float(gold["loss_f64"])),
                grad=rel_l2(_grad(nets, fs.flat), gold["grad_f64"]))
    assert max(errs.values()) < TOL, errs
    torch.manual_seed(int(gold["seed"]))
    solver, nets, gen = WM.make_solver(name, width)
    solver.fused = "require"
    assert np.array_equal(R.get_flat(nets).cpu().numpy(), gold["params0"])
    torch.manual_seed(int(gold["seed"]) + 2)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        for _ in range(3):
            solver.run_train_epoch()
    assert solver.fused_active and solver._fused_sys.fusedk is not None
    hist = np.array(solver.metrics_history["train_loss"])
    errs = dict(loss=float(np.max(np.abs(hist - gold["traj_loss"]) / np.abs(gold["traj_loss"]))),
                params=rel_l2(R.get_flat(nets).cpu().numpy(), gold["traj_params"]))
    assert errs["loss"] < 2e-5 and errs["params"] < 1e-5, (errs, hist, gold["traj_loss"])


def test_solver_on_lotka_volterra_with_two_wide_networks():
    """Solver1D, two FCNN(1, 1, (128,)): 25 epochs on the fused path (one closure launch per epoch) against the composite
    torch path from one seed."""
    from neurodiffeq_amd import diff
    from neurodiffeq_amd.conditions import IVP
    from neurodiffeq_amd.networks import FCNN
    from neurodiffeq_amd.solvers import Solver1D

    def run(mode):
        torch.manual_seed(0)
        s = Solver1D(WM.equations("lv", diff), [IVP(0.0, WM.LV_X0), IVP(0.0, WM.LV_Y0)], t_min=0.0, t_max=1.0,
                     nets=[FCNN(1, 1, hidden_units=(128,)) for _ in range(2)], n_batches_valid=1)
        s.fused = mode
        s.fit(25, tqdm_file=None)
        return s
    a, b = run("require"), run("off")
    assert a.fused_active and not b.fused_active
    assert a._fused_sys.fusedk is not None and a._fused_sys.fusedk.n_nets == 2 and a._fused_sys.launches_per_step() == 2
    assert len(a.metrics_history["train_loss"]) == 25 and len(a.metrics_history["valid_loss"]) == 25
    assert np.allclose(a.metrics_history["train_loss"], b.metrics_history["train_loss"], rtol=3e-4)
    assert np.allclose(a.metrics_history["valid_loss"], b.metrics_history["valid_loss"], rtol=3e-4)
    best = R.get_flat(list(a.best_nets)).cpu().numpy()
    assert best.size == 2 * (3 * 128 + 1) and np.isfinite(best).all()
