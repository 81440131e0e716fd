"""Systems of 2 .. 3 one-hidden-layer networks of 80 / 128 units behind ONE closure launch (csrc/ndq_wide.h:
wide_multi_closure_kernel / wide_multi_closure_tv_kernel) on the GPU: against the three-kernel pipeline of the same
FusedSystem, the fp64 autograd oracle and the goldens the unmodified reference produced (wm1, wm2).

Bounds: tests/test_gpu_wide.py's for the one-network wide closure -- 1e-5 (rel-L2 / relative) against the fp64 oracle and
the reference's goldens, 2e-6 between the two launch modes; trajectories 2e-5 (loss) / 1e-5 (parameters)."""
import os

import numpy as np
import pytest
import torch

from oracle import autograd_ref as R
from tests import wide_multi_problems as WM

pytestmark = pytest.mark.gpu
TOL = 1e-5            # closure vs fp64 oracle / reference golden (tests/test_gpu_wide.py: TOL)
TOL_MODES = 2e-6      # single launch vs three-kernel pipeline (tests/test_gpu_wide.py: the README network, "1k" vs "3k")
SIZES = [1, 17, 1000, 4097]      # one lane | one point past a tile | a ragged last tile | more tiles than one round of workgroups


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def _grad(nets, flats):
    where = {}
    for fp in flats:
        for prm, off in zip(fp.params, fp._offsets):
            where[id(prm)] = fp.grad[off:off + prm.numel()]
    return torch.cat([where[id(prm)].reshape(-1) for net in nets for prm in net.parameters()]).cpu().numpy()


_SYSTEMS = {}


def _system(name, width):
    """(nets, closure FusedSystem, pipeline FusedSystem, initial flat parameters), built once per (system, width)."""
    from neurodiffeq_amd.engine import FusedSystem
    key = (name, width)
    if key not in _SYSTEMS:
        torch.manual_seed(0)
        nets, conds, eqs, nc = WM.make(name, width)
        flat0 = R.get_flat(nets).clone()
        for net in nets:
            net.to("cuda")
        one = FusedSystem(nets, conds, eqs, nc, "cuda", single_kernel=True)
        three = FusedSystem(nets, conds, eqs, nc, "cuda", single_kernel=False)
        _SYSTEMS[key] = (nets, one, three, flat0)
    return _SYSTEMS[key]


_ORACLE = {}


def _oracle(name, width, n, flat0):
    """fp64 loss and flat gradient of the batch (computed once per case, never modified)."""
    key = (name, width, n)
    if key not in _ORACLE:
        nets, enf, eqs = WM.make_oracle(name, width)
        R.set_flat(nets, flat0.double())
        out = R.closure(nets, enf, eqs, [c.double() for c in WM.batch(name, n, 100 + n)])
        _ORACLE[key] = (out["loss"].item(), R.get_flat_grad(nets).numpy().copy())
    return _ORACLE[key]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name,width", WM.GPU_CASES, ids=[f"{a}-{b}" for a, b in WM.GPU_CASES])
def test_closure_launch_matches_pipeline_and_oracle(name, width, n):
    from neurodiffeq_amd import codegen
    nets, one, three, flat0 = _system(name, width)
    assert one.fusedk is not None and three.fusedk is None
    assert codegen.fuse_mode(one.program, one.descs) == "wide_multi" and one.fusedk.n_nets == WM.SYSTEMS[name][1]
    # (3) one closure launch + one sums / tail launch; the pipeline's count is what it was before this mode existed
    assert one.launches_per_step() == 2 and one.launches_per_step() < three.launches_per_step()
    R.set_flat(nets, flat0)
    coords = WM.batch(name, n, 100 + n)
    want_loss, want_grad = _oracle(name, width, n, flat0)
    # (1) closure launch vs pipeline vs fp64 oracle
    got = {}
    for tag, fs in (("closure", one), ("pipeline", three)):
        b, m = fs.step(coords, train=True, slot=0)
        torch.cuda.synchronize()
        assert m == n and (b["fusedk"] is not None) == (tag == "closure")
        got[tag] = (fs.loss_buf[0].item(), _grad(nets, fs.flat))
    assert one.fusedk is not None, getattr(one, "fused_check", None)      # (the first-batch self-check kept the build)
    errs = dict(loss_vs_oracle=abs(got["closure"][0] - want_loss) / abs(want_loss),
                grad_vs_oracle=rel_l2(got["closure"][1], want_grad),
                loss_vs_pipeline=abs(got["closure"][0] - got["pipeline"][0]) / abs(got["pipeline"][0]),
                grad_vs_pipeline=rel_l2(got["closure"][1], got["pipeline"][1]))
    print(name, width, n, errs)
    # every network on its own as well: a small network's error must not hide behind a large one's norm
    off = 0
    for k, fp in enumerate(one.flat):
        sl = slice(off, off + fp.numel)
        errs[f"grad{k}_vs_oracle"] = rel_l2(got["closure"][1][sl], want_grad[sl])
        errs[f"grad{k}_vs_pipeline"] = rel_l2(got["closure"][1][sl], got["pipeline"][1][sl])
        off += fp.numel
    assert all(v < (TOL if k.endswith("oracle") else TOL_MODES) for k, v in errs.items()), errs
    # (2) a second launch on the same inputs: the same bits everywhere
    b, _ = one.step(coords, train=True, slot=0)
    torch.cuda.synchronize()
    first = ([t.clone() for t in b["fused_partials_all"]], b["fused_loss_partials"].clone(), one.loss_buf[:1].clone(),
             [fp.grad.clone() for fp in one.flat])
    b2, _ = one.step(coords, train=True, slot=0)
    torch.cuda.synchronize()
    assert b2 is b
    assert all(torch.equal(x, y) for x, y in zip(first[0], b["fused_partials_all"])) and torch.equal(first[1], b["fused_loss_partials"])
    assert torch.equal(first[2], one.loss_buf[:1]) and all(torch.equal(x, fp.grad) for x, fp in zip(first[3], one.flat))
    assert np.array_equal(_grad(nets, one.flat), got["closure"][1]) and one.loss_buf[0].item() == got["closure"][0]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name,width", WM.GPU_CASES, ids=[f"{a}-{b}" for a, b in WM.GPU_CASES])
def test_train_and_validation_launch_matches_the_separate_launches(name, width, n):
    """wide_multi_closure_tv_kernel: its training workgroups leave the partial rows of the training launch bit for bit, its
    validation workgroups the loss of the forward-only launch (held to the launch-mode tolerance; the oracle bounds the value)."""
    from neurodiffeq_amd.engine import _c_vp, _ptr
    nets, one, three, flat0 = _system(name, width)
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
    assert vb["fusedk"] is fk
    params_pp = (_c_vp * len(one.flat))(*[fp.flat.data_ptr() for fp in one.flat])
    parts = [torch.full_like(t, float("nan")) for t in want_parts]
    lp, vp = torch.full_like(want_lp, float("nan")), torch.full_like(want_vp, float("nan"))
    parts_pp = (_c_vp * len(parts))(*[t.data_ptr() for t in parts])
    seed = 1.0 / (float(n) * one.loss_norm)
    rc = fk.lib.ndq_fused_launch_tv(one._coord_ptr(b, 0), b["ld"], n, params_pp, parts_pp, _ptr(lp), seed,
                                    one._coord_ptr(vb, 0), vb["ld"], nv, _ptr(vp), None, stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(lp, want_lp) and all(torch.equal(a, w) for a, w in zip(parts, want_parts))     # loss and gradient rows
    vloss = float(vp.double().sum().item()) / (nv * one.loss_norm)
    assert abs(vloss - want_vloss) < TOL_MODES * abs(want_vloss), (vloss, want_vloss)
    onets, enf, eqs = WM.make_oracle(name, width)
    R.set_flat(onets, flat0.double())
    oracle = R.closure(onets, enf, eqs, [c.double() for c in vcoords], backward=False)["loss"].item()
    assert abs(vloss - oracle) < TOL * abs(oracle), (vloss, oracle)


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
