"""Systems of 2 .. 3 narrow networks in float64 behind ONE closure launch (csrc/ndq_mlp.h: fused_multi_closure_kernel /
fused_multi_closure_tv_kernel compiled under NDQ_F64) on the GPU: against the fp64 three-kernel pipeline of the same tree, the
numbers the unmodified reference produced in double (c1.npz; c1_f64.npz: its float64 defaults end to end) and itself.

Sizes: one lane, one point short of / past a tile, a ragged tile behind four full ones (more than one round for the two tile
slots of a K = 2 workgroup needs more than 2 x 256 tiles: 4 099 points is 257 tiles -- K = 3's single slot goes round again,
K = 2 spreads over 129 workgroups with a ragged last one).

Bounds: 1e-13 (relative / rel-L2) between closure and pipeline, the bound tests/test_gpu_parity.py's fp64 epoch test puts on
two fp64 routes through the same arithmetic; 25 epochs: 1e-12 on the loss history, 5e-13 on the parameters (the factors 10
and 5 tests/test_gpu_site_closure.py puts between its one-step and its 25-epoch bounds); 1e-9 against the reference's fp64
numbers, as tests/test_gpu_netfamily.py::test_fp64_pipeline_matches_reference_golden and tests/test_gpu_wide.py (w22)."""
import os
import warnings

import numpy as np
import pytest
import torch

from oracle import autograd_ref as R
from tests import f64_multi_problems as FP

pytestmark = pytest.mark.gpu
TOL_MODES = 1e-13
TOL_GOLDEN = 1e-9
SIZES = [1, 15, 17, 64 + 5, 4096 + 3]


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


_SYSTEMS = {}


def _system(name):
    """(nets, closure system, pipeline system) of ``name``: one set of networks behind two separately built engines."""
    if name not in _SYSTEMS:
        from neurodiffeq_amd.engine import FusedSystem
        torch.manual_seed(0)
        nets, conds, eqs, d, cfv = FP.make(name)
        for net in nets:
            net.to("cuda")
        kw = dict(compute_func_val=cfv, dtype=torch.float64)
        _SYSTEMS[name] = (nets, FusedSystem(nets, conds, eqs, d, "cuda", **kw),
                          FusedSystem(nets, conds, eqs, d, "cuda", single_kernel=False, **kw))
    return _SYSTEMS[name]


def _step(fs, coords):
    b, n = fs.step(coords, train=True, slot=0, want_funcs=True, want_resid=True)
    torch.cuda.synchronize()
    return b, dict(loss=fs.loss_buf[0].item(), grads=[fp.grad.cpu().numpy().copy() for fp in fs.flat],
                   funcs=b["funcs"][:fs.n_funcs, :n].cpu().numpy().copy(), resid=b["resid"][:fs.n_eq, :n].cpu().numpy().copy())


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", FP.GPU_NAMES)
def test_closure_launch_matches_the_fp64_pipeline(name, n):
    from neurodiffeq_amd import codegen
    with warnings.catch_warnings():
        # a closure kernel its first-batch self-check rejects would pass everything below on the pipeline: an error here
        warnings.simplefilter("error", RuntimeWarning)
        nets, one, three = _system(name)
        K = len(nets)
        assert one.f64 and three.f64 and one.fusedk is not None and three.fusedk is None
        assert codegen.can_fuse_multi_f64(one.program, one.descs) and not codegen.can_fuse_f64(one.program, one.descs)
        assert one.fusedk.n_nets == K and one.fusedk.threads == 64 * K * (2 if K == 2 else 1)
        assert one.fusedk.lib.ndq_fused_pull_ok() == 0 and one.fusedk.lib.ndq_fused_loop_ok() == 0
        assert one.launches_per_step() == 2 + 2 * K < three.launches_per_step()
        assert not one.fast_ready() and not one.fit_ready()
        tiles, slots = -(-n // 16), (2 if K == 2 else 1)
        if n == 4099 and slots == 1:
            assert one.fusedk.blocks(n) == 256 and tiles == 257           # one wave group goes round the tile loop again
        else:
            assert tiles <= slots * one.fusedk.blocks(n)
        coords = FP.batch(name, n, 100 + n)
        b1, got = _step(one, coords)
        b3, want = _step(three, coords)
        assert b1["fusedk"] is not None and b3["fusedk"] is None
        _, again = _step(one, coords)
    assert one.fusedk is not None, getattr(one, "fused_check", None)      # (the first-batch self-check kept the build)
    assert one.fused_check["reproducible"] and one.fused_check["grad_rel_l2"] < TOL_MODES
    errs = dict(loss=abs(got["loss"] - want["loss"]) / abs(want["loss"]))
    for k in range(K):
        errs[f"grad{k}"] = rel_l2(got["grads"][k], want["grads"][k])
    for k in range(got["funcs"].shape[0]):
        errs[f"funcs{k}"] = rel_l2(got["funcs"][k], want["funcs"][k])
    for e in range(got["resid"].shape[0]):
        errs[f"resid{e}"] = rel_l2(got["resid"][e], want["resid"][e])
    print(name, n, errs)
    assert max(errs.values()) < TOL_MODES, errs
    # two runs: bit for bit
    assert got["loss"] == again["loss"] and all(np.array_equal(a, g) for a, g in zip(again["grads"], got["grads"]))
    assert np.array_equal(got["funcs"], again["funcs"]) and np.array_equal(got["resid"], again["resid"])


@pytest.mark.parametrize("n", [17, 4099])
@pytest.mark.parametrize("name", ["c1", "uvp16"])
def test_train_plus_validation_launch_is_the_plain_launches_bit_for_bit(name, n):
    """What engine.verify_fused asserts for fp32 modules: gradient and loss partial sums of the training workgroups of the
    train + validation launch == the plain training launch, loss partial sums of its validation workgroups == the
    forward-only launch; alone and together."""
    nets, one, _ = _system(name)
    coords = FP.batch(name, n, 200 + n)
    b, n_up = one.upload(coords)
    one.set_batch_size(n_up)
    stream = one._stream()
    one.fused_closure(b, n_up, stream, True, n_up, 0, False)
    assert one._tv_matches_plain(b, n_up, n_up, stream)


def test_closure_matches_the_references_double_results_c1(golden_dir):
    from tests import configs
    from tests.test_gpu_netfamily import _grad_in_torch_order
    from neurodiffeq_amd.engine import FusedSystem
    gold = np.load(os.path.join(golden_dir, "c1.npz"))
    torch.manual_seed(0)
    cfg = configs.make("c1", 64)
    for net in cfg["nets"]:
        net.double().to("cuda")
    R.set_flat(cfg["nets"], torch.from_numpy(gold["params0"]).double())
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        fs = FusedSystem(cfg["nets"], cfg["conds"], configs.fused_equations(cfg), 1, "cuda", compute_func_val=configs.func_val(cfg),
                         dtype=torch.float64)
        assert fs.fusedk is not None and fs.fusedk.n_nets == 2
        b, n = fs.step([torch.from_numpy(c).double() for c in gold["coords"]], train=True, slot=0, want_funcs=True, want_resid=True)
        torch.cuda.synchronize()
    assert fs.fusedk is not None and b["fusedk"] is not None
    errs = dict(funcs=rel_l2(b["funcs"][:, :n].T.cpu().numpy(), gold["funcs_f64"]),
                residuals=rel_l2(b["resid"][:, :n].T.cpu().numpy()[:, :gold["residuals_f64"].shape[1]], gold["residuals_f64"]),
                loss=abs(fs.loss_buf[0].item() - float(gold["loss_f64"])) / abs(float(gold["loss_f64"])),
                grad=rel_l2(_grad_in_torch_order(cfg["nets"], fs.flat), gold["grad_f64"]))
    print(errs)
    assert max(errs.values()) < TOL_GOLDEN, errs


def test_w8_in_double_keeps_the_pipeline_and_matches_the_reference(golden_dir):
    """w8's two tanh 32 x 32 networks carry a Neumann end each (four evaluation sites): outside the fp64 closures.  In double it
    runs the three-kernel pipeline, against the same golden numbers."""
    from tests import configs
    from tests.test_gpu_netfamily import _grad_in_torch_order
    from neurodiffeq_amd.engine import FusedSystem
    gold = np.load(os.path.join(golden_dir, "w8.npz"))
    torch.manual_seed(0)
    cfg = configs.make("w8", None)
    for net in cfg["nets"]:
        net.double().to("cuda")
    R.set_flat(cfg["nets"], torch.from_numpy(gold["params0"]).double())
    fs = FusedSystem(cfg["nets"], cfg["conds"], configs.fused_equations(cfg), 1, "cuda", compute_func_val=configs.func_val(cfg),
                     dtype=torch.float64)
    assert fs.fusedk is None and fs.n_sites == 4
    b, n = fs.step([torch.from_numpy(c).double() for c in gold["coords"]], train=True, slot=0, want_funcs=True, want_resid=True)
    torch.cuda.synchronize()
    errs = dict(funcs=rel_l2(b["funcs"][:, :n].T.cpu().numpy(), gold["funcs_f64"]),
                residuals=rel_l2(b["resid"][:, :n].T.cpu().numpy()[:, :gold["residuals_f64"].shape[1]], gold["residuals_f64"]),
                loss=abs(fs.loss_buf[0].item() - float(gold["loss_f64"])) / abs(float(gold["loss_f64"])),
                grad=rel_l2(_grad_in_torch_order(cfg["nets"], fs.flat), gold["grad_f64"]))
    assert max(errs.values()) < TOL_GOLDEN, errs


def _c1_default_precision_trajectory(gold):
    from tests import configs
    from neurodiffeq_amd.utils import set_tensor_type
    set_tensor_type(device="cpu", float_bits=64)          # (cpu default device: the host generator's numbers, bit for bit)
    try:
        torch.manual_seed(int(gold["seed"]))
        solver, cfg = configs.make_solver("c1", 64)
        assert np.array_equal(R.get_flat(cfg["nets"]).cpu().numpy(), gold["params0"])    # same initialisation, in double
        solver.fused = "require"
        torch.manual_seed(int(gold["seed"]) + 2)
        with warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)
            for _ in range(3):
                solver.run_train_epoch()
        assert solver.fused_active and solver._fused_sys.f64
        hist = np.array(solver.metrics_history["train_loss"])
        params = R.get_flat(cfg["nets"]).cpu().numpy()
        return solver, dict(loss=float(np.max(np.abs(hist - gold["traj_loss"]) / np.abs(gold["traj_loss"]))),
                            params=rel_l2(params, gold["traj_params"]))
    finally:
        set_tensor_type(device="cpu", float_bits=32)


@pytest.mark.parametrize("mode", ["closure", "pipeline"])
def test_three_epochs_follow_the_reference_under_its_float64_defaults(golden_dir, monkeypatch, mode):
    """C1 at 64 points the way an unchanged reference script runs it (tests/golden/make_f64_multi_golden.py: networks
    initialised in double, points drawn in double, three epochs of the default Adam) against the product's solver from the same
    seeds.  Bound 1e-9, tests/test_gpu_wide.py's for the same comparison (w22); the pipeline -- what the commit before the
    fp64 multi-network closure ran, NDQ_F64_CLOSURE=0 here -- and the closure are held to it alike.
    Measured distance from the fixture (loss history, max relative / final parameters, rel-L2):
        pipeline  loss 0.0 (bit for bit)   parameters 2.32e-17
        closure   loss 1.39e-16             parameters 2.43e-17"""
    gold = np.load(os.path.join(golden_dir, "c1_f64.npz"))
    if mode == "pipeline":
        monkeypatch.setenv("NDQ_F64_CLOSURE", "0")
    solver, errs = _c1_default_precision_trajectory(gold)
    assert (solver._fused_sys.fusedk is not None) == (mode == "closure")
    print(mode, errs)
    assert errs["loss"] < TOL_GOLDEN and errs["params"] < TOL_GOLDEN, errs


def test_solver_fit_in_double_on_the_closure_follows_the_pipeline(monkeypatch):
    """Solver1D.fit, 25 Adam epochs of C1 with fp64 networks: one closure launch per epoch, then the separate fixed-order sums
    and the epoch tail in double (2 + 2 K launches; the one sums-and-tail launch of the fp32 route has no fp64 counterpart
    yet), against the three-kernel pipeline (NDQ_F64_CLOSURE=0) from the same seed."""
    from tests import configs

    def run(closure):
        if closure:
            monkeypatch.delenv("NDQ_F64_CLOSURE", raising=False)
        else:
            monkeypatch.setenv("NDQ_F64_CLOSURE", "0")
        torch.manual_seed(0)
        s, cfg = configs.make_solver("c1", 64)
        for net in cfg["nets"]:
            net.double()
        s.fused = "require"
        torch.manual_seed(7)
        with warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)
            s.fit(25, tqdm_file=None)
        return s, cfg
    (a, ca), (b, cb) = run(True), run(False)
    assert a.fused_active and b.fused_active and a._fused_sys.f64 and b._fused_sys.f64
    assert a._fused_sys.fusedk is not None and b._fused_sys.fusedk is None
    assert a._fused_sys.launches_per_step() == 6 < b._fused_sys.launches_per_step()
    ha, hb = np.array(a.metrics_history["train_loss"]), np.array(b.metrics_history["train_loss"])
    assert ha.dtype == np.float64 and len(ha) == len(hb) == 25
    assert a._fused_sys._fast["loss_hist"].dtype == torch.float64
    pa, pb = R.get_flat(ca["nets"]).cpu().numpy(), R.get_flat(cb["nets"]).cpu().numpy()
    errs = dict(loss=float(np.max(np.abs(ha - hb) / np.abs(hb))), params=rel_l2(pa, pb))
    print(errs)
    assert pa.dtype == np.float64 and errs["loss"] < 10 * TOL_MODES and errs["params"] < 5 * TOL_MODES, errs


def test_four_networks_at_32x32_follow_the_lds_gate():
    """K = 4 at 32 x 32 in double: the module is built, and the engine keeps it exactly when it fits 160 KiB of LDS."""
    from neurodiffeq_amd import codegen
    from neurodiffeq_amd.engine import FusedSystem
    torch.manual_seed(0)
    nets, conds, eqs, d, cfv = FP.make(FP.OVER_NAME)
    for net in nets:
        net.to("cuda")
    fs = FusedSystem(nets, conds, eqs, d, "cuda", dtype=torch.float64)
    assert codegen.can_fuse_multi_f64(fs.program, fs.descs)
    lib = codegen.FusedKernel(codegen.build_fused(fs.program, fs.descs[0], f64=True), True).lib
    assert (fs.fusedk is not None) == (lib.ndq_fused_lds_bytes() <= 160 * 1024)
    b, n = fs.step(FP.batch(FP.OVER_NAME, 33, 5), train=True, slot=0)
    torch.cuda.synchronize()
    assert np.isfinite(fs.loss_buf[0].item()) and (b["fusedk"] is not None) == (fs.fusedk is not None)
