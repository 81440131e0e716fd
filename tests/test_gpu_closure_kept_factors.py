"""The 8-wave build of the single-launch closure kernel (two waves per SIMD, csrc/ndq_mlp.h: Cfg::REUSE_FWD) lets the
reverse pass reuse the forward pass's last-layer activation streams and activation factors.  C2's problem
(Laplace, DirichletBVP2D, FCNN 2-32-32-1) through that build, forced for small batches, against

* the 4-wave build of the same module (it has always kept its activations) on the same batch and parameters: both run
  the same per-tile arithmetic, so they differ by the fp32 summation order across workgroups only.  Bound: 1e-5 on the
  gradient (rel-L2) and on the loss, the bound tests/test_gpu_parity.py::
  test_closure_kernel_self_check_accepts_good_and_rejects_bad_kernels puts on closure kernel versus pipeline;
* the fp64 autograd oracle (oracle/autograd_ref.py) under the 1e-5 rel-L2 contract -- at the trained state, where the
  residual is a cancellation of O(1) terms, under the bound of tests/test_gpu_parity.py::
  test_near_convergence_parity_against_the_reference_trained_state: the contract, or twice the reference's own
  fp32-vs-fp64 error where that is larger.
"""
import os

import numpy as np
import pytest
import torch

from oracle import autograd_ref as R

pytestmark = pytest.mark.gpu

TOL = 1e-5
FULL_GRID = 16 * 8 * 256        # points of one tile per wave of a full grid: 16 points x 8 waves x 256 workgroups


def rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def _system(nets, cfg, eight_waves):
    from neurodiffeq_amd.engine import FusedSystem
    from tests import configs
    fs = FusedSystem(nets, cfg["conds"], configs.fused_equations(cfg), 2, "cuda", single_kernel=True)
    assert fs.fusedk is not None
    if eight_waves:
        fs.WIDE_MIN_POINTS = 0
        fs.prefers_wide = lambda n: True
    else:
        fs.fusedk_wide = False
    return fs


def _closure(fs, coords, threads):
    b, n = fs.step(coords, train=True, slot=0)
    torch.cuda.synchronize()
    assert b["fusedk"].threads == threads, b["fusedk"].threads
    assert fs.fused_check["reproducible"], fs.fused_check
    return float(fs.loss_buf[0].item()), fs.flat[0].grad.cpu().numpy().copy()


def _both_builds(act, params, coords):
    """(loss, grad) of one closure launch of the 8-wave build and of the 4-wave build."""
    from tests import configs
    from neurodiffeq_amd.networks import FCNN
    torch.manual_seed(0)
    cfg = configs.make("c2", 8)
    nets = [FCNN(2, 1, hidden_units=(32, 32), actv={"tanh": torch.nn.Tanh, "sigmoid": torch.nn.Sigmoid}[act])]
    if params is not None:
        R.set_flat(nets, params)
    flat = R.get_flat(nets).cpu()
    for net in nets:
        net.to("cuda")
    wide = _closure(_system(nets, cfg, True), coords, 512)
    narrow = _closure(_system(nets, cfg, False), coords, 256)
    return flat, wide, narrow


def _oracle(act, flat, coords):
    ocfg = R.build_config("c2", 8, dtype=torch.float64)
    nets = [R.make_fcnn(2, 1, (32, 32), act, torch.float64)]
    R.set_flat(nets, flat.double())
    out = R.closure(nets, ocfg["enforcers"], ocfg["pde"], [c.double() for c in coords])
    return float(out["loss"].item()), R.get_flat_grad(nets).numpy()


def _batch(n):
    g = torch.Generator().manual_seed(7)
    return [torch.rand(n, generator=g), torch.rand(n, generator=g)]


def _check(name, wide, narrow, want, bound64):
    errs = dict(loss_vs_4wave=abs(wide[0] - narrow[0]) / abs(narrow[0]), grad_vs_4wave=rel_l2(wide[1], narrow[1]),
                loss_vs_fp64=abs(wide[0] - want[0]) / abs(want[0]), grad_vs_fp64=rel_l2(wide[1], want[1]))
    print(name, errs, "bound vs fp64:", bound64, flush=True)
    assert errs["loss_vs_4wave"] < TOL and errs["grad_vs_4wave"] < TOL, errs
    assert errs["loss_vs_fp64"] < bound64["loss"] and errs["grad_vs_fp64"] < bound64["grad"], (errs, bound64)


# 1 point: a single partly filled tile, every other wave idle.  FULL_GRID + 5: every wave of a full grid has one tile, a
# ragged remainder gives some waves a second one (tile loop + partial tile).  sigmoid: a second Act<>'s factors.
@pytest.mark.parametrize("act,n", [("tanh", 1), ("tanh", FULL_GRID + 5), ("sigmoid", FULL_GRID + 5)])
def test_eight_wave_closure_matches_four_wave_build_and_fp64_oracle(act, n):
    coords = _batch(n)
    flat, wide, narrow = _both_builds(act, None, coords)
    want = _oracle(act, flat, coords)
    _check(f"{act}_{n}", wide, narrow, want, dict(loss=TOL, grad=TOL))


def test_eight_wave_closure_at_the_trained_state(golden_dir):
    """C2 near convergence (tests/golden/c2_trained.npz: the reference's parameters after 5 000 epochs and one of its
    batches, 64 x 64 points): freshly initialised networks hide errors in the derivative streams."""
    gold = np.load(os.path.join(golden_dir, "c2_trained.npz"))
    coords = [torch.from_numpy(c) for c in gold["coords"]]
    flat, wide, narrow = _both_builds("tanh", gold["params"], coords)
    want = float(gold["loss_f64"]), gold["grad_f64"]
    yard = dict(loss=abs(float(gold["loss_f32"]) - float(gold["loss_f64"])) / float(gold["loss_f64"]),
                grad=rel_l2(gold["grad_f32"], gold["grad_f64"]))
    _check("trained", wide, narrow, want, {k: max(TOL, 2.0 * v) for k, v in yard.items()})
