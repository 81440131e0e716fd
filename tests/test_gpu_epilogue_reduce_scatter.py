"""The reduce-scatter epilogue of the single-launch closure kernel (csrc/ndq_mlp.h: block_reduce_store_rs,
NDQ_EPILOGUE_RS) keeps every summation tree of the epilogue it replaces: C2's problem (Laplace, DirichletBVP2D, FCNN
2-32-32-1) through the 8-wave build, forced for small batches, and through the 4-wave build, each compiled with the
switch on (the default) and with -DNDQ_EPILOGUE_RS=0 -- loss and the whole gradient must agree to the bit.

A ragged network (20 units per layer) keeps block_reduce_store; its closure must still meet the 1e-5 contract against the
fp64 autograd oracle (tests/test_gpu_parity.py: TOL).
"""
import numpy as np
import pytest
import torch

from oracle import autograd_ref as R

pytestmark = pytest.mark.gpu

TOL = 1e-5
ACTS = {"tanh": torch.nn.Tanh, "sigmoid": torch.nn.Sigmoid}


def _closure(monkeypatch, act, n, eight_waves, rs):
    """(loss, grad) of one closure launch on n points; rs: which epilogue the modules are compiled with."""
    from neurodiffeq_amd.engine import FusedSystem
    from neurodiffeq_amd.networks import FCNN
    from tests import configs
    if rs:
        monkeypatch.delenv("NDQ_JIT_FLAGS", raising=False)
    else:
        monkeypatch.setenv("NDQ_JIT_FLAGS", "-DNDQ_EPILOGUE_RS=0")
    torch.manual_seed(0)
    cfg = configs.make("c2", 8)
    nets = [FCNN(2, 1, hidden_units=(32, 32), actv=ACTS[act]).to("cuda")]
    g = torch.Generator().manual_seed(7)
    coords = [torch.rand(n, generator=g), torch.rand(n, generator=g)]
    fs = FusedSystem(nets, cfg["conds"], configs.fused_equations(cfg), 2, "cuda", single_kernel=True)
    assert fs.fusedk is not None
    if eight_waves:
        fs.WIDE_MIN_POINTS = 0
        fs.prefers_wide = lambda n: True
    else:
        fs.fusedk_wide = False
    b, _ = fs.step(coords, train=True, slot=0)
    torch.cuda.synchronize()
    assert b["fusedk"].threads == (512 if eight_waves else 256), b["fusedk"].threads
    assert fs.fused_check["reproducible"], fs.fused_check
    return np.float32(fs.loss_buf[0].item()), fs.flat[0].grad.cpu().numpy().copy()


# 1 point: seven waves deposit zeros.  17: two waves, a partial tile.  16 * 8 + 5: every wave of a workgroup busy, one
# ragged tile.  32 773: many workgroups, second-stage sums.  sigmoid: a second Act<>.
@pytest.mark.parametrize("eight_waves", [True, False], ids=["8wave", "4wave"])
@pytest.mark.parametrize("act,n", [("tanh", 1), ("tanh", 17), ("tanh", 16 * 8 + 5), ("tanh", 32773), ("sigmoid", 16 * 8 + 5)])
def test_epilogue_switch_on_and_off_agree_to_the_bit(monkeypatch, act, n, eight_waves):
    loss1, grad1 = _closure(monkeypatch, act, n, eight_waves, True)
    loss0, grad0 = _closure(monkeypatch, act, n, eight_waves, False)
    diff = np.flatnonzero(grad1.view(np.uint32) != grad0.view(np.uint32))
    print(f"{act} n={n} eight_waves={eight_waves}: loss {loss1!r} / {loss0!r}, {diff.size} of {grad1.size} gradient entries differ",
          flush=True)
    assert np.isfinite(grad1).all() and np.abs(grad1).max() > 0
    assert loss1.view(np.uint32) == loss0.view(np.uint32), (loss1, loss0)
    assert diff.size == 0, (diff[:16], grad1[diff[:16]], grad0[diff[:16]])


def test_ragged_network_keeps_the_old_epilogue_and_its_bound():
    from neurodiffeq_amd.engine import FusedSystem
    from tests import zoo
    torch.manual_seed(11)
    system = zoo.build("shape_20x3")
    nets, conds, pde = system.product()
    flat = R.get_flat(nets)
    coords = system.sample(16 * 8 + 5, seed=5)
    onets, enforcers, opde = system.oracle(flat)
    want = R.closure(onets, enforcers, opde, coords)
    want_grad = R.get_flat_grad(onets).numpy()
    for net in nets:
        net.to("cuda")
    fs = FusedSystem(nets, conds, pde, system.n_coords, "cuda")
    assert fs.fusedk is not None
    fs.step([c.float() for c in coords], train=True, slot=0)
    torch.cuda.synchronize()
    assert fs.fused_check["reproducible"], fs.fused_check
    got = np.concatenate([fp.grad.cpu().numpy() for fp in fs.flat])
    errs = dict(loss=abs(fs.loss_buf[0].item() - want["loss"].item()) / abs(want["loss"].item()),
                grad=float(np.linalg.norm(got - want_grad) / np.linalg.norm(want_grad)))
    print("shape_20x3", errs, flush=True)
    assert max(errs.values()) < TOL, errs
