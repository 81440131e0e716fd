"""Systems with Neumann ends on one-hidden-layer networks of 65 .. 512 units -- 2 .. 4 evaluation sites of fewer networks --
behind ONE closure launch (csrc/ndq_wide.h: wide_multi_closure_kernel / wide_multi_closure_tv_kernel with site traits) on the
GPU: against the fp64 autograd oracle (tests/wide_site_problems.py), the per-site three-kernel pipeline of the same FusedSystem,
the goldens the unmodified reference produced (ws1, ws2) and the composite torch path of the solvers.

Sizes: one lane, one point past a tile, a ragged last tile (every case); several workgroups with a ragged last one (one case
per site count); the first size past one round of the capped grid -- 256 workgroups x 4 waves x 16 points + 1, read from the
module --, where a wave goes round the tile loop again.

Bounds: tests/test_gpu_parity.py's TOL (1e-5, rel-L2 / relative) against the oracle and the goldens; 2e-6 between the closure
launch and the pipeline (tests/test_gpu_wide_multi.py: TOL_MODES); trajectories 2e-5 (loss history) / 1e-5 (parameters)."""
import os
import warnings

import numpy as np
import pytest
import torch

from oracle import autograd_ref as R
from tests import wide_site_problems as SP

pytestmark = pytest.mark.gpu
TOL = 1e-5
TOL_MODES = 2e-6
SIZES = [1, 17, 1000]
MAX_BLOCKS = 256
SECOND_TRIP = MAX_BLOCKS * 4 * 16 + 1      # (asserted against the module's workgroup shape where it is used)


def _matrix():
    out = []
    for name in SP.NAMES:
        sizes = SIZES + ([4097] if name in SP.MORE_BLOCKS else []) + ([SECOND_TRIP] if name in SP.TILE_LOOP else [])
        out += [pytest.param(name, n, id=f"{name}-{n}") for n in sizes]
    return out


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def _grad(nets, flats):
    where = {}
    for fp in flats:
        for prm, off in zip(fp.params, fp._offsets):
            where[id(prm)] = fp.grad[off:off + prm.numel()]
    return [torch.cat([where[id(prm)].reshape(-1) for prm in net.parameters()]).cpu().numpy() for net in nets]


_SYSTEMS, _ORACLE = {}, {}


def _system(name):
    """(nets, closure FusedSystem, pipeline FusedSystem, initial flat parameters, equations), built once per case."""
    from neurodiffeq_amd.engine import FusedSystem
    if name not in _SYSTEMS:
        _SYSTEMS.clear()
        _ORACLE.clear()
        torch.manual_seed(0)
        nets, conds, eqs, nc = SP.make(name)
        flat0 = R.get_flat(nets).clone()
        for net in nets:
            net.to("cuda")
        one = FusedSystem(nets, conds, eqs, nc, "cuda", single_kernel=True)
        three = FusedSystem(nets, conds, eqs, nc, "cuda", single_kernel=False)
        _SYSTEMS[name] = (nets, one, three, flat0, eqs)
    return _SYSTEMS[name]


def _oracle(name, n, seed, flat0, backward=True):
    """fp64 closure of ``SP.batch(name, n, seed)``, computed once per case and batch, never modified."""
    key = (name, n, seed, backward)
    if key not in _ORACLE:
        nets, enf, eqs = SP.make_oracle(name)
        R.set_flat(nets, flat0.double())
        out = R.closure(nets, enf, eqs, [c.double() for c in SP.batch(name, n, seed)], backward=backward)
        grads = [torch.cat([p.grad.reshape(-1) for p in net.parameters()]).numpy().copy() for net in nets] if backward else None
        _ORACLE[key] = dict(loss=out["loss"].item(), grad=grads, funcs=out["funcs"].numpy().T.copy(),
                            resid=out["residuals"].numpy().T.copy(),
                            theta=np.array([p.grad.item() for p in eqs.theta]) if backward else None)
    return _ORACLE[key]


def _step(fs, nets, eqs, coords, n):
    b, m = fs.step(coords, train=True, slot=0, want_funcs=True, want_resid=True)
    fs.attach_theta_grads()
    torch.cuda.synchronize()
    assert m == n
    return b, dict(loss=fs.loss_buf[0].item(), grad=_grad(nets, fs.flat), funcs=b["funcs"][:fs.n_user_funcs, :n].cpu().numpy(),
                   resid=b["resid"][:fs.n_eq, :n].cpu().numpy(), theta=np.array([p.grad.item() for p in eqs.theta]))


def _compare(got, want, tag, errs, pointwise=True):
    errs[f"loss_vs_{tag}"] = abs(got["loss"] - want["loss"]) / abs(want["loss"])
    for k, (g, w) in enumerate(zip(got["grad"], want["grad"])):          # each network's block over that block's own norm
        errs[f"grad{k}_vs_{tag}"] = rel_l2(g, w)
    for j in range(len(want["theta"])):
        errs[f"theta{j}_vs_{tag}"] = float(abs(got["theta"][j] - want["theta"][j]) / np.linalg.norm(want["theta"]))
    if pointwise:
        for k in range(got["funcs"].shape[0]):
            errs[f"funcs{k}_vs_{tag}"] = rel_l2(got["funcs"][k], want["funcs"][k])
        for e in range(got["resid"].shape[0]):
            errs[f"resid{e}_vs_{tag}"] = rel_l2(got["resid"][e], want["resid"][e])


@pytest.mark.parametrize("name,n", _matrix())
def test_closure_launch_matches_oracle_and_pipeline(name, n):
    from neurodiffeq_amd import codegen
    sites = SP.sites(name)
    with warnings.catch_warnings():
        # a closure kernel its first-batch self-check rejects would pass everything below on the pipeline: an error here
        warnings.simplefilter("error", RuntimeWarning)
        nets, one, three, flat0, eqs = _system(name)
        assert one.fusedk is not None and three.fusedk is None
        assert codegen.fuse_mode(one.program, one.descs) == "wide_sites" and one.site_net == sites
        assert one.fusedk.n_nets == len(nets) == SP.n_nets(name) and one.fusedk.threads == 256
        assert one.launches_per_step() == 2 and three.launches_per_step() > 2
        tiles, slots = -(-n // 16), one.fusedk.threads // 64
        if n == SECOND_TRIP:      # the grid is capped and one tile is left over: ONE wave goes round the tile loop again
            assert n == MAX_BLOCKS * slots * 16 + 1 and one.fusedk.blocks(n) == one.fusedk.blocks(n - 1) == MAX_BLOCKS
            assert tiles == slots * MAX_BLOCKS + 1
        else:
            assert tiles <= slots * one.fusedk.blocks(n) and (n < 4097 or one.fusedk.blocks(n) > 1)
        R.set_flat(nets, flat0)
        coords = SP.batch(name, n, 100 + n)
        want = _oracle(name, n, 100 + n, flat0)
        got = {}
        for tag, fs in (("closure", one), ("pipeline", three)):
            b, got[tag] = _step(fs, nets, eqs, coords, n)
            assert (b["fusedk"] is not None) == (tag == "closure")
    assert one.fusedk is not None, getattr(one, "fused_check", None)      # (the first-batch self-check kept the build)
    errs = {}
    _compare(got["closure"], want, "oracle", errs)
    _compare(got["closure"], got["pipeline"], "pipeline", errs, pointwise=False)
    side = {}
    _compare(got["pipeline"], want, "pipeline-oracle", side)              # (printed, not asserted: which side is off if one is)
    print(name, n, errs, side)
    bad = {k: v for k, v in errs.items() if not v < (TOL if k.endswith("_vs_oracle") else TOL_MODES)}
    assert not bad, (bad, side)
    # a second launch on the same inputs: the same bits everywhere
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
    assert one.loss_buf[0].item() == got["closure"]["loss"]
    assert all(np.array_equal(x, y) for x, y in zip(_grad(nets, one.flat), got["closure"]["grad"]))


@pytest.mark.parametrize("name,n", _matrix())
def test_train_and_validation_launch_matches_the_separate_launches(name, n):
    """wide_multi_closure_tv_kernel with site traits: its training workgroups leave the partial rows of the training launch bit
    for bit (one row per workgroup and network: the sites are added in the waves' accumulators), and with them the training
    gradients; its validation workgroups the loss of the forward-only launch."""
    from neurodiffeq_amd.engine import _c_vp, _ptr
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        nets, one, three, flat0, eqs = _system(name)
        R.set_flat(nets, flat0)
        coords = SP.batch(name, n, 100 + n)
        nv = n + 5
        vcoords = SP.batch(name, nv, 900 + n)
        b, _ = one.step(coords, train=True, slot=0)
        torch.cuda.synchronize()
        want_parts = [t.clone() for t in b["fused_partials_all"]]
        want_lp = b["fused_loss_partials"].clone()
        want_grad = [fp.grad.clone() for fp in one.flat]
        vb, _ = one.step(vcoords, train=False, slot=1)
        torch.cuda.synchronize()
    want_vloss = one.loss_buf[1].item()
    fk, stream = b["fusedk"], one._stream()
    assert fk is not None and vb["fusedk"] is fk
    tb, vblocks = fk.blocks(n), fk.blocks(nv)
    assert tb == b["fused_blocks"] == want_lp.numel() and all(t.shape[0] == tb for t in want_parts) and vblocks == vb["fused_blocks"]
    params_pp = (_c_vp * len(one.flat))(*[fp.flat.data_ptr() for fp in one.flat])
    parts = [torch.full_like(t, float("nan")) for t in want_parts]
    lp, vp = torch.full_like(want_lp, float("nan")), torch.full((vblocks,), float("nan"), device="cuda")
    parts_pp = (_c_vp * len(parts))(*[t.data_ptr() for t in parts])
    seed = 1.0 / (float(n) * one.loss_norm)
    if one.n_theta:
        want_tp = b["theta_partials"][:tb].clone()
        b["theta_partials"][:tb].fill_(float("nan"))
        one._bind_theta(b, fk.lib, True)
    rc = fk.lib.ndq_fused_launch_tv(one._coord_ptr(b, 0), b["ld"], n, params_pp, parts_pp, _ptr(lp), seed,
                                    one._coord_ptr(vb, 0), vb["ld"], nv, _ptr(vp), None, stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(lp, want_lp) and all(torch.equal(a, w) for a, w in zip(parts, want_parts))
    assert not one.n_theta or torch.equal(b["theta_partials"][:tb], want_tp)
    # ... and so the training gradients: the same second-stage sum over the same rows
    for fp, part, want in zip(one.flat, parts, want_grad):
        rc = one.L.ndq_reduce_partials(_ptr(part), tb, fp.numel, _ptr(fp.grad), 0, 1.0, stream)
        assert rc == 0
        torch.cuda.synchronize()
        assert torch.equal(fp.grad, want)
    vloss = float(vp.double().sum().item()) / (nv * one.loss_norm)
    oracle = _oracle(name, nv, 900 + n, flat0, backward=False)["loss"]
    errs = dict(vloss_vs_forward_launch=abs(vloss - want_vloss) / abs(want_vloss), vloss_vs_oracle=abs(vloss - oracle) / abs(oracle))
    print(name, n, errs)
    assert errs["vloss_vs_forward_launch"] < TOL_MODES and errs["vloss_vs_oracle"] < TOL, errs


def test_off_switch_keeps_the_pipeline(monkeypatch):
    from neurodiffeq_amd.engine import FusedSystem
    monkeypatch.setenv("NDQ_NO_WIDE_SITE_FUSE", "1")
    torch.manual_seed(0)
    nets, conds, eqs, nc = SP.make(SP.NAMES[0])
    for net in nets:
        net.to("cuda")
    fs = FusedSystem(nets, conds, eqs, nc, "cuda", single_kernel=True)
    assert fs.fusedk is None and fs.launches_per_step() > 2
    assert len({fs.descs[k].key() for k in range(fs.n_sites)}) == 2          # every site on its own stream set


def test_module_over_the_lds_budget_is_dropped_and_the_pipeline_is_right():
    """Three 512-unit networks of three inputs at four sites: the mode is "wide_sites", the module answers 197 120 bytes of LDS
    and engine.FusedSystem drops it without a word; the system then runs the per-site pipeline, checked against the oracle."""
    from neurodiffeq_amd import codegen
    from neurodiffeq_amd.engine import FusedSystem
    torch.manual_seed(0)
    nets, conds, eqs, nc = SP.make_over()
    flat0 = R.get_flat(nets).clone()
    for net in nets:
        net.to("cuda")
    n = 17
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        fs = FusedSystem(nets, conds, eqs, nc, "cuda", single_kernel=True)
        assert codegen.fuse_mode(fs.program, fs.descs) == "wide_sites" and fs.site_net == SP.OVER_SITES
        assert fs.fusedk is None and fs.launches_per_step() > 2
        coords = SP.over_batch(n, 5)
        b, got = _step(fs, nets, eqs, coords, n)
    assert b["fusedk"] is None
    onets, enf, oeqs = SP.make_over_oracle()
    R.set_flat(onets, flat0.double())
    out = R.closure(onets, enf, oeqs, [c.double() for c in coords])
    want = dict(loss=out["loss"].item(), grad=[torch.cat([p.grad.reshape(-1) for p in net.parameters()]).numpy() for net in onets],
                funcs=out["funcs"].numpy().T, resid=out["residuals"].numpy().T, theta=np.zeros(0))
    errs = {}
    _compare(got, want, "oracle", errs)
    print(errs)
    assert max(errs.values()) < TOL, errs


@pytest.mark.parametrize("gname", list(SP.GOLDEN))
def test_reference_goldens_through_the_wide_site_closure(golden_dir, gname):
    """One closure on the reference's own inputs (tests/golden/ws1.npz, ws2.npz, produced by the unmodified reference): function
    values, residuals, loss and flat gradient through the new kernel."""
    from neurodiffeq_amd import codegen
    from neurodiffeq_amd.engine import FusedSystem
    gold = np.load(os.path.join(golden_dir, f"{gname}.npz"))
    torch.manual_seed(0)
    nets, conds, eqs, nc = SP.make(SP.GOLDEN[gname])
    for net in nets:
        net.to("cuda")
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        fs = FusedSystem(nets, conds, eqs, nc, "cuda")
        assert fs.fusedk is not None and codegen.fuse_mode(fs.program, fs.descs) == "wide_sites"
        R.set_flat(nets, gold["params0"])
        b, n = fs.step([torch.from_numpy(c) for c in gold["coords"]], train=True, slot=0, want_funcs=True, want_resid=True)
        torch.cuda.synchronize()
    assert fs.fusedk is not None and b["fusedk"] is not None and n == SP.GOLDEN_POINTS
    grad = np.concatenate([fp.grad.cpu().numpy() for fp in fs.flat])
    errs = dict(funcs=rel_l2(b["funcs"][:, :n].T.cpu().numpy(), gold["funcs_f64"]),
                residuals=rel_l2(b["resid"][:, :n].T.cpu().numpy(), gold["residuals_f64"]),
                loss=abs(fs.loss_buf[0].item() - float(gold["loss_f64"])) / abs(float(gold["loss_f64"])),
                grad=rel_l2(grad, gold["grad_f64"]))
    print(gname, errs)
    assert max(errs.values()) < TOL, errs


@pytest.mark.parametrize("gname", list(SP.GOLDEN))
def test_solver_on_the_fused_path_follows_the_composite_path(gname):
    """Solver2D (heat with two Neumann ends: one 128-unit network, three sites) and Solver1D (the pair of two-point problems:
    two networks, four sites): 25 Adam epochs on the fused path -- one closure launch per epoch -- against the composite torch
    path from the same seed."""
    def run(mode):
        torch.manual_seed(0)
        s, nets = SP.make_solver(SP.GOLDEN[gname])
        s.fused = mode
        torch.manual_seed(7)
        with warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)
            s.fit(25, tqdm_file=None)
        return s, nets
    (a, na), (b, nb) = run("require"), run("off")
    assert a.fused_active and not b.fused_active
    assert a._fused_sys.fusedk is not None and a._fused_sys.launches_per_step() == 2
    ha, hb = np.array(a.metrics_history["train_loss"]), np.array(b.metrics_history["train_loss"])
    assert len(ha) == len(hb) == 25
    errs = dict(loss=float(np.max(np.abs(ha - hb) / np.abs(hb))),
                params=rel_l2(R.get_flat(na).cpu().numpy(), R.get_flat(nb).cpu().numpy()))
    print(gname, errs)
    assert errs["loss"] < 2e-5 and errs["params"] < 1e-5, errs
