"""Inverse problems, the end of the epoch on the device -- the parts that need no GPU: the eligibility rule as a pure function,
FusedAdam's binding of the scalars on CPU tensors, and the per-scalar Adam constants the launch is handed."""
import ctypes
import math

import numpy as np
import torch

from neurodiffeq_amd import _lib
from neurodiffeq_amd.engine import theta_tail_eligible, theta_tail_switch
from neurodiffeq_amd.optim import FusedAdam

CPU = torch.device("cpu")


def _scalars():
    return [torch.nn.Parameter(torch.tensor(0.05)), torch.nn.Parameter(torch.tensor(0.8))]


def _eligible(scalars, optimizer, environ=None, **kw):
    args = dict(enabled=theta_tail_switch(environ or {}), f64=False, closure=True, sharded=False, device=CPU, scalars=scalars,
                n_theta=len(scalars), optimizer=optimizer)
    args.update(kw)
    return theta_tail_eligible(**args)


def test_switch_is_on_by_default_and_off_with_the_variable():
    assert theta_tail_switch({}) and theta_tail_switch({"NDQ_NO_THETA_TAIL": "0"})
    assert not theta_tail_switch({"NDQ_NO_THETA_TAIL": "1"})


def test_eligibility_rule():
    net = torch.nn.Linear(1, 1)
    th = _scalars()
    fused = FusedAdam(list(net.parameters()) + th)
    assert _eligible(th, fused)
    # the fallbacks: each keeps the general path
    assert not _eligible(th, torch.optim.Adam(list(net.parameters()) + th))
    assert not _eligible(th, fused, device=torch.device("cuda"))                       # scalars on the CPU, system on the GPU
    assert not _eligible(th, FusedAdam(list(net.parameters()) + th[:1]))              # one scalar missing from the optimiser
    amsgrad = FusedAdam(net.parameters())
    amsgrad.add_param_group(dict(params=th, amsgrad=True))
    assert not _eligible(th, amsgrad)
    assert not _eligible(th, fused, environ={"NDQ_NO_THETA_TAIL": "1"})
    # ... and the other clauses
    assert not _eligible(th, fused, f64=True) and not _eligible(th, fused, closure=False) and not _eligible(th, fused, sharded=True)
    assert not _eligible([], fused, n_theta=1)                                         # frozen arguments only
    assert not _eligible(th, fused, n_theta=_lib.NDQ_THETA_MAX + 1)
    w = torch.nn.Parameter(torch.zeros(2, 2))
    assert not _eligible([(w, 1)], FusedAdam([w]))                                     # entry of a larger tensor
    assert not _eligible([w], FusedAdam([w]))
    d = torch.nn.Parameter(torch.tensor(0.5, dtype=torch.float64))
    assert not _eligible([d], FusedAdam([d]))


def test_fused_adam_binds_scalars_adopting_state_with_torch_adams_layout():
    torch.manual_seed(0)
    th, ref_th = _scalars(), _scalars()
    opt = FusedAdam([dict(params=[th[0]]), dict(params=[th[1]], lr=1e-2, betas=(0.8, 0.9))])
    ref = torch.optim.Adam([dict(params=[ref_th[0]]), dict(params=[ref_th[1]], lr=1e-2, betas=(0.8, 0.9))])
    for o, ps in ((opt, th), (ref, ref_th)):          # two stock steps: state exists before the binding
        for _ in range(2):
            for i, p in enumerate(ps):
                p.grad = torch.tensor(0.3 + i)
            o.step()
    owner = object()
    # a system vector of three arguments: index 1 is a frozen runtime constant, the trainable scalars sit at 0 and 2
    opt.bind_scalars(owner, {0: th[0], 2: th[1]}, 3, CPU)
    assert opt.scalars_bound(owner) and not opt.scalars_bound(object())
    m, v, per = opt.theta_slot()
    assert m.shape == (3,) and [(j, s) for j, _, s in per] == [(0, 3), (2, 3)]
    assert per[0][1]["lr"] == 1e-3 and per[1][1]["lr"] == 1e-2 and per[1][1]["betas"] == (0.8, 0.9)
    for j, p, q in ((0, th[0], ref_th[0]), (2, th[1], ref_th[1])):
        st = opt.state[p]
        assert st["exp_avg"].data_ptr() == m[j:].data_ptr() and st["exp_avg_sq"].data_ptr() == v[j:].data_ptr()    # views
        assert st["exp_avg"].shape == p.shape
        assert torch.equal(st["exp_avg"], ref.state[q]["exp_avg"]) and torch.equal(st["exp_avg_sq"], ref.state[q]["exp_avg_sq"])
    assert m[1] == 0 and v[1] == 0
    # state_dict: torch.optim.Adam's layout, lazily tracked step counts brought up to date (one device-side update was handed out)
    sd, ref_sd = opt.state_dict(), ref.state_dict()
    assert sd["param_groups"] == ref_sd["param_groups"]
    assert sd["state"].keys() == ref_sd["state"].keys()
    for k in sd["state"]:
        assert sd["state"][k].keys() == ref_sd["state"][k].keys()
        assert float(sd["state"][k]["step"]) == 3.0 and float(ref_sd["state"][k]["step"]) == 2.0
        assert sd["state"][k]["exp_avg"].shape == ref_sd["state"][k]["exp_avg"].shape
    # loading drops the binding; the next bind adopts what was loaded
    fresh_th = _scalars()
    fresh = FusedAdam([dict(params=[fresh_th[0]]), dict(params=[fresh_th[1]], lr=1e-2, betas=(0.8, 0.9))])
    fresh.load_state_dict(sd)
    assert not fresh.scalars_bound(owner)
    fresh.bind_scalars(owner, {0: fresh_th[0], 2: fresh_th[1]}, 3, CPU)
    m2, v2, per2 = fresh.theta_slot()
    assert torch.equal(m2, m) and torch.equal(v2, v) and [s for _, _, s in per2] == [4, 4]


def test_per_scalar_constants_are_adam_consts_of_the_scalars_group_and_step():
    L = _lib.lib()
    assert L.ndq_theta_step_bytes() == ctypes.sizeof(_lib.ThetaStep)
    th = _lib.ThetaStep()
    groups = [dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, step=1),
              dict(lr=1e-2, betas=(0.8, 0.9), eps=1e-6, weight_decay=0.01, step=2),
              dict(lr=3e-4, betas=(0.5, 0.99), eps=1e-8, weight_decay=0.0, step=1000)]
    th.n_theta = len(groups)
    for j, g in enumerate(groups):
        th.lr[j], (th.beta1[j], th.beta2[j]), th.eps[j], th.weight_decay[j], th.step[j] = \
            g["lr"], g["betas"], g["eps"], g["weight_decay"], g["step"]
    out = (ctypes.c_float * 7)()
    f32 = lambda x: float(np.float32(x))
    for j, g in enumerate(groups):
        assert L.ndq_theta_step_consts(ctypes.byref(th), j, out) == 0
        b1, b2 = f32(g["betas"][0]), f32(g["betas"][1])
        # adam_consts (csrc/ndq_tail.h): the hyper-parameters as floats, the bias corrections in double, narrowed
        want = [f32(g["lr"]), b1, b2, f32(g["eps"]), f32(g["weight_decay"]), f32(1.0 - b1 ** g["step"]),
                f32(math.sqrt(1.0 - b2 ** g["step"]))]
        assert list(out) == want, (j, list(out), want)
    assert L.ndq_theta_step_consts(ctypes.byref(th), 3, out) != 0
