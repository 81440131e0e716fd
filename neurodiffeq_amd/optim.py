"""Fused Adam for flat network parameters (``ndq_adam_step``, include/ndq.h).

The reference's default optimiser is ``torch.optim.Adam(params)`` stepped once per epoch (solvers.py:182,331-341).
:class:`FusedAdam` IS a ``torch.optim.Adam`` (same hyper-parameters, same ``state_dict`` layout: per-parameter
``step`` / ``exp_avg`` / ``exp_avg_sq``) whose state tensors are views of flat buffers once a solver has bound its
:class:`~neurodiffeq_amd.networks.FlatParams`; ``step()`` then costs one kernel launch per network instead of a
foreach chain.  Parameters that are not bound fall back to the stock implementation."""
import ctypes

import torch

from . import _lib


class FusedAdam(torch.optim.Adam):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        self._bound = []            # [(FlatParams, exp_avg_flat, exp_avg_sq_flat, group)]
        self._bound_ids = set()
        self._steps = {}
        self._dirty_steps = False
        self._theta = None          # scalars of an inverse problem bound to a system's flat [NT] buffers (bind_scalars)

    # pickling / deepcopy (checkpoints: callbacks.py:129-155, solvers_utils.py:281-398): torch serialises defaults,
    # state and param_groups only, so the per-parameter ``step`` tensors are brought up to date first and the
    # binding to a solver's flat buffers -- device pointers -- is dropped; the next solver binds afresh and adopts the
    # moments / step counts from ``state``.
    def __getstate__(self):
        self._sync_step_tensors()
        return super().__getstate__()

    def __setstate__(self, state):
        super().__setstate__(state)
        self._bound, self._bound_ids, self._steps, self._dirty_steps = [], set(), {}, False
        self._theta = None

    def load_state_dict(self, state_dict):
        """Loaded moments / step counts live in fresh tensors: drop the binding, the solver binds again before its next
        native epoch and ``bind`` adopts them."""
        super().load_state_dict(state_dict)
        self._bound, self._bound_ids, self._steps, self._dirty_steps = [], set(), {}, False
        self._theta = None

    def bind(self, flat_params):
        """Adopt the flat buffers of ``flat_params`` (list of FlatParams) for every parameter this optimiser owns."""
        if [id(fp) for fp, *_ in self._bound] == [id(fp) for fp in flat_params]:
            return
        self._sync_step_tensors()              # a re-bind (system rebuilt mid-training) adopts the CURRENT step counts
        group_of = {id(p): g for g in self.param_groups for p in g["params"]}
        self._bound, self._bound_ids = [], set()
        for fp in flat_params:
            groups = {id(group_of.get(id(p))) for p in fp.params}
            if len(groups) != 1 or None in [group_of.get(id(p)) for p in fp.params]:
                continue                        # not (entirely) ours, or split across groups: leave to torch
            group = group_of[id(fp.params[0])]
            m = torch.zeros_like(fp.grad)
            v = torch.zeros_like(fp.grad)
            steps = set()
            for p, off in zip(fp.params, fp._offsets):
                st = self.state[p]
                mv, vv = m[off:off + p.numel()].view(p.shape), v[off:off + p.numel()].view(p.shape)
                if "exp_avg" in st:
                    mv.copy_(st["exp_avg"]); vv.copy_(st["exp_avg_sq"])
                    steps.add(int(st["step"]))
                else:
                    steps.add(0)
                    st["step"] = torch.tensor(0.0, dtype=torch.float32)
                st["exp_avg"], st["exp_avg_sq"] = mv, vv
            if len(steps) != 1:
                continue
            self._steps[id(fp)] = steps.pop()
            self._bound.append((fp, m, v, group))
            self._bound_ids.update(id(p) for p in fp.params)

    def bound(self, fp):
        return any(f is fp and not g.get("amsgrad") and not g.get("maximize") for f, _, _, g in self._bound)

    def fast_slot(self, fp):
        """(exp_avg, exp_avg_sq, group, step AFTER the next update) for the solver's native epoch path, which performs
        the Adam update on the device itself (ndq_epoch_tail); None if ``fp`` is not bound / not eligible."""
        for f, m, v, group in self._bound:
            if f is fp and not group.get("amsgrad") and not group.get("maximize"):
                self._steps[id(fp)] += 1
                self._dirty_steps = True
                return m, v, group, self._steps[id(fp)]
        return None

    def fast_slots(self, fp, k):
        """``fast_slot`` for ``k`` consecutive updates performed by one native call (ndq_fused_fit_run): the step count
        returned is the one AFTER the first of them; the counter advances by ``k``."""
        for f, m, v, group in self._bound:
            if f is fp and not group.get("amsgrad") and not group.get("maximize"):
                first = self._steps[id(fp)] + 1
                self._steps[id(fp)] += k
                self._dirty_steps = True
                return m, v, group, first
        return None

    # ---- trainable scalars of the equations (inverse problems): the same arrangement as bind() for FlatParams.  The system
    # keeps its NT scalars in one device vector; their moments become views of two flat [NT] buffers, so the sums + tail launch of
    # an epoch can step them (include/ndq.h: ndq_theta_step).  Step counts are per scalar and tracked lazily.
    def owns_scalar(self, p):
        """Is ``p`` in a parameter group of this optimiser that the device-side update can serve (no amsgrad / maximize)?"""
        for g in self.param_groups:
            if any(q is p for q in g["params"]):
                return not g.get("amsgrad") and not g.get("maximize")
        return False

    def bind_scalars(self, owner, scalars, n_theta, device):
        """``scalars``: {index in the system's vector: one-element Parameter} -- the trainable ones, all owned by this optimiser
        (``owns_scalar``).  Existing moments / step counts are adopted; entries of the [n_theta] buffers that belong to frozen
        arguments stay zero and are never written.  ``owner``: the object whose vector this is (a re-bind to the same one is free)."""
        th = self._theta
        if th is not None and th["owner"] is owner and all(self.state[p].get("exp_avg") is v for p, v in zip(th["params"], th["mviews"])):
            return
        self._sync_step_tensors()
        m = torch.zeros(n_theta, dtype=torch.float32, device=device)
        v = torch.zeros(n_theta, dtype=torch.float32, device=device)
        idx, params, steps, mviews = [], [], [], []
        for j, p in sorted(scalars.items()):
            st = self.state[p]
            mv, vv = m[j:j + 1].view(p.shape), v[j:j + 1].view(p.shape)
            if "exp_avg" in st:
                mv.copy_(st["exp_avg"]); vv.copy_(st["exp_avg_sq"])
                steps.append(int(st["step"]))
            else:
                steps.append(0)
                st["step"] = torch.tensor(0.0, dtype=torch.float32)
            st["exp_avg"], st["exp_avg_sq"] = mv, vv
            idx.append(j); params.append(p); mviews.append(mv)
        self._theta = dict(owner=owner, m=m, v=v, idx=idx, params=params, steps=steps, mviews=mviews)

    def scalars_bound(self, owner):
        th = self._theta
        return th is not None and th["owner"] is owner

    def theta_slot(self):
        """(exp_avg [NT], exp_avg_sq [NT], [(index, group, step AFTER the next update)] per bound scalar) for the native epoch,
        which updates the scalars on the device; the counters advance.  Hyper-parameters: the scalar's own group, read now."""
        th = self._theta
        group_of = {id(p): g for g in self.param_groups for p in g["params"]}
        out = []
        for i, (j, p) in enumerate(zip(th["idx"], th["params"])):
            th["steps"][i] += 1
            out.append((j, group_of[id(p)], th["steps"][i]))
        self._dirty_steps = True
        return th["m"], th["v"], out

    def _sync_step_tensors(self):
        if getattr(self, "_dirty_steps", False):
            for fp, _, _, _ in self._bound:
                for p in fp.params:
                    self.state[p]["step"].fill_(float(self._steps[id(fp)]))
            th = getattr(self, "_theta", None)
            if th is not None:
                for p, step in zip(th["params"], th["steps"]):
                    self.state[p]["step"].fill_(float(step))
            self._dirty_steps = False

    def state_dict(self):
        self._sync_step_tensors()
        return super().state_dict()

    @torch.no_grad()
    def step(self, closure=None):
        self._sync_step_tensors()
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        fused = set()
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream) if self._bound else None
        for fp, m, v, group in self._bound:
            if not (fp._is_flat() and fp.grads_attached()) or group.get("amsgrad") or group.get("maximize"):
                continue
            self._steps[id(fp)] += 1
            step = self._steps[id(fp)]
            b1, b2 = group["betas"]
            f64 = fp.grad.dtype == torch.float64          # fp64 systems: the same kernel in double (libndq64.so)
            adam = _lib.lib64().ndq64_adam_step if f64 else _lib.lib().ndq_adam_step
            rc = adam(fp.flat.data_ptr(), fp.grad.data_ptr(), m.data_ptr(), v.data_ptr(), fp.numel,
                      float(group["lr"]), b1, b2, group["eps"], group["weight_decay"], step, stream)
            _lib.check(rc, "ndq_adam_step")
            for p in fp.params:
                self.state[p]["step"] += 1
            fused.update(id(p) for p in fp.params)
        if len(fused) < sum(len(g["params"]) for g in self.param_groups):
            # anything not handled above: stock Adam on the remaining parameters
            saved = [g["params"] for g in self.param_groups]
            try:
                for g in self.param_groups:
                    g["params"] = [p for p in g["params"] if id(p) not in fused]
                super().step()
            finally:
                for g, ps in zip(self.param_groups, saved):
                    g["params"] = ps
            th = self._theta
            if th is not None:           # bound scalars stepped by the stock implementation: follow its step counts
                th["steps"] = [int(self.state[p]["step"]) if "step" in self.state[p] else s for p, s in zip(th["params"], th["steps"])]
        return loss
