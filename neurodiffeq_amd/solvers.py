"""Solvers with the reference's public surface (neurodiffeq/solvers.py): ``BaseSolver`` / ``Solver1D`` /
``Solver2D`` / ``GenericSolver``, ``fit`` / ``run_train_epoch`` / ``run_valid_epoch`` / ``get_solution`` /
``get_residuals`` / ``get_internals``, the hooks ``compute_func_val`` / ``additional_loss`` /
``_do_optimizer_step`` and the ``metrics_history`` / ``best_nets`` / ``lowest_loss`` bookkeeping that callbacks read.

The epoch control flow is the reference's (``_run_epoch``, solvers.py:343-424: zero_grad once, accumulate gradients
over ``n_batches`` generator draws, one optimizer step, history, best-network snapshot).  What differs is the
per-batch compute:

* **fused path** (nets on an MI355X, FCNN nets the kernels support, default / ``'l2'`` loss): the closure is the
  launch sequence of :class:`neurodiffeq_amd.engine.FusedSystem`; nothing is synchronised until the epoch's loss is
  read once.  A missing/broken ``libndq.so`` raises -- it is never papered over.
* **composite path**: the reference's closure on torch autograd, for everything outside the fused scope (custom
  loss functions / ``additional_loss`` overrides, closure optimisers such as LBFGS, Neumann ``IBVP1D``, non-FCNN
  networks, fp64, or a host without a GPU).
"""
import inspect
import sys
import warnings
from abc import ABC, abstractmethod
from copy import deepcopy
from itertools import chain

import torch
import torch.nn as nn

from . import _lib
from .conditions import BaseCondition
from .generators import (Generator1D, Generator2D, GeneratorSpherical, SamplerGenerator, draws_are_static,
                         draws_have_fixed_size, device_source, on_default_device)
from . import autograd_ops
from .losses import _losses
from .networks import FCNN, describe
from .neurodiffeq import safe_diff as diff
from .optim import FusedAdam
from .symbolic import MetricTraceUnsupported, TraceUnsupported, captured_unchanged
from .networks import STRUCTURE as _net_structure
import os as _os
_QUICK_KEY = _os.environ.get("NDQ_QUICK_KEY", "1") != "0"        # (A/B switch of the per-epoch identity check in _fused_system)
_LC = []


def _library_code():
    """engine.library_code, imported once (engine imports this module's siblings: a function-level `from .engine import` costs
    half a microsecond of importlib bookkeeping per epoch)."""
    if not _LC:
        from .engine import library_code
        _LC.append(library_code)
    return _LC[0]


_CLOSURE_CACHE = {}


def _requires_closure(optimizer):
    """True for optimisers whose ``step`` needs a closure (LBFGS-style, solvers.py:29-32); cached per optimiser class
    because ``inspect.signature`` costs more than a whole fused training epoch."""
    cls = type(optimizer)
    r = _CLOSURE_CACHE.get(cls)
    if r is None:
        p = inspect.signature(optimizer.step).parameters.get("closure")
        r = _CLOSURE_CACHE[cls] = bool(p) and p.default == inspect._empty
    return r


def _unique_params(nets):
    seen, out = set(), []
    for p in chain.from_iterable(n.parameters() for n in nets):
        if id(p) not in seen:
            seen.add(id(p))
            out.append(p)
    return out


def sobolev_equations(diff_eqs, n_funcs, semi=False):
    """The Sobolev norms of the reference (losses.py:17-26) are the mean square over the columns
    [r_1 .. r_neq, d(sum_e r_e)/dx_1 .. d(sum_e r_e)/dx_d] (``semi``: the derivative columns alone), i.e. the l2 loss
    of this extended residual list.  It traces only when the extra derivative stays within second-order network
    streams (first-order systems); otherwise the tracer raises and the composite path takes over."""
    def extended(*variables):
        res = list(diff_eqs(*variables))
        total = res[0]
        for r in res[1:]:
            total = total + r
        grads = [diff(total, x) for x in variables[n_funcs:]]
        return grads if semi else res + grads
    return extended


def _default_l2(residual, funcs, coords):
    return (residual ** 2).mean()


class BaseSolver(ABC):
    #: epochs between UNCONDITIONAL re-traces of diff_eqs / the conditions (program.eq_probe).  Every epoch a StateWatch
    #: compares the Python state those callables can reach (closure cells, globals they name, condition attributes ...)
    #: with what it was at trace time -- a few comparisons -- and re-traces at once when something moved; this period only
    #: bounds how long state the watch cannot see (fetched through foreign code) could stay frozen.  fit() without
    #: callbacks re-traces at every chunk boundary as well.
    EQ_PROBE_EVERY = 1024
    LOSS_PROBE_EVERY = 1        # epochs between re-probes of a traced custom loss (see _fused_system): every epoch -- a probe
    #                             is one Python re-trace of the callable on a hash-consed graph, and a loss that follows
    #                             solver state (a penalty switched on at epoch N) must never train on a stale kernel

    """See the module docstring; constructor arguments are the reference's (solvers.py:36-140)."""

    #: 'auto' -> fused when possible, composite otherwise (with a warning on a GPU); 'require' -> raise if the fused
    #: path cannot be used; 'off' -> always composite.
    fused = "auto"

    def __init__(self, diff_eqs, conditions, nets=None, train_generator=None, valid_generator=None,
                 analytic_solutions=None, optimizer=None, loss_fn=None, n_batches_train=1, n_batches_valid=4,
                 metrics=None, n_input_units=None, n_output_units=None, shuffle=None, batch_size=None,
                 criterion=None):
        attrs_of_the_subclass = frozenset(self.__dict__)       # set before super().__init__(): possibly equation state
        if criterion is not None:
            warnings.warn("`criterion` is deprecated; use `loss_fn`", FutureWarning)
            loss_fn = criterion if loss_fn is None else loss_fn
        if shuffle:
            warnings.warn("param `shuffle` is deprecated and ignored; shuffling should be performed by generators",
                          FutureWarning)
        if batch_size is not None:
            warnings.warn("param `batch_size` is deprecated and ignored; specify n_batches_train and "
                          "n_batches_valid instead", FutureWarning)
        self.diff_eqs = diff_eqs
        self.conditions = conditions
        self.n_funcs = len(conditions)
        if nets is None:
            self.nets = [FCNN(n_input_units=n_input_units, n_output_units=n_output_units, hidden_units=(32, 32),
                              actv=nn.Tanh) for _ in range(self.n_funcs)]
        else:
            self.nets = nets
        if train_generator is None:
            raise ValueError("train_generator must be specified")
        if valid_generator is None:
            raise ValueError("valid_generator must be specified")

        # the reference runs on "cuda if available" (its import selects it, README FAQ); same here for the networks
        self.device = torch.device("cuda") if torch.cuda.is_available() else torch.device("cpu")
        if self.device.type == "cuda":
            for n in self.nets:
                n.to(self.device)

        self.metrics_fn = metrics if metrics else {}
        if analytic_solutions:
            warnings.warn("The `analytic_solutions` argument is deprecated and could lead to unstable behavior. "
                          "Pass a `metrics` dict instead.", FutureWarning)

            def analytic_mse(*args):
                x = args[-n_input_units:]
                u_hat = analytic_solutions(*x)
                u = args[:-n_input_units]
                u, u_hat = torch.stack(u), torch.stack(u_hat)
                return ((u - u_hat) ** 2).mean()

            if "analytic_mse" in self.metrics_fn:
                warnings.warn("Ignoring `analytic_solutions` in presence of key 'analytic_mse' in `metrics`",
                              FutureWarning)
            else:
                self.metrics_fn["analytic_mse"] = analytic_mse

        self._history = {"train_loss": [], "valid_loss": []}
        self._history.update({"train__" + name: [] for name in self.metrics_fn})
        self._history.update({"valid__" + name: [] for name in self.metrics_fn})

        self.optimizer = optimizer if optimizer else FusedAdam(_unique_params(self.nets))
        self._set_loss_fn(loss_fn)
        # (the reference samples on torch's default device, generators.py:152,264: under a cuda default device the noise of
        # the grid / spherical generators is drawn on the MI355X -- generators.on_default_device)
        self.generator = {"train": SamplerGenerator(on_default_device(train_generator)),
                          "valid": SamplerGenerator(on_default_device(valid_generator))}
        self.n_batches = {"train": n_batches_train, "valid": n_batches_valid}
        self._batch = {"train": None, "valid": None}
        if self.n_batches["valid"] == 0 and _requires_closure(self.optimizer):
            warnings.warn(f"Setting n_batches_valid=0 will update lowest_loss and best_net with training loss "
                          f"instead of validation loss. This is a problem for {self.optimizer.__class__} optimizer "
                          f"because it updates the parameters before the training loss computed. "
                          f"This leads to potentially worse solution in `best_net`!", RuntimeWarning)
        self._best_nets = None
        self._best_flat = None          # device snapshots of the flat parameters (fused path)
        self._lowest_loss = None
        self.local_epoch = 0
        self._max_local_epoch = 0
        self._stop_training = False
        self._phase = None
        self._fused_sys = None
        self._composite_plain = False   # composite path: plain torch forwards (set when an equation needs order > 2)
        self._loss_probe_count = 0
        self._loss_time_dependent = False
        self._eq_watch = None                  # _pystate.StateWatch over what diff_eqs / the conditions can read
        self._eq_probe_countdown = 1           # epochs until the next unconditional re-trace (second use, then EQ_PROBE_EVERY)
        self._fused_key = None
        self._metrics_follow_state = False     # a traced metric changed between epochs: metrics on the host from then on
        self._fused_quick = None               # what _fused_key was made of, object by object (the per-epoch identity check)
        self._fused_quick_parts = None
        self._fast_tracks_best = False
        self.dist = None                # optional neurodiffeq_amd.parallel.BatchSharding
        # the solver's own bookkeeping attributes: not equation state when diff_eqs is a bound method (_pystate.StateWatch)
        self._own_attrs = (frozenset(self.__dict__) - attrs_of_the_subclass) | {"_own_attrs", "_best_nets_from_device", "_dtype_probe", "_eq_watch_warned", "_lc", "_volatile",
                                                       "_eval_key", "_eval_sys", "_host_metrics", "_resid_key", "_resid_sys", "_autocast_warned"}

    # ------------------------------------------------------------------------------------------ loss function
    def _set_loss_fn(self, criterion):
        if criterion is None:
            self.loss_fn = _default_l2
        elif isinstance(criterion, nn.modules.loss._Loss):
            self.loss_fn = lambda r, f, x: criterion(r, torch.zeros_like(r))
        elif isinstance(criterion, str):
            self.loss_fn = _losses[criterion.lower()]
        elif callable(criterion):
            self.loss_fn = criterion
        else:
            raise TypeError(f"Unknown type of criterion {type(criterion)}")

    # ------------------------------------------------------------------------------------------ small properties
    @property
    def metrics_history(self):
        """Dict of history lists (solvers.py:174-180).  On the native fast path epoch losses are recorded on the
        device; reading this property (callbacks, user code, ``fit``'s end) pulls them over in one copy."""
        self._flush_device_history()
        return self._history

    @metrics_history.setter
    def metrics_history(self, value):
        self._flush_device_history()
        self._history = value

    @property
    def lowest_loss(self):
        self._flush_device_history()
        return self._lowest_loss

    @lowest_loss.setter
    def lowest_loss(self, value):
        self._flush_device_history()
        self._lowest_loss = value
        if self._fused_sys is not None and getattr(self._fused_sys, "_fast", None) is not None:
            self._fused_sys._fast["best_loss"].fill_(float("inf") if value is None else float(value))

    def _flush_device_history(self):
        system = self._fused_sys
        fs = getattr(system, "_fast", None) if system is not None else None
        if fs is None or (fs["pending"] == 0 and fs["pending_valid"] == 0):
            return
        losses, vlosses, best = system.fast_flush()
        if self.dist is not None:
            self.dist.check()       # a data-parallel exchange that gave up on a peer is an error, not a statistic
        self._history["train_loss"].extend(losses)
        self._history["valid_loss"].extend(vlosses)
        if best < float("inf") and (self._lowest_loss is None or best < self._lowest_loss):
            self._lowest_loss = best
            self._best_flat = list(fs["best_flat"])            # device snapshots written by ndq_epoch_tail
            self._best_nets = None

    @property
    def global_epoch(self):
        pending = 0
        if self._fused_sys is not None and getattr(self._fused_sys, "_fast", None) is not None:
            pending = self._fused_sys._fast["pending"]
        return len(self._history["train_loss"]) + pending

    @property
    def batch(self):
        return self._batch

    @property
    def _batch_examples(self):
        warnings.warn("`._batch_examples` has been deprecated in favor of `._batch` and will be removed in a future "
                      "version", FutureWarning)
        return self._batch

    @property
    def criterion(self):
        warnings.warn(f"`{self.__class__.__name__}`.criterion is a deprecated alias for `.loss_fn`")
        return self.loss_fn

    @criterion.setter
    def criterion(self, loss_fn):
        warnings.warn(f"`{self.__class__.__name__}`.criterion is a deprecated alias for `.loss_fn`")
        self.loss_fn = loss_fn

    @property
    def best_nets(self):
        """Networks of the epoch with the lowest loss (solvers.py:434-441).  On the fused path the snapshot is a flat
        device copy taken without a host round trip; module copies are materialised on first access."""
        self._flush_device_history()
        if self._best_flat is not None:
            nets = deepcopy(self.nets)
            # one snapshot per DISTINCT module, in first-appearance order (engine.trace_system: a module shared by several
            # functions -- nets = [A, A, B] -- is one parameter set; deepcopy keeps the sharing)
            distinct = []
            for n in nets:
                if not any(n is m for m in distinct):
                    distinct.append(n)
            with torch.no_grad():
                for net, flat in zip(distinct, self._best_flat):
                    off = 0
                    for p in describe(net, dtype=flat.dtype)["params"]:      # the flat vector's order (networks.FlatParams)
                        p.copy_(flat[off:off + p.numel()].view(p.shape))
                        off += p.numel()
            self._best_nets = nets
            self._best_flat = None
            self._best_nets_from_device = True
        return self._best_nets

    @best_nets.setter
    def best_nets(self, nets):
        self._best_nets, self._best_flat = nets, None

    # ------------------------------------------------------------------------------------------ hooks
    def compute_func_val(self, net, cond, *coordinates):
        return cond.enforce(net, *coordinates)

    def additional_loss(self, residual, funcs, coords):
        return 0.0

    def _do_optimizer_step(self, closure=None):
        if closure is None:
            self.optimizer.step()
        else:
            self.optimizer.step(closure=closure)

    # ------------------------------------------------------------------------------------------ history
    def _update_history(self, value, metric_type, key):
        self._phase = key
        self._flush_device_history()
        if metric_type == "loss":
            self._history[f"{key}_{metric_type}"].append(value)
        elif metric_type in self.metrics_fn:
            self._history[f"{key}__{metric_type}"].append(value)
        else:
            raise KeyError(f"metric '{metric_type}' not specified")

    def _update_train_history(self, value, metric_type):
        self._update_history(value, metric_type, key="train")

    def _update_valid_history(self, value, metric_type):
        self._update_history(value, metric_type, key="valid")

    def _generate_batch(self, key):
        self._phase = key
        ex = self.generator[key].get_examples()
        if not (len(ex) and ex[0].dim() == 2 and ex[0].shape[1] == 1):
            ex = [v.reshape(-1, 1) for v in ex]
        self._batch[key] = ex
        return ex

    def _generate_train_batch(self):
        return self._generate_batch("train")

    def _generate_valid_batch(self):
        return self._generate_batch("valid")

    # ------------------------------------------------------------------------------------------ fused system
    def _fused_system_key(self, cfv):
        """(key, reason, loss_kind, working dtype) of the fused system the solver's current objects ask for."""
        reason = None
        loss_kind = "l2" if self.loss_fn is _default_l2 else \
            next((k for k in ("l2", "l1", "infinity", "h1", "h1 semi") if self.loss_fn is _losses[k]), None)
        extra_loss = type(self).additional_loss is not BaseSolver.additional_loss
        if loss_kind is None or extra_loss:
            # a user loss_fn (solvers.py:216-226) and / or an additional_loss override (:587-604): traced together as
            # ONE callable -> the per-point term of a batch mean (symbolic.SymScalar); anything it does that is not
            # linear in batch means of per-point expressions raises TraceUnsupported -> composite path
            if loss_kind in ("h1", "h1 semi"):
                reason = "additional_loss override together with a Sobolev loss"
            loss_kind = "custom"
        if _requires_closure(self.optimizer) and self.dist is not None:
            reason = "closure-based optimizer under data parallelism"
        # working precision = the networks' (fp64 is the reference's default, neurodiffeq/__init__.py:22: such systems run
        # the three-kernel pipeline on the fp64 build of the stream kernels)
        # (first parameter of every network: this runs every epoch; describe() checks the rest when the system is built)
        # (nn.Module.parameters() walks the module tree: ~3 us per network and epoch; the first parameter of every network
        # is looked up once per set of network objects)
        net_ids = tuple(id(n) for n in self.nets)
        probe = self.__dict__.get("_dtype_probe")
        if probe is None or probe[0] != net_ids:
            probe = self._dtype_probe = (net_ids, [p for p in (next(iter(n.parameters()), None) for n in self.nets) if p is not None])
        dtypes = {p.dtype for p in probe[1]}
        sys_dtype = torch.float64 if dtypes == {torch.float64} else torch.float32
        # (fp64 under data parallelism: the per-batch launch sequence in double on every rank's shard, one all-reduce of the
        # [gradient | loss] vector in double through torch.distributed, the device-side tail in double -- parallel.py)
        if self._loss_time_dependent:
            reason = "epoch-dependent loss function"
        # (STRUCTURE[0]: bumped by a layer / parameter / hook set on any network the kernels serve -- networks.track_structure)
        key = (id(self.diff_eqs), net_ids, tuple(id(c) for c in self.conditions),
               cfv, reason, loss_kind, sys_dtype,
               id(self.loss_fn) if loss_kind == "custom" else None,
               tuple((name, id(fn)) for name, fn in self.metrics_fn.items()), _net_structure[0])
        self._fused_quick_parts = (self.diff_eqs, list(self.nets), list(self.conditions), cfv, self.loss_fn, self.optimizer,
                                   dict(self.metrics_fn), _net_structure[0], self._loss_time_dependent, self.dist, type(self),
                                   [(p, p.dtype) for p in probe[1]])
        return key, reason, loss_kind, sys_dtype

    def _fused_system(self, n_coords):
        """The compiled fused step for the current (diff_eqs, nets, conditions, loss), or None -> composite path.
        Re-keyed every epoch because callbacks may swap any of these between epochs (solvers.py:496-497)."""
        if self.fused == "off" or self.device.type != "cuda":
            if self.fused == "require":
                raise _lib.NdqError("fused='require' but no MI355X is visible")
            return None
        if torch.is_autocast_enabled():
            # `with torch.autocast("cuda"): solver.fit(...)`: the reference's linear layers then run in half precision and its
            # results carry that (1e-3); the kernels have one precision.  The reference's closure it is, said once
            if self.fused == "require":
                raise _lib.NdqError("fused='require' but torch.autocast is enabled: the fused kernels do not change precision with it")
            if not self.__dict__.get("_autocast_warned"):
                self._autocast_warned = True
                warnings.warn("neurodiffeq_amd: torch.autocast is enabled; this solver runs the reference's closure on torch autograd "
                              "while it is (the fused MI355X kernels compute in the networks' own precision).", RuntimeWarning)
            self._flush_device_history()
            return None
        # (this runs every epoch and the host is the bottleneck of the headline step: when every OBJECT the key below is made of
        # is the one it was made of last time, the key is last time's -- one chain of identity comparisons instead of five
        # generator expressions)
        q = self.__dict__.get("_fused_quick") if _QUICK_KEY else None
        cfv = getattr(self.compute_func_val, "__func__", self.compute_func_val)
        if q is not None and self.diff_eqs is q[0] and self.nets == q[1] and self.conditions == q[2] and cfv is q[3] \
                and self.loss_fn is q[4] and self.optimizer is q[5] and self.metrics_fn == q[6] and _net_structure[0] == q[7] \
                and self._loss_time_dependent is q[8] and self.dist is q[9] and type(self) is q[10] and self._fused_key is q[11] \
                and all(p.dtype is dt for p, dt in q[12]):
            key = q[11]
            reason, loss_kind, sys_dtype = key[4], key[5], key[6]
        else:
            key, reason, loss_kind, sys_dtype = self._fused_system_key(cfv)
            self._fused_quick = None
            if key == self._fused_key:
                key = self._fused_key            # (the same system as last epoch: from the next epoch on the quick check serves it)
                parts = self._fused_quick_parts
                self._fused_quick = parts[:11] + (key, parts[11])
        if key == self._fused_key and self._fused_sys is not None and \
                not all(fp.all_trainable() and (not fp.act_state or fp.act_unchanged()) for fp in self._fused_sys.flat):
            self._flush_device_history()
            self._fused_key = None              # a layer frozen by a callback (describe() sends the system to the composite path) / a number
            #                                     of an activation module changed (Swish.beta, ELU.alpha: rebuilt for the new value, or left)
        if key == self._fused_key and self._fused_sys is not None and not self._equations_unchanged(self._fused_sys):
            # the callables compute something else now: rebuild below (cached by source) -- with the outside numbers that
            # moved since the compiled trace as RUNTIME constants (symbolic.Graph.external): a coefficient ramped every epoch
            # costs one rebuild, not one per value
            self._note_volatile(self._fused_sys)
            self._fused_key = None
        if key == self._fused_key:
            sysm = self._fused_sys
            # scalar tensors captured by the equations are constants of the generated kernel: re-trace when one of them
            # was modified in place since (callbacks annealing a coefficient between epochs)
            if sysm is not None and not captured_unchanged(sysm.program.g):
                if self._equations_unchanged(sysm, force=True):
                    # same program: every tensor that moved is a runtime constant by now and the re-trace refreshed its value
                    sysm.program.g.captured[:] = [(t, t._version, t.item()) for t, _, _ in sysm.program.g.captured]
                else:
                    self._note_volatile(sysm)
            if sysm is None or captured_unchanged(sysm.program.g):
                # a traced loss_fn / additional_loss is frozen into the generated kernel; callables that follow solver
                # state (a penalty weight annealed with self.global_epoch, ...) are re-probed on their second use and
                # then every LOSS_PROBE_EVERY epochs: if they now trace to a different term, the solver leaves the fused
                # path (loudly) rather than train on a stale loss
                # traced metrics are per-point terms of the same kernels: re-probed every epoch they are evaluated (a solver
                # with metrics synchronises every epoch anyway); one that follows Python state is evaluated on the host from
                # then on, as the reference does it (solvers.py:377-379) -- training stays fused
                mprobe = getattr(sysm.program, "metric_probe", None) if sysm is not None else None
                if mprobe is not None:
                    try:
                        same = mprobe()
                    except Exception:       # noqa: BLE001
                        same = False
                    if not same:
                        self._metrics_follow_state = True
                        self._flush_device_history()
                        self._fused_key = None
                        return self._fused_system(n_coords)
                probe = getattr(sysm.program, "loss_probe", None) if sysm is not None else None
                if probe is None:
                    return sysm
                self._loss_probe_count += 1
                if self._loss_probe_count != 1 and self._loss_probe_count % self.LOSS_PROBE_EVERY:
                    return sysm
                try:
                    same = probe()
                except Exception:       # noqa: BLE001 -- whatever the callable does now, it is not what was compiled
                    same = False
                if same:
                    return sysm
                self._flush_device_history()     # epochs the native path still holds on the device belong to the history
                self._fused_key, self._fused_sys = key, None
                reason = ("the loss function / additional_loss changed between epochs (it depends on solver or Python state, "
                          "which a traced kernel freezes)")
                if self.fused == "require":
                    raise _lib.NdqError(f"fused='require' but the system is outside the fused path: {reason}")
                warnings.warn(f"neurodiffeq_amd: this solver is NOT on the fused MI355X path any more ({reason}); it runs "
                              "the reference's closure on torch autograd instead.", RuntimeWarning)
                self._loss_time_dependent = True
                return None
        self._flush_device_history()
        self._fused_key, self._fused_sys = key, None
        if reason is None:
            try:
                from .engine import FusedSystem
                eqs, kind = self.diff_eqs, loss_kind
                if loss_kind in ("h1", "h1 semi"):
                    eqs, kind = sobolev_equations(self.diff_eqs, len(self.nets), semi=(loss_kind == "h1 semi")), "l2"
                elif loss_kind == "custom":
                    kind = lambda r, f, x: self.loss_fn(r, f, x) + self.additional_loss(r, f, x)
                self._host_metrics = False
                try:
                    if self._metrics_follow_state and self.metrics_fn:
                        raise MetricTraceUnsupported("a metric reads Python state that changes between epochs")
                    self._fused_sys = FusedSystem(self.nets, self.conditions, eqs, n_coords, self.device,
                                                  compute_func_val=self.compute_func_val, loss=kind,
                                                  metrics=list(self.metrics_fn.values()), dtype=sys_dtype,
                                                  volatile=self._volatile_for(key))
                except MetricTraceUnsupported:
                    # metrics are observers: training stays fused, the metrics are evaluated on the host from the
                    # function values of every batch (not under data parallelism: a shard's metric is not the batch's)
                    if self.dist is not None:
                        raise
                    self._fused_sys = FusedSystem(self.nets, self.conditions, eqs, n_coords, self.device,
                                                  compute_func_val=self.compute_func_val, loss=kind, metrics=(),
                                                  dtype=sys_dtype, volatile=self._volatile_for(key))
                    self._host_metrics = True
                self._watch_equations()
                self._refuse_self_mutating_equations()
                if isinstance(self.optimizer, FusedAdam):
                    self.optimizer.bind(self._fused_sys.flat)
            except TraceUnsupported as e:
                reason = str(e)
            except _lib.NdqError:
                raise
            except Exception as e:       # user code that does something a traced column cannot (tensor methods, ...)
                if self.fused == "require":
                    raise
                reason = f"tracing the equations failed with {type(e).__name__}: {e}"
        if self._fused_sys is None:
            if self.fused == "require":
                raise _lib.NdqError(f"fused='require' but the system is outside the fused path: {reason}")
            warnings.warn(f"neurodiffeq_amd: this solver is NOT on the fused MI355X path ({reason}); it runs the "
                          "reference's closure on torch autograd instead -- same results, typically 10-100x slower per "
                          "step.  Pass fused='require' to make this an error.", RuntimeWarning)
        return self._fused_sys

    def _note_volatile(self, sysm):
        """``sysm`` no longer computes what the callables do: remember which outside numbers moved, for the rebuild."""
        suggest = getattr(sysm.program, "suggest_volatile", None)
        if suggest is not None and self._fused_key is not None:
            self._volatile = (self._fused_key[:4], suggest())

    def _volatile_for(self, key):
        """Positions of outside numbers the next trace of these callables takes as runtime constants (engine.trace_system)."""
        held = self.__dict__.get("_volatile")
        return held[1] if held is not None and held[0] == key[:4] else frozenset()

    def _watch_equations(self):
        """Remember the Python state diff_eqs / the conditions / compute_func_val can read (solvers.py:380 re-evaluates them
        every batch; the traced kernels froze it)."""
        self._eq_watch = self._new_state_watch()
        self._eq_probe_countdown = 1

    def _refuse_self_mutating_equations(self):
        """Callables that CHANGE the state they read whenever they run -- a call counter (``eq.calls += 1``), a list they append
        to, ``next()`` on something -- compute something else at every evaluation, and the reference evaluates them once per
        batch (solvers.py:380).  A traced kernel evaluates them never again, a re-trace per epoch not as often as the reference
        does: only the reference's own closure is faithful.  Found by running them once more (``eq_probe``) right after the
        watch was taken: a watch that is dirty after that was dirtied by the callables themselves."""
        watch, sysm = self._eq_watch, self._fused_sys
        probe = getattr(sysm.program, "eq_probe", None) if sysm is not None else None
        if watch is None or probe is None or len(watch) == 0:
            return
        try:
            probe()
        except Exception:       # noqa: BLE001 -- a callable that fails on its second evaluation is not one to trace either
            pass
        if watch.dirty():
            self._fused_sys, self._eq_watch = None, None
            raise TraceUnsupported("the equations / conditions change the Python state they read every time they are evaluated "
                                   "(a call counter, a list they append to, ...); only the reference's own closure evaluates "
                                   "them as often as the reference does")

    def _equations_unchanged(self, sysm, force=False):
        """False: the user's equations / conditions now trace to something else than the kernels of ``sysm`` were compiled
        from (a Python float, dict entry or attribute they read was changed, e.g. by a callback).  The cheap state watch
        runs every call; the re-trace when the watch is dirty, on the second use, every EQ_PROBE_EVERY calls, on ``force``
        (chunk boundaries of the multi-epoch fit path) -- and on EVERY call when the watch is incomplete (the walk met state
        it cannot stamp, _pystate.StateWatch: fail-closed, the reference re-evaluates every batch, solvers.py:380)."""
        watch = self._eq_watch
        dirty = watch is None or watch.dirty()
        blind = watch is not None and not watch.complete
        self._eq_probe_countdown -= 1
        if not (dirty or blind or force or self._eq_probe_countdown <= 0):
            return True                       # (the per-epoch cost: one compiled chain of comparisons, _pystate.StateWatch)
        probe = getattr(sysm.program, "eq_probe", None)
        if probe is None:
            return True
        if blind and not self.__dict__.get("_eq_watch_warned"):
            self._eq_watch_warned = True
            warnings.warn("neurodiffeq_amd: the equations / conditions read state that cannot be compared between epochs ("
                          + "; ".join(watch.incomplete) + "). They are re-traced every epoch instead (about 0.1 - 0.7 ms of host "
                          "time per epoch) and fit() runs epoch by epoch; results are unaffected.", RuntimeWarning)
        if self._eq_probe_countdown <= 0:
            self._eq_probe_countdown = self.EQ_PROBE_EVERY
        same = probe()
        if dirty:
            self._watch_equations_refresh()
        return same

    def _eq_watch_blocks_chunks(self):
        """The multi-epoch native call runs K epochs with no Python in between: only when everything the equations can read
        is stamped (a complete watch) is "nothing ran, nothing changed" a safe conclusion."""
        return self._eq_watch is None or not self._eq_watch.complete

    def _watch_equations_refresh(self):
        countdown = self._eq_probe_countdown
        self._eq_watch = self._new_state_watch()
        self._eq_probe_countdown = countdown

    def _new_state_watch(self):
        from ._pystate import StateWatch
        try:
            return StateWatch([self.diff_eqs, self.compute_func_val] + list(self.conditions), skip_modules=self.nets)
        except Exception as e:       # noqa: BLE001 -- an object the walk cannot read: no watch = re-trace every epoch (slow, never stale)
            if not self.__dict__.get("_eq_watch_warned"):
                self._eq_watch_warned = True
                warnings.warn(f"neurodiffeq_amd: the Python state read by the equations could not be indexed ({type(e).__name__}: "
                              f"{e}); the equations are re-traced every epoch instead.", RuntimeWarning)
            return None

    @property
    def fused_active(self):
        return self._fused_sys is not None

    # ------------------------------------------------------------------------------------------ epoch
    def _run_epoch(self, key):
        """One epoch on train/valid points (solvers.py:343-424)."""
        if self.n_batches[key] <= 0:
            return
        self._phase = key
        library_code = _library_code()
        inner = getattr(self.generator[key], "generator", None)
        if type(inner).__module__ == "neurodiffeq_amd.generators" and type(inner).__name__ in ("DeviceGenerator", "ResidentBatchGenerator") \
                and type(self)._generate_batch is BaseSolver._generate_batch:
            with library_code():           # device-side / resident batches: library code end to end (engine.library_code)
                first_batch = self._generate_batch(key)
        else:
            first_batch = self._generate_batch(key)
        system = self._fused_system(len(first_batch))
        if system is None:
            return self._run_epoch_composite(key, first_batch)
        if self.dist is not None:
            n_all = first_batch[0].shape[0]
            if n_all < self.dist.world_size and not self.dist.presharded:
                raise ValueError(f"a batch of {n_all} points cannot be sharded over {self.dist.world_size} ranks")
            # the largest shard decides which closure-kernel build serves the batch: the same on every rank
            system.select_n = n_all if self.dist.presharded else -(-n_all // self.dist.world_size)
        nb = self.n_batches[key]
        with library_code() as lc:         # (user code below -- further batches -- runs inside lc.user_code())
            self._lc = lc
            # (a batch with no points at all -- a FilterGenerator that kept nothing: the reference's mean over nothing is nan and
            # so is everything after it, solvers.py:369-395; the kernels have no such launch.  Asked in here: under a global
            # TorchFunctionMode every tensor attribute read outside library_code costs ~0.6 us)
            empty = first_batch[0].shape[0] == 0
            done = False if empty else self._run_epoch_native(key, system, first_batch)
        if empty:
            return self._run_epoch_composite(key, first_batch)
        if done:
            return
        metric_values = {name: 0.0 for name in self.metrics_fn}
        if system.loss_buf.numel() < nb:
            system.loss_buf = torch.zeros(nb, dtype=system.dt, device=self.device)
        closure_opt = key == "train" and _requires_closure(self.optimizer)
        if key == "train" and not closure_opt:
            self.optimizer.zero_grad()
        shard = self.dist
        for batch_id in range(nb):
            batch = first_batch if batch_id == 0 else self._generate_batch(key)
            n_all = batch[0].shape[0]
            lo, hi = shard.bounds(n_all) if shard else (0, n_all)
            if closure_opt:
                # LBFGS-style optimisers (solvers.py:397-400): one optimizer.step(closure) per batch; every call of the
                # closure is one fused closure evaluation that overwrites the gradients and returns the batch loss
                last = {}

                def closure():
                    last["bn"] = system.step(batch, train=True, slot=batch_id, accumulate=False, n_global=n_all,
                                             want_funcs=bool(self.metrics_fn))
                    for fp in system.flat:
                        fp.attach_grads()
                    system.attach_theta_grads()
                    return system.loss_buf[batch_id].clone()
                self._do_optimizer_step(closure=closure)
                b, n = last["bn"]
            else:
                b, n = system.step(batch, train=(key == "train"), slot=batch_id, accumulate=(batch_id > 0),
                                   n_global=shard.global_n(n_all) if shard else n_all, lo=lo, hi=hi,
                                   want_funcs=bool(self.metrics_fn))
            if self.metrics_fn and getattr(self, "_host_metrics", False):
                # metrics the tracer cannot express: the reference's own evaluation (solvers.py:377-379) on the function
                # values the kernels wrote out for this batch
                funcs, coords = system.func_columns(b, n), system.coord_columns(b, n)
                for name, fn in self.metrics_fn.items():
                    metric_values[name] += float(fn(*funcs, *coords))
            elif self.metrics_fn:
                # traced with the system: per-point terms in extra function rows; metric = their mean over the GLOBAL
                # batch (shard sums are added up across ranks)
                sums = system.metric_sums(b, n)
                if shard:
                    sums = sums.contiguous()
                    shard.all_reduce_flat(sums)
                vals = (sums / float(shard.global_n(n_all) if shard else n_all)).tolist()
                for name, v in zip(self.metrics_fn, vals):
                    metric_values[name] += v
        if key == "train":
            for fp in system.flat:
                fp.attach_grads()
        if shard:
            shard.all_reduce(system, nb, train=(key == "train"))
        if key == "train":
            system.attach_theta_grads()      # trainable scalars of the equations: .grad for the user's optimiser
        epoch_loss = system.loss_buf[:nb].sum().item() / nb           # the epoch's only host synchronisation
        self._update_history(epoch_loss, "loss", key)
        if key == "valid" or self.n_batches["valid"] == 0:
            self._update_best(key)
        if key == "train" and not closure_opt:
            self._do_optimizer_step()
        for name in self.metrics_fn:
            self._update_history(metric_values[name] / nb, name, key)

    def _native_ok(self):
        """May the epoch's bookkeeping stay on the device?  (default hooks, FusedAdam, no metrics)"""
        cls = type(self)
        return (not self.metrics_fn and isinstance(self.optimizer, FusedAdam)
                and cls._do_optimizer_step is BaseSolver._do_optimizer_step
                and cls._update_best is BaseSolver._update_best
                and cls._update_history is BaseSolver._update_history)

    def _run_epoch_native(self, key, system, first_batch):
        """Whole epoch with no host synchronisation.  Single-network systems with one batch per training epoch go
        through ONE native call (engine.fast_train_epoch: closure kernel + fused sums/tail kernel); every other fused
        system runs its per-batch launch sequence and then the device-side epoch tail (loss history ring, best
        snapshot, fused Adam per network).  Inverse problems -- trainable scalars inside the equations -- whose FusedAdam owns
        the scalars (engine.theta_tail_eligible) and that train on one batch per epoch stay here too: the training epoch is ONE
        native call of two launches whose sums + tail launch also reduces and steps the scalars
        (engine.fast_train_epoch_theta), validation epochs the per-batch sequence + epoch_tail.  Returns False if the general
        (host-synchronising) path must run."""
        if not self._native_ok():
            return False
        theta_route = False
        if system._theta_trainable:
            # trainable equation coefficients: on the device when the optimiser is a FusedAdam that owns every one of them
            # (NDQ_NO_THETA_TAIL=1: never), else stepped by the user's optimiser on the general path.  Decided per system, for
            # training and validation epochs alike, so that one history never mixes the two kinds of bookkeeping
            theta_route = self.n_batches["train"] == 1 and system.theta_tail_ready(self.optimizer, self.dist)
            if not theta_route:
                system.disown_theta()
                return False
        # (FROZEN scalar arguments -- runtime constants of a ramped coefficient, the batch size in the arithmetic: symbolic.Graph
        # .external / .nbatch -- need no optimiser: such systems keep the device-side epoch; step() refreshes the arguments.
        # fast_ready() / fit_ready() stay False for them, so they take the per-batch launch sequence + epoch_tail below)
        # (fp64 systems -- the reference's default precision -- have no multi-epoch call: they run their per-batch launch
        # sequence (closure kernel in double, or the three-kernel pipeline) and then the device-side epoch tail in double,
        # ndq64_epoch_tail: 2 + 2 K launches behind a closure kernel.  Opt-in, NDQ_F64_FUSED_TAIL=1: a one-batch training
        # epoch behind a closure kernel is ONE native call of two launches, engine.fast_train_epoch_nets -- same bits)
        train = key == "train"
        nb = self.n_batches[key]
        track_best = (not train) or self.n_batches["valid"] == 0
        if train and system.fusedk is not None:
            n_all = first_batch[0].shape[0]
            lo, hi = self.dist.bounds(n_all) if self.dist else (0, n_all)
            if system.needs_check(hi - lo):
                # first training batch served by this build of the single-launch closure kernel: it proves itself against
                # the three-kernel pipeline (engine.verify_fused) before any parameter is updated with its gradients
                ok = system.verify_on(first_batch, self.dist.global_n(n_all) if self.dist else n_all, lo, hi)
                if self.dist and not self.dist.agree(ok, self.device) and ok:
                    system.reject_fused()                 # ranks must take the same path: another rank rejected its kernel
        if theta_route:
            if system.fusedk is None:             # the closure kernel was rejected just now: no device-side scalar update
                system.disown_theta()
                return False
            if train:
                # (before any step counter advances: the one launch takes ONE Adam step count for all networks)
                if not all(self.optimizer.bound(fp) for fp in system.flat):
                    self.optimizer.bind(system.flat)
                if not all(self.optimizer.bound(fp) for fp in system.flat) or \
                        len({self.optimizer._steps.get(id(fp)) for fp in system.flat}) != 1:
                    system.disown_theta()
                    return False
            system.own_theta()
        fs = system.fast_state()
        if max(fs["pending"], fs["pending_valid"]) >= system.HIST:
            self._flush_device_history()
        # a best loss found on the host path (or set by the user) must be what the device compares against
        if fs["pending"] == 0 and fs["pending_valid"] == 0:
            fs["best_loss"].fill_(float("inf") if self._lowest_loss is None else float(self._lowest_loss))
        slots = None
        if train:
            if not all(self.optimizer.bound(fp) for fp in system.flat):
                self.optimizer.bind(system.flat)     # a new / unpickled / re-loaded optimiser: adopt its state first
                if not all(self.optimizer.bound(fp) for fp in system.flat):
                    return False
            slots = [self.optimizer.fast_slot(fp) for fp in system.flat]
        shard = self.dist
        # (a static validation set served nb times -- the default: 4 x the same grid -- is nb identical losses: one batch)
        one_batch = nb == 1 or (not train and draws_are_static(self.generator["valid"]))
        if theta_route and train:
            # inverse problem: closure launch + ONE sums / tail launch that also steps the scalars of the equations
            system.fast_train_epoch_theta(first_batch, self.optimizer, slots, track_best)
        elif shard is None and one_batch and system.fit_ready() and self._fit_epoch(key, system, first_batch, slots):
            pass        # one epoch through ndq_fused_fit_run: the device code the multi-epoch path of fit() runs
        elif train and nb == 1 and len(system.flat) > 1 and system.fast_ready(shard) and len({s[3] for s in slots}) == 1:
            # several networks behind one closure launch, all at the same Adam step (always, unless states were edited)
            system.fast_train_epoch_nets(first_batch, slots, track_best)
        elif train and nb == 1 and shard is None and system.f64_tail_ready() and len({s[3] for s in slots}) == 1:
            # fp64, opt-in (NDQ_F64_FUSED_TAIL=1): closure launch + ONE sums / tail launch in double for all networks
            system.fast_train_epoch_nets(first_batch, slots, track_best)
        elif train and nb == 1 and len(system.flat) == 1 and system.fast_ready(shard):
            batch = first_batch
            n_all = batch[0].shape[0]
            if shard is not None:
                lo, hi = shard.bounds(n_all)
                if (lo, hi) != (0, n_all):
                    batch = [c[lo:hi] for c in batch]
            system.fast_train_epoch(batch, self.optimizer, slots[0], track_best,
                                    n_global=shard.global_n(n_all) if shard else n_all, dist=shard)
        else:
            if system.loss_buf.numel() < nb:
                system.loss_buf = torch.zeros(nb, dtype=system.dt, device=self.device)
            batches = [first_batch]
            if nb > 1:
                with self._lc.user_code():           # the generators are user code: torch's global modes apply to them
                    batches += [self._generate_batch(key) for _ in range(nb - 1)]
            if not train and nb > 1:
                # a static validation set served nb times (the default: 4 x the same 'equally-spaced' grid) gives nb
                # identical losses under unchanged parameters: evaluate it once, the mean is that value
                if all(b is batches[0] for b in batches[1:]) and batches[0][0].device.type != "cuda":
                    batches = batches[:1]          # SamplerGenerator served the same unchanged columns again
                else:
                    k0 = system.static_key(batches[0])
                    if k0 is not None and all(system.static_key(b) == k0 for b in batches[1:]):
                        batches = batches[:1]
            for batch_id, batch in enumerate(batches):
                n_all = batch[0].shape[0]
                lo, hi = shard.bounds(n_all) if shard else (0, n_all)
                system.step(batch, train=train, slot=batch_id, accumulate=(batch_id > 0),
                            n_global=shard.global_n(n_all) if shard else n_all, lo=lo, hi=hi)
            if shard:
                shard.all_reduce(system, len(batches), train=train)
            system.epoch_tail(key, len(batches), track_best, slots)
        if train:
            for fp in system.flat:
                if not fp.grads_attached():
                    fp.attach_grads()
        self._phase = key
        return True

    def _fit_epoch(self, key, system, batch, slots):
        """ONE training or validation epoch (one batch) through engine.fit_run.  False: not applicable here."""
        train = key == "train"
        if train:
            if len({s[3] for s in slots}) != 1:
                return False                          # networks at different Adam steps (edited optimiser state)
            src = device_source(batch)
            if src is not None and src.prefetch:
                return False                          # the prefetching device sampler rides on ndq_fused_step_run's tail
        n_all = batch[0].shape[0]
        if system.needs_check(n_all):
            return False
        b, n = system.upload(batch)
        ptr = system._coord_ptr(b, 0).value
        if train:
            # fast_slot() has advanced every step counter by one already: slots[k][3] is the step after this update
            system.fit_run([ptr], n, b["ld"], slots, None, track_best=1 if self.n_batches["valid"] == 0 else 0)
        else:
            system.fit_run([], 0, 0, None, (ptr, n, b["ld"]), track_best=2)
        return True

    #: methods the reference's fit loop goes through every epoch (solvers.py:443-497); the multi-epoch path skips them
    _PER_EPOCH_METHODS = ("run_train_epoch", "run_valid_epoch", "_run_epoch", "_generate_batch", "_generate_train_batch",
                          "_generate_valid_batch")

    #: epochs per native call of the multi-epoch fit path (bounded further by the device-side history ring and by 64 MiB
    #: of staged collocation points)
    FIT_CHUNK = 256

    def _fit_chunk(self, remaining):
        """Up to ``remaining`` epochs of (training epoch, validation epoch) with ONE native call (engine.fit_run ->
        ndq_fused_fit_run) when nothing has to run on the host in between: the solver's default hooks, FusedAdam, one
        training batch per epoch from a generator of the reference's own classes, a static validation set (or none),
        no data parallelism.  The training batches of the whole chunk are drawn from torch's CPU generator in the
        reference's call order (bit-identical points) and uploaded as one block.  Returns the number of epochs run;
        0 = not applicable right now, the caller runs one epoch the ordinary way (solvers.py:443-497)."""
        system = self._fused_sys
        if system is None or self.dist is not None or self.n_batches["train"] != 1 or remaining < 2:
            return 0
        if not self._native_ok() or not system.fit_ready() or getattr(system.program, "loss_probe", None) is not None:
            return 0
        if system.n_data:
            # per-point data columns ride behind the coordinates of every uploaded batch (engine.upload); the blocks this
            # path stages hold coordinates only, so such systems run epoch by epoch
            return 0
        cls = type(self)
        if any(getattr(cls, m) is not getattr(BaseSolver, m) for m in self._PER_EPOCH_METHODS):
            return 0                      # a subclass hooks the per-epoch methods the reference's fit loop calls: keep calling them
        nv = self.n_batches["valid"]
        tg, vg = self.generator["train"], self.generator["valid"]
        if not draws_have_fixed_size(tg) or (nv > 0 and not draws_are_static(vg)):
            return 0
        if type(tg.generator).__name__ == "DeviceGenerator":
            return 0
        if self._fused_system(system.n_coords) is not system:      # something was swapped since the last epoch
            return 0
        if self._eq_watch_blocks_chunks():
            return 0                      # equations that may follow the epoch counter / unstampable state: epoch by epoch
        if not self._equations_unchanged(system, force=True):       # chunk boundary: unconditional re-trace (EQ_PROBE_EVERY)
            self._fused_key = None
            return 0
        n = tg.size
        if system.needs_check(n):
            return 0
        if not all(self.optimizer.bound(fp) for fp in system.flat):
            return 0
        if len({self.optimizer._steps.get(id(fp)) for fp in system.flat}) != 1:
            return 0                      # networks at different Adam step counts (edited optimiser state): epoch by epoch
        fs = system.fast_state()
        if max(fs["pending"], fs["pending_valid"]) + 2 > system.HIST:
            self._flush_device_history()
        k_max = min(self.FIT_CHUNK, max(2, (64 << 20) // (4 * system.n_coords * (n + 63))))
        K = min(remaining, k_max, system.HIST - max(fs["pending"], fs["pending_valid"]))
        if K < 2:
            return 0
        if fs["pending"] == 0 and fs["pending_valid"] == 0:
            fs["best_loss"].fill_(float("inf") if self._lowest_loss is None else float(self._lowest_loss))
        # ---- validation set: static, resident
        valid = None
        if nv > 0:
            vcols = self._generate_batch("valid")        # static: no RNG draw, the same columns every time
            vres = system.resident_ptr(vcols)
            if vcols[0].shape[0] < 1 or (vres is None and vcols[0].device.type == "cuda"):
                return 0
            valid = (vres[0], vcols[0].shape[0], vres[1]) if vres is not None else system.static_block(vcols)
        # ---- K training batches in the generator's own draw order
        self._phase = "train"
        trace = getattr(self, "_fit_trace", None)          # diagnostics (scripts/fit_profile.py): host seconds per phase
        if trace is not None:
            import time
            t0 = time.perf_counter()
        block = tg.generator.bulk_examples(K)
        if trace is not None:
            t1 = time.perf_counter()
        if block is not None:
            tg._last = None
            dev, ld = system.stage_batches(block, n, reserve=k_max)
            stride = 4 * system.n_coords * ld
            ptrs = [dev.data_ptr() + e * stride for e in range(K)]
            self._batch["train"] = [block[-1, i].reshape(-1, 1).clone().requires_grad_(True) for i in range(block.shape[1])]
        else:
            draws = [self._generate_batch("train") for _ in range(K)]
            if any(len(d) != system.n_coords or d[0].shape[0] != n for d in draws):
                raise RuntimeError(f"{tg.generator!r} returned batches of different shapes although its class draws a "
                                   "fixed number of points")
            if all(d is draws[0] for d in draws[1:]) and draws[0][0].device.type != "cuda":
                ptr, _, ld = system.static_block(draws[0])            # a static training set: one resident block
                ptrs = [ptr] * K
            elif draws[0][0].device.type == "cuda":
                res = [system.resident_ptr(d) for d in draws]
                if any(r is None or r[1] != res[0][1] for r in res):
                    # device batches that are not SoA blocks: nothing was consumed that could not be served again
                    block = torch.stack([torch.stack([c.detach().reshape(-1) for c in d]) for d in draws])
                    dev = block.to(torch.float32)
                    ld = (n + 63) // 64 * 64
                    pad = torch.zeros(K, system.n_coords, ld, dtype=torch.float32, device=dev.device)
                    pad[:, :, :n] = dev
                    system._fit_keep = pad
                    ptrs = [pad.data_ptr() + e * 4 * system.n_coords * ld for e in range(K)]
                else:
                    ld = res[0][1]
                    ptrs = [r[0] for r in res]
            else:
                block = torch.stack([torch.stack([c.detach().reshape(-1) for c in d]) for d in draws])
                dev, ld = system.stage_batches(block, n, reserve=k_max)
                stride = 4 * system.n_coords * ld
                ptrs = [dev.data_ptr() + e * stride for e in range(K)]
        slots = [self.optimizer.fast_slots(fp, K) for fp in system.flat]
        if len({s[3] for s in slots}) != 1:
            raise RuntimeError("the networks of this solver are at different Adam step counts; call fit() with "
                               "callbacks or run epochs one by one")
        if trace is not None:
            t2 = time.perf_counter()
        system.fit_run(ptrs, n, ld, slots, valid, track_best=2 if nv > 0 else 1)
        if trace is not None:
            trace.append((K, t1 - t0, t2 - t1, time.perf_counter() - t2))
        for fp in system.flat:
            if not fp.grads_attached():
                fp.attach_grads()
        self._phase = "valid" if nv > 0 else "train"
        return K

    def _run_epoch_composite(self, key, first_batch):
        """The reference's closure on torch autograd, for systems outside the fused scope."""
        epoch_loss, batch_loss = 0.0, 0.0
        metric_values = {name: 0.0 for name in self.metrics_fn}
        closure_opt = _requires_closure(self.optimizer)
        if key == "train" and not closure_opt:
            self.optimizer.zero_grad()
        dev = self.device
        for batch_id in range(self.n_batches[key]):
            batch = first_batch if batch_id == 0 else self._generate_batch(key)
            if batch[0].device != dev:
                batch = [c.detach().to(dev).requires_grad_(True) for c in batch]
                self._batch[key] = batch

            def closure(zero_grad=True):
                # the networks' forward passes go through the HIP stream kernels (autograd_ops.MlpJet, derivatives up to
                # second order); equations / losses that differentiate further re-run on the plain torch forward
                if self._composite_plain:
                    with autograd_ops.native_autograd(False):
                        return closure_body(zero_grad)
                try:
                    # (a Solver never reads the .grad of its sampled coordinates: no extra launch for them)
                    with autograd_ops.native_autograd(None, coordinate_grads=False):
                        return closure_body(zero_grad)
                except autograd_ops.JetOrderError:
                    self._composite_plain = True
                    with autograd_ops.native_autograd(False):
                        return closure_body(zero_grad)

            def closure_body(zero_grad=True):
                nonlocal batch_loss
                if key == "train" and zero_grad:
                    self.optimizer.zero_grad()
                funcs = [self.compute_func_val(n, c, *batch) for n, c in zip(self.nets, self.conditions)]
                for name in self.metrics_fn:
                    metric_values[name] += self.metrics_fn[name](*funcs, *batch).item()
                residuals = torch.cat(self.diff_eqs(*funcs, *batch), dim=1)
                try:
                    loss = self.loss_fn(residuals, funcs, batch) + self.additional_loss(residuals, funcs, batch)
                except TypeError as e:
                    warnings.warn("You might need to update your code. Since v0.4.0; both `criterion` and "
                                  "`additional_loss` requires three inputs: `residual`, `funcs`, and `coords`.",
                                  FutureWarning)
                    raise e
                if key == "train":
                    loss.backward()
                    batch_loss = loss.item()
                return loss

            if key == "train":
                if closure_opt:
                    self._do_optimizer_step(closure=closure)
                else:
                    closure(zero_grad=False)
                epoch_loss += batch_loss
            else:
                epoch_loss += closure().item()
        self._update_history(epoch_loss / self.n_batches[key], "loss", key)
        if key == "valid" or self.n_batches["valid"] == 0:
            self._update_best(key)
        if key == "train" and not closure_opt:
            self._do_optimizer_step()
        for name in self.metrics_fn:
            self._update_history(metric_values[name] / self.n_batches[key], name, key)

    def run_train_epoch(self):
        self._run_epoch("train")

    def run_valid_epoch(self):
        self._run_epoch("valid")

    def _update_best(self, key):
        current_loss = self.metrics_history[key + "_loss"][-1]
        if (self._lowest_loss is None) or current_loss < self._lowest_loss:
            self._lowest_loss = current_loss
            outside = self._fused_sys is not None and any(isinstance(p, tuple) for p in self._fused_sys.theta_params)
            if self._fused_sys is not None and not outside:
                for fp in self._fused_sys.flat:
                    fp.sync()
                self._best_flat = [fp.flat.clone() for fp in self._fused_sys.flat]
                self._best_nets = None
            else:
                # (a symbolic skip connection's weights live outside the kernels' flat vectors: snapshot the modules themselves)
                if self._fused_sys is not None:
                    for fp in self._fused_sys.flat:
                        fp.sync()
                self.best_nets = deepcopy(self.nets)

    def fit(self, max_epochs, callbacks=(), tqdm_file=sys.stderr, **kwargs):
        """Run ``max_epochs`` epochs of (train, valid, callbacks) -- solvers.py:443-497."""
        self._stop_training = False
        self._max_local_epoch = max_epochs
        monitor = kwargs.pop("monitor", None)
        if monitor:
            warnings.warn("Passing `monitor` is deprecated, use a MonitorCallback and pass a list of callbacks instead")
            callbacks = [monitor.to_callback()] + list(callbacks)
        if kwargs:
            raise ValueError(f"Unknown keyword argument(s): {list(kwargs.keys())}")
        bar = None
        if tqdm_file is not None:
            try:
                from tqdm.auto import tqdm
                bar = tqdm(total=max_epochs, desc="Training Progress", colour="blue", file=tqdm_file, dynamic_ncols=True)
            except ImportError:  # pragma: no cover
                pass
        done = 0
        try:
            while done < max_epochs and not self._stop_training:
                # with no callback to run between epochs, whole chunks of epochs go through one native call
                k = self._fit_chunk(max_epochs - done) if not callbacks else 0
                if k == 0:
                    self.local_epoch = done + 1
                    self.run_train_epoch()
                    self.run_valid_epoch()
                    for cb in callbacks:
                        cb(self)
                    k = 1
                done += k
                self.local_epoch = done
                if bar is not None:
                    bar.update(k)
        finally:
            if bar is not None:
                bar.close()
        self._flush_device_history()

    # ------------------------------------------------------------------------------------------ results
    @abstractmethod
    def get_solution(self, copy=True, best=True):
        pass  # pragma: no cover

    def _solution(self, cls, copy, best):
        nets = self.best_nets if best else self.nets
        conditions = self.conditions
        if copy:
            nets, conditions = deepcopy(nets), deepcopy(conditions)
        return cls(nets, conditions)

    def _get_internal_variables(self):
        return {
            "metrics": self.metrics_fn, "n_batches": self.n_batches, "best_nets": self.best_nets,
            "criterion": self.loss_fn, "loss_fn": self.loss_fn, "conditions": self.conditions,
            "global_epoch": self.global_epoch, "lowest_loss": self.lowest_loss, "n_funcs": self.n_funcs,
            "nets": self.nets, "optimizer": self.optimizer, "diff_eqs": self.diff_eqs, "generator": self.generator,
            "train_generator": self.generator["train"], "valid_generator": self.generator["valid"],
        }

    def get_internals(self, var_names=None, return_type="list", param_names=None):
        if param_names is not None:
            warnings.warn("`param_names` is deprecated; use `var_names`", FutureWarning)
            var_names = param_names
        available = self._get_internal_variables()
        if var_names == "all" or var_names is None:
            return available
        if isinstance(var_names, str):
            return available[var_names]
        if return_type == "list":
            return [available[name] for name in var_names]
        if return_type == "dict":
            return {name: available[name] for name in var_names}
        raise ValueError(f"unrecognized return_type = {return_type}")

    def _fused_residuals(self, coords, best):
        """Residual columns through the forward + generated pointwise kernels (no autograd graph); None -> composite."""
        if self.device.type != "cuda" or self.fused == "off" or any(c.dtype not in (torch.float32, torch.float64)
                                                                    for c in coords):
            return None
        nets = self.best_nets if best else self.nets
        if nets is None:
            return None
        key = (tuple(id(n) for n in nets), id(self.diff_eqs), tuple(id(c) for c in self.conditions), len(coords), _net_structure[0])
        # the reference evaluates diff_eqs / the conditions afresh on every call (solvers.py:606-646): a cached trace is used
        # again only if a re-trace on the same symbols still arrives at it (program.eq_probe: ~0.1 - 0.7 ms, this is not the
        # training loop); numbers that moved since become runtime constants of the rebuild (symbolic.Graph.external)
        volatile = frozenset()
        held = self._resid_sys if getattr(self, "_resid_key", None) == key else None
        if held is not None and not held.program.eq_probe():
            volatile = held.program.suggest_volatile()
            self._resid_key = None
        if getattr(self, "_resid_key", None) != key:
            self._resid_key, self._resid_sys = key, None
            try:
                from .engine import FusedSystem
                self._resid_sys = FusedSystem(nets, self.conditions, self.diff_eqs, len(coords), self.device,
                                              compute_func_val=self.compute_func_val, single_kernel=False, volatile=volatile)
            except TraceUnsupported:
                pass
        if self._resid_sys is None:
            return None
        res = self._resid_sys.residuals([c.detach().to(torch.float32) for c in coords])
        return [res[e].clone() for e in range(res.shape[0])]

    def get_residuals(self, *coords, to_numpy=False, best=True, no_reshape=False):
        """Residuals of ``diff_eqs`` at given points (solvers.py:606-646)."""
        coords = [c if isinstance(c, torch.Tensor) else torch.tensor(c) for c in coords]
        original_shape = coords[0].shape
        fused = self._fused_residuals(coords, best)
        if fused is not None:
            residuals = [r.reshape(-1, 1) if no_reshape else r.reshape(*original_shape) for r in fused]
            if to_numpy:
                residuals = [r.cpu().numpy() for r in residuals]
            return residuals if len(residuals) > 1 else residuals[0]
        coords = [c.detach().to(self.device).reshape(-1, 1).requires_grad_() for c in coords]
        solution = self.get_solution(copy=False, best=best)
        funcs = solution(*coords, to_numpy=False, no_reshape=no_reshape)
        if isinstance(funcs, torch.Tensor):
            funcs = [funcs]
        residuals = self.diff_eqs(*funcs, *coords)
        if not no_reshape:
            residuals = [r.reshape(*original_shape) for r in residuals]
        if to_numpy:
            residuals = [r.detach().cpu().numpy() for r in residuals]
        return residuals if len(residuals) > 1 else residuals[0]


class BaseSolution(ABC):
    """Callable solution object (solvers.py:649-720)."""

    def __init__(self, nets, conditions):
        if nets is None:
            raise RuntimeError("The nets cannot be None, check if you disabled validation and used `best`=True with "
                               "`get_solution` / `get_residual`")
        self.nets = [nets] * len(conditions) if isinstance(nets, nn.Module) else nets
        self.conditions = conditions

    @abstractmethod
    def _compute_u(self, net, condition, *coords):
        pass  # pragma: no cover

    def __call__(self, *coords, to_numpy=False, no_reshape=False, as_type=None):
        if as_type is not None:
            warnings.warn("`as_type` is deprecated; use `to_numpy`", FutureWarning)
            to_numpy = as_type
        coords = [c if isinstance(c, torch.Tensor) else torch.tensor(c) for c in coords]
        original_shape = coords[0].shape
        try:
            dev = next(self.nets[0].parameters()).device
        except StopIteration:  # pragma: no cover
            dev = coords[0].device
        coords = [c.to(dev).reshape(-1, 1) for c in coords]
        if isinstance(to_numpy, str):
            if to_numpy in ("tf", "torch"):
                to_numpy = False
            elif to_numpy == "np":
                to_numpy = True
            else:
                raise ValueError(f"Unrecognized `as_type` option: '{to_numpy}'")
        us = self._fused_values(coords)
        if us is None:      # composite (torch) evaluation: anything the tracer / kernels do not cover
            us = [self._compute_u(net, con, *coords) for con, net in zip(self.conditions, self.nets)]
        if not no_reshape:
            us = [u.reshape(*original_shape) for u in us]
        if to_numpy:
            us = [u.detach().cpu().numpy() for u in us]
        return us if len(self.nets) > 1 else us[0]


    def _fused_values(self, coords):
        """u_i at the given (N, 1) coordinate columns through the forward-only gfx950 kernels, or None when the
        solution cannot be traced / the networks are not on an MI355X.  ``_compute_u`` itself is what gets traced, so
        subclasses (harmonic expansions, ...) are covered without extra code."""
        if coords[0].device.type != "cuda" or coords[0].dtype != torch.float32 or coords[0].requires_grad \
                or len(set(id(n) for n in self.nets)) != len(self.nets):
            return None
        key = (tuple(id(n) for n in self.nets), tuple(id(c) for c in self.conditions), len(coords), _net_structure[0])
        # (a boundary value stored on a condition object may have been changed since the cached trace: re-probed on every
        # call like _fused_residuals -- the reference's solutions call cond.enforce afresh, solvers.py:682-720)
        volatile = frozenset()
        held = self._eval_sys if getattr(self, "_eval_key", None) == key else None
        if held is not None and not held.program.eq_probe():
            volatile = held.program.suggest_volatile()
            self._eval_key = None
        if getattr(self, "_eval_key", None) != key:
            self._eval_key, self._eval_sys = key, None
            try:
                from .engine import FusedSystem
                self._eval_sys = FusedSystem(self.nets, self.conditions, None, len(coords), coords[0].device,
                                             compute_func_val=self._compute_u, single_kernel=False, volatile=volatile)
            except (TraceUnsupported, _lib.NdqError):
                pass
        if self._eval_sys is None:
            return None
        return [v.clone() for v in self._eval_sys.split_functions(self._eval_sys.evaluate(coords))]


class GenericSolution(BaseSolution):
    def _compute_u(self, net, condition, *coords):
        return condition.enforce(net, *coords)


class Solution1D(GenericSolution):
    pass


class Solution2D(GenericSolution):
    pass


class SolutionSpherical(GenericSolution):
    """u(r, theta, phi) of a network that takes all three coordinates (solvers.py:971-980)."""


class SolutionSphericalHarmonics(SolutionSpherical):
    """u = sum_k R_k(r) Y_k(theta, phi) with the network producing the coefficient vector R (solvers.py:983-1018)."""

    def __init__(self, nets, conditions, max_degree=None, harmonics_fn=None):
        super().__init__(nets, conditions)
        if harmonics_fn is None and max_degree is None:
            raise ValueError("harmonics_fn should be specified")
        if max_degree is not None:
            warnings.warn("`max_degree` is DEPRECATED; pass `harmonics_fn` instead, which takes precedence",
                          FutureWarning)
            from .function_basis import RealSphericalHarmonics
            self.harmonics_fn = RealSphericalHarmonics(max_degree=max_degree)
        if harmonics_fn is not None:
            self.harmonics_fn = harmonics_fn

    def _compute_u(self, net, condition, rs, thetas, phis):
        return torch.sum(condition.enforce(net, rs) * self.harmonics_fn(thetas, phis), dim=1)


class SolverSpherical(BaseSolver):
    """PDE systems in spherical coordinates (r, theta, phi) (solvers.py:761-968).  ``enforcer(net, cond, coords)``
    replaces ``cond.enforce(net, *coords)`` -- e.g. the harmonic expansion
    ``(cond.enforce(net, r) * Y(theta, phi)).sum(1, keepdim=True)`` of pde_spherical.py:253-254."""

    def __init__(self, pde_system, conditions, r_min=None, r_max=None, nets=None, train_generator=None,
                 valid_generator=None, analytic_solutions=None, optimizer=None, loss_fn=None, n_batches_train=1,
                 n_batches_valid=4, metrics=None, enforcer=None, n_output_units=1, shuffle=None, batch_size=None):
        if (train_generator is None or valid_generator is None) and (r_min is None or r_max is None):
            raise ValueError(f"Either generator is not provided, r_min and r_max should be both provided: "
                             f"got r_min={r_min}, r_max={r_max}, train_generator={train_generator}, "
                             f"valid_generator={valid_generator}")
        if train_generator is None:
            train_generator = GeneratorSpherical(512, r_min, r_max, method="equally-spaced-noisy")
        if valid_generator is None:
            valid_generator = GeneratorSpherical(512, r_min, r_max, method="equally-spaced-noisy")
        self.r_min, self.r_max = r_min, r_max
        self.enforcer = enforcer
        super().__init__(diff_eqs=pde_system, conditions=conditions, nets=nets, train_generator=train_generator,
                         valid_generator=valid_generator, analytic_solutions=analytic_solutions, optimizer=optimizer,
                         loss_fn=loss_fn, n_batches_train=n_batches_train, n_batches_valid=n_batches_valid,
                         metrics=metrics, n_input_units=3, n_output_units=n_output_units, shuffle=shuffle,
                         batch_size=batch_size)

    def _auto_enforce(self, net, cond, *coordinates):
        if self.enforcer:
            return self.enforcer(net, cond, coordinates)
        # fill cond.enforce with as many leading coordinates as its parameterisation takes
        fn = cond.parameterize if cond.__class__.enforce == BaseCondition.enforce else cond.enforce
        n_params = len(inspect.signature(fn).parameters)
        return cond.enforce(net, *coordinates[:n_params - 1])

    def compute_func_val(self, net, cond, *coordinates):
        return self._auto_enforce(net, cond, *coordinates)

    def get_solution(self, copy=True, best=True, harmonics_fn=None):
        nets = self.best_nets if best else self.nets
        conditions = self.conditions
        if copy:
            nets, conditions = deepcopy(nets), deepcopy(conditions)
        if harmonics_fn:
            return SolutionSphericalHarmonics(nets, conditions, harmonics_fn=harmonics_fn)
        return SolutionSpherical(nets, conditions)

    def _get_internal_variables(self):
        d = super()._get_internal_variables()
        d.update(r_min=self.r_min, r_max=self.r_max, enforcer=self.enforcer)
        return d


class GenericSolver(BaseSolver):
    def get_solution(self, copy=True, best=True):
        return self._solution(GenericSolution, copy, best)


class Solver1D(BaseSolver):
    """ODE systems in one independent variable (solvers.py:1020-1186)."""

    def __init__(self, ode_system, conditions, t_min=None, t_max=None, nets=None, train_generator=None,
                 valid_generator=None, analytic_solutions=None, optimizer=None, loss_fn=None, n_batches_train=1,
                 n_batches_valid=4, metrics=None, n_output_units=1, batch_size=None, shuffle=None):
        if (train_generator is None or valid_generator is None) and (t_min is None or t_max is None):
            raise ValueError(f"Either generator is not provided, t_min and t_max should be both provided: \n"
                             f"got t_min={t_min}, t_max={t_max}, train_generator={train_generator}, "
                             f"valid_generator={valid_generator}")
        if train_generator is None:
            train_generator = Generator1D(32, t_min=t_min, t_max=t_max, method="equally-spaced-noisy")
        if valid_generator is None:
            valid_generator = Generator1D(32, t_min=t_min, t_max=t_max, method="equally-spaced")
        self.t_min, self.t_max = t_min, t_max
        super().__init__(diff_eqs=ode_system, conditions=conditions, nets=nets, train_generator=train_generator,
                         valid_generator=valid_generator, analytic_solutions=analytic_solutions, optimizer=optimizer,
                         loss_fn=loss_fn, n_batches_train=n_batches_train, n_batches_valid=n_batches_valid,
                         metrics=metrics, n_input_units=1, n_output_units=n_output_units, shuffle=shuffle,
                         batch_size=batch_size)

    def get_solution(self, copy=True, best=True):
        return self._solution(Solution1D, copy, best)

    def _get_internal_variables(self):
        d = super()._get_internal_variables()
        d.update(t_min=self.t_min, t_max=self.t_max)
        return d


class BundleSolution1D(GenericSolution):
    pass


class BundleSolver1D(BaseSolver):
    """A bundle of ODE solutions: the networks take ``(t, *theta)`` where ``theta`` are equation parameters and / or
    condition parameters sampled next to ``t`` (solvers.py:1189-1420).  ``eq_param_index`` selects which of the bundle
    inputs the ODE callable receives after ``(*funcs, t)``.  On the fused path the extra inputs are ordinary input
    coordinates of the network whose derivative streams are simply not requested."""

    def __init__(self, ode_system, conditions, t_min=None, t_max=None, theta_min=None, theta_max=None,
                 eq_param_index=(), nets=None, train_generator=None, valid_generator=None, analytic_solutions=None,
                 optimizer=None, loss_fn=None, n_batches_train=1, n_batches_valid=4, metrics=None, n_output_units=1,
                 batch_size=None, shuffle=None):
        if (train_generator is None or valid_generator is None) and (t_min is None or t_max is None):
            raise ValueError(f"Either generator is not provided, t_min and t_max should be both provided: \n"
                             f"got t_min={t_min}, t_max={t_max}, train_generator={train_generator}, "
                             f"valid_generator={valid_generator}")
        theta_min = (theta_min,) if isinstance(theta_min, (float, int)) else tuple(theta_min or ())
        theta_max = (theta_max,) if isinstance(theta_max, (float, int)) else tuple(theta_max or ())
        if len(theta_min) != len(theta_max):
            raise ValueError(f"length of theta_min and theta_max must be equal, got {len(theta_min)} != {len(theta_max)}")
        r_min, r_max = (t_min,) + theta_min, (t_max,) + theta_max
        n_input_units = len(r_min)
        if train_generator is None:
            train_generator = Generator1D(32, t_min=t_min, t_max=t_max, method="equally-spaced-noisy")
            for lo, hi in zip(theta_min, theta_max):
                train_generator ^= Generator1D(32, t_min=lo, t_max=hi, method="equally-spaced-noisy")
        if valid_generator is None:
            valid_generator = Generator1D(32, t_min=t_min, t_max=t_max, method="equally-spaced")
            for lo, hi in zip(theta_min, theta_max):
                valid_generator ^= Generator1D(32, t_min=lo, t_max=hi, method="equally-spaced")
        self.r_min, self.r_max = r_min, r_max
        n_funcs, n_coords = len(conditions), 1
        picked = tuple(n_funcs + n_coords + idx for idx in eq_param_index)
        self.eq_param_index = picked

        def bundle_eqs(*variables):
            return ode_system(*variables[:n_funcs + n_coords], *(variables[i] for i in picked))

        super().__init__(diff_eqs=bundle_eqs, conditions=conditions, nets=nets, train_generator=train_generator,
                         valid_generator=valid_generator, analytic_solutions=analytic_solutions, optimizer=optimizer,
                         loss_fn=loss_fn, n_batches_train=n_batches_train, n_batches_valid=n_batches_valid,
                         metrics=metrics, n_input_units=n_input_units, n_output_units=n_output_units, shuffle=shuffle,
                         batch_size=batch_size)

    def get_solution(self, copy=True, best=True):
        return self._solution(BundleSolution1D, copy, best)

    def _get_internal_variables(self):
        d = super()._get_internal_variables()
        d.update(r_min=self.r_min, r_max=self.r_max, eq_param_index=self.eq_param_index)
        return d


class Solver2D(BaseSolver):
    """PDE systems in two independent variables (solvers.py:1427-1593)."""

    def __init__(self, pde_system, conditions, xy_min=None, xy_max=None, nets=None, train_generator=None,
                 valid_generator=None, analytic_solutions=None, optimizer=None, loss_fn=None, n_batches_train=1,
                 n_batches_valid=4, metrics=None, n_output_units=1, batch_size=None, shuffle=None):
        if (train_generator is None or valid_generator is None) and (xy_min is None or xy_max is None):
            raise ValueError(f"Either generator is not provided, xy_min and xy_max should be both provided: \n"
                             f"got xy_min={xy_min}, xy_max={xy_max}, train_generator={train_generator}, "
                             f"valid_generator={valid_generator}")
        if train_generator is None:
            train_generator = Generator2D((32, 32), xy_min=xy_min, xy_max=xy_max, method="equally-spaced-noisy")
        if valid_generator is None:
            valid_generator = Generator2D((32, 32), xy_min=xy_min, xy_max=xy_max, method="equally-spaced")
        self.xy_min, self.xy_max = xy_min, xy_max
        super().__init__(diff_eqs=pde_system, conditions=conditions, nets=nets, train_generator=train_generator,
                         valid_generator=valid_generator, analytic_solutions=analytic_solutions, optimizer=optimizer,
                         loss_fn=loss_fn, n_batches_train=n_batches_train, n_batches_valid=n_batches_valid,
                         metrics=metrics, n_input_units=2, n_output_units=n_output_units, shuffle=shuffle,
                         batch_size=batch_size)

    def get_solution(self, copy=True, best=True):
        return self._solution(Solution2D, copy, best)

    def _get_internal_variables(self):
        d = super()._get_internal_variables()
        d.update(xy_min=self.xy_min, xy_max=self.xy_max)
        return d
