"""The fused train / evaluation step of one PDE system on one MI355X.

This is the compute core of ``BaseSolver._run_epoch``'s closure (reference: solvers.py:369-395) re-expressed as a
fixed launch sequence on one HIP stream, per batch:

    H2D (one SoA block)  ->  ndq_mlp_jet_fwd  x n_nets          FCNN.forward + every diff() over it
                         ->  generated pointwise kernel          parameterize + diff_eqs + sum r^2 + adjoint seeds
                         ->  ndq_mlp_jet_bwd  x n_nets           loss.backward() through the networks
                         ->  ndq_reduce_partials                 .grad accumulation (+ the loss scalar)

No host synchronisation happens inside a step; the loss stays in HBM until the caller reads it.
"""
import ctypes
import functools
import os

import torch

from . import _lib, codegen, generators
from .networks import FlatParams, describe
from .symbolic import Graph, Sym, TraceUnsupported, trace_scope

_c_vp = ctypes.c_void_p


def _ptr(t):
    return _c_vp(t.data_ptr())


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None) or \
    (lambda idx: torch.cuda.current_stream(idx).cuda_stream)


def _round_up(n, m):
    return (n + m - 1) // m * m


class _Lib64:
    """libndq64.so behind libndq.so's names (``ndq_mlp_jet_fwd`` -> ``ndq64_mlp_jet_fwd`` ...): the fp64 build of the
    stream kernels and of the fixed-order sums, which is all the three-kernel pipeline needs."""

    def __init__(self):
        self._lib = _lib.lib64()

    def __getattr__(self, name):
        return getattr(self._lib, name.replace("ndq_", "ndq64_", 1))


def _ends(c):
    """Raw bytes of the first and the last element of a host tensor (two memory reads through ctypes: ~0.3 us)."""
    n = c.numel()
    if n == 0:
        return ()
    if c.is_contiguous():
        p, e = c.data_ptr(), c.element_size()
        return (ctypes.string_at(p, e), ctypes.string_at(p + (n - 1) * e, e))
    f = c.detach().reshape(-1)
    return (f[0].item(), f[-1].item())


class library_code:
    """``with library_code():`` around host code of this package that names the device of everything it creates.  A global
    TorchFunctionMode -- torch.set_default_device('cuda'), the reference's import default, installs one -- intercepts every
    tensor method call (``data_ptr``, ``shape``, ``device`` ...: ~1 us each, ~40 of them per native epoch, more than the
    epoch's 26 us of kernels); user callables (conditions, equations, generators, callbacks) are never run under this."""
    __slots__ = ("ctx",)

    def __enter__(self):
        self.ctx = torch._C.DisableTorchFunction() if torch._C._len_torch_function_stack() else None
        if self.ctx is not None:
            self.ctx.__enter__()
        return self

    def __exit__(self, *exc):
        if self.ctx is not None:
            self.ctx.__exit__(*exc)
            self.ctx = None
        return False

    def user_code(self):
        """``with lc.user_code():`` inside the block, around a call into user code (a generator's ``get_examples``): the
        global modes are back in force for its duration."""
        return _UserCode(self)


class _UserCode:
    __slots__ = ("lc", "was")

    def __init__(self, lc):
        self.lc = lc

    def __enter__(self):
        self.was = self.lc.ctx is not None
        if self.was:
            self.lc.ctx.__exit__(None, None, None)
            self.lc.ctx = None

    def __exit__(self, *exc):
        if self.was:
            self.lc.ctx = torch._C.DisableTorchFunction()
            self.lc.ctx.__enter__()
        return False


def trace_system(nets, conditions, diff_eqs, n_coords, compute_func_val=None, loss="l2", metrics=(), f64=False,
                 volatile=frozenset()):
    """Trace (conditions, diff_eqs) once on symbolic columns and lower them to a pointwise program.

    Needs no GPU (used by ``__graft_entry__.build`` to pre-compile the generated kernels); raises
    :class:`TraceUnsupported` when the system is outside the fused scope.  Returns ``(program, descs)`` with
    ``descs[k]`` the ``ndq_mlp_desc`` of network k (stream set widened to one libndq.so has kernels for).

    volatile: positions (in the order the callables hand them to the trace, ``symbolic.Graph.external``) of outside numbers
    that become RUNTIME constants of the generated kernels instead of literals -- what ``program.suggest_volatile()`` of an
    earlier trace of the same callables returned after a re-trace that differed in such numbers only (a coefficient ramped
    by a callback: one rebuild, then every further value is an argument update).  fp32 only."""
    L = _Lib64() if f64 else _lib.lib()
    all_nets, conditions = list(nets), list(conditions)
    # one parameter set per DISTINCT module: the reference's single_net / ith_unit mode (ode.py:276-280, pde.py:301-305)
    # and EnsembleCondition share one multi-output network between several functions -- its symbols are output units
    # of ONE network (one stream array, one gradient), not copies
    nets = []
    for n in all_nets:
        if not any(n is m for m in nets):
            nets.append(n)
    from .networks import track_structure
    for n in nets:
        track_structure(n)           # (from here on a replaced layer / re-assigned weight / new hook re-keys the solver's system)
    infos = [describe(n, dtype=torch.float64 if f64 else torch.float32) for n in nets]
    if any(i is None for i in infos):
        raise TraceUnsupported("a network is not an FCNN the gfx950 kernels support")
    g = Graph(n_coords)
    g.f64 = bool(f64)                # (Sym.dtype: constants made "like" a traced column keep the kernels' precision)
    g.volatile = frozenset() if f64 else frozenset(volatile)      # (the fp64 pipeline has no scalar arguments)
    if f64 and any(i.get("skip_sym") is not None for i in infos):
        raise TraceUnsupported("a skip connection above 64 hidden units on the fp64 pipeline (its weights are kernel arguments: fp32 only)")
    g.register_nets(nets, [i["n_out"] for i in infos], skips=[i.get("skip_sym") for i in infos])
    cfv = compute_func_val or (lambda net, cond, *coords: cond.enforce(net, *coords))
    with trace_scope(g):
        coords = [Sym(g, g.coord(i), leaf=True) for i in range(n_coords)]
        funcs = [cfv(n, c, *coords) for n, c in zip(all_nets, conditions)]
        res = diff_eqs(*funcs, *coords) if diff_eqs is not None else []     # None: evaluation of the functions only
        if isinstance(res, Sym):
            res = [res]
        def column(r):
            if isinstance(r, Sym):
                return r
            try:
                return Sym(g, g.const(float(r)))
            except (TypeError, ValueError, RuntimeError):
                raise TraceUnsupported(f"an equation returned {type(r).__name__}, not a traced (N, 1) column or a scalar")
        res = [column(r) for r in res]
        eq_ext = list(g.ext_log)         # the outside numbers the conditions and equations read, in order (suggest_volatile)
        # a function is an (N, 1) column or -- EnsembleCondition on one multi-output network (conditions.py:157-202), used
        # as ONE solver function whose columns the equations pick apart -- an (N, k) matrix: k rows of the function buffer
        from .symbolic import SymMat
        func_columns = []
        for f in funcs:
            if isinstance(f, Sym):
                func_columns.append([f])
            elif isinstance(f, SymMat) and all(isinstance(c, Sym) for c in f.cols):
                func_columns.append(list(f.cols))
            else:
                raise TraceUnsupported(f"a condition returned {type(f).__name__}, not traced (N, k) values")
        # what this trace arrived at, for eq_probe below: the node of every function column and residual
        eq_nodes = tuple(c.i for cols in func_columns for c in cols) + ("|",) + tuple(r.i for r in res)

        def eq_probe():
            """Run the conditions and the equations AGAIN on the same symbolic coordinates.  The graph is hash-consed, so
            an unchanged system arrives at the same nodes; a Python float read from a dict / closure / attribute that a
            callback has changed since (``solvers.py:380`` re-evaluates ``diff_eqs`` every batch) gives another constant
            node and with it other residual nodes.  True: what the kernels were compiled from is still what the user's
            callables compute."""
            n_captured = len(g.captured)
            twins_before = set(getattr(g, "twins", ()))
            # boundary columns of Neumann ends (symbolic.Graph.vcoord) are replayed, not created again: fresh ones would be
            # other coordinates, other sites and other nodes, and every probe would report a changed system
            n_vcoords, n_sites, known_sites = len(g.vcoords), len(g.site_net), dict(g._sites)
            g._vreplay = 0
            g.ext_log = []
            eq_probe.last_ext = None
            try:
                with trace_scope(g):
                    f2 = [cfv(n, c, *coords) for n, c in zip(all_nets, conditions)]
                    r2 = diff_eqs(*f2, *coords) if diff_eqs is not None else []
                    if isinstance(r2, Sym):
                        r2 = [r2]
                    r2 = [column(r) for r in r2]
                cols = []
                for f in f2:
                    if isinstance(f, Sym):
                        cols.append(f.i)
                    elif isinstance(f, SymMat) and all(isinstance(c, Sym) for c in f.cols):
                        cols.extend(c.i for c in f.cols)
                    else:
                        return False
                eq_probe.last_ext = list(g.ext_log)
                return tuple(cols) + ("|",) + tuple(r.i for r in r2) == eq_nodes
            except Exception as e:       # noqa: BLE001 -- whatever the callables do now, it is not what was compiled
                if not getattr(eq_probe, "warned", False):
                    eq_probe.warned = True       # said once: an unexpected kernel rebuild can be traced back to this
                    import warnings
                    warnings.warn(f"neurodiffeq_amd: re-tracing the equations raised {type(e).__name__}: {e}; the system is "
                                  "rebuilt from a fresh trace.  (On the fused path diff_eqs / the conditions run on symbolic "
                                  "columns, once per re-trace: they should be free of side effects.)", RuntimeWarning)
                return False
            finally:
                g._vreplay = None
                for idx in [i for i in g.vcoords if i >= n_coords + n_vcoords]:     # (what a CHANGED boundary left behind)
                    del g.vcoords[idx]
                del g.site_net[n_sites:]
                for key in [k for k in g._sites if k not in known_sites]:
                    g.net_deps.pop(g._sites[key], None)
                    g.net_nout.pop(g._sites[key], None)
                    del g._sites[key]
                del g.captured[n_captured:]       # (the probe's own captures are the same tensors again)
                for key in [k for k in getattr(g, "twins", ()) if k not in twins_before]:
                    del g.twins[key]              # (twins of the tensors this probe created: they would pile up)

        def suggest_volatile():
            """After an ``eq_probe()`` that returned False: the positions to trace as runtime constants next time -- the
            current ones plus every outside number whose value differs from the compiled trace's (same count of numbers
            in both: the callables took the same path).  Any set is safe (module symbolic: Graph.external)."""
            last = getattr(eq_probe, "last_ext", None)
            if last is None or len(last) != len(eq_ext):
                return frozenset(g.volatile)
            return frozenset(g.volatile) | {i for i, (a, b) in enumerate(zip(eq_ext, last)) if a != b and (a == a or b == b)}

        # a custom loss: callable(residual (N, n_eq), funcs, coords) -> scalar (solvers.py:216-226; the solver passes
        # loss_fn + additional_loss as ONE callable) traced to the per-point term whose batch mean it is
        loss_term = None
        loss_probe = None
        if callable(loss):
            from .symbolic import SymMat, SymScalar
            loss_callable = loss
            val = loss(SymMat(res) if res else Sym(g, g.const(0.0)), list(funcs), list(coords))
            if not isinstance(val, SymScalar):
                raise TraceUnsupported(f"the loss function returned {type(val).__name__}, not a batch mean of traced values")
            loss_term, loss = val.term.i, "custom"

            def loss_probe():
                """Run the loss callable again on the same traced columns: the node it returns (the graph is hash-consed)
                differs from the compiled term iff the callable now computes something else -- e.g. a weight that follows
                ``solver.global_epoch``; such a value is a CONSTANT of the generated kernel."""
                with trace_scope(g):
                    again = loss_callable(SymMat(res) if res else Sym(g, g.const(0.0)), list(funcs), list(coords))
                return isinstance(again, SymScalar) and again.term.i == loss_term
        # metrics: callable(*funcs, *coords) -> scalar (solvers.py:377-379), evaluated as extra per-point function
        # rows whose batch mean is the metric
        metric_terms = []
        for fn in metrics:
            from .symbolic import MetricTraceUnsupported, SymScalar
            try:
                val = fn(*funcs, *coords)
            except Exception as e:      # noqa: BLE001 -- whatever the metric does to a traced column that it cannot take
                raise MetricTraceUnsupported(f"a metric could not be traced ({type(e).__name__}: {e})") from e
            if not isinstance(val, SymScalar):
                raise MetricTraceUnsupported(f"a metric returned {type(val).__name__}, not a batch mean of traced values")
            metric_terms.append(val.term)
        metric_fns = list(metrics)

        def metric_probe():
            """Run the metric callables again on the same traced columns: True iff every one still arrives at the per-point term
            that was compiled (a metric that reads Python state -- the amplitude of an analytic solution a callback changes --
            is a constant of the kernel otherwise; the reference re-evaluates metrics every batch, solvers.py:377-379)."""
            with trace_scope(g):
                for fn, term in zip(metric_fns, metric_terms):
                    again = fn(*funcs, *coords)
                    if not (isinstance(again, SymScalar) and again.term.i == term.i):
                        return False
            return True
    for k, info in enumerate(infos):       # a net that never appears in an equation still needs a layout
        g.net_deps.setdefault(k, tuple(range(info["d"])))
        g.net_nout.setdefault(k, info["n_out"])
    descs = {}

    def allow_lap(k, coords):
        """Is there a kernel for site k with the second derivatives w.r.t. ``coords`` merged into one Laplacian stream?"""
        info = infos[g.site_net[k]]
        deps = g.net_deps[k]
        if os.environ.get("NDQ_NO_LAP") or any(c not in deps for c in coords) or info["n_out"] != 1:
            return False
        mask2 = 0
        for c in coords:
            a = deps.index(c)
            mask2 |= 1 << codegen.pair_list(len(deps)).index((a, a))
        d = _lib.MlpDesc(len(deps), 1, mask2, info["hidden"], info["layers"], info["act"], info["n_out"], 1, info["skip"], 0, info["actp"], info["widths"], info["mono"])
        return codegen.ensure_mlp_kernels(d, f64=f64)

    def widen(k, st):
        info = infos[g.site_net[k]]
        if st.d != info["d"]:
            raise TraceUnsupported("network input width differs from the number of coordinates fed to it")
        if st.lap:                      # allow_lap already checked that this exact kernel exists
            descs[k] = _lib.MlpDesc(st.d, 1, st.mask2, info["hidden"], info["layers"], info["act"], info["n_out"], 1, info["skip"], 0, info["actp"], info["widths"], info["mono"])
            codegen.ensure_mlp_kernels(descs[k], f64=f64)
            return
        # exact stream set: from libndq.so's table, else compiled on first use as an extension module ...
        exact = _lib.MlpDesc(st.d, 1 if (st.first or st.mask2) else 0, st.mask2, info["hidden"], info["layers"],
                             info["act"], info["n_out"], 0, info["skip"], st.mask3, info["actp"], info["widths"], info["mono"],
                             getattr(st, "mask4", 0))
        if codegen.ensure_mlp_kernels(exact, f64=f64):
            st.first, st.mask2 = exact.first, exact.mask2
            descs[k] = exact
            return
        if st.mask3 or getattr(st, "mask4", 0):
            raise TraceUnsupported(f"no gfx950 kernel for third- / fourth-order streams of FCNN d={st.d} hidden={info['hidden']} "
                                   f"layers={info['layers']} act={info['act']} (mask3={st.mask3:#b})")
        # ... else the cheapest superset the table has (NDQ_JIT_MLP=0, or a shape the templates cannot express)
        npair = st.d * (st.d + 1) // 2
        best = None
        for first in ((1,) if st.first else (0, 1)):
            for mask2 in range(1 << npair):
                if (mask2 & st.mask2) != st.mask2 or (mask2 and not first):
                    continue
                d = _lib.MlpDesc(st.d, first, mask2, info["hidden"], info["layers"], info["act"], info["n_out"], 0,
                                 info["skip"], 0, info["actp"], info["widths"], info["mono"])
                if L.ndq_mlp_supported(ctypes.byref(d)):
                    cost = first * st.d + bin(mask2).count("1")
                    if best is None or cost < best[0]:
                        best = (cost, d)
        if best is None:
            raise TraceUnsupported(f"no gfx950 kernel for FCNN d={st.d} hidden={info['hidden']} layers="
                                   f"{info['layers']} streams(first={st.first}, mask2={st.mask2:#b})")
        st.first, st.mask2 = best[1].first, best[1].mask2
        descs[k] = best[1]

    # (which systems get one common stream set is the code generator's question: it knows the closure kernels' rules)
    unify = functools.partial(codegen.unify, site_net=g.site_net, n_coords=n_coords, vcoords=g.vcoords, infos=infos, f64=f64)
    program = codegen.PointwiseProgram(g, [r.i for r in res],
                                       [c.i for cols in func_columns for c in cols] + [m.i for m in metric_terms],
                                       len(nets), widen=widen, allow_lap=allow_lap, unify=unify, loss=loss,
                                       loss_term=loss_term)
    program.n_metrics = len(metric_terms)        # the last n_metrics "functions" are per-point metric terms
    program.func_widths = [len(cols) for cols in func_columns]    # columns of every solver function, in order
    program.loss_probe = loss_probe              # custom losses: "does the callable still trace to the compiled term?"
    program.metric_probe = metric_probe if metric_terms else None
    program.eq_probe = eq_probe                  # equations / conditions: "do they still trace to the compiled residuals?"
    program.suggest_volatile = suggest_volatile  # ... and if not: which outside numbers moved (-> runtime constants)
    program.unique_nets = nets                   # distinct modules, in first-appearance order: one parameter set each
    return program, descs


def wants_closure(program, descs, f64):
    """Does a single-launch closure kernel exist for this traced system?  fp32: any mode of ``codegen.fuse_mode``.  fp64: one
    network on the plain closure kernel (``codegen.can_fuse_f64``) or 2..4 narrow networks on the multi-network one
    (``codegen.can_fuse_multi_f64``, which NDQ_NO_MULTI_FUSE turns off with the fp32 mode); NDQ_F64_CLOSURE=0 keeps every fp64
    system on the three-kernel pipeline."""
    if not f64:
        return codegen.can_fuse(program, descs)
    if os.environ.get("NDQ_F64_CLOSURE", "1") == "0":
        return False
    return codegen.can_fuse_f64(program, descs) or codegen.can_fuse_multi_f64(program, descs)


def f64_fused_tail_switch(environ=None):
    """NDQ_F64_FUSED_TAIL=1 (opt-in; unset, "0" or anything else: off): fp64 systems behind a closure kernel finish a training
    epoch with ONE sums + tail launch in double (``ndq64_fused_step_run``) instead of 1 + 2 K launches.
    A pure function of the mapping it is given (default: the process environment)."""
    environ = os.environ if environ is None else environ
    return environ.get("NDQ_F64_FUSED_TAIL", "0") == "1"


def theta_tail_switch(environ=None):
    """On by default; NDQ_NO_THETA_TAIL=1 keeps inverse problems on the general epoch path (host-side optimiser step for the
    scalars).  A pure function of the mapping it is given (default: the process environment)."""
    environ = os.environ if environ is None else environ
    return environ.get("NDQ_NO_THETA_TAIL", "0") != "1"


def theta_tail_eligible(*, enabled, f64, closure, sharded, device, scalars, n_theta, optimizer):
    """May the sums + tail launch of a training epoch step the trainable scalars of the equations (include/ndq.h:
    ndq_theta_step)?  A pure function of what it is given: ``enabled`` (``theta_tail_switch``), fp32, a closure
    kernel, no data-parallel shard, at least one trainable scalar and no more than the launch carries, every one of them a
    WHOLE one-element float32 ``nn.Parameter`` on ``device`` (not entry k of a larger tensor) that ``optimizer`` -- a
    FusedAdam -- owns in a group without amsgrad / maximize."""
    from .optim import FusedAdam
    if not enabled or f64 or not closure or sharded or not scalars or n_theta > _lib.NDQ_THETA_MAX:
        return False
    if not isinstance(optimizer, FusedAdam):
        return False
    device = torch.device(device)
    for p in scalars:
        if isinstance(p, tuple) or not isinstance(p, torch.nn.Parameter) or p.numel() != 1:
            return False
        # ("cuda" without an index names the current device: only two explicit indices can differ)
        same = p.device.type == device.type and (p.device.index is None or device.index is None or p.device.index == device.index)
        if not same or p.dtype != torch.float32 or not optimizer.owns_scalar(p):
            return False
    return True


class FusedSystem:
    def __init__(self, nets, conditions, diff_eqs, n_coords, device, compute_func_val=None, single_kernel=True,
                 loss="l2", metrics=(), dtype=torch.float32, volatile=frozenset()):
        """single_kernel: for single-network systems use the one-launch fused closure kernel (forward + pointwise +
        reverse, csrc/ndq_mlp.h: fused_closure_kernel); otherwise (and for multi-network systems) the three-kernel
        pipeline through HBM streams."""
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.NdqError("the fused path needs an MI355X (device 'cuda'); no CPU fallback exists for it")
        # dtype float64 (the reference's default precision, neurodiffeq/__init__.py:22): the fp64 build of the stream kernels
        # (libndq64.so) with the generated pointwise kernel compiled in double; single-network systems on the plain closure
        # kernel get that kernel compiled in double as well (codegen.can_fuse_f64), systems of 2..4 narrow networks the
        # multi-network closure kernel (codegen.can_fuse_multi_f64); the epoch tail runs on the device
        # (ndq64_epoch_tail; opt-in, NDQ_F64_FUSED_TAIL=1: sums and tail in ONE launch, ndq64_fused_step_run); pull / loop mode,
        # the multi-epoch fit() call and the 8-wave build are fp32 only
        from . import _canary
        _canary.check()              # once per process: the gfx950 hazard reproducer through / without the assembly fix-up pass
        self.dt = dtype
        self.f64 = dtype == torch.float64
        self.esize = 8 if self.f64 else 4
        self.L = _Lib64() if self.f64 else _lib.lib()
        self.f64_fused_tail = self.f64 and f64_fused_tail_switch()      # read once, here (f64_tail_ready)
        self.theta_tail = theta_tail_switch()                           # likewise (theta_tail_ready)
        self._theta_owned = False         # True: theta_buf is authoritative for the trainable scalars (own_theta)
        self.nets, self.conditions, self.n_coords = list(nets), list(conditions), n_coords
        self.program, self.descs = trace_system(self.nets, self.conditions, diff_eqs, n_coords, compute_func_val, loss,
                                                metrics, f64=self.f64, volatile=volatile)
        self.nets = list(self.program.unique_nets)      # a module shared by several functions is ONE parameter set
        # rows of the function-value buffer: the solver's functions, then one per-point term per traced metric
        self.n_eq, self.n_funcs = len(self.program.residuals), len(self.program.funcs)
        self.n_metrics = self.program.n_metrics
        self.n_user_funcs = self.n_funcs - self.n_metrics
        self.loss_norm = self.program.loss_norm      # loss = sum over points of the per-point term / (N * loss_norm)
        # trainable scalars of the equations (nn.Parameter coefficients of inverse problems; the reference re-runs diff_eqs
        # under autograd every batch, solvers.py:380): kernel arguments whose gradient is one more fixed-order sum of
        # per-point adjoints; per-point data columns ((N, 1) tensors aligned with the batch): input rows behind the coordinates
        self.theta_params = list(self.program.g.params)
        # ... and the RUNTIME constants among them (symbolic.Graph.external: outside numbers that change between epochs --
        # frozen host scalars the re-trace refills; no gradient, no optimiser)
        self.theta_frozen = sorted(self.program.g.frozen)
        self._theta_trainable = [j for j in range(len(self.theta_params)) if j not in self.program.g.frozen]
        self._theta_frozen_seen = None
        self.data_cols = list(self.program.g.data)
        self.n_theta, self.n_data = len(self.theta_params), len(self.data_cols)
        self.n_rows = n_coords + self.n_data
        if (self.n_theta or self.n_data) and self.f64:
            raise TraceUnsupported("trainable equation coefficients / data columns on the fp64 pipeline")
        # first use of a system: its pointwise kernel and its single-launch closure kernel are compiled CONCURRENTLY (two
        # hipcc pipelines side by side; cached in-tree afterwards)
        from . import _hipcc
        # (fp64: one network on the plain closure kernel compiled in double, or 2..4 networks on the multi-network one --
        # codegen.can_fuse_multi_f64; NDQ_F64_CLOSURE=0: three-kernel pipeline only)
        want_fused = single_kernel and wants_closure(self.program, self.descs, self.f64)
        with _hipcc.deferred():
            pw_so = codegen.build(self.program, f64=self.f64)
            fused_so = codegen.build_fused(self.program, self.descs[0], f64=self.f64) if want_fused else None
        self.kernel = codegen.PointwiseKernel(pw_so, self.f64)
        self.fusedk = None
        # the 8-wave build of the closure kernel (two waves per SIMD), built on first use for batches of at least
        # WIDE_MIN_POINTS points: None = not tried yet, False = not available / rejected
        self.fusedk_wide = None if (os.environ.get("NDQ_FUSED_WIDE", "1") != "0" and not _canary.STATUS["refuse_two_waves"]
                                    and not self.f64) else False
        self._self_check = os.environ.get("NDQ_SELF_CHECK", "1") != "0"
        self._verified = set()                       # id() of the closure-kernel variants that passed verify_fused
        if fused_so is not None:
            fk = codegen.FusedKernel(fused_so, self.f64)
            if fk.lib.ndq_fused_lds_bytes() <= 160 * 1024:       # K weight images + staging must fit one workgroup's LDS
                self.fusedk = fk
        self.flat = [FlatParams(n, self.device, dtype) for n in self.nets]
        # evaluation sites: (network, coordinate tuple) pairs; site k < n_nets is network k at its first tuple, further
        # sites (networks evaluated on a boundary as well: Neumann conditions) follow.  Stream arrays are per site.
        self.site_net = list(self.program.site_net)
        self.n_sites = len(self.site_net)
        self.vcoords = dict(self.program.g.vcoords)
        # rows of the stream / adjoint-stream arrays of site k: [n_streams][n_out]
        self.ns = [self.program.streams[k].n_streams * self.program.streams[k].n_out for k in range(self.n_sites)]
        self.site_deps = [tuple(self.program.streams[k].deps) for k in range(self.n_sites)]
        # a site whose inputs are a run of consecutive batch coordinates reads the batch block in place ...
        self.coord0 = [d[0] if all(c < n_coords for c in d) and list(d) == list(range(d[0], d[0] + len(d))) else None
                       for d in self.site_deps]                     # ... any other gets a gathered block of its own
        for k in range(self.n_sites):
            assert self.L.ndq_mlp_num_params(ctypes.byref(self.descs[k])) == self.flat[self.site_net[k]].numel
        self._bufs = {}
        self._resident_cache = {}
        self._static, self._static_seen = {}, {}
        self._dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.loss_buf = torch.zeros(64, dtype=dtype, device=self.device)
        if self.n_theta:
            self.theta_buf = torch.zeros(self.n_theta, dtype=dtype, device=self.device)
            self.gtheta = torch.zeros(self.n_theta, dtype=dtype, device=self.device)
            self.kernel.lib.ndq_pw_bind_theta.argtypes = [_c_vp, _c_vp]
            self.kernel.lib.ndq_pw_bind_theta.restype = None

    # ------------------------------------------------------------------------------------------ trainable scalars
    def set_batch_size(self, n_global):
        """The batch size as a number of the equations (`u / x.shape[0]`: symbolic.Graph.nbatch): the GLOBAL batch's point
        count -- what x.shape[0] is in the reference's closure (solvers.py:369-395) -- goes into its frozen kernel argument;
        refresh_theta uploads it when it changed."""
        t = getattr(self.program.g, "_nbatch_t", None)
        if t is not None:
            t.fill_(float(n_global))

    def refresh_theta(self):
        """Current values of the equations' trainable scalars -> the device vector the kernels read."""
        if self.n_theta:
            with torch.no_grad():
                def value(p):      # a 1-element tensor, or entry k of a tensor (symbolic.Graph.param_elem)
                    v = p[0].detach().reshape(-1)[p[1]] if isinstance(p, tuple) else p.detach().reshape(())
                    return v.to(self.device, self.dt)
                owned = self._theta_owned and self._theta_views_intact()
                if not self.theta_frozen:
                    if not owned:
                        self.theta_buf.copy_(torch.stack([value(p) for p in self.theta_params]))
                    return
                if self._theta_trainable and not owned:
                    live = torch.stack([value(self.theta_params[j]) for j in self._theta_trainable])
                    self.theta_buf[self._theta_trainable] = live
                values = tuple(float(self.theta_params[j]) for j in self.theta_frozen)
                if values != self._theta_frozen_seen:          # (one small H2D copy when a re-trace brought new values)
                    self._theta_frozen_seen = values
                    self.theta_buf[self.theta_frozen] = torch.tensor(values, dtype=self.dt).to(self.device)

    def _bind_theta(self, b, lib, fused):
        """Hand a kernel module the scalars' vector and the block-partial rows of this buffer set."""
        if self.n_theta:
            fn = lib.ndq_fused_bind_theta if fused else lib.ndq_pw_bind_theta
            fn(_ptr(self.theta_buf), _ptr(b["theta_partials"]))

    def reduce_theta(self, b, blocks, stream, accumulate):
        """Second stage of the scalars' gradient: fixed-order sum of the block partial rows -> ``gtheta``."""
        if self.n_theta:
            rc = self.L.ndq_reduce_partials(_ptr(b["theta_partials"]), blocks, self.n_theta, _ptr(self.gtheta),
                                            1 if accumulate else 0, 1.0, stream)
            _lib.check(rc, "ndq_reduce_partials(theta)")

    def attach_theta_grads(self):
        """``p.grad`` of every trainable scalar = its entry of ``gtheta`` (what loss.backward() leaves, solvers.py:393)."""
        for j, p in enumerate(self.theta_params):
            if j in self.program.g.frozen:
                continue
            if isinstance(p, tuple):             # entry k of a tensor (a symbolic skip connection's weight matrix)
                t, k = p
                if t.grad is None:
                    t.grad = torch.zeros_like(t)
                t.grad.reshape(-1)[k] = self.gtheta[j].to(t.device, t.dtype)
                continue
            g = self.gtheta[j].reshape(p.shape).to(p.device, p.dtype)
            if p.grad is not None and p.grad.shape == g.shape and p.grad.data_ptr() != self.gtheta[j].data_ptr():
                p.grad.copy_(g)
            else:
                p.grad = g.clone()       # never a view of the shared buffer: the next epoch rewrites gtheta in place

    # ---- the device owns the trainable scalars (the sums + tail launch steps them: fast_train_epoch_theta)
    def theta_tail_ready(self, optimizer, dist=None):
        """Can a one-batch training epoch of this inverse problem end on the device -- closure launch + ONE sums / tail launch
        that also reduces and steps the trainable scalars (``theta_tail_eligible``; NDQ_NO_THETA_TAIL=1 when the system was
        built: never)?  ``fast_ready()`` / ``fit_ready()`` keep their meaning."""
        return theta_tail_eligible(enabled=self.theta_tail, f64=self.f64, closure=self.fusedk is not None,
                                   sharded=dist is not None, device=self.device,
                                   scalars=[self.theta_params[j] for j in self._theta_trainable], n_theta=self.n_theta,
                                   optimizer=optimizer)

    def _theta_views_intact(self):
        base = self.theta_buf.data_ptr()
        return all(self.theta_params[j].data_ptr() == base + 4 * j for j in self._theta_trainable)

    def own_theta(self):
        """``theta_buf`` becomes authoritative: every trainable scalar's ``.data`` is a view of its element (as FlatParams does
        for network parameters), so an in-place edit by the user is what the next launch reads and what the tail writes is
        what ``k.item()`` shows; ``k.grad`` is a VIEW of ``gtheta[j]`` -- like the ``.grad`` views of network parameters it is
        rewritten in place by the next epoch (same stream, so never mid-read); a user who keeps a gradient clones it.
        Frozen entries keep refresh_theta's mechanism."""
        if not (self._theta_owned and self._theta_views_intact()):
            with torch.no_grad():
                for j in self._theta_trainable:
                    p = self.theta_params[j]
                    if p.data_ptr() != self.theta_buf.data_ptr() + 4 * j:
                        self.theta_buf[j:j + 1].copy_(p.detach().reshape(1))
                        p.data = self.theta_buf[j:j + 1].view(p.shape)
            self._theta_owned = True
        for j in self._theta_trainable:
            p = self.theta_params[j]
            if p.grad is None or p.grad.data_ptr() != self.gtheta.data_ptr() + 4 * j:
                p.grad = self.gtheta[j:j + 1].view(p.shape)

    def disown_theta(self):
        """Back to the general path (another optimiser, ...): the host-side values are authoritative again.  The views stay
        (a copy of a value onto itself is harmless); gradients become tensors of their own at the next attach_theta_grads."""
        self._theta_owned = False

    def fast_train_epoch_theta(self, batch, optimizer, adam_slots, track_best):
        """A one-batch training epoch of an inverse problem from ONE native call of two launches and no host synchronisation:
        closure kernel, then the sums + tail launch of all networks with the scalars as its last row
        (ndq_fused_theta_step_run for one network, ndq_fused_theta_multi_step_run for 2..4).  The caller has checked
        ``theta_tail_ready`` and that all networks are at one Adam step."""
        fs = self.fast_state()
        b, n = self.upload(batch)
        self.set_batch_size(n)
        self.own_theta()
        self.refresh_theta()                         # (frozen runtime constants only)
        K = len(self.flat)
        key = (n, b["ld"], id(b), "theta")
        ent = fs["structs"].get(key)
        if ent is None:
            arr = (_lib.FusedStep * K)()
            for k in range(K):
                self._fill_step(arr[k], k, n, b["ld"], b["fused_blocks"], b["fused_partials_all"][k], b["fused_loss_partials"])
            arr[0].launch = b["fused_launch"]
            th = _lib.ThetaStep()
            th.n_theta, th.frozen = self.n_theta, sum(1 << j for j in self.theta_frozen)
            th.theta, th.partials, th.gtheta = self.theta_buf.data_ptr(), b["theta_partials"].data_ptr(), self.gtheta.data_ptr()
            ent = fs["structs"][key] = (arr, th)
        arr, th = ent
        if not optimizer.scalars_bound(self):
            optimizer.bind_scalars(self, {j: self.theta_params[j] for j in self._theta_trainable}, self.n_theta, self.device)
        tm, tv, per_scalar = optimizer.theta_slot()
        th.adam_m, th.adam_v = tm.data_ptr(), tv.data_ptr()
        for j, group, tstep in per_scalar:
            th.lr[j], (th.beta1[j], th.beta2[j]), th.eps[j] = group["lr"], group["betas"], group["eps"]
            th.weight_decay[j], th.step[j] = group["weight_decay"], tstep
        step = adam_slots[0][3]
        for k, fp in enumerate(self.flat):
            fp.sync()
            m, v, group, _ = adam_slots[k]
            st = arr[k]
            st.params = fp.flat.data_ptr()
            st.seed = 1.0 / (float(n) * self.loss_norm)
            st.best_flat = fs["best_flat"][k].data_ptr() if track_best else None
            self._set_adam(st, m, v, group)
        self._bind_theta(b, b["fusedk"].lib, True)
        coords, stream = self._coord_ptr(b, 0), self._stream()
        if K == 1:
            rc = self.L.ndq_fused_theta_step_run(arr, ctypes.byref(th), coords, step, fs["pending"], fs["parity"], stream)
        else:
            rc = self.L.ndq_fused_theta_multi_step_run(arr, K, _c_vp(b["fused_launch_multi"]), ctypes.byref(th), coords, step,
                                                       fs["pending"], fs["parity"], stream)
        _lib.check(rc, "ndq_fused_theta_step_run")
        fs["pending"] += 1
        fs["parity"] ^= 1

    # ------------------------------------------------------------------------------------------ buffers
    def _resident_ld(self, batch):
        """Leading dimension if ``batch`` is rows of ONE contiguous fp32 SoA block (ResidentBatchGenerator), else 0."""
        if self.n_data or any(c.dtype != self.dt or not c.is_contiguous() for c in batch):
            return 0         # (data columns travel in the rows behind the coordinates: the block is assembled per batch)
        p0 = batch[0].data_ptr()
        if len(batch) == 1:
            return _round_up(batch[0].numel(), 64) if p0 % 16 == 0 else 0
        step = batch[1].data_ptr() - p0
        if step <= 0 or step % self.esize or step // self.esize < batch[0].numel():
            return 0
        if any(c.data_ptr() != p0 + i * step for i, c in enumerate(batch)):
            return 0
        return step // self.esize

    MAX_BUFFER_SETS = 8
    # Which build serves a batch: both run "rounds" of one 16-point tile per wave over 256 workgroups -- 1 024 waves
    # (4-wave build, one per SIMD) or 2 048 (8-wave build, two per SIMD).  Measured on the C2 step: 4-wave
    # 11.3 + 4.1 us per round (15.4 / 23.6 / 27.6 us at 1 / 3 / 4 rounds), 8-wave 12.8 + 6.7 us per round (26.2 us at 2
    # rounds for anything from 32 769 to 65 536 points, 66 us at 8).  So 65 536 points (4 vs 2 rounds) and everything from
    # ~115 k points up go to the 8-wave build, 33 k - 49 k and 66 k - 82 k points (3 vs 2, 5 vs 3 rounds) do not.
    WIDE_MIN_POINTS = int(os.environ.get("NDQ_FUSED_WIDE_MIN", 0))

    def _wide_possible(self):
        """Does csrc/ndq_mlp.h give this shape an 8-wave build at all?  (Cfg::BWD_THREADS: per-wave state of more than 40
        fragment blocks keeps the whole register file, i.e. 4 waves -- no point compiling to find that out)"""
        mode = codegen.MODES.get(codegen.fuse_mode(self.program, self.descs))
        if mode is not None and not mode.eight_wave:
            return False            # (the multi-row kernels: codegen.MODES says why)
        if mode is not None and mode.eight_wave_opt_in:
            return os.environ.get(mode.eight_wave_opt_in, "0") == "1"
        d = self.descs[0]
        nb, layers = (d.hidden + 15) // 16, d.layers
        ns = self.L.ndq_mlp_num_streams(ctypes.byref(d))
        return nb * nb * (layers - 1) + nb * ns * layers <= 40

    @staticmethod
    def prefers_wide(n):
        tiles = (n + 15) // 16
        r4, r8 = -(-tiles // 1024), -(-tiles // 2048)
        return 0.37 + 1.63 * r8 < r4

    def needs_check(self, n):
        """Has the closure-kernel build serving batches of ``n`` points still to pass verify_fused?"""
        fk = self.fused_variant(n) if self._self_check else None
        return fk is not None and id(fk) not in self._verified

    select_n = None     # data parallel: the LARGEST shard size of the current batch, identical on every rank, so that all
    #                     ranks choose -- and verify -- the same closure-kernel build (shard sizes may differ by one point)

    def fused_variant(self, n):
        """The closure-kernel build that serves a batch of ``n`` points (None: three-kernel pipeline)."""
        if self.fusedk is None:
            return None
        n = self.select_n or n
        memo = self.__dict__.get("_variant_memo")
        if memo is not None and memo[0] == n and memo[1] is self.fusedk_wide:
            return memo[2]                    # (asked three times per epoch)
        fk = self._fused_variant(n)
        if self.fusedk_wide is not None:      # the 8-wave build has been tried: the answer for this n is final
            self._variant_memo = (n, self.fusedk_wide, fk)
        return fk

    def _fused_variant(self, n):
        if n >= self.WIDE_MIN_POINTS and self.prefers_wide(n) and self.fusedk_wide is not False:
            if self.fusedk_wide is None and not self._wide_possible():
                self.fusedk_wide = False
            if self.fusedk_wide is None:
                wide = codegen.FusedKernel(codegen.build_fused(self.program, self.descs[0], threads=512))
                # shapes whose per-wave state needs the whole register file compile to the same 4-wave kernel
                ok = wide.threads > self.fusedk.threads and wide.lib.ndq_fused_lds_bytes() <= 160 * 1024
                self.fusedk_wide = wide if ok else False
            if self.fusedk_wide is not False:
                return self.fusedk_wide
        return self.fusedk

    def buffers(self, n, ld=None):
        key = (n, ld)
        b = self._bufs.get(key)
        if b is not None:
            self._bufs[key] = self._bufs.pop(key)           # most recently used last
            return b
        # batch sizes that change every epoch (FilterGenerator, ...) must not pile up buffer sets: keep the most
        # recently used few; an evicted set is freed once the launches that use it have drained (stream-ordered)
        while len(self._bufs) >= self.MAX_BUFFER_SETS:
            old = self._bufs.pop(next(iter(self._bufs)))
            fs = getattr(self, "_fast", None)
            if fs is not None:
                for k in [k for k in fs["structs"] if k[2] == id(old)]:
                    del fs["structs"][k]
            self._resident_cache = {k: v for k, v in self._resident_cache.items() if v[1] is not old}
        ld = ld or _round_up(n, 64)
        dev, f32 = self.device, self.dt              # (name kept: the working precision of this system)
        b = dict(ld=ld,
                 coords_own=torch.zeros(self.n_rows, ld, dtype=f32, device=dev),
                 # host staging ring: a pinned block may only be rewritten once its async H2D copy has completed
                 # (the native epoch path never synchronises, so the host can run several epochs ahead)
                 pinned=[torch.zeros(self.n_rows, ld, dtype=f32, device="cpu").pin_memory() for _ in range(4)],
                 pin_events=[None] * 4, pin_next=0,
                 jets=[torch.zeros(ns, ld, dtype=f32, device=dev) for ns in self.ns],
                 gbar=[torch.zeros(ns, ld, dtype=f32, device=dev) for ns in self.ns],
                 funcs=torch.zeros(self.n_funcs, ld, dtype=f32, device=dev),
                 resid=torch.zeros(max(self.n_eq, 1), ld, dtype=f32, device=dev),
                 pw_blocks=self.kernel.blocks(n))
        b["loss_partials"] = torch.zeros(b["pw_blocks"], dtype=f32, device=dev)
        b["bwd_blocks"] = [self.L.ndq_mlp_bwd_blocks(ctypes.byref(self.descs[k]), n) for k in range(self.n_sites)]
        b["partials"] = [torch.empty(nb, self.flat[self.site_net[k]].numel, dtype=f32, device=dev)
                         for k, nb in enumerate(b["bwd_blocks"])]
        # gathered coordinate blocks of the sites that do not read the batch block in place: virtual coordinates are
        # constant rows (filled here, once), real ones are copied in before every forward pass
        b["site_coords"] = {}
        for k, deps in enumerate(self.site_deps):
            if self.coord0[k] is None:
                blk = torch.zeros(len(deps), ld, dtype=f32, device=dev)
                for row, c in enumerate(deps):
                    if c in self.vcoords:
                        blk[row].fill_(self.vcoords[c])
                b["site_coords"][k] = blk
        fk = b["fusedk"] = self.fused_variant(n)
        if fk is not None:
            b["fused_launch"] = ctypes.cast(fk.lib.ndq_fused_launch, ctypes.c_void_p).value
            b["fused_launch_multi"] = ctypes.cast(fk.lib.ndq_fused_launch_multi, ctypes.c_void_p).value
            b["fused_blocks"] = fk.blocks(n)
            b["fused_partials_all"] = [torch.empty(b["fused_blocks"], fp.numel, dtype=f32, device=dev) for fp in self.flat]
            b["fused_partials"] = b["fused_partials_all"][0]
            b["fused_partials_pp"] = (_c_vp * len(self.nets))(*[t.data_ptr() for t in b["fused_partials_all"]])
            b["fused_loss_partials"] = torch.zeros(b["fused_blocks"], dtype=f32, device=dev)
        if self.n_theta:
            rows = max(b["pw_blocks"], b.get("fused_blocks", 0))
            b["theta_partials"] = torch.zeros(rows, self.n_theta, dtype=f32, device=dev)
        b["jets_pp"] = (_c_vp * self.n_sites)(*[t.data_ptr() for t in b["jets"]])
        b["gbar_pp"] = (_c_vp * self.n_sites)(*[t.data_ptr() for t in b["gbar"]])
        b["coords"], b["coords_rows"] = b["coords_own"], None
        self._bufs[key] = b
        return b

    def upload(self, batch, lo=0, hi=None):
        """Copy rows [lo, hi) of the sampled batch (list of (N, 1) or (N,) tensors) into the SoA device block."""
        n_all = batch[0].numel()
        hi = n_all if hi is None else hi
        n = hi - lo
        if batch[0].device.type == "cuda" and lo == 0 and hi == n_all:
            hit = self._resident_cache.get(id(batch))        # same list object served again by a resident generator
            if hit is not None and hit[0] is batch:
                b = hit[1]
                b["coords_rows"] = hit[2]
                return b, n
            ld = self._resident_ld(batch)
            if ld:
                b = self.buffers(n, ld=ld)
                b["coords"] = batch[0].reshape(-1)          # row 0 of the resident SoA block; rows are ld apart
                b["coords_rows"] = [c.reshape(-1) for c in batch]
                if len(self._resident_cache) < 64:
                    self._resident_cache[id(batch)] = (batch, b, b["coords_rows"])
                return b, n
        if batch[0].device.type != "cuda" and not self.n_data:
            hit = self._static_batch(batch, lo, hi, n)
            if hit is not None:
                return hit, n
        b = self.buffers(n)
        b["coords"], b["coords_rows"] = b["coords_own"], None
        if self.n_data:
            for col in self.data_cols:
                if col.numel() != n_all:
                    raise _lib.NdqError(f"a per-point data column of the equations has {col.numel()} entries, the batch "
                                        f"{n_all} points: data columns must be aligned with the generator's points")
            batch = list(batch) + [col.detach().to(batch[0].device) for col in self.data_cols]
        if batch[0].device.type == "cuda":
            for i, c in enumerate(batch):
                b["coords_own"][i, :n].copy_(c.detach().reshape(-1)[lo:hi])
        else:
            k = b["pin_next"]
            b["pin_next"] = (k + 1) % len(b["pinned"])
            if b["pin_events"][k] is not None:
                b["pin_events"][k].synchronize()
            pinned = b["pinned"][k]
            for i, c in enumerate(batch):
                pinned[i, :n].copy_(c.detach().reshape(-1)[lo:hi])
            b["coords_own"].copy_(pinned, non_blocking=True)
            ev = b["pin_events"][k] or torch.cuda.Event()
            ev.record(self._stream_obj())            # (Event.record() without a stream looks the current one up: 10 us)
            b["pin_events"][k] = ev
        return b, n

    def _stream(self):
        """hipStream_t of torch's current stream on this device as a ctypes pointer (the raw getter is ~10x cheaper
        than building a torch.cuda.Stream object, and this runs several times per epoch)."""
        return _c_vp(_raw_stream(self._dev_index))

    def _stream_obj(self):
        """torch's current stream on this device as a ``torch.cuda.Stream`` (for ``Event.record``): built once per raw stream
        -- ``torch.cuda.current_stream()`` costs ~10 us per call, the raw getter 0.3 us."""
        raw = _raw_stream(self._dev_index)
        c = self.__dict__.get("_stream_cache")
        if c is None or c[0] != raw:
            c = self._stream_cache = (raw, torch.cuda.current_stream(self.device))
        return c[1]

    @staticmethod
    def static_key(batch):
        """Identity of a host batch's contents (storage, offset, length, version counter); None for device batches."""
        if batch[0].device.type == "cuda":
            return None
        # (+ the first and the last value: an edit through `.data` / a numpy view -- a grid shifted or rescaled in place by a
        # callback -- bumps no version counter; two samples per column see every such edit that moves the ends, for ~1 us)
        return tuple((c.untyped_storage().data_ptr(), c.storage_offset(), c.numel(), c._version) + _ends(c) for c in batch)

    def _static_batch(self, batch, lo, hi, n):
        """Host batches that come back unchanged (static generators: 'equally-spaced' grids, StaticGenerator,
        PredefinedGenerator -- the default validation sets) are uploaded once and then read in place.  Identity =
        same storage, offset, length and torch version counter; the tensors of cached entries and of the last few
        candidates are kept alive, so an address can never come back with different contents."""
        key = self.static_key(batch) + (lo, hi)
        hit = self._static.get(key)
        if hit is not None:
            b = self.buffers(n, ld=hit[1].shape[1])
            b["coords"], b["coords_rows"] = hit[2][0], hit[2]
            return b
        if key in self._static_seen and len(self._static) < 16:      # second sighting: promote to a resident block
            ld = _round_up(n, 64)
            block = torch.zeros(self.n_coords, ld, dtype=self.dt, device=self.device)
            host = torch.stack([c.detach().reshape(-1)[lo:hi].to(self.dt) for c in batch])
            block[:, :n].copy_(host)
            rows = [block[i] for i in range(self.n_coords)]
            self._static[key] = (list(batch), block, rows)
            b = self.buffers(n, ld=ld)
            b["coords"], b["coords_rows"] = rows[0], rows
            return b
        self._static_seen[key] = list(batch)
        while len(self._static_seen) > 8:
            self._static_seen.pop(next(iter(self._static_seen)))
        return None

    def static_block(self, batch):
        """(device pointer, n, ld) of a resident copy of an unchanging HOST batch (list of coordinate columns): uploaded
        on first use, found again by storage identity + version counter (see ``_static_batch``)."""
        n = batch[0].numel()
        key = self.static_key(batch) + (0, n)
        hit = self._static.get(key)
        if hit is None:
            while len(self._static) >= 16:
                self._static.pop(next(iter(self._static)))
            ld = _round_up(n, 64)
            block = torch.zeros(self.n_coords, ld, dtype=self.dt, device=self.device)
            block[:, :n].copy_(torch.stack([c.detach().reshape(-1).to(self.dt) for c in batch]))
            hit = self._static[key] = (list(batch), block, [block[i] for i in range(self.n_coords)])
        return hit[2][0].data_ptr(), n, hit[1].shape[1]

    def _coord_ptr(self, b, row):
        if b["coords_rows"] is not None:
            return _c_vp(b["coords_rows"][row].data_ptr())
        return _c_vp(b["coords_own"][row].data_ptr())

    def coord_columns(self, b, n):
        if b["coords_rows"] is not None:
            return [c[:n].view(-1, 1) for c in b["coords_rows"]]
        return [b["coords_own"][i, :n].view(-1, 1) for i in range(self.n_coords)]

    def split_functions(self, rows):
        """[n_user_funcs][n] rows of the function buffer -> one (n, k) tensor per solver function (k = 1 except for a
        multi-column function such as EnsembleCondition on a multi-output network)."""
        out, r = [], 0
        for k in self.program.func_widths:
            out.append(rows[r].reshape(-1, 1) if k == 1 else rows[r:r + k].t())
            r += k
        return out

    def func_columns(self, b, n):
        return self.split_functions(b["funcs"][:self.n_user_funcs, :n])

    def metric_sums(self, b, n):
        """Sum over the (local) points of every traced metric's per-point term: device tensor [n_metrics]."""
        return b["funcs"][self.n_user_funcs:self.n_funcs, :n].sum(dim=1)

    # ------------------------------------------------------------------------------------------ launches
    def _site_coords(self, b, k, n, refresh):
        """Device pointer of site k's coordinate block [d][ld]: the batch block itself, or the site's gathered block
        (``refresh``: copy the real coordinate rows of the current batch in first)."""
        if self.coord0[k] is not None:
            return self._coord_ptr(b, self.coord0[k])
        blk = b["site_coords"][k]
        if refresh:
            for row, c in enumerate(self.site_deps[k]):
                if c not in self.vcoords:
                    src = b["coords_rows"][c] if b["coords_rows"] is not None else b["coords_own"][c]
                    blk[row, :n].copy_(src[:n])
        return _c_vp(blk.data_ptr())

    def forward(self, b, n, stream):
        for fp in self.flat:
            fp.sync()
        for k in range(self.n_sites):
            fp = self.flat[self.site_net[k]]
            rc = self.L.ndq_mlp_jet_fwd(ctypes.byref(self.descs[k]), self._site_coords(b, k, n, True), b["ld"], n,
                                        _ptr(fp.flat), _ptr(b["jets"][k]), b["ld"], stream)
            _lib.check(rc, "ndq_mlp_jet_fwd")

    def evaluate(self, coords):
        """Function values u_i(coords) through the forward-only kernels: list of n_coords tensors (any device, n
        elements each) -> device tensor [n_funcs][n].  Replaces BaseSolution._compute_u's torch forward
        (solvers.py:682-725)."""
        b, n = self.upload([c.reshape(-1) for c in coords])
        stream = self._stream()
        self.set_batch_size(n)
        self.refresh_theta()
        self.forward(b, n, stream)
        self.pointwise(b, n, stream, False, n, want_funcs=True)
        return b["funcs"][:self.n_user_funcs, :n]

    def residuals(self, coords):
        """Residual columns r_e(coords) of the traced PDE system: device tensor [n_eq][n] (get_residuals,
        solvers.py:606-646, without building an autograd graph)."""
        b, n = self.upload([c.reshape(-1) for c in coords])
        stream = self._stream()
        self.set_batch_size(n)
        self.refresh_theta()
        self.forward(b, n, stream)
        self.pointwise(b, n, stream, False, n, want_resid=True)
        return b["resid"][:, :n]

    def pointwise(self, b, n, stream, train, n_global, want_funcs=False, want_resid=False):
        seed = 1.0 / (float(n_global) * self.loss_norm)
        self._bind_theta(b, self.kernel.lib, False)
        rc = self.kernel.lib.ndq_pw_launch(self._coord_ptr(b, 0), b["ld"], n, b["jets_pp"],
                                           b["gbar_pp"] if train else None, b["ld"],
                                           _ptr(b["funcs"]) if want_funcs else None,
                                           _ptr(b["resid"]) if want_resid else None,
                                           _ptr(b["loss_partials"]), seed, stream)
        _lib.check(rc, "ndq_pw_launch")
        return seed

    def backward(self, b, n, stream, accumulate, after_forward=False):
        """after_forward: this call directly follows ``forward`` on the same batch and parameters (one training step).  The
        layer-by-layer kernels of deep wide networks (csrc/ndq_deep.h) then keep the activations their forward call left in
        the module's workspace instead of recomputing them (a module serves one evaluation site at a time: with several
        sites of one shape only the last forward is still there, the others recompute -- the module checks)."""
        seen = set()
        for k in range(self.n_sites):
            net = self.site_net[k]
            fp = self.flat[net]
            ext = codegen.mlp_ext_module(self.descs[k], self.f64) if after_forward else None
            hint = getattr(ext, "ndq_ext_reuse_forward", None) if ext is not None else None
            if hint is not None:
                hint(1)
            rc = self.L.ndq_mlp_jet_bwd(ctypes.byref(self.descs[k]), self._site_coords(b, k, n, False), b["ld"], n,
                                        _ptr(fp.flat), _ptr(b["gbar"][k]), b["ld"], _ptr(b["partials"][k]), stream)
            if hint is not None:
                hint(0)
            _lib.check(rc, "ndq_mlp_jet_bwd")
            # every site of a network adds into that network's gradient (the first one overwrites unless accumulating)
            rc = self.L.ndq_reduce_partials(_ptr(b["partials"][k]), b["bwd_blocks"][k], fp.numel, _ptr(fp.grad),
                                            1 if (accumulate or net in seen) else 0, 1.0, stream)
            _lib.check(rc, "ndq_reduce_partials")
            seen.add(net)

    def reduce_loss(self, b, stream, seed, slot):
        rc = self.L.ndq_reduce_partials(_ptr(b["loss_partials"]), b["pw_blocks"], 1,
                                        _c_vp(self.loss_buf.data_ptr() + self.esize * slot), 0, seed, stream)
        _lib.check(rc, "ndq_reduce_partials(loss)")

    def verify_fused(self, b, n, n_global=None):
        """First use of this system's single-launch closure kernel: run it twice and the three-kernel pipeline once on
        the batch at hand and compare the gradients.  The closure kernel is generated and compiled per system, its
        register allocation differs from build to build, and gfx950 has shown hazards the compiler does not know
         -- a kernel that is not bit-reproducible, or that disagrees with the independently compiled
        forward / pointwise / adjoint kernels, is not used: the system continues on the three-kernel pipeline (still
        all-HIP) with a warning.  One host synchronisation, once per system and kernel build (the 8-wave build for
        large batches is checked when it is first used; if only that one fails, the 4-wave build takes over);
        NDQ_SELF_CHECK=0 skips it.  Returns False if a build was rejected: ``b`` is then stale, upload again."""
        fk = b.get("fusedk")
        if fk is None or not self._self_check or id(fk) in self._verified:
            return True
        self._verified.add(id(fk))
        n_global = n if n_global is None else n_global
        stream = self._stream()
        keep = [fp.grad_loss.clone() for fp in self.flat], self.loss_buf[:1].clone()

        def grads():
            return (torch.cat([fp.grad for fp in self.flat] + ([self.gtheta] if self.n_theta else [])).clone(),
                    self.loss_buf[:1].clone())
        runs = []
        for _ in range(2):
            self.fused_closure(b, n, stream, True, n_global, 0, False)
            runs.append(grads())
        tv_same = self._tv_matches_plain(b, n, n_global, stream) if (self.FIT_RUN and not self.n_theta and not self.f64) else True
        pipe = []
        for _ in range(2):
            self.forward(b, n, stream)
            seed = self.pointwise(b, n, stream, True, n_global, False, False)
            self.backward(b, n, stream, False)
            self.reduce_theta(b, b["pw_blocks"], stream, False)
            self.reduce_loss(b, stream, seed, 0)
            pipe.append(grads())
        for fp, g in zip(self.flat, keep[0]):
            fp.grad_loss.copy_(g)
        self.loss_buf[:1].copy_(keep[1])
        if not all(bool(torch.isfinite(x).all()) for pair in runs + pipe for x in pair):
            # inf / nan on this batch (points far outside the domain, a diverged state): nan != nan, nothing can be compared.
            # The reference trains on -- to nan (solvers.py:369-395) --, and so does this path; the build stays unverified and
            # the next finite batch checks it
            self._verified.discard(id(fk))
            self.fused_check = dict(inconclusive="non-finite gradients / loss on the batch at hand")
            return True
        same = bool(torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]))
        pipe_same = bool(torch.equal(pipe[0][0], pipe[1][0]) and torch.equal(pipe[0][1], pipe[1][1]))
        ref = pipe[0][0].double()
        err = float((runs[0][0].double() - ref).norm() / ref.norm().clamp_min(1e-30))
        lerr = float((runs[0][1] - pipe[0][1]).abs() / pipe[0][1].abs().clamp_min(1e-30))
        self.fused_check = dict(reproducible=same, pipeline_reproducible=pipe_same, grad_rel_l2=err, loss_rel=lerr,
                                train_valid_launch_identical=tv_same)
        same = same and tv_same
        if os.environ.get("NDQ_SELF_CHECK_LOG"):          # evidence for SELF_CHECK_TOL: one JSON line per checked kernel
            import json
            with open(os.environ["NDQ_SELF_CHECK_LOG"], "a") as fh:
                fh.write(json.dumps(dict(self.fused_check, n=n, threads=fk.threads, nets=len(self.flat))) + "\n")
        if not pipe_same:
            raise _lib.NdqError(f"the three-kernel pipeline of this system is not bit-reproducible ({self.fused_check}); "
                                "refusing to train on it")
        if same and err < self.SELF_CHECK_TOL and lerr < self.SELF_CHECK_TOL:
            return True
        import warnings
        if fk is self.fusedk_wide:
            warnings.warn(f"8-wave closure kernel rejected by its self-check ({self.fused_check}); large batches of this "
                          "system use the 4-wave build as well", RuntimeWarning)
        else:
            warnings.warn(f"single-launch closure kernel rejected by its self-check ({self.fused_check}); this system "
                          "continues on the three-kernel pipeline", RuntimeWarning)
            self.fusedk = None
        self.fusedk_wide = False
        # buffer sets carry the build they were made for (block counts, partial-sum rows, launchers): start over
        self._bufs.clear()
        self._resident_cache.clear()
        self._fast = None
        return False

    def _tv_matches_plain(self, b, n, n_global, stream):
        """The train + validation launch of this closure-kernel build (fit(): several epochs per native call) against the
        plain launches it stands in for, on the batch at hand, bit for bit: gradient and loss partial sums of its
        training workgroups == the training launch (which has just run: ``b`` still holds its partial sums), loss
        partial sums of its validation workgroups == the forward-only launch; alone and together."""
        fk = b["fusedk"]
        dev, f32 = self.device, self.dt          # (the module's scalar type: double for an fp64 system)
        seed = 1.0 / (float(n_global) * self.loss_norm)
        params_pp = (_c_vp * len(self.flat))(*[fp.flat.data_ptr() for fp in self.flat])
        want_parts = [t.clone() for t in b["fused_partials_all"]]
        want_loss = b["fused_loss_partials"].clone()
        blocks = b["fused_blocks"]
        ev = torch.zeros(blocks, dtype=f32, device=dev)
        rc = fk.lib.ndq_fused_launch_multi(self._coord_ptr(b, 0), b["ld"], n, params_pp, None, _ptr(ev), None, None, b["ld"],
                                           seed, 0, stream)
        _lib.check(rc, "ndq_fused_launch_multi")
        ok = True
        for with_train, with_valid in ((True, True), (True, False), (False, True)):
            parts = [torch.full_like(t, float("nan")) for t in want_parts]
            lp = torch.full_like(want_loss, float("nan"))
            vp = torch.full_like(ev, float("nan"))
            parts_pp = (_c_vp * len(parts))(*[t.data_ptr() for t in parts])
            rc = fk.lib.ndq_fused_launch_tv(self._coord_ptr(b, 0) if with_train else None, b["ld"], n if with_train else 0,
                                            params_pp, parts_pp if with_train else None, _ptr(lp) if with_train else None,
                                            seed, self._coord_ptr(b, 0) if with_valid else None, b["ld"],
                                            n if with_valid else 0, _ptr(vp) if with_valid else None, None, stream)
            _lib.check(rc, "ndq_fused_launch_tv")
            if with_train:
                ok = ok and torch.equal(lp, want_loss) and all(torch.equal(a, w) for a, w in zip(parts, want_parts))
            if with_valid:
                ok = ok and torch.equal(vp, ev)
        return bool(ok)

    # closure kernel vs three-kernel pipeline on the first training batch: both are fp32 evaluations held to the 1e-5
    # contract, so they may differ by at most twice that.  Measured over the 190 closure kernels of the GPU test-suite
    # (profiles/archive/r03/r03c_self_check_distribution.json): median 1.6e-8, 99th percentile 7e-7, maximum 5.2e-6 (C2 at the
    # reference-trained state, where the residual is a cancellation and the reference's own fp32 gradient is 4e-4 off).
    SELF_CHECK_TOL = 2e-5

    def reject_fused(self):
        """Give up the single-launch closure kernel of this system (all builds): three-kernel pipeline from here on."""
        self.fusedk, self.fusedk_wide, self._fast = None, False, None
        self._bufs.clear()
        self._resident_cache.clear()

    def verify_on(self, batch, n_global=None, lo=0, hi=None):
        b, n = self.upload(batch, lo, hi)
        self.set_batch_size(n if n_global is None else n_global)      # (scalar arguments of the equations: as step() does)
        self.refresh_theta()
        ok = self.verify_fused(b, n, n_global)
        if batch[0].device.type != "cuda":       # the epoch uploads this batch again: not a sign of a static generator
            self._static_seen.pop(self.static_key(batch) + (lo, batch[0].numel() if hi is None else hi), None)
        return ok

    def fused_closure(self, b, n, stream, train, n_global, slot, accumulate, want_funcs=False, want_resid=False):
        """The whole closure in ONE launch (one network, or 2..4 networks of one shape -- up to 48 units, or one hidden layer
        of 65 .. 512), then the fixed-order second-stage sums, network by network."""
        for fp in self.flat:
            fp.sync()
        seed = 1.0 / (float(n_global) * self.loss_norm)
        params_pp = (_c_vp * len(self.flat))(*[fp.flat.data_ptr() for fp in self.flat])
        self._bind_theta(b, b["fusedk"].lib, True)
        rc = b["fusedk"].lib.ndq_fused_launch_multi(self._coord_ptr(b, 0), b["ld"], n, params_pp,
                                                    b["fused_partials_pp"] if train else None,
                                                    _ptr(b["fused_loss_partials"]),
                                                    _ptr(b["funcs"]) if want_funcs else None,
                                                    _ptr(b["resid"]) if want_resid else None, b["ld"], seed,
                                                    1 if train else 0, stream)
        _lib.check(rc, "ndq_fused_launch_multi")
        if train:
            for fp, part in zip(self.flat, b["fused_partials_all"]):
                rc = self.L.ndq_reduce_partials(_ptr(part), b["fused_blocks"], fp.numel, _ptr(fp.grad),
                                                1 if accumulate else 0, 1.0, stream)
                _lib.check(rc, "ndq_reduce_partials")
            self.reduce_theta(b, b["fused_blocks"], stream, accumulate)
        rc = self.L.ndq_reduce_partials(_ptr(b["fused_loss_partials"]), b["fused_blocks"], 1,
                                        _c_vp(self.loss_buf.data_ptr() + self.esize * slot), 0, seed, stream)
        _lib.check(rc, "ndq_reduce_partials(loss)")

    # ------------------------------------------------------------------------------------------ native epoch
    HIST = 8192

    def fast_ready(self, dist=None):
        """Can a whole training epoch go through one native call?  (single-launch closure; the data-parallel hook exists
        for one network only).  Systems with scalar arguments of the equations (``n_theta``) are not served by THESE calls:
        with trainable ones owned by a FusedAdam the epoch goes through ``fast_train_epoch_theta`` (``theta_tail_ready``)."""
        return self.fusedk is not None and (len(self.nets) == 1 or dist is None) and not self.f64 and not self.n_theta

    def f64_tail_ready(self):
        """Can a training epoch of this fp64 system (one batch, no data-parallel shard, all networks at one Adam step -- the
        caller's part of the condition) go through ``ndq64_fused_step_run``: the closure launch + ONE sums / tail launch in
        double?  Opt-in (NDQ_F64_FUSED_TAIL=1 when the system was built); ``fast_ready()`` keeps its meaning."""
        return self.f64 and self.f64_fused_tail and self.fusedk is not None and not self.n_theta

    def launches_per_step(self):
        """Kernel launches of one native training epoch with one batch (bench.py reports it per config)."""
        if self.f64_tail_ready():
            return 2                                     # closure kernel + ONE sums/tail kernel in double (all networks)
        if self.fusedk is not None and self.f64:
            # closure kernel, loss sum; per network: gradient sum, epoch tail (in double) -- 4 for one network, 6 for two
            return 2 + 2 * len(self.flat)
        if self.fusedk is not None:
            return 2                                     # closure kernel + ONE sums/tail kernel (all networks)
        # pipeline: forward per site, pointwise, (adjoint + sums) per site, loss sum, epoch tail per network
        total = 1 + 1 + len(self.flat)
        for k in range(self.n_sites):
            d = self.descs[k]
            if d.hidden > 64 and d.layers >= 2:
                # deep wide networks (csrc/ndq_launch.h: deep_kernels_fwd / deep_kernels_bwd) are SEQUENCES of launches: weight
                # planes + one GEMM per hidden layer 2..L (the last one writes the output streams when one chunk holds all
                # units, else + the head kernel); adjoint: (head pass above 128 units) + per layer 2..L one weight-gradient and
                # one reverse GEMM + ONE sum of all partial rows; + the entry's own gradient-row sum
                wide_head = 1 if d.hidden > 128 else 0          # (hidden = the widest layer)
                total += (1 + (d.layers - 1) + wide_head) + (wide_head + 2 * (d.layers - 1) + 1) + 1
            else:
                total += 1 + 2
        return total

    def fast_state(self):
        """Device-side epoch bookkeeping of the native fast path: loss ring, best-loss ping-pong, best snapshot."""
        if getattr(self, "_fast", None) is None:
            dev, f32 = self.device, self.dt        # (fp64 systems keep their bookkeeping in double: ndq64_epoch_tail)
            self._fast = dict(loss_hist=torch.zeros(self.HIST, dtype=f32, device=dev),
                              valid_hist=torch.zeros(self.HIST, dtype=f32, device=dev),
                              best_loss=torch.full((2,), float("inf"), dtype=f32, device=dev),
                              best_flat=[torch.zeros_like(fp.grad) for fp in self.flat], parity=0, pending=0,
                              pending_valid=0, structs={})
        return self._fast

    def _fill_step(self, st, k, n, ld, blocks, partials, loss_partials):
        """The batch-invariant fields of network k's ``_lib.FusedStep``: sizes, partial rows, where the reduced gradient,
        the epoch loss and the epoch bookkeeping go."""
        fs, fp = self.fast_state(), self.flat[k]
        st.n, st.ldc, st.ldj, st.blocks, st.n_params = n, ld, ld, blocks, fp.numel
        if partials is not None:
            st.partials, st.loss_partials = partials.data_ptr(), loss_partials.data_ptr()
        st.grad, st.loss_slot = fp.grad.data_ptr(), fp.grad_loss.data_ptr() + self.esize * fp.numel
        st.loss_hist, st.best_loss = fs["loss_hist"].data_ptr(), fs["best_loss"].data_ptr()

    @staticmethod
    def _set_adam(st, m, v, group):
        """An Adam slot (FusedAdam.fast_slot: moments + parameter group) into a ``_lib.FusedStep``."""
        st.adam_m, st.adam_v = m.data_ptr(), v.data_ptr()
        (st.beta1, st.beta2), st.lr, st.eps, st.weight_decay = group["betas"], group["lr"], group["eps"], group["weight_decay"]

    @staticmethod
    def _tail_args(fp, adam_slot):
        """The leading arguments of ndq_epoch_tail for one network: parameters, gradient, Adam slot (None: a validation epoch)."""
        if adam_slot is None:
            return _ptr(fp.flat), None, None, None, fp.numel, 0.0, 0.0, 0.0, 0.0, 0.0, 1
        m, v, group, step = adam_slot
        return (_ptr(fp.flat), _ptr(fp.grad), _ptr(m), _ptr(v), fp.numel, group["lr"], *group["betas"], group["eps"],
                group["weight_decay"], step)

    def epoch_tail(self, kind, n_batches, track_best, adam_slots=None):
        """Device-side end of an epoch for ANY fused system (pipeline or single-launch), after the per-batch
        ``step()`` calls filled ``loss_buf[:n_batches]`` and the gradient buffers: mean loss -> history ring, best
        snapshot of every network when ``track_best``, and -- training epochs -- the fused Adam update of every
        network (adam_slots[k] = FusedAdam.fast_slot(flat[k])).  No host synchronisation."""
        fs = self.fast_state()
        stream = self._stream()
        train = kind == "train"
        hist = fs["loss_hist"] if train else fs["valid_hist"]
        idx = fs["pending"] if train else fs["pending_valid"]
        parity = fs["parity"]
        for k, fp in enumerate(self.flat):
            fp.sync()
            args = self._tail_args(fp, adam_slots[k] if train else None)
            rc = self.L.ndq_epoch_tail(*args, _ptr(self.loss_buf), n_batches, _ptr(hist), idx, _ptr(fs["best_loss"]),
                                       parity, _ptr(fs["best_flat"][k]) if track_best else None, 1 if k == 0 else 0,
                                       stream)
            _lib.check(rc, "ndq_epoch_tail")
        if train:
            fs["pending"] += 1
        else:
            fs["pending_valid"] += 1
        fs["parity"] ^= 1

    def fast_train_epoch_nets(self, batch, adam_slots, track_best):
        """A training epoch of all networks behind ONE closure launch from one native call: closure kernel, then one sums +
        tail launch for all networks.  fp32 (2..4 networks, ``fast_ready``): ndq_fused_multi_step_run.  fp64 (1..4 networks,
        ``f64_tail_ready``): ndq64_fused_step_run, which leaves, bit for bit, what step() + epoch_tail() leave -- the loss in
        ``loss_buf[0]`` included.  The caller has checked that all networks are at one Adam step (slot 0's is used)."""
        fs = self.fast_state()
        b, n = self.upload(batch)
        K = len(self.flat)
        step_type, run = (_lib.FusedStep64, "ndq64_fused_step_run") if self.f64 else (_lib.FusedStep, "ndq_fused_multi_step_run")
        key = (n, b["ld"], id(b), "f64" if self.f64 else "multi")
        arr = fs["structs"].get(key)
        if arr is None:
            arr = (step_type * K)()
            for k in range(K):
                self._fill_step(arr[k], k, n, b["ld"], b["fused_blocks"], b["fused_partials_all"][k], b["fused_loss_partials"])
            fs["structs"][key] = arr
        step = adam_slots[0][3]
        for k, fp in enumerate(self.flat):
            fp.sync()
            m, v, group, _ = adam_slots[k]
            st = arr[k]
            st.params = fp.flat.data_ptr()
            st.seed = 1.0 / (float(n) * self.loss_norm)
            if self.f64:
                st.loss_slot = self.loss_buf.data_ptr()      # (where the step() + epoch_tail() route keeps the loss of batch 0)
            st.best_flat = fs["best_flat"][k].data_ptr() if track_best else None
            self._set_adam(st, m, v, group)
        rc = getattr(self.L, run)(arr, K, _c_vp(b["fused_launch_multi"]), self._coord_ptr(b, 0), step, fs["pending"], fs["parity"],
                                  self._stream())
        _lib.check(rc, run)
        fs["pending"] += 1
        fs["parity"] ^= 1

    def fast_train_epoch(self, batch, optimizer, adam_slot, track_best, n_global=None, dist=None):
        """One whole training epoch (n_batches = 1) of a single-network system with zero host synchronisation:
        closure kernel -> fused second-stage sums [-> all-reduce] -> device-side epoch tail (loss history, best
        snapshot, Adam).  ``adam_slot`` = (exp_avg, exp_avg_sq, group dict, step count AFTER this update)."""
        fs = self.fast_state()
        b, n = self.upload(batch)
        fp = self.flat[0]
        fp.sync()
        m, v, group, step = adam_slot
        key = (n, b["ld"], id(b))
        st = fs["structs"].get(key)
        if st is None:
            st = _lib.FusedStep()
            st.launch = b["fused_launch"]
            self._fill_step(st, 0, n, b["ld"], b["fused_blocks"], b["fused_partials"], b["fused_loss_partials"])
            fs["structs"][key] = st
        n_global = n if n_global is None else n_global
        st.params = fp.flat.data_ptr()
        st.seed = 1.0 / (float(n_global) * self.loss_norm)
        st.best_flat = fs["best_flat"][0].data_ptr() if track_best else None
        self._set_adam(st, m, v, group)
        stream = self._stream()
        coords = self._coord_ptr(b, 0)
        hist_index, parity = fs["pending"], fs["parity"]
        # a prefetching DeviceGenerator: the tail kernel's extra workgroups draw the next batch into the block this
        # step's closure kernel has just read (single GPU only: the data-parallel tail is a different kernel)
        src = generators.device_source(batch) if dist is None else None
        if src is not None and src.prefetch and b["coords_rows"] is not None:
            st.next_sampler = ctypes.addressof(src.desc)
            st.next_seed, st.next_draw, st.next_stream = src.seed, src.draw, src.stream_id
            nxt = src.block_of(src.draw)              # (src.draw is the NEXT draw number: the other block of the pair)
            st.next_coords, st.next_ldc = nxt.data_ptr(), nxt.shape[1]
        else:
            src, st.next_sampler = None, None
        direct = dist.direct(self.device, fp.numel + 1) if dist is not None else None
        if dist is None or direct is not None:
            # one native call; with data parallelism the RCCL all-reduce of [grad | loss] is enqueued by it, on the
            # same stream, between the local sums and the tail
            st.allreduce, st.comm = direct if direct is not None else (None, None)
            rc = self.L.ndq_fused_step_run(ctypes.byref(st), coords, step, hist_index, parity, stream)
            _lib.check(rc, "ndq_fused_step_run")
            if src is not None:
                src.prefetched = src.draw
        else:
            st.adam_m = st.adam_v = None
            st.allreduce = st.comm = None
            rc = self.L.ndq_fused_step_run(ctypes.byref(st), coords, step, hist_index, parity, stream)
            _lib.check(rc, "ndq_fused_step_run")
            dist.all_reduce_flat(fp.grad_loss)
            rc = self.L.ndq_epoch_tail(*self._tail_args(fp, adam_slot), _c_vp(st.loss_slot), 1, _ptr(fs["loss_hist"]),
                                       hist_index, _ptr(fs["best_loss"]), parity,
                                       _ptr(fs["best_flat"][0]) if track_best else None, 1, stream)
            _lib.check(rc, "ndq_epoch_tail")
        fs["pending"] += 1
        fs["parity"] ^= 1

    # ------------------------------------------------------------------------------------------ several epochs per call
    FIT_RUN = os.environ.get("NDQ_FIT_RUN", "1") != "0"
    FIT_PULL = os.environ.get("NDQ_FIT_PULL", "1") != "0"      # one launch per epoch for small grids (pull prologue)
    FIT_LOOP = os.environ.get("NDQ_FIT_LOOP", "1") != "0"      # one launch per RUN of epochs for one-workgroup grids

    def fit_ready(self):
        """May epochs of this system go through ndq_fused_fit_run (closure launch with training + validation workgroups,
        one sums / tail launch per epoch, any number of epochs per native call)?  Single GPU, single-launch closure."""
        return self.FIT_RUN and self.fusedk is not None and not self.f64 and not self.n_theta

    def resident_ptr(self, batch):
        """(device pointer of row 0, leading dimension) if ``batch`` -- a list of (N, 1) / (N,) coordinate columns -- is the
        rows of ONE resident fp32 SoA block the kernels can read in place (ResidentBatchGenerator, blocks staged by
        ``stage_batches``), else None."""
        if batch[0].device.type != "cuda" or len(batch) != self.n_coords:
            return None
        ld = self._resident_ld(batch)
        return (batch[0].data_ptr(), ld) if ld else None

    def stage_batches(self, host_block, n, reserve=0):
        """Host tensor [K][n_coords][n] (any float dtype) -> resident fp32 device block [K][n_coords][ld]: ONE pinned copy
        and ONE asynchronous H2D transfer for K epochs' worth of collocation points.  Returns (block, ld).  Two pinned
        staging blocks alternate; one is rewritten only after its previous transfer has completed.  ``reserve``: the
        largest K the caller will come with -- both blocks are allocated once, for that (page-locking memory costs
        milliseconds, measured up to 65 ms: not something to repeat as the chunks grow)."""
        K = host_block.shape[0]
        ld = _round_up(n, 64)
        st = self.__dict__.setdefault("_stage", dict(pinned=[None, None], events=[None, None], next=0, dev=[None, None]))
        i = st["next"]
        st["next"] ^= 1
        need = K * self.n_coords * ld
        if st["pinned"][i] is None or st["pinned"][i].numel() < need:
            if st["events"][i] is not None:
                st["events"][i].synchronize()
            size = max(need, reserve * self.n_coords * ld)
            for j in (0, 1):
                if st["pinned"][j] is None or st["pinned"][j].numel() < size:
                    if st["events"][j] is not None:
                        st["events"][j].synchronize()
                    st["pinned"][j] = torch.zeros(size, dtype=torch.float32, device="cpu", pin_memory=True)
                    st["dev"][j] = torch.zeros(size, dtype=torch.float32, device=self.device)
        elif st["events"][i] is not None:
            st["events"][i].synchronize()
        pinned = st["pinned"][i][:need].view(K, self.n_coords, ld)
        # (numpy: a strided / converting torch copy of this size goes through the intra-op thread pool, whose wake-up
        # costs more than the copy)
        import numpy as np
        np.copyto(pinned.numpy()[:, :, :n], host_block.detach().numpy(), casting="same_kind")
        dev = st["dev"][i][:need].view(K, self.n_coords, ld)
        dev.copy_(pinned, non_blocking=True)
        ev = st["events"][i] or torch.cuda.Event()
        ev.record()
        st["events"][i] = ev
        return dev, ld

    def fit_run(self, train_ptrs, n, ld, adam_slots, valid=None, track_best=0, n_global=None):
        """``len(train_ptrs)`` training epochs (n_batches_train = 1; ``train_ptrs[e]`` = device pointer of epoch e's resident
        [n_coords][ld] batch of ``n`` points) and -- ``valid = (ptr, n_valid, ld_valid)`` -- the validation epoch after each of
        them, through ONE native call (include/ndq.h: ndq_fused_fit_run; no host synchronisation).  No training pointers
        + ``valid``: one stand-alone validation epoch.  ``adam_slots[k]`` = (exp_avg, exp_avg_sq, group, step AFTER the
        first update) per network; ``track_best``: 0 none, 1 lowest training loss, 2 lowest validation loss."""
        fs = self.fast_state()
        K = len(train_ptrs)
        if K:
            self._fit_last_n = n
        # the closure-kernel build follows the TRAINING batch size; stand-alone validation epochs use the build of the
        # training epochs around them, so that a validation loss does not depend on how epochs are grouped into calls
        fk = self.fused_variant(n if K else (getattr(self, "_fit_last_n", None) or valid[1]))
        key = (id(fk), n if K else 0, ld if K else 0, (valid[1], valid[2]) if valid else None)
        cache = fs.setdefault("fit", {})
        ent = cache.get(key)
        if ent is None:
            if len(cache) >= 8:
                cache.pop(next(iter(cache)))
            dev, f32 = self.device, torch.float32
            ff = _lib.FusedFit()
            ff.launch = ctypes.cast(fk.lib.ndq_fused_launch_tv, ctypes.c_void_p).value
            ff.n_nets = len(self.flat)
            keep = []
            blocks = fk.blocks(n) if K else 0
            lparts = torch.zeros(max(blocks, 1), dtype=f32, device=dev)
            keep.append(lparts)
            for k, fp in enumerate(self.flat):
                part = torch.empty(blocks, fp.numel, dtype=f32, device=dev) if K else None
                keep.append(part)
                self._fill_step(ff.net[k], k, *((n, ld, blocks) if K else (0, 0, 0)), part, lparts)
                ff.net[k].best_flat = fs["best_flat"][k].data_ptr()
            if valid is not None:
                vparts = torch.zeros(fk.blocks(valid[1]), dtype=f32, device=dev)
                keep.append(vparts)
                ff.valid_n, ff.valid_ldc, ff.valid_blocks = valid[1], valid[2], vparts.numel()
                ff.valid_scale = 1.0 / (float(valid[1]) * self.loss_norm)
                ff.valid_loss_partials, ff.valid_hist = vparts.data_ptr(), fs["valid_hist"].data_ptr()
            # pull mode (small grids: the closure launch of an epoch finishes the previous one itself, one launch per epoch;
            # include/ndq.h): a second set of state / partial buffers
            ff.pull_ok = 0
            if K and self.FIT_PULL and 0 < blocks * len(self.flat) <= 16 and fk.lib.ndq_fused_pull_ok():   # ndq_tail.h: kPullMaxWork
                ff.pull_ok = 1
                for k, fp in enumerate(self.flat):
                    alt = [torch.zeros(fp.numel, dtype=f32, device=dev) for _ in range(3)]
                    apart = torch.empty(blocks, fp.numel, dtype=f32, device=dev)
                    keep.extend(alt + [apart])
                    ff.alt_params[k], ff.alt_m[k], ff.alt_v[k] = (t.data_ptr() for t in alt)
                    ff.alt_partials[k] = apart.data_ptr()
                alp = torch.zeros(max(blocks, 1), dtype=f32, device=dev)
                keep.append(alp)
                ff.alt_loss_partials = alp.data_ptr()
                if valid is not None:
                    avp = torch.zeros(ff.valid_blocks, dtype=f32, device=dev)
                    keep.append(avp)
                    ff.alt_valid_loss_partials = avp.data_ptr()
                # loop mode (one workgroup for the training grid, one for the validation grid: a run of epochs is one launch)
                if self.FIT_LOOP and blocks == 1 and (valid is None or ff.valid_blocks == 1) and len(self.flat) <= 2 \
                        and fk.lib.ndq_fused_loop_ok():
                    ff.launch_loop = ctypes.cast(fk.lib.ndq_fused_launch_loop, ctypes.c_void_p).value
                    ff.loop_ok = 1
            ent = cache[key] = (ff, keep, fk, {}, (_c_vp * 1)(), ctypes.byref(ff))
        ff = ent[0]
        step0 = 1
        # (this runs once per epoch on the per-epoch path, where the HOST is the bottleneck at the headline size: ctypes
        # struct fields are rewritten only when their values changed)
        last = ent[3]
        for k, fp in enumerate(self.flat):
            fp.sync()
            if K:
                m, v, group, step0 = adam_slots[k]
                now = (fp.flat.data_ptr(), n if n_global is None else n_global, m.data_ptr(), v.data_ptr(), group["lr"],
                       group["betas"], group["eps"], group["weight_decay"])
            else:
                now = (fp.flat.data_ptr(),)
            if last.get(k) != now:
                last[k] = now
                st = ff.net[k]
                st.params = now[0]
                if K:
                    st.seed = 1.0 / (float(now[1]) * self.loss_norm)
                    self._set_adam(st, m, v, group)
        vc = valid[0] if valid is not None else None
        if last.get("v") != (vc, track_best):
            last["v"] = (vc, track_best)
            ff.valid_coords = vc
            ff.track_best = track_best
        if K == 1:
            coords = ent[4]
            coords[0] = train_ptrs[0]
        else:
            coords = (_c_vp * max(K, 1))(*train_ptrs) if K else None
        rc = self.L.ndq_fused_fit_run(ent[5], K, coords, step0, fs["pending"], fs["pending_valid"], fs["parity"],
                                      self._stream())
        _lib.check(rc, "ndq_fused_fit_run")
        tails = K + (1 if valid is not None else 0)
        fs["pending"] += K
        if valid is not None:
            fs["pending_valid"] += max(K, 1)
        fs["parity"] ^= tails & 1

    def fast_flush(self):
        """Read back (ONE synchronising copy) the train / valid epoch losses recorded since the last flush and the
        best loss: returns (train_losses, valid_losses, best_loss)."""
        fs = getattr(self, "_fast", None)
        if fs is None or (fs["pending"] == 0 and fs["pending_valid"] == 0):
            return [], [], None
        k, kv = fs["pending"], fs["pending_valid"]
        vals = torch.cat([fs["loss_hist"][:k], fs["valid_hist"][:kv],
                          fs["best_loss"][fs["parity"]:fs["parity"] + 1]]).tolist()
        fs["pending"] = fs["pending_valid"] = 0
        return vals[:k], vals[k:k + kv], vals[k + kv]

    def step(self, batch, train, slot=0, accumulate=False, n_global=None, lo=0, hi=None, want_funcs=False,
             want_resid=False):
        """One closure evaluation (solvers.py:369-395) on rows [lo, hi) of ``batch``; the (shard of the) mean squared
        residual lands in ``loss_buf[slot]`` and, when ``train``, parameter gradients in every ``FlatParams.grad``."""
        b, n = self.upload(batch, lo, hi)
        n_global = n if n_global is None else n_global
        stream = self._stream()
        self.set_batch_size(n_global)
        self.refresh_theta()
        if train and not accumulate and not self.verify_fused(b, n, n_global):
            b, n = self.upload(batch, lo, hi)            # a closure-kernel build was rejected: fresh buffer set
        if b["fusedk"] is not None:
            self.fused_closure(b, n, stream, train, n_global, slot, accumulate, want_funcs, want_resid)
            return b, n
        self.forward(b, n, stream)
        seed = self.pointwise(b, n, stream, train, n_global, want_funcs, want_resid)
        if train:
            self.backward(b, n, stream, accumulate, after_forward=True)
            self.reduce_theta(b, b["pw_blocks"], stream, accumulate)
        self.reduce_loss(b, stream, seed, slot)
        return b, n
