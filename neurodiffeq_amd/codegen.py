"""HIP code generation for the traced pointwise stage (see :mod:`neurodiffeq_amd.symbolic`).

One generated kernel per traced PDE system does, per collocation point, everything the reference does between the
network forward and the parameter backward: condition re-parameterisation (conditions.py ``parameterize``), the
user's residuals (``diff_eqs``, solvers.py:380, with every ``diff`` already resolved symbolically), the squared
residual sum for the loss (solvers.py:218) and the adjoint of that loss w.r.t. every network output stream -- the
seed of ``loss.backward()`` (solvers.py:393).  It is the HBM-bound kernel of the path: it reads the coordinates and
the streams, writes the adjoint streams (+ optionally function values / residuals) and one partial sum per block.

The launcher it exports has the ``ndq_pointwise_fn`` signature of include/ndq.h.
"""
import ctypes
import hashlib
import os
import re
from collections import namedtuple

from .symbolic import Graph, TraceUnsupported

HERE = os.path.dirname(os.path.abspath(__file__))
JIT_DIR = os.path.join(HERE, "_jit")
from . import _hipcc        # noqa: E402  (hipcc + the device-assembly fix-up pass; see _hipcc.py)


def _extra_flags():
    """Tuning knobs for experiments: NDQ_JIT_FLAGS="-DNDQ_X=1 ..." is appended to hipcc and hashed into the cache key."""
    return os.environ.get("NDQ_JIT_FLAGS", "").split()


# ----------------------------------------------------------------------------------------------- stream layout
def pair_list(d):
    return [(a, b) for a in range(d) for b in range(a, d)]


def triple_list(d):
    return [(a, b, c) for a in range(d) for b in range(a, d) for c in range(b, d)]


#: bf16 plane products of the single-launch closure kernels' GEMMs (csrc/ndq_mlp.h: NDQ_FWD_NPROD / NDQ_HBAR_NPROD / NDQ_WG_NPROD):
#: forward 6 (the derivative streams keep fp32 class: 5 puts u_xx of the reference's trained C3 state at 3.2e-5), reverse 4,
#: weight gradients 3 -- measured against the unmodified reference's fp64 numbers in profiles/r06_headline_ab.md.  The generic
#: adjoint kernels behind the C-ABI keep all six (arbitrary seeds).  NDQ_JIT_FLAGS may override (A/B runs).
CLOSURE_PRODUCTS = ("#ifndef NDQ_HBAR_NPROD\n#define NDQ_HBAR_NPROD 4\n#endif\n"
                    "#ifndef NDQ_WG_NPROD\n#define NDQ_WG_NPROD 3\n#endif\n")


def quad_list(d):
    return [(a, b, c, e) for a in range(d) for b in range(a, d) for c in range(b, d) for e in range(c, d)]


def _m4_arg(desc):
    """Trailing template argument of ndq::Cfg for fourth-order streams -- appended only when there are any, so that the
    generated source (and with it the build cache key) of every other module stays what it was."""
    return f", {desc.mask4}u" if getattr(desc, "mask4", 0) else ""


class NetStreams:
    """Which derivative streams of net ``k`` the residual needs, closed to a set the MLP kernels provide.

    deps: global coordinate indices fed to the net (in order).  Stream slots follow include/ndq.h."""

    def __init__(self, deps, n_out):
        self.deps = tuple(deps)
        self.d = len(deps)
        self.n_out = n_out
        self.first = 0
        self.mask2 = 0
        self.mask3 = 0          # third-order triples (include/ndq.h: ndq_mlp_desc.mask3)
        self.mask4 = 0          # fourth-order quadruples (ndq_mlp_desc.mask4; round 6)
        self.lap = 0            # 1: the diagonal pairs of mask2 travel as ONE stream holding their sum

    def need(self, mi):
        """mi: multi-index of GLOBAL coordinate indices, or ("L", a, b, ..) for the Laplacian stream."""
        if mi and mi[0] == "L":
            self.first, self.lap = 1, 1
            for c in mi[1:]:
                a = self.deps.index(c)
                self.mask2 |= 1 << pair_list(self.d).index((a, a))
            return
        loc = tuple(sorted(self.deps.index(c) for c in mi))
        if len(loc) >= 1:
            self.first = 1
        if len(loc) == 2:
            self.mask2 |= 1 << pair_list(self.d).index(loc)
        if len(loc) == 3:               # a triple travels with its three pairs (the recurrence needs them)
            self.mask3 |= 1 << triple_list(self.d).index(loc)
            for pair in ((loc[0], loc[1]), (loc[0], loc[2]), (loc[1], loc[2])):
                self.mask2 |= 1 << pair_list(self.d).index(pair)
        if len(loc) == 4:               # a quadruple travels with its four triples and six pairs (Faa di Bruno over the positions)
            if self.d > 3:
                raise TraceUnsupported("fourth-order derivatives of a network with more than three inputs are outside the fused path")
            self.mask4 |= 1 << quad_list(self.d).index(loc)
            for i in range(4):
                tri = tuple(loc[j] for j in range(4) if j != i)
                self.mask3 |= 1 << triple_list(self.d).index(tri)
                for j in range(i + 1, 4):
                    self.mask2 |= 1 << pair_list(self.d).index((loc[i], loc[j]))
        if len(loc) > 4:
            raise TraceUnsupported("derivatives of network outputs beyond fourth order are outside the fused path")

    @property
    def n_streams(self):
        return (1 + self.first * self.d + (1 if self.lap else bin(self.mask2).count("1")) + bin(self.mask3).count("1")
                + bin(self.mask4).count("1"))

    def slot(self, mi):
        if mi and mi[0] == "L":
            return 1 + self.d
        assert not (self.lap and len(mi) == 2)
        loc = tuple(sorted(self.deps.index(c) for c in mi))
        if len(loc) == 0:
            return 0
        if len(loc) == 1:
            return 1 + loc[0]
        if len(loc) == 4:
            k = quad_list(self.d).index(loc)
            assert (self.mask4 >> k) & 1 and not self.lap
            return 1 + self.d + bin(self.mask2).count("1") + bin(self.mask3).count("1") + bin(self.mask4 & ((1 << k) - 1)).count("1")
        if len(loc) == 3:
            k = triple_list(self.d).index(loc)
            assert (self.mask3 >> k) & 1 and not self.lap
            return 1 + self.d + bin(self.mask2).count("1") + bin(self.mask3 & ((1 << k) - 1)).count("1")
        k = pair_list(self.d).index(loc)
        assert (self.mask2 >> k) & 1
        return 1 + self.d + bin(self.mask2 & ((1 << k) - 1)).count("1")


# ----------------------------------------------------------------------------------------------- expression emission
def _lit(v):
    if v != v or v in (float("inf"), float("-inf")):
        raise ValueError("non-finite constant in traced expression")
    s = repr(float(v))          # shortest decimal that round-trips the double: exact for the fp32 and the fp64 build alike
    if "." not in s and "e" not in s and "n" not in s:
        s += ".0"
    return s + "f"


def _powi_expr(x, n):
    if n == 0:
        return "1.0f"
    if n == 1:
        return x
    if n <= 8:
        return "(" + "*".join([x] * n) + ")"
    return f"powf({x}, {float(n)}f)"


_UN_FWD = {
    "neg": "-{a}", "sin": "sinf({a})", "cos": "cosf({a})", "tan": "tanf({a})", "exp": "expf({a})",
    "log": "logf({a})", "tanh": "tanhf({a})", "sqrt": "sqrtf({a})", "abs": "fabsf({a})", "sinh": "sinhf({a})",
    "cosh": "coshf({a})", "sigmoid": "(1.0f/(1.0f+expf(-{a})))", "recip": "(1.0f/{a})",
    "sign": "(({a}>0.0f)-({a}<0.0f))",
    "log1p": "log1pf({a})", "expm1": "expm1f({a})", "erf": "erff({a})", "atan": "atanf({a})",
    "floor": "floorf({a})", "ceil": "ceilf({a})", "round": "rintf({a})", "trunc": "truncf({a})",       # (rint: half to even, like torch.round)
    "detach": "{a}",
}
# adjoint factor of the single child: child_adj += b * factor ; {a} child value, {v} node value
_UN_ADJ = {
    "neg": "-{b}", "sin": "{b}*cosf({a})", "cos": "-{b}*sinf({a})", "tan": "{b}*(1.0f+{v}*{v})",
    "exp": "{b}*{v}", "log": "{b}/{a}", "tanh": "{b}*(1.0f-{v}*{v})", "sqrt": "{b}/(2.0f*{v})",
    "abs": "{b}*(({a}>0.0f)-({a}<0.0f))", "sinh": "{b}*coshf({a})", "cosh": "{b}*sinhf({a})",
    "sigmoid": "{b}*{v}*(1.0f-{v})", "recip": "-{b}*{v}*{v}", "sign": None,
    "log1p": "{b}/(1.0f+{a})", "expm1": "{b}*({v}+1.0f)", "erf": "{b}*1.1283791670955126f*expf(-{a}*{a})",
    "atan": "{b}/(1.0f+{a}*{a})",
    "floor": None, "ceil": None, "round": None, "trunc": None, "detach": None,      # (no adjoint flows into the child)
}


def _forward_lines(g, order, val, symbols=()):
    """The forward half of a traced DAG as straight-line fp32 statements, one ``const float v<i>`` per node of ``order`` (children
    first).  val(i): the C expression of node i's value; symbols: the network symbols in use (``s[k]``), in order."""
    L = []
    for i in order:
        n = g.nodes[i]
        op = n[0]
        if op in ("const", "coord", "data", "param"):
            continue
        if op == "net":
            L.append(f"  const float v{i} = s[{symbols.index(i)}];")
            continue
        if op in ("add", "sub", "mul", "div"):
            sym = {"add": "+", "sub": "-", "mul": "*", "div": "/"}[op]
            e = f"{val(n[1])} {sym} {val(n[2])}"
        elif op == "powi":
            e = _powi_expr(val(n[1]), n[2])
        elif op == "powc":
            e = f"powf({val(n[1])}, {_lit(n[2])})"
        elif op == "atan2":
            e = f"atan2f({val(n[1])}, {val(n[2])})"
        elif op in ("gt", "ge"):          # masks: 1.0f / 0.0f
            e = f"(({val(n[1])} {'>' if op == 'gt' else '>='} {val(n[2])}) ? 1.0f : 0.0f)"
        elif op == "where":               # a select, not a blend (symbolic.BINARY)
            e = f"(({val(n[1])} != 0.0f) ? {val(n[2])} : {val(n[3])})"
        else:
            e = _UN_FWD[op].format(a=val(n[1]))
        L.append(f"  const float v{i} = {e};")
    return L


def _closure_host(mode, N, R, f64):
    """Tail of a generated closure module: the traits struct ``Closure`` (what differs between the closure kernels; the
    contract is the file comment of csrc/ndq_closure_host.h), then that header -- the launchers and every ndq_fused_* export.
    mode: the ``ClosureMode`` record, whose C++ texts are filled with N parameter sets and R stream rows (networks or
    evaluation sites).  The loop-mode kernel is fp32 only (csrc/ndq_tail.h) and exists for up to ``mode.loop_max`` rows."""
    text = lambda t, **kw: t.format(N=N, R=R, **kw)
    loop = bool(mode.loop) and not f64 and R <= mode.loop_max
    no_pull = "\n  static constexpr bool NO_PULL = true;" if mode.traits else ""
    return f"""struct Closure {{
  using Cfg = CFG;
  using Pw = PW;
  using Args = ndq::{mode.args};
  static constexpr int K = {N}, THREADS = {text(mode.threads)}, POINTS = {mode.points}, SLOTS = {text(mode.slots)};{no_pull}
  static constexpr auto train = &{text(mode.kern, train='true')};
  static constexpr auto eval = &{text(mode.kern, train='false')};
  static constexpr auto tv = &{text(mode.tv)};
  static constexpr auto loop = {'&' + text(mode.loop) if loop else 'nullptr'};
  static constexpr size_t LDS_TRAIN = {text(mode.lds, train='true')}, LDS_EVAL = {text(mode.lds, train='false')}, LDS_LOOP = {text(mode.lds_loop) if loop else 0};
}};
}}  // namespace
#include "ndq_closure_host.h"
"""


class PointwiseProgram:
    """A traced system lowered to straight-line fp32 code.

    graph      : symbolic.Graph
    residuals  : node ids, one per equation (columns of the reference's (N, n_eq) residual, solvers.py:381)
    funcs      : node ids of the re-parameterised function values (one per condition, solvers.py:373-375)
    streams    : {net_idx: NetStreams}
    """

    LOSS_KINDS = ("l2", "l1", "infinity", "custom")

    def __init__(self, graph: Graph, residuals, funcs, n_nets, widen=None, allow_lap=None, unify=None, loss="l2",
                 loss_term=None):
        """widen(net_idx, NetStreams): optional hook that may enlarge ``first`` / ``mask2`` of a net to the nearest
        stream set libndq.so has kernels for (slots are assigned after it ran).
        unify(streams dict): optional hook run before ``widen`` that may give several networks one common stream set
        (so that one multi-network closure kernel can serve them).
        allow_lap(net_idx, coords) -> bool: may the second derivatives of net k w.r.t. ``coords`` be merged into one
        Laplacian stream (asked only after the merge has been proven valid symbolically)."""
        assert loss in self.LOSS_KINDS and (loss == "custom") == (loss_term is not None)
        # per-point loss term (losses.py:4-12): sum r^2 | sum |r| | max |r|, averaged by the host; "custom": the traced
        # per-point term of a user loss_fn (+ additional_loss), node ``loss_term`` -- loss = mean over points of it
        self.loss = loss
        self.g = graph
        self.residuals = list(residuals)
        self.funcs = list(funcs)
        self.loss_term = loss_term
        if allow_lap is not None:
            # the loss term is held to the same standard as the residuals: it may see pure second derivatives of a
            # network only through their sum if those are to travel as one Laplacian stream
            extra = [loss_term] if loss_term is not None else []
            merged = self._merge_laplacian(self.residuals + extra, self.funcs, n_nets, allow_lap)
            self.residuals = merged[:len(self.residuals)]
            if extra:
                self.loss_term = merged[-1]
        self.n_nets = n_nets                    # parameter sets
        self.site_net = list(getattr(graph, "site_net", None) or range(n_nets))
        self.n_sites = len(self.site_net)       # (network, coordinate tuple) pairs: stream arrays are per site
        self.n_coords = graph.n_coords
        self.n_data = len(getattr(graph, "data", ()))       # per-point data columns: input rows behind the coordinates
        self.n_theta = len(getattr(graph, "params", ()))    # trainable scalars of the equations: kernel arguments
        self.order = graph.reachable(self.residuals + self.funcs + ([self.loss_term] if self.loss_term is not None else []))
        self.streams = {}
        for k in range(self.n_sites):
            deps = graph.net_deps.get(k)
            if deps is None:
                continue
            self.streams[k] = NetStreams(deps, graph.net_nout[k])
        self.symbols = []          # net nodes in use, in order
        for i in self.order:
            n = graph.nodes[i]
            if n[0] == "net":
                self.streams[n[1]].need(n[3])
                self.symbols.append(i)
        if unify is not None:
            unify(self.streams)
        if widen is not None:
            for k, st in self.streams.items():
                widen(k, st)
        self.source = self._emit()
        self.key = hashlib.sha1((self.source + _build_tag()).encode()).hexdigest()[:16]

    # ---- Laplacian-stream rewrite
    def _merge_laplacian(self, residuals, funcs, n_nets, allow_lap):
        """If every residual depends on the pure second derivatives N_aa of a network output only through their SUM
        (d r / d N_aa is the same expression for all a, and free of the N_bb), replace them by one symbol
        L = sum_a N_aa: r(N_xx, N_yy, ..) = r0 + c (N_xx + N_yy + ..) = r(L, 0, ..).  Proven on the DAG, per network."""
        g = self.g
        order = g.reachable(list(residuals) + list(funcs))
        second = {}
        third = set()
        for i in order:
            n = g.nodes[i]
            if n[0] == "net" and len(n[3]) == 2 and n[3][0] != "L":
                second.setdefault(n[1], []).append(i)
            if n[0] == "net" and len(n[3]) >= 3 and n[3][0] != "L":
                third.add(n[1])          # third-order streams need every pair on its own: no Laplacian stream
        for k in third:
            second.pop(k, None)
        func_set = set(g.reachable(list(funcs)))
        out = list(residuals)
        for k, leaves in second.items():
            mis = [g.nodes[i][3] for i in leaves]
            if any(a != b for a, b in mis) or len(leaves) < 2:
                continue                                     # mixed partials present, or nothing to merge
            if any(i in func_set for i in leaves):
                continue
            by_out = {}
            for i in leaves:
                by_out.setdefault(g.nodes[i][2], []).append(i)
            coords = sorted({mi[0] for mi in mis})
            if any(sorted(g.nodes[i][3][0] for i in ls) != coords for ls in by_out.values()):
                continue                                     # every output must use the same coordinate set
            leafset = set(leaves)
            ok = True
            for r in out:
                for o, ls in by_out.items():
                    ds = [g.diff(r, ("n", i)) for i in ls]
                    if any(d != ds[0] for d in ds) or any(j in leafset for j in g.reachable([ds[0]])):
                        ok = False
            if not ok or not allow_lap(k, tuple(coords)):
                continue
            mapping = {}
            for o, ls in by_out.items():
                lap = g.net(k, o, ("L",) + tuple(coords))
                for j, i in enumerate(sorted(ls, key=lambda i: g.nodes[i][3])):
                    mapping[i] = lap if j == 0 else g.const(0.0)
            memo = {}
            out = [g.subst(r, mapping, memo) for r in out]
        return out

    # ---- helpers
    def _val(self, i):
        n = self.g.nodes[i]
        if n[0] == "const":
            return _lit(n[1])
        if n[0] == "coord":
            return f"c{n[1]}"
        if n[0] == "data":
            return f"d{n[1]}"
        if n[0] == "param":
            return f"t{n[1]}"
        return f"v{i}"

    def sym_location(self, i):
        _, k, o, mi = self.g.nodes[i]
        st = self.streams[k]
        return k, st.slot(mi) * st.n_out + o

    def _emit_point_fn(self):
        g = self.g
        L = []
        # which nodes depend on a network symbol (only those carry adjoints)
        dep = {}
        for i in self.order:
            n = g.nodes[i]
            # (runtime constants -- frozen 'param' leaves, symbolic.Graph.external -- carry no adjoint)
            dep[i] = n[0] == "net" or (n[0] == "param" and n[1] not in getattr(g, "frozen", ())) or any(dep[c] for c in g.children(i))
        res_order = g.reachable(self.residuals)
        res_set = set(res_order)
        L.append("// ---- forward")
        L += _forward_lines(g, self.order, self._val, self.symbols)
        for e, i in enumerate(self.residuals):
            L.append(f"  r[{e}] = {self._val(i)};")
        if self.loss == "custom":
            L.append(f"  r[{len(self.residuals)}] = {self._val(self.loss_term)};      // per-point loss term")
        for m, i in enumerate(self.funcs):
            L.append(f"  f[{m}] = {self._val(i)};")
        L.append("  if (!want_adj) return;")
        L.append(f"// ---- adjoint of the per-point loss term ({self.loss}, scaled by seed) w.r.t. the network streams")
        terms = {}
        neq = len(self.residuals)
        if self.loss == "custom":
            res_order = g.reachable([self.loss_term])
            res_set = set(res_order)
            if dep.get(self.loss_term):
                terms[self.loss_term] = ["seed"]
        if self.loss == "infinity" and neq > 1:      # d max_e |r_e|: the first maximal entry carries the seed
            L.append("  int amax = 0; float vmax = fabsf(r[0]);")
            L.append(f"  for (int e = 1; e < {neq}; ++e) if (fabsf(r[e]) > vmax) {{ vmax = fabsf(r[e]); amax = e; }}")
        for e, i in enumerate(self.residuals if self.loss != "custom" else []):
            if dep.get(i):
                v = self._val(i)
                sign = f"(({v}) > 0.0f ? seed : (({v}) < 0.0f ? -seed : 0.0f))"
                if self.loss == "l2":
                    t = f"(2.0f*seed)*{v}"
                elif self.loss == "l1" or neq == 1:
                    t = sign
                else:
                    t = f"(amax == {e} ? {sign} : 0.0f)"
                terms.setdefault(i, []).append(t)
        for i in reversed(res_order):
            if i not in terms or not dep[i]:
                continue
            n = g.nodes[i]
            op = n[0]
            L.append(f"  const float b{i} = {' + '.join(terms[i])};")
            b = f"b{i}"
            if op in ("net", "param"):
                continue

            def push(child, expr):
                if dep[child]:
                    terms.setdefault(child, []).append(expr)

            if op == "add":
                push(n[1], b); push(n[2], b)
            elif op == "sub":
                push(n[1], b); push(n[2], f"-{b}")
            elif op == "mul":
                push(n[1], f"{b}*{self._val(n[2])}"); push(n[2], f"{b}*{self._val(n[1])}")
            elif op == "div":
                push(n[1], f"{b}/{self._val(n[2])}")
                push(n[2], f"-{b}*v{i}/{self._val(n[2])}")
            elif op == "atan2":
                L.append(f"  const float q{i} = {b}/({self._val(n[1])}*{self._val(n[1])} + {self._val(n[2])}*{self._val(n[2])});")
                push(n[1], f"q{i}*{self._val(n[2])}"); push(n[2], f"-q{i}*{self._val(n[1])}")
            elif op in ("gt", "ge"):
                pass                          # piecewise constant: nothing flows through a mask
            elif op == "where":
                push(n[2], f"(({self._val(n[1])} != 0.0f) ? {b} : 0.0f)")
                push(n[3], f"(({self._val(n[1])} != 0.0f) ? 0.0f : {b})")
            elif op == "powi":
                push(n[1], f"{b}*{float(n[2])}f*{_powi_expr(self._val(n[1]), n[2] - 1)}")
            elif op == "powc":
                push(n[1], f"{b}*{_lit(n[2])}*powf({self._val(n[1])}, {_lit(n[2] - 1.0)})")
            else:
                t = _UN_ADJ[op]
                if t is not None:
                    push(n[1], t.format(b=b, a=self._val(n[1]), v=f"v{i}"))
        for idx, i in enumerate(self.symbols):
            L.append(f"  g[{idx}] = {'b%d' % i if (i in terms and i in res_set) else '0.0f'};")
        # per-point adjoints of the trainable scalars: behind the stream adjoints in g (summed over the points by the kernels)
        nsym = len(self.symbols)
        for j in range(self.n_theta):
            i = g._ids.get(("param", j))
            L.append(f"  g[{nsym + j}] = {'b%d' % i if (i is not None and i in terms and i in res_set) else '0.0f'};")
        return "\n".join(L)

    def point_fn_source(self):
        nc = self.n_coords
        body = self._emit_point_fn()
        neq = len(self.residuals)
        if self.loss == "custom":
            term = f"r[{neq}]"
        elif self.loss == "l2":
            term = " + ".join(f"r[{e}]*r[{e}]" for e in range(neq)) or "0.0f"
        elif self.loss == "l1":
            term = " + ".join(f"fabsf(r[{e}])" for e in range(neq)) or "0.0f"
        else:
            term = "0.0f"
            for e in range(neq):
                term = f"fmaxf({term}, fabsf(r[{e}]))"
        nd, nt = self.n_data, self.n_theta
        return f"""// c: {nc} coordinate(s) | {nd} per-point data value(s) | {nt} trainable scalar(s) of the equations;  g: adjoints of the
// {len(self.symbols)} stream symbol(s) | of the {nt} trainable scalar(s)
NDQ_PW_INLINE void ndq_pw_point(const float* c, const float* s, float seed, int want_adj, float* r, float* f, float* g) {{
{chr(10).join(f"  const float c{i} = c[{i}];" for i in range(nc))}
{chr(10).join(f"  const float d{j} = c[{nc + j}];" for j in range(nd))}
{chr(10).join(f"  const float t{j} = c[{nc + nd + j}];" for j in range(nt))}
{chr(10).join(f"  const float c{i} = {_lit(v)};   // virtual coordinate (boundary value)" for i, v in sorted(self.g.vcoords.items()))}
{body}
}}
// per-point loss term ({self.loss}); the host averages it: seed = 1 / (N * n_eq) for l2 / l1, 1 / N for infinity
NDQ_PW_INLINE float ndq_pw_loss(const float* r) {{ return {term}; }}
"""

    @property
    def loss_norm(self):
        """what the sum over points of the per-point loss term is divided by, per point"""
        return 1 if self.loss in ("infinity", "custom") else max(len(self.residuals), 1)

    @property
    def n_r(self):
        """length of the per-point ``r`` array: residuals (+ the loss term of a traced custom loss)"""
        return max(len(self.residuals) + (1 if self.loss == "custom" else 0), 1)

    def fused_source(self, desc, f64=False):
        """Source of the single-launch closure kernel (csrc/ndq_mlp.h: fused_closure_kernel for one network,
        fused_multi_closure_kernel for 2..4 networks of one shape and stream set) specialised with this program's
        per-point function.  desc: the ndq_mlp_desc shared by all networks.
        f64: the same module in double (csrc/ndq_mlp.h under NDQ_F64: per-point GEMMs on the f64 MFMA, no bf16 planes, no
        pull / loop mode) -- one network on the plain closure (``can_fuse_f64``), or 2..4 networks on the multi-network
        closure (``can_fuse_multi_f64``)."""
        if f64:
            return "#define NDQ_F64 1\n" + source_f64(self._fused_source(desc, True))
        return self._fused_source(desc, False)

    def _site_traits(self):
        """The traits struct of an evaluation-site module (csrc/ndq_mlp.h: SiteIdentity is the contract): which network wave
        group k runs, whether it is that network's first site (rank 0: its waves write the gradient row), and which of its
        inputs are boundary values."""
        S, sn = self.n_sites, self.site_net
        rank = [sn[:k].count(sn[k]) for k in range(S)]
        virt = [[(d, self.g.vcoords[c]) for d, c in enumerate(self.streams[k].deps) if c in self.g.vcoords] for k in range(S)]
        vmask = [sum(1 << d for d, _ in v) for v in virt]
        chain = lambda vals, fmt: " : ".join([f"k == {k} ? {fmt(v)}" for k, v in enumerate(vals[:-1])] + [fmt(vals[-1])])
        values = "".join(f"(k == {k} && d == {d}) ? {_lit(v)} : " for k in range(S) for d, v in virt[k]) + "0.0f"
        lits = "; ".join(f"site {k} input {d} = {_lit(v)}" for k in range(S) for d, v in virt[k])
        return f"""// evaluation sites: wave group k runs network NET[k] = {{{", ".join(map(str, sn))}}}
// boundary values: {lits}
struct SITES {{
  static constexpr bool ON = true;
  static constexpr int net(int k) {{ return {chain(sn, str)}; }}
  static constexpr int rank(int k) {{ return {chain(rank, str)}; }}
  static constexpr unsigned vmask(int k) {{ return {chain(vmask, lambda v: f"{v}u")}; }}
  static constexpr float value(int k, int d) {{ return {values}; }}
}};
"""

    def closure_mode(self, desc):
        """The ``ClosureMode`` record of the closure kernel that serves this program when every site has descriptor ``desc``."""
        name = fuse_mode(self, {k: desc for k in range(max(self.n_nets, self.n_sites))})
        assert name is not None
        return MODES[name]

    def _fused_source(self, desc, f64):
        """One generated closure module, assembled from the mode's record: title comment, defines, kernel header, the per-point
        function, CFG, the site traits where the mode has them, PW around one of the two per-point interfaces, and the host
        tail.  N parameter sets, R stream rows (one per network, or one per evaluation site).
        jets: the kernels of csrc/ndq_mlp.h hand ``apply`` a point's streams as arrays ``jets[R][NS]`` / ``gj`` (one output per
              network, every network reads all coordinates).
        rows: one point per lane; stream values and adjoint seeds travel through an LDS tile as rows ``srow`` / ``grow``,
              [row][n_streams][n_out] -- any number of outputs, any subset of the batch coordinates as inputs (``PW::dep``; a
              site's boundary values are the traits' business, not dep's).  The grouped kernel of csrc/ndq_mlp.h pads the outputs
              of a stream to 16 (ndq::group_w), the kernels of csrc/ndq_wide.h do not."""
        mode = self.closure_mode(desc)
        assert mode.f64 or not f64
        N, R, st = self.n_nets, self.n_sites, self.streams[0]
        width = st.n_streams * st.n_out
        if mode.rows:
            assert all(self.streams[k].n_streams * self.streams[k].n_out == width for k in range(R))
            gw = st.n_out if not mode.padded_rows or st.n_out == 1 else (st.n_out + 15) // 16 * 16
            at = lambda k, loc: f"[{k * width + (loc // st.n_out) * gw + loc % st.n_out}]"
            src, dst = "srow", "grow"
        else:
            at = (lambda k, loc: f"[{loc}]") if R == 1 else (lambda k, loc: f"[{k}][{loc}]")
            src, dst = "jets", "gj"
        used, loads = {}, []
        for idx, i in enumerate(self.symbols):
            k, loc = self.sym_location(i)
            used[(k, loc)] = idx
            loads.append(f"    s[{idx}] = {src}{at(k, loc)};")
        stores = [f"    {dst}{at(k, loc)} = {'g[%d]' % used[(k, loc)] if (k, loc) in used else '0.0f'};"
                  for k in range(R) for loc in range(width)]
        nsym = max(len(self.symbols), 1)
        neq, nf = len(self.residuals), len(self.funcs)
        guard = "    if (!want_adj) return;\n" if mode.rows else ""
        point = f"""{chr(10).join(loads)}
    ndq_pw_point(c, s, seed, want_adj, r, f, g);
{guard}{chr(10).join(stores)}
#pragma unroll
    for (int j = 0; j < NT; ++j) gth[j] = g[{len(self.symbols)} + j];
  }}
}};
"""
        if mode.rows:
            deps = list(range(self.n_coords)) if mode.traits else list(st.deps)
            dep_fn = " : ".join(f"d == {d} ? {c}" for d, c in enumerate(deps)) + " : 0"
            lead = ("grouped single-launch closure kernel (forward streams -> LDS exchange ->\n"
                    "// per-point stage, one point per lane -> reverse pass)")
            check = f'static_assert(CFG::NS * CFG::NOUT == {width}, "stream layout of the traced program and of the kernel disagree");\n'
            pw = f"""struct PW {{
  // NC rows of the coordinate block per point: the batch coordinates, then ND data columns; NT trainable scalars
  static constexpr int NEQ = {neq}, NF = {nf}, ND = {self.n_data}, NT = {self.n_theta}, NC = {self.n_coords} + ND, NR = {self.n_r};
  static constexpr int dep(int d) {{ return {dep_fn}; }}     // batch coordinate fed to network input d
  static __device__ __forceinline__ float loss(const float* r) {{ return ndq_pw_loss(r); }}
  static __device__ __forceinline__ void apply(const float (&cc)[NC], const float* th, const float* srow, float seed, int want_adj,
                                               float (&r)[{self.n_r}], float (&f)[{max(nf, 1)}], float* grow, float* gth) {{
    float c[NC + NT], s[{nsym}], g[{nsym} + NT];
#pragma unroll
    for (int d = 0; d < NC; ++d) c[d] = cc[d];
#pragma unroll
    for (int j = 0; j < NT; ++j) c[NC + j] = th[j];
"""
        else:
            dims = "" if R == 1 else f"[{R}]"
            head = mode.apply_head.format(jets=f"const float (&jets){dims}[CFG::NS]", gj=f"float (&gj){dims}[CFG::NS]",
                                          r=f"float (&r)[{self.n_r}]", f=f"float (&f)[{max(nf, 1)}]")
            lead, check = "single-launch closure kernel (forward streams + pointwise stage +\n// reverse pass)", ""
            pw = f"""struct PW {{
  // ND per-point data columns (rows D .. D + ND of the coordinate block), NT trainable scalars of the equations
  static constexpr int NEQ = {neq}, NF = {nf}, NR = {self.n_r}, ND = {self.n_data}, NT = {self.n_theta};
  static __device__ __forceinline__ float loss(const float* r) {{ return ndq_pw_loss(r); }}
{head}
    float c[CFG::D + ND + NT], s[{nsym}], g[{nsym} + NT];
#pragma unroll
    for (int d = 0; d < CFG::D; ++d) c[d] = x[d];
#pragma unroll
    for (int j = 0; j < ND + NT; ++j) c[CFG::D + j] = xe[j];
"""
        # hidden-layer weight gradients from the bf16x3 planes through transposing LDS reads (csrc/ndq_mlp.h Cfg::WG_TR; shapes
        # it does not cover, or whose R images would not fit the LDS, ignore the switch).  NDQ_WG_TR_K: weight images in LDS --
        # one per row, a network with two sites is staged twice
        wg_tr = f"#ifndef NDQ_WG_TR\n#define NDQ_WG_TR 1\n#endif\n#define NDQ_WG_TR_K {R}\n" if mode.wg_tr else ""
        return f"""// GENERATED by neurodiffeq_amd/codegen.py -- {lead} of one PDE system{mode.what.format(N=N, R=R)}, gfx950.
{wg_tr}{CLOSURE_PRODUCTS if mode.products else ""}#include "{mode.header}"
#define NDQ_PW_INLINE __device__ __forceinline__
#ifndef NDQ_MAX_BLOCKS
#define NDQ_MAX_BLOCKS 256     // closure workgroups per launch {mode.blocks_note}
#endif
{self.point_fn_source()}
namespace {{
using CFG = {mode.cfg(desc)};
{check}{self._site_traits() if mode.traits else ""}{pw}{point}{_closure_host(mode, N, R, f64)}"""

    def _emit(self):
        nsym = max(len(self.symbols), 1)
        neq, nf, nc, nn = len(self.residuals), len(self.funcs), self.n_coords, self.n_sites
        loads, stores = [], []
        for idx, i in enumerate(self.symbols):
            k, loc = self.sym_location(i)
            loads.append(f"    s[{idx}] = a.jets[{k}][(size_t){loc} * a.ldj + n];")
        # adjoint stores: every slot of every net is written (unused streams get 0 so the backward kernel can read them)
        for k, st in sorted(self.streams.items()):
            used = {}
            for idx, i in enumerate(self.symbols):
                kk, loc = self.sym_location(i)
                if kk == k:
                    used[loc] = idx
            for loc in range(st.n_streams * st.n_out):
                val = f"g[{used[loc]}]" if loc in used else "0.0f"
                stores.append(f"      a.gbar[{k}][(size_t){loc} * a.ldj + n] = {val};")
        src = f"""// GENERATED by neurodiffeq_amd/codegen.py -- fused pointwise stage of one traced PDE system (gfx950).
// per point: {nc} coords + {len(self.symbols)} stream symbols in, {neq} residual(s), {nf} function value(s), adjoints out.
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define NDQ_PW_INLINE __device__ __forceinline__
#else
#include <math.h>
#include <stddef.h>
#define NDQ_PW_INLINE static inline
#endif

#define NDQ_PW_NC {nc}
#define NDQ_PW_ND {self.n_data}
#define NDQ_PW_NT {self.n_theta}
#define NDQ_PW_NSYM {len(self.symbols)}
#define NDQ_PW_NEQ {neq}
#define NDQ_PW_NR {self.n_r}
#define NDQ_PW_NF {nf}
#define NDQ_PW_NNETS {nn}

{self.point_fn_source()}
#ifdef __HIPCC__
struct PwArgs {{
  const float* coords;
  const float* jets[NDQ_PW_NNETS];
  float* gbar[NDQ_PW_NNETS];
  float* funcs;
  float* resid;
  float* loss_partials;
  int n, ldc, ldj, want_adj;
  float seed;
  const float* theta;          // [NDQ_PW_NT] trainable scalars of the equations
  float* theta_partials;       // [gridDim.x][NDQ_PW_NT] block sums of their per-point adjoints
}};

extern "C" __global__ __launch_bounds__(256) void ndq_pw_kernel(PwArgs a) {{
  const int n = blockIdx.x * 256 + threadIdx.x;
  float sq = 0.f;
  float gt[NDQ_PW_NT > 0 ? NDQ_PW_NT : 1] = {{0.f}};
  if (n < a.n) {{
    float c[NDQ_PW_NC + NDQ_PW_ND + NDQ_PW_NT], s[{nsym}], r[{self.n_r}], f[{max(nf, 1)}], g[{nsym} + NDQ_PW_NT];
#pragma unroll
    for (int i = 0; i < NDQ_PW_NC + NDQ_PW_ND; ++i) c[i] = a.coords[(size_t)i * a.ldc + n];   // data rows follow the coordinates
#pragma unroll
    for (int j = 0; j < NDQ_PW_NT; ++j) c[NDQ_PW_NC + NDQ_PW_ND + j] = a.theta[j];
{chr(10).join(loads)}
    ndq_pw_point(c, s, a.seed, a.want_adj, r, f, g);
    if (a.want_adj) {{
#pragma unroll
      for (int j = 0; j < NDQ_PW_NT; ++j) gt[j] = g[NDQ_PW_NSYM + j];
    }}
    sq += ndq_pw_loss(r);
    if (a.resid) {{
#pragma unroll
      for (int e = 0; e < NDQ_PW_NEQ; ++e) a.resid[(size_t)e * a.ldj + n] = r[e];
    }}
    if (a.funcs) {{
#pragma unroll
      for (int m = 0; m < NDQ_PW_NF; ++m) a.funcs[(size_t)m * a.ldj + n] = f[m];
    }}
    if (a.want_adj) {{
{chr(10).join(stores)}
    }}
  }}
  // fixed-order block reduction of the squared residuals: wave shuffle tree, then the 4 waves in order
  for (int off = 32; off > 0; off >>= 1) sq += __shfl_down(sq, off);
  __shared__ float wsum[4];
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = sq;
  __syncthreads();
  if (threadIdx.x == 0) a.loss_partials[blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
#if NDQ_PW_NT > 0
  // the same fixed-order block sums for the adjoints of the trainable scalars
  __shared__ float tsum[4][NDQ_PW_NT];
#pragma unroll
  for (int j = 0; j < NDQ_PW_NT; ++j) {{
    float v = gt[j];
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    if ((threadIdx.x & 63) == 0) tsum[threadIdx.x >> 6][j] = v;
  }}
  __syncthreads();
  if (threadIdx.x < NDQ_PW_NT && a.want_adj && a.theta_partials)
    a.theta_partials[(size_t)blockIdx.x * NDQ_PW_NT + threadIdx.x] =
        (tsum[0][threadIdx.x] + tsum[1][threadIdx.x]) + (tsum[2][threadIdx.x] + tsum[3][threadIdx.x]);
#endif
}}

extern "C" int ndq_pw_blocks(int n) {{ return (n + 255) / 256; }}
extern "C" int ndq_pw_num_theta() {{ return NDQ_PW_NT; }}
extern "C" int ndq_pw_num_data() {{ return NDQ_PW_ND; }}

// trainable scalars of the equations: values read by every launch, block sums of their adjoints written by training launches
static const float* g_theta = nullptr;
static float* g_theta_partials = nullptr;
extern "C" void ndq_pw_bind_theta(const float* theta, float* theta_partials) {{ g_theta = theta; g_theta_partials = theta_partials; }}

extern "C" int ndq_pw_launch(const float* coords, int ldc, int n, const float* const* jets, float* const* gbar, int ldj,
                             float* funcs, float* resid, float* loss_partials, float seed_scale, void* stream) {{
  if (!coords || !jets || !loss_partials || n <= 0) return -2;
  if (NDQ_PW_NT > 0 && !g_theta) return -2;
  PwArgs a;
  a.theta = g_theta; a.theta_partials = g_theta_partials;
  a.coords = coords;
  for (int k = 0; k < NDQ_PW_NNETS; ++k) {{
    a.jets[k] = jets[k];
    a.gbar[k] = gbar ? gbar[k] : nullptr;
  }}
  a.funcs = funcs; a.resid = resid; a.loss_partials = loss_partials;
  a.n = n; a.ldc = ldc; a.ldj = ldj; a.want_adj = gbar ? 1 : 0; a.seed = seed_scale;
  hipLaunchKernelGGL(ndq_pw_kernel, dim3((n + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  return (int)hipGetLastError();
}}
#endif
"""
        return src

    # ---- algorithmic HBM traffic per point (bytes), for the roofline report
    def bytes_per_point(self, train=True, write_resid=False, write_funcs=False):
        b = 4 * self.n_coords + 4 * len(self.symbols)
        if train:
            b += 4 * sum(st.n_streams * st.n_out for st in self.streams.values())
        if write_resid:
            b += 4 * len(self.residuals)
        if write_funcs:
            b += 4 * len(self.funcs)
        return b


# ----------------------------------------------------------------------------------------------- build / load
class PointwiseKernel:
    def __init__(self, so_path, f64=False):
        self.path = so_path
        self.lib = ctypes.CDLL(so_path)
        self.lib.ndq_pw_launch.restype = ctypes.c_int
        self.lib.ndq_pw_launch.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.c_double if f64 else ctypes.c_float, ctypes.c_void_p]
        self.lib.ndq_pw_blocks.restype = ctypes.c_int
        self.lib.ndq_pw_blocks.argtypes = [ctypes.c_int]

    def blocks(self, n):
        return self.lib.ndq_pw_blocks(n)


def so_path_for(program: PointwiseProgram, f64=False):
    return os.path.join(JIT_DIR, f"pw{'64' if f64 else ''}_{program.key}.so")


_F64_FUNCS = re.compile(r"\b(pow|sin|cos|tan|exp|log|tanh|sqrt|fabs|sinh|cosh|fmax|log1p|expm1|erf|atan|atan2|floor|ceil|rint|trunc)f\(")
_F64_LITERAL = re.compile(r"(?<![\w.])((?:\d+\.\d*|\.\d+|\d+)(?:[eE][-+]?\d+)?)f\b")


def source_f64(source):
    """The generated pointwise source in double precision (the reference's default dtype, neurodiffeq/__init__.py:22):
    the emitter writes ``float``, ``expf(..)``-style calls and ``1.0f``-style literals only, so the fp64 build is a
    textual rewrite of the same program -- types, math calls, literal suffixes."""
    out = re.sub(r"\bfloat\b", "double", source)
    out = _F64_FUNCS.sub(lambda m: m.group(1) + "(", out)
    return _F64_LITERAL.sub(lambda m: m.group(1), out)


def build(program: PointwiseProgram, force=False, f64=False):
    """Compile the generated source for gfx950 (in-tree cache keyed by the source hash) and return the .so path."""
    os.makedirs(JIT_DIR, exist_ok=True)
    so = so_path_for(program, f64)
    src = so[:-3] + ".hip"
    if os.path.exists(so) and not force:
        return so
    with open(src, "w") as fh:
        fh.write(source_f64(program.source) if f64 else program.source)
    try:
        _hipcc.compile_shared(src, so, defer=True)
    except RuntimeError as e:
        raise RuntimeError(f"hipcc failed for generated pointwise kernel {src}:\n{str(e)[-4000:]}") from e
    return so


def load(program: PointwiseProgram, f64=False):
    return PointwiseKernel(build(program, f64=f64), f64)


# ----------------------------------------------------------------------------------------------- fused closure kernel
class FusedKernel:
    def __init__(self, so_path, f64=False):
        self.path = so_path
        self.lib = ctypes.CDLL(so_path)
        vp, ci, cf = ctypes.c_void_p, ctypes.c_int, (ctypes.c_double if f64 else ctypes.c_float)
        self.lib.ndq_fused_launch.restype = ci
        self.lib.ndq_fused_launch.argtypes = [vp, ci, ci, vp, vp, vp, vp, vp, ci, cf, ci, vp]
        self.lib.ndq_fused_launch_multi.restype = ci
        self.lib.ndq_fused_launch_multi.argtypes = [vp, ci, ci, vp, vp, vp, vp, vp, ci, cf, ci, vp]
        self.lib.ndq_fused_launch_tv.restype = ci
        self.lib.ndq_fused_launch_tv.argtypes = [vp, ci, ci, vp, vp, vp, cf, vp, ci, ci, vp, vp, vp]
        self.lib.ndq_fused_pull_ok.restype = ci
        self.lib.ndq_fused_launch_loop.restype = ci
        self.lib.ndq_fused_launch_loop.argtypes = [vp, ci, ci, cf, vp, ci, ci, vp, vp]
        self.lib.ndq_fused_loop_ok.restype = ci
        self.lib.ndq_fused_bind_theta.restype = None
        self.lib.ndq_fused_bind_theta.argtypes = [vp, vp]
        self.lib.ndq_fused_blocks.restype = ci
        self.lib.ndq_fused_blocks.argtypes = [ci]
        self.lib.ndq_fused_num_params.restype = ci
        self.lib.ndq_fused_num_nets.restype = ci
        self.lib.ndq_fused_threads.restype = ci
        self.threads = self.lib.ndq_fused_threads()
        self.lib.ndq_fused_lds_bytes.restype = ctypes.c_ulong
        self.n_nets = self.lib.ndq_fused_num_nets()

    def blocks(self, n):
        return self.lib.ndq_fused_blocks(n)


def _cache_key(source, more_flags=()):
    """Cache key of a generated module: its source (with the package location factored out, so a relocated checkout
    keeps its cache), the kernel headers it instantiates and the extra compile flags (NDQ_JIT_FLAGS, then ``more_flags``:
    the same key whichever of the two ways a flag came in)."""
    text = source.replace(HERE, "<neurodiffeq_amd>")
    flags = _extra_flags() + list(more_flags)
    return hashlib.sha1((text + _header_digest() + " ".join(flags) + _build_tag()).encode()).hexdigest()[:16]


def _build_tag():
    """What the build pipeline itself contributes to a cache key (the assembly fix-up pass and its version)."""
    return _hipcc.FIXUP_VERSION if _hipcc.fixup_enabled() else "no-fixup"


def _sampler_digest():
    h = hashlib.sha1()
    for name in ("csrc/ndq_sample.h", "csrc/ndq_sample_map.h"):
        with open(os.path.join(HERE, name), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()


def _header_digest():
    h = hashlib.sha1()
    for name in ("csrc/ndq_mlp.h", "csrc/ndq_tail.h", "csrc/ndq_launch.h", "csrc/ndq_wide.h", "csrc/ndq_deep.h", "csrc/ndq_closure_host.h",
                 "../include/ndq.h"):
        with open(os.path.join(HERE, name), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()


# ----------------------------------------------------------------------------------------------- sampler stages
MAP_MAX_ROWS = 6        # include/ndq.h NDQ_TABLE_MAX_AXES: rows of a plan point, rows a map may hand out
#: the user's arithmetic as written: no mul + add -> fma (a mask `x*x + y*y < 1` sees the products torch sees; + - * /, comparisons
#: and `where` are then torch's fp32 bit for bit).  The host build takes it as a flag.  The device build takes it as
#: `#pragma clang fp contract(off)` in front of ndq_map_point only: as a hipcc FLAG it also changes how the backend expands logf
#: inside the leaf laws of csrc/ndq_sample.h (a separate add instead of the last fused multiply-add), and a point recomputed by
#: the module would then differ by an ulp from the point sample_plan_kernel stores for the same (seed, draw, stream, i)
MAP_HOST_FLAGS = ["-ffp-contract=off"]


class SamplerMapProgram:
    """The traced stages of a device-drawn generator (generators.trace_stages: the callables of TransformGenerator /
    FilterGenerator above a plan) lowered to straight-line fp32: the forward half of a :class:`PointwiseProgram` only -- no network
    symbols, no adjoint, no data columns.  ``outs``: node ids of the rows handed out; ``keep``: node id of the AND of the filters'
    masks, or None; ``d_in``: rows of a plan point.  ``source`` is ONE text for both build targets: hipcc (the kernels and the
    launcher of csrc/ndq_sample_map.h, :func:`build_sampler_map`) and a host compiler (:func:`build_sampler_map_cpu`: the same
    ``ndq_map_point`` behind a loop over points, for tests without a GPU)."""

    def __init__(self, graph: Graph, outs, keep, d_in):
        self.g, self.outs, self.keep, self.d_in, self.d_out = graph, list(outs), keep, int(d_in), len(outs)
        if not 1 <= self.d_out <= MAP_MAX_ROWS or not 1 <= self.d_in <= MAP_MAX_ROWS:
            raise ValueError(f"a sampler map takes and hands out 1 .. {MAP_MAX_ROWS} rows, not {self.d_in} -> {self.d_out}")
        self.order = graph.reachable(self.outs + ([keep] if keep is not None else []))
        for i in self.order:
            n = graph.nodes[i]
            if n[0] in ("net", "param", "data") or (n[0] == "coord" and n[1] >= self.d_in):
                raise TraceUnsupported(f"a sampler stage may read the rows of its point and numbers only, not a {n[0]!r} leaf")
        self.source = self._emit()
        self.key = _cache_key(self.source + _sampler_digest())

    def _val(self, i):
        n = self.g.nodes[i]
        return _lit(n[1]) if n[0] == "const" else (f"c{n[1]}" if n[0] == "coord" else f"v{i}")

    def point_fn_source(self):
        used = sorted({self.g.nodes[i][1] for i in self.order if self.g.nodes[i][0] == "coord"})
        L = [f"  const float c{c} = v[{c}];" for c in used]
        L += _forward_lines(self.g, self.order, self._val)
        L += [f"  v[{r}] = {self._val(i)};" for r, i in enumerate(self.outs)]
        L.append(f"  keep = {self._val(self.keep)} != 0.0f;" if self.keep is not None else "  keep = true;")
        return ("NDQ_MAP_INLINE void ndq_map_point(float (&v)[6], bool& keep) {\n" + "\n".join(L) + "\n}\n")

    def _emit(self):
        return f"""// GENERATED by neurodiffeq_amd/codegen.py -- the per-point stages (TransformGenerator / FilterGenerator callables) of one
// device-drawn generator: {self.d_in} row(s) of a plan point in, {self.d_out} row(s) out{', a keep mask' if self.keep is not None else ''}.
#define NDQ_MAP_DIN {self.d_in}
#define NDQ_MAP_DOUT {self.d_out}
#define NDQ_MAP_FILTER {int(self.keep is not None)}
#ifdef __HIPCC__
#include "ndq_sample.h"
#define NDQ_MAP_INLINE __device__ __forceinline__
#pragma clang fp contract(off)
#else
#include <math.h>
#define NDQ_MAP_INLINE static inline
#endif
{self.point_fn_source()}
#ifdef __HIPCC__
#include "ndq_sample_map.h"
#else
// rows [NDQ_MAP_DIN][n] -> out [NDQ_MAP_DOUT][n], keep [n]: ndq_map_point at every point (host build, for tests)
extern "C" void ndq_map_cpu(const float* rows, int n, float* out, unsigned char* keep) {{
  for (int i = 0; i < n; ++i) {{
    float v[6] = {{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}};
    for (int c = 0; c < NDQ_MAP_DIN; ++c) v[c] = rows[(size_t)c * n + i];
    bool k = true;
    ndq_map_point(v, k);
    for (int c = 0; c < NDQ_MAP_DOUT; ++c) out[(size_t)c * n + i] = v[c];
    keep[i] = k ? 1 : 0;
  }}
}}
#endif
"""


class SamplerMapKernel:
    def __init__(self, so_path):
        self.path = so_path
        self.lib = ctypes.CDLL(so_path)
        vp, ci, u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_ulonglong
        self.lib.ndq_map_launch.restype = ci
        self.lib.ndq_map_launch.argtypes = [vp, vp, u64, u64, ctypes.c_uint, vp, ci, ci, vp, ci, vp]
        self.rows_in, self.rows_out = self.lib.ndq_map_rows_in(), self.lib.ndq_map_rows_out()
        self.filters = bool(self.lib.ndq_map_filters())
        self.launch = self.lib.ndq_map_launch


def build_sampler_map(program: SamplerMapProgram, force=False):
    """Compile the map / filter module of ``program`` for gfx950 (in-tree cache keyed by the generated source, the sampler headers
    and the flags) and return the .so path."""
    os.makedirs(JIT_DIR, exist_ok=True)
    so = os.path.join(JIT_DIR, f"smap_{program.key}.so")
    src = so[:-3] + ".hip"
    if os.path.exists(so) and not force:
        return so
    with open(src, "w") as fh:
        fh.write(program.source)
    try:
        _hipcc.compile_shared(src, so, _extra_flags(), defer=True)
    except RuntimeError as e:
        raise RuntimeError(f"hipcc failed for generated sampler map module {src}:\n{str(e)[-4000:]}") from e
    return so


_MAP_MODULES = {}


def load_sampler_map(program: SamplerMapProgram):
    k = _MAP_MODULES.get(program.key)
    if k is None:
        k = _MAP_MODULES[program.key] = SamplerMapKernel(build_sampler_map(program))
    return k


def build_sampler_map_cpu(program: SamplerMapProgram, force=False):
    """The same source through the host C++ compiler (the ``#else`` branches): ``ndq_map_cpu`` runs ``ndq_map_point`` over a
    batch of rows.  No GPU, no hipcc; no contraction, like ndq_map_point in the device build."""
    os.makedirs(JIT_DIR, exist_ok=True)
    so = os.path.join(JIT_DIR, f"smap_cpu_{program.key}.so")
    if os.path.exists(so) and not force:
        return so
    src = so[:-3] + ".cpp"
    with open(src, "w") as fh:
        fh.write(program.source)
    import subprocess
    tmp = f"{so}.{os.getpid()}.tmp"
    cxx = os.environ.get("CXX", "g++")
    proc = subprocess.run([cxx, "-O2", "-std=c++17", "-fno-fast-math"] + MAP_HOST_FLAGS + ["-shared", "-fPIC", src, "-o", tmp],
                          capture_output=True, text=True)
    if proc.returncode != 0:
        raise RuntimeError(f"{cxx} failed for generated sampler map module {src}:\n{proc.stderr[-4000:]}")
    os.replace(tmp, so)
    return so


def run_sampler_map_cpu(program: SamplerMapProgram, rows):
    """rows [d_in][n] fp32 -> (out [d_out][n] fp32, keep [n] bool) through the host build."""
    import numpy as np
    lib = ctypes.CDLL(build_sampler_map_cpu(program))
    rows = np.ascontiguousarray(rows, dtype=np.float32).reshape(program.d_in, -1)
    n = rows.shape[1]
    out, keep = np.zeros((program.d_out, n), np.float32), np.zeros(n, np.uint8)
    lib.ndq_map_cpu.restype = None
    lib.ndq_map_cpu.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    lib.ndq_map_cpu(rows.ctypes.data, n, out.ctypes.data, keep.ctypes.data)
    return out, keep.astype(bool)


# ----------------------------------------------------------------------------------------------- MLP kernel extensions
# libndq.so carries a table of (shape, stream set) kernel pairs; anything else the templates can express is compiled
# on first use as a tiny extension module (one Cfg: forward + adjoint kernel) and registered with libndq.so, after
# which the ordinary C-ABI entry points serve it.  Cached in-tree like the generated pointwise kernels.
_MLP_EXT = {}


MAX_INPUTS = 6          # network inputs the templates are instantiated for (Streams<D, ...>: D (D + 1) / 2 pair bits)
MAX_LAYERS = 8          # hidden layers of one width (networks.describe); the LDS footprint decides at registration


def mlp_ext_allowed(desc):
    """Can ndq_mlp.h express this descriptor?  (H = 1..64, 1..8 hidden layers of one width or 1..4 of different widths,
    d <= 6; the LDS footprint is checked by ndq_mlp_register once the module is built.)"""
    if os.environ.get("NDQ_JIT_MLP", "1") == "0":
        return False
    npair = desc.d * (desc.d + 1) // 2
    diag = 0
    for a in range(desc.d):
        diag |= 1 << pair_list(desc.d).index((a, a))
    if desc.mask3:              # third order: tanh / sin / sigmoid, every triple with its three pairs, no Laplacian stream,
        #                         d <= 4 (five inputs have more triples than the 32 mask bits)
        if desc.lap or desc.d > 4 or desc.act not in (0, 1, 2, 5, 6, 7) or desc.mask3 >> len(triple_list(desc.d)):
            return False
        for k, (a, b, c) in enumerate(triple_list(desc.d)):
            if (desc.mask3 >> k) & 1 and not all((desc.mask2 >> pair_list(desc.d).index(p)) & 1
                                                   for p in ((a, b), (a, c), (b, c))):
                return False
    if desc.mask4:              # fourth order (round 6): tanh / sin / sigmoid, d <= 3, every quadruple with its pairs and triples
        if (desc.lap or desc.d > 3 or desc.act not in (0, 1, 2) or desc.actp or desc.mono or is_wide(desc)
                or desc.mask4 >> len(quad_list(desc.d))):
            return False
        for k, q in enumerate(quad_list(desc.d)):
            if (desc.mask4 >> k) & 1:
                for i in range(4):
                    tri = tuple(q[j] for j in range(4) if j != i)
                    if not (desc.mask3 >> triple_list(desc.d).index(tri)) & 1:
                        return False
                    for j in range(i + 1, 4):
                        if not (desc.mask2 >> pair_list(desc.d).index((q[i], q[j]))) & 1:
                            return False
    if desc.widths:           # per-layer widths: 1..hidden each, the widest equal to `hidden`, nothing beyond `layers`
        bits, most = (10, 3) if is_wide(desc) else (8, 4)      # (csrc/ndq_deep.h: 10 bits x 2 .. 3 layers; csrc/ndq_mlp.h: 8 x 4)
        ws = [(desc.widths >> (bits * l)) & ((1 << bits) - 1) for l in range(most)]
        if (desc.widths >> (bits * most)) or desc.layers > most or any(w for w in ws[desc.layers:]) or min(ws[:desc.layers]) < 1 \
                or max(ws[:desc.layers]) != desc.hidden or (is_wide(desc) and desc.layers < 2):
            return False
    if desc.mono and (not 0 < desc.mono < 256 or desc.mask3 or desc.skip or desc.hidden > 48):
        return False          # monomial features: degrees 1..8, up to second order, H <= 48, no skip connection
    if is_wide(desc) and (desc.skip or desc.actp or desc.mono or desc.n_out > 16):
        return False          # wider than 64 units (csrc/ndq_wide.h: one hidden layer; csrc/ndq_deep.h: 2 .. 8): plain FCNN
    return (1 <= desc.d <= MAX_INPUTS and 1 <= desc.hidden <= MAX_HIDDEN and 1 <= desc.layers <= (4 if desc.widths else MAX_LAYERS)
            and desc.act in (0, 1, 2, 3, 4, 5, 6, 7) and 1 <= desc.n_out <= 64 and desc.first in (0, 1)
            and 0 <= desc.mask2 < (1 << npair) and (desc.first == 1 or desc.mask2 == 0)
            and (desc.lap == 0 or (desc.n_out == 1 and desc.mask2 != 0 and (desc.mask2 & ~diag) == 0))
            and desc.skip in (0, 1) and desc.actp in (0, 1, 2) and (desc.actp == 0 or desc.act in (3, 4)))


MAX_HIDDEN = 512        # include/ndq.h NDQ_MAX_HIDDEN


def is_wide(desc):
    """Shapes served by csrc/ndq_wide.h (units over lanes, weights in registers) instead of csrc/ndq_mlp.h (16-point MFMA
    fragments, weights resident in LDS): hidden layers wider than 64 units."""
    return desc.hidden > 64


def mlp_cfg(desc, n_out):
    """The ndq::Cfg instantiation of a descriptor with ``n_out`` outputs (csrc/ndq_mlp.h: hidden layers of up to 64 units)."""
    return (f"ndq::Cfg<{desc.d}, {desc.first}, {desc.mask2}u, {(desc.hidden + 15) // 16}, {desc.layers}, {desc.act}, {n_out}, "
            f"{desc.lap}, {desc.skip}, {desc.mask3}u, {desc.actp}, {desc.hidden if (desc.hidden % 16 or desc.widths) else 0}, "
            f"{desc.widths}u, {desc.mono}u{_m4_arg(desc)}>")


def deep_cfg(desc):
    """The ndq::DeepCfg instantiation of a descriptor (2 .. 8 hidden layers of 65 .. 512 units, csrc/ndq_deep.h)."""
    return (f"ndq::DeepCfg<{desc.d}, {desc.first}, {desc.mask2}u, {desc.lap}, {desc.mask3}u, {desc.hidden}, {desc.layers}, "
            f"{desc.act}, {desc.n_out}" + (f", {desc.widths}u>" if desc.widths else ">"))


def wide_cfg(desc):
    """The ndq::WideCfg instantiation of a descriptor (one hidden layer of 65 .. 512 units)."""
    return (f"ndq::WideCfg<{desc.d}, {desc.first}, {desc.mask2}u, {desc.lap}, {desc.mask3}u, {desc.hidden}, {desc.act}, "
            f"{desc.n_out}>")


#: extra hipcc flags of modules built from csrc/ndq_wide.h: its tile code is 16 rounds x U units of independent scalar
#: chains; the SLP vectoriser pairs them ACROSS rounds into v_pk_* (no faster on gfx950: a packed fp32 op issues like two),
#: which drags every round's live values to the end of the tile -- 512 VGPRs + 200 .. 700 spilled against 227 without
WIDE_FLAGS = ["-fno-slp-vectorize"]


def padded_width(hidden):
    """Width the kernels lay a hidden layer out for: the next multiple of 16 (csrc/ndq_mlp.h: Cfg::H vs Cfg::HR)."""
    return (hidden + 15) // 16 * 16


def mlp_ext_source(desc, f64=False):
    header = "ndq_launch.h"              # -I csrc, as above
    record = "ndq64_mlp_kernels" if f64 else "ndq_mlp_kernels"
    if is_wide(desc) and desc.layers >= 2:
        return f"""// GENERATED by neurodiffeq_amd/codegen.py -- layer-by-layer forward / adjoint kernels of one deep FCNN wider than 64
// units (csrc/ndq_deep.h)
#include "{header}"
using CFG = {deep_cfg(desc)};
extern "C" const {record}* ndq_ext_kernels(void) {{
  static const {record} k = ndq::make_deep_kernels<CFG>();
  return &k;
}}
// 1: the next adjoint call may use the activations the last forward call left in the workspace (same parameters, same batch)
extern "C" void ndq_ext_reuse_forward(int on) {{ ndq::deep_last().reuse = on != 0; }}
"""
    if is_wide(desc):
        return f"""// GENERATED by neurodiffeq_amd/codegen.py -- forward-stream and adjoint kernels of one single-hidden-layer FCNN wider
// than 64 units (csrc/ndq_wide.h)
{"#define NDQ_F64 1" if f64 else ""}
#include "{header}"
using CFG = {wide_cfg(desc)};
extern "C" const {record}* ndq_ext_kernels(void) {{
  static const {record} k = ndq::make_wide_kernels<CFG>();
  return &k;
}}
"""
    return f"""// GENERATED by neurodiffeq_amd/codegen.py -- forward-stream and adjoint kernels of one FCNN shape / stream set
{"#define NDQ_F64 1" if f64 else ""}
#include "{header}"
using CFG = {mlp_cfg(desc, desc.n_out)};
extern "C" const {record}* ndq_ext_kernels(void) {{
  static const {record} k = ndq::make_kernels<CFG>();
  return &k;
}}
"""


def build_mlp_ext(desc, force=False, f64=False):
    os.makedirs(JIT_DIR, exist_ok=True)
    source = mlp_ext_source(desc, f64)
    key = _cache_key(source)
    so = os.path.join(JIT_DIR, f"mlp{'64' if f64 else ''}_{key}.so")
    src = os.path.join(JIT_DIR, f"mlp{'64' if f64 else ''}_{key}.hip")
    if os.path.exists(so) and not force:
        return so
    with open(src, "w") as fh:
        fh.write(source)
    try:
        _hipcc.compile_shared(src, so, _extra_flags() + (WIDE_FLAGS if is_wide(desc) and desc.layers == 1 else []))
    except RuntimeError as e:
        raise RuntimeError(f"hipcc failed for MLP kernel extension {src}:\n{str(e)[-4000:]}") from e
    return so


def ensure_mlp_kernels(desc, f64=False):
    """True if libndq.so (``f64``: libndq64.so) can serve ``desc`` -- from its table, or after building + registering an
    extension module."""
    from . import _lib
    L = _lib.lib64() if f64 else _lib.lib()
    supported = L.ndq64_mlp_supported if f64 else L.ndq_mlp_supported
    register = L.ndq64_mlp_register if f64 else L.ndq_mlp_register
    if supported(ctypes.byref(desc)):
        return True
    # fp64: twice the LDS per weight -- ndq64_mlp_register turns down what does not fit; wider than 64 units only ONE hidden
    # layer (csrc/ndq_wide.h compiled in double: forward-stream and adjoint kernels; csrc/ndq_deep.h is fp32 only)
    if not mlp_ext_allowed(desc) or (f64 and desc.hidden > 64 and desc.layers != 1):
        return False
    key = desc.key() + (("f64",) if f64 else ())
    if key in _MLP_EXT:
        return _MLP_EXT[key] is not None
    _MLP_EXT[key] = None
    try:
        ext = ctypes.CDLL(build_mlp_ext(desc, f64=f64))
    except RuntimeError as e:                     # the templates reject this combination: not a supported shape
        import warnings
        warnings.warn(f"could not build an MLP kernel extension for {key}: {str(e)[:400]}")
        return False
    except OSError as e:                          # no hipcc / unreadable module: the native path is broken, say so
        raise _lib.NdqError(f"cannot build or load the MLP kernel extension for {key}: {e}") from e
    ext.ndq_ext_kernels.restype = ctypes.c_void_p
    if register(ctypes.c_void_p(ext.ndq_ext_kernels())) != 0:
        return False                              # e.g. the shape needs more LDS than a workgroup has
    _MLP_EXT[key] = ext                           # keep the module (and its record) alive
    return bool(supported(ctypes.byref(desc)))


def mlp_ext_module(desc, f64=False):
    """The loaded extension module serving ``desc`` (None: the descriptor is served by libndq.so's own table)."""
    return _MLP_EXT.get(desc.key() + (("f64",) if f64 else ()))


def can_fuse_f64(program, descs):
    """fp64 systems: the single-launch closure exists for ONE network on the plain closure kernel (no grouped / wide /
    multi-network variant in double)."""
    mode = fuse_mode(program, descs)        # (one network: of the modes with an fp64 build, only the plain closure can come back)
    return program.n_nets == 1 and mode is not None and MODES[mode].f64 and descs[0].hidden <= 64


def can_fuse_multi_f64(program, descs):
    """fp64 systems of 2..4 networks: the multi-network closure kernel compiled in double (``fuse_mode`` "multi": one shape
    and stream set, one output each, every network reading all coordinates, padded width <= 48) -- no evaluation sites, no
    third- / fourth-order streams, no skip weights / trainable activation parameters / monomial front end.  Whether the
    module fits the LDS of one workgroup is the engine's question to the built module (``ndq_fused_lds_bytes``).
    ``can_fuse_f64`` keeps its meaning: the one-network closure."""
    K = program.n_nets
    if not (2 <= K <= 4) or program.n_sites != K or descs is None:
        return False
    mode = fuse_mode(program, descs)        # (2..4 networks, as many sites: of the modes with an fp64 build, only "multi")
    if mode is None or not MODES[mode].f64:
        return False
    d0 = descs[0]
    if d0.n_out != 1 or _high_order(d0) or d0.skip or d0.actp or d0.mono:
        return False
    return not any(_high_order(program.streams[k]) for k in range(K))


def fused_build_plan(program: PointwiseProgram, desc, threads=None, f64=False, more_flags=()):
    """What ``build_fused`` compiles, without compiling it: (source, extra hipcc flags, cache key) of the closure module."""
    source = program.fused_source(desc, f64=f64)
    flags = (_extra_flags() + list(more_flags) + ([f"-DNDQ_BWD_THREADS={int(threads)}"] if threads else [])
             + (WIDE_FLAGS if program.closure_mode(desc).wide_flags else []))
    return source, flags, _cache_key(source + (f"|threads={int(threads)}" if threads else ""), more_flags)


def build_fused(program: PointwiseProgram, desc, force=False, threads=None, f64=False, more_flags=()):
    """Compile the fused closure kernel of a single-network system for gfx950 (in-tree cache keyed by the generated
    source AND the kernel header it instantiates).  ``threads=512``: the 8-wave build (two waves per SIMD where the
    per-wave state fits 256 registers; csrc/ndq_mlp.h NDQ_BWD_THREADS) the engine uses for large batches.
    ``more_flags``: compile flags behind those of NDQ_JIT_FLAGS, as if they had been given there (the same cache entry)."""
    os.makedirs(JIT_DIR, exist_ok=True)
    source, flags, key = fused_build_plan(program, desc, threads, f64, more_flags)
    so = os.path.join(JIT_DIR, f"fused_{key}.so")
    src = os.path.join(JIT_DIR, f"fused_{key}.hip")
    if os.path.exists(so) and not force:
        return so
    with open(src, "w") as fh:
        fh.write(source)
    try:
        _hipcc.compile_shared(src, so, flags, defer=True)
    except RuntimeError as e:
        raise RuntimeError(f"hipcc failed for generated fused kernel {src}:\n{str(e)[-4000:]}") from e
    return so


#: What a closure mode is, beyond the rule that selects it (``fuse_mode``): the facts the engine and the build ask about and the
#: C++ texts its generated module is assembled from (``PointwiseProgram._fused_source``, ``_closure_host``).  In the texts {N} is
#: the number of parameter sets, {R} the number of stream rows -- networks, or evaluation sites -- and {train} the kernel's mode.
ClosureMode = namedtuple("ClosureMode", [
    "header",        # kernel header, found through -I csrc (_hipcc.BASE_FLAGS): sources and cache keys do not depend on the checkout path
    "rows",          # per-point interface: False = jets[R][NS] / gj arrays, True = srow / grow rows through the LDS exchange
    "padded_rows",   # rows: a stream's outputs are padded to 16 (ndq::group_w)
    "traits",        # the module carries the site traits (_site_traits); no pull mode then
    "wg_tr",         # the preamble sets NDQ_WG_TR / NDQ_WG_TR_K
    "products",      # the preamble carries CLOSURE_PRODUCTS
    "off",           # environment variable that turns the mode off, or None
    "f64",           # a build in double exists
    "eight_wave",    # an 8-wave build can exist (engine.FusedSystem._wide_possible) ...
    "eight_wave_opt_in",    # ... only if this environment variable is "1"
    "wide_flags",    # compiled with WIDE_FLAGS
    "what", "blocks_note", "apply_head",         # title comment, NDQ_MAX_BLOCKS comment, head of PW::apply (jets)
    "cfg", "args", "threads", "points", "slots", "kern", "tv", "lds", "loop", "lds_loop", "loop_max"])

_APPLY = """  // xe: the point's ND data values, then the NT scalars;  gth (want_adj): per-point adjoints of the scalars
  static __device__ __forceinline__ void apply(const float (&x)[CFG::D], const float* xe, {jets}, float seed,
                                               int want_adj, {r}, {f},
                                               {gj}, float* gth) {{"""
_APPLY_SITES = """  // x: the batch point (every site's real inputs);  jets / gj: streams and their adjoints, per SITE
  static __device__ __forceinline__ void apply(const float (&x)[CFG::D], const float* xe, {jets},
                                               float seed, int want_adj, {r}, {f},
                                               {gj}, float* gth) {{"""
_TILE = ClosureMode(
    header="ndq_mlp.h", rows=False, padded_rows=False, traits=False, wg_tr=True, products=True, off=None, f64=True,
    eight_wave=True, eight_wave_opt_in=None, wide_flags=False, what=" with {N} network(s)",
    blocks_note="(one per CU; experiments: 512 = two 8-wave workgroups per CU)", apply_head=_APPLY,
    cfg=lambda desc: mlp_cfg(desc, 1), args="FusedArgs", threads="CFG::BWD_THREADS", points="16", slots="CFG::BWD_THREADS / 64",
    kern="ndq::fused_closure_kernel<CFG, PW, {train}>", tv="ndq::fused_closure_tv_kernel<CFG, PW>",
    lds="ndq::fused_lds_bytes<CFG>({train})", loop="ndq::fused_closure_loop_kernel<CFG, PW>",
    lds_loop="ndq::fused_loop_lds_bytes<CFG>()", loop_max=1)
# workgroup shape: waves x tiles per round (multi-network closure: R x G waves, G tile slots -- csrc/ndq_mlp.h).  No 8-wave
# build: R x G waves, one per SIMD, whatever the batch size (multi_threads)
_MULTI = _TILE._replace(
    off="NDQ_NO_MULTI_FUSE", eight_wave=False, args="FusedMultiArgs", threads="ndq::multi_threads<{R}>()",
    slots="ndq::multi_group<{R}>()", kern="ndq::fused_multi_closure_kernel<CFG, {R}, PW, {train}>",
    tv="ndq::fused_multi_closure_tv_kernel<CFG, {R}, PW>", lds="(ndq::fused_multi_lds_bytes<CFG, {R}>({train}))",
    loop="ndq::fused_multi_closure_loop_kernel<CFG, {R}, PW>", lds_loop="(ndq::fused_multi_loop_lds_bytes<CFG, {R}>())", loop_max=2)
_GROUP = _TILE._replace(
    rows=True, padded_rows=True, wg_tr=False, off="NDQ_NO_GROUP_FUSE", f64=False, what="", apply_head=None,
    eight_wave_opt_in="NDQ_GROUP_WIDE",         # experiment: 8 waves with 32-point groups
    cfg=lambda desc: mlp_cfg(desc, desc.n_out), points="16 * ndq::group_tiles<CFG>()",
    kern="ndq::fused_group_closure_kernel<CFG, PW, {train}>", tv="ndq::fused_group_closure_tv_kernel<CFG, PW>",
    lds="ndq::group_lds_bytes<CFG>({train})", loop=None, lds_loop=None, loop_max=0)
_WIDE = _GROUP._replace(
    header="ndq_wide.h", padded_rows=False, off="NDQ_NO_WIDE_FUSE", eight_wave_opt_in=None, wide_flags=True, cfg=lambda desc: wide_cfg(desc),
    points="16", kern="ndq::wide_closure_kernel<CFG, PW, {train}>", tv="ndq::wide_closure_tv_kernel<CFG, PW>",
    lds="(ndq::wide_closure_lds_bytes<CFG, PW>())")
# no 8-wave build: one wave per SIMD holds R networks' accumulators (csrc/ndq_wide.h: NDQ_WIDE_THREADS)
_WIDE_MULTI = _WIDE._replace(
    off="NDQ_NO_WIDE_MULTI_FUSE", eight_wave=False, what=" with {R} networks", args="FusedMultiArgs",
    kern="ndq::wide_multi_closure_kernel<CFG, {R}, PW, {train}>", tv="ndq::wide_multi_closure_tv_kernel<CFG, {R}, PW>",
    lds="(ndq::wide_multi_closure_lds_bytes<CFG, {R}, PW>())")
MODES = {
    "tile": _TILE, "multi": _MULTI, "group": _GROUP, "wide": _WIDE, "wide_multi": _WIDE_MULTI,
    # R = 2..4 evaluation sites of N networks on R wave groups: stream arrays per site, parameter sets and gradient partials per
    # network behind the multi-network argument struct (N = 1 included).  No CLOSURE_PRODUCTS: every GEMM keeps all six bf16
    # plane products.  A network's gradient is the SUM of its sites' and those nearly cancel (u - u(x_b) - w u_x(x_b): the
    # output bias drops out exactly), so the 4- / 3-product reverse and weight-gradient GEMMs of the other closure modules,
    # 1e-6 of each site's gradient, come to 1e-5 of the network's (measured: heat equation with two Neumann ends 1.25e-5
    # against fp64 with them, 2e-7 without); these systems are launch-bound
    "sites": _MULTI._replace(
        traits=True, products=False, off="NDQ_NO_SITE_FUSE", f64=False, what=" with {N} network(s) at {R} evaluation sites",
        blocks_note="(one per CU)", apply_head=_APPLY_SITES, kern="ndq::fused_multi_closure_kernel<CFG, {R}, PW, {train}, SITES>",
        tv="ndq::fused_multi_closure_tv_kernel<CFG, {R}, PW, SITES>", loop=None, lds_loop=None, loop_max=0),
    # R slices, N unit images (csrc/ndq_wide.h: wide_multi_closure_body with site traits); parameter sets and gradient
    # partials per network behind the multi-network argument struct, as the narrow site modules
    "wide_sites": _WIDE_MULTI._replace(
        traits=True, off="NDQ_NO_WIDE_SITE_FUSE", what=" with {N} network(s) at {R} evaluation sites",
        kern="ndq::wide_multi_closure_kernel<CFG, {R}, PW, {train}, SITES>",
        tv="ndq::wide_multi_closure_tv_kernel<CFG, {R}, PW, SITES>", lds="(ndq::wide_multi_closure_lds_bytes<CFG, {R}, PW, {N}>())"),
}


def fuse_mode(program: PointwiseProgram, descs=None):
    """Which single-launch closure kernel serves the system, if any:
    "tile"   one single-output network reading all coordinates (fused_closure_kernel),
    "multi"  2..4 such networks of ONE shape and stream set, H <= 48 (fused_multi_closure_kernel),
    "group"  one network with several outputs and / or reading only some of the batch coordinates, H <= 48
             (fused_group_closure_kernel: per-point stage on one point per lane through an LDS exchange tile);
             NDQ_FUSE_GROUP=1 sends every eligible single-network system there.
    "wide"   one network with ONE hidden layer of 65 .. 512 units (csrc/ndq_wide.h: wide_closure_kernel),
    "wide_multi"  2..4 such networks of one shape, stream set and input coordinates (wide_multi_closure_kernel);
             NDQ_NO_WIDE_MULTI_FUSE is its off-switch.
    "sites"  networks evaluated on a boundary as well (Neumann ends): 2..4 evaluation sites of fewer networks, all of one
             shape and stream set, one output, H <= 48, fp32, no third- / fourth-order streams; every site reads all batch
             coordinates, some of them replaced by a boundary value (fused_multi_closure_kernel with site traits, one wave
             group per site); NDQ_NO_SITE_FUSE is its off-switch.
    "wide_sites"  the same family on networks with ONE hidden layer of 65 .. 512 units: 2..4 sites of fewer networks of one
             shape and stream set, one output, fp32, no skip / trainable activation parameters / monomial front end, no
             third- / fourth-order streams (wide_multi_closure_kernel with site traits: one wave runs all sites of a tile
             and sums a network's gradient over its sites in its own registers); NDQ_NO_WIDE_SITE_FUSE is its off-switch.
    None     three-kernel pipeline."""
    K, S, nc = program.n_nets, program.n_sites, program.n_coords
    d0 = descs[0] if descs is not None and 0 in descs else None
    if K >= 1 and S > K:
        wide = d0 is not None and is_wide(d0)
        if not _sites_ok(program, descs) or _switched_off("wide_sites" if wide else "sites"):
            return None
        if wide:
            return "wide_sites" if _wide_one_layer(d0.hidden, d0.layers, d0.skip, d0.actp, d0.mono) else None
        return "sites" if _fits_multi(d0.hidden) else None
    if K < 1 or K > 4 or S != K or any(k not in program.streams for k in range(K)):
        return None
    streams = [program.streams[k] for k in range(K)]
    plain = all(tuple(st.deps) == tuple(range(nc)) and st.n_out == 1 for st in streams)
    batch_inputs = all(c < nc for c in streams[0].deps)       # network 0 reads batch coordinates only, any subset of them
    if K == 1:
        if d0 is not None and is_wide(d0):
            # one hidden layer wider than 64 units: csrc/ndq_wide.h's closure kernel (any number of outputs, any subset of
            # the batch coordinates as inputs)
            return "wide" if (d0.layers == 1 and batch_inputs and not _switched_off("wide")) else None
        group_ok = d0 is not None and _fits_multi(d0.hidden) and batch_inputs and not _switched_off("group")
        if plain and not (group_ok and os.environ.get("NDQ_FUSE_GROUP") == "1"):     # (the redirect takes PLAIN systems too)
            return "tile"
        return "group" if group_ok else None
    if descs is not None and all(k in descs for k in range(K)) and any(is_wide(descs[k]) for k in range(K)):
        # (one descriptor, so network 0's width is every network's; no descriptor exceeds MAX_HIDDEN)
        ok = (_one_shape(descs, K) and _wide_one_layer(d0.hidden, d0.layers, d0.skip, d0.actp, d0.mono) and batch_inputs
              and all(tuple(st.deps) == tuple(streams[0].deps) for st in streams) and not _switched_off("wide_multi"))
        return "wide_multi" if ok else None
    if not plain:
        return None
    if descs is None or not _one_shape(descs, K) or not _fits_multi(descs[0].hidden):
        return None
    return None if _switched_off("multi") else "multi"


def _sites_ok(program, descs):
    """``fuse_mode``: what both evaluation-site closure kernels ask of a system, whatever the width of its networks.
    (fp64 systems never get here with a say: the modes with sites have no fp64 build.)"""
    S = program.n_sites
    if not (2 <= S <= 4) or any(k not in program.streams for k in range(S)):
        return False
    if descs is None or any(k not in descs for k in range(S)) or not _one_shape(descs, S):
        return False
    if descs[0].n_out != 1 or _high_order(descs[0]):
        return False
    return all(st.n_out == 1 and not _high_order(st) and _site_inputs(st.deps, program.n_coords, program.g.vcoords)
               for st in (program.streams[k] for k in range(S)))


# ---- the conditions the rules above and ``unify`` share, each stated once
def _switched_off(name):
    """Is closure mode ``name`` turned off by its environment variable?"""
    off = MODES[name].off
    return bool(off and os.environ.get(off))


def _one_shape(descs, n):
    """Do sites 0 .. n-1 have ONE descriptor (network shape and stream set)?"""
    return len({descs[k].key() for k in range(n)}) == 1


def _fits_multi(hidden):
    """The narrow multi-row kernels (multi, sites, group) hold their weight images in LDS: padded width up to 48."""
    return padded_width(hidden) <= 48


def _wide_one_layer(hidden, layers, skip, actp, mono):
    """What csrc/ndq_wide.h's multi-row closure kernels take: ONE hidden layer of 65 .. 512 units, plain FCNN."""
    return 64 < hidden <= MAX_HIDDEN and layers == 1 and not (skip or actp or mono)


def _high_order(st):
    """Third- or fourth-order streams in a stream set (``NetStreams``) or a descriptor."""
    return bool(st.mask3 or getattr(st, "mask4", 0))


def _site_inputs(deps, n_coords, vcoords):
    """Entry a of an evaluation site's inputs: batch coordinate a, or a boundary value."""
    return len(deps) == n_coords and all(c == a or c in vcoords for a, c in enumerate(deps))


def unify(streams, site_net, n_coords, vcoords, infos, f64):
    """The ``unify`` hook of ``PointwiseProgram``.  2..4 networks of ONE shape reading all coordinates: give them the union
    of their stream sets, so that the multi-network closure kernel (one launch for the whole system) can serve them; a network
    then carries at most a few streams it does not need -- these systems are launch-bound, not compute-bound.  The same for
    2..4 evaluation sites of fewer networks ("sites", "wide_sites"): every site reads all batch coordinates, some replaced by
    a boundary value -- stream sets are per input POSITION.  streams: {site: NetStreams}; infos: ``networks.describe`` per network.
    It decides BEFORE the descriptors exist what ``fuse_mode`` decides after them, from the same predicates.  Kept as they are:
    fp64 leaves site systems alone (no fp64 build with sites) but unifies plain multi-network ones (``can_fuse_multi_f64``, which
    NDQ_NO_MULTI_FUSE turns off with the fp32 mode); the wide-site test here also asks for ``widths == 0``; wide networks
    WITHOUT sites ("wide_multi") are not unified, their width fails ``_fits_multi``."""
    K, S, i0 = len(infos), len(site_net), infos[0]
    wide_sites = (S > K and _wide_one_layer(i0["hidden"], i0["layers"], i0["skip"], i0["actp"], i0["mono"])
                  and not i0["widths"])
    if S > K:
        if not (2 <= S <= 4) or len(streams) != S or f64 or _switched_off("wide_sites" if wide_sites else "sites"):
            return
        if not all(_site_inputs(st.deps, n_coords, vcoords) for st in streams.values()):
            return
    elif not (2 <= K <= 4) or len(streams) != K or _switched_off("multi"):
        return
    shape = {(i["d"], i["hidden"], i["layers"], i["act"], i["n_out"], i["skip"], i["actp"], i["widths"], i["mono"]) for i in infos}
    if len(shape) != 1 or i0["n_out"] != 1 or not (wide_sites or _fits_multi(i0["hidden"])):
        return
    if S == K and any(tuple(st.deps) != tuple(range(n_coords)) for st in streams.values()):
        return
    sts = list(streams.values())
    if any(_high_order(st) for st in sts):
        return              # third- / fourth-order stream sets are served network by network (three-kernel pipeline)
    if len({(st.first, st.mask2, st.lap) for st in sts}) == 1:
        return
    lap = max(st.lap for st in sts)
    if lap and any((not st.lap) and st.mask2 for st in sts):
        return              # some network needs its second derivatives one by one, another only their sum
    first, mask2 = max(st.first for st in sts), 0
    for st in sts:
        mask2 |= st.mask2
    for st in sts:
        st.first, st.mask2, st.lap = first, mask2, lap


def can_fuse(program: PointwiseProgram, descs=None):
    return fuse_mode(program, descs) is not None
