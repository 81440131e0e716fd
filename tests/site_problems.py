"""Systems whose conditions have Neumann ends -- the network is evaluated on the boundary as well, a further *evaluation site*
of the same parameters -- which the "sites" single-launch closure serves (csrc/ndq_mlp.h: fused_multi_closure_kernel with site
traits), stated once for the product (neurodiffeq_amd) and once for the fp64 autograd oracle, from the same equations.  The
oracle's re-parameterisations are written here, independently of neurodiffeq_amd/conditions.py, from the reference's formulas
(conditions.py:512-884) on plain torch autograd: a boundary column is a fresh leaf the network is differentiated against.
Shared by tests/test_site_closure.py, tests/test_gpu_site_closure.py, scripts/site_closure_timing.py and the build step that
compiles these systems' modules ahead of the GPU tests.

Domains are NOT the unit interval and the boundary data depend on t, so a wrong literal or a swapped end shows."""
import torch

X0, X1 = -0.5, 1.5          # the space interval of every case
T0 = 0.25                   # initial time of the heat cases (t in [T0, T0 + 1])
KAPPA = 0.3                 # diffusivity; the trainable scalar's initial value in "heat-theta"
SCALE = 100.0               # second equation of the two-network systems: its gradient is ~1e4 times the first's

#: name -> (kind, site map, hidden units, activation)
CASES = {
    "heat-nd": ("heat", [0, 0], (32, 32), "tanh"),
    "heat-dn": ("heat", [0, 0], (32, 32), "tanh"),
    "heat-nn": ("heat", [0, 0, 0], (32, 32), "tanh"),
    "heat-nn-sin40": ("heat", [0, 0, 0], (40,), "sin"),        # 40 pads to 48: ragged unit rows
    "bvp-nn": ("bvp", [0, 0, 0], (32, 32), "tanh"),            # every input of both boundary sites is a boundary value
    "pair-011": ("pair", [0, 1, 1], (32, 32), "tanh"),
    "pair-010": ("pair", [0, 1, 0], (32, 32), "tanh"),
    "pair-0101": ("pair", [0, 1, 0, 1], (32, 32), "tanh"),
    "pair-0101-h40": ("pair", [0, 1, 0, 1], (40, 40), "tanh"),  # the largest module: four sites, two layers padded to 48
    "heat-theta": ("heat", [0, 0], (32, 32), "tanh"),          # the diffusivity is trainable (PW::NT = 1)
}
NAMES = list(CASES)
#: ends of every condition of a case: "d" Dirichlet, "n" Neumann, (x_min, x_max)
ENDS = {"heat-nd": ["nd"], "heat-dn": ["dn"], "heat-nn": ["nn"], "heat-nn-sin40": ["nn"], "bvp-nn": ["nn"],
        "pair-011": ["dd", "dn"], "pair-010": ["nd", "dd"], "pair-0101": ["nd", "dn"], "pair-0101-h40": ["nd", "dn"], "heat-theta": ["nd"]}
#: cases that also run at 4 097 points (one per site count) and at 16 400 (the grid is capped: waves take further trips)
MORE_BLOCKS = ["heat-nd", "heat-nn", "pair-0101"]
TILE_LOOP = ["heat-dn", "bvp-nn"]


def n_inputs(name):
    return 2 if CASES[name][0] == "heat" else 1


def n_nets(name):
    return max(CASES[name][1]) + 1


# ---- boundary data (functions of t for the heat cases, numbers for the two-point problems)
def _u_init(x):
    return torch.cos(2.0 * x) + 0.5 * x


def _left_val(t):
    return 0.3 * torch.sin(2.0 * t) + 0.1 * t


def _right_val(t):
    return 0.5 * t * t - 0.2 * t


def _left_prime(t):
    return 1.0 + 0.7 * t


def _right_prime(t):
    return torch.cos(3.0 * t) - 0.4


BVP_VALUES = dict(x_min_val=1.25, x_max_val=-0.75, x_min_prime=-0.5, x_max_prime=0.8)


def equations(name, d, theta=None):
    """Residuals of case ``name`` against a ``diff(u, t, order=1)``; ``theta``: the trainable scalars (``.theta`` of the result)."""
    kind = CASES[name][0]
    if name == "heat-theta":
        kappa = theta[0]
        eqs = lambda u, x, t: [d(u, t) - kappa * d(u, x, order=2) - torch.sin(x) * t]
    elif kind == "heat":
        eqs = lambda u, x, t: [d(u, t) - KAPPA * d(u, x, order=2) - torch.sin(x) * t]
    elif kind == "bvp":
        eqs = lambda u, x: [d(u, x, order=2) + u - torch.sin(x)]
    else:
        eqs = lambda u, v, x: [d(u, x, order=2) + u - v, SCALE * (d(v, x, order=2) - v + torch.sin(x) + 0.1 * u)]
    eqs.theta = list(theta or ())
    return eqs


def _theta(name, dtype):
    return [torch.nn.Parameter(torch.tensor(KAPPA, dtype=dtype))] if name == "heat-theta" else None


def _bvp_kwargs(ends):
    kw = {("x_min_val" if ends[0] == "d" else "x_min_prime"): None, ("x_max_val" if ends[1] == "d" else "x_max_prime"): None}
    return {k: BVP_VALUES[k] for k in kw}


def make(name):
    """(nets, conditions, equations, n_coords) of the product; draws the networks from torch's current RNG state."""
    from neurodiffeq_amd import diff
    from neurodiffeq_amd.conditions import IBVP1D, DoubleEndedBVP1D
    from neurodiffeq_amd.networks import FCNN, SinActv
    kind, _, hidden, act = CASES[name]
    actv = {"tanh": torch.nn.Tanh, "sin": SinActv}[act]
    nets = [FCNN(n_inputs(name), 1, hidden_units=hidden, actv=actv) for _ in range(n_nets(name))]
    conds = []
    for ends in ENDS[name]:
        if kind == "heat":
            kw = {("x_min_val" if ends[0] == "d" else "x_min_prime"): (_left_val if ends[0] == "d" else _left_prime),
                  ("x_max_val" if ends[1] == "d" else "x_max_prime"): (_right_val if ends[1] == "d" else _right_prime)}
            conds.append(IBVP1D(X0, X1, T0, _u_init, **kw))
        else:
            conds.append(DoubleEndedBVP1D(X0, X1, **_bvp_kwargs(ends)))
    return nets, conds, equations(name, diff, _theta(name, torch.float32)), n_inputs(name)


# ---- the oracle's re-parameterisations (plain torch)
def _at_boundary(net, xb, like, others):
    """(N(xb, ..), dN/dx(xb, ..)) with the boundary column a fresh leaf (conditions.py:577-579)."""
    col = torch.full_like(like, xb).requires_grad_(True)
    u = net(torch.cat([col] + list(others), dim=1))
    du, = torch.autograd.grad(u, col, grad_outputs=torch.ones_like(u), create_graph=True)
    return u, du


def _ibvp(ends):
    """conditions.py:669-712: u(x, T0) = u_init(x); a value or a slope at each end of [X0, X1]."""
    w = X1 - X0

    def enforce(net, x, t):
        u = net(torch.cat([x, t], dim=1))
        xt, grow = (x - X0) / w, 1 - torch.exp(-(t - T0))
        t0 = torch.full_like(t, T0)
        delta = lambda fn: fn(t) - fn(t0)
        if ends == "dn":
            u1, d1 = _at_boundary(net, X1, x, [t])
            return delta(_left_val) + _u_init(x) + xt * w * delta(_right_prime) + xt * grow * (u - w * d1 - u1)
        if ends == "nd":
            u0, d0 = _at_boundary(net, X0, x, [t])
            return delta(_right_val) + _u_init(x) + (xt - 1) * w * delta(_left_prime) + (1 - xt) * grow * (u + w * d0 - u0)
        u0, d0 = _at_boundary(net, X0, x, [t])
        u1, d1 = _at_boundary(net, X1, x, [t])
        a = _u_init(x) - 0.5 * (1 - xt) ** 2 * w * delta(_left_prime) + 0.5 * xt ** 2 * w * delta(_right_prime)
        return a + grow * (u - xt * w * d0 + 0.5 * xt ** 2 * w * (d0 - d1))
    return enforce


def _debvp(ends):
    """conditions.py:823-884: two-point conditions, a value or a slope at each end."""
    w, v = X1 - X0, BVP_VALUES

    def enforce(net, x):
        u = net(x)
        xt = (x - X0) / w
        if ends == "dd":
            return v["x_min_val"] * (1 - xt) + v["x_max_val"] * xt + xt * (1 - xt) * u
        if ends == "dn":
            u1, d1 = _at_boundary(net, X1, x, [])
            return (1 - xt) * v["x_min_val"] + 0.5 * xt ** 2 * v["x_max_prime"] * w + xt * (u - u1 + v["x_min_val"] - d1 * w)
        if ends == "nd":
            u0, d0 = _at_boundary(net, X0, x, [])
            return xt * v["x_max_val"] - 0.5 * (1 - xt) ** 2 * v["x_min_prime"] * w + (1 - xt) * (u - u0 + v["x_max_val"] + d0 * w)
        u0, d0 = _at_boundary(net, X0, x, [])
        u1, d1 = _at_boundary(net, X1, x, [])
        a = -0.5 * (1 - xt) ** 2 * w * v["x_min_prime"] + 0.5 * xt ** 2 * w * v["x_max_prime"]
        return a + 0.5 * xt ** 2 * (u - u1 - 0.5 * d1 * w) + 0.5 * (1 - xt) ** 2 * (u - u0 + 0.5 * d0 * w)
    return enforce


def make_oracle(name, dtype=torch.float64):
    """(nets, enforcers, equations) of the fp64 autograd oracle: same shapes, parameters to be set with ``R.set_flat``."""
    from oracle import autograd_ref as R
    kind, _, hidden, act = CASES[name]
    nets = [R.make_fcnn(n_inputs(name), 1, hidden, act, dtype) for _ in range(n_nets(name))]
    enf = [(_ibvp if kind == "heat" else _debvp)(ends) for ends in ENDS[name]]
    return nets, enf, equations(name, R.ref_diff, _theta(name, dtype))


def batch(name, n, seed):
    """``n`` points of the case's domain as a list of fp32 columns, from a generator of its own."""
    g = torch.Generator().manual_seed(seed)
    cols = [X0 + (X1 - X0) * torch.rand(n, generator=g, dtype=torch.float32)]
    if n_inputs(name) == 2:
        cols.append(T0 + torch.rand(n, generator=g, dtype=torch.float32))
    return cols


def trace(name):
    """(program, descs) of the case as the engine traces it (no GPU)."""
    from neurodiffeq_amd import engine
    torch.manual_seed(0)
    nets, conds, eqs, nc = make(name)
    return engine.trace_system(nets, conds, eqs, nc)


def boundary_literals(name):
    """What the module's traits must say: per site, {input position: boundary value}.  Sites follow the networks in the order the
    conditions ask for them: x_min before x_max, condition by condition."""
    out = [{} for _ in range(n_nets(name))]
    for ends in ENDS[name]:
        out += [{0: xb} for e, xb in zip(ends, (X0, X1)) if e == "n"]
    assert len(out) == len(CASES[name][1])
    return out

