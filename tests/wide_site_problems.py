"""The systems of tests/site_problems.py -- conditions with Neumann ends, whose networks are evaluated on the boundary as well
-- on networks with ONE hidden layer of 65 .. 512 units: what the "wide_sites" single-launch closure serves (csrc/ndq_wide.h:
wide_multi_closure_kernel with site traits).  Equations, boundary data and the fp64 oracle's re-parameterisations are those of
site_problems, stated there once for product and oracle; a case here names one of them, a width and an activation.
Shared by tests/test_wide_site_closure.py, tests/test_gpu_wide_site_closure.py, tests/golden/make_wide_site_golden.py,
scripts/wide_site_timing.py and the build step that compiles these systems' modules ahead of the GPU tests."""
import torch

from tests import site_problems as SP

#: name -> (system of site_problems, hidden units, activation).  Unit-lane layouts of csrc/ndq_wide.h's WideCfg: up to 128
#: units 16 unit lanes x 4 point lanes, up to 256 units 32 x 2, above 64 x 1; U = units per lane
CASES = {
    "heat-nd-65": ("heat-nd", 65, "tanh"),            # 16 lanes, U = 5, the last unit row holds ONE unit
    "heat-dn-128": ("heat-dn", 128, "tanh"),          # 16 lanes, U = 8, full rows
    "heat-nn-129": ("heat-nn", 129, "tanh"),          # 32 lanes, U = 5, ragged (4 x 32 + 1); three sites of one network
    "heat-nn-300-sin": ("heat-nn", 300, "sin"),       # 64 lanes, U = 5, ragged (4 x 64 + 44)
    "bvp-nn-512": ("bvp-nn", 512, "tanh"),            # 64 lanes, U = 8; every input of both boundary sites is a literal
    "pair-011-80": ("pair-011", 80, "tanh"),          # 16 lanes, U = 5
    "pair-010-200": ("pair-010", 200, "tanh"),        # 32 lanes, U = 7, ragged (6 x 32 + 8)
    "pair-0101-128": ("pair-0101", 128, "tanh"),      # four sites, two networks
    "pair-0101-512": ("pair-0101", 512, "tanh"),      # ... on the widest layout
    "heat-theta-128": ("heat-theta", 128, "tanh"),    # the diffusivity is trainable (PW::NT = 1)
    "heat-nd-96-gelu": ("heat-nd", 96, "gelu"),       # sigma(0) = 0 but sigma'(0) != 0 in the padding units' rows
    "heat-dn-200-sigmoid": ("heat-dn", 200, "sigmoid"),   # sigma(0) != 0 in the padding units
}
NAMES = list(CASES)
#: cases that also run at 4 097 points (one per site count) and at the first size past one round of the capped grid
MORE_BLOCKS = ["heat-nd-65", "heat-nn-129", "pair-0101-128"]
TILE_LOOP = ["heat-dn-128", "bvp-nn-512"]
#: the goldens the unmodified reference produced (tests/golden/make_wide_site_golden.py): name -> case
GOLDEN = {"ws1": "heat-nn-128", "ws2": "pair-0101-128"}
#: (the golden of heat with two Neumann ends on 128 units is a case of its own, not in the size matrix; scripts/wide_site_timing.py
#: times it and its 512-unit twin, the README's showcase width)
GOLDEN_CASES = {"heat-nn-128": ("heat-nn", 128, "tanh"), "pair-0101-128": CASES["pair-0101-128"], "heat-nn-512": ("heat-nn", 512, "tanh")}
#: training grid of the goldens: 16 x 16 points of the heat cases' domain, 256 points of the interval
GOLDEN_POINTS = 256


def _case(name):
    return CASES[name] if name in CASES else GOLDEN_CASES[name]


def base(name):
    return _case(name)[0]


def width(name):
    return _case(name)[1]


def sites(name):
    """The site map: network of every evaluation site."""
    return SP.CASES[base(name)][1]


def n_nets(name):
    return SP.n_nets(base(name))


def n_inputs(name):
    return SP.n_inputs(base(name))


def n_streams(name):
    """Stream rows of every site after the stream sets were unified: value and first derivatives; u_xx of the interior site,
    and for the heat cases u_xt as well (the boundary sites' slope enters the equation through its time derivative)."""
    return 5 if n_inputs(name) == 2 else 3


def unit_lanes(name):
    w = width(name)
    return 64 if w > 256 else (32 if w > 128 else 16)


def keep_all(name):
    """csrc/ndq_wide.h WideMulti::KEEP_ALL restated: do the activation states of all S sites of a tile (16 points x W padded
    units, two values each, over 64 lanes) fit 128 registers?"""
    ul = unit_lanes(name)
    u, rounds = -(-width(name) // ul), 16 // (64 // ul)
    return len(sites(name)) * rounds * u * 2 <= 128


def make(name):
    """(nets, conditions, equations, n_coords) of the product; draws the networks from torch's current RNG state."""
    from neurodiffeq_amd.networks import FCNN, SinActv
    b, w, act = _case(name)
    _, conds, eqs, nc = SP.make(b)          # (its narrow networks are dropped: conditions and equations are what is shared)
    actv = {"tanh": torch.nn.Tanh, "sin": SinActv, "sigmoid": torch.nn.Sigmoid, "gelu": torch.nn.GELU}[act]
    nets = [FCNN(nc, 1, hidden_units=(w,), actv=actv) for _ in range(n_nets(name))]
    return nets, conds, eqs, nc


def make_oracle(name, dtype=torch.float64):
    """(nets, enforcers, equations) of the fp64 autograd oracle: same shapes, parameters to be set with ``R.set_flat``."""
    from oracle import autograd_ref as R
    b, w, act = _case(name)
    _, enf, eqs = SP.make_oracle(b, dtype)
    nets = [R.make_fcnn(n_inputs(name), 1, (w,), act, dtype) for _ in range(n_nets(name))]
    return nets, enf, eqs


def batch(name, n, seed):
    return SP.batch(base(name), n, seed)


def trace(name, f64=False):
    """(program, descs) of the case as the engine traces it (no GPU)."""
    from neurodiffeq_amd import engine
    torch.manual_seed(0)
    nets, conds, eqs, nc = make(name)
    return engine.trace_system(nets, conds, eqs, nc, f64=f64)


def boundary_literals(name):
    """What the module's traits must say: per site, {input position: boundary value}.  Sites follow the networks in the order
    the conditions ask for them, x_min before x_max, condition by condition; the space coordinate is input 0 of every case."""
    out = [{} for _ in range(n_nets(name))]
    for ends in SP.ENDS[base(name)]:
        out += [{0: xb} for e, xb in zip(ends, (SP.X0, SP.X1)) if e == "n"]
    assert len(out) == len(sites(name))
    return out


def make_solver(name, **kw):
    """The product's solver of a golden system, built as tests/golden/make_wide_site_golden.py builds the reference's: one
    generator for both roles, default Adam.  Returns (solver, nets)."""
    from neurodiffeq_amd.generators import Generator1D, Generator2D
    from neurodiffeq_amd.solvers import Solver1D, Solver2D
    nets, conds, eqs, nc = make(name)
    kw.setdefault("n_batches_valid", 0)
    if nc == 1:
        gen = Generator1D(GOLDEN_POINTS, SP.X0, SP.X1, "equally-spaced-noisy")
        s = Solver1D(eqs, conds, t_min=SP.X0, t_max=SP.X1, nets=nets, train_generator=gen, valid_generator=gen, **kw)
    else:
        gen = Generator2D((16, 16), (SP.X0, SP.T0), (SP.X1, SP.T0 + 1.0), "equally-spaced-noisy")
        s = Solver2D(eqs, conds, xy_min=(SP.X0, SP.T0), xy_max=(SP.X1, SP.T0 + 1.0), nets=nets, train_generator=gen,
                     valid_generator=gen, **kw)
    return s, nets


# ---- a system of the family that does not fit one workgroup's LDS: three FCNN(3, 1, (512,)) with every second derivative (ten
# stream rows, 42 KiB of unit image per network), one of them anchored to its own values on the plane x = X0 -- four sites (the
# value only: the slope there would meet the equations' second derivatives as a third-order stream, outside the family).  engine.FusedSystem drops its module.
OVER_LDS = "anchored3-512"
OVER_WIDTH, OVER_SITES = 512, [0, 1, 2, 0]


def _over_equations(d):
    def hess(u, x, y, t):
        return (d(u, x, order=2) + 0.5 * d(u, y, order=2) - d(u, t, order=2) + d(d(u, x), y) - 0.3 * d(d(u, x), t)
                + 0.7 * d(d(u, y), t))
    eqs = lambda u, v, w, x, y, t: [hess(u, x, y, t) + v * d(u, x) - w, hess(v, x, y, t) - u * d(v, y) + d(w, t),
                                    hess(w, x, y, t) + u - d(v, t)]
    eqs.theta = []
    return eqs


def make_over():
    """(nets, conditions, equations, n_coords) of the product for the over-budget system."""
    from neurodiffeq_amd import conditions as C, diff
    from neurodiffeq_amd.networks import FCNN

    class Anchored(C.BaseCondition):
        """u - u(X0, y, t) + y t: zero plus data on the plane x = X0, through the network's own value there"""

        def enforce(self, net, x, y, t):
            u = C._raw_output(net, (x, y, t), self.ith_unit)
            u0 = C._raw_output(net, (C._boundary_column(x, SP.X0), y, t), self.ith_unit)
            return u - u0 + y * t

    nets = [FCNN(3, 1, hidden_units=(OVER_WIDTH,)) for _ in range(3)]
    return nets, [Anchored(), C.NoCondition(), C.NoCondition()], _over_equations(diff), 3


def make_over_oracle(dtype=torch.float64):
    from oracle import autograd_ref as R

    def anchored(net, x, y, t):
        return net(torch.cat([x, y, t], dim=1)) - net(torch.cat([torch.full_like(x, SP.X0), y, t], dim=1)) + y * t

    plain = lambda net, x, y, t: net(torch.cat([x, y, t], dim=1))
    nets = [R.make_fcnn(3, 1, (OVER_WIDTH,), "tanh", dtype) for _ in range(3)]
    return nets, [anchored, plain, plain], _over_equations(R.ref_diff)


def over_batch(n, seed):
    g = torch.Generator().manual_seed(seed)
    return [SP.X0 + (SP.X1 - SP.X0) * torch.rand(n, generator=g, dtype=torch.float32) for _ in range(3)]
