"""Systems of 2 .. 4 one-hidden-layer networks wider than 64 units -- what the "wide_multi" single-launch closure serves
(csrc/ndq_wide.h: wide_multi_closure_kernel) -- stated once for the product (neurodiffeq_amd) and once for the fp64 autograd
oracle (oracle/autograd_ref.py), from the same equations.  Shared by tests/test_wide_multi.py, tests/test_gpu_wide_multi.py,
the golden script next to tests/golden/make_golden.py and the build step that compiles these systems' modules ahead of the
GPU tests."""
import torch

#: name -> (kind, networks, network inputs)
SYSTEMS = {"lv": ("ode", 2, 1), "uvp": ("pde", 3, 2), "four": ("ode", 4, 1)}
#: (system, width) pairs the GPU tests launch: their modules are compiled by the build step
GPU_CASES = [("lv", 80), ("lv", 128), ("uvp", 80), ("uvp", 128)]
#: modules tests/test_wide_multi.py loads without a GPU: the GPU cases' first two, K = 4 at both ends of the width range
CPU_CASES = [("lv", 80), ("uvp", 128), ("four", 72), ("four", 512)]
#: the goldens the unmodified reference produced (tests/golden/make_wide_multi_golden.py): name -> (system, width)
GOLDEN = {"wm1": ("lv", 128), "wm2": ("uvp", 128)}

LV_X0, LV_Y0 = 1.5, 1.0
T_MIN, T_MAX = 0.0, 1.0


def equations(name, d):
    """The residuals of system ``name`` written against a ``diff(u, t, order=1)``: the product's, the oracle's, the reference's."""
    if name == "lv":           # Lotka-Volterra (the reference's README system of ODEs)
        return lambda x, y, t: [d(x, t) - (1.5 * x - x * y), d(y, t) - (x * y - 3.0 * y)]
    if name == "uvp":          # three coupled fields, every one through its Laplacian and first derivatives
        lap = lambda u, x, y: d(u, x, order=2) + d(u, y, order=2)
        return lambda u, v, p, x, y: [lap(u, x, y) + v * d(u, x) - p * d(u, y),
                                      lap(v, x, y) + u * d(v, y) + p * d(v, x) - u,
                                      lap(p, x, y) - d(u, x) * d(v, y) + d(p, x) + d(p, y)]
    if name == "four":         # a ring of four first-order equations
        return lambda a, b, c, e, t: [d(a, t) + b, d(b, t) - a * c, d(c, t) + e * b, d(e, t) - a]
    raise KeyError(name)


def _edge(k):
    return lambda s: torch.sin(3.14159 * s) * (0.5 + 0.25 * k)


def make(name, width):
    """(nets, conditions, equations, n_coords) of the product; draws the networks from torch's current RNG state."""
    from neurodiffeq_amd import diff
    from neurodiffeq_amd.conditions import IVP, DirichletBVP2D
    from neurodiffeq_amd.networks import FCNN
    kind, K, d_in = SYSTEMS[name]
    nets = [FCNN(d_in, 1, hidden_units=(width,)) for _ in range(K)]
    if name == "lv":
        conds = [IVP(T_MIN, LV_X0), IVP(T_MIN, LV_Y0)]
    elif name == "four":
        conds = [IVP(T_MIN, 1.0 + 0.5 * k) for k in range(K)]
    else:
        zero = lambda s: 0 * s
        conds = [DirichletBVP2D(0, _edge(k), 1, zero, 0, zero, 1, zero) for k in range(K)]
    return nets, conds, equations(name, diff), d_in


def make_single(name, width):
    """ONE network of system ``name``'s shape and stream set (the "wide" closure of the same WideCfg): first-order decay for
    the ODE systems, a Laplacian with first derivatives for the PDE system."""
    from neurodiffeq_amd import diff
    from neurodiffeq_amd.conditions import IVP, DirichletBVP2D
    from neurodiffeq_amd.networks import FCNN
    d_in = SYSTEMS[name][2]
    net = FCNN(d_in, 1, hidden_units=(width,))
    if d_in == 1:
        return [net], [IVP(T_MIN, 1.0)], (lambda u, t: [diff(u, t) + u]), 1
    zero = lambda s: 0 * s
    eq = lambda u, x, y: [diff(u, x, order=2) + diff(u, y, order=2) + u * diff(u, x) - diff(u, y)]
    return [net], [DirichletBVP2D(0, _edge(0), 1, zero, 0, zero, 1, zero)], eq, 2


def make_oracle(name, width, dtype=torch.float64):
    """(nets, enforcers, equations) of the fp64 autograd oracle: same shapes, parameters to be set with ``R.set_flat``."""
    from oracle import autograd_ref as R
    kind, K, d_in = SYSTEMS[name]
    nets = [R.make_fcnn(d_in, 1, (width,), "tanh", dtype) for _ in range(K)]
    if name == "lv":
        enf = [R.ivp(T_MIN, LV_X0), R.ivp(T_MIN, LV_Y0)]
    elif name == "four":
        enf = [R.ivp(T_MIN, 1.0 + 0.5 * k) for k in range(K)]
    else:
        zero = lambda s: 0 * s
        enf = [R.dirichlet_bvp2d(0, _edge(k), 1, zero, 0, zero, 1, zero) for k in range(K)]
    return nets, enf, equations(name, R.ref_diff)


def batch(name, n, seed):
    """``n`` points of the unit interval / square as a list of fp32 columns, from a generator of its own."""
    g = torch.Generator().manual_seed(seed)
    return [torch.rand(n, generator=g, dtype=torch.float32) for _ in range(SYSTEMS[name][2])]


def generator(name, make_1d, make_2d):
    """The 256-point training generator of the golden systems from a Generator1D / Generator2D class (the product's here,
    the reference's in tests/golden/make_wide_multi_golden.py)."""
    if SYSTEMS[name][2] == 1:
        return make_1d(256, T_MIN, T_MAX, "equally-spaced-noisy")
    return make_2d((16, 16), (0, 0), (1, 1), "equally-spaced-noisy")


def make_solver(name, width, **kw):
    """The product's solver of a golden system, built as tests/golden/make_golden.py builds the reference's: one generator for
    both roles, default Adam.  Returns (solver, nets, generator)."""
    from neurodiffeq_amd.generators import Generator1D, Generator2D
    from neurodiffeq_amd.solvers import Solver1D, Solver2D
    nets, conds, eqs, d_in = make(name, width)
    gen = generator(name, Generator1D, Generator2D)
    kw.setdefault("n_batches_valid", 0)
    if d_in == 1:
        s = Solver1D(eqs, conds, t_min=T_MIN, t_max=T_MAX, nets=nets, train_generator=gen, valid_generator=gen, **kw)
    else:
        s = Solver2D(eqs, conds, xy_min=(0, 0), xy_max=(1, 1), nets=nets, train_generator=gen, valid_generator=gen, **kw)
    return s, nets, gen
