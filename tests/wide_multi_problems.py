"""Systems of 2 .. 4 one-hidden-layer networks wider than 64 units -- what the "wide_multi" single-launch closure serves
(csrc/ndq_wide.h: wide_multi_closure_kernel) -- stated once for the product (neurodiffeq_amd) and once for the fp64 autograd
oracle (oracle/autograd_ref.py), from the same equations.  Shared by tests/test_wide_multi.py, tests/test_gpu_wide_multi.py,
the golden script next to tests/golden/make_golden.py and the build step that compiles these systems' modules ahead of the
GPU tests."""
import torch

#: name -> (kind, networks, network inputs, activation -- None: the one the case names)
SYSTEMS = {"lv": ("ode", 2, 1, "tanh"), "uvp": ("pde", 3, 2, "tanh"), "four": ("ode", 4, 1, "tanh"),
           "ode3": ("ode", 2, 1, "sin"), "mix": ("pde", 2, 2, None), "mix4": ("pde", 4, 2, None), "lvtheta": ("ode", 2, 1, "tanh")}
#: the cases the GPU tests launch, (system, width) or (system, width, activation): their modules are compiled by the build step.
#: Each is the first to run something of csrc/ndq_wide.h's WideCfg / WideMulti (UL = unit lanes, U = units per lane):
GPU_CASES = [
    ("lv", 65),                  # minimum width: the last unit row holds one unit; every network's states kept (KEEP_ALL)
    ("lv", 80), ("lv", 128),     # 16 unit lanes (both goldens' width: 128)
    ("lv", 200),                 # 32 unit lanes, ragged (6 x 32 + 8); states recomputed by the second forward pass
    ("lv", 300),                 # 64 unit lanes, ragged (4 x 64 + 44)
    ("uvp", 80), ("uvp", 128),
    ("uvp", 200), ("uvp", 512),  # K = 3: the Laplacian stream on 32 / 64 unit lanes
    ("four", 72), ("four", 512), # K = 4 on the narrowest and the widest layout
    ("ode3", 80), ("ode3", 200), # third-order streams, sin: with kept states and with the second forward pass
    ("mix", 200, "sigmoid"),     # mixed second derivatives (three second-order streams); sigma(0) != 0 in the padding units
    ("mix", 129, "swish"),       # 4 x 32 + 1
    ("mix", 96, "gelu"),
    ("lvtheta", 128),            # trainable scalars in the equations (PW::NT = 2)
    ("mix4", 512, "tanh"),       # over the LDS budget of one workgroup: the engine keeps the pipeline
]
#: the cases whose closure module does not fit 160 KiB of LDS (engine.FusedSystem drops it)
OVER_LDS = [("mix4", 512, "tanh")]
#: modules tests/test_wide_multi.py loads without a GPU: the GPU cases' first two, K = 4 at both ends of the width range
CPU_CASES = [("lv", 80), ("uvp", 128), ("four", 72), ("four", 512)]
#: the goldens the unmodified reference produced (tests/golden/make_wide_multi_golden.py): name -> (system, width)
GOLDEN = {"wm1": ("lv", 128), "wm2": ("uvp", 128)}

LV_X0, LV_Y0 = 1.5, 1.0
LVTHETA = (1.5, 3.0)             # lvtheta: the rate constants of a x - x y and x y - b y, trainable
T_MIN, T_MAX = 0.0, 1.0


def case_id(case):
    return "-".join(map(str, case))


def activation(case):
    """Name of the hidden layer's activation (oracle.autograd_ref.ACTIVATIONS' names)."""
    return case[2] if len(case) > 2 else SYSTEMS[case[0]][3]


def n_streams(name):
    """Stream rows per network (value, first derivatives, second / third order) the system traces to."""
    return {"lv": 2, "four": 2, "lvtheta": 2, "uvp": 4, "ode3": 4, "mix": 6, "mix4": 6}[name]


def equations(name, d, theta=None):
    """The residuals of system ``name`` written against a ``diff(u, t, order=1)``: the product's, the oracle's, the reference's.
    ``theta``: the trainable scalars of the systems that have some (the returned callable carries them as ``.theta``)."""
    eqs = _equations(name, d, theta)
    eqs.theta = list(theta or ())
    return eqs


def _equations(name, d, theta):
    if name == "lvtheta":      # Lotka-Volterra with its two rate constants trainable (an inverse problem's equations)
        a, b = theta
        return lambda x, y, t: [d(x, t) - (a * x - x * y), d(y, t) - (x * y - b * y)]
    if name == "ode3":         # two third-order equations, each through the other's second and first derivative
        return lambda x, y, t: [d(x, t, order=3) + d(y, t, order=2) + x * d(y, t),
                                d(y, t, order=3) - d(x, t, order=2) + y * d(x, t)]
    if name == "mix":          # every second derivative of both fields, the mixed one included
        dxy = lambda u, x, y: d(d(u, x), y)
        return lambda u, v, x, y: [d(u, x, order=2) + dxy(u, x, y) - d(v, y, order=2) + u * d(v, x) + d(u, y),
                                   d(v, x, order=2) + dxy(v, x, y) + d(u, y, order=2) - v * d(u, x) + d(v, y)]
    if name == "mix4":         # the same construction as a ring of four: field k coupled to field k + 1
        dxy = lambda u, x, y: d(d(u, x), y)

        def ring(*a):
            f, (x, y) = a[:4], a[4:]
            out = []
            for k in range(4):
                u, v, s = f[k], f[(k + 1) % 4], (1.0 if k % 2 == 0 else -1.0)
                out.append(d(u, x, order=2) + dxy(u, x, y) - s * d(v, y, order=2) + s * u * d(v, x) + d(u, y))
            return out
        return ring
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


def _theta(name, dtype):
    """The trainable scalars of the system's equations at their initial values (``lvtheta``: the two rate constants)."""
    if name != "lvtheta":
        return None
    return [torch.nn.Parameter(torch.tensor(v, dtype=dtype)) for v in LVTHETA]


def make(name, width, act=None):
    """(nets, conditions, equations, n_coords) of the product; draws the networks from torch's current RNG state."""
    from neurodiffeq_amd import diff
    from neurodiffeq_amd.conditions import IVP, DirichletBVP2D
    from neurodiffeq_amd.networks import FCNN, SinActv, Swish
    kind, K, d_in, sys_act = SYSTEMS[name]
    actv = {"tanh": torch.nn.Tanh, "sin": SinActv, "sigmoid": torch.nn.Sigmoid, "swish": Swish, "gelu": torch.nn.GELU}[act or sys_act]
    nets = [FCNN(d_in, 1, hidden_units=(width,), actv=actv) for _ in range(K)]
    if name in ("lv", "lvtheta"):
        conds = [IVP(T_MIN, LV_X0), IVP(T_MIN, LV_Y0)]
    elif name == "ode3":
        conds = [IVP(T_MIN, 1.0), IVP(T_MIN, 0.5)]
    elif name == "four":
        conds = [IVP(T_MIN, 1.0 + 0.5 * k) for k in range(K)]
    else:
        zero = lambda s: 0 * s
        conds = [DirichletBVP2D(0, _edge(k), 1, zero, 0, zero, 1, zero) for k in range(K)]
    return nets, conds, equations(name, diff, _theta(name, torch.float32)), d_in


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


def make_oracle(name, width, act=None, dtype=torch.float64):
    """(nets, enforcers, equations) of the fp64 autograd oracle: same shapes, parameters to be set with ``R.set_flat``; the
    equations' trainable scalars are fp64 parameters of the oracle's own (``equations.theta``)."""
    from oracle import autograd_ref as R
    kind, K, d_in, sys_act = SYSTEMS[name]
    nets = [R.make_fcnn(d_in, 1, (width,), act or sys_act, dtype) for _ in range(K)]
    if name in ("lv", "lvtheta"):
        enf = [R.ivp(T_MIN, LV_X0), R.ivp(T_MIN, LV_Y0)]
    elif name == "ode3":
        enf = [R.ivp(T_MIN, 1.0), R.ivp(T_MIN, 0.5)]
    elif name == "four":
        enf = [R.ivp(T_MIN, 1.0 + 0.5 * k) for k in range(K)]
    else:
        zero = lambda s: 0 * s
        enf = [R.dirichlet_bvp2d(0, _edge(k), 1, zero, 0, zero, 1, zero) for k in range(K)]
    return nets, enf, equations(name, R.ref_diff, _theta(name, dtype))


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
