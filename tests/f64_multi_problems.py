"""Systems of 2 .. 4 narrow networks trained in float64 -- what the multi-network closure kernel compiled in double serves
(csrc/ndq_mlp.h: fused_multi_closure_kernel under NDQ_F64; codegen.can_fuse_multi_f64).  Shared by
tests/test_f64_multi_closure.py, tests/test_gpu_f64_multi_closure.py, scripts/f64_multi_timing.py and the build step that
compiles these systems' modules ahead of the GPU tests."""
import torch

#: the systems the GPU tests launch: name -> what it is the first to run
#:   c1      tests/configs.py: Lotka-Volterra on two sin 32 x 32 networks, d = 1, first-order streams (reference golden)
#:   lv_tanh the same equations on two tanh 32 x 32 networks
#:   mix32   tests/wide_multi_problems.py "mix" at ONE hidden layer of 32 units: d = 2, all three second-order streams
#:   uvp16   tests/wide_multi_problems.py "uvp" at 16 units: K = 3, d = 2, the Laplacian stream, one unit block
GPU_NAMES = ["c1", "lv_tanh", "mix32", "uvp16"]
#: K = 4 at 32 x 32 (one tile slot per workgroup): 145 664 B of LDS in double -- whether a module fits the 160 KiB of one
#: workgroup is what the engine's gate decides, and the tests hold the gate to the module's own figure
OVER_NAME = "four32"
NAMES = GPU_NAMES + [OVER_NAME]


def make(name):
    """(nets, conditions, equations, n_coords, compute_func_val) of the product in double; draws the networks from torch's
    current RNG state."""
    from neurodiffeq_amd import diff
    from neurodiffeq_amd.conditions import IVP
    from neurodiffeq_amd.networks import FCNN
    from tests import configs, wide_multi_problems as wm
    cfv = None
    if name == "c1":
        cfg = configs.make("c1", 64)
        nets, conds, eqs, d, cfv = cfg["nets"], cfg["conds"], configs.fused_equations(cfg), configs.n_coords(cfg), configs.func_val(cfg)
    elif name == "lv_tanh":
        nets = [FCNN(1, 1, hidden_units=(32, 32)) for _ in range(2)]
        conds = [IVP(0.0, 1.5), IVP(0.0, 1.0)]
        eqs, d = (lambda u, v, t: [diff(u, t) - (u - u * v), diff(v, t) - (u * v - v)]), 1
    elif name == "mix32":
        nets, conds, eqs, d = wm.make("mix", 32, "tanh")
    elif name == "uvp16":
        nets, conds, eqs, d = wm.make("uvp", 16)
    elif name == "four32":
        nets = [FCNN(1, 1, hidden_units=(32, 32)) for _ in range(4)]
        conds = [IVP(0.0, 1.0 + 0.5 * k) for k in range(4)]
        eqs, d = wm.equations("four", diff), 1
    else:
        raise KeyError(name)
    for net in nets:
        net.double()
    return nets, conds, eqs, d, cfv


def batch(name, n, seed):
    """``n`` points of the unit interval / square as a list of fp64 columns, from a generator of its own."""
    g = torch.Generator().manual_seed(seed)
    d = 2 if name in ("mix32", "uvp16") else 1
    return [torch.rand(n, generator=g, dtype=torch.float64) for _ in range(d)]
