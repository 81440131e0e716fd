"""Problems of tests/test_gpu_f64_tail.py that no other module describes.  Shared with the build step, which compiles their
modules ahead of the GPU tests."""
import torch

#: the coefficient of ``ramp_system`` before and after the one change the test makes
RAMP_VALUES = (1.0, 0.7)


def ramp_system(state):
    """(nets, conditions, equations, n_coords, compute_func_val) of Lotka-Volterra on two tanh 32 x 32 networks in double with
    the Python float ``state['a']`` inside the equations (the reference re-evaluates them every batch: a callback may change
    it between epochs).  Draws the networks from torch's current RNG state."""
    from neurodiffeq_amd import diff
    from neurodiffeq_amd.conditions import IVP
    from neurodiffeq_amd.networks import FCNN
    nets = [FCNN(1, 1, hidden_units=(32, 32)).double() for _ in range(2)]
    conds = [IVP(0.0, 1.5), IVP(0.0, 1.0)]
    eqs = lambda u, v, t: [diff(u, t) - (state["a"] * u - u * v), diff(v, t) - (u * v - v)]
    return nets, conds, eqs, 1, None


def batch(d, n, seed):
    """``n`` points of the unit interval / square as a list of ``d`` fp64 columns, from a generator of its own."""
    g = torch.Generator().manual_seed(seed)
    return [torch.rand(n, generator=g, dtype=torch.float64) for _ in range(d)]
