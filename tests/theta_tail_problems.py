"""Inverse problems of tests/test_gpu_theta_tail.py that no other problem module has, and the list ``build()`` compiles for it:
a system of two narrow networks with trainable rate constants, and an equation that reads a RAMPED outside number (a frozen
kernel argument after one rebuild) next to a trainable coefficient."""
import torch

RAMP = (0.05, 0.035, 0.0245, 0.01715)        # the outside number before every epoch of the mixed test


def narrow_pair():
    """(nets, conditions, equations, n_coords, scalars): Lotka-Volterra on two FCNN(1, 1, (32, 32)) with both rate constants
    trainable.  Draws the networks from torch's current RNG state."""
    from neurodiffeq_amd import diff
    from neurodiffeq_amd.conditions import IVP
    from neurodiffeq_amd.networks import FCNN
    nets = [FCNN(1, 1, hidden_units=(32, 32)) for _ in range(2)]
    a, b = torch.nn.Parameter(torch.tensor(1.5)), torch.nn.Parameter(torch.tensor(3.0))
    eqs = lambda x, y, t: [diff(x, t) - (a * x - x * y), diff(y, t) - (x * y - b * y)]
    return nets, [IVP(0.0, 1.5), IVP(0.0, 1.0)], eqs, 1, [a, b]


def ramped(state=None):
    """(nets, conditions, equations, n_coords, scalars, state): u' + nu u^2 - k sin t with ``state['nu']`` an outside Python
    number the caller moves between epochs and ``k`` a trainable coefficient."""
    from neurodiffeq_amd import diff
    from neurodiffeq_amd.conditions import IVP
    from neurodiffeq_amd.networks import FCNN
    state = {"nu": RAMP[0]} if state is None else state
    k = torch.nn.Parameter(torch.tensor(2.0))
    eqs = lambda u, t: [diff(u, t) + state["nu"] * u ** 2 - k * torch.sin(t)]
    return [FCNN(1, 1, hidden_units=(32, 32))], [IVP(0.0, 1.5)], eqs, 1, [k], state


def build_programs():
    """[(name, program, descs)] of every generated module the GPU tests of this feature use beyond the ones other problem
    modules list: traced here, compiled by ``build()``.  No GPU needed."""
    from neurodiffeq_amd.engine import trace_system
    out = []
    torch.manual_seed(0)
    nets, conds, eqs, nc, _ = narrow_pair()
    out.append(("theta-tail/narrow-pair",) + trace_system(nets, conds, eqs, nc))
    torch.manual_seed(0)
    nets, conds, eqs, nc, _, state = ramped()
    lit = trace_system(nets, conds, eqs, nc)
    out.append(("theta-tail/ramped-literal",) + lit)
    state["nu"] = RAMP[1]                               # the first move: the re-trace names the position, the rebuild freezes it
    assert not lit[0].eq_probe()
    vol = lit[0].suggest_volatile()
    out.append(("theta-tail/ramped-frozen",) + trace_system(nets, conds, eqs, nc, volatile=vol))
    return out
