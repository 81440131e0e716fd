"""Goldens of the wide evaluation-site closure from the UNMODIFIED reference: ws1 (heat equation with two Neumann ends, one
FCNN(2, 1, (128,)): three evaluation sites) and ws2 (a pair of two-point problems with one Neumann end each, two
FCNN(1, 1, (128,)): four sites), 256 points each.  Run where the reference is installed, next to make_golden.py, whose recipe
this reuses unchanged (one closure in fp64 / fp32 on the reference generator's draw, then a 3-epoch Adam trajectory of the
reference solver): the two systems are registered as configs of that script and written by its ``make``.  Equations, domains
and boundary data come from tests/site_problems.py through tests/wide_site_problems.py, instantiated with the reference's
``diff``, networks, conditions and generators."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (puts the reference on sys.path and imports it)

import importlib.util  # noqa: E402


def _by_file(name):
    """tests/<name>.py of this repository as module ``tests.<name>`` (the reference ships a ``tests`` package of its own, which
    is the one on sys.path here)."""
    spec = importlib.util.spec_from_file_location(f"tests.{name}", os.path.join(os.path.dirname(HERE), f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[f"tests.{name}"] = mod
    spec.loader.exec_module(mod)
    return mod


SP = _by_file("site_problems")
WS = _by_file("wide_site_problems")


def config(name):
    case = WS.GOLDEN[name]
    system, width = WS.base(case), WS.width(case)
    heat = SP.CASES[system][0] == "heat"

    def build():
        nets = [MG.FCNN(WS.n_inputs(case), 1, hidden_units=(width,)) for _ in range(WS.n_nets(case))]
        conds = []
        for ends in SP.ENDS[system]:
            if heat:
                kw = {("x_min_val" if ends[0] == "d" else "x_min_prime"): (SP._left_val if ends[0] == "d" else SP._left_prime),
                      ("x_max_val" if ends[1] == "d" else "x_max_prime"): (SP._right_val if ends[1] == "d" else SP._right_prime)}
                conds.append(MG.IBVP1D(x_min=SP.X0, x_max=SP.X1, t_min=SP.T0, t_min_val=SP._u_init, **kw))
            else:
                conds.append(MG.DoubleEndedBVP1D(SP.X0, SP.X1, **SP._bvp_kwargs(ends)))
        if heat:
            gen = MG.Generator2D((16, 16), (SP.X0, SP.T0), (SP.X1, SP.T0 + 1.0), "equally-spaced-noisy")
            return dict(kind="2d", pde=SP.equations(system, MG.diff), nets=nets, conds=conds, gen=gen)
        gen = MG.Generator1D(WS.GOLDEN_POINTS, SP.X0, SP.X1, "equally-spaced-noisy")
        return dict(kind="1d", pde=SP.equations(system, MG.diff), nets=nets, conds=conds, gen=gen, t=(SP.X0, SP.X1))
    return build


if __name__ == "__main__":
    for name in WS.GOLDEN:
        MG.CONFIGS[name] = config(name)
        MG.make(name)
