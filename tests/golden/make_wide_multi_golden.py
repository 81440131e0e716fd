"""Goldens of the multi-network wide closure from the UNMODIFIED reference: wm1 (Lotka-Volterra, two FCNN(1, 1, (128,))) and
wm2 (three coupled fields, three FCNN(2, 1, (128,))), 256 points each.  Run where the reference is installed, next to
make_golden.py, whose recipe this reuses unchanged (one closure in fp64 / fp32 on the reference generator's draw, then a
3-epoch Adam trajectory of the reference solver): the two systems are registered as configs of that script and written by
its ``make``.  The equations and domains come from tests/wide_multi_problems.py, instantiated with the reference's ``diff``,
networks, conditions and generators."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (puts the reference on sys.path and imports it)

import importlib.util  # noqa: E402

# (by file: the reference ships a ``tests`` package of its own, which is the one on sys.path here)
_spec = importlib.util.spec_from_file_location("wide_multi_problems", os.path.join(os.path.dirname(HERE), "wide_multi_problems.py"))
WM = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(WM)


def config(name):
    system, width = WM.GOLDEN[name]
    kind, K, d_in = WM.SYSTEMS[system][:3]

    def build():
        nets = [MG.FCNN(d_in, 1, hidden_units=(width,)) for _ in range(K)]
        if system == "lv":
            conds = [MG.IVP(WM.T_MIN, WM.LV_X0), MG.IVP(WM.T_MIN, WM.LV_Y0)]
        else:
            zero = lambda s: 0 * s
            conds = [MG.DirichletBVP2D(x_min=0, x_min_val=WM._edge(k), x_max=1, x_max_val=zero, y_min=0, y_min_val=zero,
                                       y_max=1, y_max_val=zero) for k in range(K)]
        gen = WM.generator(system, MG.Generator1D, MG.Generator2D)
        cfg = dict(kind="1d" if d_in == 1 else "2d", pde=WM.equations(system, MG.diff), nets=nets, conds=conds, gen=gen)
        if d_in == 1:
            cfg["t"] = (WM.T_MIN, WM.T_MAX)
        return cfg
    return build


if __name__ == "__main__":
    for name in WM.GOLDEN:
        MG.CONFIGS[name] = config(name)
        MG.make(name)
