"""TEST INFRASTRUCTURE ONLY -- the two small bundle problems the GPU solver tests of tests/test_sampler_table.py train on
table-drawn GeneratorND batches; the build compiles their kernels (__graft_entry__.build)."""


def bundle_problem(axes):
    """u' = -lam u, u(0) = 1 with ``axes`` = 2 inputs (t, lam), or -- ``axes`` = 4 -- u' = -a u + b c with inputs (t, a, b, c):
    (nets, conditions, ode of the solver, residuals over every coordinate, generator, eq_param_index).  Build the networks
    under the seed the caller wants."""
    from neurodiffeq_amd import diff
    from neurodiffeq_amd.conditions import BundleIVP
    from neurodiffeq_amd.generators import GeneratorND
    from neurodiffeq_amd.networks import FCNN
    nets = [FCNN(axes, 1, hidden_units=(32, 32))]
    conds = [BundleIVP(t_0=0.0, u_0=1.0)]
    if axes == 2:
        ode = lambda u, t, lam: [diff(u, t) + lam * u]
        gen = GeneratorND(grid=(16, 8), r_min=(0.0, 0.1), r_max=(1.0, 2.0), methods=("equally-spaced", "log-spaced"))
    else:
        ode = lambda u, t, a, b, c: [diff(u, t) + a * u - b * c]
        gen = GeneratorND(grid=(6, 4, 3, 2), r_min=(0.0, 0.5, 0.1, -1.0), r_max=(1.0, 2.0, 1.0, 1.0),
                          methods=("equally-spaced", "log-spaced", "chebyshev2", "equally-spaced"))
    return dict(nets=nets, conds=conds, ode=ode, pde=lambda u, *coords: ode(u, *coords), gen=gen,
                eq_param_index=tuple(range(axes - 1)))
