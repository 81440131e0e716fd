"""TEST INFRASTRUCTURE ONLY -- the generators with per-point stages (TransformGenerator / FilterGenerator above a plan) that the GPU
part of tests/test_sampler_map.py draws on the device, in one place: ``__graft_entry__.build`` compiles their generated modules
(codegen.SamplerMapProgram) ahead of the tests from the same definitions.  Few distinct callables on purpose: each distinct traced
DAG is one hipcc run."""
import numpy as np
import torch

from neurodiffeq_amd.generators import (BatchGenerator, FilterGenerator, Generator1D, Generator2D, GeneratorND, ResampleGenerator,
                                        TransformGenerator)

Transform, Filter, Resample, Batch = TransformGenerator, FilterGenerator, ResampleGenerator, BatchGenerator
TWO_PI = 6.2831853


def polar(r, th):
    return r * torch.cos(TWO_PI * th), r * torch.sin(TWO_PI * th)


def one_to_three(t):
    return t, t * t, 2.0 * t + 1.0


def three_to_two(x, y, z):
    return x + y, y * z - x


def affine2(x, y):
    return 2.0 * x - 1.0, y + x


def shift(x, y):
    return x - 0.25, y / 3.0


def above_half(xs):
    return xs[0] > 0.5


class Disk:
    """x^2 + y^2 < radius^2 with the radius read from the instance at every call: state a callback may move."""

    def __init__(self, radius):
        self.radius = radius

    def __call__(self, xs):
        return xs[0] * xs[0] + xs[1] * xs[1] < self.radius * self.radius


def disk_small(xs):
    return xs[0] * xs[0] + xs[1] * xs[1] < 0.25


def centred(x, y):
    return 2.0 * x - 1.0, 2.0 * y - 1.0


def rotate(x, y):
    return x + y, x - y


def mesh_64x5():
    return Generator1D(64, method="equally-spaced") ^ Generator1D(5, method="equally-spaced")


def nd3():
    return GeneratorND((4, 3, 5), (0.0,) * 3, (1.0,) * 3, ("equally-spaced",) * 3, noisy=False)


def square(grid=(32, 32)):
    return Generator2D(grid, (-1.0, -1.0), (1.0, 1.0))


#: name -> () -> (generator with stages, the same tree without its stages, [stage callables inner to outer as ('map' | 'filter', f)])
MAP_CASES = {
    "polar-16x16-noisy": lambda: _case(Generator2D((16, 16)), lambda g: Transform(g, transform=polar), [("map", polar)]),
    "1-to-3-rows-257": lambda: _case(Generator1D(257, method="equally-spaced"), lambda g: Transform(g, transform=one_to_three),
                                     [("map", one_to_three)]),
    "3-to-2-rows-nd": lambda: _case(nd3(), lambda g: Transform(g, transform=three_to_two), [("map", three_to_two)]),
    "above-batch-resample": lambda: _case(Batch(Resample(mesh_64x5()), 48), lambda g: Transform(g, transform=affine2), [("map", affine2)]),
    "between-batch-and-resample": lambda: _between(),
    "nested-transforms": lambda: _case(mesh_64x5(), lambda g: Transform(Transform(g, transform=affine2), transforms=[None, torch.abs]),
                                       [("map", affine2), ("map", lambda x, y: (x, torch.abs(y)))]),
}


def _case(base, wrap, stages):
    return wrap(base), base, stages


def _between():
    rs = Resample(mesh_64x5())
    return Batch(Transform(rs, transform=affine2), 48), Batch(rs, 48), [("map", affine2)]


FILTER_SIZES = (1, 255, 256, 257, 1000, 70000)


def filter_1d(kind, n):
    """'all' / 'none' / 'grid': ONE callable (above_half) over three intervals -- one generated module."""
    base = {"all": lambda: Generator1D(n, 0.6, 1.0), "none": lambda: Generator1D(n, 0.0, 0.4),
            "grid": lambda: Generator1D(n, 0.0, 1.0, method="equally-spaced")}[kind]()
    return Filter(base, above_half), base, [("filter", above_half)]


FILTER_CASES = {
    "disk-32x32-jittered": lambda: _case(square(), lambda g: Filter(g, Disk(0.9)), [("filter", Disk(0.9))]),
    "disk-264x266-jittered": lambda: _case(square((264, 266)), lambda g: Filter(g, Disk(0.9)), [("filter", Disk(0.9))]),
    "disk-above-batch": lambda: _case(Batch(Resample(square((20, 20))), 300), lambda g: Filter(g, Disk(0.9)), [("filter", Disk(0.9))]),
    "transform-filter-transform": lambda: _case(
        Generator2D((20, 20)), lambda g: Transform(Filter(Transform(g, transform=centred), disk_small), transform=rotate),
        [("map", centred), ("filter", disk_small), ("map", rotate)]),
}


def all_staged_generators():
    """Every distinct (plan rows, stages) the GPU tests draw: what ``__graft_entry__.build`` compiles ahead."""
    torch.manual_seed(0)
    out = [make()[0] for make in MAP_CASES.values()] + [make()[0] for make in FILTER_CASES.values()]
    out.append(filter_1d("grid", 8)[0])
    out.append(Filter(square(), Disk(0.5)))                  # the second radius of the live-change test
    out.append(Filter(square(), disk_small))
    return out


def apply_stages(rows, stages):
    """The stage callables themselves, in torch fp32 on the CPU: rows [d][n] -> (rows [d_out][kept], mask [n] of the points kept)."""
    cols = [torch.from_numpy(np.ascontiguousarray(r)) for r in rows]
    keep = torch.ones(len(cols[0]), dtype=torch.bool)
    for kind, f in stages:
        if kind == "filter":
            keep &= f(cols)
        else:
            out = f(*cols)
            cols = [out] if isinstance(out, torch.Tensor) else list(out)
    return np.stack([c.numpy() for c in cols])[:, keep.numpy()], keep.numpy()
