"""Collocation-point generators with the reference's names, arguments and draw order
(neurodiffeq/generators.py:107-1064).

Generators are the *input producer* of the hot path, not part of it: the classes with the reference's names always
sample on the host with torch's global CPU generator, in the same call sequence as the reference, so that a given
``torch.manual_seed`` yields bit-identical points (the north-star parity contract); the solver uploads each batch to
HBM as one SoA block.  Two additions without a reference counterpart keep the producer off the step's critical path:
:class:`ResidentBatchGenerator` (pre-sampled batches resident in HBM) and :class:`DeviceGenerator` (the same
distributions drawn by a Philox kernel on the MI355X, a fresh batch per epoch with no PCIe hand-off)."""
import ctypes
import os
import warnings
import weakref

import numpy as np
import torch

_CPU = torch.device("cpu")
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None) or (lambda idx: torch.cuda.current_stream(idx).cuda_stream)


def _chebyshev_first(a, b, n):
    nodes = torch.cos(((torch.arange(n, device=_CPU) + 0.5) / n) * np.pi)
    return (((a + b) + (b - a) * nodes) / 2).requires_grad_(True)


def _chebyshev_second(a, b, n):
    nodes = torch.cos(torch.arange(n, device=_CPU) / float(n - 1) * np.pi)
    return (((a + b) + (b - a) * nodes) / 2).requires_grad_(True)


def _chebyshev_second_noisy(a, b, n):
    nodes = torch.cos((torch.arange(n, device=_CPU) + (torch.rand(n, device=_CPU) * 2 - 1)) / float(n - 1) * np.pi)
    return (((a + b) + (b - a) * nodes) / 2).requires_grad_(True)


def _latin_hypercube(a, b, n):
    edges = torch.linspace(a, b, steps=n + 1, device=_CPU)
    pts = torch.rand(n, device=_CPU) * (edges[1] - edges[0])
    pts += edges[:-1]
    pts = pts[torch.randperm(n, device=_CPU)]
    return pts.requires_grad_(True)


def _log_bounds(t_min, t_max, whence):
    if t_min <= 0 or t_max <= 0:
        raise ValueError(f"the interval [{t_min}, {t_max}] cannot be used for log-sampling in {whence}; "
                         f"if you meant [10^{t_min}, 10^{t_max}], pass {10 ** t_min} and {10 ** t_max}")
    return np.log10(t_min), np.log10(t_max)


def _rows_inplace(z, scale, shift):
    """``z * scale + shift`` in place (two roundings, like ``mul_`` then ``add_``) with broadcasting, on numpy views: the
    same IEEE operations as torch's, minus torch's intra-op thread pool -- a block of a few hundred batches is above
    its parallel grain size, and waking that pool costs more than the arithmetic (measured 55 ms against 0.2 ms)."""
    zn = z.numpy()
    if scale is not None:
        np.multiply(zn, scale.numpy(), out=zn)
    np.add(zn, shift.numpy(), out=zn)
    return z


#: attributes a generator of the reference reads WHEN IT DRAWS (generators.py:107-416: the getters are lambdas over ``self``), i.e.
#: what a callback can change between epochs with effect -- the grid tensors, the noise widths, the getter itself.  (t_min / t_max /
#: grid are consumed by __init__: changing them later has no effect in the reference either.)
_LIVE = ("getter", "get_r", "examples", "grid_x", "grid_y", "grid_z", "noise_std", "noise_xstd", "noise_ystd", "size", "shape", "method")
#: the same for the generators DeviceGenerator draws from tables (GeneratorND, the node-table laws of Generator1D); a tuple of its
#: own: _LIVE also feeds the bulk-draw stamp of the other generators
_LIVE_TABLE = ("grid_r", "grid_std", "getter", "examples", "noise_std", "size", "method")
#: what a ResampleGenerator / BatchGenerator above a plan reads when it draws (BatchGenerator.cached_xs is host state: the device
#: draw has no cache, its window is a function of the draw number)
_LIVE_INDEX = ("size", "replacement", "generator")
#: ... and a TransformGenerator / FilterGenerator of the root chain (FilterGenerator.size is an OUTPUT of a draw: the kept count)
_LIVE_STAGE = ("trans", "filter_fn", "update_size", "generator")


def live_stamp(gen, names=_LIVE):
    """What ``gen`` would draw from right now, cheaply comparable: (attribute, value) for numbers, (attribute, id, version) for
    tensors / callables.  A shortcut that was derived from the generator's state (one-call bulk draws, a device-side sampler's
    descriptor) is only valid while this stamp is what it was."""
    out = [type(gen).get_examples]
    d = gen.__dict__
    for name in names:
        v = d.get(name)
        if isinstance(v, torch.Tensor):
            out.append((id(v), v._version))
        elif isinstance(v, (list, tuple)):
            out.append(tuple(v))
        else:
            out.append(v)
    return out


def _bulk_validate(gen):
    """First use, or a callback has changed what the generator draws from (noise width, grid tensors, the getter): whatever was
    cached or proven for the old state is void."""
    stamp = live_stamp(gen)
    if gen.__dict__.get("_bulk_stamp") != stamp:
        gen.__dict__.pop("_bulk_rows", None)
        gen._bulk_ok = None
        gen._bulk_stamp = stamp


def _checked_bulk(gen, k, draw):
    """``draw(k)`` -> host tensor [k][d][size] holding what ``k`` consecutive ``gen.get_examples()`` calls would return,
    drawn with ONE call into torch's CPU generator (the multi-epoch fit path of the solvers draws the batches of a whole
    chunk of epochs at once).  torch's ``normal_`` fills blocks of 16 values from 16 uniform draws, so one long call
    reproduces a sequence of short ones exactly when every short one is a whole number of blocks -- but that is a
    property of torch's kernels, not of its API: the first use on a generator proves it (two batches drawn both ways
    from the same RNG state, which is restored) and the generator falls back to one call per batch if it does not hold."""
    _bulk_validate(gen)
    ok = gen.__dict__.get("_bulk_ok")
    if ok is None:
        state = torch.get_rng_state()
        try:
            two = draw(2)
            torch.set_rng_state(state)
            seq = []
            for _ in range(2):
                ex = gen.get_examples()
                ex = [ex] if isinstance(ex, torch.Tensor) else list(ex)
                seq.append(torch.stack([e.detach().reshape(-1) for e in ex]))
            after = torch.get_rng_state()
            torch.set_rng_state(state)
            draw(2)
            ok = bool(torch.equal(two, torch.stack(seq)) and torch.equal(after, torch.get_rng_state()))
        except Exception:       # noqa: BLE001 -- whatever went wrong, the one-call-per-batch path is always right
            ok = False
        torch.set_rng_state(state)
        gen._bulk_ok = ok
    return draw(k) if ok else None


class BaseGenerator:
    def __init__(self):
        self.size = None

    def get_examples(self):
        pass  # pragma: no cover

    def bulk_examples(self, k):
        """``k`` consecutive draws as one host tensor [k][d][size], bit-identical to ``k`` calls of ``get_examples`` and
        leaving torch's RNG in the same state -- or None when this generator has no such shortcut (callers then simply
        call ``get_examples`` ``k`` times)."""
        return None

    @staticmethod
    def check_generator(obj):
        if not isinstance(obj, BaseGenerator):
            raise ValueError(f"{obj} is not a generator")

    def __add__(self, other):
        self.check_generator(other)
        return ConcatGenerator(self, other)

    def __mul__(self, other):
        self.check_generator(other)
        return EnsembleGenerator(self, other)

    def __xor__(self, other):
        self.check_generator(other)
        return MeshGenerator(self, other)

    def _internal_vars(self):
        return dict(size=self.size)

    def __repr__(self):
        d = self._internal_vars()
        return f"{self.__class__.__name__}({', '.join(f'{k}={d[k]!r}' for k in d)})"


class Generator1D(BaseGenerator):
    """1-D points on [t_min, t_max] (generators.py:107-191); ``method`` as in the reference."""

    def __init__(self, size, t_min=0.0, t_max=1.0, method="uniform", noise_std=None, bit_exact_cpu=False):
        super().__init__()
        self.bit_exact_cpu = bool(bit_exact_cpu)      # True: never drawn on the device (see on_default_device)
        self.size, self.t_min, self.t_max, self.method = size, t_min, t_max, method
        self.noise_std = noise_std if noise_std else ((t_max - t_min) / size) / 4.0
        fixed = None
        if method == "uniform":
            self.examples = torch.zeros(size, requires_grad=True, device=_CPU)
            self.getter = lambda: self.examples + torch.rand(size, device=_CPU) * (t_max - t_min) + t_min
        elif method in ("equally-spaced", "equally-spaced-noisy"):
            fixed = torch.linspace(t_min, t_max, size, requires_grad=True, device=_CPU)
        elif method in ("log-spaced", "log-spaced-noisy"):
            lo, hi = _log_bounds(t_min, t_max, self.__class__)
            fixed = torch.logspace(lo, hi, size, requires_grad=True, device=_CPU)
        elif method in ("chebyshev", "chebyshev1"):
            fixed = _chebyshev_first(t_min, t_max, size)
        elif method == "chebyshev2":
            fixed = _chebyshev_second(t_min, t_max, size)
        elif method == "chebyshev2-noisy":
            self.getter = lambda: _chebyshev_second_noisy(t_min, t_max, size)
        elif method == "latin-hypercube":
            self.getter = lambda: _latin_hypercube(t_min, t_max, size)
        else:
            raise ValueError(f"Unknown method: {method}")
        if fixed is not None:
            self.examples = fixed
            if method.endswith("-noisy"):
                self.getter = lambda: torch.normal(mean=self.examples, std=self.noise_std)
            else:
                self.getter = lambda: self.examples

    def get_examples(self):
        return self.getter()

    def bulk_examples(self, k):
        # torch.normal(mean=m, std=s) is normal_(0, s) followed by add_(m): the same two steps over k batches at once
        if self.method in ("equally-spaced-noisy", "log-spaced-noisy") and self.size % 16 == 0:
            mean = self.examples.detach()
            return _checked_bulk(self, k, lambda kk: _rows_inplace(
                torch.empty(kk, 1, self.size, dtype=mean.dtype, device=_CPU).normal_(0, self.noise_std), None, mean))
        return None

    def _internal_vars(self):
        d = super()._internal_vars()
        d.update(t_min=self.t_min, t_max=self.t_max, method=self.method, noise_std=self.noise_std)
        return d


class Generator2D(BaseGenerator):
    """Points on a (possibly noisy) m x n grid over [x0,x1] x [y0,y1] (generators.py:194-314).  For the noisy grid
    the x noise is drawn before the y noise, each with one ``torch.normal`` over the flattened ij-meshgrid."""

    def __init__(self, grid=(10, 10), xy_min=(0.0, 0.0), xy_max=(1.0, 1.0), method="equally-spaced-noisy",
                 xy_noise_std=None, bit_exact_cpu=False):
        super().__init__()
        self.bit_exact_cpu = bool(bit_exact_cpu)
        self.grid, self.size = grid, grid[0] * grid[1]
        self.xy_min, self.xy_max, self.method, self.xy_noise_std = xy_min, xy_max, method, xy_noise_std
        axes = None
        if method in ("equally-spaced", "equally-spaced-noisy"):
            axes = [torch.linspace(xy_min[i], xy_max[i], grid[i], requires_grad=True, device=_CPU) for i in (0, 1)]
        elif method in ("chebyshev", "chebyshev1"):
            axes = [_chebyshev_first(xy_min[i], xy_max[i], grid[i]) for i in (0, 1)]
        elif method == "chebyshev2":
            axes = [_chebyshev_second(xy_min[i], xy_max[i], grid[i]) for i in (0, 1)]
        elif method == "latin-hypercube":
            axes = [_latin_hypercube(xy_min[i], xy_max[i], grid[i]) for i in (0, 1)]
        elif method == "chebyshev2-noisy":
            def draw():
                ax = [_chebyshev_second_noisy(xy_min[i], xy_max[i], grid[i]) for i in (0, 1)]
                gx, gy = torch.meshgrid(ax[0], ax[1], indexing="ij")
                return gx.flatten(), gy.flatten()
            self.getter = draw
        else:
            raise ValueError(f"Unknown method: {method}")
        if axes is not None:
            gx, gy = torch.meshgrid(axes[0], axes[1], indexing="ij")
            self.grid_x, self.grid_y = gx.flatten(), gy.flatten()
            if method == "equally-spaced-noisy":
                if xy_noise_std:
                    self.noise_xstd, self.noise_ystd = xy_noise_std
                else:
                    self.noise_xstd = ((xy_max[0] - xy_min[0]) / grid[0]) / 4.0
                    self.noise_ystd = ((xy_max[1] - xy_min[1]) / grid[1]) / 4.0
                self.getter = lambda: (torch.normal(mean=self.grid_x, std=self.noise_xstd),
                                       torch.normal(mean=self.grid_y, std=self.noise_ystd))
            else:
                self.getter = lambda: (self.grid_x, self.grid_y)

    def get_examples(self):
        return self.getter()

    def bulk_examples(self, k):
        # per batch the x noise is drawn before the y noise: one normal_ over [k][x | y][size] with per-element std
        # (torch.normal(mean=m, std=s) = normal_(0, s) + add_(m), and normal_(0, s) is the standard normal draw times s in
        # one rounding: one standard normal_ over [k][x | y][size], then the scale and the shift per row)
        if self.method == "equally-spaced-noisy" and self.size % 16 == 0:
            # (built from the generator's CURRENT grid tensors and noise widths on every call -- once per chunk of epochs: a copy
            # kept across calls would miss `g.grid_y.data.mul_(2.0)`, which no version counter sees)
            mean = torch.stack([self.grid_x.detach(), self.grid_y.detach()]).unsqueeze(0)
            std = torch.tensor([self.noise_xstd, self.noise_ystd], dtype=mean.dtype, device=_CPU).view(1, 2, 1)
            return _checked_bulk(self, k, lambda kk: _rows_inplace(
                torch.empty(kk, 2, self.size, dtype=mean.dtype, device=_CPU).normal_(), std, mean))
        return None

    def _internal_vars(self):
        d = super()._internal_vars()
        d.update(grid=self.grid, xy_min=self.xy_min, xy_max=self.xy_max, method=self.method,
                 xy_noise_std=self.xy_noise_std)
        return d


class GeneratorSpherical(BaseGenerator):
    """Points (r, theta, phi) with directions uniform-ish on the sphere (generators.py:572-655); same draw order as the
    reference: three ``rand`` for the direction, three ``randint`` signs, then the radius."""

    def __init__(self, size, r_min=0., r_max=1., method="equally-spaced-noisy", bit_exact_cpu=False):
        super().__init__()
        self.bit_exact_cpu = bool(bit_exact_cpu)
        if r_min < 0 or r_max < r_min:
            raise ValueError(f"Illegal range [{r_min}, {r_max}]")
        if method == "equally-spaced-noisy":        # r^2 ~ U[r_min^2, r_max^2]
            lo, span = r_min ** 2, r_max ** 2 - r_min ** 2
            self.get_r = lambda: torch.sqrt(span * torch.rand(self.shape, device=_CPU) + lo)
        elif method == "equally-radius-noisy":      # r ~ U[r_min, r_max]
            lo, span = r_min, r_max - r_min
            self.get_r = lambda: span * torch.rand(self.shape, device=_CPU) + lo
        else:
            raise ValueError(f"Unknown method: {method}")
        self.size, self.r_min, self.r_max, self.method = size, r_min, r_max, method
        self.shape = (size,)

    def get_examples(self):
        a, b, c = (torch.rand(self.shape, device=_CPU) for _ in range(3))
        denom = a + b + c
        eps = 1e-6
        x, y, z = (torch.sqrt(v / denom) + eps for v in (a, b, c))
        sx, sy, sz = (torch.randint(0, 2, self.shape, dtype=x.dtype, device=_CPU) * 2 - 1 for _ in range(3))
        x, y, z = x * sx, y * sy, z * sz
        theta = torch.acos(z).requires_grad_(True)
        phi = (-torch.atan2(y, x) + np.pi).requires_grad_(True)   # atan2 ranges (-pi, pi]; shift to [0, 2pi)
        r = self.get_r().requires_grad_(True)
        return r, theta, phi

    def _internal_vars(self):
        d = super()._internal_vars()
        d.update(r_min=self.r_min, r_max=self.r_max, method=self.method)
        return d


class Generator3D(BaseGenerator):
    """Points on a (noisy) 3-D grid (generators.py:317-416)."""

    def __init__(self, grid=(10, 10, 10), xyz_min=(0.0, 0.0, 0.0), xyz_max=(1.0, 1.0, 1.0),
                 method="equally-spaced-noisy", bit_exact_cpu=False):
        super().__init__()
        self.bit_exact_cpu = bool(bit_exact_cpu)
        self.grid, self.size = grid, grid[0] * grid[1] * grid[2]
        self.xyz_min, self.xyz_max, self.method = xyz_min, xyz_max, method
        if method in ("equally-spaced", "equally-spaced-noisy"):
            axes = [torch.linspace(xyz_min[i], xyz_max[i], grid[i], requires_grad=True, device=_CPU) for i in range(3)]
        elif method in ("chebyshev", "chebyshev1"):
            axes = [_chebyshev_first(xyz_min[i], xyz_max[i], grid[i]) for i in range(3)]
        elif method == "chebyshev2":
            axes = [_chebyshev_second(xyz_min[i], xyz_max[i], grid[i]) for i in range(3)]
        else:
            raise ValueError(f"Unknown method: {method}")
        gx, gy, gz = torch.meshgrid(*axes, indexing="ij")
        self.grid_x, self.grid_y, self.grid_z = gx.flatten(), gy.flatten(), gz.flatten()
        if method == "equally-spaced-noisy":
            self.noise_std = [((xyz_max[i] - xyz_min[i]) / grid[i]) / 4.0 for i in range(3)]
            self.getter = lambda: tuple(torch.normal(mean=m, std=s) for m, s in
                                        zip((self.grid_x, self.grid_y, self.grid_z), self.noise_std))
        else:
            self.getter = lambda: (self.grid_x, self.grid_y, self.grid_z)

    def get_examples(self):
        return self.getter()


class ConcatGenerator(BaseGenerator):
    """``g1 + g2``: concatenated samples (generators.py:658-691)."""

    def __init__(self, *generators):
        super().__init__()
        self.generators = generators
        self.size = sum(g.size for g in generators)

    def get_examples(self):
        draws = [g.get_examples() for g in self.generators]
        if isinstance(draws[0], torch.Tensor):
            return torch.cat(draws)
        return tuple(torch.cat(parts) for parts in zip(*draws))


class EnsembleGenerator(BaseGenerator):
    """``g1 * g2``: same number of points, more dimensions (generators.py:826-876)."""

    def __init__(self, *generators):
        super().__init__()
        self.size = generators[0].size
        for i, g in enumerate(generators):
            if g.size != self.size:
                raise ValueError(f"gens[{i}].size ({g.size}) != gens[0].size ({self.size})")
        self.generators = generators

    def get_examples(self):
        out = ()
        for g in self.generators:
            ex = g.get_examples()
            out += (ex,) if isinstance(ex, torch.Tensor) else tuple(ex)
        return out[0] if len(out) == 1 else out


class MeshGenerator(BaseGenerator):
    """``g1 ^ g2``: ij-meshgrid of the sub-generators' samples, flattened (generators.py:848-901); nested meshes are
    flattened into one (``(g1 ^ g2) ^ g3 == MeshGenerator(g1, g2, g3)``)."""

    def __init__(self, *generators):
        super().__init__()
        self.generators = []
        for g in generators:
            self.generators += list(g.generators) if isinstance(g, MeshGenerator) else [g]
        self.size = int(np.prod([g.size for g in self.generators]))

    def get_examples(self):
        parts = ()
        for g in self.generators:
            ex = g.get_examples()
            parts += (ex,) if isinstance(ex, torch.Tensor) else tuple(ex)
        if len(parts) == 1:
            return parts[0]
        return tuple(m.flatten() for m in torch.meshgrid(*parts, indexing="ij"))

    def _internal_vars(self):
        d = super()._internal_vars()
        d.update(generators=self.generators)
        return d


class StaticGenerator(BaseGenerator):
    """Draw once, return the same points forever (generators.py:694-720)."""

    def __init__(self, generator):
        super().__init__()
        self.generator, self.size = generator, generator.size
        self.examples = generator.get_examples()

    def get_examples(self):
        return self.examples


class PredefinedGenerator(BaseGenerator):
    """Fixed user-supplied points (generators.py:723-756)."""

    def __init__(self, *xs):
        super().__init__()
        self.xs = [x if isinstance(x, torch.Tensor) else torch.tensor(x, device=_CPU) for x in xs]
        self.xs = [x.detach().clone().reshape(-1).requires_grad_(True) for x in self.xs]
        self.size = len(self.xs[0])
        if any(len(x) != self.size for x in self.xs):
            raise ValueError("tensors of different lengths encountered")
        if len(self.xs) == 1:
            self.xs = self.xs[0]

    def get_examples(self):
        return self.xs


class GeneratorND(BaseGenerator):
    """Points on an N-dimensional (noisy) grid with a sampling method per axis (generators.py:419-569):
    'equally-spaced', 'uniform', 'log-spaced', 'exp-spaced' (keyword ``base``), 'chebyshev' / 'chebyshev1', 'chebyshev2';
    keyword ``cut`` slices each axis, ``abs_value`` folds the jittered samples to non-negative values.  The jitter is
    one ``torch.normal`` per axis over the flattened ij-meshgrid, in axis order."""

    def __init__(self, grid=(10, 10), r_min=(0.0, 0.0), r_max=(1.0, 1.0), methods=("equally-spaced", "equally-spaced"),
                 noisy=True, r_noise_std=None, **kwargs):
        super().__init__()
        self.size = int(np.prod(grid))
        self.grid, self.r_min, self.r_max = grid, r_min, r_max
        self.methods, self.noisy, self.r_noise_std = methods, noisy, r_noise_std
        tup = lambda v: (v,) if isinstance(v, (int, float)) else v
        methods = [methods] if isinstance(methods, str) else methods
        grid, r_min, r_max = tup(grid), tup(r_min), tup(r_max)
        r_noise_std = tup(r_noise_std) if r_noise_std is not None else None
        n_dim = len(grid)
        cut = kwargs.pop("cut", tuple((None, None) for _ in range(n_dim)))
        base = tup(kwargs.pop("base", tuple(10 for _ in range(n_dim))))
        abs_value = kwargs.pop("abs_value", False)
        if kwargs:
            raise ValueError(f"Unknown keyword argument(s): {list(kwargs.keys())}")
        if cut[0] is None or isinstance(cut[0], (int, float)):
            cut = (cut,)
        axes, stds = [], []
        for i in range(n_dim):
            lo, hi, n, method = r_min[i], r_max[i], grid[i], methods[i]
            std = r_noise_std[i] if r_noise_std else ((hi - lo) / n) / 4.0
            if method == "equally-spaced":
                x = torch.linspace(lo, hi, n, requires_grad=True, device=_CPU)
                sd = std * torch.ones(n)
            elif method == "uniform":
                x = torch.zeros(n, requires_grad=True, device=_CPU) + torch.rand(n, device=_CPU) * (hi - lo) + lo
                sd = torch.zeros(n)
            elif method == "log-spaced":
                a, b = np.log10(lo), np.log10(hi)
                x = torch.logspace(a, b, n, requires_grad=True, device=_CPU)
                sd = std * torch.logspace(a, b, n, device=_CPU)
            elif method == "exp-spaced":
                x = torch.linspace(base[i] ** lo, base[i] ** hi, n, device=_CPU)
                x = (torch.log(x) / np.log(base[i])).clone().detach().requires_grad_(True)
                sd = (std * x).clone().detach()
            elif method in ("chebyshev", "chebyshev1"):
                x, sd = _chebyshev_first(lo, hi, n), std * torch.ones(n)
            elif method == "chebyshev2":
                x, sd = _chebyshev_second(lo, hi, n), std * torch.ones(n)
            else:
                raise ValueError(f"Unknown method: {method}")
            axes.append(x[cut[i][0]:cut[i][1]])
            stds.append(sd[cut[i][0]:cut[i][1]])
        # per-axis nodes / widths (after `cut`) the meshgrids are built from, and the fold: read by table_spec only
        self.axis_r, self.axis_std, self.abs_value = axes, stds, bool(abs_value)
        self.grid_r = [m.flatten() for m in torch.meshgrid(*axes, indexing="ij")]
        self.grid_std = [m.flatten() for m in torch.meshgrid(*stds, indexing="ij")]
        if not noisy:
            self.getter = lambda: tuple(self.grid_r)
        elif abs_value:
            self.getter = lambda: tuple(torch.abs(torch.normal(m, s)) for m, s in zip(self.grid_r, self.grid_std))
        else:
            self.getter = lambda: tuple(torch.normal(m, s) for m, s in zip(self.grid_r, self.grid_std))

    def get_examples(self):
        return self.getter()

    def _internal_vars(self):
        d = super()._internal_vars()
        d.update(grid=self.grid, r_min=self.r_min, r_max=self.r_max, methods=self.methods, noisy=self.noisy,
                 r_noise_std=self.r_noise_std)
        return d


class TransformGenerator(BaseGenerator):
    """Applies ``transforms[i]`` to the i-th sample vector (``None`` = identity), or one ``transform`` to all of them
    at once (generators.py:752-801)."""

    def __init__(self, generator, transforms=None, transform=None):
        super().__init__()
        self.generator, self.size = generator, generator.size
        if transforms is not None and transform is not None:
            raise ValueError("transform and transforms cannot be both specified")
        if transforms is not None:
            self.trans = [(lambda x: x) if t is None else t for t in transforms]
        else:
            self.trans = transform if transform is not None else (lambda x: x)

    def get_examples(self):
        xs = self.generator.get_examples()
        if isinstance(xs, torch.Tensor):
            return self.trans(xs) if callable(self.trans) else self.trans[0](xs)
        if callable(self.trans):
            return self.trans(*xs)
        return tuple(t(x) for t, x in zip(self.trans, xs))

    def _internal_vars(self):
        d = super()._internal_vars()
        d.update(generator=self.generator, trans=self.trans)
        return d


class FilterGenerator(BaseGenerator):
    """Keeps the samples where ``filter_fn(list of sample vectors)`` (a boolean mask) holds (generators.py:904-952)."""

    def __init__(self, generator, filter_fn, size=None, update_size=True):
        super().__init__()
        self.generator, self.filter_fn = generator, filter_fn
        self.size = generator.size if size is None else size
        self.update_size = update_size

    def get_examples(self):
        xs = self.generator.get_examples()
        xs = [xs] if isinstance(xs, torch.Tensor) else xs
        mask = self.filter_fn(xs)
        xs = [x[mask] for x in xs]
        if self.update_size:
            self.size = len(xs[0])
        return xs[0] if len(xs) == 1 else xs

    def _internal_vars(self):
        d = super()._internal_vars()
        d.update(generator=self.generator, filter_fn=self.filter_fn)
        return d


class ResampleGenerator(BaseGenerator):
    """Shuffled sub-sample of another generator's output, with or without replacement (generators.py:955-993); the index
    draw (``randint`` / ``randperm``) precedes the inner generator's own draw, like in the reference."""

    def __init__(self, generator, size=None, replacement=False):
        super().__init__()
        self.generator = generator
        self.size = generator.size if size is None else size
        self.replacement = replacement

    def get_examples(self):
        if self.replacement:
            idx = torch.randint(self.generator.size, (self.size,), device=_CPU)
        else:
            idx = torch.randperm(self.generator.size, device=_CPU)[:self.size]
        xs = self.generator.get_examples()
        return xs[idx] if isinstance(xs, torch.Tensor) else [x[idx] for x in xs]

    def _internal_vars(self):
        d = super()._internal_vars()
        d.update(generator=self.generator, replacement=self.replacement)
        return d


class BatchGenerator(BaseGenerator):
    """Serves another generator's samples ``batch_size`` at a time from a cache that is refilled when it runs short
    (generators.py:996-1043)."""

    def __init__(self, generator, batch_size):
        super().__init__()
        if generator.size <= 0:
            raise ValueError(f"generator has size {generator.size} <= 0")
        self.generator, self.size = generator, batch_size
        first = generator.get_examples()
        self.cached_xs = [first] if isinstance(first, torch.Tensor) else list(first)

    def get_examples(self):
        while len(self.cached_xs[0]) < self.size:
            more = self.generator.get_examples()
            more = [more] if isinstance(more, torch.Tensor) else more
            self.cached_xs = [torch.cat([x, m]) for x, m in zip(self.cached_xs, more)]
        batch = [x[:self.size] for x in self.cached_xs]
        self.cached_xs = [x[self.size:] for x in self.cached_xs]
        return batch[0] if len(batch) == 1 else batch

    def _internal_vars(self):
        d = super()._internal_vars()
        d.update(generator=self.generator)
        return d


_STATIC_METHODS = {Generator1D: ("equally-spaced", "log-spaced", "chebyshev", "chebyshev1", "chebyshev2"),
                   Generator2D: ("equally-spaced", "chebyshev", "chebyshev1", "chebyshev2", "latin-hypercube"),
                   Generator3D: ("equally-spaced", "chebyshev", "chebyshev1", "chebyshev2")}


def draws_are_static(g):
    """True if ``g.get_examples()`` provably returns the same points on every call without touching the RNG (the default
    validation grids, StaticGenerator, PredefinedGenerator, combinations of those)."""
    if isinstance(g, SamplerGenerator):
        return draws_are_static(g.generator)
    if type(g) in _STATIC_METHODS:
        return g.method in _STATIC_METHODS[type(g)]
    if type(g) in (StaticGenerator, PredefinedGenerator):
        return True
    if type(g) is GeneratorND:
        return not g.noisy and "uniform" not in (g.methods if not isinstance(g.methods, str) else (g.methods,))
    if type(g) in (ConcatGenerator, EnsembleGenerator, MeshGenerator):
        return all(draws_are_static(x) for x in g.generators)
    return False


def draws_have_fixed_size(g):
    """True if every ``g.get_examples()`` is known to return ``g.size`` points (the reference's own generator classes
    except FilterGenerator / TransformGenerator, whose user callables may do anything)."""
    if isinstance(g, SamplerGenerator):
        return draws_have_fixed_size(g.generator)
    if type(g) in (Generator1D, Generator2D, Generator3D, GeneratorND, GeneratorSpherical, StaticGenerator,
                   PredefinedGenerator, ResidentBatchGenerator):
        return True
    if type(g) in (ConcatGenerator, EnsembleGenerator, MeshGenerator):
        return all(draws_have_fixed_size(x) for x in g.generators)
    if type(g) is ResampleGenerator and not g.replacement and g.size > g.generator.size:
        return False                  # randperm(generator.size)[:size] yields generator.size points, not `size`
    if type(g) in (ResampleGenerator, BatchGenerator):
        return draws_have_fixed_size(g.generator)
    return False


class SamplerGenerator(BaseGenerator):
    """Solver-side wrapper: always returns a list of ``(N, 1)`` columns that require grad (generators.py:1046-1064)."""

    def __init__(self, generator):
        super().__init__()
        self.generator, self.size = generator, generator.size
        self._last = None

    def get_examples(self):
        samples = self.generator.get_examples()
        if isinstance(samples, torch.Tensor):
            samples = [samples]
        if samples[0].device.type == "cuda" and not samples[0].requires_grad:
            if samples[0].dim() == 2:
                return samples                                   # resident batch: already (N, 1) views, zero-copy
            return [s.reshape(-1, 1) for s in samples]
        # a static generator hands back the very same tensors every time (default validation grids): serve the same
        # columns again (the engine recognises them and skips the upload); fresh leaves as far as autograd can tell
        last = self._last
        if last is not None and len(last[0]) == len(samples) and \
                all(a is b and b._version == v for a, b, v in zip(last[0], samples, last[1])):
            for c in last[2]:
                c.grad = None
            return last[2]
        cols = [s.reshape(-1, 1).detach().requires_grad_(True) for s in samples]
        self._last = (tuple(samples), tuple(s._version for s in samples), cols)
        return cols


class ResidentBatchGenerator(BaseGenerator):
    """Pre-sampled batches kept resident in HBM as SoA blocks ``[n_batches][d][ld]`` and served round-robin.

    New (no reference counterpart): it removes the host sampling + PCIe hand-off from a training step when the
    points can be drawn ahead of time -- ``ResidentBatchGenerator.presample(gen, k, device)`` draws ``k`` batches from
    any generator in the reference's RNG order (so they are the same points the reference would train on) and
    uploads them once.  ``get_examples`` returns views into the current block; the fused engine recognises them and
    reads the block in place (no copy)."""

    def __init__(self, blocks, size):
        super().__init__()
        self.blocks, self.size, self._next = blocks, size, 0
        self._views = {}

    @classmethod
    def presample(cls, generator, n_batches, device, lo=0, hi=None):
        draws = []
        for _ in range(n_batches):
            ex = generator.get_examples()
            ex = [ex] if isinstance(ex, torch.Tensor) else list(ex)
            draws.append(torch.stack([e.detach().reshape(-1)[lo:hi] for e in ex]))
        n = draws[0].shape[1]
        ld = (n + 63) // 64 * 64
        blocks = torch.zeros(n_batches, draws[0].shape[0], ld, dtype=torch.float32, device=device)
        blocks[:, :, :n] = torch.stack(draws).to(device)
        return cls(blocks, n)

    def get_examples(self):
        k = self._next % self.blocks.shape[0]
        self._next += 1
        views = self._views.get(k)
        if views is None:         # (N, 1) column views of the block's rows, built once per block
            blk = self.blocks[k]
            views = self._views[k] = [blk[i, :self.size].reshape(-1, 1) for i in range(blk.shape[0])]
        return views


class TableSpec:
    """Host-side description of a table draw (``ndq_table_sampler_desc`` minus the device pointers): per axis the number of
    nodes, the law, the fp32 node table (None for 'chebyshev2-noisy') and the fp32 width table (None: exact nodes)."""

    def __init__(self, n, law, mean, std, lo, hi, abs_value):
        self.n, self.law, self.mean, self.std, self.lo, self.hi, self.abs_value = n, law, mean, std, lo, hi, bool(abs_value)
        self.d = len(n)


_f32 = lambda t: np.ascontiguousarray(t.detach().cpu().numpy(), dtype=np.float32)
_TABLE_1D = ("log-spaced", "log-spaced-noisy", "chebyshev", "chebyshev1", "chebyshev2")


def table_spec(g):
    """:class:`TableSpec` of a generator the table sampler (``ndq_sample_table``) can draw: ``GeneratorND`` (every method,
    ``cut``, ``noisy`` or not, ``abs_value``, up to six axes) and the node-table laws of ``Generator1D``.  The tables are the
    tensors the generator built for itself, so exact nodes are the reference's own numbers.  ``ValueError`` for everything
    else: 'latin-hypercube' (a permutation of jittered strata: stays on the host), the wrapper generators (``g1 + g2``, ``g1 * g2``,
    ``g1 ^ g2``, Static / Predefined generators and a root-level Resample / Batch are composed from leaf laws by :func:`plan_spec`,
    not here), and a ``GeneratorND``
    whose ``grid_r`` / ``grid_std`` -- what its own getter draws from -- are no longer the meshgrids of its per-axis tensors
    (replaced or edited after construction: the tables would draw another law than the host getter)."""
    from . import _lib
    normal, cheb2n = _lib.NDQ_AXIS_NORMAL, _lib.NDQ_AXIS_CHEB2_NOISY
    if type(g) is GeneratorND and 1 <= len(g.axis_r) <= _lib.NDQ_TABLE_MAX_AXES:
        d = len(g.axis_r)
        mean = [_f32(x) for x in g.axis_r]
        std = [_f32(x) for x in g.axis_std] if g.noisy else [None] * d
        n = [len(m) for m in mean]
        idx = np.unravel_index(np.arange(int(np.prod(n))), n)
        for what, tables, grids in (("grid_r", mean, g.grid_r), ("grid_std", std, g.grid_std if g.noisy else [None] * d)):
            if len(grids) != d or any(t is not None and not np.array_equal(t[idx[c]], _f32(grids[c])) for c, t in enumerate(tables)):
                raise ValueError(f"{what} of {g!r} was changed after construction: it is not the meshgrid of the per-axis tables")
        # (the reference folds inside the noisy getter only: noisy=False hands out the nodes as they are)
        return TableSpec(n, [normal] * d, mean, std, [0.0] * d, [0.0] * d, g.noisy and g.abs_value)
    if type(g) is Generator1D and g.method in _TABLE_1D:
        mean = _f32(g.examples)
        std = np.full(len(mean), g.noise_std, dtype=np.float32) if g.method.endswith("-noisy") else None
        return TableSpec([len(mean)], [normal], [mean], [std], [0.0], [0.0], False)
    if type(g) is Generator1D and g.method == "chebyshev2-noisy":
        return TableSpec([int(g.size)], [cheb2n], [None], [None], [float(g.t_min)], [float(g.t_max)], False)
    raise ValueError(f"the table sampler cannot draw {g!r} on the device")


class PlanLeaf:
    """One leaf of a :class:`PlanSpec`: ``kind`` 'simple' (``desc``: the ``ndq_sampler_desc`` of :meth:`DeviceGenerator.describe`),
    'table' (``table``: the :class:`TableSpec`) or 'data' (``data``: the generator's fixed tensors as fp32 rows); ``row0`` /
    ``rows``: the output rows it writes; ``size``: its number of points; ``live``: the attributes it reads when it draws."""

    def __init__(self, gen, kind, rows, size, live, desc=None, table=None, data=None):
        self.gen, self.kind, self.rows, self.size, self.live = gen, kind, rows, size, live
        self.desc, self.table, self.data, self.row0 = desc, table, data, 0


class PlanIndex:
    """The root-level Resample / Batch part of a :class:`PlanSpec` (``ndq_plan_index_desc``): ``mode`` 'none' | 'permute' (a
    ResampleGenerator without replacement) | 'replace' (with), ``n`` points of the plan, ``m`` points of one (resampled) inner draw
    (``m == n`` without a Resample), ``batch``: 0, or the BatchGenerator's batch size."""

    def __init__(self, mode, n, m, batch):
        self.mode, self.n, self.m, self.batch = mode, n, m, batch


class PlanSpec:
    """Host-side description of a composed draw (``ndq_plan_sampler_desc`` minus the device pointers): ``leaves`` numbered
    depth-first from 0, ``segments`` = [(mode, first leaf, leaf count, point offset, points)] with mode 'leaf' / 'ensemble' /
    'mesh', ``d`` rows, ``size`` points handed out per draw, ``wrappers``: every Concat / Ensemble / Mesh node of the tree (and the
    root-level Resample / Batch / Transform / Filter nodes), ``index``: None, or the :class:`PlanIndex` of a Resample / Batch root
    -- ``size`` is then ``index.batch or index.m``, the plan's own points are ``index.n``.  ``stages``: the per-point stages of the
    root chain from inner to outer, each ``('map', callable or list of callables)`` (a TransformGenerator's ``trans``) or
    ``('filter', fn)``; ``stage_nodes``: the generators they belong to; ``d_out``: rows handed out (``d`` without stages);
    ``filtered``: a filter is among the stages -- ``size`` is then the capacity of a draw, the kept count varies.  With stages:
    ``trace`` = (Graph, out nodes, keep node or None) of :func:`trace_stages`, ``watch``: the ``_pystate.StateWatch`` of the
    callables."""

    def __init__(self, d, size, leaves, segments, wrappers, index=None, stages=(), stage_nodes=()):
        self.d, self.leaves, self.segments, self.wrappers, self.index = d, leaves, segments, wrappers, index
        self.size = size if index is None else (index.batch or index.m)
        self.stages, self.stage_nodes, self.d_out = list(stages), list(stage_nodes), d
        self.filtered = any(kind == "filter" for kind, _ in self.stages)
        self.trace = self.watch = None


PLAN_MAX_LEAVES = 8
PLAN_MAX_ROWS = 6          # include/ndq.h NDQ_TABLE_MAX_AXES
#: leaf l of a plan draws under this seed (leaf 0: ``seed`` itself); two leaves never share a Philox key
plan_leaf_seed = lambda seed, l: (int(seed) + l * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
#: the index map of a Resample root (permutation rounds, with-replacement indices) draws under this key: the leaves own the
#: multipliers 0 .. PLAN_MAX_LEAVES - 1, so no leaf shares it
plan_index_seed = lambda seed: (int(seed) + PLAN_MAX_LEAVES * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF


def _plan_leaf(g):
    if isinstance(g, (ConcatGenerator, EnsembleGenerator, MeshGenerator)):
        raise ValueError(f"{g!r} is a wrapper, not a leaf")           # (callers name the nesting)
    if isinstance(g, (StaticGenerator, PredefinedGenerator)):          # DATA: the fixed tensors themselves, whatever is wrapped
        name = "examples" if isinstance(g, StaticGenerator) else "xs"
        ex = getattr(g, name)
        ex = [ex] if isinstance(ex, torch.Tensor) else list(ex)
        if not ex or any((not isinstance(e, torch.Tensor)) or e.dtype != torch.float32 or e.numel() != ex[0].numel() for e in ex):
            raise ValueError(f"the fixed points of {g!r} are not float32 tensors of one length: they cannot be handed out exactly")
        if ex[0].numel() < 1:
            raise ValueError(f"{g!r} holds no points")
        return PlanLeaf(g, "data", len(ex), ex[0].numel(), (name,), data=[_f32(e).reshape(-1) for e in ex])
    if isinstance(g, Generator1D) and g.method == "latin-hypercube":
        raise ValueError(f"'latin-hypercube' is a permutation and stays on the host, alone or inside a wrapper: {g!r}")
    try:
        desc = DeviceGenerator.describe(g)
        from . import _lib
        size = int(np.prod(list(desc.n)[:desc.d])) if desc.kind == _lib.NDQ_SAMPLE_GRID else int(desc.n[0])
        return PlanLeaf(g, "simple", int(desc.d), size, _LIVE, desc=desc)
    except ValueError:
        pass
    try:
        spec = table_spec(g)
    except ValueError:
        raise ValueError(f"the device sampler cannot draw {g!r} (neither a leaf law nor Concat / Ensemble / Mesh)") from None
    return PlanLeaf(g, "table", spec.d, int(np.prod(spec.n)), _LIVE_TABLE, table=spec)


def plan_spec(g, _redraw=False):
    """:class:`PlanSpec` of a composed generator the plan sampler (``ndq_sample_plan``) draws in one launch.  Normal form::

        plan    := Concat[segment, ...]                       (a lone segment is a plan of one segment)
        segment := leaf | Ensemble[leaf, ...] | Mesh[one-row leaf, ...]
        leaf    := what DeviceGenerator.describe accepts | what table_spec accepts
                 | PredefinedGenerator | StaticGenerator     (DATA: its fixed float32 tensors, uploaded once, exact)

    Concat inside Concat and Ensemble inside Ensemble are flattened (MeshGenerator flattens itself).  Leaves are numbered
    depth-first from 0; leaf ``l`` draws under ``plan_leaf_seed(seed, l)`` with its leaf-local point index as Philox counter
    word 0, so a composed draw is the ``torch.cat`` / tuple / ``torch.meshgrid(indexing="ij")`` composition of what
    ``DeviceGenerator(leaf, seed=plan_leaf_seed(seed, l))`` hands out -- two leaves never share a key, the same object used
    twice included (the reference draws ``g ^ g`` as two independent draws), and a mesh factor's jitter at a node is the same
    for every partner node (the reference draws each factor once, then meshgrids).  ``ValueError`` naming the node for:
    Concat inside Mesh / Ensemble, Mesh inside Ensemble, Ensemble inside Mesh, a mesh factor of more than one row (the
    reference makes every row an axis and gets ``size`` wrong), ensemble members of different sizes, segments with
    different row counts, more than six rows, more than eight leaves, 'latin-hypercube', and every other wrapper
    (the Sampler generator; Resample / Batch / Transform / Filter anywhere but in the root chain).

    At the ROOT only, drawn by ``ndq_sample_plan_indexed`` (still one launch, ``PlanSpec.index`` set)::

        root      := Batch[resampled] | resampled
        resampled := Resample[plan] | plan

    ``BatchGenerator(inner, bs)``: draw ``t`` is the window ``[t * bs, (t + 1) * bs)`` of the concatenated stream of inner draws
    (the reference's FIFO cache: the draw its constructor makes is inner draw 0, and a batch may straddle inner draws), so
    ``BatchGenerator(ResampleGenerator(g), bs)`` is a shuffled epoch over ``g`` served ``bs`` points at a time.
    ``ResampleGenerator(plan, size, replacement)``: element ``r`` of inner draw ``k`` is plan point ``j(r)`` of the plan's draw
    ``k`` -- ``replacement=False``: the head of a random permutation of the plan's points (a swap-or-not shuffle evaluated per
    index), ``True``: independent uniform indices -- under ``plan_index_seed(seed)``.  ``ValueError`` naming the node for
    ``Resample[Batch[...]]``, two Resamples, two Batches, ``replacement=False`` with ``size > generator.size`` (the reference then
    yields ``generator.size`` points, not ``size``), ``size < 1`` and a ``generator.size`` that is not the plan's point count.

    Per-point STAGES in the root chain, drawn by a generated module (``codegen.SamplerMapProgram``, csrc/ndq_sample_map.h)::

        root   := stage* over (Batch[resampled] | resampled)
        stage  := Transform | Filter

    A ``TransformGenerator`` may sit above the root or between Batch and Resample (a per-point map commutes with the window;
    below a Resample it stays refused: put it one level up, the points are the same); several compose in nesting order and may
    change the number of rows (1 .. 6).  A ``FilterGenerator`` sits above every Resample / Batch (its output size varies);
    transforms and further filters may sit above it: masks AND together, a later stage sees the rows as transformed so far.
    ``PlanSpec.stages`` / ``stage_nodes`` / ``d_out`` / ``filtered`` describe them, ``trace`` / ``watch`` are :func:`trace_stages`'
    result and the ``_pystate.StateWatch`` of the callables; every stage node joins ``wrappers``.  ``ValueError`` naming the node
    for a stage inside Concat / Ensemble / Mesh, a Filter below Resample / Batch, more than six output rows, a Filter whose
    ``size`` is not what it wraps, ``update_size=False``, whatever :func:`trace_stages` refuses, and callables whose state cannot
    be watched.  (``_redraw``: a DeviceGenerator re-plans a tree it has been drawing -- a Filter's ``size`` is then the last kept
    count.)"""
    wrappers, leaves, segments = [], [], []
    batch, resample = None, None
    root, stages = g, []                                # (stages: outer to inner while the chain is walked)
    while isinstance(g, (BatchGenerator, ResampleGenerator, TransformGenerator, FilterGenerator)):
        node, g = g, g.generator
        wrappers.append(node)
        if isinstance(node, TransformGenerator):
            if resample is not None:
                raise ValueError(f"TransformGenerator inside ResampleGenerator stays outside the plan sampler's normal form: {node!r} in "
                                 f"{resample!r} -- put it above the ResampleGenerator (a per-point map commutes with the index map: the "
                                 "same points)")
            stages.append((("map", node.trans), node))
        elif isinstance(node, FilterGenerator):
            if batch is not None or resample is not None:
                raise ValueError(f"FilterGenerator below {type(resample or batch).__name__} is outside the plan sampler's normal form (the "
                                 f"size of its draw varies, the index map is built for a fixed one): {node!r} in {resample or batch!r}")
            if not node.update_size:
                raise ValueError(f"{node!r} has update_size=False: the device hand-out always reports the number of points it kept "
                                 "(its tensors have that length), so `size` cannot stay behind")
            if not _redraw and node.size != g.size:
                raise ValueError(f"{node!r} has size = {node.size!r}, but the generator it filters yields {g.size} points")
            stages.append((("filter", node.filter_fn), node))
        elif isinstance(node, BatchGenerator):
            if resample is not None:
                raise ValueError(f"BatchGenerator inside ResampleGenerator is outside the plan sampler's normal form: "
                                 f"{node!r} in {resample!r}")
            if batch is not None:
                raise ValueError(f"BatchGenerator inside BatchGenerator is outside the plan sampler's normal form: {node!r} in {batch!r}")
            batch = node
            if not isinstance(batch.size, (int, np.integer)) or not 1 <= batch.size <= 2 ** 31 - 1:
                raise ValueError(f"{batch!r} has batch size {batch.size!r}: the device sampler serves 1 .. 2^31 - 1 points per draw")
        else:
            if resample is not None:
                raise ValueError(f"ResampleGenerator inside ResampleGenerator is outside the plan sampler's normal form: "
                                 f"{node!r} in {resample!r}")
            resample = node
            if not isinstance(resample.size, (int, np.integer)) or not 1 <= resample.size <= 2 ** 31 - 1:
                raise ValueError(f"{resample!r} has size {resample.size!r}: the device sampler draws 1 .. 2^31 - 1 points")
    stages.reverse()

    def no_stage(sub, node):                           # (stages inside Concat / Ensemble / Mesh: a later change)
        if isinstance(sub, (TransformGenerator, FilterGenerator)):
            raise ValueError(f"{type(sub).__name__} inside {type(node).__name__} is outside the plan sampler's normal form (per-point "
                             f"stages sit in the root chain only): {sub!r} in {node!r}")

    def parts(node):                                   # Concat inside Concat: flattened
        if isinstance(node, ConcatGenerator):
            wrappers.append(node)
            if not node.generators:
                raise ValueError(f"{node!r} concatenates nothing")
            for sub in node.generators:
                no_stage(sub, node)
                yield from parts(sub)
        else:
            yield node

    def members(node, kind, inside):                   # Ensemble inside Ensemble (Mesh inside Mesh): flattened
        wrappers.append(node)
        if not node.generators:
            raise ValueError(f"{node!r} combines nothing")
        for sub in node.generators:
            no_stage(sub, node)
            if isinstance(sub, kind):
                yield from members(sub, kind, inside)
            elif isinstance(sub, (ConcatGenerator, EnsembleGenerator, MeshGenerator)):
                raise ValueError(f"{type(sub).__name__} inside {inside} is outside the plan sampler's normal form: {sub!r} in {node!r}")
            else:
                yield sub

    d = None
    offset = 0
    for node in parts(g):
        first = len(leaves)
        if isinstance(node, EnsembleGenerator):
            mode, own = "ensemble", [_plan_leaf(m) for m in members(node, EnsembleGenerator, "EnsembleGenerator")]
            if any(f.size != own[0].size for f in own):
                raise ValueError(f"the members of {node!r} draw different numbers of points: {[f.size for f in own]}")
            size, row = own[0].size, 0
            for f in own:
                f.row0, row = row, row + f.rows
        elif isinstance(node, MeshGenerator):
            mode, own = "mesh", [_plan_leaf(m) for m in members(node, MeshGenerator, "MeshGenerator")]
            for f in own:
                if f.rows != 1:
                    raise ValueError(f"a mesh factor must be a one-row generator (the reference makes every row of {f.gen!r} an axis "
                                     f"of the mesh and gets `size` wrong): {node!r}")
            size, row = int(np.prod([f.size for f in own], dtype=np.int64)), len(own)
            for c, f in enumerate(own):
                f.row0 = c
        else:
            mode, own = "leaf", [_plan_leaf(node)]
            size, row = own[0].size, own[0].rows
        if d is not None and row != d:
            raise ValueError(f"the segments of {g!r} have different numbers of rows: {node!r} has {row}, the ones before it {d}")
        d = row
        leaves += own
        segments.append((mode, first, len(own), offset, size))
        offset += size
    from . import _lib
    if d > _lib.NDQ_TABLE_MAX_AXES:
        raise ValueError(f"{g!r} has {d} rows: the plan sampler writes at most {_lib.NDQ_TABLE_MAX_AXES}")
    if len(leaves) > PLAN_MAX_LEAVES:
        raise ValueError(f"{g!r} has {len(leaves)} leaves: the plan sampler takes at most {PLAN_MAX_LEAVES}")
    if offset > 2 ** 31 - 1:
        raise ValueError(f"{g!r} draws {offset} points: more than 2^31 - 1")
    index = None
    if batch is not None or resample is not None:
        mode, m = "none", offset
        if resample is not None:
            if resample.generator.size != offset:
                raise ValueError(f"{resample!r} draws its indices below generator.size = {resample.generator.size}, but the generator "
                                 f"yields {offset} points")
            mode, m = ("replace" if resample.replacement else "permute"), int(resample.size)
            if mode == "permute" and m > offset:
                raise ValueError(f"{resample!r} without replacement yields generator.size = {offset} points, not size = {m}: "
                                 "the device sampler draws blocks of a fixed size")
        index = PlanIndex(mode, offset, m, int(batch.size) if batch is not None else 0)
    plan = PlanSpec(d, offset, leaves, segments, wrappers, index, [st for st, _ in stages], [node for _, node in stages])
    if stages:
        from . import _pystate
        plan.trace = trace_stages(plan)
        plan.d_out = len(plan.trace[1])
        plan.watch = _pystate.StateWatch([f for _, fn in plan.stages for f in (fn if isinstance(fn, (list, tuple)) else [fn])])
        if not plan.watch.complete:
            raise ValueError(f"the callables of the stages of {root!r} read state that cannot be watched for changes "
                             f"({'; '.join(plan.watch.incomplete)}): the device sampler would go on drawing a stale transform / filter")
    return plan


def trace_stages(plan):
    """The stages of ``plan`` run ONCE on symbolic columns (:mod:`neurodiffeq_amd.symbolic`: one ``coord`` per plan row) ->
    ``(Graph, out_nodes, keep_node | None)``: the rows handed out and the AND of the filters' masks as nodes of one DAG, which
    ``codegen.SamplerMapProgram`` lowers to ``ndq_map_point``.  A map stage is called like ``TransformGenerator.get_examples``
    calls it (one callable on all columns, or a list of callables column by column) and its outputs are the next stage's
    columns; a filter stage receives the LIST of current columns and returns a mask.  Fails closed -- ``ValueError`` naming the
    stage's generator for: anything the tracer cannot express, an output that is not a per-point column, more than six rows, a
    map that returns a mask, a filter that does not, the batch size read into arithmetic."""
    from . import symbolic
    from .symbolic import Sym
    g = symbolic.Graph(plan.d)
    keep = None
    with symbolic.trace_scope(g):
        cols = [Sym(g, g.coord(c), leaf=True) for c in range(plan.d)]
        for k, ((kind, fn), node) in enumerate(zip(plan.stages, plan.stage_nodes)):
            where = f"stage {k} ({'transform' if kind == 'map' else 'filter'}) of the device draw, {node!r}"
            try:
                if kind == "filter":
                    out = fn(list(cols))
                elif callable(fn):
                    out = fn(*cols)
                else:                                  # (like the reference: zip stops at the shorter of the two)
                    out = fn[0](cols[0]) if len(cols) == 1 else tuple(t(x) for t, x in zip(fn, cols))
            except symbolic.TraceUnsupported as e:
                raise ValueError(f"{where} cannot be traced: {e}") from None
            except Exception as e:       # noqa: BLE001 -- user code that fails on symbolic columns: the host generator stays
                raise ValueError(f"{where} cannot be traced: {type(e).__name__}: {e}") from None
            if kind == "filter":
                if not (isinstance(out, Sym) and out.isbool):
                    raise ValueError(f"{where}: filter_fn must return a boolean mask of the points, not {type(out).__name__}")
                keep = out if keep is None else (keep & out)
                continue
            out = [out] if isinstance(out, (Sym, torch.Tensor)) or not isinstance(out, (tuple, list)) else list(out)
            for o in out:
                if not isinstance(o, Sym):
                    raise ValueError(f"{where}: every output must be a per-point column of the batch length, not {type(o).__name__}")
                if o.isbool:
                    raise ValueError(f"{where}: a transform returned a boolean mask where a column of coordinates is expected")
            if not 1 <= len(out) <= PLAN_MAX_ROWS:
                raise ValueError(f"{where} hands out {len(out)} rows: the device sampler writes 1 .. {PLAN_MAX_ROWS}")
            cols = [o._plain() for o in out]
    outs, keep = [c.i for c in cols], (keep.i if keep is not None else None)
    for i in g.reachable(outs + ([keep] if keep is not None else [])):
        if g.nodes[i][0] == "param":
            raise ValueError(f"a stage of {plan.stage_nodes[-1]!r} reads the batch size (x.shape[0], len(x), x.numel()) into its "
                             "arithmetic: the device draw evaluates one point at a time")
        if g.nodes[i][0] in ("net", "data"):
            raise ValueError(f"a stage of {plan.stage_nodes[-1]!r} reads something other than the rows of its point")
    return g, outs, keep


# (N, 1) view lists handed out by DeviceGenerators -> the generator (engine.fast_train_epoch asks for a prefetch)
_DEVICE_SOURCES = {}


def _forget_sources(ids):
    for i in ids:
        _DEVICE_SOURCES.pop(i, None)


def device_source(batch):
    """The DeviceGenerator that handed out ``batch`` (its own list of views), or None."""
    ref = _DEVICE_SOURCES.get(id(batch))
    g = ref() if ref is not None else None
    return g if (g is not None and any(v is batch for v in g._views_all)) else None


class DeviceGenerator(BaseGenerator):
    """Draws the distribution of a reference generator ON the MI355X (csrc/ndq_sample.h through ``ndq_sample``).

    New (no reference counterpart): host sampling is the floor of a fused step
    (``torch.normal`` over 2 x 65 536 points costs ~10x the whole fused C2 step).  Wrapping a generator keeps its
    distribution -- grid geometry, jitter standard deviation, radial law -- but draws from a counter-based
    Philox4x32-10 stream: batch number ``k`` of a given ``seed`` (default ``torch.initial_seed()`` at construction) and
    ``stream_id`` (default: the process rank, so data-parallel ranks draw disjoint streams) is always the same
    points, yet they are NOT the numbers the reference's host generator would produce, hence opt-in.

    Supported: ``Generator1D`` ('uniform', 'equally-spaced', 'equally-spaced-noisy'), ``Generator2D`` / ``Generator3D``
    ('equally-spaced', 'equally-spaced-noisy'), ``GeneratorSpherical`` (both radial laws) through ``ndq_sample``; and, from
    per-axis node / width tables uploaded once (:func:`table_spec`, ``ndq_sample_table``): ``GeneratorND`` (1..6 axes, every
    method, ``cut``, ``noisy`` or not, ``abs_value``) and ``Generator1D`` 'log-spaced', 'log-spaced-noisy', 'chebyshev' /
    'chebyshev1', 'chebyshev2', 'chebyshev2-noisy' (no ``prefetch`` for these); and, composed by ONE kernel (:func:`plan_spec`,
    ``ndq_sample_plan``, no ``prefetch`` either): ``g1 + g2`` (ConcatGenerator), ``g1 * g2`` (EnsembleGenerator) and ``g1 ^ g2``
    (MeshGenerator) over any of the above, ``StaticGenerator`` and ``PredefinedGenerator`` (their fixed points, uploaded once and
    handed out bit for bit); leaf ``l`` of a composition draws under ``plan_leaf_seed(seed, l)``, so the batch is the
    composition of what a DeviceGenerator of each leaf hands out under that seed; and, at the ROOT of any of the above, by that
    same launch (``ndq_sample_plan_indexed``): ``ResampleGenerator`` (with or without replacement) and ``BatchGenerator`` --
    ``DeviceGenerator(BatchGenerator(ResampleGenerator(g), bs))`` is a shuffled epoch over ``g`` served ``bs`` points per draw
    with no ``randperm``, gather or upload; draw ``t`` is the window ``[t * bs, (t + 1) * bs)`` of the stream of inner draws, the
    permutation is a swap-or-not shuffle under ``plan_index_seed(seed)`` evaluated per point.  Opt-in: :func:`on_default_device`
    never wraps these; and, above the root of any of the above, ``TransformGenerator`` and ``FilterGenerator`` (:func:`plan_spec`
    "stages"): the user's callables are traced once, compiled into a small module and applied per point -- a transform in the
    plan's single launch, a filter by three launches (count, scan, order-preserving compact) plus ONE 4-byte readback of the
    kept count per draw, the only host synchronisation of any route (a batch's length is part of its tensors' shape); ``size``
    and the wrapped FilterGenerator's ``size`` follow the kept count, the views of a filtered draw are built per draw.
    Not drawn on the device: 'latin-hypercube' (a permutation), alone or inside a wrapper, the Sampler generator,
    Transform / Filter / Resample / Batch outside the root chain, stages that cannot be traced or watched, and compositions
    outside the normal form of :func:`plan_spec`.  ``get_examples`` enqueues
    one kernel on the current stream and returns ``(N, 1)`` views of ONE resident SoA block which the fused engine
    reads in place; the block is overwritten by the next draw (stream-ordered, so the previous step has consumed it).
    (Drawing the next batch on a side stream while the current one trains was tried: the event waits between the two
    streams cost more than the 4 us kernel they hide -- 41 us per step instead of 33 -- and it was dropped.)
    """

    def __init__(self, generator, device=None, seed=None, stream_id=None, prefetch=False, dtype=torch.float32):
        """dtype: torch.float32, or torch.float64 for fp64 solvers (the reference's default precision): the kernel draws fp32
        points, the handed-out tensors are their exact images in double (one device-side copy per draw)."""
        super().__init__()
        from . import _lib
        if dtype not in (torch.float32, torch.float64):
            raise ValueError(f"dtype must be torch.float32 or torch.float64, got {dtype}")
        if not torch.cuda.is_available():
            raise _lib.NdqError("DeviceGenerator samples with a gfx950 kernel and needs an MI355X; use the wrapped "
                                "generator itself for host sampling")
        self.generator, self.size = generator, generator.size
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        self.seed = int(torch.initial_seed() if seed is None else seed) & 0xFFFFFFFFFFFFFFFF
        self.stream_id = int(os.environ.get("RANK", "0")) if stream_id is None else int(stream_id)
        self.draw = 0
        self.table = None            # the TableSpec when the batch is drawn by ndq_sample_table (second route), else None
        self.plan = None             # the PlanSpec when the batch is drawn by ndq_sample_plan (third route), else None
        try:
            self.desc = self.describe(generator)
            names = _LIVE
        except ValueError:
            try:
                spec, plan = table_spec(generator), None
            except ValueError:
                spec, plan = None, plan_spec(generator)      # (ValueError: no sampler draws this generator)
            if prefetch:
                raise ValueError(f"prefetch=True is not available for {generator!r}: the epoch tail's prefetch draws "
                                 "ndq_sampler_desc laws only, and this generator is drawn from tables")
            if plan is None:
                self._set_table(spec)
                self.size = int(np.prod(spec.n))     # (GeneratorND: `cut` shortens the draw, `size` stays the product of `grid`)
                names = _LIVE_TABLE
            else:
                self._set_plan(plan)
                self.size = plan.size                # (the points actually produced: a GeneratorND leaf counts its table size)
                names = ()                           # (the whole tree is watched: _restamp)
        # the descriptor froze what the wrapped generator draws from; the reference reads it at every draw (generators.py:107-416),
        # so a callback that changes a noise width / replaces a grid tensor or the getter has to be seen: live_stamp per draw
        self._live_names = tuple(n for n in names if n in vars(generator))
        self._restamp()
        self._on_host = False
        self._L = _lib.lib()
        ld = (self.size + 63) // 64 * 64
        # rows of the resident block / rows handed out: a plan with stages draws d rows per point and hands out d_out
        rows, self._rows_out = (self.desc.d, self.desc.d) if self.plan is None else (max(self.plan.d, self.plan.d_out), self.plan.d_out)
        # prefetch=True: a solver on the single-launch native path lets the extra workgroups of its sums + tail kernel
        # draw the NEXT batch (ndq_fused_step.next_sampler) -- the sampler launch leaves the step.  The points are the
        # same (draw k is a function of (seed, k, stream_id) only).  Two blocks alternate (draw k lives in block k & 1), so
        # the tensors handed out for an epoch keep that epoch's points until the END of the following epoch.
        self.prefetch = bool(prefetch)
        self.blocks = [torch.zeros(rows, ld, dtype=torch.float32, device=self.device) for _ in range(2 if self.prefetch else 1)]
        self.dtype = dtype
        # fp64: the tensors handed out are views of double blocks the fp32 draws are copied into
        self._out_blocks = self.blocks if dtype == torch.float32 else [torch.zeros_like(b, dtype=dtype) for b in self.blocks]
        self._views_all = [[blk[i, :self.size].reshape(-1, 1) for i in range(self._rows_out)] for blk in self._out_blocks]
        self.block, self._views = self.blocks[0], self._views_all[0]
        self.prefetched = None       # draw number already sitting in its block, drawn ahead by a tail kernel
        self.launches = 0            # sampler kernels this generator launched itself (diagnostics / tests)
        self.readbacks = 0           # kept counts read back from the device (filter route: one per draw)
        # (weak: the registry must not keep a generator -- two device blocks -- alive after its solver is gone; the entries go
        # with it, before the ids of its view lists can be reused.  The filter route hands out a new list per draw -- its length
        # is the kept count --: _filtered_views replaces the generator's entry, the registry does not grow)
        self._source_ids = set()
        weakref.finalize(self, _forget_sources, self._source_ids)
        for views in self._views_all:
            self._register(views)

    def _register(self, views):
        _DEVICE_SOURCES[id(views)] = weakref.ref(self)
        self._source_ids.add(id(views))

    @staticmethod
    def describe(g):
        """``ndq_sampler_desc`` of a reference-style generator; ``ValueError`` for what the kernel does not draw."""
        from . import _lib
        d = _lib.SamplerDesc()
        grid_methods = ("equally-spaced", "equally-spaced-noisy")

        def grid(ns, lo, hi, std):
            d.kind, d.d = _lib.NDQ_SAMPLE_GRID, len(ns)
            for i in range(len(ns)):
                d.n[i], d.lo[i], d.hi[i], d.noise_std[i] = int(ns[i]), float(lo[i]), float(hi[i]), float(std[i])
        if isinstance(g, Generator1D) and g.method == "uniform":
            d.kind, d.d = _lib.NDQ_SAMPLE_UNIFORM, 1
            d.n[0], d.lo[0], d.hi[0] = g.size, g.t_min, g.t_max
        elif isinstance(g, Generator1D) and g.method in grid_methods:
            grid([g.size], [g.t_min], [g.t_max], [g.noise_std if g.method.endswith("noisy") else 0.0])
        elif isinstance(g, Generator2D) and g.method in grid_methods:
            grid(g.grid, g.xy_min, g.xy_max, [g.noise_xstd, g.noise_ystd] if g.method.endswith("noisy") else [0.0, 0.0])
        elif isinstance(g, Generator3D) and g.method in grid_methods:
            grid(g.grid, g.xyz_min, g.xyz_max, g.noise_std if g.method.endswith("noisy") else [0.0] * 3)
        elif isinstance(g, GeneratorSpherical):
            d.kind, d.d = _lib.NDQ_SAMPLE_SPHERICAL, 3
            d.n[0], d.lo[0], d.hi[0] = g.size, g.r_min, g.r_max
            d.radial = int(g.method == "equally-radius-noisy")
        else:
            raise ValueError(f"DeviceGenerator cannot draw {g!r} on the device")
        return d

    def _upload(self, tables):
        """{key: fp32 array} -> (ONE device buffer holding them all -- one upload, kept alive by this generator --, {key: device
        address})."""
        parts, at, where = [], 0, {}
        for key, t in tables.items():
            where[key] = at
            parts.append(np.pad(t, (0, -len(t) % 4)))      # every table starts 16-byte aligned
            at += len(parts[-1])
        buf = torch.from_numpy(np.concatenate(parts) if parts else np.zeros(4, np.float32)).to(self.device)
        return buf, {key: buf.data_ptr() + 4 * at for key, at in where.items()}

    @staticmethod
    def _spec_tables(spec, tag=()):
        """The node / width tables of a TableSpec, keyed for _upload / _fill_table."""
        return {tag + (kind, c): t for kind, tables in (("mean", spec.mean), ("std", spec.std)) for c, t in enumerate(tables)
                if t is not None}

    @staticmethod
    def _fill_table(d, spec, where, tag=()):
        d.d, d.abs_value = spec.d, int(spec.abs_value)
        for c in range(spec.d):
            d.n[c], d.law[c], d.lo[c], d.hi[c] = spec.n[c], spec.law[c], spec.lo[c], spec.hi[c]
            d.mean[c] = where.get(tag + ("mean", c))
            d.std[c] = where.get(tag + ("std", c))

    def _set_table(self, spec):
        """Descriptor of the table route: every node / width table of ``spec`` in ONE device buffer, the descriptor's pointers
        into it."""
        from . import _lib
        d = _lib.TableSamplerDesc()
        buf, where = self._upload(self._spec_tables(spec))
        self._fill_table(d, spec, where)
        self.table, self._table_buf, self.desc = spec, buf, d

    def _set_plan(self, plan):
        """Descriptor of the plan route: the node, width and DATA tables of ALL leaves in ONE device buffer, uploaded here and never
        again; the descriptor itself travels by value with every launch (no per-draw copy to the device)."""
        from . import _lib
        tables = {}
        for l, f in enumerate(plan.leaves):
            if f.kind == "table":
                tables.update(self._spec_tables(f.table, (l,)))
            elif f.kind == "data":
                tables.update({(l, "data", c): row for c, row in enumerate(f.data)})
        buf, where = self._upload(tables)
        d = _lib.PlanSamplerDesc()
        d.d, d.n_leaves, d.n_segments = plan.d, len(plan.leaves), len(plan.segments)
        for l, f in enumerate(plan.leaves):
            leaf = d.leaf[l]
            leaf.kind = {"simple": _lib.NDQ_LEAF_SIMPLE, "table": _lib.NDQ_LEAF_TABLE, "data": _lib.NDQ_LEAF_DATA}[f.kind]
            leaf.row0, leaf.rows, leaf.n = f.row0, f.rows, f.size
            if f.kind == "simple":
                leaf.u.simple = f.desc
            elif f.kind == "table":
                self._fill_table(leaf.u.table, f.table, where, (l,))
            else:
                for c in range(f.rows):
                    leaf.u.data[c] = where[l, "data", c]
        modes = {"leaf": _lib.NDQ_SEG_LEAF, "ensemble": _lib.NDQ_SEG_ENSEMBLE, "mesh": _lib.NDQ_SEG_MESH}
        for k, (mode, first, count, offset, size) in enumerate(plan.segments):
            g = d.seg[k]
            g.mode, g.first, g.count, g.offset, g.size = modes[mode], first, count, offset, size
        self.plan, self._table_buf, self.desc = plan, buf, d
        self._index = None               # the ndq_plan_index_desc of a Resample / Batch root (ndq_sample_plan_indexed), else None
        if plan.index is not None:
            ix = _lib.PlanIndexDesc()
            ix.mode = {"none": _lib.NDQ_INDEX_NONE, "permute": _lib.NDQ_INDEX_PERMUTE, "replace": _lib.NDQ_INDEX_REPLACE}[plan.index.mode]
            ix.m, ix.batch = plan.index.m, plan.index.batch
            self._index = ix
        # stages (TransformGenerator / FilterGenerator in the root chain): the generated module that draws plan + stages
        self._map = self._work = None
        if plan.stages:
            from . import codegen
            graph, outs, keep = plan.trace
            self._map = codegen.load_sampler_map(codegen.SamplerMapProgram(graph, outs, keep, plan.d))
            if plan.filtered:        # [kept | per-workgroup counts -> offsets]: owned by the generator, rewritten by every draw
                self._work = torch.zeros(1 + (plan.size + 255) // 256, dtype=torch.int32, device=self.device)

    def get_examples(self):
        if torch._C._len_torch_function_stack():          # a global default-device mode: see engine.library_code
            with torch._C.DisableTorchFunction():
                return self._get_examples()
        return self._get_examples()

    def block_of(self, draw):
        """The block draw number ``draw`` lives in."""
        return self.blocks[draw & 1] if self.prefetch else self.blocks[0]

    def _restamp(self):
        g = self.generator
        self._stamp = live_stamp(g, self._live_names)
        d = vars(g)
        # the per-draw form of the same stamp: object identity of every live attribute + the version counters of the tensors
        self._quick = tuple((n, d.get(n)) for n in self._live_names)
        tensors = [v for _, v in self._quick]
        # (table route: GeneratorND keeps its tensors in lists, and ``grid_std[0] = ...`` keeps the list -- its elements as well)
        self._quick_l = tuple((v, tuple(v)) for v in tensors if isinstance(v, (list, tuple))) if self.table is not None else ()
        tensors += [e for _, elements in self._quick_l for e in elements]
        self._quick_t = tuple((v, v._version) for v in tensors if isinstance(v, torch.Tensor))
        self._quick_f = type(g).get_examples
        # plan route: the `generators` tuple of every wrapper in the tree and every leaf under the name tuple of its kind
        # (DATA leaves: `examples` / `xs`), by identity; their lists and tensors join the element / version checks above
        self._quick_tree = ()
        if self.plan is not None:
            watched = [(w, _LIVE_INDEX if isinstance(w, (ResampleGenerator, BatchGenerator)) else
                        _LIVE_STAGE if isinstance(w, (TransformGenerator, FilterGenerator)) else ("generators",))
                       for w in self.plan.wrappers] + [(f.gen, f.live) for f in self.plan.leaves]
            tree = tuple((vars(o), n, vars(o).get(n), type(o), type(o).get_examples) for o, names in watched for n in names if n in vars(o))
            values = [e[2] for e in tree]
            lists = tuple((v, tuple(v)) for v in values if isinstance(v, (list, tuple)))
            values += [e for _, elements in lists for e in elements]
            self._quick_tree, self._quick_l = tree, self._quick_l + lists
            self._quick_t += tuple((v, v._version) for v in values if isinstance(v, torch.Tensor))

    def _unchanged(self, quick=None):
        g = self.generator
        d = g.__dict__
        for n, v in (self._quick if quick is None else quick):
            if d.get(n) is not v:
                return False
        for od, n, v, cls, fn in self._quick_tree:
            if od.get(n) is not v or cls.get_examples is not fn:
                return False
        for v, elements in self._quick_l:
            if len(v) != len(elements) or any(x is not y for x, y in zip(v, elements)):
                return False
        for t, ver in self._quick_t:
            if t._version != ver:
                return False
        return type(g).get_examples is self._quick_f

    def _wrapped_changed(self):
        """The wrapped generator no longer draws what the descriptor says.  Noise widths alone: a new descriptor.  Anything else (grid
        tensors replaced / edited in place, another getter, another size): the wrapped generator's own host draw from now on,
        copied into the resident block -- what the reference would train on."""
        g = self.generator
        if self.plan is not None and self.plan.stages:
            return self._stages_changed()
        if self.plan is not None:                # (no partial rebuilds on this route: any change anywhere in the tree)
            self._to_host()
            return self._restamp()
        if self.table is not None:
            return self._table_changed()
        try:
            new = self.describe(g)
            same_shape = new.kind == self.desc.kind and new.d == self.desc.d and list(new.n) == list(self.desc.n) and g.size == self.size
        except Exception:       # noqa: BLE001
            new, same_shape = None, False
        numbers_only = same_shape and all(
            a == b for n, a, b in zip(("type",) + self._live_names, self._stamp, live_stamp(g, self._live_names))
            if not n.startswith("noise"))
        if numbers_only:
            self.desc = new
            self.prefetched = None              # (a batch drawn ahead by a tail kernel used the old widths)
        else:
            self._to_host()
        self._restamp()

    MAX_STAGE_REBUILDS = 3

    def _stages_changed(self):
        """A plan with stages whose tree changed (``trans`` / ``filter_fn`` replaced, another wrapped generator) or whose callables
        read Python state that moved (a captured radius: ``PlanSpec.watch``): plan, trace and build again -- one hipcc run unless the
        generated source was built before -- as long as the block still fits; after MAX_STAGE_REBUILDS of them, or when the new tree
        cannot be drawn on the device, the wrapped generator's own host draw from now on."""
        self._rebuilds = getattr(self, "_rebuilds", 0) + 1
        plan = None
        if self._rebuilds <= self.MAX_STAGE_REBUILDS:
            try:
                plan = plan_spec(self.generator, _redraw=True)
            except ValueError:
                plan = None
        if plan is None or not plan.stages or plan.size != self.plan.size or plan.d_out != self._rows_out \
                or max(plan.d, plan.d_out) != self.block.shape[0]:
            self._to_host()
        else:
            self._set_plan(plan)
        self._restamp()

    def _to_host(self):
        self._on_host, self.prefetch, self.prefetched = True, False, None
        warnings.warn("neurodiffeq_amd: a generator wrapped by DeviceGenerator was changed in a way the device sampler cannot "
                      "follow (grid tensors / getter / size); its own host draw is used from now on (the reference's numbers, "
                      "uploaded every epoch).", RuntimeWarning)

    def _table_changed(self):
        """Table route: a new ``noise_std`` number on a Generator1D rebuilds the width table; anything else (node or width tensors
        replaced / edited, another getter, size or method): the wrapped generator's own host draw from now on."""
        g = self.generator
        rest_same = self._unchanged(tuple(p for p in self._quick if p[0] != "noise_std"))
        spec = None
        if rest_same and type(g) is Generator1D and isinstance(g.noise_std, (int, float)):
            try:
                spec = table_spec(g)
            except ValueError:
                spec = None
        if spec is not None and (spec.n, spec.law) == (self.table.n, self.table.law):
            self._set_table(spec)
        else:
            self._to_host()
        self._restamp()

    def _host_examples(self):
        ex = self.generator.get_examples()
        ex = [ex] if isinstance(ex, torch.Tensor) else list(ex)
        if len(ex) != self._rows_out or ex[0].numel() != self._views_all[0][0].shape[0]:
            self.size = ex[0].numel()
            return [e.detach().reshape(-1, 1).to(self.device, self.dtype) for e in ex]      # (another shape altogether: plain tensors)
        block, views = self._out_blocks[0], self._views_all[0]
        for i, e in enumerate(ex):
            block[i, :self.size].copy_(e.detach().reshape(-1))
        self.block, self._views = self.blocks[0], views
        self.draw += 1
        return views

    def _get_examples(self):
        if self._on_host:
            return self._host_examples()
        if not self._unchanged() or (self.plan is not None and self.plan.watch is not None and self.plan.watch.dirty()):
            self._wrapped_changed()
            if self._on_host:
                return self._host_examples()
        if self.plan is not None and self._map is not None:
            return self._staged_examples()
        block = self.block_of(self.draw)
        if self.prefetched == self.draw:          # a tail kernel has drawn this batch already
            self.prefetched = None
        else:
            stream = ctypes.c_void_p(_raw_stream(self.device.index))       # (torch.cuda.current_stream(): ~10 us per call)
            sample = self._L.ndq_sample if self.table is None else self._L.ndq_sample_table
            if self.plan is not None:
                sample = self._L.ndq_sample_plan
            if self.plan is not None and self._index is not None:
                sample = self._L.ndq_sample_plan_indexed
                rc = sample(ctypes.byref(self.desc), ctypes.byref(self._index), self.seed, self.draw, self.stream_id, block.data_ptr(),
                            block.shape[1], stream)
            else:
                rc = sample(ctypes.byref(self.desc), self.seed, self.draw, self.stream_id, block.data_ptr(), block.shape[1], stream)
            if rc != 0:
                from . import _lib
                raise _lib.NdqError(f"{sample.__name__} failed with code {rc}")
            self.launches += 1
        slot = (self.draw & 1) if self.prefetch else 0
        if self.dtype != torch.float32:
            self._out_blocks[slot].copy_(block)          # (stream-ordered behind the draw)
        views = self._views_all[slot]
        self.block, self._views = block, views
        self.draw += 1
        return views

    def _staged_examples(self):
        """One draw of a plan with stages through its generated module (csrc/ndq_sample_map.h).  Transform only: ONE launch into
        the fixed views.  With a filter: three stream-ordered launches (count, scan, compact), then the kept count is read back --
        one 4-byte device-to-host copy on the compute stream per draw, the only host synchronisation of this route: a batch's
        length is part of its tensors' shape.  The views of that draw are built here; ``size`` -- this generator's and the
        outermost FilterGenerator's -- follows the kept count (the reference's ``update_size=True``)."""
        block = self.blocks[0]
        stream = ctypes.c_void_p(_raw_stream(self.device.index))
        work = self._work
        rc = self._map.launch(ctypes.addressof(self.desc), ctypes.addressof(self._index) if self._index is not None else None,
                              self.seed, self.draw, self.stream_id, block.data_ptr(), block.shape[1], block.shape[0],
                              work.data_ptr() if work is not None else None, work.numel() if work is not None else 0, stream)
        if rc != 0:
            from . import _lib
            raise _lib.NdqError(f"ndq_map_launch failed with code {rc}")
        self.launches += 3 if work is not None else 1
        if self.dtype != torch.float32:
            self._out_blocks[0].copy_(block)             # (stream-ordered behind the draw)
        views = self._views_all[0]
        if work is not None:
            kept = int(work[0].item())
            self.readbacks += 1
            if kept != views[0].shape[0]:
                views = self._filtered_views(kept)
            self.size = kept
            for node in reversed(self.plan.stage_nodes):
                if isinstance(node, FilterGenerator):
                    node.size = kept
                    break
        self.block, self._views = block, views
        self.draw += 1
        return views

    def _filtered_views(self, kept):
        """The (kept, 1) views of a filtered draw; they take the place of the previous list here and in the registry of
        :func:`device_source`."""
        _forget_sources(self._source_ids)
        self._source_ids.clear()
        out = self._out_blocks[0]
        views = [out[i, :kept].reshape(-1, 1) for i in range(self._rows_out)]
        self._views_all = [views]
        self._register(views)
        return views

    def _internal_vars(self):
        d = super()._internal_vars()
        d.update(generator=self.generator, seed=self.seed, stream_id=self.stream_id)
        return d


# ------------------------------------------------------------------------------------------------ default-device sampling
# The reference draws on torch's DEFAULT device (generators.py:152,158,264-265: torch.linspace / torch.normal without a
# device argument); its import default is cuda where one exists (neurodiffeq/__init__.py:22), and there the noise comes from
# the GPU's Philox stream -- itself not the CPU generator's numbers.  Same rule here: a solver built while torch's default
# device is cuda draws the NOISE of Generator1D / 2D / 3D / Spherical on the MI355X (DeviceGenerator: Philox4x32-10, seeded
# from torch's cuda generator (one draw per wrapped generator), so torch.manual_seed still fixes the run; every rank draws the SAME batch and takes its
# shard); with a CPU default device nothing changes: host draws, bit for bit the reference's CPU numbers.  Index sampling
# (randperm / randint: ResampleGenerator, BatchGenerator, latin-hypercube, the spherical signs of the host path) and every
# wrapper generator stay on the CPU generator bit for bit in both cases.  ``Generator2D(..., bit_exact_cpu=True)`` or
# ``set_default_sampling("cpu")`` keep a generator on the host under a cuda default device as well.
_SAMPLING = {"mode": os.environ.get("NDQ_SAMPLING", "auto")}


def set_default_sampling(mode):
    """"auto" (default): follow torch's default device;  "cpu": always sample on the host (the reference's CPU numbers bit
    for bit, 17x slower per step at the headline size);  "device": device-side noise whenever an MI355X is visible."""
    if mode not in ("auto", "cpu", "device"):
        raise ValueError(f"mode must be 'auto', 'cpu' or 'device', got {mode!r}")
    _SAMPLING["mode"] = mode


def _seed_from_torch_cuda_rng():
    dev = torch.device("cuda", torch.cuda.current_device())
    return int(torch.randint(0, 1 << 62, (1,), dtype=torch.int64, device=dev).item())


def on_default_device(gen):
    """``gen`` itself, or -- when noise is to be drawn on the device (see above) and the kernel knows the distribution -- a
    DeviceGenerator around it."""
    mode = _SAMPLING["mode"]
    if mode == "cpu" or gen is None or getattr(gen, "bit_exact_cpu", False) or not torch.cuda.is_available():
        return gen
    if type(gen) not in (Generator1D, Generator2D, Generator3D, GeneratorSpherical):
        return gen
    if mode == "auto" and torch.get_default_device().type != "cuda":
        return gen
    dtype = torch.get_default_dtype()
    if dtype not in (torch.float32, torch.float64):
        return gen
    if not (type(gen) is GeneratorSpherical or gen.method == "uniform" or gen.method == "equally-spaced-noisy"):
        return gen                 # static grids are uploaded once and read in place; other laws: host
    try:
        # prefetch: on the single-launch native path the next batch is drawn by spare workgroups of the epoch's own sums /
        # tail launch (no sampler launch); the handed-out tensors keep an epoch's points until the end of the next epoch
        # (an fp64 default dtype -- the reference's import default is cuda + float64 -- gets the fp32 draws as doubles)
        # the Philox key is (seed, draw number, stream id): every wrapped generator needs a seed of its OWN, or two generators
        # of one law -- the default train / valid pair of SolverSpherical, every solver of a process -- would replay the same
        # points.  The reference's generators all consume the one global RNG of the default device; here each
        # takes its seed from that RNG once, at construction: torch.manual_seed still fixes the run, data-parallel ranks
        # seeded alike still draw the same batches, and no two generators share a stream.
        return DeviceGenerator(gen, seed=_seed_from_torch_cuda_rng(), stream_id=0, prefetch=True, dtype=dtype)
    except ValueError:
        return gen
