"""TEST INFRASTRUCTURE ONLY -- numpy restatement of the plan sampler (neurodiffeq_amd/csrc/ndq_sample.h:
sample_plan_kernel; include/ndq.h: ndq_sample_plan): the leaf draws of oracle/philox_ref.py and tests/sampler_table_ref.py
under the derived leaf seeds, composed with np.concatenate / side by side / np.meshgrid(indexing="ij").

Leaf l of a ``generators.PlanSpec`` draws under ``leaf_seed(seed, l)`` with the draw number and stream id of the whole
draw and its leaf-LOCAL point index as Philox counter word 0 -- i.e. exactly what the single-leaf restatements compute."""
import numpy as np

from oracle import philox_ref as P
from tests import sampler_table_ref as T

UNIFORM, GRID, SPHERICAL = 0, 1, 2          # NDQ_SAMPLE_* of include/ndq.h
GOLDEN = 0x9E3779B97F4A7C15
F = np.float32


def leaf_seed(seed, l):
    return (seed + l * GOLDEN) % 2 ** 64


def leaf_draw(leaf, seed, draw, stream_id=0):
    """[rows][size] fp32: what the leaf alone draws under ``seed`` (a ``generators.PlanLeaf``)."""
    if leaf.kind == "data":
        return np.stack(leaf.data)
    if leaf.kind == "table":
        return T.sample_table(leaf.table, seed, draw, stream_id)
    s = leaf.desc
    d = s.d
    if s.kind == UNIFORM:
        return P.sample_uniform(s.n[0], list(s.lo)[:d], list(s.hi)[:d], seed, draw, stream_id)
    if s.kind == GRID:
        return P.sample_grid(list(s.n)[:d], list(s.lo)[:d], list(s.hi)[:d], list(s.noise_std)[:d], seed, draw, stream_id)
    return P.sample_spherical(s.n[0], s.lo[0], s.hi[0], s.radial, seed, draw, stream_id)


def leaf_draws(plan, seed, draw, stream_id=0):
    return [leaf_draw(f, leaf_seed(seed, l), draw, stream_id) for l, f in enumerate(plan.leaves)]


def compose(plan, per_leaf):
    """per_leaf[l]: [rows_l][size_l] -> [d][plan.size], composed as the reference's wrapper generators compose their
    sub-generators' draws: Concat = concatenate along the points, Ensemble = rows side by side, Mesh = ij-meshgrid of the
    one-row factors, flattened (last factor fastest)."""
    out = []
    for mode, first, count, _offset, size in plan.segments:
        own = [np.asarray(per_leaf[l]) for l in range(first, first + count)]
        if mode == "mesh":
            rows = [m.reshape(-1) for m in np.meshgrid(*[x[0] for x in own], indexing="ij")]
        else:
            rows = [r for x in own for r in x]
        seg = np.stack(rows)
        assert seg.shape == (plan.d, size), (seg.shape, plan.d, size)
        out.append(seg)
    return np.concatenate(out, axis=1)


def sample_plan(plan, seed, draw, stream_id=0):
    """``plan``: a ``generators.PlanSpec`` -> [d][size] fp32, what ndq_sample_plan writes."""
    return compose(plan, leaf_draws(plan, seed, draw, stream_id)).astype(F)


def leaf_exact_rows(leaf):
    """Per row of the leaf: True when it carries no jitter (exact grid / exact nodes / DATA) -- the kernel's numbers are then the
    host tensors' bit for bit."""
    if leaf.kind == "data":
        return [True] * leaf.rows
    if leaf.kind == "table":
        return [leaf.table.law[c] == T.NORMAL and leaf.table.std[c] is None for c in range(leaf.rows)]
    return [leaf.desc.kind == GRID and leaf.desc.noise_std[c] == 0.0 for c in range(leaf.rows)]
