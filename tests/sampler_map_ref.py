"""TEST INFRASTRUCTURE ONLY -- numpy restatement of the map / filter route of the device sampler (neurodiffeq_amd/csrc/ndq_sample_map.h,
codegen.SamplerMapProgram): the traced DAG of the stages interpreted in np.float32, one rounding per node, in node order, on the
rows the plan restatements produce (tests/sampler_plan_ref.py, tests/sampler_index_ref.py), then ``rows[:, keep]``; and the
count -> scan -> compact scheme of the filter kernels restated index by index."""
import numpy as np

from tests import sampler_index_ref as X
from tests import sampler_plan_ref as R

F = np.float32
_UNARY = {"neg": np.negative, "sin": np.sin, "cos": np.cos, "tan": np.tan, "exp": np.exp, "log": np.log, "tanh": np.tanh,
          "sqrt": np.sqrt, "abs": np.abs, "sinh": np.sinh, "cosh": np.cosh, "sign": np.sign, "log1p": np.log1p, "expm1": np.expm1,
          "atan": np.arctan, "floor": np.floor, "ceil": np.ceil, "round": np.rint, "trunc": np.trunc, "detach": lambda a: a,
          "sigmoid": lambda a: F(1.0) / (F(1.0) + np.exp(-a)), "recip": lambda a: F(1.0) / a}
_BINARY = {"add": np.add, "sub": np.subtract, "mul": np.multiply, "div": np.divide, "atan2": np.arctan2}


def eval_stages(trace, rows):
    """trace: (Graph, out nodes, keep node | None) of generators.trace_stages; rows [d][n] fp32 -> (out [d_out][n] fp32, keep [n])."""
    g, outs, keep = trace
    rows = np.asarray(rows, dtype=F)
    n = rows.shape[1]
    val = {}
    with np.errstate(all="ignore"):
        for i in g.reachable(list(outs) + ([keep] if keep is not None else [])):
            node = g.nodes[i]
            op = node[0]
            if op == "const":
                v = np.full(n, F(node[1]), dtype=F)
            elif op == "coord":
                v = rows[node[1]]
            elif op in _BINARY:
                v = _BINARY[op](val[node[1]], val[node[2]])
            elif op in ("gt", "ge"):
                v = ((val[node[1]] > val[node[2]]) if op == "gt" else (val[node[1]] >= val[node[2]])).astype(F)
            elif op == "where":
                v = np.where(val[node[1]] != 0, val[node[2]], val[node[3]])
            elif op == "powi":
                a = val[node[1]]
                if node[2] <= 8:                              # the emitted product (a*a*...*a), left to right
                    v = a
                    for _ in range(node[2] - 1):
                        v = (v * a).astype(F)
                else:
                    v = np.power(a, F(node[2]))
            elif op == "powc":
                v = np.power(val[node[1]], F(node[2]))
            else:
                v = _UNARY[op](val[node[1]])
            val[i] = np.asarray(v, dtype=F)
    out = np.stack([val[i] for i in outs])
    return out, (val[keep] != 0 if keep is not None else np.ones(n, dtype=bool))


def plan_rows(plan, seed, draw, stream_id=0):
    """The rows of the plan itself (its Resample / Batch root included), before any stage."""
    return X.sample_plan_indexed(plan, seed, draw, stream_id) if plan.index is not None else R.sample_plan(plan, seed, draw, stream_id)


def sample_plan_map(plan, seed, draw, stream_id=0):
    """[d_out][kept] fp32: what the generated module hands out for draw ``draw`` of a ``generators.PlanSpec`` with stages."""
    out, keep = eval_stages(plan.trace, plan_rows(plan, seed, draw, stream_id))
    return out[:, keep]


def compact(rows, keep):
    """count_kernel -> scan_kernel -> compact_kernel, index by index: workgroups of 256 points in four waves of 64; the kept count
    of every workgroup; exclusive offsets by chunks of 256 workgroups with a running carry; a kept point lands at
    offset[workgroup] + (kept lanes below it in its wave) + (kept counts of the lower waves).  -> (rows [d][kept], kept)."""
    rows, keep = np.asarray(rows), np.asarray(keep, dtype=bool)
    n = keep.size
    nb = (n + 255) // 256
    padded = np.zeros(nb * 256, dtype=bool)
    padded[:n] = keep
    waves = padded.reshape(nb, 4, 64)
    wave_counts = waves.sum(axis=2)                           # [nb][4]
    counts = (wave_counts[:, 0] + wave_counts[:, 1]) + (wave_counts[:, 2] + wave_counts[:, 3])
    offsets, carry = np.zeros(nb, dtype=np.int64), 0
    for base in range(0, nb, 256):                            # scan_kernel: one chunk of 256 counts at a time
        chunk = counts[base:base + 256]
        incl = np.cumsum(chunk)
        offsets[base:base + 256] = carry + incl - chunk
        carry += int(incl[-1])
    lane_rank = np.cumsum(waves, axis=2) - waves              # kept lanes below this one in the wave
    lower = np.cumsum(wave_counts, axis=1) - wave_counts      # kept counts of the lower waves
    pos = (offsets[:, None, None] + lower[:, :, None] + lane_rank).reshape(-1)[:n]
    out = np.zeros((rows.shape[0], carry), dtype=rows.dtype)
    out[:, pos[keep]] = rows[:, keep]
    return out, carry
