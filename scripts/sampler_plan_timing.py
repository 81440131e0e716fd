#!/usr/bin/env python
"""One fresh batch of a COMPOSED generator -- 65 536 points -- four ways, for two generators:
  interior+edge  Generator2D((240, 240)) + Generator1D(7936) * Generator1D(7936)        (concat of a leaf and an ensemble)
  mesh           Generator1D(256, 'equally-spaced-noisy') ^ Generator1D(256, 0.1, 10, 'log-spaced-noisy')
  (a) plan_kernel    ndq_sample_plan launched back to back on one stream (HIP events around DRAWS launches)
  (b) device_draw    DeviceGenerator.get_examples() on the plan route: the same launch plus its host side, HIP events
  (c) host_draw      the wrapped generator's get_examples() on the host, the columns copied into a pinned [d][ld] block and one
                     H2D copy (host clock around a loop that ends in a synchronise)
  (d) leafwise_draw  the composition as it had to be done before: one DeviceGenerator per leaf, then torch.cat / torch.meshgrid
                     into a [d][ld] block (HIP events)
Medians over REPS windows, after a warm-up.  Prints one JSON line per generator.
usage: scripts/sampler_plan_timing.py [DRAWS] > sampler_plan_timing.json"""
import ctypes
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neurodiffeq_amd.generators import DeviceGenerator, Generator1D, Generator2D, plan_leaf_seed  # noqa: E402

DRAWS = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
REPS = 7
sync = torch.cuda.synchronize


def events_us(body, k):
    out = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        sync()
        a.record()
        for i in range(k):
            body(i)
        b.record()
        sync()
        out.append(a.elapsed_time(b) * 1e3 / k)
    return out


def wall_us(body, k):
    out = []
    for _ in range(REPS):
        sync()
        t0 = time.perf_counter()
        for i in range(k):
            body(i)
        sync()
        out.append((time.perf_counter() - t0) * 1e6 / k)
    return out


def interior_edge():
    make = lambda: Generator2D((240, 240)) + Generator1D(7936) * Generator1D(7936)
    g = make()
    leaves = [DeviceGenerator(leaf, seed=plan_leaf_seed(1, l)) for l, leaf in
              enumerate((g.generators[0],) + tuple(g.generators[1].generators))]
    blk = torch.zeros(2, 65536, device="cuda")

    def leafwise(_):
        (x, y), (a,), (b,) = (dg.get_examples() for dg in leaves)
        torch.cat((x.reshape(-1), a.reshape(-1)), out=blk[0])
        torch.cat((y.reshape(-1), b.reshape(-1)), out=blk[1])
    return make, leafwise


def mesh():
    make = lambda: Generator1D(256, 0.0, 1.0, "equally-spaced-noisy") ^ Generator1D(256, 0.1, 10.0, "log-spaced-noisy")
    g = make()
    leaves = [DeviceGenerator(leaf, seed=plan_leaf_seed(1, l)) for l, leaf in enumerate(g.generators)]
    blk = torch.zeros(2, 65536, device="cuda")

    def leafwise(_):
        (t,), (k,) = (dg.get_examples() for dg in leaves)
        mt, mk = torch.meshgrid(t.reshape(-1), k.reshape(-1), indexing="ij")
        blk[0].view(256, 256).copy_(mt)
        blk[1].view(256, 256).copy_(mk)
    return make, leafwise


for name, case in (("interior+edge", interior_edge), ("mesh", mesh)):
    torch.manual_seed(0)
    make, leafwise = case()
    host = make()
    dg = DeviceGenerator(make(), seed=1)
    n, d, ld = dg.size, dg.desc.d, dg.block.shape[1]
    assert (n, d) == (65536, 2) and dg.plan is not None
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def kernel(i):
        rc = dg._L.ndq_sample_plan(ctypes.byref(dg.desc), dg.seed, i, 0, dg.block.data_ptr(), ld, stream)
        assert rc == 0, rc

    pinned = torch.zeros(d, ld, dtype=torch.float32).pin_memory()
    dev = torch.zeros(d, ld, dtype=torch.float32, device="cuda")

    def host_draw(_):
        for row, col in zip(pinned, host.get_examples()):
            row[:n].copy_(col.detach())
        dev.copy_(pinned, non_blocking=True)

    for i in range(200):                                   # warm-up of every timed path
        kernel(i)
        dg.get_examples()
        leafwise(i)
    for i in range(20):
        host_draw(i)
    res = {"generator": name, "points": n, "rows": d, "leaves": len(dg.plan.leaves), "draws_per_window": DRAWS, "windows": REPS,
           "bytes_written_per_draw": 4 * d * n}
    for what, us in (("plan_kernel", events_us(kernel, DRAWS)), ("device_draw", events_us(lambda i: dg.get_examples(), DRAWS)),
                     ("host_draw", wall_us(host_draw, max(DRAWS // 10, 100))), ("leafwise_draw", events_us(leafwise, DRAWS))):
        res[what + "_us"] = {"median": round(statistics.median(us), 3), "min": round(min(us), 3), "max": round(max(us), 3)}
    res["host_over_device"] = round(res["host_draw_us"]["median"] / res["device_draw_us"]["median"], 1)
    res["leafwise_over_device"] = round(res["leafwise_draw_us"]["median"] / res["device_draw_us"]["median"], 2)
    print(json.dumps(res), flush=True)
