#!/usr/bin/env python
"""One mini-batch of BatchGenerator(ResampleGenerator(g), bs), g = Generator2D((256, 256)) (noisy, 65 536 points), four ways, for
bs = 65 536 and bs = 4 096:
  (a) index_kernel   ndq_sample_plan_indexed launched back to back on one stream (HIP events around DRAWS launches)
  (b) device_draw    DeviceGenerator(BatchGenerator(ResampleGenerator(g), bs)).get_examples(): the same launch plus its host side
  (c) host_draw      the wrapped generator's get_examples() on the host (randperm, the inner draw and the gather once per 65 536 / bs
                     batches, the cache slicing every batch), the columns copied into a pinned [d][ld] block and one H2D copy
                     (host clock around a loop that ends in a synchronise): the route of a mini-batched solver without this kernel
  (d) plain_kernel   ndq_sample_plan of g alone (all 65 536 points, no index), launched back to back: what the window and the
                     permutation add to a draw of bs = 65 536
Medians over REPS windows, after a warm-up.  Prints one JSON line per batch size.
usage: scripts/sampler_index_timing.py [DRAWS] > sampler_index_timing.json"""
import ctypes
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neurodiffeq_amd.generators import BatchGenerator, DeviceGenerator, Generator2D, ResampleGenerator  # noqa: E402

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


for bs in (65536, 4096):
    torch.manual_seed(0)
    make = lambda: BatchGenerator(ResampleGenerator(Generator2D((256, 256))), bs)
    host = make()
    dg = DeviceGenerator(make(), seed=1)
    n, d, ld = dg.size, dg.desc.d, dg.block.shape[1]
    assert (n, d) == (bs, 2) and dg.plan.index is not None and (dg.plan.index.mode, dg.plan.index.n) == ("permute", 65536)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    full = torch.zeros(d, 65536, dtype=torch.float32, device="cuda")

    def kernel(i):
        rc = dg._L.ndq_sample_plan_indexed(ctypes.byref(dg.desc), ctypes.byref(dg._index), dg.seed, i, 0, dg.block.data_ptr(), ld, stream)
        assert rc == 0, rc

    def plain(i):
        rc = dg._L.ndq_sample_plan(ctypes.byref(dg.desc), dg.seed, i, 0, full.data_ptr(), 65536, stream)
        assert rc == 0, rc

    pinned = torch.zeros(d, ld, dtype=torch.float32).pin_memory()
    dev = torch.zeros(d, ld, dtype=torch.float32, device="cuda")

    def host_draw(_):
        for row, col in zip(pinned, host.get_examples()):
            row[:n].copy_(col.detach())
        dev.copy_(pinned, non_blocking=True)

    for i in range(200):                                   # warm-up of every timed path
        kernel(i)
        plain(i)
        dg.get_examples()
    for i in range(32):
        host_draw(i)
    res = {"batch": bs, "plan_points": 65536, "rows": d, "rounds": 2 * 16 + 8, "draws_per_window": DRAWS, "windows": REPS,
           "bytes_written_per_draw": 4 * d * n}
    for what, us in (("index_kernel", events_us(kernel, DRAWS)), ("device_draw", events_us(lambda i: dg.get_examples(), DRAWS)),
                     ("host_draw", wall_us(host_draw, max(DRAWS // 10, 64))), ("plain_kernel", events_us(plain, DRAWS))):
        res[what + "_us"] = {"median": round(statistics.median(us), 3), "min": round(min(us), 3), "max": round(max(us), 3)}
    res["host_over_device"] = round(res["host_draw_us"]["median"] / res["device_draw_us"]["median"], 1)
    res["index_over_plain_kernel"] = round(res["index_kernel_us"]["median"] / res["plain_kernel_us"]["median"], 2)
    print(json.dumps(res), flush=True)
