#!/usr/bin/env python
"""One fresh batch of a GeneratorND -- 65 536 points, three axes ('equally-spaced', 'log-spaced', 'chebyshev2') -- three ways:
  table_kernel   ndq_sample_table launched back to back on one stream (HIP events around DRAWS launches)
  device_draw    DeviceGenerator.get_examples(): the same launch plus its host side (change stamp, views), HIP events
  host_draw      what a solver pays without it: the wrapped generator's get_examples() on the host, the three columns copied into a
                 pinned [3][ld] block and one H2D copy (host clock around a loop that ends in a synchronise)
Medians over REPS windows, after a warm-up.  Prints one JSON line.
usage: scripts/sampler_table_timing.py [DRAWS] > sampler_table_timing.json"""
import ctypes
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neurodiffeq_amd.generators import DeviceGenerator, GeneratorND  # noqa: E402

DRAWS = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
REPS = 7
torch.manual_seed(0)
make = lambda: GeneratorND((64, 32, 32), (0.0, 0.1, -1.0), (1.0, 10.0, 1.0), ("equally-spaced", "log-spaced", "chebyshev2"))
host = make()
dg = DeviceGenerator(make(), seed=1)
n, d, ld = dg.size, dg.desc.d, dg.block.shape[1]
assert (n, d) == (65536, 3)
sync = torch.cuda.synchronize
stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


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


def kernel(i):
    rc = dg._L.ndq_sample_table(ctypes.byref(dg.desc), dg.seed, i, 0, dg.block.data_ptr(), ld, stream)
    assert rc == 0, rc


pinned = torch.zeros(d, ld, dtype=torch.float32).pin_memory()
dev = torch.zeros(d, ld, dtype=torch.float32, device="cuda")


def host_draw(_):
    for row, col in zip(pinned, host.get_examples()):
        row[:n].copy_(col.detach())
    dev.copy_(pinned, non_blocking=True)


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


for i in range(200):                                   # warm-up of every timed path
    kernel(i)
    dg.get_examples()
for i in range(20):
    host_draw(i)
res = {"points": n, "axes": d, "draws_per_window": DRAWS, "windows": REPS, "bytes_written_per_draw": 4 * d * n}
for name, us in (("table_kernel", events_us(kernel, DRAWS)), ("device_draw", events_us(lambda i: dg.get_examples(), DRAWS)),
                 ("host_draw", wall_us(host_draw, max(DRAWS // 10, 100)))):
    res[name + "_us"] = {"median": round(statistics.median(us), 3), "min": round(min(us), 3), "max": round(max(us), 3)}
res["table_kernel_GB_per_s"] = round(res["bytes_written_per_draw"] / res["table_kernel_us"]["median"] * 1e-3, 1)
res["host_over_device"] = round(res["host_draw_us"]["median"] / res["device_draw_us"]["median"], 1)
print(json.dumps(res))
