#!/usr/bin/env python
"""One training epoch (Solver.run_train_epoch, one batch of 65 536 resident points) of the two systems the reference goldens
wm1 / wm2 pin, on both routes:
  wm1   Lotka-Volterra, two FCNN(1, 1, (128,))                  65 536 points of [0, 1]
  wm2   three coupled fields, three FCNN(2, 1, (128,))          256 x 256 points of the unit square
  closure    the "wide_multi" single-launch closure + one sums / tail launch (csrc/ndq_wide.h: wide_multi_closure_kernel)
  pipeline   the three-kernel pipeline these systems ran on before that mode existed (NDQ_NO_WIDE_MULTI_FUSE=1: the same
             kernels and the same host code as a checkout without the mode; on such a checkout both legs report it)
Every (system, route) leg is a child process of its own under `timeout`; the first leg that fails ends the run.  Per leg: WARMUP
epochs, then WINDOWS windows of STEPS epochs, host clock around a loop that ends in a synchronise; the median window counts.
Prints one JSON line per leg and a last line with the ratios.
usage: scripts/wide_multi_timing.py [STEPS] > wide_multi_timing.jsonl"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARMUP, WINDOWS = 30, 7
LEG_SECONDS = 240


def leg(name, route, steps):
    if route == "pipeline":
        os.environ["NDQ_NO_WIDE_MULTI_FUSE"] = "1"
    sys.path.insert(0, ROOT)
    import torch
    from neurodiffeq_amd.generators import Generator1D, Generator2D, ResidentBatchGenerator, SamplerGenerator
    from neurodiffeq_amd.solvers import Solver1D, Solver2D
    from tests import wide_multi_problems as WM
    system, width = WM.GOLDEN[name]
    torch.manual_seed(0)
    nets, conds, eqs, d_in = WM.make(system, width)
    if d_in == 1:
        gen = Generator1D(65536, WM.T_MIN, WM.T_MAX, "equally-spaced-noisy")
        solver = Solver1D(eqs, conds, t_min=WM.T_MIN, t_max=WM.T_MAX, nets=nets, train_generator=gen, valid_generator=gen, n_batches_valid=0)
    else:
        gen = Generator2D((256, 256), (0, 0), (1, 1), "equally-spaced-noisy")
        solver = Solver2D(eqs, conds, xy_min=(0, 0), xy_max=(1, 1), nets=nets, train_generator=gen, valid_generator=gen, n_batches_valid=0)
    solver.fused = "require"
    torch.manual_seed(1)
    solver.generator["train"] = SamplerGenerator(ResidentBatchGenerator.presample(gen, 4, "cuda"))
    for _ in range(WARMUP):
        solver.run_train_epoch()
    torch.cuda.synchronize()
    fs = solver._fused_sys
    assert solver.fused_active
    us = []
    for _ in range(WINDOWS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            solver.run_train_epoch()
        torch.cuda.synchronize()
        us.append((time.perf_counter() - t0) * 1e6 / steps)
    hist = solver.metrics_history["train_loss"]
    print(json.dumps({"system": name, "route": route, "points": 65536, "networks": len(nets), "width": width,
                      "single_launch": fs.fusedk is not None,
                      "launches_per_step": fs.launches_per_step(), "steps_per_window": steps, "windows": WINDOWS,
                      "us_per_epoch": {"median": round(statistics.median(us), 2), "min": round(min(us), 2), "max": round(max(us), 2)},
                      "loss_first": hist[0], "loss_last": hist[-1], "device": torch.cuda.get_device_name(0)}), flush=True)


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    results = {}
    for name in ("wm1", "wm2"):
        for route in ("pipeline", "closure"):
            proc = subprocess.run(["timeout", "-k", "10", str(LEG_SECONDS), sys.executable, os.path.abspath(__file__), "--leg", name,
                                   route, str(steps)], capture_output=True, text=True)
            sys.stderr.write(proc.stderr[-2000:])
            if proc.returncode != 0:
                print(json.dumps({"system": name, "route": route, "failed": proc.returncode}), flush=True)
                return proc.returncode
            line = proc.stdout.strip().splitlines()[-1]
            print(line, flush=True)
            results[(name, route)] = json.loads(line)["us_per_epoch"]["median"]
    print(json.dumps({"pipeline_over_closure": {name: round(results[(name, "pipeline")] / results[(name, "closure")], 3)
                                                for name in ("wm1", "wm2")}}), flush=True)
    return 0


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--leg":
        leg(sys.argv[2], sys.argv[3], int(sys.argv[4]))
    else:
        sys.exit(main())
