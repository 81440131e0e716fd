#!/usr/bin/env python
"""One training epoch (Solver.run_train_epoch, one batch of resident points) of fp64 systems behind a closure kernel, on this
tree's two routes for the end of the epoch:
  separate   the default: loss sum, then per network a gradient sum and an epoch tail (2 + 2 K launches)
  fused      NDQ_F64_FUSED_TAIL=1: ONE sums + tail launch in double behind the closure launch (2 launches)
Systems: C1 in double (two sin 32 x 32 networks, tests/configs.py) at 1 024 and 65 536 points, C2 in double (one network) at
65 536 points.  ALTERNATING pairs -- separate, fused, separate, fused, ... -- so that drift of the machine shows as spread
between pairs instead of as a difference between the routes.  Every leg is a child process of its own under `timeout`; the
first leg that fails ends the run.  Per leg: WARMUP epochs, then WINDOWS windows of STEPS epochs, host clock around a loop that
ends in a synchronise; the median window counts.  Prints one JSON line per leg and a last line with the per-pair ratios.
usage: scripts/f64_tail_timing.py [--pairs N] [--steps K] > f64_tail_timing.jsonl"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARMUP, WINDOWS = 30, 5
LEG_SECONDS = 240
CASES = (("c1", 1024), ("c1", 65536), ("c2", 65536))


def leg(route, name, points, steps):
    if route == "fused":
        os.environ["NDQ_F64_FUSED_TAIL"] = "1"
    else:
        os.environ.pop("NDQ_F64_FUSED_TAIL", None)
    sys.path.insert(0, ROOT)
    import torch
    from neurodiffeq_amd.generators import ResidentBatchGenerator, SamplerGenerator
    from tests import configs
    torch.manual_seed(0)
    solver, cfg = configs.make_solver(name, points if name == "c1" else int(round(points ** 0.5)))
    for net in cfg["nets"]:
        net.double()
    solver.fused = "require"
    torch.manual_seed(1)
    solver.generator["train"] = SamplerGenerator(ResidentBatchGenerator.presample(cfg["gen"], 4, "cuda"))
    for _ in range(WARMUP):
        solver.run_train_epoch()
    torch.cuda.synchronize()
    fs = solver._fused_sys
    assert solver.fused_active and fs.f64 and fs.fusedk is not None and fs.f64_tail_ready() == (route == "fused")
    us = []
    for _ in range(WINDOWS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            solver.run_train_epoch()
        torch.cuda.synchronize()
        us.append((time.perf_counter() - t0) * 1e6 / steps)
    hist = solver.metrics_history["train_loss"]
    print(json.dumps({"system": name, "route": route, "points": points, "networks": len(cfg["nets"]),
                      "launches_per_step": fs.launches_per_step(), "steps_per_window": steps, "windows": WINDOWS,
                      "us_per_epoch": {"median": round(statistics.median(us), 2), "min": round(min(us), 2), "max": round(max(us), 2)},
                      "loss_first": hist[0], "loss_last": hist[-1], "device": torch.cuda.get_device_name(0)}), flush=True)


def _run(route, name, points, steps):
    proc = subprocess.run(["timeout", "-k", "10", str(LEG_SECONDS), sys.executable, os.path.abspath(__file__), "--leg", route, name,
                           str(points), str(steps)], capture_output=True, text=True)
    sys.stderr.write(proc.stderr[-2000:])
    if proc.returncode != 0:
        print(json.dumps({"system": name, "route": route, "points": points, "failed": proc.returncode}), flush=True)
        return None
    line = proc.stdout.strip().splitlines()[-1]
    print(line, flush=True)
    return json.loads(line)


def main(argv):
    opt = {"--pairs": "4", "--steps": "200"}
    for flag in list(opt):
        if flag in argv:
            opt[flag] = argv[argv.index(flag) + 1]
    pairs, steps = int(opt["--pairs"]), int(opt["--steps"])
    summary = {}
    for name, points in CASES:
        sep, fus, ratios, same = [], [], [], []
        for _ in range(pairs):
            a = _run("separate", name, points, steps)
            if a is None:
                return 1
            b = _run("fused", name, points, steps)
            if b is None:
                return 1
            sep.append(a["us_per_epoch"]["median"])
            fus.append(b["us_per_epoch"]["median"])
            ratios.append(round(sep[-1] / fus[-1], 3))
            same.append(a["loss_last"] == b["loss_last"])
        summary[f"{name}@{points}"] = {"separate_us": sep, "fused_us": fus, "separate_over_fused": ratios,
                                       "fused_faster_in_every_pair": all(r > 1.0 for r in ratios), "same_last_loss": all(same)}
    print(json.dumps({"summary": summary}), flush=True)
    return 0


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--leg":
        leg(sys.argv[2], sys.argv[3], int(sys.argv[4]), int(sys.argv[5]))
    else:
        sys.exit(main(sys.argv[1:]))
