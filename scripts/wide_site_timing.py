#!/usr/bin/env python
"""One training epoch (Solver.run_train_epoch, one batch of resident points) of the heat equation with two Neumann ends -- one
network at three evaluation sites (tests/wide_site_problems.py: heat-nn) -- on FCNN(2, 1, (128,)) and FCNN(2, 1, (512,)), at
1 024 and 65 536 points, on three builds:
  parent    a checkout of the PARENT commit (`--parent DIR`, a built tree): the per-site three-kernel pipeline
  closure   this tree: the "wide_sites" single-launch closure + one sums / tail launch
  off       this tree with NDQ_NO_WIDE_SITE_FUSE=1: the per-site pipeline of this tree
in ALTERNATING rounds -- parent, closure, off, parent, closure, off, ... -- so that drift of the machine shows as spread between
rounds instead of as a difference between the builds.
Every leg is a child process of its own under `timeout`; the first leg that fails ends the run.  Per leg: WARMUP epochs, then
WINDOWS windows of STEPS epochs, host clock around a loop that ends in a synchronise; the median window counts, and the leg
reports its own spread (min, max).  Launches per epoch are the engine's count (FusedSystem.launches_per_step).
Prints one JSON line per leg and a last line with the per-round ratios.
usage: scripts/wide_site_timing.py [--parent DIR] [--pairs N] [--steps K] > wide_site_timing.jsonl"""
import importlib.util
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARMUP, WINDOWS = 30, 5
LEG_SECONDS = 240
WIDTHS = (128, 512)
SIZES = (1024, 65536)


def _problems():
    """tests/site_problems.py and tests/wide_site_problems.py of THIS tree (a parent checkout has no wide_site_problems); they
    import neurodiffeq_amd from whatever tree leads sys.path."""
    mods = {}
    for name in ("site_problems", "wide_site_problems"):
        spec = importlib.util.spec_from_file_location(f"tests.{name}", os.path.join(ROOT, "tests", f"{name}.py"))
        mods[name] = importlib.util.module_from_spec(spec)
        sys.modules[f"tests.{name}"] = mods[name]
        spec.loader.exec_module(mods[name])
    return mods["site_problems"], mods["wide_site_problems"]


def system(width):
    """(nets, conditions, equations) of the timed system: wide_site_problems' heat-nn on one hidden layer of ``width`` units."""
    SP, WS = _problems()
    nets, conds, eqs, _ = WS.make(f"heat-nn-{width}")
    return SP, nets, conds, eqs


def leg(tree, route, width, points, steps):
    if route == "off":
        os.environ["NDQ_NO_WIDE_SITE_FUSE"] = "1"
    sys.path.insert(0, tree)
    import torch
    from neurodiffeq_amd.generators import Generator2D, ResidentBatchGenerator, SamplerGenerator
    from neurodiffeq_amd.solvers import Solver2D
    torch.manual_seed(0)
    SP, nets, conds, eqs = system(width)
    side = int(round(points ** 0.5))
    lo, hi = (SP.X0, SP.T0), (SP.X1, SP.T0 + 1.0)
    gen = Generator2D((side, side), lo, hi, "equally-spaced-noisy")
    solver = Solver2D(eqs, conds, xy_min=lo, xy_max=hi, nets=nets, train_generator=gen, valid_generator=gen, n_batches_valid=0)
    solver.fused = "require"
    torch.manual_seed(1)
    solver.generator["train"] = SamplerGenerator(ResidentBatchGenerator.presample(gen, 4, "cuda"))
    for _ in range(WARMUP):
        solver.run_train_epoch()
    torch.cuda.synchronize()
    fs = solver._fused_sys
    assert solver.fused_active and (fs.fusedk is not None) == (route == "closure")
    us = []
    for _ in range(WINDOWS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            solver.run_train_epoch()
        torch.cuda.synchronize()
        us.append((time.perf_counter() - t0) * 1e6 / steps)
    hist = solver.metrics_history["train_loss"]
    print(json.dumps({"width": width, "route": route, "points": points, "sites": fs.n_sites,
                      "single_launch": fs.fusedk is not None, "launches_per_step": fs.launches_per_step(),
                      "steps_per_window": steps, "windows": WINDOWS,
                      "us_per_epoch": {"median": round(statistics.median(us), 2), "min": round(min(us), 2), "max": round(max(us), 2)},
                      "loss_first": hist[0], "loss_last": hist[-1], "device": torch.cuda.get_device_name(0)}), flush=True)


def _run(tree, route, width, points, steps):
    proc = subprocess.run(["timeout", "-k", "10", str(LEG_SECONDS), sys.executable, os.path.abspath(__file__), "--leg", tree, route,
                           str(width), str(points), str(steps)], capture_output=True, text=True)
    sys.stderr.write(proc.stderr[-2000:])
    if proc.returncode != 0:
        print(json.dumps({"width": width, "route": route, "points": points, "failed": proc.returncode}), flush=True)
        return None
    line = proc.stdout.strip().splitlines()[-1]
    print(line, flush=True)
    return json.loads(line)["us_per_epoch"]["median"]


def main(argv):
    opt = {"--parent": None, "--pairs": "4", "--steps": "200"}
    for flag in list(opt):
        if flag in argv:
            opt[flag] = argv[argv.index(flag) + 1]
    parent, pairs, steps = opt["--parent"], int(opt["--pairs"]), int(opt["--steps"])
    summary = {}
    for width in WIDTHS:
        for points in SIZES:
            rows = {"parent": [], "closure": [], "off": []}
            for _ in range(pairs):
                for route in (("parent",) if parent else ()) + ("closure", "off"):
                    us = _run(os.path.abspath(parent) if route == "parent" else ROOT, route, width, points, steps)
                    if us is None:
                        return 1
                    rows[route].append(us)
            summary[f"{width}@{points}"] = {
                "closure_us": rows["closure"], "off_us": rows["off"], "parent_us": rows["parent"],
                "parent_over_closure": [round(a / b, 3) for a, b in zip(rows["parent"], rows["closure"])],
                "off_over_closure": [round(a / b, 3) for a, b in zip(rows["off"], rows["closure"])]}
    print(json.dumps({"summary": summary}), flush=True)
    return 0


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--leg":
        leg(sys.argv[2], sys.argv[3], int(sys.argv[4]), int(sys.argv[5]), int(sys.argv[6]))
    else:
        sys.exit(main(sys.argv[1:]))
