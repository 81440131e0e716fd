#!/usr/bin/env python
"""One training epoch (Solver.run_train_epoch, one batch of resident points) of two-network systems with fp64 networks -- the
reference's default precision -- at 1 024 and 65 536 points:
  c1        Lotka-Volterra, two FCNN(1, 1, (32, 32), SinActv)      (tests/configs.py)
  lv_tanh   the same equations on two tanh networks                (tests/f64_multi_problems.py)
and, with --single, the one-network fp64 headline (c2: 2-D Laplace, FCNN(2, 1, (32, 32))) for reference,
on the route of the PARENT commit (the fp64 three-kernel pipeline: `--parent DIR`, a built checkout -- or, without it, this tree
under NDQ_F64_CLOSURE=0, which restores that launch sequence kernel for kernel) and on this tree's default route (the
multi-network closure kernel compiled in double, then the separate sums and epoch tails), in ALTERNATING pairs -- parent, new,
parent, new, ... -- so that drift of the machine shows as spread between pairs instead of as a difference between the routes.
Every leg is a child process of its own under `timeout`; the first leg that fails ends the run.  Per leg: WARMUP epochs, then
WINDOWS windows of STEPS epochs, host clock around a loop that ends in a synchronise; the median window counts.
Prints one JSON line per leg and a last line with the per-pair ratios.
usage: scripts/f64_multi_timing.py [--parent DIR] [--pairs N] [--steps K] [--single] > f64_multi_timing.jsonl"""
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
SYSTEMS = ("c1", "lv_tanh")
SIZES = (1024, 65536)


def _problems():
    """tests/f64_multi_problems.py of THIS tree (a parent checkout has none); it imports neurodiffeq_amd from whatever tree
    leads sys.path."""
    spec = importlib.util.spec_from_file_location("f64_multi_problems", os.path.join(ROOT, "tests", "f64_multi_problems.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def leg(tree, route, name, points, steps):
    if route == "pipeline":
        os.environ["NDQ_F64_CLOSURE"] = "0"
    sys.path.insert(0, tree)
    import torch
    from neurodiffeq_amd.generators import Generator1D, Generator2D, ResidentBatchGenerator, SamplerGenerator
    from neurodiffeq_amd.solvers import Solver1D, Solver2D
    torch.manual_seed(0)
    if name == "c2":
        from tests import configs
        cfg = configs.make("c2", 8)
        side = int(round(points ** 0.5))
        nets = [n.double() for n in cfg["nets"]]
        gen = Generator2D((side, side), (0, 0), (1, 1), "equally-spaced-noisy")
        solver = Solver2D(cfg["pde"], cfg["conds"], xy_min=(0, 0), xy_max=(1, 1), nets=nets, train_generator=gen,
                          valid_generator=gen, n_batches_valid=0)
    else:
        nets, conds, eqs, _, _ = _problems().make(name)
        lo, hi = (0.1, 12.0) if name == "c1" else (0.0, 1.0)
        gen = Generator1D(points, lo, hi, "equally-spaced-noisy")
        solver = Solver1D(eqs, conds, t_min=lo, t_max=hi, nets=nets, train_generator=gen, valid_generator=gen, n_batches_valid=0)
    solver.fused = "require"
    torch.manual_seed(1)
    solver.generator["train"] = SamplerGenerator(ResidentBatchGenerator.presample(gen, 4, "cuda"))
    for _ in range(WARMUP):
        solver.run_train_epoch()
    torch.cuda.synchronize()
    fs = solver._fused_sys
    assert solver.fused_active and fs.f64
    us = []
    for _ in range(WINDOWS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            solver.run_train_epoch()
        torch.cuda.synchronize()
        us.append((time.perf_counter() - t0) * 1e6 / steps)
    hist = solver.metrics_history["train_loss"]
    print(json.dumps({"system": name, "route": route, "points": points, "networks": len(nets),
                      "single_launch": fs.fusedk is not None, "launches_per_step": fs.launches_per_step(),
                      "steps_per_window": steps, "windows": WINDOWS,
                      "us_per_epoch": {"median": round(statistics.median(us), 2), "min": round(min(us), 2), "max": round(max(us), 2)},
                      "loss_first": hist[0], "loss_last": hist[-1], "device": torch.cuda.get_device_name(0)}), flush=True)


def _run(tree, route, name, points, steps):
    proc = subprocess.run(["timeout", "-k", "10", str(LEG_SECONDS), sys.executable, os.path.abspath(__file__), "--leg", tree, route,
                           name, str(points), str(steps)], capture_output=True, text=True)
    sys.stderr.write(proc.stderr[-2000:])
    if proc.returncode != 0:
        print(json.dumps({"system": name, "route": route, "points": points, "failed": proc.returncode}), flush=True)
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
    for name in SYSTEMS + (("c2",) if "--single" in argv else ()):
        for points in SIZES:
            ratios, new, old_all = [], [], []
            for _ in range(pairs):
                old = _run(os.path.abspath(parent) if parent else ROOT, "pipeline", name, points, steps)
                us = _run(ROOT, "closure", name, points, steps)
                if us is None or old is None:
                    return 1
                new.append(us)
                old_all.append(old)
                ratios.append(round(old / us, 3))
            summary[f"{name}@{points}"] = {"closure_us": new, "pipeline_us": old_all, "pipeline_over_closure": ratios}
    print(json.dumps({"summary": summary}), flush=True)
    return 0


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--leg":
        leg(sys.argv[2], sys.argv[3], sys.argv[4], int(sys.argv[5]), int(sys.argv[6]))
    else:
        sys.exit(main(sys.argv[1:]))
