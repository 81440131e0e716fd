"""us per run_train_epoch() of an inverse problem: the device route (closure launch + ONE sums / tail launch that also steps the
scalars of the equations) against the parent commit's route, taken as THIS tree under NDQ_NO_THETA_TAIL=1 (the general epoch path:
per-network sums, host-side read of the loss, optimiser step from Python).  Alternating pairs, every leg a process of its own
under its own time limit.  Writes profiles/theta_tail_timing.md and profiles/theta_tail_timing.jsonl.

    python scripts/theta_tail_timing.py [--pairs 4]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [("inv1", 1024), ("inv1", 65536), ("lvtheta", 1024)]


def leg(case, n, epochs=400, warmup=50):
    """One process, one route (the environment decides): median-free plain mean over ``epochs`` epochs after ``warmup``."""
    import itertools
    import torch
    sys.path.insert(0, ROOT)
    from neurodiffeq_amd.generators import Generator1D, Generator2D
    from neurodiffeq_amd.optim import FusedAdam
    from neurodiffeq_amd.solvers import Solver1D, Solver2D
    torch.manual_seed(0)
    if case == "inv1":
        from tests import configs
        cfg = configs.make_inverse("inv1")
        g = int(round(n ** 0.5))
        gen = Generator2D((g, g), (-1, 0), (1, 1), "equally-spaced-noisy")
        nets, theta = cfg["nets"], cfg["theta"]
        make = lambda opt: Solver2D(cfg["pde"], cfg["conds"], xy_min=(-1, 0), xy_max=(1, 1), nets=nets, train_generator=gen,
                                    valid_generator=gen, optimizer=opt, n_batches_valid=0)
    else:
        from tests import wide_multi_problems as W
        nets, conds, eqs, _ = W.make("lvtheta", 128)
        theta = eqs.theta
        gen = Generator1D(n, W.T_MIN, W.T_MAX, "equally-spaced-noisy")
        make = lambda opt: Solver1D(eqs, conds, t_min=W.T_MIN, t_max=W.T_MAX, nets=nets, train_generator=gen, valid_generator=gen,
                                    optimizer=opt, n_batches_valid=0)
    for net in nets:
        net.to("cuda")
    for p in theta:
        p.data = p.data.to("cuda")
    solver = make(FusedAdam(itertools.chain((p for net in nets for p in net.parameters()), theta), lr=1e-3))
    solver.fused = "require"
    for _ in range(warmup):
        solver.run_train_epoch()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(epochs):
        solver.run_train_epoch()
    torch.cuda.synchronize()
    us = (time.perf_counter() - t0) / epochs * 1e6
    ready = solver._fused_sys.theta_tail_ready(solver.optimizer)
    print(json.dumps(dict(case=case, n=n, device_route=bool(ready), us_per_epoch=us, last_loss=solver.metrics_history["train_loss"][-1])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--leg", nargs=2)
    args = ap.parse_args()
    if args.leg:
        return leg(args.leg[0], int(args.leg[1]))
    rows = []
    for case, n in CASES:
        for pair in range(args.pairs):
            for route, switch in (("device", "0"), ("parent", "1")):
                env = dict(os.environ, NDQ_NO_THETA_TAIL=switch)
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", case, str(n)], env=env, cwd=ROOT,
                                     capture_output=True, text=True, timeout=240)
                if out.returncode != 0:
                    raise SystemExit(f"{case} {n} {route}: exit {out.returncode}\n{out.stderr[-2000:]}")
                row = json.loads(out.stdout.strip().splitlines()[-1])
                assert row["device_route"] == (route == "device"), row
                rows.append(dict(row, pair=pair, route=route))
                print(rows[-1], flush=True)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "theta_tail_timing.jsonl"), "w") as fh:
        for r in rows:
            fh.write(json.dumps(r) + "\n")
    lines = ["# Inverse problems: device-side end of the epoch against the general path", "",
             "us per `run_train_epoch()`; `parent` = this tree under `NDQ_NO_THETA_TAIL=1` (the parent commit's route). "
             "Alternating pairs, one process per leg (scripts/theta_tail_timing.py).", "",
             "| case | points | pair | device route | parent route | ratio |", "|---|---|---|---|---|---|"]
    lost = []
    for case, n in CASES:
        for pair in range(args.pairs):
            d = next(r for r in rows if (r["case"], r["n"], r["pair"], r["route"]) == (case, n, pair, "device"))["us_per_epoch"]
            p = next(r for r in rows if (r["case"], r["n"], r["pair"], r["route"]) == (case, n, pair, "parent"))["us_per_epoch"]
            lines.append(f"| {case} | {n} | {pair} | {d:.1f} | {p:.1f} | {p / d:.2f}x |")
            if d >= p:
                lost.append((case, n, pair))
    lines += ["", "Pairs the device route lost: " + (", ".join(map(str, lost)) if lost else "none") + "."]
    with open(os.path.join(ROOT, "profiles", "theta_tail_timing.md"), "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
