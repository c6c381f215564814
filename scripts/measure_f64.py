#!/usr/bin/env python3
"""Device time per step of the double-precision mode (lbm_step_kernel_f64, include/lbm_d2q9_f64.h) beside the float one-step kernel,
on one GPU in one session: lbm64_last_run_kernel_ms / lbm_last_run_kernel_ms, the two contexts of a workload alternating run by run,
medians.  The float context is made with LBM_TUNE_MULTI_K=0 and LBM_TUNE_TILE_MAX=0, which select lbm_step_kernel (describe() is
checked: the comparison is one step per launch on both sides).

    python scripts/measure_f64.py [--quick] [--work NAME] [--out profiles/r07/f64_step.txt]

Run it under a time limit, one workload per process (--work; --out then appends), the steps chained so that a failure ends the session:

    F=profiles/r07/f64_step.txt; rm -f $F
    timeout -k 10 300 python scripts/measure_f64.py --work 8192 --out $F &&
    timeout -k 10 120 python scripts/measure_f64.py --work 1024 --out $F &&
    timeout -k 10 120 python scripts/measure_f64.py --work 128  --out $F

Bytes: a step reads and writes nine populations per cell, 144 B per cell-step in double and 72 B in float (the obstacle bit and the
partial sums are not counted).  A record, not a gate."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import mpilattice_boltzmann_amd as lbm  # noqa: E402
from mpilattice_boltzmann_amd import f64  # noqa: E402


def deck(name):
    if name in ("1024x1024", "128x128"):
        d = os.path.join(ROOT, "tests", "golden", "decks")
        p = f64.read_params64(os.path.join(d, f"input_{name}.params"))
        return p, lbm.read_obstacles(os.path.join(d, f"obstacles_{name}.dat"), p.nx, p.ny)[0]
    nx, ny = (int(v) for v in name.split("x"))
    p = lbm.Params(nx=nx, ny=ny, max_iters=200, reynolds_dim=100, density=0.1, accel=0.005, omega=1.85)
    return p, lbm.synthetic_obstacles(nx, ny, p=0.005, seed=42, walls=True)


def measure(name, steps, reps, warm, lines):
    p, obst = deck(name)
    cells = p.nx * p.ny
    os.environ["LBM_TUNE_MULTI_K"] = "0"                 # read when the context is made: the float path's one-step kernel
    os.environ["LBM_TUNE_TILE_MAX"] = "0"
    single = lbm.Partition(p, lbm.count_free_cells(obst), obst)
    double = f64.Grid64(p, obst)
    kernels = {"float": single.describe()["kernel"], "double": double.describe()["kernel"]}
    if not kernels["float"].startswith("lbm_step_kernel"):
        raise SystemExit(f"the float context runs {kernels['float']}, not the one-step kernel")
    runs = {"float": single, "double": double}
    us = {k: [] for k in runs}
    for q in runs.values():
        for _ in range(warm):
            q.run(steps)
    for _ in range(reps):
        for k, q in runs.items():                        # alternate: both see the same drift of the card
            q.run(steps)
            ms, launches = q.last_run_kernel_ms()
            assert launches == steps, (k, launches)
            us[k].append(1e3 * ms / steps)
    desc = double.describe()
    single.close()
    double.close()
    med = {k: statistics.median(v) for k, v in us.items()}
    bytes_per = {"float": 72, "double": 144}
    tbs = {k: bytes_per[k] * cells / (med[k] * 1e-6) / 1e12 for k in runs}
    lines.append(f"{name}  {steps} steps per run, {reps} runs each, alternating; double launch: {desc['blocks']} blocks x {desc['cells_per_block']} cells")
    for k in runs:
        lines.append(f"  {k:7s} {kernels[k]:32s} us/step median {med[k]:9.3f}  min {min(us[k]):9.3f}  max {max(us[k]):9.3f}   {bytes_per[k]} B/cell-step -> {tbs[k]:.3f} TB/s")
    lines.append(f"  double / float: time {med['double'] / med['float']:.3f}, bytes per second {tbs['double'] / tbs['float']:.3f}")
    print("\n".join(lines[-4:]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="small step counts (a functional check of this script)")
    ap.add_argument("--work", help="one workload only: 8192, 1024 or 128 (--out appends)")
    ap.add_argument("--out")
    a = ap.parse_args()
    lbm.build()
    lines = ["# scripts/measure_f64.py: lbm_step_kernel_f64 beside the float one-step kernel, device time per step (events around the step launches)"]
    if a.quick:
        work = {"1024": ("1024x1024", 40, 3, 1), "128": ("128x128", 400, 3, 1)}
    else:
        work = {"8192": ("8192x8192", 200, 5, 1), "1024": ("1024x1024", 2000, 5, 1), "128": ("128x128", 40000, 5, 1)}
    if a.work:
        if a.work not in work:
            ap.error(f"--work: one of {', '.join(work)}")
        work = {a.work: work[a.work]}
        if a.out and os.path.exists(a.out):
            lines = []                  # a later step of the chain: the heading is there
    for name, steps, reps, warm in work.values():
        measure(name, steps, reps, warm, lines)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a" if a.work else "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
