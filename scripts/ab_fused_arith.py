#!/usr/bin/env python3
"""A/B of LBM_FLAG_FUSED_ARITH against the default arithmetic on one GPU, back to back in one session: device time per step from
lbm_last_run_kernel_ms, the default and the fused context of a workload alternating run by run.

    python scripts/ab_fused_arith.py [--quick] [--work NAME] [--out profiles/r05/ab_fused_arith.txt]

Run it under a time limit, one workload per process (--work; --out then appends), the steps chained so that a failure ends the session:

    F=profiles/r05/ab_fused_arith.txt; rm -f $F
    timeout -k 10 240 python scripts/ab_fused_arith.py --work 8192x200  --out $F &&
    timeout -k 10 300 python scripts/ab_fused_arith.py --work 8192x2000 --out $F &&
    timeout -k 10 120 python scripts/ab_fused_arith.py --work 1024      --out $F &&
    timeout -k 10 120 python scripts/ab_fused_arith.py --work 128       --out $F

Workloads: 8192 x 8192 synthetic deck, 200 steps per run; the same as 3 runs of 2000 steps (sustained: the card settles at its power
limit); the shipped 1024 x 1024 and 128 x 128 decks.  Socket power and shader clock from the card's hwmon files (bench.PowerSampler)
over each variant's runs, where they can be read.  A record, not a gate: the ratio is printed whichever side of 1 it falls."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mpilattice_boltzmann_amd as lbm  # noqa: E402


def deck(name):
    if name in ("1024x1024", "128x128"):
        d = os.path.join(ROOT, "tests", "golden", "decks")
        p = lbm.read_params(os.path.join(d, f"input_{name}.params"))
        return p, lbm.read_obstacles(os.path.join(d, f"obstacles_{name}.dat"), p.nx, p.ny)[0]
    nx, ny = (int(v) for v in name.split("x"))
    p = lbm.Params(nx=nx, ny=ny, max_iters=2000, reynolds_dim=100, density=0.1, accel=0.005, omega=1.85)
    return p, lbm.synthetic_obstacles(nx, ny, p=0.005, seed=42, walls=True)


def measure(name, steps, reps, warm, lines):
    from bench import PowerSampler
    p, obst = deck(name)
    free = lbm.count_free_cells(obst)
    parts = {"default": lbm.Partition(p, free, obst), "fused": lbm.Partition(p, free, obst, flags=lbm._capi.FLAG_FUSED_ARITH)}
    us = {k: [] for k in parts}
    power = {}
    for k, q in parts.items():
        for _ in range(warm):
            q.run(steps)
    for rep in range(reps):
        for k, q in parts.items():                      # alternate: both see the same drift of the card
            sampler = PowerSampler(None).start()
            q.run(steps)
            ms, _ = q.last_run_kernel_ms()
            power[k] = sampler.stop() or power.get(k)
            us[k].append(1e3 * ms / steps)
    kernels = {k: q.describe()["kernel"] for k, q in parts.items()}
    for q in parts.values():
        q.close()
    med = {k: statistics.median(v) for k, v in us.items()}
    lines.append(f"{name}  {steps} steps per run, {reps} runs each, alternating")
    for k in parts:
        pw = power.get(k) or {}
        watts = f"  socket {pw['socket_w_median']:.0f} W of {pw['cap_w']:.0f}, sclk {pw['sclk_mhz_median']:.0f} MHz" if pw.get("socket_w_median") and pw.get("cap_w") and pw.get("sclk_mhz_median") else ""
        lines.append(f"  {k:8s} {kernels[k]:42s} us/step median {med[k]:9.3f}  min {min(us[k]):9.3f}  max {max(us[k]):9.3f}{watts}")
    lines.append(f"  fused / default = {med['fused'] / med['default']:.4f}")
    print("\n".join(lines[-4:]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="small step counts (a functional check of this script)")
    ap.add_argument("--work", help="one workload only: 8192x200, 8192x2000, 1024 or 128 (--out appends)")
    ap.add_argument("--out")
    a = ap.parse_args()
    lbm.build()
    lines = ["# scripts/ab_fused_arith.py: LBM_FLAG_FUSED_ARITH against the default arithmetic, device time (lbm_last_run_kernel_ms)"]
    if a.quick:
        work = {"1024": ("1024x1024", 40, 3, 1), "128": ("128x128", 400, 3, 1)}
    else:
        work = {"8192x200": ("8192x8192", 200, 5, 1), "8192x2000": ("8192x8192", 2000, 3, 0), "1024": ("1024x1024", 2000, 5, 1), "128": ("128x128", 40000, 5, 1)}
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
