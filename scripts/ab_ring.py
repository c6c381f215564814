#!/usr/bin/env python3
"""A/B of library knobs on a 1-rank peer-to-peer ring (box-to-box spread exceeds what a per-run overhead of 10-20 us is
worth): one ring per setting in one process, short runs, rings alternated round-robin, wall time of `run(steps)` + device
synchronise per run as bench.py times it.

    python scripts/ab_ring.py --grid 8192x1024 --steps 20 --rounds 40 - LBM_TUNE_MACRO_GHOST=16

Each positional argument is one setting: comma-separated KEY=VALUE pairs put into the environment while its ring is created
(the library reads its knobs when it creates a context or a transport: csrc/lbm_knobs.h); a setting "-" is the default
environment.  The key LBM_EXCHANGE in a setting is that ring's loop (p2p | rccl) instead of --exchange; --rank-grid 1x1 makes the rings
one rank of the tile (2-D) decomposition:

    python scripts/ab_ring.py --grid 2048x512 --rank-grid 1x1 --steps 400 --rounds 24 - LBM_EXCHANGE=rccl

--per-context is the only mode and is accepted for old command lines; --single runs the grid as one periodic
launch per macro-step instead of a ring."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import mpilattice_boltzmann_amd as lbm  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--grid", default="8192x1024")
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=40)
ap.add_argument("--exchange", default="p2p")
ap.add_argument("--rank-grid", default="", help="1x1: a tile rank that is its own neighbour in all four directions")
ap.add_argument("--per-context", action="store_true", help="the only mode (every setting gets its own ring)")
ap.add_argument("--single", action="store_true")
ap.add_argument("settings", nargs="+")
a = ap.parse_args()
nx, ny = (int(v) for v in a.grid.split("x"))
p = lbm.Params(nx, ny, a.steps, 10, 0.1, 0.005, 1.85)
obst = lbm.synthetic_obstacles(nx, ny, 0.005, 42, True)
def apply(setting):
    keys = []
    if setting != "-":
        for kv in setting.split(","):
            k, v = kv.split("=")
            os.environ[k] = v
            keys.append(k)
    return keys


def make():
    if a.single:
        return lbm.Simulation(p, obst)
    exchange = os.environ.get("LBM_EXCHANGE", a.exchange)
    if a.rank_grid:
        return lbm.Simulation(p, obst, exchange=exchange, strict=True, rank_grid=tuple(int(v) for v in a.rank_grid.split("x")))
    return lbm.Simulation(p, obst, flags=lbm._capi.FLAG_FORCE_HALO, exchange=exchange, strict=True)


sims = {}
for s in a.settings:
    keys = apply(s)
    sims[s] = make()
    assert sims[s].loop in ("single", os.environ.get("LBM_EXCHANGE", a.exchange)), sims[s].describe()
    for k in keys:
        os.environ.pop(k, None)
    sims[s].run(a.steps)
res = {s: [] for s in a.settings}
for r in range(a.rounds):
    for s in a.settings:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sims[s].run(a.steps)
        torch.cuda.synchronize()
        res[s].append((time.perf_counter() - t0) / a.steps * 1e6)
for s in a.settings:
    v = res[s][2:]
    print(f"{s:40s} min {min(v):7.2f}  med {statistics.median(v):7.2f}  max {max(v):7.2f} us/step", flush=True)
for sim in sims.values():
    sim.close()
