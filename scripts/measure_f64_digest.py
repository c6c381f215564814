#!/usr/bin/env python3
"""Time of a state digest of the double-precision mode (include/lbm_d2q9_f64_digest.h) beside the gather it replaces, on one GPU in one
session: Grid64.digest() beside Grid64.get_cells(), and with --ranks N Rows64.digest() beside Rows64.get_cells() on N ranks of device
0.  Host clock around each call (every one of them ends in a stream synchronise), the two sides alternating call by call after two
warm-up calls of each, medians with the min - max spread.

    python scripts/measure_f64_digest.py --work 8192x8192 [--ranks 8] [--out profiles/r19/f64_digest.txt]

Run it under a time limit, one workload per process (--out appends), the steps chained so that a failure ends the session:

    F=profiles/r19/f64_digest.txt; rm -f $F
    timeout -k 10 300 python scripts/measure_f64_digest.py --work 8192x8192 --out $F &&
    timeout -k 10 120 python scripts/measure_f64_digest.py --work 1024x1024 --out $F &&
    timeout -k 10 300 python scripts/measure_f64_digest.py --work 8192x8192 --ranks 8 --out $F

--kernels: nothing is timed; three digests and one get_observables of the grid, for a kernel trace taken around the process (the
device time of lbm64_row_digest_kernel beside lbm64_observables_kernel, which reads the same 72 B per cell and writes 32 B more).

Bytes: a digest reads nine doubles per cell once, 72 B per cell, and brings 8 B per row to the host; get_cells moves 72 B per cell
through a device transpose, PCIe and a host copy.  A record, not a gate."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import mpilattice_boltzmann_amd as lbm  # noqa: E402
from mpilattice_boltzmann_amd import f64  # noqa: E402


def timed(call):
    t0 = time.perf_counter()
    out = call()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--work", default="8192x8192")
    ap.add_argument("--ranks", type=int, default=0, help="0: one Grid64; N: Rows64 on N ranks of device 0")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    nx, ny = (int(v) for v in a.work.split("x"))
    p =lbm.Params(nx=nx, ny=ny, max_iters=4, reynolds_dim=128, density=0.1, accel=0.005, omega=1.85)
    obst = np.zeros((ny, nx), np.int32)
    make = (lambda: f64.Rows64(p, obst, a.ranks, devices=[0] * a.ranks)) if a.ranks else (lambda: f64.Grid64(p, obst))
    with make() as g:
        g.run(3)                                          # a state that is not the rest state, in the second grid
        if a.kernels:
            for _ in range(3):
                g.digest()
            g.get_observables()
            return
        for _ in range(2):
            g.digest()
            g.get_cells()
        t_digest, t_cells = [], []
        for _ in range(a.repeats):
            t, (rows, total) = timed(g.digest)
            t_digest.append(t)
            t, cells = timed(g.get_cells)
            t_cells.append(t)
        host_rows, host_total = f64.digest_host(cells[:64], nx)           # the first 64 rows against the host form
        assert np.array_equal(rows[:64], host_rows), "digest differs from the host form"
        name = g.describe()["kernel"]
    md, mc = statistics.median(t_digest), statistics.median(t_cells)
    state_bytes = 72.0 * nx * ny
    lines = [f"{nx} x {ny}, {'Rows64 on %d ranks of one GPU' % a.ranks if a.ranks else 'Grid64'} ({name}), {a.repeats} alternating calls after 2 warm-up calls, host clock",
             f"  digest()     median {md * 1e3:10.3f} ms   min {min(t_digest) * 1e3:10.3f}   max {max(t_digest) * 1e3:10.3f}   {state_bytes / md / 1e12:6.3f} TB/s of state read, {8 * ny} B to the host",
             f"  get_cells()  median {mc * 1e3:10.3f} ms   min {min(t_cells) * 1e3:10.3f}   max {max(t_cells) * 1e3:10.3f}   {state_bytes / mc / 1e9:6.2f} GB/s of state delivered",
             f"  get_cells() / digest() = {mc / md:.0f}   state digest {total:016x}", ""]
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
