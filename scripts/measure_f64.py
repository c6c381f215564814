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
partial sums are not counted).  A record, not a gate.

--tile: LBM64_FLAG_TILE_STEPS (lbm_tile_kernel_f64, several steps per launch) in every geometry beside the one-step double path of a
BASELINE build of the library (--baseline-lib: the parent commit's liblbm_d2q9.so, built beside this one and loaded privately), on the
shipped decks at full length and on 512 x 512: device time of whole runs, the contexts alternating run by run.

    F=profiles/r08/f64_tile.txt; rm -f $F
    for w in 128x128 128x256 256x256 512x512 1024x1024; do
      timeout -k 10 240 python scripts/measure_f64.py --tile --baseline-lib mpilattice-boltzmann_amd/lib/variants/liblbm_d2q9_parent.so --work $w --out $F || break
    done

--multi: LBM64_FLAG_MULTI_STEPS (lbm_multi_kernel_f64, K steps per launch of a large grid) with every built K beside the one-step double
path of the same BASELINE build, and beside LBM64_FLAG_TILE_STEPS where that flag takes the size: device time per step, the contexts
alternating run by run.  --multi-bits K: on 8192 x 7296, whose planes pass 4 GiB, 2K + 1 steps with the flag and without, populations
compared for equal bits (host-bound, about 13 GB of host memory); its line goes to the same file.

    F=profiles/r11/f64_multi.txt; rm -f $F; B=mpilattice-boltzmann_amd/lib/variants/liblbm_d2q9_parent.so
    timeout -k 10 300 python scripts/measure_f64.py --multi --baseline-lib $B --work 8192x8192 --out $F &&
    timeout -k 10 180 python scripts/measure_f64.py --multi --baseline-lib $B --work 4096x4096 --out $F &&
    timeout -k 10 120 python scripts/measure_f64.py --multi --baseline-lib $B --work 2048x2048 --out $F &&
    timeout -k 10 120 python scripts/measure_f64.py --multi --baseline-lib $B --work 1024x1024 --out $F &&
    timeout -k 10 300 python scripts/measure_f64.py --multi-bits 3 --out $F

--multi-any: LBM64_FLAG_MULTI_ANY_SIZE (the edge-tile form of lbm_multi_kernel_f64 on grids that 32 x 16 tiles do not cover) beside
the best of the same BASELINE build for the grid: its one-step kernel, or on a grid the tiles cover its LBM64_FLAG_MULTI_STEPS run,
which flag 4096 must equal in time.  One size per process:

    F=profiles/r20/f64_multi_any.txt; rm -f $F; B=mpilattice-boltzmann_amd/lib/variants/liblbm_d2q9_parent.so
    for w in 8190x8190 8192x8192 4098x4100 2050x2046 1022x1026; do
      timeout -k 10 240 python scripts/measure_f64.py --multi-any --baseline-lib $B --work $w --out $F || break
    done

--ranks N[,N] [--devices LIST] [--steps S]: row-partitioned runs (f64.Rows64, include/lbm_d2q9_f64_rows.h) with each rank count beside
the one-context one-step and LBM64_FLAG_MULTI_STEPS runs of the same grid (--work NXxNY, default 8192x8192), alternating: device and
wall time per step.  Each rank count runs three times: without a flag, with LBM_ROWS64_FLAG_MULTI_STEPS (K steps per launch and
exchange) and with LBM_ROWS64_FLAG_MULTI_ANY_SIZE (the same, and the kernel's edge-tile form on ranks the tiles do not cover, uneven
ranks among them); the minimum size is lowered to 0 so that every size is measured, and a flagged run that takes the one-step kernel
all the same is left out.  With --baseline-lib (the parent commit's build) each rank count also runs in that build, without a flag
and, where it takes the kernel there, with LBM_ROWS64_FLAG_MULTI_STEPS.  Lines under the table hold each flagged run against the
unflagged ones: the median gain beside the two max - min spreads together.  With all ranks on one device this measures the loop's
overhead, not a speed-up; --out appends.

    F=profiles/r22/f64_rows_any.txt; rm -f $F; B=mpilattice-boltzmann_amd/lib/variants/liblbm_d2q9_parent.so
    timeout -k 10 500 python scripts/measure_f64.py --ranks 1,2,8 --baseline-lib $B --work 8190x8190 --out $F &&
    timeout -k 10 300 python scripts/measure_f64.py --ranks 1,2,8 --baseline-lib $B --work 4098x4100 --out $F &&
    timeout -k 10 200 python scripts/measure_f64.py --ranks 1,2,8 --baseline-lib $B --work 2050x2046 --steps 400 --out $F &&
    timeout -k 10 200 python scripts/measure_f64.py --ranks 1,2,8 --baseline-lib $B --work 1022x1026 --steps 2000 --out $F &&
    timeout -k 10 500 python scripts/measure_f64.py --ranks 1,2,8 --baseline-lib $B --work 8192x8192 --out $F

    F=profiles/r18/f64_rows_multi.txt; rm -f $F
    timeout -k 10 400 python scripts/measure_f64.py --ranks 1,2,8 --work 8192x8192 --out $F &&
    timeout -k 10 200 python scripts/measure_f64.py --ranks 1,2,8 --work 4096x4096 --out $F &&
    timeout -k 10 200 python scripts/measure_f64.py --ranks 1,2,8 --work 2048x2048 --steps 400 --out $F &&
    timeout -k 10 200 python scripts/measure_f64.py --ranks 1,2,8 --work 1024x1024 --steps 2000 --out $F &&
    timeout -k 10 200 python scripts/measure_f64.py --ranks 1 --work 8192x1024 --out $F

--cols N [--devices LIST] [--steps S] --work NXxNY: column-partitioned runs (f64.Cols64, include/lbm_d2q9_f64_cols.h) on N ranks beside
f64.Rows64 with LBM_ROWS64_FLAG_MULTI_ANY_SIZE on the same grid and rank count, and beside one column rank's share of the grid run
alone, alternating: device and wall time per step.  One grid per process; --out appends.

    F=profiles/r23/f64_cols.txt; rm -f $F
    for w in 65536x128 32768x256 16384x512 32768x64 8192x8192; do
      timeout -k 10 240 python scripts/measure_f64.py --cols 8 --devices 0 --work $w --steps 40 --out $F || break
    done"""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np

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


TILE_GEOMS = (84, 88, 164, 168)
TILE_DECKS = {"128x128": None, "128x256": None, "256x256": None, "512x512": 10000, "1024x1024": None}      # steps; None: the deck's max_iters


class BaselineGrid64:
    """lbm64_* of another build of the library (dlopen'ed privately): create, run, last_run_kernel_ms, describe, close."""

    def __init__(self, path, p, obst, flags=0):
        # RTLD_DEEPBIND: the two builds export the same names (weak inline functions among them, whose types may differ between the
        # builds); the baseline must call its own, not those of the library the package loaded first
        self.lib = C.CDLL(os.path.abspath(path), mode=os.RTLD_LOCAL | os.RTLD_DEEPBIND)
        for name, (res, args) in f64._SIGNATURES.items():
            fn = getattr(self.lib, name)
            fn.restype, fn.argtypes = res, args
        self.lib.lbm_last_error.restype = C.c_char_p
        self.obst = np.ascontiguousarray(obst, dtype=np.int32)
        self.cp = f64._cparams(p)
        self.ctx = C.c_void_p()
        self._check(self.lib.lbm64_create(C.byref(self.ctx), C.byref(self.cp), int(self.obst.size - np.count_nonzero(self.obst)),
                                          self.obst.ctypes.data_as(C.POINTER(C.c_int)), 0, flags))

    def _check(self, rc):
        if rc:
            raise SystemExit(f"baseline library: {self.lib.lbm_last_error().decode()}")

    def run(self, n):
        av = np.zeros(n, np.float64)
        self._check(self.lib.lbm64_run(self.ctx, n, av.ctypes.data_as(C.POINTER(C.c_double))))
        return av

    def last_run_kernel_ms(self):
        ms, n = C.c_double(0.0), C.c_int(0)
        self._check(self.lib.lbm64_last_run_kernel_ms(self.ctx, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def describe(self):
        name = C.create_string_buffer(256)
        self._check(self.lib.lbm64_describe(self.ctx, name, 256, None, None, None))
        return {"kernel": name.value.decode()}

    def close(self):
        self.lib.lbm64_destroy(self.ctx)


def measure_tile(name, baseline_lib, reps, lines, steps_override=None):
    if name in ("128x128", "128x256", "256x256", "1024x1024"):
        d = os.path.join(ROOT, "tests", "golden", "decks")
        p = f64.read_params64(os.path.join(d, f"input_{name}.params"))
        obst = lbm.read_obstacles(os.path.join(d, f"obstacles_{name}.dat"), p.nx, p.ny)[0]
    else:
        p, obst = deck(name)
    steps = steps_override or TILE_DECKS[name] or p.max_iters
    os.environ["LBM_TUNE_TILE64_MAX"] = str(1 << 30)      # read when a context is made: every geometry on every deck
    runs = {"one-step (baseline build)": BaselineGrid64(baseline_lib, p, obst)}
    for geom in TILE_GEOMS:
        os.environ["LBM_TUNE_TILE64_GEOM"] = str(geom)
        g = f64.Grid64(p, obst, flags=f64.FLAG_TILE_STEPS)
        if not g.describe()["kernel"].startswith("lbm_tile_kernel_f64<"):
            raise SystemExit(f"{name}, geometry {geom}: the context runs {g.describe()['kernel']}")
        runs[f"<{geom // 10},{geom % 10}>"] = g
    kernels = {k: q.describe()["kernel"] for k, q in runs.items()}
    first = {k: q.run(steps) for k, q in runs.items()}     # the warm-up run: every context from the rest state
    base = first["one-step (baseline build)"]
    for k, av in first.items():                            # the same run: av_vels agree to the order of their additions
        if not np.allclose(av, base, rtol=1e-12, atol=0.0):
            raise SystemExit(f"{name}, {k}: av_vels differ from the baseline's by {np.max(np.abs(av - base) / base):.3e}")
    ms = {k: [] for k in runs}
    for _ in range(reps):
        for k, q in runs.items():                          # alternate: all see the same drift of the card
            q.run(steps)
            ms[k].append(q.last_run_kernel_ms()[0])
    for q in runs.values():
        q.close()
    lines.append(f"{name}  {steps} steps per run, {reps} runs each, alternating; device time of a run's step launches")
    for k in runs:
        v = ms[k]
        lines.append(f"  {k:26s} {kernels[k]:28s} s/run median {statistics.median(v) / 1e3:9.5f}  min {min(v) / 1e3:9.5f}  max {max(v) / 1e3:9.5f}   us/step {1e3 * statistics.median(v) / steps:8.3f}")
    b = ms["one-step (baseline build)"]
    best = min((k for k in runs if k.startswith("<")), key=lambda k: statistics.median(ms[k]))
    gain = statistics.median(b) - statistics.median(ms[best])
    spreads = (max(b) - min(b)) + (max(ms[best]) - min(ms[best]))
    lines.append(f"  fastest geometry {best}: baseline / tiled {statistics.median(b) / statistics.median(ms[best]):.3f}; median gain {gain / 1e3:.5f} s against "
                 f"the two max - min spreads together {spreads / 1e3:.5f} s -> {'a win' if gain > spreads else 'no win'}")
    print("\n".join(lines[-(len(runs) + 2):]), flush=True)


MULTI_K = (2, 3, 4)                                          # every K lbm_multi_kernel_f64 is built for
MULTI_WORK = {"1024x1024": 1200, "2048x2048": 240, "4096x4096": 120, "8192x8192": 60}      # steps per run: multiples of every K


def measure_multi(name, baseline_lib, reps, lines, steps_override=None):
    """LBM64_FLAG_MULTI_STEPS with every built K beside the one-step double kernel of the baseline build (and, where the tiled kernel
    takes the size, beside LBM64_FLAG_TILE_STEPS): device time per step, the contexts alternating run by run."""
    p, obst = deck(name)
    steps = steps_override or MULTI_WORK[name]
    n0 = len(lines)
    os.environ["LBM_TUNE_MULTI64_MIN"] = "0"              # read when a context is made: every K on every size
    base_key = "one-step (baseline build)"
    runs = {base_key: BaselineGrid64(baseline_lib, p, obst)}
    if not runs[base_key].describe()["kernel"].startswith("lbm_step_kernel_f64<"):
        raise SystemExit(f"{name}: the baseline runs {runs[base_key].describe()['kernel']}")
    for k in MULTI_K:
        os.environ["LBM_TUNE_MULTI64_K"] = str(k)
        g = f64.Grid64(p, obst, flags=f64.FLAG_MULTI_STEPS)
        if not g.describe()["kernel"].startswith(f"lbm_multi_kernel_f64<{k}"):
            raise SystemExit(f"{name}, K = {k}: the context runs {g.describe()['kernel']}")
        runs[f"K = {k}"] = g
    tiled = f64.Grid64(p, obst, flags=f64.FLAG_TILE_STEPS)   # default knobs: the tiled kernel where LBM_TUNE_TILE64_MAX lets it
    if tiled.describe()["kernel"].startswith("lbm_tile_kernel_f64<"):
        runs["tiled (flag 512)"] = tiled
    else:
        tiled.close()
    kernels = {k: q.describe()["kernel"] for k, q in runs.items()}
    first = {k: q.run(steps) for k, q in runs.items()}     # the warm-up run: every context from the rest state
    for k, av in first.items():                            # the same run: av_vels agree to the order of their additions
        if not np.allclose(av, first[base_key], rtol=1e-12, atol=0.0):
            raise SystemExit(f"{name}, {k}: av_vels differ from the baseline's by {np.max(np.abs(av - first[base_key]) / first[base_key]):.3e}")
    us = {k: [] for k in runs}
    for _ in range(reps):
        for k, q in runs.items():                          # alternate: all see the same drift of the card
            q.run(steps)
            us[k].append(1e3 * q.last_run_kernel_ms()[0] / steps)
    for q in runs.values():
        q.close()
    med = {k: statistics.median(v) for k, v in us.items()}
    spread = {k: max(v) - min(v) for k, v in us.items()}
    lines.append(f"{name}  {steps} steps per run, {reps} runs each, alternating; device time of a run's step launches, us per step")
    for k in runs:
        lines.append(f"  {k:26s} {kernels[k]:28s} us/step median {med[k]:9.3f}  min {min(us[k]):9.3f}  max {max(us[k]):9.3f}   {144 * p.nx * p.ny / med[k] / 1e6:6.3f} TB/s at 144 B/cell-step")
    best = min((k for k in runs if k.startswith("K = ")), key=lambda k: med[k])
    for other in [k for k in runs if not k.startswith("K = ")]:
        gain, spreads = med[other] - med[best], spread[other] + spread[best]
        lines.append(f"  fastest {best} against {other}: {med[other] / med[best]:.3f} x; median gain {gain:.3f} us against the two max - min spreads together "
                     f"{spreads:.3f} us -> {'a win' if gain > spreads else 'no win'}")
    print("\n".join(lines[n0:]), flush=True)


MULTI_ANY_STEPS = ((1 << 25, 60), (1 << 23, 120), (1 << 21, 240), (0, 1200))      # steps per run by cells: multiples of every K


def measure_multi_any(name, baseline_lib, reps, lines, steps_override=None):
    """LBM64_FLAG_MULTI_ANY_SIZE at the library's K beside the parent commit's best for the same grid, in the baseline build: the
    one-step kernel on a grid that 32 x 16 tiles do not cover, LBM64_FLAG_MULTI_STEPS on one they do (the same kernel: the two must
    agree within their spreads).  Device time per step, the contexts alternating run by run."""
    p, obst = deck(name)
    steps = steps_override or next(s for cells, s in MULTI_ANY_STEPS if p.nx * p.ny >= cells)
    n0 = len(lines)
    os.environ["LBM_TUNE_MULTI64_MIN"] = "0"              # read when a context is made: every size is measured
    exact = p.nx % 32 == 0 and p.ny % 16 == 0
    base_key = "parent build, flag 1024" if exact else "parent build, one step"
    runs = {base_key: BaselineGrid64(baseline_lib, p, obst, flags=f64.FLAG_MULTI_STEPS if exact else 0)}
    runs["flag 4096"] = f64.Grid64(p, obst, flags=f64.FLAG_MULTI_ANY_SIZE)
    if exact:
        runs["flag 1024"] = f64.Grid64(p, obst, flags=f64.FLAG_MULTI_STEPS)
    kernels = {k: q.describe()["kernel"] for k, q in runs.items()}
    want = "lbm_multi_kernel_f64<" if exact else "lbm_step_kernel_f64<"
    if not kernels[base_key].startswith(want) or not kernels["flag 4096"].startswith("lbm_multi_kernel_f64<") or kernels["flag 4096"].endswith(",edge>") == exact:
        raise SystemExit(f"{name}: the contexts run {kernels}")
    first = {k: q.run(steps) for k, q in runs.items()}     # the warm-up run: every context from the rest state
    for k, av in first.items():                            # the same run: av_vels agree to the order of their additions
        if not np.allclose(av, first[base_key], rtol=1e-12, atol=0.0):
            raise SystemExit(f"{name}, {k}: av_vels differ from the baseline's by {np.max(np.abs(av - first[base_key]) / first[base_key]):.3e}")
    us = {k: [] for k in runs}
    for _ in range(reps):
        for k, q in runs.items():                          # alternate: all see the same drift of the card
            q.run(steps)
            us[k].append(1e3 * q.last_run_kernel_ms()[0] / steps)
    blocks = runs["flag 4096"].describe()["blocks"]
    for q in runs.values():
        q.close()
    med = {k: statistics.median(v) for k, v in us.items()}
    spread = {k: max(v) - min(v) for k, v in us.items()}
    lines.append(f"{name}  {steps} steps per run, {reps} runs each, alternating; {blocks} tiles; device time of a run's step launches, us per step")
    for k in runs:
        lines.append(f"  {k:26s} {kernels[k]:32s} us/step median {med[k]:9.3f}  min {min(us[k]):9.3f}  max {max(us[k]):9.3f}   {144 * p.nx * p.ny / med[k] / 1e6:6.3f} TB/s at 144 B/cell-step"
                     f"   {1e3 * med[k] / blocks:7.3f} ns per tile-step")
    gain, spreads = med[base_key] - med["flag 4096"], spread[base_key] + spread["flag 4096"]
    if exact:
        lines.append(f"  flag 4096 against {base_key}: {med[base_key] / med['flag 4096']:.4f} x; median difference {gain:.3f} us against the two max - min spreads together "
                     f"{spreads:.3f} us -> {'the same time' if abs(gain) <= spreads else 'DIFFERENT'}")
    else:
        lines.append(f"  flag 4096 against {base_key}: {med[base_key] / med['flag 4096']:.3f} x; median gain {gain:.3f} us against the two max - min spreads together "
                     f"{spreads:.3f} us -> {'a win' if gain > spreads else 'no win'}")
    print("\n".join(lines[n0:]), flush=True)


def multi_bits(ks, lines):
    """8192 x 7296 (the nine planes pass 4 GiB): 2K + 1 steps from tests/test_f64.py's separable state with the flag and without;
    populations compared by row blocks for equal bits."""
    nx, ny = 8192, 7296
    p = lbm.Params(nx=nx, ny=ny, max_iters=2, reynolds_dim=10, density=0.1, accel=0.005, omega=1.85)
    obst = lbm.synthetic_obstacles(nx, ny, p=0.005, seed=42, walls=True)
    w0, w1, w2 = p.density * 4.0 / 9.0, p.density / 9.0, p.density / 36.0
    cells = np.empty((ny, nx, 9), np.float64)
    cells[:] = np.array([w0] + [w1] * 4 + [w2] * 4)
    cells *= (1.0 + 0.03 * np.sin(0.013 * np.arange(ny)))[:, None, None]
    cells *= (1.0 + 0.03 * np.cos(0.007 * np.arange(nx)))[None, :, None]
    os.environ["LBM_TUNE_MULTI64_MIN"] = "0"
    for k in ks:
        os.environ["LBM_TUNE_MULTI64_K"] = str(k)
        got, kernels = {}, {}
        for flags in (0, f64.FLAG_MULTI_STEPS):
            with f64.Grid64(p, obst, flags=flags) as g:
                kernels[flags] = g.describe()["kernel"]
                g.set_cells(cells)
                av = g.run(2 * k + 1)
                got[flags] = (g.get_cells(), av, g.last_run_kernel_ms()[1])
        if not kernels[f64.FLAG_MULTI_STEPS].startswith(f"lbm_multi_kernel_f64<{k}") or not kernels[0].startswith("lbm_step_kernel_f64<"):
            raise SystemExit(f"8192x7296: the contexts run {kernels}")
        (off, av_off, n_off), (on, av_on, n_on) = got[0], got[f64.FLAG_MULTI_STEPS]
        bad = [y0 for y0 in range(0, ny, 512) if not np.array_equal(off[y0:y0 + 512].view(np.uint64), on[y0:y0 + 512].view(np.uint64))]
        lines.append(f"8192x7296  {2 * k + 1} steps from a separable state: {kernels[0]} in {n_off} launches, {kernels[f64.FLAG_MULTI_STEPS]} in {n_on}; "
                     f"populations by row blocks of 512: {'equal bits in every block' if not bad else f'DIFFERENT in blocks at rows {bad}'}; "
                     f"av_vels differ by at most {float(np.max(np.abs(av_on - av_off) / av_off)):.2e} relative")
        print(lines[-1], flush=True)
        del got, off, on
        if bad:
            raise SystemExit("8192x7296: the populations differ")


class BaselineRows64:
    """lbm_rows64_* of another build of the library (dlopen'ed privately, as BaselineGrid64): create, run, last_run_ms, describe, close."""

    def __init__(self, path, p, obst, nranks, devices=None, flags=0):
        self.lib = C.CDLL(os.path.abspath(path), mode=os.RTLD_LOCAL | os.RTLD_DEEPBIND)
        for name, (res, args) in f64._ROWS_SIGNATURES.items():
            fn = getattr(self.lib, name)
            fn.restype, fn.argtypes = res, args
        self.lib.lbm_last_error.restype = C.c_char_p
        self.obst = np.ascontiguousarray(obst, dtype=np.int32)
        self.cp = f64._cparams(p)
        self.run_ = C.c_void_p()
        dev = None if devices is None else (C.c_int * len(devices))(*devices)
        self._check(self.lib.lbm_rows64_create(C.byref(self.run_), C.byref(self.cp), int(self.obst.size - np.count_nonzero(self.obst)),
                                               self.obst.ctypes.data_as(C.POINTER(C.c_int)), nranks, dev, flags))

    def _check(self, rc):
        if rc:
            raise SystemExit(f"baseline library: {self.lib.lbm_last_error().decode()}")

    def run(self, n):
        av = np.zeros(n, np.float64)
        self._check(self.lib.lbm_rows64_run(self.run_, n, av.ctypes.data_as(C.POINTER(C.c_double))))
        return av

    def last_run_ms(self):
        ms, n = C.c_double(0.0), C.c_int(0)
        self._check(self.lib.lbm_rows64_last_run_ms(self.run_, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def describe(self):
        name = C.create_string_buffer(256)
        blocks = C.c_longlong(0)
        self._check(self.lib.lbm_rows64_describe(self.run_, name, 256, None, C.byref(blocks), None, None))
        return {"kernel": name.value.decode(), "blocks": blocks.value}

    def close(self):
        self.lib.lbm_rows64_destroy(self.run_)


PARENT = " (parent build)"


def measure_rows(name, ranks, devices, steps, reps, lines, baseline_lib=None):
    """Row-partitioned runs (f64.Rows64, include/lbm_d2q9_f64_rows.h) with each rank count of `ranks` beside the one-context one-step
    kernel and the one-context LBM64_FLAG_MULTI_STEPS run of the same grid: per step, the device time (events: for a partitioned run
    the largest span over the ranks) and the host's wall time around run(), which ends in a synchronise.  The contexts alternate run by
    run.  With all ranks on one device their kernels serialise: the difference to the one-context figure is the loop's overhead.
    Each rank count runs without a flag, with LBM_ROWS64_FLAG_MULTI_STEPS and with LBM_ROWS64_FLAG_MULTI_ANY_SIZE (a flagged run that
    takes the one-step kernel all the same is left out); with `baseline_lib` also in that build, without a flag and, where it takes the
    kernel there, with LBM_ROWS64_FLAG_MULTI_STEPS."""
    import time
    p, obst = deck(name)
    n0 = len(lines)
    os.environ["LBM_TUNE_MULTI64_MIN"] = "0"              # read when a context is made: the multi-step kernels on every size the tiles cover
    runs = {"one context, one step": f64.Grid64(p, obst)}
    multi = f64.Grid64(p, obst, flags=f64.FLAG_MULTI_STEPS)
    if multi.describe()["kernel"].startswith("lbm_multi_kernel_f64<"):
        runs["one context, multi-step"] = multi
    else:
        multi.close()
    for n in ranks:
        dev = None if devices is None else [devices[r % len(devices)] for r in range(n)]
        key = f"{n} rank{'s' if n > 1 else ''}"
        runs[key] = f64.Rows64(p, obst, n, devices=dev)
        made = [(key + ", multi-step", f64.Rows64(p, obst, n, devices=dev, flags=f64.FLAG_ROWS_MULTI_STEPS)),
                (key + ", any-size", f64.Rows64(p, obst, n, devices=dev, flags=f64.FLAG_ROWS_MULTI_ANY_SIZE))]
        if baseline_lib:
            runs[key + PARENT] = BaselineRows64(baseline_lib, p, obst, n, devices=dev)
            made.append((key + ", multi-step" + PARENT, BaselineRows64(baseline_lib, p, obst, n, devices=dev, flags=f64.FLAG_ROWS_MULTI_STEPS)))
        for k, flagged in made:
            if flagged.describe()["kernel"].startswith("lbm_rows_multi_kernel_f64<"):
                runs[k] = flagged
            else:
                flagged.close()                            # the flag changes nothing on this run
    shapes = {k: q.describe() for k, q in runs.items()}
    first = {k: q.run(steps) for k, q in runs.items()}     # the warm-up run: every context from the rest state
    base = first["one context, one step"]
    for k, av in first.items():                            # the same run: av_vels agree to the order of their additions
        if not np.allclose(av, base, rtol=1e-12, atol=0.0):
            raise SystemExit(f"{name}, {k}: av_vels differ from the one-step context's by {np.max(np.abs(av - base) / base):.3e}")
    dev_us, wall_us = {k: [] for k in runs}, {k: [] for k in runs}
    for _ in range(reps):
        for k, q in runs.items():                          # alternate: all see the same drift of the card
            t0 = time.perf_counter()
            q.run(steps)
            wall_us[k].append(1e6 * (time.perf_counter() - t0) / steps)
            ms = q.last_run_ms()[0] if isinstance(q, (f64.Rows64, BaselineRows64)) else q.last_run_kernel_ms()[0]
            dev_us[k].append(1e3 * ms / steps)
    for q in runs.values():
        q.close()
    where = "the library's default (rank r on device r % device count)" if devices is None else f"devices {devices}, cycled"
    lines.append(f"{name}  {steps} steps per run, {reps} runs each, alternating; ranks on {where}; us per step")
    for k in runs:
        d, w = dev_us[k], wall_us[k]
        lines.append(f"  {k:38s} {shapes[k]['kernel']:38s} {shapes[k]['blocks']:6d} blocks   device median {statistics.median(d):9.3f}  min {min(d):9.3f}  max {max(d):9.3f}"
                     f"   wall median {statistics.median(w):9.3f}  min {min(w):9.3f}  max {max(w):9.3f}")
    def against(k, off, same=False):
        med = {q: statistics.median(dev_us[q]) for q in (off, k)}
        gain = med[off] - med[k]
        spreads = (max(dev_us[off]) - min(dev_us[off])) + (max(dev_us[k]) - min(dev_us[k]))
        cells = p.nx * min(lbm.decompose(p.ny, int(off.split()[0]))[0])
        verdict = ("the same time" if abs(gain) <= spreads else "DIFFERENT") if same else ("a win" if gain > spreads else "no win")
        lines.append(f"  {k} against {off} ({cells} cells in the smallest rank): {med[off] / med[k]:.3f} x; median gain {gain:.3f} us against the two max - min "
                     f"spreads together {spreads:.3f} us -> {verdict}")

    for n in ranks:
        key = f"{n} rank{'s' if n > 1 else ''}"
        for flagged in (key + ", multi-step", key + ", any-size"):
            if flagged in runs:
                against(flagged, key)
                if key + PARENT in runs:
                    against(flagged, key + PARENT)           # the parent's run of the same shape without a flag
        if key + ", multi-step" + PARENT in runs:              # the same kernel in both builds
            for flagged in (key + ", multi-step", key + ", any-size"):
                if flagged in runs:
                    against(flagged, key + ", multi-step" + PARENT, same=True)
    print("\n".join(lines[n0:]), flush=True)


def measure_cols(name, nranks, devices, steps, reps, lines):
    """Column-partitioned runs (f64.Cols64, include/lbm_d2q9_f64_cols.h) beside the row-partitioned run of the same grid and rank count
    under LBM_ROWS64_FLAG_MULTI_ANY_SIZE (whatever kernel that takes: on thin ranks the one-step one), and beside ONE column rank's
    share of the grid run alone as a periodic grid of its own (nx / nranks x ny on one column rank): device time (the largest span over
    the ranks) and the host's wall time per step, the runs alternating.  With all ranks on one device their kernels serialise: this
    compares the two partitions' work and exchange volume on one GPU, not a speed-up over several."""
    import time
    p, obst = deck(name)
    n0 = len(lines)
    os.environ["LBM_TUNE_MULTI64_MIN"] = "0"              # read when a run is made: the rows' multi-step kernel on every size it can tile
    dev = None if devices is None else [devices[r % len(devices)] for r in range(nranks)]
    runs = {f"{nranks} column ranks": f64.Cols64(p, obst, nranks, devices=dev),
            f"{nranks} row ranks, any-size": f64.Rows64(p, obst, nranks, devices=dev, flags=f64.FLAG_ROWS_MULTI_ANY_SIZE)}
    share_nx = p.nx // nranks
    if nranks > 1 and share_nx % 2 == 0 and share_nx >= 32:
        ps, os_ = deck(f"{share_nx}x{p.ny}")
        runs["1 column rank's share alone"] = f64.Cols64(ps, os_, 1, devices=None if dev is None else dev[:1])
    shapes = {k: q.describe() for k, q in runs.items()}
    first = {k: q.run(steps) for k, q in runs.items()}     # the warm-up run: every run from the rest state
    ck, rk = list(runs)[:2]
    if not np.allclose(first[ck], first[rk], rtol=1e-12, atol=0.0):     # the same run: av_vels agree to the order of their additions
        raise SystemExit(f"{name}: av_vels of the column and the row run differ by {np.max(np.abs(first[ck] - first[rk]) / first[rk]):.3e}")
    dev_us, wall_us = {k: [] for k in runs}, {k: [] for k in runs}
    for _ in range(reps):
        for k, q in runs.items():                          # alternate: all see the same drift of the card
            t0 = time.perf_counter()
            q.run(steps)
            wall_us[k].append(1e6 * (time.perf_counter() - t0) / steps)
            dev_us[k].append(1e3 * q.last_run_ms()[0] / steps)
    for q in runs.values():
        q.close()
    where = "the library's default (rank r on device r % device count)" if devices is None else f"devices {devices}, cycled"
    lines.append(f"{name}  {steps} steps per run, {reps} runs each, alternating; ranks on {where}; us per step")
    for k in runs:
        d, w = dev_us[k], wall_us[k]
        lines.append(f"  {k:32s} {shapes[k]['kernel']:40s} {shapes[k]['blocks']:6d} blocks  {shapes[k]['state_bytes'] / 2 ** 20:9.1f} MiB   device median {statistics.median(d):9.3f}  min {min(d):9.3f}"
                     f"  max {max(d):9.3f}   wall median {statistics.median(w):9.3f}  min {min(w):9.3f}  max {max(w):9.3f}")
    med = {k: statistics.median(dev_us[k]) for k in (ck, rk)}
    gain = med[rk] - med[ck]
    spreads = (max(dev_us[rk]) - min(dev_us[rk])) + (max(dev_us[ck]) - min(dev_us[ck]))
    verdict = "columns win" if gain > spreads else "rows win" if -gain > spreads else "level"
    lines.append(f"  rows / columns: {med[rk] / med[ck]:.3f} x; median difference {gain:.3f} us against the two max - min spreads together {spreads:.3f} us -> {verdict}")
    print("\n".join(lines[n0:]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="small step counts (a functional check of this script)")
    ap.add_argument("--work", help="one workload only: 8192, 1024 or 128 (--out appends)")
    ap.add_argument("--out")
    ap.add_argument("--tile", action="store_true", help="LBM64_FLAG_TILE_STEPS in every geometry against --baseline-lib's one-step path; --work: a deck")
    ap.add_argument("--multi", action="store_true", help="LBM64_FLAG_MULTI_STEPS with every built K against --baseline-lib's one-step path; --work: a size")
    ap.add_argument("--multi-bits", metavar="K[,K]", help="the 8192 x 7296 bit comparison of lbm_multi_kernel_f64<K> with the one-step kernel (--out appends)")
    ap.add_argument("--multi-any", action="store_true", help="LBM64_FLAG_MULTI_ANY_SIZE against --baseline-lib's best for the grid; --work: NXxNY (--out appends)")
    ap.add_argument("--baseline-lib", help="liblbm_d2q9.so of the parent commit")
    ap.add_argument("--ranks", metavar="N[,N]", help="row-partitioned runs (f64.Rows64) with these rank counts beside the one-context runs; --work: NXxNY (default 8192x8192)")
    ap.add_argument("--devices", metavar="LIST", help="with --ranks: HIP ordinals, rank r on LIST[r %% len(LIST)] (default: the library's, r %% device count)")
    ap.add_argument("--steps", type=int, help="with --ranks: steps per run (default 200)")
    ap.add_argument("--cols", type=int, metavar="N", help="column-partitioned runs (f64.Cols64) on N ranks beside Rows64 with LBM_ROWS64_FLAG_MULTI_ANY_SIZE; --work: NXxNY; --devices, --steps as for --ranks")
    a = ap.parse_args()
    lbm.build()
    if a.cols:
        if not a.work:
            ap.error("--cols needs --work NXxNY")
        lines = [] if a.out and os.path.exists(a.out) else [
            "# scripts/measure_f64.py --cols: column-partitioned double-precision runs (lbm_cols_multi_kernel_f64 + lbm64_push_ghost_cols_kernel per rank-launch) beside the "
            "row-partitioned run of the same grid and rank count under LBM_ROWS64_FLAG_MULTI_ANY_SIZE, and one column rank's share alone",
            "# device: events around a run's launches, over its steps, the largest span over the ranks; wall: the host's clock around run()"]
        measure_cols(a.work, a.cols, [int(v) for v in a.devices.split(",")] if a.devices else None, a.steps or (12 if a.quick else 200), 3 if a.quick else 5, lines)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as fh:
                fh.write("\n".join(lines) + "\n")
        return 0
    if a.ranks:
        lines = [] if a.out and os.path.exists(a.out) else [
            "# scripts/measure_f64.py --ranks: row-partitioned double-precision runs (lbm_rows_kernel_f64 + lbm64_push_rows_kernel per rank-step; \"multi-step\": "
            "LBM_ROWS64_FLAG_MULTI_STEPS, \"any-size\": LBM_ROWS64_FLAG_MULTI_ANY_SIZE, lbm_rows_multi_kernel_f64 + lbm64_push_ghost_rows_kernel per rank-launch) beside the one-context runs",
            "# device: events around a run's step launches, over its steps (partitioned: the largest span over the ranks); wall: the host's clock around run()"]
        measure_rows(a.work or "8192x8192", [int(v) for v in a.ranks.split(",")], [int(v) for v in a.devices.split(",")] if a.devices else None,
                     a.steps or (12 if a.quick else 200), 3 if a.quick else 5, lines, baseline_lib=a.baseline_lib)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as fh:
                fh.write("\n".join(lines) + "\n")
        return 0
    if a.multi_bits:
        lines = []
        multi_bits([int(v) for v in a.multi_bits.split(",")], lines)
        if a.out:
            with open(a.out, "a") as fh:
                fh.write("\n".join(lines) + "\n")
        return 0
    if a.multi_any:
        if not a.baseline_lib or not os.path.exists(a.baseline_lib) or not a.work:
            ap.error("--multi-any needs --work NXxNY and --baseline-lib, an existing build of the library")
        lines = [] if a.out and os.path.exists(a.out) else [
            "# scripts/measure_f64.py --multi-any: LBM64_FLAG_MULTI_ANY_SIZE (the edge-tile form of lbm_multi_kernel_f64 where 32 x 16 tiles do not cover the grid) beside "
            "the parent commit's best for the same grid, in the parent commit's build",
            "# device time per step (lbm64_last_run_kernel_ms: events around the step launches of a run, over its steps); LBM_TUNE_MULTI64_MIN=0, the library's K"]
        measure_multi_any(a.work, a.baseline_lib, 3 if a.quick else 5, lines, steps_override=12 if a.quick else None)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as fh:
                fh.write("\n".join(lines) + "\n")
        return 0
    if a.multi:
        if not a.baseline_lib or not os.path.exists(a.baseline_lib):
            ap.error("--multi needs --baseline-lib, an existing build of the library")
        sizes = [a.work] if a.work else list(MULTI_WORK)
        if any(d not in MULTI_WORK for d in sizes):
            ap.error(f"--work: one of {', '.join(MULTI_WORK)}")
        lines = [] if a.work and a.out and os.path.exists(a.out) else [
            "# scripts/measure_f64.py --multi: lbm_multi_kernel_f64 (LBM64_FLAG_MULTI_STEPS), every built K, beside the one-step double path of the parent commit's build",
            "# device time per step (lbm64_last_run_kernel_ms: events around the step launches of a run, over its steps)"]
        for d in sizes:
            measure_multi(d, a.baseline_lib, 3 if a.quick else 5, lines, steps_override=12 if a.quick else None)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a" if a.work else "w") as fh:
                fh.write("\n".join(lines) + "\n")
        return 0
    if a.tile:
        if not a.baseline_lib or not os.path.exists(a.baseline_lib):
            ap.error("--tile needs --baseline-lib, an existing build of the library")
        decks = [a.work] if a.work else list(TILE_DECKS)
        if any(d not in TILE_DECKS for d in decks):
            ap.error(f"--work: one of {', '.join(TILE_DECKS)}")
        lines = [] if a.work and a.out and os.path.exists(a.out) else [
            "# scripts/measure_f64.py --tile: lbm_tile_kernel_f64 (LBM64_FLAG_TILE_STEPS), every geometry, beside the one-step double path of the parent commit's build",
            "# device time of whole runs (lbm64_last_run_kernel_ms: events around the step launches of a run)"]
        for d in decks:
            measure_tile(d, a.baseline_lib, 3 if a.quick else 5, lines, steps_override=200 if a.quick else None)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a" if a.work else "w") as fh:
                fh.write("\n".join(lines) + "\n")
        return 0
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
