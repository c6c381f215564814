#!/usr/bin/env python3
"""Randomised cross-check of the kernel family on one GPU: every case runs the same deck through the
library's own choice (lbm_multi_kernel / lbm_tile_kernel, random K / geometry / tile width, 1-rank rings over the
peer-to-peer and the RCCL loop, with the three forms of the sum|u| terms) and through the one-step
kernel (LBM_TUNE_MULTI_K=0, LBM_TUNE_TILE_MAX=0), and the final populations must agree bit for bit.
No oracle involved (the one-step kernel is pinned to it by the test suite): thousands of cells x
hundreds of shapes in a minute.

    python scripts/fuzz_kernels.py [--cases 300] [--seed 1]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")        # the "tiles" cases run several ranks of one process on this GPU: a hardware queue each (read when HIP initialises)
import mpilattice_boltzmann_amd as lbm  # noqa: E402


def run_tiles(p, obst, px, py, steps):
    """The px x py ranks of a tile (2-D) decomposition as contexts of this process, one host thread each, over the peer-to-peer loop.
    None when the grid cannot be tiled that way (a rank outside K-step mode)."""
    size = px * py
    free = lbm.count_free_cells(obst)
    try:
        lays = [lbm.tile_layout(p, px, py, r) for r in range(size)]
    except lbm.LbmError:
        return None, None, None
    parts = [lbm.Partition(p, free, lbm.obstacle_window(obst, lays[r]), tile_of=(r, px, py)) for r in range(size)]
    rings = lbm.P2PRing.local_ring(parts)
    halves = [steps // 2, steps - steps // 2] if steps > 1 else [steps]
    tot = np.concatenate([lbm.P2PRing.run_all(rings, n)[0] for n in halves])
    cells = np.empty((p.ny, p.nx, 9), dtype=np.float32)
    for q, l in zip(parts, lays):
        cells[l["y0"]:l["y0"] + l["ny_local"], l["x0"]:l["x0"] + l["nx_local"]] = q.get_cells()
    for ring in rings:
        ring.close()
    for q in parts:
        q.close()
    av = (tot * np.float64(np.float32(1.0) / np.float32(free))).astype(np.float32)
    return cells.view(np.uint32).copy(), av, lays[0]

def run_partitions(p, obst, size, steps, kstep):
    """`size` row partitions of one grid on one GPU, exchanged by device copies in the order of the step loops."""
    import torch
    free = int(obst.size - obst.sum())
    ny_local, displs = lbm.decompose(p.ny, size)
    dev = torch.device("cuda", 0)
    if kstep:
        parts = [lbm.Partition(p, free, obst[displs[r]:displs[r] + ny_local[r]], displs[r], obstacles_global=obst) for r in range(size)]
        K = parts[0].macro_steps
        if K == 0 or any(q.macro_steps != K for q in parts):
            for q in parts:
                q.close()
            return None, None
    else:
        parts = [lbm.Partition(p, free, obst[displs[r]:displs[r] + ny_local[r]], displs[r], flags=lbm._capi.FLAG_ONE_STEP) for r in range(size)]
        for q in parts:
            q.bind_halo_tensors(dev)
    torch.cuda.synchronize()
    tstream = torch.cuda.Stream(dev)
    st = tstream.cuda_stream
    with torch.cuda.stream(tstream):
        if kstep:
            for q in parts:
                q.macro_prepare(steps, st)
            done = 0
            while done < steps:
                for r, q in enumerate(parts):
                    q.macro_receive_from(parts[(r - 1) % size], lbm.NORTH, st)
                    q.macro_receive_from(parts[(r + 1) % size], lbm.SOUTH, st)
                for q in parts:
                    q.macro_interior(st)
                    q.macro_edge(st)
                k = parts[0].macro_next
                for q in parts:
                    q.macro_finish(st)
                done += k
        else:
            for q in parts:
                q.step_prepare(steps, st)
            for _ in range(steps):
                for r, q in enumerate(parts):          # each partition's outgoing rows into its neighbours' incoming buffers
                    south, north = parts[(r - 1) % size], parts[(r + 1) % size]
                    south.halo_recv(lbm.NORTH).copy_(q.halo_send(lbm.SOUTH), non_blocking=True)
                    north.halo_recv(lbm.SOUTH).copy_(q.halo_send(lbm.NORTH), non_blocking=True)
                for q in parts:
                    q.step_interior(st)
                    q.step_boundary(st)
                    q.step_finish(st)
        sums = sum(q.step_collect(steps, st) for q in parts)
    tstream.synchronize()
    cells = np.concatenate([q.get_cells() for q in parts], axis=0).view(np.uint32).copy()
    for q in parts:
        q.close()
    return cells, (sums * np.float64(np.float32(1.0) / np.float32(free))).astype(np.float32)


KNOBS = ["LBM_TUNE_MULTI_K", "LBM_TUNE_TILE_MAX", "LBM_TUNE_TILE_GEOM", "LBM_TUNE_MACRO_K", "LBM_TUNE_NARROW_MAX", "LBM_TUNE_MULTI_TILE",
         "LBM_TUNE_TILE_SINGLE_MAX", "LBM_P2P_SCHEDULE", "LBM_TUNE_MACRO_GHOST", "LBM_TUNE_MACRO_GROUP", "LBM_TUNE_TILE_GHOST_ROWS"]


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=300)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--scale", type=int, default=1, help="multiplies the upper bounds of the random grid sizes")
    ap.add_argument("--tiles-case", default="", help="(internal) one case of the tile decomposition, as JSON, in this fresh process")
    a = ap.parse_args(argv)
    if a.tiles_case:
        return tiles_case(json.loads(a.tiles_case))
    saved = {k: os.environ.get(k) for k in KNOBS}          # the cases set these; put the caller's values back at the end
    try:
        return fuzz(a)
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def tiles_case(c) -> int:
    """One `tiles` case: the ranks of the decomposition as contexts of this process against the one-step kernel on the whole grid."""
    rng = np.random.default_rng(c["seed"])
    nx, ny, steps = c["nx"], c["ny"], c["steps"]
    obst = (rng.random((ny, nx)) < c["dens"]).astype(np.int32)
    if c["walls"]:
        obst[0, :] = obst[-1, :] = 1
    if obst.all():
        obst[1, 1] = 0
    p = lbm.Params(nx, ny, steps, 4, c["density"], c["accel"], c["omega"])
    os.environ.update(c["env"])
    cells, av, lay0 = run_tiles(p, obst, c["px"], c["py"], steps)
    for k in KNOBS:
        os.environ.pop(k, None)
    if cells is None:
        print(f"tiles {c['px']}x{c['py']} {nx}x{ny}: not eligible, skipped ok")
        return 0
    os.environ.update({"LBM_TUNE_MULTI_K": "0", "LBM_TUNE_TILE_MAX": "0"})
    s1 = lbm.Simulation(p, obst)
    av1 = s1.run(steps)
    c1 = s1.local_cells().view(np.uint32).copy()
    s1.close()
    same = np.array_equal(cells, c1)
    avd = float(np.max(np.abs(av - av1) / np.maximum(np.abs(av1), 1e-30)))
    good = same and avd <= 1e-6
    print(f"tiles {c['px']}x{c['py']} {nx}x{ny} steps {steps} K {lay0['macro_k']} ghost {lay0['ghost']}/{lay0['ghost_x']} group {lay0['group']} "
          f"cells_same={same} av_rel={avd:.2e} {'ok' if good else 'MISMATCH'}")
    return 0 if good else 1


def fuzz(a) -> int:
    rng = np.random.default_rng(a.seed)
    bad = 0
    for case in range(a.cases):
        kind = rng.choice(["multi", "tile", "ring", "parts", "parts1", "forms", "parts", "tiles"])      # (weights: "parts" twice, "vector" twice below)
        flags_fast = 0
        if kind == "forms":
            # the one-step kernels among themselves: one cell per lane / four cells per lane, with and
            # without non-temporal stores, any nx (odd too) and ny >= 3
            nx, ny = int(rng.integers(1, 300)), int(rng.integers(3, 120))
            form = rng.choice(["narrow", "vector", "vector", "nt", "no_nt"])
            env = {"LBM_TUNE_TILE_MAX": "0", "LBM_TUNE_MULTI_K": "0"}
            if form == "narrow":
                env["LBM_TUNE_NARROW_MAX"] = str(1 << 30)
            elif form == "vector":
                env["LBM_TUNE_NARROW_MAX"] = "0"
            else:
                env["LBM_TUNE_NARROW_MAX"] = "0"
                flags_fast = {"nt": lbm._capi.FLAG_NT_STORES, "no_nt": lbm._capi.FLAG_NO_NT_STORES}[form]
        elif kind == "tile":
            T = int(rng.choice([8, 16]))
            nx, ny = T * int(rng.integers(1, 20)), T * int(rng.integers(1, 20))
            if ny < 3:
                ny = T * 2
            env = {"LBM_TUNE_TILE_MAX": str(1 << 30), "LBM_TUNE_TILE_GEOM": str(T * 10 + int(rng.choice([4, 8]))), "LBM_TUNE_MULTI_K": "0",
                   "LBM_TUNE_TILE_SINGLE_MAX": str(rng.choice([0, 256, 512]))}        # x-pairs only / one cell per lane in the late sub-steps
        else:
            nx = 2 * int(rng.integers(64, 400 * a.scale)) if rng.random() < 0.7 else 64 * int(rng.integers(2, 12 * a.scale))
            ny = int(rng.integers(32, 300 * a.scale))
            K = int(rng.integers(1, 5))
            env = {"LBM_TUNE_TILE_MAX": "0", "LBM_TUNE_MULTI_K": str(K), "LBM_TUNE_MACRO_K": str(max(K, 2) if kind in ("ring", "parts") else K),
                   "LBM_TUNE_MULTI_TILE": str(rng.choice([32, 64])), "LBM_P2P_SCHEDULE": str(rng.choice(["edge", "serial"])),
                   # ghost rows = steps between two halo exchanges: 0 -> K rows, an exchange before every launch (tails of 1 and 2 steps); 4 -> four at
                   # any K (3s and 4s at K = 3); more: groups of several launches, the first advancing the ghost rows the later ones read
                   "LBM_TUNE_MACRO_GHOST": str(rng.choice([0, 4, 7, 8, 12, 16])), "LBM_TUNE_MACRO_GROUP": str(rng.choice([0, 0, 1, 2, 3]))}
            if env["LBM_TUNE_MACRO_GROUP"] == "0":
                del env["LBM_TUNE_MACRO_GROUP"]
        steps = int(rng.integers(1, 40))
        dens = float(rng.choice([0.0, 0.002, 0.05, 0.3]))
        p = lbm.Params(nx, ny, steps, 4, float(rng.choice([0.1, 1.0])), float(rng.choice([0.005, 0.05, 0.5])), float(rng.choice([0.7, 1.3, 1.85, 1.97])))
        obst = (rng.random((ny, nx)) < dens).astype(np.int32)
        if rng.random() < 0.5:
            obst[0, :] = obst[-1, :] = 1
        if rng.random() < 0.2:
            obst[ny - 2, :] = 1
        if obst.all():
            obst[1, 1] = 0
        if kind == "tiles":
            # the tile (2-D) decomposition on a random rank grid: blocks of >= 128 columns and >= 32 rows so that every rank is eligible.  In a
            # process of its own: the ranks share this GPU and need a hardware queue each (a wait kernel must never sit in front of the push it
            # waits for), which a process that has created and destroyed hundreds of streams no longer guarantees (seen: a bounded wait
            # timing out in case 39 of seed 77 here, the same case green in a fresh process)
            px, py = int(rng.integers(1, 4)), int(rng.integers(1, 4))
            spec = {"px": px, "py": py, "nx": 2 * int(rng.integers(64 * px, 64 * px + 200 * a.scale)), "ny": int(rng.integers(32 * py + 3, 32 * py + 260 * a.scale)),
                    "steps": steps, "dens": dens, "walls": bool(rng.random() < 0.5), "seed": int(rng.integers(1, 1 << 30)),
                    "density": p.density, "accel": p.accel, "omega": p.omega,
                    "env": {k: v for k, v in env.items() if k in ("LBM_TUNE_MACRO_K", "LBM_TUNE_MULTI_TILE", "LBM_TUNE_MACRO_GHOST", "LBM_TUNE_MACRO_GROUP")}}
            if rng.random() < 0.4:
                spec["env"]["LBM_TUNE_TILE_GHOST_ROWS"] = "1"      # column blocks (py = 1) that keep ghost rows instead of wrapping in the launch
            child_env = {k: v for k, v in os.environ.items() if k not in KNOBS}
            child_env["GPU_MAX_HW_QUEUES"] = "16"        # whatever the caller's environment says: a queue per rank
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--tiles-case", json.dumps(spec)], capture_output=True, text=True, timeout=600, env=child_env)
            line = ([l for l in r.stdout.splitlines() if l.startswith("tiles ")] or ["tiles: no verdict"])[-1]
            if r.returncode != 0 or " ok" not in line:
                bad += 1
                print(f"MISMATCH case {case}: {line} spec {spec}\n{r.stderr[-1500:]}", flush=True)
            else:
                print(f"case {case}: {line}", flush=True)
            continue
        if kind in ("parts", "parts1"):
            size = int(rng.integers(2, 6))
            if kind == "parts" and ny < 32 * size + 3:
                ny = 32 * size + int(rng.integers(3, 40))
                obst = (rng.random((ny, nx)) < dens).astype(np.int32)
                p = lbm.Params(nx, ny, steps, 4, p.density, p.accel, p.omega)
            for k in KNOBS:
                os.environ.pop(k, None)
            os.environ.update(env)
            cells, av = run_partitions(p, obst, size, steps, kind == "parts")
            for k in KNOBS:
                os.environ.pop(k, None)
            os.environ.update({"LBM_TUNE_MULTI_K": "0", "LBM_TUNE_TILE_MAX": "0"})
            s1 = lbm.Simulation(p, obst)
            av1 = s1.run(steps)
            c1 = s1.local_cells().view(np.uint32).copy()
            s1.close()
            if cells is None:
                continue
            same = np.array_equal(cells, c1)
            avd = float(np.max(np.abs(av - av1) / np.maximum(np.abs(av1), 1e-30)))
            if not same or avd > 1e-6:
                bad += 1
                print(f"MISMATCH case {case}: {kind} x{size} {nx}x{ny} steps {steps} env {env} dens {dens} cells_same={same} av_rel={avd:.2e}", flush=True)
            elif case % 25 == 0:
                print(f"case {case}: {kind} x{size} {nx}x{ny} steps {steps} ok", flush=True)
            continue
        res = []
        for variant in ("fast", "one-step"):
            for k in KNOBS:
                os.environ.pop(k, None)
            flags, kw = 0, {}
            if variant == "fast":
                os.environ.update(env)
                flags = flags_fast
                if kind == "ring":                                   # 1-rank ring over the peer-to-peer or the RCCL loop
                    flags, kw = lbm._capi.FLAG_FORCE_HALO, {"exchange": str(rng.choice(["p2p", "rccl"])), "strict": True}
                if kind in ("multi", "tile", "ring"):                # the other forms of the sum|u| terms: populations must not move
                    flags |= int(rng.choice([0, 0, lbm._capi.FLAG_FAST_AVVELS, lbm._capi.FLAG_EXACT_AVVELS]))
            else:
                os.environ.update({"LBM_TUNE_MULTI_K": "0", "LBM_TUNE_TILE_MAX": "0"})
            s = lbm.Simulation(p, obst, flags=flags, **kw)
            desc = s.partition.describe()["kernel"] if variant == "fast" else None
            av = np.concatenate([s.run(steps // 2), s.run(steps - steps // 2)]) if steps > 1 else s.run(steps)
            res.append((s.local_cells().view(np.uint32).copy(), av, desc))
            s.close()
        same = np.array_equal(res[0][0], res[1][0])
        avd = float(np.max(np.abs(res[0][1] - res[1][1]) / np.maximum(np.abs(res[1][1]), 1e-30)))
        if not same or avd > 1e-6:
            bad += 1
            print(f"MISMATCH case {case}: {kind} {nx}x{ny} steps {steps} env {env} dens {dens} kernel {res[0][2]} cells_same={same} av_rel={avd:.2e}", flush=True)
        elif case % 25 == 0:
            print(f"case {case}: {kind} {nx}x{ny} steps {steps} {res[0][2]} ok", flush=True)
    print(f"{a.cases} cases, {bad} mismatches")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
