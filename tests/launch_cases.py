"""The fixed table of runs whose step-kernel dispatches are pinned (tests/golden/launches_parent.json), and the recorder that
makes them on a GPU under a kernel trace and reads the trace back.

  rocprofv3 --kernel-trace --output-format csv -d DIR -- python tests/launch_cases.py run     every case once, STEPS steps, one thread
  python tests/launch_cases.py collect DIR OUT.json [COMMIT]     the lbm_multi_kernel / lbm_tile_kernel dispatches, per case
  python tests/launch_cases.py listing DIR OUT.txt               every dispatch of the trace, one line each (profiles/rNN/kernel_trace_*.txt)

A case is one context — or, for a tile grid of several ranks, all of them, stepped together.  Every context creation launches
lbm_init_kernel exactly once and nothing else does, which is how `collect` cuts the trace into cases.  tests/test_launch_plan.py
replays the recording on a CPU from the library's LaunchPlans.
"""
from __future__ import annotations

import csv
import glob
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plan_cases  # noqa: E402

STEPS = plan_cases.STEPS
WHOLE = [s for s in plan_cases.WHOLE if s[0] * s[1] <= 1024 * 1024]
RINGS = plan_cases.RINGS
SCHEDULES = ("serial", "edge")
# names of tests/test_tile_split_phase.py's LAYOUTS: nx, ny, px, py, knobs
TILES = {"256x128_1x1": (256, 128, 1, 1, {}),
         "256x128_1x1_yghost": (256, 128, 1, 1, {"LBM_TUNE_TILE_GHOST_ROWS": "1"}),
         "128x32_1x1_yghost": (128, 32, 1, 1, {"LBM_TUNE_TILE_GHOST_ROWS": "1"}),
         "224x64_2x1": (224, 64, 2, 1, {})}
TUNE = ("LBM_TUNE_MACRO_K", "LBM_TUNE_MACRO_GHOST", "LBM_TUNE_MACRO_GROUP", "LBM_TUNE_TILE_GHOST_ROWS", "LBM_TUNE_TILE_GHOST_X", "LBM_P2P_SCHEDULE",
        "LBM_TUNE_MULTI_REMAP", "LBM_TUNE_TILE_PAD_GRID")
FAMILIES = re.compile(r"lbm_(multi|tile)_kernel<")


def cases() -> list[dict]:
    """One dict per case: kind, nx, ny, env, contexts (how many it creates), and schedule (rings) or name / px / py (tiles)."""
    out = [{"kind": "whole", "nx": nx, "ny": ny, "env": {}, "contexts": 1} for nx, ny in WHOLE]
    out += [{"kind": "ring", "nx": nx, "ny": ny, "env": {"LBM_P2P_SCHEDULE": s}, "schedule": s, "contexts": 1} for nx, ny in RINGS for s in SCHEDULES]
    out += [{"kind": "tiles", "name": name, "nx": nx, "ny": ny, "px": px, "py": py, "env": dict(env), "contexts": px * py}
            for name, (nx, ny, px, py, env) in TILES.items()]
    return out


def params_of(lbm, case: dict):
    return plan_cases.params_of(lbm, case)


def run_case(lbm, case: dict) -> None:
    import numpy as np
    from mpilattice_boltzmann_amd import host
    p = params_of(lbm, case)
    obst = np.zeros((p.ny, p.nx), dtype=np.int32)
    free = p.nx * p.ny
    if case["kind"] == "whole":
        with host.Partition(p, free, obst, 0, 0, 0) as part:
            part.run(STEPS)
    elif case["kind"] == "ring":
        flags = lbm._capi.FLAG_FORCE_HALO
        part = host.Partition(p, free, host.obstacle_window(obst, host.rank_layout(p, 1, 0, flags)), device=0, flags=flags, rank_of=(0, 1))
        ring = host.P2PRing.local_ring([part])[0]
        ring.run(STEPS)
        ring.close()
        part.close()
    else:
        px, py = case["px"], case["py"]
        lays = [host.tile_layout(p, px, py, r, 0) for r in range(px * py)]
        parts = [host.Partition(p, free, host.obstacle_window(obst, lays[r]), device=0, tile_of=(r, px, py)) for r in range(px * py)]
        nbs = [q.tile_neighbours() for q in parts]
        for q in parts:
            q.tile_prepare(STEPS)
        done = 0
        while done < STEPS:            # tests/test_tile_split_phase.py's _exchange and _step_tiles, interior + edge
            for q in parts:
                q.macro_pack_x()
            for q, nb in zip(parts, nbs):
                q.macro_receive_from_x(parts[nb["west"]], 1)
                q.macro_receive_from_x(parts[nb["east"]], 0)
            for q in parts:
                q.macro_unpack_x()
            if parts[0].macro_pack_floats:
                for q in parts:
                    q.macro_pack()
                for q, nb in zip(parts, nbs):
                    q.macro_receive_from_y(parts[nb["south"]], 1)
                    q.macro_receive_from_y(parts[nb["north"]], 0)
                for q in parts:
                    q.macro_unpack()
            for q in parts:
                q.macro_interior()
                q.macro_edge()
            done += parts[0].macro_next
            for q in parts:
                q.macro_finish()
        for q in parts:
            q.step_collect(STEPS)
            q.close()


def run_all(lbm) -> None:
    import torch
    for case in cases():
        for k in TUNE:
            os.environ.pop(k, None)
        os.environ.update(case["env"])
        run_case(lbm, case)
        torch.cuda.synchronize()
    for k in TUNE:
        os.environ.pop(k, None)


def read_trace(path: str) -> list[dict]:
    """Every dispatch of a rocprofv3 kernel trace (a csv file, or a directory that holds one), in order of its start."""
    files = [path] if os.path.isfile(path) else sorted(glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True))
    assert len(files) == 1, f"one kernel trace expected under {path}: {files}"
    with open(files[0], newline="") as fh:
        rows = list(csv.DictReader(fh))
    rows.sort(key=lambda r: (int(r["Start_Timestamp"]), int(r.get("Dispatch_Id", 0) or 0)))
    return [{"kernel": r["Kernel_Name"], "grid": [int(r[f"Grid_Size_{a}"]) for a in "XYZ"], "workgroup": [int(r[f"Workgroup_Size_{a}"]) for a in "XYZ"],
             "lds": int(r.get("LDS_Block_Size", 0) or 0)} for r in rows]


def collect(path: str, commit: str = "") -> dict:
    rows = read_trace(path)
    inits = [i for i, r in enumerate(rows) if "lbm_init_kernel" in r["kernel"]]
    table = cases()
    assert len(inits) == sum(c["contexts"] for c in table), (len(inits), "context creations in the trace")
    out, first = [], 0
    for case in table:
        begin = inits[first]
        first += case["contexts"]
        end = inits[first] if first < len(inits) else len(rows)
        row = dict(case)
        row["dispatches"] = [[r["kernel"], r["grid"][0], r["workgroup"][0]] for r in rows[begin:end] if FAMILIES.search(r["kernel"])]
        assert all(r["grid"][1:] == [1, 1] and r["workgroup"][1:] == [1, 1] for r in rows[begin:end] if FAMILIES.search(r["kernel"]))
        out.append(row)
    return {"commit": commit, "steps": STEPS, "rows": out}


if __name__ == "__main__":
    if sys.argv[1] == "run":
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        import mpilattice_boltzmann_amd as pkg
        pkg.build()
        run_all(pkg)
        print(f"ran {len(cases())} cases")
    elif sys.argv[1] == "collect":
        doc = collect(sys.argv[2], sys.argv[4] if len(sys.argv) > 4 else "")
        with open(sys.argv[3], "w") as fh:                            # one case per line
            fh.write('{"commit": %s, "steps": %d, "rows": [\n' % (json.dumps(doc["commit"]), doc["steps"]))
            fh.write(",\n".join(json.dumps(r) for r in doc["rows"]))
            fh.write("\n]}\n")
        print(f"collected {sum(len(r['dispatches']) for r in doc['rows'])} dispatches of {len(doc['rows'])} cases")
    elif sys.argv[1] == "listing":
        with open(sys.argv[3], "w") as fh:
            fh.write("# kernel name | grid (x y z) | workgroup (x y z) | LDS bytes — one line per dispatch, in order\n")
            for r in read_trace(sys.argv[2]):
                fh.write(f"{r['kernel']} | {' '.join(map(str, r['grid']))} | {' '.join(map(str, r['workgroup']))} | {r['lds']}\n")
    else:
        raise SystemExit(__doc__)
