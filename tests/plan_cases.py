"""The fixed table of contexts whose kernel, sizes and launches are pinned (tests/golden/plans_parent.json), and the
recorder that reads them off live contexts through the public Python API only.

  python tests/plan_cases.py OUT.json [COMMIT]     record on the GPU (COMMIT goes into the file)

tests/test_plan.py replays the table on a CPU through the library's planning entry points; its GPU test runs the
recorder again and compares row for row.
"""
from __future__ import annotations

import json
import os
import sys

STEPS = 11     # run length of the recorded launch lists

WHOLE = [(128, 128), (128, 256), (256, 256), (512, 256), (512, 512), (768, 768), (1024, 1024), (2048, 2048), (64, 16), (130, 100),
         (100, 100), (127, 64), (96, 2048), (100, 40000)]
RINGS = [(1024, 128), (1024, 64), (1024, 31), (2048, 1024)]                      # one-rank rings, FLAG_FORCE_HALO
TILES = [(512, 512, 1, 1), (512, 512, 2, 1), (1024, 512, 2, 2)]                  # every rank of each
FLAGGED = [(512, 512, f) for f in ("FLAG_FAST_AVVELS", "FLAG_EXACT_AVVELS", "FLAG_FUSED_ARITH", "FLAG_ONE_STEP", "FLAG_NT_STORES")] + \
          [(128, 128, "FLAG_FUSED_ARITH"), (128, 128, "FLAG_FAST_AVVELS")]
# each knob on the whole grids whose plan it moves (and one it must leave alone)
KNOBS = [("LBM_TUNE_MULTI_K", "3", [(1024, 1024), (512, 512), (256, 256)]),
         ("LBM_TUNE_TILE_GEOM", "164", [(256, 256), (128, 128), (512, 512)]),
         ("LBM_TUNE_MULTI_GEOM", "0", [(1024, 1024), (130, 100)]),
         ("LBM_TUNE_NARROW_MAX", "0", [(100, 100), (127, 64)]),
         ("LBM_TUNE_TILE_MAX", "0", [(256, 256), (128, 128), (64, 16)])]


def cases() -> list[dict]:
    """One dict per context: kind, nx, ny, flags (names), env, and px / py / rank for tile ranks."""
    out = [{"kind": "whole", "nx": nx, "ny": ny, "flags": [], "env": {}} for nx, ny in WHOLE]
    out += [{"kind": "ring", "nx": nx, "ny": ny, "flags": ["FLAG_FORCE_HALO"], "env": {}} for nx, ny in RINGS]
    out += [{"kind": "tile", "nx": nx, "ny": ny, "flags": [], "env": {}, "px": px, "py": py, "rank": r}
            for nx, ny, px, py in TILES for r in range(px * py)]
    out += [{"kind": "whole", "nx": nx, "ny": ny, "flags": [f], "env": {}} for nx, ny, f in FLAGGED]
    out += [{"kind": "whole", "nx": nx, "ny": ny, "flags": [], "env": {knob: value}} for knob, value, shapes in KNOBS for nx, ny in shapes]
    return out


def flags_of(lbm, case: dict) -> int:
    flags = 0
    for name in case["flags"]:
        flags |= getattr(lbm._capi, name)
    return flags


def params_of(lbm, case: dict):
    return lbm.Params(nx=case["nx"], ny=case["ny"], max_iters=STEPS, reynolds_dim=10, density=0.1, accel=0.005, omega=1.85)


def record_case(lbm, case: dict) -> dict:
    """Create the case's context and read everything the public API shows of its plan."""
    import numpy as np
    from mpilattice_boltzmann_amd import host
    p, flags = params_of(lbm, case), flags_of(lbm, case)
    obst = np.zeros((p.ny, p.nx), dtype=np.int32)
    free = p.nx * p.ny
    saved = {k: os.environ.get(k) for k in case["env"]}
    os.environ.update(case["env"])
    try:
        if case["kind"] == "whole":
            part = host.Partition(p, free, obst, 0, 0, flags)
        elif case["kind"] == "ring":
            part = host.Partition(p, free, host.obstacle_window(obst, host.rank_layout(p, 1, 0, flags)), device=0, flags=flags, rank_of=(0, 1))
        else:
            lay = host.tile_layout(p, case["px"], case["py"], case["rank"], flags)
            part = host.Partition(p, free, host.obstacle_window(obst, lay), device=0, flags=flags, tile_of=(case["rank"], case["px"], case["py"]))
        row = dict(case)
        d = part.describe()
        row.update(kernel=d["kernel"], cells_per_launch=d["cells_per_launch"], state_bytes=d["state_bytes"], halo_floats=part.halo_floats,
                   macro_pack_floats=part.macro_pack_floats, macro_pack_floats_x=part.macro_pack_floats_x)
        if case["kind"] == "tile":
            row["tile_info"] = part.tile_info()
        if case["kind"] == "whole":
            part.set_profile(True)
            part.run(STEPS)
            row["launch_steps"] = [s for s, _ in part.launch_profile()]
        part.close()
        return row
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def record(lbm, commit: str = "") -> dict:
    return {"commit": commit, "steps": STEPS, "rows": [record_case(lbm, c) for c in cases()]}


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import mpilattice_boltzmann_amd as pkg
    pkg.build()
    doc = record(pkg, sys.argv[2] if len(sys.argv) > 2 else "")
    with open(sys.argv[1], "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(f"recorded {len(doc['rows'])} contexts")
