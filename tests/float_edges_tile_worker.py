"""The ranks of a px x py tile decomposition as contexts of ONE process on the states of tests/test_float_edges.py (test helper, run as
a fresh process by that module with GPU_MAX_HW_QUEUES raised, as tests/tile_inprocess_worker.py is).  Every state is written block by
block with set_cells, run for `steps` steps through the peer-to-peer loop, read back block by block and compared, assembled, with the
whole-grid reference by the module's rules.
argv: nx ny px py K ghost steps"""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main() -> int:
    nx, ny, px, py, K, ghost, steps = (int(v) for v in sys.argv[1:8])
    for knob in ("LBM_TUNE_TILE_GHOST_ROWS", "LBM_P2P_SCHEDULE", "LBM_TUNE_MACRO_GROUP"):
        os.environ.pop(knob, None)
    os.environ["LBM_TUNE_MACRO_K"] = str(K)
    os.environ["LBM_TUNE_MACRO_GHOST"] = str(ghost)
    import mpilattice_boltzmann_amd as lbm
    import test_float_edges as fe
    size = px * py
    p, obst = fe._deck(nx, ny)
    lp = lbm.Params(nx, ny, p.max_iters, p.reynolds_dim, p.density, p.accel, p.omega)
    free = lbm.count_free_cells(obst)
    lays = [lbm.tile_layout(lp, px, py, r, 0) for r in range(size)]
    groups = lbm.plan_groups(lays[0]["macro_k"], lays[0]["ghost"], lays[0]["group"], steps)
    assert len(groups) >= 2 and len(groups[0]) >= 2, groups                   # a group of launches and a tail
    assert lays[0]["ghost_x"] > 0 and (lays[0]["ghost_y"] > 0) == (py > 1), lays[0]
    parts = [lbm.Partition(lp, free, lbm.obstacle_window(obst, lays[r]), tile_of=(r, px, py)) for r in range(size)]
    assert all(q.describe()["kernel"] == f"lbm_multi_kernel<{K}>" for q in parts), parts[0].describe()
    rings = lbm.P2PRing.local_ring(parts)
    assert f"tiles {px} x {py}" in rings[0].describe(), rings[0].describe()
    for state in fe.STATES:
        name = fe.state_for(state, nx, ny, steps)
        cells0 = fe._state(name, nx, ny)
        ref, terms = fe._reference(name, nx, ny, steps)
        for q, l in zip(parts, lays):
            q.set_cells(cells0[l["y0"]:l["y0"] + l["ny_local"], l["x0"]:l["x0"] + l["nx_local"]])
        with np.errstate(all="ignore"):
            out = lbm.P2PRing.run_all(rings, steps)
        for r in range(1, size):                                 # the reduction is bitwise the same on every rank
            assert np.array_equal(out[r], out[0], equal_nan=True)
        cells = np.empty((ny, nx, 9), np.float32)
        for q, l in zip(parts, lays):
            cells[l["y0"]:l["y0"] + l["ny_local"], l["x0"]:l["x0"] + l["nx_local"]] = q.get_cells()
        what = f"{px} x {py} tile ranks of {nx}x{ny}, K = {K}, {name} {steps} steps"
        fe._compare_cells(cells, ref, what)
        counts = fe._compare_sums(np.asarray(out[0], np.float64), terms, obst, "parts", "compensated", what, functools.partial(fe._inputs, name, nx, ny),
                                  extra=size - 2)
        if name in ("W1", "blocks"):
            assert counts[3] == 0, counts
        if name == "W1":
            assert counts == (0, 0, steps, 0), counts
    for ring in rings:
        ring.close()
    for q in parts:
        q.close()
    print(f"EDGE TILES ok {px}x{py}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
