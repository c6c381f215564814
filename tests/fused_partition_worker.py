"""Ranks of one fused-arithmetic run (LBM_FLAG_FUSED_ARITH) as contexts of ONE process, one host thread per rank (test helper, run as
a fresh process by tests/test_fused_arith.py with GPU_MAX_HW_QUEUES raised, as tests/p2p_inprocess_worker.py).  The ranks' state
digests must add up to the digest of a single fused context of the same deck and steps, and the per-step sums must agree with its.
argv: rows <nx> <ny> <ranks> <runs>  |  tiles <nx> <ny> <px> <py> <runs>      (runs: comma separated step counts)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main() -> int:
    import mpilattice_boltzmann_amd as lbm
    kind, nx, ny = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
    fused = lbm._capi.FLAG_FUSED_ARITH
    if kind == "rows":
        size, runs = int(sys.argv[4]), [int(v) for v in sys.argv[5].split(",")]
    else:
        px, py, runs = int(sys.argv[4]), int(sys.argv[5]), [int(v) for v in sys.argv[6].split(",")]
        size = px * py
    steps = sum(runs)
    p = lbm.Params(nx, ny, steps, 4, 0.1, 0.01, 1.7)
    obst = lbm.synthetic_obstacles(nx, ny, 0.02, nx * 5 + ny, True)
    obst[ny - 2, 5:11] = 1                                          # blocked cells on the accelerate row
    free = lbm.count_free_cells(obst)
    if kind == "rows":
        lays = [lbm.rank_layout(p, size, r, fused) for r in range(size)]
        assert all(l["ny_local"] >= 32 for l in lays) and (size < 3 or len({l["ny_local"] for l in lays}) > 1), lays
        parts = [lbm.Partition(p, free, lbm.obstacle_window(obst, lays[r]), flags=fused, rank_of=(r, size)) for r in range(size)]
    else:
        lays = [lbm.tile_layout(p, px, py, r, fused) for r in range(size)]
        parts = [lbm.Partition(p, free, lbm.obstacle_window(obst, lays[r]), flags=fused, tile_of=(r, px, py)) for r in range(size)]
    for q in parts:
        d = q.describe()
        assert d["fused_arith"] and d["kernel"].startswith("lbm_multi_kernel<") and "fused arithmetic" in d["kernel"], d
    rings = lbm.P2PRing.local_ring(parts)
    out = [lbm.P2PRing.run_all(rings, n) for n in runs]
    for o in out:
        for r in range(1, size):
            assert np.array_equal(o[r], o[0])
    sums = np.concatenate([o[0] for o in out])
    digest = 0
    for q in parts:
        digest = (digest + q.checksum()) % (1 << 64)
    for ring in rings:
        ring.close()
    for q in parts:
        q.close()
    whole = lbm.Partition(p, free, obst, flags=fused)
    assert "fused" in whole.describe()["kernel"], whole.describe()
    whole.run(steps)
    ref_sums = whole.step_collect(steps)
    ref_digest = whole.checksum()
    exact = lbm.Partition(p, free, obst)
    exact.run(steps)
    exact_digest = exact.checksum()
    whole.close(); exact.close()
    assert digest == ref_digest, "the ranks' populations differ from a single fused context's"
    assert digest != exact_digest, "the fused run gave the exact arithmetic's bits"
    rel = np.max(np.abs(sums - ref_sums) / ref_sums)
    print(f"per-step sums against one context: {rel:.3e}")
    assert sums.shape == (steps,) and rel < 1e-12, rel
    print("FUSED PARTITIONS ok")
    return 0


if __name__ == "__main__":
    sys.exit(main())
