"""The px x py tile grid of tests/test_tile_split_phase.py's fused-arithmetic case on a peer-to-peer ring of ONE process, one host thread
per rank (test helper, run as a fresh process with GPU_MAX_HW_QUEUES raised, as tests/tile_inprocess_worker.py: ranks that share a device
need a hardware queue each).  Prints one JSON line: the ranks' summed state digest, and the digest the exact arithmetic gives.
argv: nx ny px py runs(comma separated)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main() -> int:
    import mpilattice_boltzmann_amd as lbm
    nx, ny, px, py = (int(v) for v in sys.argv[1:5])
    runs = [int(v) for v in sys.argv[5].split(",")]
    for k in ("LBM_TUNE_MACRO_K", "LBM_TUNE_MACRO_GHOST", "LBM_TUNE_MACRO_GROUP", "LBM_TUNE_TILE_GHOST_ROWS", "LBM_TUNE_TILE_GHOST_X", "LBM_P2P_SCHEDULE"):
        os.environ.pop(k, None)
    fused = lbm._capi.FLAG_FUSED_ARITH
    p = lbm.Params(nx, ny, sum(runs), 4, 0.1, 0.01, 1.7)
    obst = lbm.synthetic_obstacles(nx, ny, 0.03, nx * 5 + ny, False)          # the deck of test_tile_split_phase._deck
    free = lbm.count_free_cells(obst)
    size = px * py
    lays = [lbm.tile_layout(p, px, py, r, fused) for r in range(size)]
    parts = [lbm.Partition(p, free, lbm.obstacle_window(obst, lays[r]), flags=fused, tile_of=(r, px, py)) for r in range(size)]
    rings = lbm.P2PRing.local_ring(parts)
    for n in runs:
        lbm.P2PRing.run_all(rings, n)
    digest = sum(q.checksum() for q in parts) % (1 << 64)
    for ring in rings:
        ring.close()
    for q in parts:
        q.close()
    with lbm.Partition(p, free, obst) as exact:
        exact.run(sum(runs))
        exact_digest = exact.checksum()
    print(json.dumps({"digest": digest, "exact_digest": exact_digest}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
