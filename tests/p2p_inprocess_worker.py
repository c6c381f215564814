"""Several ranks of one peer-to-peer run as contexts of ONE process, one host thread per rank (test helper, run
as a fresh process by tests/test_gpu_parity.py with GPU_MAX_HW_QUEUES raised: ranks that share a device need a
hardware queue each — see lbm_p2p_connect).  argv: nx ny size K schedule [runs=<steps,...>] [max_iters=<n>] [want=<ghost>,<group>]
(runs: default 20,11; max_iters: the deck's step count the contexts are created with — below the longest run, the per-step sums
buffers grow between runs; want: the layout every rank must have)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main() -> int:
    nx, ny, size, K = (int(v) for v in sys.argv[1:5])
    opts = dict(a.split("=", 1) for a in sys.argv[6:])
    runs = [int(v) for v in opts.get("runs", "20,11").split(",")]
    steps = sum(runs)
    max_iters = int(opts.get("max_iters", steps))
    os.environ["LBM_TUNE_MACRO_K"] = str(K)
    os.environ["LBM_P2P_SCHEDULE"] = sys.argv[5]
    import mpilattice_boltzmann_amd as lbm
    import oracle_lib
    p = lbm.Params(nx, ny, max_iters, 4, 0.1, 0.01, 1.7)
    obst = lbm.synthetic_obstacles(nx, ny, 0.03, nx * 5 + ny, False)
    free = lbm.count_free_cells(obst)
    lays = [lbm.rank_layout(p, size, r) for r in range(size)]
    assert all(l["macro_k"] == K for l in lays), lays
    if "want" in opts:
        assert all([l["ghost"], l["group"]] == [int(v) for v in opts["want"].split(",")] for l in lays), lays
    parts = [lbm.Partition(p, free, lbm.obstacle_window(obst, lays[r]), rank_of=(r, size)) for r in range(size)]
    rings = lbm.P2PRing.local_ring(parts)
    assert all("serial" in r.describe() and "in-process" in r.describe() for r in rings), rings[0].describe()
    out = [lbm.P2PRing.run_all(rings, n) for n in runs]
    for o in out:
        for r in range(1, size):                                # the reduction is bitwise the same on every rank
            assert np.array_equal(o[r], o[0])
    cells = np.concatenate([q.get_cells() for q in parts], axis=0)
    for ring in rings:
        ring.close()
    for q in parts:
        q.close()
    ref_cells, _, ref_exact = oracle_lib.run(lbm.Params(nx, ny, steps, 4, 0.1, 0.01, 1.7), obst, steps, nthreads=4)
    assert np.array_equal(cells.view(np.uint32), ref_cells.view(np.uint32))
    av = np.concatenate([o[0] for o in out]) * np.float64(np.float32(1.0) / np.float32(free))
    assert av.shape == (steps,) and np.max(np.abs(av - ref_exact) / ref_exact) < 1e-12
    print("IN-PROCESS RING ok")
    return 0


if __name__ == "__main__":
    sys.exit(main())
