"""One rank of a tile (2-D) decomposition stepped by the RCCL loop, one GPU per rank (test helper, launched by torch.distributed.run
from tests/test_tile_split_phase.py on a box with several GPUs; the pattern of tests/p2p_worker.py, whose tile cases belong to the
peer-to-peer loop).  The ranks form a gloo group, Simulation hands rank 0's RCCL id to every rank; rank 0 compares the ranks' summed
state digest with a single-GPU run of the deck and the gathered populations with the oracle.

    python -m torch.distributed.run --nproc-per-node N ... tests/tile_rccl_worker.py '<json list of cases>'
case = {"nx", "ny", "grid": [px, py], "walls", "schedule" ("edge" | "serial" | ""), "step_allreduce", "runs" (default [19, 7])}"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main() -> int:
    import torch
    import torch.distributed as dist
    import mpilattice_boltzmann_amd as lbm
    import oracle_lib
    cases = json.loads(sys.argv[1])
    device = int(os.environ["LOCAL_RANK"])
    torch.cuda.set_device(device)
    dist.init_process_group("gloo")
    rank, size = dist.get_rank(), dist.get_world_size()
    print(f"RANK {rank} UP", flush=True)          # the group exists: whatever happens from here on is a verdict, never retried (conftest.py)
    bad = 0
    for i, c in enumerate(cases):
        if c.get("schedule"):
            os.environ["LBM_RCCL_SCHEDULE"] = c["schedule"]
        else:
            os.environ.pop("LBM_RCCL_SCHEDULE", None)
        runs = c.get("runs", [19, 7])
        total = sum(runs)
        px, py = c["grid"]
        p = lbm.Params(c["nx"], c["ny"], total, 4, 0.1, 0.01, 1.7)
        obst = lbm.synthetic_obstacles(p.nx, p.ny, 0.03, p.nx * 5 + p.ny, bool(c.get("walls")))
        sim = lbm.Simulation(p, obst, device=device, distributed=True, exchange="rccl", strict=True, step_allreduce=bool(c.get("step_allreduce")),
                             rank_grid=(px, py))
        d = sim.describe()
        assert d["loop"] == "rccl" and d["rccl_nranks"] == size == px * py and d["step_allreduce"] == bool(c.get("step_allreduce")), d
        info = sim.partition.tile_info()
        assert (info["px"], info["py"], info["ry"] * px + info["rx"]) == (px, py, rank) and info["ghost_x"] > 0, info
        av = np.concatenate([sim.run(n) for n in runs])
        everyone = [None] * size
        dist.all_gather_object(everyone, av.tobytes())
        same_av = all(b == everyone[0] for b in everyone)          # the reduction is bitwise the same on every rank
        digests = [None] * size
        dist.all_gather_object(digests, sim.partition.checksum())
        cells = sim.gather_cells()
        sim.close()
        ok = True
        if rank == 0:
            ref_cells, _, ref_exact = oracle_lib.run(p, obst, total, nthreads=4)
            ok = bool(np.array_equal(cells.view(np.uint32), ref_cells.view(np.uint32)))
            err = float(np.max(np.abs(av.astype(np.float64) - ref_exact) / ref_exact))
            ok = ok and err < 1e-6 and same_av
            whole = lbm.Simulation(p, obst, device=device)         # the single-GPU digest: the ranks' digests add up to it
            whole.run(total)
            ok = ok and (sum(digests) % (1 << 64)) == whole.partition.checksum()
            whole.close()
            print(f"CASE {i} {'ok' if ok else 'FAILED'} ranks={size} {c} av_err={err:.2e} same_av={same_av}", flush=True)
        flag = [ok]
        dist.broadcast_object_list(flag, src=0)
        bad += 0 if flag[0] else 1
    dist.barrier()
    dist.destroy_process_group()
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
