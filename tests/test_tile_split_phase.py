"""Ranks of the tile (2-D) decomposition stepped through the split-phase calls (lbm_tile_prepare, lbm_macro_pack_x / lbm_macro_unpack_x,
lbm_macro_pack / lbm_macro_unpack on storage rows, lbm_macro_exchange_local_x / _y) and through the RCCL loop, include/lbm_d2q9.h and
include/lbm_d2q9_rccl.h: the packed two-phase exchange — columns first, then whole storage rows, which carries the corners — against the
oracle bit for bit, the message layout against the numpy slices the header documents, the neighbour rule against numpy.roll."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

AV_EXACT_RTOL = 1e-6
RUNS = (19, 7)                       # the second run prepares again and ends on the 3 / 4 tail split
TUNE = ("LBM_TUNE_MACRO_K", "LBM_TUNE_MACRO_GHOST", "LBM_TUNE_MACRO_GROUP", "LBM_TUNE_TILE_GHOST_ROWS", "LBM_TUNE_TILE_GHOST_X", "LBM_RCCL_SCHEDULE")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# deck, rank grid, knobs, then the layout the case is named for (checked before anything runs: a change of the layout rule shows up as a
# layout failure): macro_k, ghost, ghost_x, ghost_y, launches per exchange, owned columns per rank-grid column, owned rows per rank-grid row
LAYOUTS = {
    "256x128_2x2": (256, 128, 2, 2, {}, dict(macro_k=4, ghost=8, ghost_x=8, ghost_y=8, group=2), [128, 128], [64, 64]),
    "256x64_2x2": (256, 64, 2, 2, {}, dict(ghost=4, ghost_x=4, ghost_y=4, group=1), [128, 128], [32, 32]),
    "388x134_3x2": (388, 134, 3, 2, {}, dict(ghost=8, ghost_x=8, ghost_y=8), [130, 130, 128], [67, 67]),
    "388x134_3x2_k3": (388, 134, 3, 2, {"LBM_TUNE_MACRO_K": "3"}, dict(macro_k=3, ghost=8, ghost_x=8, ghost_y=8), [130, 130, 128], [67, 67]),
    "388x100_3x3": (388, 100, 3, 3, {}, dict(ghost=4, ghost_x=4, ghost_y=4), [130, 130, 128], [34, 33, 33]),       # (the reference's rule deals the spare row to the first rank)
    "388x100_3x1": (388, 100, 3, 1, {}, dict(ghost=8, ghost_x=8, ghost_y=0), [130, 130, 128], [100]),
    "224x64_2x1": (224, 64, 2, 1, {}, dict(ghost_x=8, ghost_y=0), [112, 112], [64]),
    "224x96_1x2": (224, 96, 1, 2, {}, dict(), [224], [48, 48]),
    "256x128_2x2_ghost7": (256, 128, 2, 2, {"LBM_TUNE_MACRO_GHOST": "7"}, dict(ghost=7, ghost_x=8, ghost_y=7, group=1), [128, 128], [64, 64]),
    "256x128_1x1": (256, 128, 1, 1, {}, dict(ghost=32, ghost_x=32, ghost_y=0, group=8), [256], [128]),
    "256x128_1x1_yghost": (256, 128, 1, 1, {"LBM_TUNE_TILE_GHOST_ROWS": "1"}, dict(ghost=16, ghost_x=16, ghost_y=16, group=4), [256], [128]),
    "128x32_1x1_yghost": (128, 32, 1, 1, {"LBM_TUNE_TILE_GHOST_ROWS": "1"}, dict(ghost=4, ghost_x=4, ghost_y=4), [128], [32]),
}
WALLS = {"388x134_3x2", "224x96_1x2", "256x128_1x1_yghost"}


def _set_knobs(monkeypatch, env):
    for k in TUNE:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _deck(lbm, name, flags=0):
    nx, ny, px, py, env, want, cols, rows = LAYOUTS[name]
    p = lbm.Params(nx, ny, sum(RUNS), 4, 0.1, 0.01, 1.7)
    obst = lbm.synthetic_obstacles(nx, ny, 0.03, nx * 5 + ny, name in WALLS)
    lays = [lbm.tile_layout(p, px, py, r, flags) for r in range(px * py)]
    for r, lay in enumerate(lays):
        for key, val in want.items():
            assert lay[key] == val, (name, r, key, lay)
        assert (lay["nx_local"], lay["ny_local"]) == (cols[r % px], rows[r // px]), (name, r, lay)
        assert lay["ghost_y"] == (0 if py == 1 and "LBM_TUNE_TILE_GHOST_ROWS" not in env else lay["ghost"]), (name, lay)
    return p, obst, lays


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """The oracle's run of a case's deck, computed once and shared (read-only) by the tests that need it."""
    import mpilattice_boltzmann_amd as lbm
    import oracle_lib
    nx, ny = LAYOUTS[name][:2]
    p = lbm.Params(nx, ny, sum(RUNS), 4, 0.1, 0.01, 1.7)
    obst = lbm.synthetic_obstacles(nx, ny, 0.03, nx * 5 + ny, name in WALLS)
    cells, _, exact = oracle_lib.run(p, obst, sum(RUNS), nthreads=4)
    cells.setflags(write=False)
    exact.setflags(write=False)
    return cells, exact


# ---- 1. the neighbour rule (no GPU) ----------------------------------------------------------------------------------------------

def test_tile_neighbours_are_the_periodic_rank_grid(lbm):
    for px in range(1, 6):
        for py in range(1, 6):
            grid = np.arange(px * py).reshape(py, px)
            want = dict(south=np.roll(grid, 1, axis=0), north=np.roll(grid, -1, axis=0), west=np.roll(grid, 1, axis=1), east=np.roll(grid, -1, axis=1))
            for rank in range(px * py):
                got = lbm.tile_neighbours(px, py, rank)
                assert got == {k: int(v[rank // px, rank % px]) for k, v in want.items()}, (px, py, rank, got)
    for bad in ((0, 1, 0), (1, 0, 0), (2, 2, 4), (2, 2, -1), (-1, -1, 0)):
        with pytest.raises(lbm.LbmError, match="lbm_tile_neighbours: bad argument"):
            lbm.tile_neighbours(*bad)
    lib = lbm.load_library()
    assert lib.lbm_tile_neighbours(2, 2, 0, None) != 0


# ---- 2. whole tile grids through the split-phase calls, one process, one stream ---------------------------------------------------

def _exchange(parts, nbs, st):
    """One packed exchange of every rank, as a caller with its own communicator makes it: columns first, then (ranks with ghost rows)
    whole storage rows; the messages move by device copies between the ranks' buffers."""
    for q in parts:
        q.macro_pack_x(st)
    for q, nb in zip(parts, nbs):
        q.macro_receive_from_x(parts[nb["west"]], 1, st)       # the west neighbour's east-going message: my incoming from the west
        q.macro_receive_from_x(parts[nb["east"]], 0, st)
    for q in parts:
        q.macro_unpack_x(st)
    if parts[0].macro_pack_floats == 0:                        # column blocks: the rows wrap inside the launch
        return
    for q in parts:
        q.macro_pack(st)
    for q, nb in zip(parts, nbs):
        q.macro_receive_from_y(parts[nb["south"]], 1, st)      # the south neighbour's north-going message: my incoming from the south
        q.macro_receive_from_y(parts[nb["north"]], 0, st)
    for q in parts:
        q.macro_unpack(st)


def _step_tiles(lbm, parts, steps, one_launch):
    """`steps` iterations of every rank of a tile grid through the split-phase calls; returns the summed per-step tot_u."""
    import torch
    lay0 = parts[0].tile_info()
    plan = lbm.plan_groups(lay0["macro_k"], lay0["ghost"], lay0["group"], steps)
    nbs = [q.tile_neighbours() for q in parts]
    seen = []
    tstream = torch.cuda.Stream(torch.device("cuda", 0))
    st = tstream.cuda_stream
    with torch.cuda.stream(tstream):
        for q in parts:
            q.tile_prepare(steps, st)
        done = 0
        while done < steps:
            _exchange(parts, nbs, st)
            for q in parts:
                if one_launch:
                    q.macro_all(st)
                else:
                    q.macro_interior(st)
                    q.macro_edge(st)
            k, n = parts[0].macro_next, parts[0].macro_launches
            assert 1 <= k <= 32 and all(q.macro_next == k and q.macro_launches == n for q in parts)
            seen.append((k, n))
            for q in parts:
                q.macro_finish(st)
            done += k
        sums = sum(q.step_collect(steps, st) for q in parts)
    tstream.synchronize()
    assert seen == [(sum(g), len(g)) for g in plan], (seen, plan)
    return sums


GRID_CASES = [n for n in LAYOUTS if n != "128x32_1x1_yghost"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", GRID_CASES)
def test_tile_grid_through_the_split_phase_calls(lbm, monkeypatch, name):
    """Every rank of the grid as a context of this process: runs of 19 and 7 steps, populations bit for bit the oracle's, per-step
    sums, the groups lbm_plan_group gives, digests that add up to one whole context's.  Half the cases make the first launch of a
    group as interior + edge, the other half as one launch."""
    _set_knobs(monkeypatch, LAYOUTS[name][4])
    p, obst, lays = _deck(lbm, name)
    if name == "388x134_3x2_k3":
        assert lbm.plan_groups(3, 8, lays[0]["group"], RUNS[0])[:2] == [[4, 3], [3, 3]]
    px, py = LAYOUTS[name][2:4]
    free = lbm.count_free_cells(obst)
    ref_cells, ref_exact = _oracle(name)
    parts = [lbm.Partition(p, free, lbm.obstacle_window(obst, lays[r]), tile_of=(r, px, py)) for r in range(px * py)]
    try:
        assert all(q.tile_info() == lays[r] for r, q in enumerate(parts))
        assert {int(q.macro_pack_floats_x) for q in parts} == {9 * l["ny_local"] * l["ghost_x"] for l in lays}
        one_launch = GRID_CASES.index(name) % 2 == 1
        sums = np.concatenate([_step_tiles(lbm, parts, n, one_launch) for n in RUNS])
        cells = np.empty((p.ny, p.nx, 9), dtype=np.float32)
        digest = 0
        for q, l in zip(parts, lays):
            cells[l["y0"]:l["y0"] + l["ny_local"], l["x0"]:l["x0"] + l["nx_local"]] = q.get_cells()
            digest = (digest + q.checksum()) % (1 << 64)
    finally:
        for q in parts:
            q.close()
    assert np.array_equal(bits(cells), bits(ref_cells)), "populations differ from the oracle"
    av = sums * np.float64(np.float32(1.0) / np.float32(free))
    err = np.max(np.abs(av - ref_exact) / ref_exact)
    print(f"{name}: av_vels against the oracle {err:.3e}")
    assert av.shape == (sum(RUNS),) and err < AV_EXACT_RTOL
    with lbm.Partition(p, free, obst) as whole:
        whole.run(sum(RUNS))
        assert digest == whole.checksum()


@pytest.mark.gpu
def test_fused_arithmetic_gives_the_peer_to_peer_ring_its_bits(lbm, monkeypatch):
    """LBM_FLAG_FUSED_ARITH promises the same bits whatever advances the state: the 2 x 2 grid through the split-phase calls against the
    same grid on a peer-to-peer ring of this box (tests/tile_fused_ring_worker.py: a ring of four ranks on one device needs a hardware
    queue per rank, hence a fresh process)."""
    name = "256x128_2x2"
    _set_knobs(monkeypatch, {})
    fused = lbm._capi.FLAG_FUSED_ARITH
    p, obst, lays = _deck(lbm, name, fused)
    free = lbm.count_free_cells(obst)
    parts = [lbm.Partition(p, free, lbm.obstacle_window(obst, lays[r]), flags=fused, tile_of=(r, 2, 2)) for r in range(4)]
    try:
        assert all("fused arithmetic" in q.describe()["kernel"] for q in parts)
        for n in RUNS:
            _step_tiles(lbm, parts, n, False)
        digest = sum(q.checksum() for q in parts) % (1 << 64)
    finally:
        for q in parts:
            q.close()
    env = dict(os.environ, GPU_MAX_HW_QUEUES="16", LBM_P2P_TIMEOUT_MS="10000")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tile_fused_ring_worker.py"), "256", "128", "2", "2", ",".join(str(n) for n in RUNS)],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    ring = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert digest == ring["digest"] and digest != ring["exact_digest"], (digest, ring)


# ---- 3. the message layout against the header's words -----------------------------------------------------------------------------

def _encoded(nx, ny):
    """Populations that say where they come from: plane * 2^20 + global y * 2^10 + global x (exact in float32), as [plane][y][x]."""
    k, y, x = np.meshgrid(np.arange(9), np.arange(ny), np.arange(nx), indexing="ij")
    return (k * (1 << 20) + y * (1 << 10) + x).astype(np.float32)


def _device_floats(lbm, ptr, n):
    """n floats at device address ptr: one device-to-host copy (hipMemcpy of the HIP runtime the library is linked to)."""
    import torch
    torch.cuda.synchronize()
    memcpy = lbm.load_library().hipMemcpy
    memcpy.restype, memcpy.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    out = np.empty(n, dtype=np.float32)
    assert ptr and memcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), out.nbytes, 2) == 0      # hipMemcpyDeviceToHost
    return out


def _column_messages(lbm, q, lay):
    n = q.macro_pack_floats_x
    assert n == 9 * lay["ny_local"] * lay["ghost_x"]
    return [_device_floats(lbm, q.macro_pack_ptr_x(d, False), n).reshape(9, lay["ny_local"], lay["ghost_x"]) for d in (0, 1)]


def _row_messages(lbm, q, lay):
    w = lay["nx_local"] + 2 * lay["ghost_x"]
    n = q.macro_pack_floats
    assert n == 9 * lay["ghost"] * w
    return [_device_floats(lbm, q.macro_pack_ptr(d, False), n).reshape(9, lay["ghost"], w) for d in (0, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,rank", [("388x134_3x2", 0), ("388x134_3x2", 5), ("224x64_2x1", 1)])
def test_packed_messages_are_the_documented_slices(lbm, monkeypatch, name, rank):
    """Storage rows of 146 floats (8-byte accesses), 144 and 128 (16-byte): the four outgoing messages of a rank whose populations encode
    (plane, global y, global x), bit for bit the numpy slices of include/lbm_d2q9.h."""
    _set_knobs(monkeypatch, LAYOUTS[name][4])
    p, obst, lays = _deck(lbm, name)
    px, py = LAYOUTS[name][2:4]
    lay = lays[rank]
    assert lay["nx_local"] + 2 * lay["ghost_x"] == {("388x134_3x2", 0): 146, ("388x134_3x2", 5): 144, ("224x64_2x1", 1): 128}[(name, rank)]
    G = _encoded(p.nx, p.ny)
    y0, nyl, x0, nxl, gx, gy = (lay[k] for k in ("y0", "ny_local", "x0", "nx_local", "ghost_x", "ghost_y"))
    with lbm.Partition(p, lbm.count_free_cells(obst), lbm.obstacle_window(obst, lay), tile_of=(rank, px, py)) as q:
        q.set_cells(np.ascontiguousarray(G[:, y0:y0 + nyl, x0:x0 + nxl].transpose(1, 2, 0)))
        q.macro_pack_x()
        west, east = _column_messages(lbm, q, lay)
        assert np.array_equal(bits(west), bits(G[:, y0:y0 + nyl, x0:x0 + gx]))
        assert np.array_equal(bits(east), bits(G[:, y0:y0 + nyl, x0 + nxl - gx:x0 + nxl]))
        if gy == 0:
            assert q.macro_pack_floats == 0 and not q.macro_pack_ptr(0, False) and not q.macro_pack_ptr(1, True)
            return
        q.macro_pack()
        south, north = _row_messages(lbm, q, lay)                  # the owned columns: the ghost-column ends are whatever the grid holds
        assert np.array_equal(bits(south[:, :, gx:gx + nxl]), bits(G[:, y0:y0 + gy, x0:x0 + nxl]))
        assert np.array_equal(bits(north[:, :, gx:gx + nxl]), bits(G[:, y0 + nyl - gy:y0 + nyl, x0:x0 + nxl]))


@pytest.mark.gpu
def test_row_messages_carry_the_corners(lbm, monkeypatch):
    """A 1 x 1 rank with ghost rows is every neighbour of itself: once its column messages have come back and are unpacked, the row
    messages' ghost-column ends are the opposite owned columns — what a diagonal neighbour receives in two hops."""
    name = "128x32_1x1_yghost"
    _set_knobs(monkeypatch, LAYOUTS[name][4])
    p, obst, lays = _deck(lbm, name)
    lay = lays[0]
    nx, ny, gx, g = p.nx, p.ny, lay["ghost_x"], lay["ghost"]
    G = _encoded(nx, ny)
    with lbm.Partition(p, lbm.count_free_cells(obst), lbm.obstacle_window(obst, lay), tile_of=(0, 1, 1)) as q:
        q.set_cells(np.ascontiguousarray(G.transpose(1, 2, 0)))
        _exchange([q], [q.tile_neighbours()], None)
        q.macro_pack()
        south, north = _row_messages(lbm, q, lay)
        for msg, rows in ((south, slice(0, g)), (north, slice(ny - g, ny))):
            assert np.array_equal(bits(msg[:, :, gx:gx + nx]), bits(G[:, rows, :]))
            assert np.array_equal(bits(msg[:, :, :gx]), bits(G[:, rows, nx - gx:]))          # west ghost columns: the last owned columns
            assert np.array_equal(bits(msg[:, :, gx + nx:]), bits(G[:, rows, :gx]))          # east ghost columns: the first owned columns


# ---- 4. the RCCL loop on one tile rank ------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("schedule", ["serial", "edge"])
@pytest.mark.parametrize("name", ["256x128_1x1", "256x128_1x1_yghost", "128x32_1x1_yghost"])
def test_rccl_loop_steps_a_tile_rank(lbm, monkeypatch, name, schedule):
    """A 1 x 1 rank grid over RCCL: the rank sends its columns (and rows) to itself, under both schedules."""
    _rccl_ring_of_one(lbm, monkeypatch, name, schedule, False)


@pytest.mark.gpu
def test_rccl_loop_steps_a_tile_rank_with_an_allreduce_per_group(lbm, monkeypatch):
    _rccl_ring_of_one(lbm, monkeypatch, "256x128_1x1_yghost", "serial", True)


def _rccl_ring_of_one(lbm, monkeypatch, name, schedule, step_allreduce):
    _set_knobs(monkeypatch, dict(LAYOUTS[name][4], LBM_RCCL_SCHEDULE=schedule))
    p, obst, lays = _deck(lbm, name)
    ref_cells, ref_exact = _oracle(name)
    sim = lbm.Simulation(p, obst, exchange="auto" if step_allreduce else "rccl", strict=True, rank_grid=(1, 1), step_allreduce=step_allreduce)
    try:
        d = sim.describe()
        assert d["loop"] == "rccl" and d["rccl_nranks"] == 1 and d["step_allreduce"] == step_allreduce and d["p2p"] is None, d
        assert sim.partition.tile_info() == lays[0]
        av = np.concatenate([sim.run(n) for n in RUNS])
        cells = sim.local_cells()
    finally:
        sim.close()
    assert np.array_equal(bits(cells), bits(ref_cells)), "populations differ from the oracle"
    err = np.max(np.abs(av.astype(np.float64) - ref_exact) / ref_exact)
    print(f"{name} {schedule}: av_vels against the oracle {err:.3e}")
    assert av.shape == (sum(RUNS),) and err < AV_EXACT_RTOL


# ---- 5. tile ranks over RCCL, one GPU each ------------------------------------------------------------------------------------------------

RCCL_TILE_CASES = {
    2: [dict(nx=388, ny=134, grid=[2, 1], walls=True), dict(nx=388, ny=134, grid=[1, 2]), dict(nx=388, ny=134, grid=[2, 1], step_allreduce=True)],
    4: [dict(nx=256, ny=128, grid=[2, 2], walls=True), dict(nx=256, ny=128, grid=[2, 2], schedule="edge")],
}


@pytest.mark.gpu
@pytest.mark.parametrize("ranks", [2, 4])
def test_tile_ranks_over_rccl_with_one_gpu_per_rank(lbm, ranks):
    """Switches itself on when the box has at least `ranks` GPUs (RCCL refuses two ranks on one device): column blocks, row blocks of
    tile ranks and a 2 x 2 grid as fresh rank processes over real links, against the single-GPU digest (tests/tile_rccl_worker.py)."""
    import torch
    from conftest import run_rank_processes
    if torch.cuda.device_count() < ranks:
        pytest.skip(f"needs {ranks} GPUs, this box has {torch.cuda.device_count()}")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", GLOO_SOCKET_IFNAME="lo")
    for k in TUNE:
        env.pop(k, None)
    cases = RCCL_TILE_CASES[ranks]
    r = run_rank_processes(lambda port: [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(ranks), "--master-addr", "127.0.0.1",
                                         "--master-port", str(port), os.path.join(ROOT, "tests", "tile_rccl_worker.py"), json.dumps(cases)],
                           env, f"tile_rccl_{ranks}", timeout=600)
    lines = [l for l in r.stdout.splitlines() if l.startswith("CASE")]
    assert r.returncode == 0 and len(lines) == len(cases) and all(" ok " in l for l in lines), (r.stdout[-2000:], r.stderr[-3000:])


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_calls_on_the_wrong_kind_of_context_say_so(lbm, monkeypatch):
    _set_knobs(monkeypatch, {})
    p = lbm.Params(256, 128, 10, 4, 0.1, 0.01, 1.7)
    obst = lbm.synthetic_obstacles(256, 128, 0.03, 3, False)
    free = lbm.count_free_cells(obst)
    with lbm.Partition(p, free, obst[:64], 0, obstacles_global=obst) as rows:          # a K-step row partition
        assert rows.macro_steps > 0 and rows.macro_pack_floats_x == 0 and not rows.macro_pack_ptr_x(0, False)
        with pytest.raises(lbm.LbmError, match="lbm_tile_prepare: not a rank of the tile decomposition"):
            rows.tile_prepare(8)
        with pytest.raises(lbm.LbmError, match="lbm_macro_pack_x: not a rank of the tile decomposition"):
            rows.macro_pack_x()
        with pytest.raises(lbm.LbmError, match="lbm_macro_unpack_x: not a rank of the tile decomposition"):
            rows.macro_unpack_x()
        with pytest.raises(lbm.LbmError, match="lbm_macro_exchange_local_x: incompatible contexts"):
            rows.macro_receive_from_x(rows, 0)
    lay = lbm.tile_layout(p, 2, 1, 0)
    with lbm.Partition(p, free, lbm.obstacle_window(obst, lay), tile_of=(0, 2, 1)) as block:      # a column block: no ghost rows
        assert lay["ghost_y"] == 0 and block.macro_pack_floats == 0 and not block.macro_pack_ptr(0, False)
        with pytest.raises(lbm.LbmError, match="lbm_macro_pack: a column block keeps no ghost rows"):
            block.macro_pack()
        with pytest.raises(lbm.LbmError, match="lbm_macro_unpack: a column block keeps no ghost rows"):
            block.macro_unpack()
        with pytest.raises(lbm.LbmError, match="lbm_macro_exchange_local_y: incompatible contexts"):
            block.macro_receive_from_y(block, 0)
        with pytest.raises(lbm.LbmError, match="peer-to-peer loop"):                   # the row protocol still turns tile ranks away
            block.macro_prepare(8)
        with pytest.raises(lbm.LbmError, match=r"rank 0 of the 2 x 1 tile decomposition, the communicator's rank 0 of 1"):
            lbm.RcclRing(block, rank=0, size=1)
        block.tile_prepare(8)                                                          # ... and the tile protocol takes them
        assert (block.macro_next, block.macro_launches) == (8, 2)
    with pytest.raises(ValueError, match="torch loop takes row blocks"):
        lbm.Simulation(p, obst, exchange="torch", rank_grid=(1, 1))
