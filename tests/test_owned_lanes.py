"""GPU tests of the two dealings of lanes in lbm_multi_kernel (kernels/multi.h): owned_substeps and k_substeps.

lbm_multi_kernel<4> on 64 x 24 tiles keeps one owned x-pair per lane for the whole launch (its flag bits and population 0 in
registers) and computes the ring of each region as extra, term-free items.  Obstacles go on every class of owned-pair position —
the tile seams, the first and last row of every tile row, the accelerate row inside a tile's ring — on grids whose last tile
column and row stick out, from a random start state, in every launch form: whole grids (plain), a row ring with ghost rows and
partial tile rows, a tile rank.  Bit-exact against the oracle; the per-step sums of the default (compensated) terms within 1e-12
of the double-precision form's.

The second half gives the same treatment to the row-pass dealing (k_substeps), which runs every other launch: K <= 3 on 64 x 16
tiles, K = 4 on 64 x 13 and 32 x 13, and every tail.  Both dealings share the source pull, the kept / counted classification, the
flag byte and the frame read, so a slip in one of those shows in both halves."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

AV_EXACT_RTOL = 1e-6
TX, TY = 64, 24


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def position_obstacles(nx, ny, seed, tx=TX, ty=TY):
    """One cell in three near every tile seam (x within 5 of a multiple of tx), on the first and last two rows of every tile row
    and on the accelerate row ny - 2; one in fifty elsewhere."""
    rng = np.random.default_rng(seed)
    x, y = np.arange(nx), np.arange(ny)
    dx = np.minimum(x % tx, tx - x % tx)
    ry = y % ty
    near = (dx <= 5)[None, :] | ((ry <= 1) | (ry >= ty - 2))[:, None]
    near[ny - 2, :] = True
    p = np.where(near, 1.0 / 3.0, 0.02)
    obst = rng.random((ny, nx)) < p
    obst[ny - 2, ::4] = False                                  # keep the accelerate row partly free
    return obst.astype(np.int32)


@pytest.fixture
def tall(monkeypatch):
    monkeypatch.setenv("LBM_TUNE_TILE_MAX", "0")
    monkeypatch.setenv("LBM_TUNE_MULTI_K", "4")
    monkeypatch.setenv("LBM_TUNE_MACRO_K", "4")
    monkeypatch.setenv("LBM_TUNE_MULTI_GEOM", "2")


# ny - 2 = 72: the accelerate row is the first row of the last (partial) tile row and lies in the ring of the one below;
# ny - 2 = 69: inside a tile, three rows below its top (the ring of the tile row above); 83: the last tile row sticks out by 11
@pytest.mark.parametrize("nx,ny", [(5 * TX + 6, 74), (3 * TX + 2, 71), (4 * TX, 83)])
def test_whole_grid_from_a_random_state(lbm, oracle, tall, nx, ny):
    steps = 13
    p = lbm.Params(nx, ny, steps, 4, 0.1, 0.01, 1.7)
    obst = position_obstacles(nx, ny, nx * 7 + ny)
    rng = np.random.default_rng(nx + ny)
    cells0 = (rng.random((ny, nx, 9), dtype=np.float32) * 0.02 + 0.004).astype(np.float32)
    part = lbm.Partition(p, lbm.count_free_cells(obst), obst)
    assert part.describe()["kernel"] == "lbm_multi_kernel<4>"
    part.set_cells(cells0)
    av = part.run(steps)
    cells = part.get_cells()
    part.close()
    ref_cells, ref_av = oracle.run_from(p, obst, cells0, steps)
    assert np.array_equal(bits(cells), bits(ref_cells))
    assert np.max(np.abs(av - ref_av) / ref_av) < AV_EXACT_RTOL


@pytest.mark.parametrize("ghost,group", [("8", "2"), ("12", "3")])
def test_row_ring_with_ghost_rows(lbm, oracle, tall, monkeypatch, ghost, group):
    """A 1-rank peer-to-peer ring: the first launches of a group also advance ghost rows (the counted form in the tiles that hold
    them), 130 rows are not a multiple of 24 (a partial last tile row), and the last launch says its ready words."""
    monkeypatch.setenv("LBM_TUNE_MACRO_GHOST", ghost)
    monkeypatch.setenv("LBM_TUNE_MACRO_GROUP", group)
    nx, ny, steps = 4 * TX + 6, 130, 26
    p = lbm.Params(nx, ny, steps, 4, 0.1, 0.01, 1.7)
    obst = position_obstacles(nx, ny, 11 + int(ghost))
    ring = lbm.Simulation(p, obst, flags=lbm._capi.FLAG_FORCE_HALO, exchange="p2p", strict=True)
    assert ring.loop == "p2p" and ring.describe()["macro_k"] == 4
    av = ring.run(steps)
    cells = ring.local_cells()
    ring.close()
    ref_cells, _, ref_exact = oracle.run(p, obst, steps, nthreads=4)
    assert np.array_equal(bits(cells), bits(ref_cells))
    assert np.max(np.abs(av.astype(np.float64) - ref_exact) / ref_exact) < AV_EXACT_RTOL


def test_tile_rank_of_one(lbm, oracle, tall):
    """A 1 x 1 rank of the tile decomposition: ghost columns, the kept and counted column ranges, rectangles of tiles."""
    nx, ny, steps = 6 * TX, 202, 25
    p = lbm.Params(nx, ny, steps, 4, 0.1, 0.01, 1.7)
    obst = position_obstacles(nx, ny, 5)
    s = lbm.Simulation(p, obst, exchange="p2p", strict=True, rank_grid=(1, 1))
    av = s.run(steps)
    cells = s.local_cells()
    s.close()
    ref_cells, _, ref_exact = oracle.run(p, obst, steps, nthreads=4)
    assert np.array_equal(bits(cells), bits(ref_cells))
    assert np.max(np.abs(av.astype(np.float64) - ref_exact) / ref_exact) < AV_EXACT_RTOL


def test_per_step_sums_against_the_double_form(lbm, oracle, tall):
    """Each lane now adds one pair's term per sub-step: the compensated per-step sums of a ring stay within 1e-12 of the
    double-precision form's and of the oracle's exact sums; av_vels of a whole grid equal value for value."""
    nx, ny, steps = 5 * TX + 6, 98, 24
    p = lbm.Params(nx, ny, steps, 4, 0.1, 0.01, 1.7)
    obst = position_obstacles(nx, ny, 3)
    free = lbm.count_free_cells(obst)
    _, _, ref_exact = oracle.run(p, obst, steps, nthreads=4)
    av, tot = {}, {}
    for k, flags in (("default", 0), ("exact", lbm._capi.FLAG_EXACT_AVVELS)):
        sim = lbm.Simulation(p, obst, flags=flags)
        av[k] = sim.run(steps)
        sim.close()
        ring = lbm.Simulation(p, obst, flags=flags | lbm._capi.FLAG_FORCE_HALO, exchange="p2p", strict=True)
        tot[k] = ring._p2p.run(steps) * np.float64(np.float32(1.0) / np.float32(free))
        ring.close()
    assert np.array_equal(av["default"], av["exact"])
    assert np.max(np.abs(tot["default"] - tot["exact"]) / tot["exact"]) < 1e-12
    assert np.max(np.abs(tot["default"] - ref_exact) / ref_exact) < 1e-12


# ---- the row-pass dealing (k_substeps): every launch but the tall K = 4 one.  The library does not report the geometry of its
# launches; LBM_TUNE_MULTI_GEOM overrides its whole choice (pick_geom in lbm_plan.cpp), so a case names the geometry it runs
# and the guard checks what can be seen: the kernel's name and the steps of every launch.
STD, NARROW = "0", "1"


def row_pass(monkeypatch, k, geom):
    monkeypatch.setenv("LBM_TUNE_TILE_MAX", "0")
    monkeypatch.setenv("LBM_TUNE_MULTI_K", str(k))
    monkeypatch.setenv("LBM_TUNE_MACRO_K", str(k))
    monkeypatch.setenv("LBM_TUNE_MULTI_GEOM", geom)


# 64 x 16 tiles, three tile columns and a sliver: 37 rows leave a last tile row of 5 and put ny - 2 = 35 in the ring below tile row 0
# (through the periodic wrap); 53 rows the same with four tile rows.  64 x 13 and 32 x 13 tiles: ny - 2 = 39 and 52 are first rows of
# the last tile row, which sticks out, and lie in the ring of the tile row below it.
@pytest.mark.parametrize("k,geom,tx,ty,nx,ny", [(1, STD, 64, 16, 3 * 64 + 2, 37), (2, STD, 64, 16, 3 * 64 + 2, 37), (3, STD, 64, 16, 3 * 64 + 2, 37),
                                                (1, STD, 64, 16, 3 * 64 + 2, 53), (2, STD, 64, 16, 3 * 64 + 2, 53), (3, STD, 64, 16, 3 * 64 + 2, 53),
                                                (4, STD, 64, 13, 3 * 64 + 2, 41), (4, STD, 64, 13, 5 * 64 + 6, 54), (4, NARROW, 32, 13, 5 * 32 + 6, 41)])
def test_row_pass_whole_grid_from_a_random_state(lbm, oracle, monkeypatch, k, geom, tx, ty, nx, ny):
    """13 steps: every run ends with a launch of another instantiation (K = 2: a 1-step tail, K = 3: 3 + 3 + 3 + 4, K = 4: 4 + 3 + 3 + 3)."""
    row_pass(monkeypatch, k, geom)
    steps = 13
    p = lbm.Params(nx, ny, steps, 4, 0.1, 0.01, 1.7)
    obst = position_obstacles(nx, ny, nx * 7 + ny + k, tx, ty)
    rng = np.random.default_rng(nx + ny + k)
    cells0 = (rng.random((ny, nx, 9), dtype=np.float32) * 0.02 + 0.004).astype(np.float32)
    part = lbm.Partition(p, lbm.count_free_cells(obst), obst)
    assert part.describe()["kernel"] == f"lbm_multi_kernel<{k}>"
    part.set_cells(cells0)
    part.set_profile(True)
    av = part.run(steps)
    launches = [n for n, _ in part.launch_profile()]
    cells = part.get_cells()
    part.close()
    assert launches == lbm.plan_steps(k, steps) and (k == 1 or len(set(launches)) > 1)
    ref_cells, ref_av = oracle.run_from(p, obst, cells0, steps)
    assert np.array_equal(bits(cells), bits(ref_cells))
    assert np.max(np.abs(av - ref_av) / ref_av) < AV_EXACT_RTOL


def test_row_pass_row_ring_with_ghost_rows(lbm, oracle, monkeypatch):
    """A 1-rank peer-to-peer ring at K = 4 on 64 x 13 tiles, 8 ghost rows and two launches per exchange: the counted form in the
    first and last tile rows of a group's first launch, 70 rows (78 with the advanced ghost rows) are no multiple of 13, and the
    group's last launch says and awaits its two ready words."""
    row_pass(monkeypatch, 4, STD)
    monkeypatch.setenv("LBM_TUNE_MACRO_GHOST", "8")
    monkeypatch.setenv("LBM_TUNE_MACRO_GROUP", "2")
    nx, ny, steps = 4 * 64 + 6, 70, 26
    p = lbm.Params(nx, ny, steps, 4, 0.1, 0.01, 1.7)
    obst = position_obstacles(nx, ny, 19, 64, 13)
    ring = lbm.Simulation(p, obst, flags=lbm._capi.FLAG_FORCE_HALO, exchange="p2p", strict=True)
    assert ring.loop == "p2p" and ring.describe()["macro_k"] == 4 and ring.partition.describe()["kernel"] == "lbm_multi_kernel<4>"
    lay = ring.partition.tile_info()
    assert (lay["ghost"], lay["group"]) == (8, 2)
    av = ring.run(steps)
    cells = ring.local_cells()
    ring.close()
    ref_cells, _, ref_exact = oracle.run(p, obst, steps, nthreads=4)
    assert np.array_equal(bits(cells), bits(ref_cells))
    assert np.max(np.abs(av.astype(np.float64) - ref_exact) / ref_exact) < AV_EXACT_RTOL


def test_row_pass_tile_rank_of_one(lbm, oracle, monkeypatch):
    """A 1 x 1 rank of the tile decomposition at K = 4 on 64 x 13 tiles: ghost columns, the kept and counted column ranges,
    rectangles of tiles, four ready words."""
    row_pass(monkeypatch, 4, STD)
    nx, ny, steps = 4 * 64, 80, 25
    p = lbm.Params(nx, ny, steps, 4, 0.1, 0.01, 1.7)
    obst = position_obstacles(nx, ny, 23, 64, 13)
    s = lbm.Simulation(p, obst, exchange="p2p", strict=True, rank_grid=(1, 1))
    assert s.describe()["macro_k"] == 4 and s.partition.describe()["kernel"] == "lbm_multi_kernel<4>"
    assert s.partition.tile_info()["ghost_x"] > 0
    av = s.run(steps)
    cells = s.local_cells()
    s.close()
    ref_cells, _, ref_exact = oracle.run(p, obst, steps, nthreads=4)
    assert np.array_equal(bits(cells), bits(ref_cells))
    assert np.max(np.abs(av.astype(np.float64) - ref_exact) / ref_exact) < AV_EXACT_RTOL


def test_row_pass_per_step_sums_against_the_double_form(lbm, oracle, monkeypatch):
    """A lane of the row-pass dealing adds several pairs' terms per sub-step, the low parts through acc_lo: on the ring's grid the
    compensated per-step sums stay within 1e-12 of the double-precision form's and of the oracle's exact sums; av_vels of the whole
    grid equal value for value."""
    row_pass(monkeypatch, 4, STD)
    monkeypatch.setenv("LBM_TUNE_MACRO_GHOST", "8")
    monkeypatch.setenv("LBM_TUNE_MACRO_GROUP", "2")
    nx, ny, steps = 4 * 64 + 6, 70, 26
    p = lbm.Params(nx, ny, steps, 4, 0.1, 0.01, 1.7)
    obst = position_obstacles(nx, ny, 29, 64, 13)
    free = lbm.count_free_cells(obst)
    _, _, ref_exact = oracle.run(p, obst, steps, nthreads=4)
    av, tot = {}, {}
    for k, flags in (("default", 0), ("exact", lbm._capi.FLAG_EXACT_AVVELS)):
        sim = lbm.Simulation(p, obst, flags=flags)
        assert sim.partition.describe()["kernel"] == ("lbm_multi_kernel<4>" if k == "default" else "lbm_multi_kernel<4, double-precision av_vels terms>")
        av[k] = sim.run(steps)
        sim.close()
        ring = lbm.Simulation(p, obst, flags=flags | lbm._capi.FLAG_FORCE_HALO, exchange="p2p", strict=True)
        assert ring.describe()["macro_k"] == 4
        tot[k] = ring._p2p.run(steps) * np.float64(np.float32(1.0) / np.float32(free))
        ring.close()
    assert np.array_equal(av["default"], av["exact"])
    assert np.max(np.abs(tot["default"] - tot["exact"]) / tot["exact"]) < 1e-12
    assert np.max(np.abs(tot["default"] - ref_exact) / ref_exact) < 1e-12
