"""GPU tests of the owned-lane dealing of the tall 4-step launch (kernels/multi.h, owned_substeps).

lbm_multi_kernel<4> on 64 x 24 tiles keeps one owned x-pair per lane for the whole launch (its flag bits and population 0 in
registers) and computes the ring of each region as extra, term-free items.  Obstacles go on every class of owned-pair position —
the tile seams, the first and last row of every tile row, the accelerate row inside a tile's ring — on grids whose last tile
column and row stick out, from a random start state, in every launch form: whole grids (plain), a row ring with ghost rows and
partial tile rows, a tile rank.  Bit-exact against the oracle; the per-step sums of the default (compensated) terms within 1e-12
of the double-precision form's."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

AV_EXACT_RTOL = 1e-6
TX, TY = 64, 24


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def position_obstacles(nx, ny, seed):
    """One cell in three near every tile seam (x within 5 of a multiple of TX), on the first and last two rows of every tile row
    and on the accelerate row ny - 2; one in fifty elsewhere."""
    rng = np.random.default_rng(seed)
    x, y = np.arange(nx), np.arange(ny)
    dx = np.minimum(x % TX, TX - x % TX)
    ry = y % TY
    near = (dx <= 5)[None, :] | ((ry <= 1) | (ry >= TY - 2))[:, None]
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
