"""GPU tests of the column growth of lbm_multi_kernel's regions (kernels/multi.h, multi_ex).

Sub-step j of a K-step launch computes the owned tile grown by K - j rows and by K - j columns rounded up to even.  Where K - j is
odd, the region's outermost column lies outside every owned cell's dependency cone and reads stale frame values; these tests put
obstacles and a random start state right at the tile seams, where such a column would first show if it leaked into an owned cell
or into the per-step sums.  Bit-exact against the oracle."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

AV_EXACT_RTOL = 1e-6


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def seam_obstacles(nx, ny, tx, seed):
    """Obstacles in the five columns on each side of every tile seam (x = multiples of tx), one cell in three there, none elsewhere."""
    rng = np.random.default_rng(seed)
    x = np.arange(nx)
    d = np.minimum(x % tx, tx - x % tx)                     # distance to the nearest seam
    near = (d <= 5)[None, :] & (rng.random((ny, nx)) < 1.0 / 3.0)
    return near.astype(np.int32)


@pytest.mark.parametrize("K,geom,tx", [(2, "0", 64), (3, "0", 64), (3, "1", 32), (4, "0", 64), (4, "1", 32), (4, "2", 64)])
def test_seam_columns_from_a_random_state(lbm, oracle, monkeypatch, K, geom, tx):
    """Every geometry of the 2-, 3- and 4-step launch from a random state, on a grid whose last tile column and row stick out."""
    monkeypatch.setenv("LBM_TUNE_TILE_MAX", "0")
    monkeypatch.setenv("LBM_TUNE_MULTI_K", str(K))
    monkeypatch.setenv("LBM_TUNE_MULTI_GEOM", geom)
    nx, ny, steps = 5 * tx + 6, 83, 3 * K + 1
    p = lbm.Params(nx, ny, steps, 4, 0.1, 0.01, 1.7)
    obst = seam_obstacles(nx, ny, tx, 100 * K + int(geom))
    rng = np.random.default_rng(K * 31 + int(geom))
    cells0 = (rng.random((ny, nx, 9), dtype=np.float32) * 0.02 + 0.004).astype(np.float32)
    part = lbm.Partition(p, lbm.count_free_cells(obst), obst)
    assert part.describe()["kernel"] == f"lbm_multi_kernel<{K}>"
    part.set_cells(cells0)
    av = part.run(steps)
    cells = part.get_cells()
    part.close()
    ref_cells, ref_av = oracle.run_from(p, obst, cells0, steps)
    assert np.array_equal(bits(cells), bits(ref_cells))
    assert np.max(np.abs(av - ref_av) / ref_av) < AV_EXACT_RTOL


@pytest.mark.parametrize("K", [3, 4])
def test_seam_columns_on_a_tile_rank_of_one(lbm, oracle, monkeypatch, K):
    """A 1 x 1 rank of the tile decomposition (ghost columns; the interior / rim split of a launch uses the reach of the first
    sub-step, multi_ex(K - 1) + 1 columns) against the oracle."""
    monkeypatch.setenv("LBM_TUNE_MACRO_K", str(K))
    nx, ny, steps = 384, 200, 6 * K + 1
    p = lbm.Params(nx, ny, steps, 4, 0.1, 0.01, 1.7)
    obst = seam_obstacles(nx, ny, 64, 7 + K)
    obst[ny - 2, ::3] = 0                                   # keep the accelerate row mostly free
    s = lbm.Simulation(p, obst, exchange="p2p", strict=True, rank_grid=(1, 1))
    av = s.run(steps)
    cells = s.local_cells()
    s.close()
    ref_cells, _, ref_exact = oracle.run(p, obst, steps, nthreads=4)
    assert np.array_equal(bits(cells), bits(ref_cells))
    assert np.max(np.abs(av - ref_exact) / ref_exact) < AV_EXACT_RTOL
