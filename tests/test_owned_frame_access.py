"""GPU tests of the owned pair's frame accesses in lbm_multi_kernel's tall geometry (kernels/multi.h owned_substeps: read_pair_own,
store_pair_own).

In sub-steps 2 .. K a lane reads and writes its owned pair through constant offsets on lane bases that are fixed for the launch: one
constant per plane, row and sub-step shift.  A wrong constant shows as a pair reading another plane or another row.  The states of the
other suites are random; here population k of cell (x, y) is (4096 + k * 4096 + (y mod 64) * 64 + (x mod 64)) * 2^-20, a value that
names its plane, row and column (all exactly representable, 0.0039 .. 0.039), and the grid has no obstacle at all, so that no
bounce-back can stand in for a swap.  Populations bit for bit against the oracle.

Grids: 192 x 72 is 3 x 3 tiles of 64 x 24, one interior tile among eight edge tiles; on 200 x 60 the last tile column and row stick
out.  K = 4 and K = 5, runs of 3, 4, 5, 9 and 13 steps, so that every tail (a launch of fewer steps on the same storage) occurs; and a
1-rank row ring with ghost rows, whose first and last tile rows take the counted form (kPartGhost)."""
import numpy as np
import pytest

from test_owned_lanes import TX, TY, bits

pytestmark = pytest.mark.gpu


def named_state(nx, ny):
    k = np.arange(9)[None, None, :]
    y = (np.arange(ny) % 64)[:, None, None]
    x = (np.arange(nx) % 64)[None, :, None]
    n = 4096 + k * 4096 + y * 64 + x
    cells = (n.astype(np.float64) * 2.0 ** -20).astype(np.float32)
    assert np.array_equal(cells.astype(np.float64) * 2.0 ** 20, n), "every value is exactly representable"
    assert len(np.unique(cells[:64, :64])) == 9 * min(ny, 64) * min(nx, 64), "distinct within a 64 x 64 block"
    return cells


def deck(lbm, nx, ny, steps):
    return lbm.Params(nx, ny, steps, 4, 0.1, 0.01, 1.7), np.zeros((ny, nx), np.int32), named_state(nx, ny)


_oracle_runs = {}


def oracle_from(oracle, lbm, nx, ny, steps):
    """The oracle's state after `steps` steps from the named state; once per grid and step count, never written to."""
    key = (nx, ny, steps)
    if key not in _oracle_runs:
        p, obst, cells0 = deck(lbm, nx, ny, steps)
        cells, _ = oracle.run_from(p, obst, cells0, steps)
        cells.setflags(write=False)
        _oracle_runs[key] = cells
    return _oracle_runs[key]


FIVE_STEP_PLANS = {3: [3], 4: [4], 5: [5], 9: [5, 4], 13: [5, 5, 3]}      # fives, then a tail of the four-step plan (tests/test_multi5.py, tests/test_plan_k5.py)


def expected_launches(lbm, K, steps):
    return lbm.plan_steps(4, steps) if K == 4 else FIVE_STEP_PLANS[steps]


@pytest.mark.parametrize("steps", [3, 4, 5, 9, 13])
@pytest.mark.parametrize("K", [4, 5])
@pytest.mark.parametrize("nx,ny", [(3 * TX, 3 * TY), (200, 60)])
def test_whole_grid_from_the_named_state(lbm, oracle, monkeypatch, nx, ny, K, steps):
    monkeypatch.setenv("LBM_TUNE_TILE_MAX", "0")
    monkeypatch.setenv("LBM_TUNE_MULTI_GEOM", "2")
    monkeypatch.setenv("LBM_TUNE_MULTI_K", str(K))
    p, obst, cells0 = deck(lbm, nx, ny, steps)
    part = lbm.Partition(p, lbm.count_free_cells(obst), obst)
    try:
        assert part.describe()["kernel"] == f"lbm_multi_kernel<{K}>"
        part.set_cells(cells0)
        part.set_profile(True)
        part.run(steps)
        launches = [k for k, _ in part.launch_profile()]
        cells = part.get_cells()
    finally:
        part.close()
    print(f"{nx} x {ny}, K = {K}, {steps} steps: launches {launches}")
    assert launches == expected_launches(lbm, K, steps)
    ref = oracle_from(oracle, lbm, nx, ny, steps)
    differing = int(np.count_nonzero(bits(cells) != bits(ref)))
    print(f"  {differing} differing population words")
    assert differing == 0


def test_row_ring_with_ghost_rows_from_the_named_state(lbm, oracle, monkeypatch):
    """A 1-rank peer-to-peer ring as tests/test_owned_lanes.py sets one up (8 ghost rows, two launches per exchange): the group's first
    launch also advances ghost rows, so its first and last tile rows run the counted form; 130 rows leave a partial last tile row."""
    monkeypatch.setenv("LBM_TUNE_TILE_MAX", "0")
    monkeypatch.setenv("LBM_TUNE_MULTI_GEOM", "2")
    monkeypatch.setenv("LBM_TUNE_MULTI_K", "4")
    monkeypatch.setenv("LBM_TUNE_MACRO_K", "4")
    monkeypatch.setenv("LBM_TUNE_MACRO_GHOST", "8")
    monkeypatch.setenv("LBM_TUNE_MACRO_GROUP", "2")
    nx, ny, steps = 200, 130, 13
    p, obst, cells0 = deck(lbm, nx, ny, steps)
    ring = lbm.Simulation(p, obst, flags=lbm._capi.FLAG_FORCE_HALO, exchange="p2p", strict=True)
    try:
        assert ring.loop == "p2p" and ring.describe()["macro_k"] == 4 and ring.partition.describe()["kernel"] == "lbm_multi_kernel<4>"
        lay = ring.partition.tile_info()
        assert (lay["ghost"], lay["group"]) == (8, 2)
        ring.partition.set_cells(cells0)             # the owned rows; the run's first push fills the ghost rows from them
        ring.run(steps)
        cells = ring.local_cells()
    finally:
        ring.close()
    ref = oracle_from(oracle, lbm, nx, ny, steps)
    assert np.array_equal(bits(cells), bits(ref))
