"""GPU tests of the interior form of sub-step 1 of lbm_multi_kernel<4> on 64 x 24 tiles (kernels/multi.h, owned_substeps).

A tile whose whole frame lies inside the grid, and which holds no row or column that is computed but not counted, takes a form of
its own in sub-step 1: two straight-line sections on nine plane bases that carry the rows' -+ nx, the owned pair's flags
constants.  Its neighbours, the edge tiles, keep the rolled form, and
both recompute each other's rings.  The shapes are the smallest in which the two forms run side by side: one interior tile among
eight edge tiles; interior and edge tiles in both directions with a partial last tile column and row; a row ring whose ghost rows
put the accelerate row inside an interior tile's frame; and the fused arithmetic, whose instantiation shares the path.  Bit-exact
against the oracle (the fused arithmetic: against its host restatement), as tests/test_owned_lanes.py does it."""
import numpy as np
import pytest

import fused_ref
from test_owned_lanes import AV_EXACT_RTOL, TX, TY, bits, position_obstacles, tall  # noqa: F401  (tall: the fixture)

pytestmark = pytest.mark.gpu

NX1, NY1, STEPS = 3 * TX, 3 * TY, 13          # 192 x 72: tile (1, 1) is the only interior one


def one_interior_tile_obstacles(nx=NX1, ny=NY1, seed=17):
    """Obstacles by position around the interior tile (columns 64 .. 127, rows 24 .. 47): its four owned corners; one cell in three
    of its ring bands (the three rows below and above it) and side ring columns (four on each side); every other cell of the columns
    63, 64, 127, 128, 129 (the seams and the neighbouring tiles' even-rounded ring columns); one in fifty elsewhere."""
    rng = np.random.default_rng(seed)
    p = np.full((ny, nx), 0.02)
    p[TY - 3:2 * TY + 3, TX - 4:2 * TX + 4] = 1.0 / 3.0
    p[TY:2 * TY, TX:2 * TX] = 0.02
    p[:, [TX - 1, TX, 2 * TX - 1, 2 * TX, 2 * TX + 1]] = 0.5
    obst = rng.random((ny, nx)) < p
    for y in (TY, 2 * TY - 1):
        for x in (TX, 2 * TX - 1):
            obst[y, x] = True
    obst[ny - 2, ::4] = False                                  # keep the accelerate row partly free
    return obst.astype(np.int32)


@pytest.fixture(scope="module")
def deck1(lbm):
    """The 192 x 72 deck and its random start state, shared and never written to."""
    p = lbm.Params(NX1, NY1, STEPS, 4, 0.1, 0.01, 1.7)
    obst = one_interior_tile_obstacles()
    rng = np.random.default_rng(NX1 + NY1)
    cells0 = (rng.random((NY1, NX1, 9), dtype=np.float32) * 0.02 + 0.004).astype(np.float32)
    for arr in (obst, cells0):
        arr.setflags(write=False)
    return p, obst, cells0


def run_whole_grid(lbm, p, obst, cells0, steps, flags=0, kernel="lbm_multi_kernel<4>"):
    part = lbm.Partition(p, lbm.count_free_cells(obst), obst, flags=flags)
    assert part.describe()["kernel"] == kernel
    part.set_cells(np.array(cells0))
    av = part.run(steps)
    cells = part.get_cells()
    part.close()
    return cells, av


def test_one_interior_tile_among_eight_edge_tiles(lbm, oracle, tall, deck1):
    p, obst, cells0 = deck1
    assert obst[TY, TX] and obst[2 * TY - 1, 2 * TX - 1] and obst[TY - 3:TY, TX:2 * TX].any() and obst[TY:2 * TY, 2 * TX:2 * TX + 4].any()
    cells, av = run_whole_grid(lbm, p, obst, cells0, STEPS)
    _, av_exact = run_whole_grid(lbm, p, obst, cells0, STEPS, flags=lbm._capi.FLAG_EXACT_AVVELS,
                                 kernel="lbm_multi_kernel<4, double-precision av_vels terms>")
    ref_cells, ref_av = oracle.run_from(p, np.array(obst), np.array(cells0), STEPS)
    differing = int(np.count_nonzero(bits(cells) != bits(ref_cells)))
    rel = float(np.max(np.abs(av - ref_av) / ref_av))
    print(f"{differing} differing population words, av_vels off by {rel:.3e}, default != exact in {int(np.count_nonzero(av != av_exact))} steps")
    assert differing == 0
    assert rel < AV_EXACT_RTOL
    assert np.array_equal(av, av_exact)


@pytest.mark.parametrize("steps", [13, 16])
def test_interior_and_edge_tiles_with_a_partial_last_column_and_row(lbm, oracle, tall, steps):
    """262 x 98: five tile columns (the last 6 wide) by five tile rows (the last 2 high), interior tiles at x0 = 64, 128, 192 and
    rows 24, 48.  The library cuts 13 steps into launches of 3 + 3 + 3 + 4 (lbm_plan_steps ends a run on 4s and 3s, never on a 1-step
    launch): three launches of the row-pass dealing, then the tall kernel on what they left; 16 steps are four launches of the tall
    kernel."""
    nx, ny, STEPS = 4 * TX + 6, 4 * TY + 2, steps
    p = lbm.Params(nx, ny, STEPS, 4, 0.1, 0.01, 1.7)
    obst = position_obstacles(nx, ny, nx * 7 + ny + 1)
    rng = np.random.default_rng(nx + ny + 1)
    cells0 = (rng.random((ny, nx, 9), dtype=np.float32) * 0.02 + 0.004).astype(np.float32)
    part = lbm.Partition(p, lbm.count_free_cells(obst), obst)
    assert part.describe()["kernel"] == "lbm_multi_kernel<4>"
    part.set_cells(cells0)
    part.set_profile(True)
    av = part.run(STEPS)
    launches = [n for n, _ in part.launch_profile()]
    cells = part.get_cells()
    part.close()
    assert launches == lbm.plan_steps(4, STEPS) == ([3, 3, 3, 4] if steps == 13 else [4, 4, 4, 4])
    ref_cells, ref_av = oracle.run_from(p, obst, cells0, STEPS)
    differing = int(np.count_nonzero(bits(cells) != bits(ref_cells)))
    rel = float(np.max(np.abs(av - ref_av) / ref_av))
    print(f"{differing} differing population words, av_vels off by {rel:.3e}")
    assert differing == 0
    assert rel < AV_EXACT_RTOL


@pytest.mark.parametrize("ny", [130, 5 * TY])
def test_accelerate_row_inside_an_interior_tile_of_a_row_ring(lbm, oracle, tall, monkeypatch, ny):
    """A 1-rank peer-to-peer ring of 262 columns, 8 ghost rows, two launches per exchange: the storage has rows above the global
    accelerate row ny - 2, so that row lies inside the frame of interior tiles that count every row — the one place the interior form
    meets tile_accel.  130 rows: the row lies in the ring band of an interior tile.  120 rows, five whole tile rows: in the launches
    that compute the owned rows only it is an OWNED row of the last tile row, which is interior (storage rows 104 .. 127 of 136), so
    owned pairs of the interior form carry the accelerate bit through every sub-step.  Obstacles on one cell in three of the rows
    ny - 4 .. ny - 1, part of the accelerate row left free."""
    monkeypatch.setenv("LBM_TUNE_MACRO_GHOST", "8")
    monkeypatch.setenv("LBM_TUNE_MACRO_GROUP", "2")
    nx, steps = 4 * TX + 6, 26
    p = lbm.Params(nx, ny, steps, 4, 0.1, 0.01, 1.7)
    obst = position_obstacles(nx, ny, 41)
    rng = np.random.default_rng(43)
    obst[ny - 4:ny, :] |= (rng.random((4, nx)) < 1.0 / 3.0).astype(np.int32)
    obst[ny - 2, ::4] = 0
    ring = lbm.Simulation(p, obst, flags=lbm._capi.FLAG_FORCE_HALO, exchange="p2p", strict=True)
    assert ring.loop == "p2p" and ring.describe()["macro_k"] == 4 and ring.partition.describe()["kernel"] == "lbm_multi_kernel<4>"
    lay = ring.partition.tile_info()
    assert (lay["ghost"], lay["group"]) == (8, 2)
    av = ring.run(steps)
    cells = ring.local_cells()
    ring.close()
    ref_cells, _, ref_exact = oracle.run(p, obst, steps, nthreads=4)
    differing = int(np.count_nonzero(bits(cells) != bits(ref_cells)))
    rel = float(np.max(np.abs(av.astype(np.float64) - ref_exact) / ref_exact))
    print(f"{differing} differing population words, av_vels off by {rel:.3e}")
    assert differing == 0
    assert rel < AV_EXACT_RTOL


@pytest.mark.parametrize("steps", [13, 16])
def test_one_interior_tile_with_the_fused_arithmetic(lbm, tall, deck1, steps):
    """The fused TERMS instantiation shares the interior form: the same deck against the host restatement of the fused arithmetic
    (13 steps: one launch of the tall kernel after 3 + 3 + 3; 16: four of them)."""
    _, obst, cells0 = deck1
    STEPS = steps
    p = lbm.Params(NX1, NY1, STEPS, 4, 0.1, 0.01, 1.7)
    cells, av = run_whole_grid(lbm, p, obst, cells0, STEPS, flags=lbm._capi.FLAG_FUSED_ARITH, kernel="lbm_multi_kernel<4, 6> (fused arithmetic)")
    ref_cells, ref_sums = fused_ref.run(p, np.array(obst), STEPS, mode="fused", cells0=np.array(cells0))
    ref_av = ref_sums * np.float64(fused_ref.free_cells_inv(obst))
    differing = int(np.count_nonzero(bits(cells) != bits(ref_cells)))
    rel = float(np.max(np.abs(av - ref_av) / ref_av))
    print(f"{differing} differing population words, av_vels off by {rel:.3e}")
    assert differing == 0
    assert rel < AV_EXACT_RTOL
