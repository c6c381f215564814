"""GPU tests of the five-step launch of whole periodic grids, lbm_multi_kernel<5, TERMS, kGeomTall, kPartPlain> (kernels/multi.h).

The launch keeps owned_substeps' dealing (one owned x-pair per lane for the whole launch on 64 x 24 tiles) and grows the frame to
72 x 32 by taking population 0 out of it: the owned pairs keep theirs in a register, the ring pairs theirs in a compact array indexed
by the pair's place in sub-step 1's ring.  What can go wrong that the four-step launch does not already show: the fourth ring row and
the wider first region, the ring index of a position (wrong index: a ring pair reads another pair's population 0), the fifth
accumulator, and the plan's tails of 4 and 3 steps on the same storage.  Obstacles as tests/test_owned_lanes.py places them, grids
whose last tile column and row stick out, a random start state; populations bit for bit against the oracle.

The form is the default from 8192 x 8192 cells (LBM_TUNE_MULTI5_MIN), the only measured size at which it won by the project's rule.
There is no case of the default plan at that size here: tests/test_gpu_parity.py test_full_size_8192_properties_and_short_parity
already runs it with no knobs, 50 steps, bit for bit against the oracle; tests/test_plan_k5.py holds which sizes take the form."""
import numpy as np
import pytest

import fused_ref
from test_owned_lanes import AV_EXACT_RTOL, TX, TY, bits

pytestmark = pytest.mark.gpu

SUMS_RTOL = 1e-12          # per-step sums of the fused arithmetic against its restatement, as tests/test_fused_arith.py holds them


def position_obstacles(nx, ny, seed):
    """One cell in three within 5 columns of a tile seam, on the first and last two rows of every tile row and on the accelerate row
    ny - 2 (partly kept free); one in fifty elsewhere."""
    rng = np.random.default_rng(seed)
    x, y = np.arange(nx), np.arange(ny)
    dx = np.minimum(x % TX, TX - x % TX)
    ry = y % TY
    near = (dx <= 5)[None, :] | ((ry <= 1) | (ry >= TY - 2))[:, None]
    near[ny - 2, :] = True
    obst = rng.random((ny, nx)) < np.where(near, 1.0 / 3.0, 0.02)
    obst[ny - 2, ::4] = False
    return obst.astype(np.int32)


@pytest.fixture
def five(monkeypatch):
    monkeypatch.setenv("LBM_TUNE_TILE_MAX", "0")
    monkeypatch.setenv("LBM_TUNE_MULTI_K", "5")
    monkeypatch.setenv("LBM_TUNE_MULTI_GEOM", "2")
    return monkeypatch


def deck(lbm, nx, ny, steps):
    p = lbm.Params(nx, ny, steps, 4, 0.1, 0.01, 1.7)
    obst = position_obstacles(nx, ny, nx * 7 + ny)
    rng = np.random.default_rng(nx + ny)
    cells0 = (rng.random((ny, nx, 9), dtype=np.float32) * 0.02 + 0.004).astype(np.float32)
    return p, obst, cells0


_oracle_runs = {}


def oracle_from(oracle, lbm, nx, ny, steps):
    """oracle.run_from of deck(nx, ny), once per grid and step count for the whole module; never written to."""
    key = (nx, ny, steps)
    if key not in _oracle_runs:
        p, obst, cells0 = deck(lbm, nx, ny, steps)
        _oracle_runs[key] = oracle.run_from(p, obst, cells0, steps)
    return _oracle_runs[key]


def run_five(lbm, nx, ny, runs, flags=0, kernel="lbm_multi_kernel<5>"):
    """`runs` calls of lbm_run from the deck's random state: av_vels of all of them, the steps of every launch, the final state."""
    p, obst, cells0 = deck(lbm, nx, ny, sum(runs))
    part = lbm.Partition(p, lbm.count_free_cells(obst), obst, flags=flags)
    try:
        assert part.describe()["kernel"] == kernel
        part.set_cells(cells0)
        part.set_profile(True)
        av, launches, sums = [], [], []
        for n in runs:
            av.append(part.run(n))
            launches += [k for k, _ in part.launch_profile()]
            sums.append(part.step_collect(n))
        cells = part.get_cells()
    finally:
        part.close()
    return np.concatenate(av), launches, cells, np.concatenate(sums)


# TX = 64, TY = 24, frame 72 x 32 (4 ring rows, 4 ring columns).
#   194 x 77, 13 steps: the accelerate row ny - 2 = 75 is the outermost (fourth) ring row above tile row 2 (rows 48 .. 71), an owned row of the
#     last tile row (72 .. 76, sticking out) and, through the wrap, a ring row below tile row 0
#   326 x 70, 12 steps: ny - 2 = 68 is an owned row of the last tile row (48 .. 69) and, through the wrap, a ring row below tile row 0 (rows
#     66 .. 69); the last tile column sticks out
#   256 x 83, 11 steps: tile columns 1 - 2 of tile row 1 are interior tiles (straight-line sub-step 1); the last tile row sticks out by 13
#   256 x 80, 5 / 6 / 7 steps: one launch, then the two tails 3 + 3 and 4 + 3
#   128 x 16 and 128 x 32, 10 steps: 26 rows are not a grid the plan tiles (fewer than 32 rows and no multiple of 16); 16 rows are, and the
#     32-row frame wraps onto itself there (ny < 32); 32 rows is the smallest height from 26 up
WHOLE_GRIDS = [(3 * TX + 2, 77, 13, [5, 5, 3]), (5 * TX + 6, 70, 12, [5, 4, 3]), (4 * TX, 83, 11, [5, 3, 3]),
               (4 * TX, 80, 5, [5]), (4 * TX, 80, 6, [3, 3]), (4 * TX, 80, 7, [4, 3]),
               (2 * TX, 16, 10, [5, 5]), (2 * TX, 32, 10, [5, 5])]


@pytest.mark.parametrize("nx,ny,steps,expect", WHOLE_GRIDS)
def test_whole_grid_from_a_random_state(lbm, oracle, five, nx, ny, steps, expect):
    av, launches, cells, _ = run_five(lbm, nx, ny, [steps])
    assert launches == expect
    ref_cells, ref_av = oracle_from(oracle, lbm, nx, ny, steps)
    differing = int(np.count_nonzero(bits(cells) != bits(ref_cells)))
    rel = float(np.max(np.abs(av - ref_av) / ref_av))
    print(f"{nx} x {ny}, {steps} steps: {differing} differing population words, av_vels off by {rel:.3e}")
    assert differing == 0
    assert rel < AV_EXACT_RTOL


@pytest.mark.parametrize("form", ["exact", "fast"])
def test_the_other_forms_of_the_terms(lbm, oracle, five, form):
    """LBM_FLAG_EXACT_AVVELS (double-precision terms) and LBM_FLAG_FAST_AVVELS (float terms) on the grid with interior tiles: the
    populations do not depend on the form; av_vels to the bound tests/test_gpu_parity.py holds both forms to."""
    flags = {"exact": lbm._capi.FLAG_EXACT_AVVELS, "fast": lbm._capi.FLAG_FAST_AVVELS}[form]
    name = {"exact": "lbm_multi_kernel<5, double-precision av_vels terms>", "fast": "lbm_multi_kernel<5, fast av_vels>"}[form]
    av, launches, cells, _ = run_five(lbm, 4 * TX, 83, [11], flags=flags, kernel=name)
    assert launches == [5, 3, 3]
    ref_cells, ref_av = oracle_from(oracle, lbm, 4 * TX, 83, 11)
    assert np.array_equal(bits(cells), bits(ref_cells))
    assert np.max(np.abs(av - ref_av) / ref_av) < AV_EXACT_RTOL


def test_the_fused_arithmetic(lbm, five):
    """LBM_FLAG_FUSED_ARITH against its restatement tests/fused_ref.c, as tests/test_fused_arith.py compares: populations bit for
    bit, per-step sums to 1e-12."""
    nx, ny, steps = 4 * TX, 83, 11
    p, obst, cells0 = deck(lbm, nx, ny, steps)
    _, launches, cells, sums = run_five(lbm, nx, ny, [steps], flags=lbm._capi.FLAG_FUSED_ARITH, kernel="lbm_multi_kernel<5, 6> (fused arithmetic)")
    assert launches == [5, 3, 3]
    ref_cells, ref_sums = fused_ref.run(p, obst, steps, mode="fused", cells0=cells0)
    assert np.array_equal(bits(cells), bits(ref_cells))
    assert np.max(np.abs(sums - ref_sums) / ref_sums) < SUMS_RTOL


def test_two_runs_on_one_context(lbm, oracle, five):
    """7 then 9 steps (4 + 3, then 5 + 4) equal 16 steps of the oracle: the accelerate-pending state between runs, and the fold of
    vectors of five, four and three across launches and runs."""
    nx, ny = 4 * TX, 83
    av, launches, cells, _ = run_five(lbm, nx, ny, [7, 9])
    assert launches == [4, 3, 5, 4]
    ref_cells, ref_av = oracle_from(oracle, lbm, nx, ny, 16)
    assert av.shape == ref_av.shape == (16,)
    assert np.array_equal(bits(cells), bits(ref_cells))
    assert np.max(np.abs(av - ref_av) / ref_av) < AV_EXACT_RTOL


def test_five_steps_against_four_steps_per_launch(lbm, five):
    """The same library with LBM_TUNE_MULTI_K=4 on a 320 x 77 grid, 13 steps: equal populations and equal av_vels, bit for bit."""
    nx, ny, steps = 5 * TX, 77, 13
    av5, launches5, cells5, _ = run_five(lbm, nx, ny, [steps])
    five.setenv("LBM_TUNE_MULTI_K", "4")
    av4, launches4, cells4, _ = run_five(lbm, nx, ny, [steps], kernel="lbm_multi_kernel<4>")
    assert launches5 == [5, 5, 3] and launches4 == lbm.plan_steps(4, steps) == [3, 3, 3, 4]
    assert np.array_equal(bits(cells5), bits(cells4))
    assert np.array_equal(bits(av5), bits(av4))


def test_per_step_sums_within_the_summation_tree_bound(lbm, five):
    """tests/test_terms_sums.py's census on the 256 x 83 grid, 11 steps, default (compensated) and double-precision terms: every
    per-step double sum within that module's bound for lbm_multi_kernel.  Its tree depth of 42 covers this launch: a lane holds one
    pair's term per sub-step (hi + lo, the pair's two cells: 2), wave_sum_vec8 is two halving swaps, one row rotation and three lane
    stages (6), one lane adds the block's 12 waves (12), and the fold is the four-step launch's (at most 20): 40."""
    import test_terms_sums as ts
    for form in ("default", "exact"):
        ts._multi_case(lbm, 4 * TX, 83, 11, form, (4 * TX + 83 + 5, (TX, 4), (TY, 4), ()), 5)
