"""CPU suite of the fused arithmetic (LBM_FLAG_FUSED_ARITH), part 1: its host restatement tests/fused_ref.c.

The restatement's exact mode is pinned to the oracle bit for bit — pull, rebound, acceleration and the sums are the code its
fused mode runs too — and the fused mode is then held to the project's acceptance rule (check/check.py's 1 % against the shipped
goldens) and to the deviation from the exact arithmetic measured on the full 128x128 deck:

    populations  1.95e-4 relative (largest over all cells and directions, after 40 000 steps)
    av_vels      3.6e-4  relative (largest over the 40 000 steps)

both far below check.py's 1e-2.  The same figures stand in DESIGN.md section 5 and in include/lbm_d2q9.h.  tests/test_fused_arith.py
holds the GPU kernels to this restatement.
"""
import os

import numpy as np
import pytest

import fused_ref
from conftest import GOLDEN, deck_paths

MEASURED_POPULATION_DEVIATION = 1.95e-4
MEASURED_AV_VELS_DEVIATION = 3.6e-4
ROOM = 4.0           # other decks accumulate differently; not a tuned pass mark: check.py's rule is 25 times further out


def shipped(oracle, digests, name):
    ppath, opath = deck_paths(name, digests)
    p = oracle.read_params(ppath)
    obst, _ = oracle.read_obstacles(opath, p.nx, p.ny)
    return p, obst


def synthetic(lbm, nx, ny, seed, walls=True, block_accel_row=False):
    p = lbm.Params(nx=nx, ny=ny, max_iters=60, reynolds_dim=8, density=0.1, accel=0.005, omega=1.85)
    obst = lbm.synthetic_obstacles(nx, ny, p=0.02, seed=seed, walls=walls)
    if block_accel_row:
        obst[ny - 2, 3:9] = 1
        obst[ny - 2, nx // 2] = 1
    return p, obst


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.mark.parametrize("case", ["128x128_200_steps", "accel_row_blocked_66x40", "odd_nx_37x24", "no_walls_48x21"])
def test_exact_mode_equals_the_oracle(lbm, oracle, digests, case):
    """Populations and per-step sums, bit for bit: the restatement's plumbing is right before its fused mode is trusted."""
    if case == "128x128_200_steps":
        p, obst = shipped(oracle, digests, "128x128")
        steps = 200
    elif case == "accel_row_blocked_66x40":
        p, obst = synthetic(lbm, 66, 40, seed=5, block_accel_row=True)
        steps = 60
    elif case == "odd_nx_37x24":
        p, obst = synthetic(lbm, 37, 24, seed=6)
        steps = 60
    else:
        p, obst = synthetic(lbm, 48, 21, seed=7, walls=False)
        steps = 60
    assert not obst[p.ny - 2].all() and (case == "no_walls_48x21" or obst[p.ny - 2].any())
    ref_cells, _, ref_exact = oracle.run(p, obst, steps)
    cells, sums = fused_ref.run(p, obst, steps, mode="exact")
    assert same_bits(cells, ref_cells)
    assert np.array_equal(sums * np.float64(fused_ref.free_cells_inv(obst)), ref_exact)


def test_fused_mode_differs_from_exact_after_one_step_and_is_deterministic(lbm):
    p, obst = synthetic(lbm, 66, 40, seed=5, block_accel_row=True)
    exact1, _ = fused_ref.run(p, obst, 1, mode="exact")
    fused1, _ = fused_ref.run(p, obst, 1, mode="fused")
    assert not same_bits(exact1, fused1)                                   # the flag means something
    assert same_bits(exact1[obst != 0], fused1[obst != 0])                 # ... in the free cells only: rebound is a copy
    a, sa = fused_ref.run(p, obst, 25, mode="fused")
    b, sb = fused_ref.run(p, obst, 25, mode="fused", nthreads=1)
    assert same_bits(a, b) and np.array_equal(sa, sb)
    # a run continued from a state equals the run made in one go
    c, sc = fused_ref.run(p, obst, 10, mode="fused")
    d, sd = fused_ref.run(p, obst, 15, mode="fused", cells0=c)
    assert same_bits(a, d) and np.array_equal(sa, np.concatenate([sc, sd]))


@pytest.fixture(scope="module")
def full_128(oracle, digests):
    """The whole 128x128 deck (40 000 steps) in the fused arithmetic and by the oracle, once for the tests below."""
    p, obst = shipped(oracle, digests, "128x128")
    cells, sums = fused_ref.run(p, obst, p.max_iters, mode="fused")
    ref_cells, ref_av, _ = oracle.run(p, obst, p.max_iters, nthreads=4)
    for a in (cells, sums, ref_cells, ref_av):
        a.setflags(write=False)
    return p, obst, cells, fused_ref.av_vels(sums, obst), ref_cells, ref_av


def test_fused_mode_passes_check_py_against_the_shipped_goldens(lbm, oracle, full_128, tmp_path):
    """The project's own acceptance rule, exactly as for the exact form (tests/test_oracle_golden.py)."""
    p, obst, cells, av, _, _ = full_128
    fs, avf = str(tmp_path / "final_state.dat"), str(tmp_path / "av_vels.dat")
    oracle.write_final_state(fs, p, cells, obst)
    oracle.write_av_vels(avf, av)
    rep = lbm.checker.check_files(os.path.join(GOLDEN, "check", "128x128.av_vels.dat.gz"),
                                  os.path.join(GOLDEN, "check", "128x128.final_state.dat.gz"), avf, fs)
    print(rep.message)
    assert rep.ok, rep.message
    assert "Both tests passed!" in rep.message


def test_fused_mode_deviation_from_the_exact_arithmetic(full_128):
    _, _, cells, av, ref_cells, ref_av = full_128
    pop = float(np.max(np.abs(cells.astype(np.float64) - ref_cells) / np.abs(ref_cells.astype(np.float64))))
    avd = float(np.max(np.abs(av.astype(np.float64) - ref_av) / ref_av.astype(np.float64)))
    print(f"fused against exact, 128x128 x 40000 steps: populations {pop:.3e}, av_vels {avd:.3e} (largest relative difference)")
    assert 0.0 < pop <= ROOM * MEASURED_POPULATION_DEVIATION
    assert 0.0 < avd <= ROOM * MEASURED_AV_VELS_DEVIATION
