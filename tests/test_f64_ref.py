"""tests/f64_ref.c — the CPU restatement of the double-precision mode — pinned to the results the reference PUBLISHED (its shipped
check files and README figures came from double-precision code), and to the float oracle's physics.  No GPU, no library call."""
import numpy as np
import pytest

import f64_ref
from conftest import deck_paths


@pytest.fixture(scope="module")
def deck128():
    return f64_ref.deck_run("128x128")       # cached per process: tests/test_f64.py reuses it


def test_full_128x128_deck_reproduces_the_shipped_results(deck128, oracle):
    """40 000 steps of the 128 x 128 deck against tests/golden/check/128x128.{av_vels,final_state}.dat.gz and README.md:78.
    Measured here (printed below, recorded in f64_ref.MEASURED_* and DESIGN.md section 5): av_vels 6.87e-13 relative, final_state
    1.26e-14 absolute, Reynolds 1.21e-13 relative — the last digit the files print.  Asserted at twice that: the arithmetic is
    deterministic and the factor covers only the two roundings to 13 digits.  The float oracle is 8e-4 away: why the mode exists."""
    p, obst, cells, serial, exact = deck128
    golden_av = f64_ref.golden_av_vels("128x128")
    av = f64_ref.av_vels(serial, obst)
    assert av.shape == golden_av.shape == (40000,)
    av_rel = float(np.max(np.abs(av - golden_av) / np.abs(golden_av)))
    golden_fs = f64_ref.golden_final_state("128x128")
    fs_abs = float(np.max(np.abs(f64_ref.final_state_values(p, cells, obst).reshape(-1, 4) - golden_fs)))
    re = f64_ref.reynolds(p, cells, obst)
    pub = float(f64_ref.published()["reynolds"]["128x128"]["value"])
    re_rel = abs(re - pub) / pub
    # the float path on the same deck
    fp = oracle.read_params(f64_ref.os.path.join(f64_ref.GOLDEN, "decks", "input_128x128.params"))
    _, av32 = oracle.run_fast(fp, obst, fp.max_iters, 8)
    float_rel = float(np.max(np.abs(av32.astype(np.float64) - golden_av) / np.abs(golden_av)))
    print(f"128x128 double restatement: av_vels {av_rel:.3e} rel, final_state {fs_abs:.3e} abs, Reynolds {re!r} ({re_rel:.3e} rel); float oracle av_vels {float_rel:.3e} rel")
    assert av_rel <= f64_ref.AV_VELS_LIMIT
    assert fs_abs <= f64_ref.FINAL_STATE_LIMIT
    assert re_rel <= f64_ref.REYNOLDS_LIMIT
    assert "%.12E" % re in ("9.763598020525E+00", "9.763598020526E+00")
    assert float_rel > 1e-5
    # the exactly rounded sums tell the same story: a serial sum of n non-negative terms errs by at most n * 2^-53 of it, far below the printing
    assert float(np.max(np.abs(f64_ref.av_vels(exact, obst) - av) / av)) <= (f64_ref.free_cells(obst) + 2) * 2.0 ** -53


def test_published_reynolds_numbers_are_data_with_sources():
    pub = f64_ref.published()["reynolds"]
    assert {k: v["source"] for k, v in pub.items()} == {"128x128": "README.md:78", "128x256": "README.md:88", "256x256": "README.md:98",
                                                        "1024x1024": "newprofiles/firstSerial1024x1024.out:8"}
    assert all(0.0 < float(v["value"]) < 100.0 for v in pub.values())


MEASURED_FLOAT_DISTANCE = 1.41e-6      # rand_64x48, 50 steps, largest population difference over the largest population


def test_same_physics_as_the_float_oracle(oracle, digests):
    """50 steps of rand_64x48: the populations agree with the float oracle to float rounding.  Measured 1.41e-6 relative to the largest
    population (the printed figure); asserted at ten times that.  (Fifty steps of float rounding, ~2^-24 each, accumulate to it.)"""
    ppath, opath = deck_paths("rand_64x48", digests)
    p64 = f64_ref.read_params(ppath)
    obst = f64_ref.read_obstacles(opath, p64.nx, p64.ny)
    cells64, _, _ = f64_ref.run(p64, obst, 50)
    cells32, _, _ = oracle.run(oracle.read_params(ppath), obst, 50)
    rel = float(np.max(np.abs(cells64 - cells32.astype(np.float64))) / np.max(cells64))
    print(f"rand_64x48, 50 steps: double restatement against float oracle {rel:.3e} of the largest population")
    assert rel <= 10 * MEASURED_FLOAT_DISTANCE



def test_thread_count_changes_no_bit(digests):
    ppath, opath = deck_paths("walls_40x24", digests)
    p = f64_ref.read_params(ppath)
    obst = f64_ref.read_obstacles(opath, p.nx, p.ny)
    c1, s1, e1 = f64_ref.run(p, obst, 30, nthreads=1)
    c7, s7, e7 = f64_ref.run(p, obst, 30, nthreads=7)
    assert np.array_equal(c1.view(np.uint64), c7.view(np.uint64)) and np.array_equal(s1, s7) and np.array_equal(e1, e7)
    # 13 + 17 steps from the intermediate state are the 30 steps
    ca, sa, _ = f64_ref.run(p, obst, 13)
    cb, sb, _ = f64_ref.run(p, obst, 17, cells0=ca)
    assert np.array_equal(cb.view(np.uint64), c1.view(np.uint64)) and np.array_equal(np.concatenate([sa, sb]), s1)


DX = (0, 1, 0, -1, 0, 1, -1, -1, 1)
DY = (0, 0, 1, 0, -1, 1, 1, -1, -1)


def _stream(state):
    """in[y, x, k] = state[y - DY[k], x - DX[k], k], periodic: what streams into each cell."""
    return np.stack([np.roll(state[..., k], (DY[k], DX[k]), axis=(0, 1)) for k in range(9)], axis=-1)


def _unstream(pulled):
    """The state whose streaming gives `pulled`: state[y - DY[k], x - DX[k], k] = pulled[y, x, k]."""
    return np.stack([np.roll(pulled[..., k], (-DY[k], -DX[k]), axis=(0, 1)) for k in range(9)], axis=-1)


def test_per_cell_entry_is_the_step():
    """f64_ref_cells (what tests/test_f64_cells.py holds the device function to) is the function f64_ref_run applies to every cell, on a
    12 x 7 grid with obstacles, some of them on the accelerated row.
      First step, no acceleration (accel = 0.0 adds 0.0 to positive populations: the same bits): from the state built by inverse streaming
      of `pulled`, one f64_ref_run step gives f64_ref_cells(pulled) exactly, and serial[0] / exact[0] are the sums of its terms.
      Second step, accelerated: f64_ref_cells(pulled) with `accel` set on row ny-2 is the state after the first step AND the second step's
      accelerate_flow; streamed and passed through f64_ref_cells again it must be exactly what one accelerated f64_ref_run step makes of
      the first step's plain result."""
    import math
    nx, ny = 12, 7
    rng = np.random.default_rng(12)
    obst = (rng.random((ny, nx)) < 0.2).astype(np.int32)
    obst[ny - 2, 3] = 1
    obst[ny - 2, 4:6] = 0
    p = f64_ref.SimpleNamespace(nx=nx, ny=ny, max_iters=1, reynolds_dim=1, density=0.1, accel=0.005, omega=1.85)
    w1, w2 = f64_ref.accel_weights(p.density, p.accel)
    assert (w1, w2) == (0.1 * 0.005 * 0.111111111111111111111111, 0.1 * 0.005 * 0.0277777777777777777777778)
    pulled = f64_ref.initial_cells(p) * rng.uniform(0.8, 1.2, (ny, nx, 9))
    pulled[ny - 2, 5] *= 1e-3                  # one free cell of the row too thin for accelerate_flow's condition
    assert np.array_equal(_stream(_unstream(pulled)), pulled)
    blocked = obst.reshape(-1)
    none = np.zeros(nx * ny, np.int32)
    row = np.zeros((ny, nx), np.int32)
    row[ny - 2] = 1

    def sums(term):
        t = term.reshape(ny, nx)
        parts = []
        for part in (t[1:ny - 1], t[0:1], t[ny - 1:ny]):        # f64_ref_run's serial[]: rows 1..ny-2, row 0, row ny-1
            acc = 0.0
            for v in part.reshape(-1).tolist():
                acc += v
            parts.append(acc)
        return parts[0] + parts[1] + parts[2], math.fsum(term.tolist())

    # first step
    still = f64_ref.SimpleNamespace(**{**vars(p), "accel": 0.0})
    plain, term = f64_ref.cells_each(pulled.reshape(-1, 9), blocked, none, p.omega, w1, w2)
    got, serial, exact = f64_ref.run(still, obst, 1, cells0=_unstream(pulled))
    assert np.array_equal(got.view(np.uint64).reshape(-1, 9), plain.view(np.uint64))
    assert np.all(term[blocked != 0] == 0.0) and np.all(term[blocked == 0] > 0.0)
    assert (serial[0], exact[0]) == sums(term)
    for k, back in enumerate((0, 3, 4, 1, 2, 7, 8, 5, 6)):
        assert np.array_equal(plain[blocked != 0, back], pulled.reshape(-1, 9)[blocked != 0, k])
    # second step
    pushed, term_pushed, mom = f64_ref.cells_each(pulled.reshape(-1, 9), blocked, row.reshape(-1), p.omega, w1, w2, moments=True)
    assert np.array_equal(term_pushed, term)
    changed = np.any(pushed != plain, axis=1).reshape(ny, nx)
    holds = ((plain[:, 3] - w1 > 0.0) & (plain[:, 6] - w2 > 0.0) & (plain[:, 7] - w2 > 0.0)).reshape(ny, nx)
    assert np.array_equal(changed, holds & (row != 0) & (obst == 0)) and not changed[ny - 2, 5]
    assert changed[ny - 2].sum() == (obst[ny - 2] == 0).sum() - 1
    out, term2 = f64_ref.cells_each(_stream(pushed.reshape(ny, nx, 9)).reshape(-1, 9), blocked, none, p.omega, w1, w2)
    got, serial, exact = f64_ref.run(p, obst, 1, cells0=plain.reshape(ny, nx, 9))
    assert np.array_equal(got.view(np.uint64).reshape(-1, 9), out.view(np.uint64))
    assert (serial[0], exact[0]) == sums(term2)
    # the moments are collide()'s: the density added left to right from 0.0
    rho = np.zeros(nx * ny)
    for k in range(9):
        rho = rho + pulled.reshape(-1, 9)[:, k]
    assert np.array_equal(mom[blocked == 0, 0], rho[blocked == 0]) and np.all(mom[blocked != 0] == 0.0)
    # run_report: this run is one the summation bounds apply to; with every density negative it is not, and the terms' magnitudes sum
    # to what the terms summed to; a cell of zeros has the term 0 * inf
    _, exact_r, status, mags = f64_ref.run_report(p, obst, 2, cells0=plain.reshape(ny, nx, 9))
    assert f64_ref.benign(status).tolist() == [True, True] and exact_r[0] == exact[0] == mags[0]
    _, exact_n, status, mags_n = f64_ref.run_report(still, obst, 1, cells0=-plain.reshape(ny, nx, 9))
    assert status.tolist() == [0] and exact_n[0] == -mags_n[0] < 0.0
    hole = plain.reshape(ny, nx, 9).copy()
    hole[:] = 0.0
    assert f64_ref.run_report(still, np.zeros_like(obst), 1, cells0=hole)[2].tolist() == [f64_ref.NAN_TERM]


def test_rest_state_and_one_hand_computed_cell():
    """The rest state and one relaxation written out by hand in Python floats (IEEE doubles), operation by operation."""
    p = f64_ref.SimpleNamespace(nx=3, ny=3, max_iters=1, reynolds_dim=1, density=0.1, accel=0.0, omega=1.7)
    cells = f64_ref.initial_cells(p)
    assert cells[0, 0].tolist() == [0.1 * 4.0 / 9.0] + [0.1 / 9.0] * 4 + [0.1 / 36.0] * 4
    rng = np.random.default_rng(5)
    state = rng.uniform(0.01, 0.2, (3, 3, 9))
    out, serial, exact = f64_ref.run(p, np.zeros((3, 3), np.int32), 1, cells0=state)
    # cell (1, 1): accel = 0.0 leaves the state as it is (f - 0.0 > 0 holds, +- 0.0 changes nothing)
    t = [state[1, 1][0], state[1, 0][1], state[0, 1][2], state[1, 2][3], state[2, 1][4], state[0, 0][5], state[0, 2][6], state[2, 2][7], state[2, 0][8]]
    t = [float(v) for v in t]
    rho = 0.0
    for v in t:
        rho += v
    rinv = 1.0 / rho
    mx = t[1] + t[5] + t[8] - t[3] - t[6] - t[7]
    my = t[2] + t[5] + t[6] - t[4] - t[7] - t[8]
    msq = mx * mx + my * my
    u5 = mx + my
    h = 0.5 * rinv * 3.0
    eq5 = (1.0 / 36.0) * (rho + u5 * 3.0 + h * (u5 * 3.0 * u5 - msq))
    assert out[1, 1, 5] == t[5] + 1.7 * (eq5 - t[5])
    eq0 = (4.0 / 9.0) * (rho - h * msq)
    assert out[1, 1, 0] == t[0] + 1.7 * (eq0 - t[0])
    assert serial[0] == pytest.approx(exact[0], rel=1e-15)
