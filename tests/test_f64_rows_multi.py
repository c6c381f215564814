"""LBM_ROWS64_FLAG_MULTI_STEPS on the GPU: row-partitioned double-precision runs that advance K steps per launch and exchange
(lbm_rows_multi_kernel_f64 and lbm64_push_ghost_rows_kernel, csrc/kernels/rows_multi64.h; the host loop in csrc/lbm_rows64.hip), held
to the CPU restatement tests/f64_ref.c with tests/test_f64_rows.py's protocol: populations bit for bit, av_vels within the bound of the
summation tree.  All ranks run on device 0; one test switches itself on where there are two GPUs or more.  Every run asserts the
kernel's name, so that a fallback to the one-step kernel cannot pass for the kernel.

THE av_vels BOUND.  A rank's sum of a step is formed by lbm_multi_kernel_f64's tree over the rank's tiles, whose relative error against
the exactly rounded sum is tests/test_f64_multi.py's multi_sum_bound(tiles) less its two roundings of the product (every term is
non-negative, so each addition errs by at most 2^-53 of its result, which is at most the total; the bound counts the longest chain of
additions a term passes through, and grows with the tiles: the rank with the most tiles has the longest).  The host then adds the ranks'
sums in rank order: nranks - 1 more additions in the chain.  Then the product with 1.0 / free_cells on both sides, which
multi_sum_bound counts.  So: multi_sum_bound(tiles of the largest rank) + (nranks - 1) * 2^-53."""
import os
import subprocess

import numpy as np
import pytest

import f64_ref
from conftest import deck_paths
from test_f64_multi import multi_sum_bound
from test_f64_rows import U, _bits, _deck, _random_state, _reference, _synthetic

pytestmark = pytest.mark.gpu

TX, TY = 32, 16


@pytest.fixture(scope="module")
def f64(lbm):
    from mpilattice_boltzmann_amd import f64 as mod
    mod.load_rows_library()
    return mod


def _force(monkeypatch, K=None):
    """A run reads the knobs when it is made.  The tests choose the kernel by shape, not by the minimum size; K None: the default."""
    monkeypatch.setenv("LBM_TUNE_MULTI64_MIN", "0")
    if K is None:
        monkeypatch.delenv("LBM_TUNE_MULTI64_K", raising=False)
    else:
        monkeypatch.setenv("LBM_TUNE_MULTI64_K", str(K))
    monkeypatch.delenv("LBM_TUNE_MAXBLOCKS", raising=False)


def _kernel_name(K, nt=False):
    return f"lbm_rows_multi_kernel_f64<{K},nt>" if nt else f"lbm_rows_multi_kernel_f64<{K}>"


def rows_multi_sum_bound(tiles, nranks):
    """The module docstring's bound."""
    return multi_sum_bound(tiles) + (nranks - 1) * U


def _check_av(av, exact, obst, tiles, nranks):
    ref = f64_ref.av_vels(exact, obst)
    assert av.shape == ref.shape
    # (a deck whose accelerated row is blocked stays at rest: every entry is 0 on both sides, and the error is taken absolutely)
    err = float(np.max(np.abs(av - ref) / ref)) if np.all(ref > 0) else float(np.max(np.abs(av - ref)))
    bound = rows_multi_sum_bound(tiles, nranks)
    print(f"  av_vels on {nranks} ranks of {tiles} tiles: {err / U:.2f} x 2^-53 against a bound of {bound / U:.0f} x 2^-53")
    assert err <= bound


def _check_desc(desc, p, nranks, K, nt=False):
    tiles = (p.nx // TX) * (p.ny // nranks // TY)
    assert desc["kernel"] == _kernel_name(K, nt), desc
    assert desc["nranks"] == nranks and desc["blocks"] == tiles and desc["cells_per_block"] == TX * TY, desc
    assert desc["state_bytes"] == 2 * 9 * 8 * p.nx * (p.ny + 2 * K * nranks), desc
    return tiles


def _parity(f64, key, p, obst, nranks, K, flags=None, nt=False, devices=None):
    """tests/test_f64_rows.py's protocol and its references (computed once per deck, shared with that file's tests).  37 steps from
    rest: at K = 4 nine full launches and a one-step tail, the direct-store form.  Then run(5) + run(7) from a random positive state
    against 12 steps: the accelerate that run(5) skipped after its last step is run(7)'s pre-pass, whose row push -1 then sends."""
    ref37, exact37, state, ref12, exact12 = _reference(key, p, obst)
    assert p.ny % (TY * nranks) == 0 and p.nx % TX == 0
    with f64.Rows64(p, obst, nranks, devices=devices if devices is not None else [0] * nranks,
                    flags=f64.FLAG_ROWS_MULTI_STEPS if flags is None else flags) as g:
        desc = g.describe()
        tiles = _check_desc(desc, p, nranks, K, nt)
        av = g.run(37)
        assert g.last_run_ms()[1] == -(-37 // K) * nranks
        assert np.array_equal(_bits(g.get_cells()), _bits(ref37)), f"{p.nx}x{p.ny} on {nranks} ranks, 37 steps from rest: {desc}"
        _check_av(av, exact37, obst, tiles, nranks)
        g.set_cells(state)
        av = np.concatenate([g.run(5), g.run(7)])
        assert g.last_run_ms()[1] == -(-7 // K) * nranks
        assert np.array_equal(_bits(g.get_cells()), _bits(ref12)), f"{p.nx}x{p.ny} on {nranks} ranks, run(5) + run(7) from a random state: {desc}"
        assert ref12.min() > 0.0                         # the premise of the bound: positive densities, non-negative terms
        _check_av(av, exact12, obst, tiles, nranks)
    return desc


# ---- the smallest shapes at which each thing can go wrong ---------------------------------------------------------------------------

# 32 x 16 on 1 rank: one tile meets itself in x; the rank is its own neighbour.  32 x 32 on 2: both neighbours are the same rank; row
# ny-2 sits in rank 0's lower ghost rows.  64 x 64 on 4: distinct neighbours, two tile columns.  96 x 32 on 1: two tile rows in a rank.
SHAPES = [(32, 16, 1, 4), (32, 32, 2, 2), (32, 32, 2, 3), (32, 32, 2, 4), (64, 64, 4, 4), (96, 32, 1, 4)]


@pytest.mark.parametrize("nx,ny,nranks,K", SHAPES)
def test_bit_parity_shapes(lbm, f64, monkeypatch, nx, ny, nranks, K):
    p, obst = _synthetic(lbm, nx, ny)
    _force(monkeypatch, K)
    _parity(f64, ("shape", nx, ny), p, obst, nranks, K)


# rand_64x48 on 3 ranks of 16 rows: two tile columns, three distinct neighbours.  The two 32 x 16 decks on 1 rank: blocked cells and
# strong forcing on the accelerated row, whose copies sit in the rank's own lower ghost rows and in the frame's ring.
DECKS = [("rand_64x48", 3, 2), ("rand_64x48", 3, 3), ("rand_64x48", 3, 4), ("accelrow_blocked_32x16", 1, 4), ("strongaccel_32x16", 1, 4)]


@pytest.mark.parametrize("name,nranks,K", DECKS)
def test_bit_parity_decks(f64, digests, monkeypatch, name, nranks, K):
    p, obst = _deck(f64, digests, name)
    _force(monkeypatch, K)
    _parity(f64, name, p, obst, nranks, K)


@pytest.mark.parametrize("flag,nt", [("FLAG_NT_STORES", True), ("FLAG_NO_NT_STORES", False)])
def test_bit_parity_under_the_nt_flags(f64, digests, monkeypatch, flag, nt):
    p, obst = _deck(f64, digests, "rand_64x48")
    _force(monkeypatch, 4)
    _parity(f64, "rand_64x48", p, obst, 3, 4, flags=f64.FLAG_ROWS_MULTI_STEPS | getattr(f64, flag), nt=nt)


def test_the_four_ways_to_run_a_grid_give_the_same_populations(f64, digests, monkeypatch):
    """12 steps from one random state: Rows64 with the flag, Rows64 without it, Grid64, Grid64 with FLAG_MULTI_STEPS."""
    p, obst = _deck(f64, digests, "rand_64x48")
    _force(monkeypatch)
    state = _random_state(p, seed=21)
    got = {}
    for tag, make in (("rows multi", lambda: f64.Rows64(p, obst, 3, devices=[0] * 3, flags=f64.FLAG_ROWS_MULTI_STEPS)),
                      ("rows", lambda: f64.Rows64(p, obst, 3, devices=[0] * 3)),
                      ("grid", lambda: f64.Grid64(p, obst)),
                      ("grid multi", lambda: f64.Grid64(p, obst, flags=f64.FLAG_MULTI_STEPS))):
        with make() as g:
            kernel = g.describe()["kernel"]
            g.set_cells(state)
            g.run(12)
            got[tag] = (kernel, _bits(g.get_cells()))
    assert got["rows multi"][0].startswith("lbm_rows_multi_kernel_f64<") and got["rows"][0] == "lbm_rows_kernel_f64<2>"
    assert got["grid"][0] == "lbm_step_kernel_f64<2>" and got["grid multi"][0].startswith("lbm_multi_kernel_f64<")
    for tag in ("rows", "grid", "grid multi"):
        assert np.array_equal(got["rows multi"][1], got[tag][1]), tag


def test_two_identical_runs_give_identical_av_vels(f64, digests, monkeypatch):
    p, obst = _deck(f64, digests, "rand_64x48")
    _force(monkeypatch)
    state = _random_state(p, seed=3)
    got = []
    for _ in range(2):
        with f64.Rows64(p, obst, 3, devices=[0, 0, 0], flags=f64.FLAG_ROWS_MULTI_STEPS) as g:
            assert g.describe()["kernel"].startswith("lbm_rows_multi_kernel_f64<")
            g.set_cells(state)
            got.append((g.run(22), g.get_cells()))
    assert np.array_equal(_bits(got[0][0]), _bits(got[1][0])) and np.array_equal(_bits(got[0][1]), _bits(got[1][1]))
    assert np.all(got[0][0] > 0)


def test_uneven_ranks_fall_back(lbm, f64, monkeypatch):
    """258 x 33 on 4 ranks (rows 9, 8, 8, 8) with the flag: the one-step kernel, exactly as without it."""
    _force(monkeypatch)
    p, obst = _synthetic(lbm, 258, 33)
    state = _random_state(p, seed=5)
    out = {}
    for flags in (0, f64.FLAG_ROWS_MULTI_STEPS):
        with f64.Rows64(p, obst, 4, devices=[0] * 4, flags=flags) as g:
            desc = g.describe()
            g.set_cells(state)
            out[flags] = (desc, g.run(9), g.get_cells(), g.last_run_ms()[1])
    off, on = out[0], out[f64.FLAG_ROWS_MULTI_STEPS]
    assert on[0] == off[0] and on[0]["kernel"] == "lbm_rows_kernel_f64<2>", on[0]
    assert on[3] == off[3] == 9 * 4
    assert np.array_equal(_bits(on[1]), _bits(off[1])) and np.array_equal(_bits(on[2]), _bits(off[2]))


# tests/test_f64_edges.py's MOVED and PATCH_BITS.  NaNs with payloads (signalling and quiet), infinities, huge values: a cell that pulls
# one of these holds a NaN a step later (inf - inf, or an overflow first), and the NaNs spread by a cell per step ...
EDGE_NAN_BITS = np.array([0x7FF4000000ABCDEF, 0xFFF8000012345678, 0x7FF0000000000001, 0x7FF0000000000000, 0xFFF0000000000000,
                          0x7FB0000000000000, 0xFFB0000000000000, 0x7FEFFFFFFFFFFFFF], np.uint64)
# ... both zeros and denormals: these stay numbers
EDGE_NUMBER_BITS = np.array([0x0000000000000000, 0x8000000000000000, 0x0000000000000001, 0x800FFFFFFFFFFFFF, 0x0000000000000ABC], np.uint64)


def test_edge_values_on_the_pushed_rows(lbm, f64, monkeypatch):
    """32 x 32 on 2 ranks, K = 4: a random positive state with EDGE_BITS written into populations of the first and last K rows of each
    rank — the rows a push sends, which the neighbour's launch then recomputes as ring cells.  5 steps (a full launch and a one-step
    tail) against the unflagged Rows64 run, by tests/test_f64_edges.py's rule: the same cells hold NaNs, and every number is the same
    bits (which of two NaN operands' payloads a sum keeps is the compiler's choice of operand order in each kernel; a NaN is a NaN on
    both sides).  What makes NaNs sits in column 14 alone: after 5 steps they reach columns 9 to 19, a third of the grid, and the
    zeros and denormals of columns 3 and 25 are still among numbers."""
    K, nranks = 4, 2
    p, obst = _synthetic(lbm, 32, 32, p_block=0.1, seed=5)
    _force(monkeypatch, K)
    state = _random_state(p, seed=13).copy()
    bits = _bits(state)
    rows = [r * 16 + i for r in range(nranks) for i in list(range(K)) + list(range(16 - K, 16))]
    n = 0
    for y in rows:
        for x, patterns in ((3, EDGE_NUMBER_BITS), (14, EDGE_NAN_BITS), (25, EDGE_NUMBER_BITS)):
            for k in ((n % 9), ((n + 4) % 9)):
                bits[y, x, k] = patterns[n % patterns.size]
                n += 1
    assert n >= 4 * (EDGE_NAN_BITS.size + EDGE_NUMBER_BITS.size)
    out = {}
    for flags in (0, f64.FLAG_ROWS_MULTI_STEPS):
        with f64.Rows64(p, obst, nranks, devices=[0] * nranks, flags=flags) as g:
            kernel = g.describe()["kernel"]
            g.set_cells(state)
            assert np.array_equal(_bits(g.get_cells()), bits)
            g.run(5)
            out[flags] = (kernel, g.get_cells())
    (k_off, ref), (k_on, got) = out[0], out[f64.FLAG_ROWS_MULTI_STEPS]
    assert k_off == "lbm_rows_kernel_f64<2>" and k_on == _kernel_name(K)
    nan_ref, nan_got = np.isnan(ref), np.isnan(got)
    print(f"  {float(np.mean(nan_ref.any(axis=2))):.1%} of the cells hold a NaN after 5 steps, {int(np.isinf(ref).sum())} infinities, {int((ref == 0).sum())} zeros")
    assert 0.02 <= float(np.mean(nan_ref.any(axis=2))) <= 0.75 and not nan_ref[:, :4].any() and not nan_ref[:, 24:].any()
    assert np.array_equal(nan_ref, nan_got), f"{int(np.sum(nan_ref != nan_got))} NaNs misplaced"
    differ = ~nan_ref & (_bits(got) != _bits(ref))
    assert not differ.any(), f"{int(differ.sum())} numbers differ, first at {tuple(np.argwhere(differ)[0])}"


# ---- at the sizes the mode is for ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def deck1024(f64, digests):
    """The 1024 x 1024 deck and 7 steps of the restatement on it, once."""
    p, obst = _deck(f64, digests, "1024x1024_t200")
    ref_cells, _, exact = f64_ref.run(p, obst, 7, nthreads=16)
    for a in (ref_cells, exact):
        a.setflags(write=False)
    return p, obst, ref_cells, exact


def _run_1024(f64, deck1024, devices):
    """7 steps: a full launch of 4 and a tail of 3.  (A rank of 8 is 2^17 cells: the default minimum for ranks; the callers lower it to 0.)"""
    p, obst, ref_cells, exact = deck1024
    nranks = len(devices)
    with f64.Rows64(p, obst, nranks, devices=devices, flags=f64.FLAG_ROWS_MULTI_STEPS) as g:
        desc = g.describe()
        tiles = _check_desc(desc, p, nranks, 4)
        av = g.run(7)
        cells = g.get_cells()
        ms, launches = g.last_run_ms()
    assert np.array_equal(_bits(cells), _bits(ref_cells)), desc
    _check_av(av, exact, obst, tiles, nranks)
    assert launches == 2 * nranks and ms > 0.0
    assert desc["state_bytes"] == 2 * 9 * 8 * 1024 * (1024 + 2 * 4 * nranks)


def test_bit_parity_1024x1024_deck_7_steps_on_8_ranks(f64, deck1024, monkeypatch):
    _force(monkeypatch)
    _run_1024(f64, deck1024, [0] * 8)


def test_whole_128x128_deck_on_4_ranks_bits_and_shipped_results(lbm, f64, monkeypatch):
    """40 000 steps on 4 ranks of 32 rows, the library's default K: about a second on the device.  The restatement's run is
    f64_ref.deck_run's, once per process."""
    _force(monkeypatch)
    p, obst, ref_cells, serial, exact = f64_ref.deck_run("128x128")
    p64 = f64.read_params64(os.path.join(f64_ref.GOLDEN, "decks", "input_128x128.params"))
    assert (p64.density, p64.accel, p64.omega) == (p.density, p.accel, p.omega)
    with f64.Rows64(p64, obst, 4, devices=[0] * 4, flags=f64.FLAG_ROWS_MULTI_STEPS) as g:
        desc = g.describe()
        assert desc["kernel"].startswith("lbm_rows_multi_kernel_f64<"), desc
        K = int(desc["kernel"][len("lbm_rows_multi_kernel_f64<"):-1])
        tiles = _check_desc(desc, p64, 4, K)
        av = g.run(p64.max_iters)
        ms, launches = g.last_run_ms()
        cells = g.get_cells()
        obs = g.get_observables()
        re = g.reynolds()
    assert launches == -(-p64.max_iters // K) * 4
    print(f"  128x128 on 4 ranks, {p64.max_iters} steps with {desc['kernel']}: {ms:.1f} ms in {launches} launches")
    assert np.array_equal(_bits(cells), _bits(ref_cells)), "populations after 40 000 steps"
    _check_av(av, exact, obst, tiles, 4)
    # against what the reference shipped: the CPU test's limits (f64_ref) plus the summation bound
    golden_av = f64_ref.golden_av_vels("128x128")
    av_rel = float(np.max(np.abs(av - golden_av) / np.abs(golden_av)))
    values = obs.copy()
    values[obst != 0] = (0.0, 0.0, 0.0, p.density * (1.0 / 3.0))
    fs_abs = float(np.max(np.abs(values.reshape(-1, 4) - f64_ref.golden_final_state("128x128"))))
    pub = float(f64_ref.published()["reynolds"]["128x128"]["value"])
    print(f"  against the shipped results: av_vels {av_rel:.3e} rel, final_state {fs_abs:.3e} abs, Reynolds {re!r}")
    assert av_rel <= f64_ref.AV_VELS_LIMIT + rows_multi_sum_bound(tiles, 4)
    assert fs_abs <= f64_ref.FINAL_STATE_LIMIT
    assert abs(re - pub) / pub <= f64_ref.REYNOLDS_LIMIT


def test_cli_row_blocks_with_the_flag(lbm, f64, digests, tmp_path):
    """LBM_PRECISION=double LBM64_RANKS=3 LBM_FLAGS=2048 bin/d2q9-bgk on rand_64x48: final_state.dat and the Reynolds line are those of
    LBM_PRECISION=double alone, and LBM_DESCRIBE's line names the new kernel with 3 * ceil(max_iters / K) launches."""
    ppath, opath = deck_paths("rand_64x48", digests)
    p, _ = _deck(f64, digests, "rand_64x48")
    env = {k: v for k, v in os.environ.items() if not k.startswith("LBM")}
    env["LBM_PRECISION"] = "double"
    out = {}
    for tag, extra in (("whole", {}), ("rows", dict(LBM64_RANKS="3", LBM_DEVICES="0,0,0", LBM_FLAGS="2048", LBM_TUNE_MULTI64_MIN="0", LBM_DESCRIBE="1"))):
        cwd = tmp_path / tag
        cwd.mkdir()
        r = subprocess.run([lbm.CLI_PATH, ppath, opath], cwd=cwd, env={**env, **extra}, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        out[tag] = (r.stdout.splitlines(), (cwd / "final_state.dat").read_bytes(), r.stderr)
    lines = out["rows"][0]
    assert lines[0] == "==done==" and lines[5].endswith("(3 ranks, double precision)")
    assert lines[1].startswith("Reynolds number:\t\t") and lines[1] == out["whole"][0][1]
    assert out["rows"][1] == out["whole"][1]
    ran = [line for line in out["rows"][2].splitlines() if line.startswith("kernel: ")]
    assert len(ran) == 1 and ran[0].startswith("kernel: lbm_rows_multi_kernel_f64<"), out["rows"][2]
    K = int(ran[0][len("kernel: lbm_rows_multi_kernel_f64<"):ran[0].index(">")])
    assert K in (2, 3, 4) and ran[0] == f"kernel: lbm_rows_multi_kernel_f64<{K}> on 3 ranks, {3 * -(-p.max_iters // K)} launches", ran[0]


def test_one_gpu_per_rank(f64, digests, deck1024, monkeypatch):
    """Switches itself on where there are at least 2 GPUs: the K rows of a push then travel as stores over a real link.  The rand_64x48
    parity on devices 0 and 1 needs 24 rows a rank, which the tiles do not cover, so it runs rand_64x48 on 3 ranks over devices 0, 1, 0;
    and the 1024 x 1024 deck's 7 steps on one rank per device, the largest power of two of them, 8 at most."""
    import torch
    count = torch.cuda.device_count()
    if count < 2:
        pytest.skip(f"needs 2 GPUs, this box has {count}")
    _force(monkeypatch, 4)
    p, obst = _deck(f64, digests, "rand_64x48")
    _parity(f64, "rand_64x48", p, obst, 3, 4, devices=[0, 1, 0])
    n = 2
    while 2 * n <= min(count, 8):
        n *= 2
    _run_1024(f64, deck1024, list(range(n)))
