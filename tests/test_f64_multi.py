"""LBM64_FLAG_MULTI_STEPS on the GPU: lbm_multi_kernel_f64<K> (csrc/kernels/multi64.h), several steps per launch of the double-precision
mode on 32 x 16 tiles with an in-place LDS frame, held to the CPU restatement tests/f64_ref.c with tests/test_f64_tile.py's recipe:
populations bit for bit for every built K, on a grid of one tile (whose frame wraps onto itself), for every length of a run's last
launch and both store forms; av_vels within the bound of the launch's summation tree; the fallbacks; the read-outs; the whole
128 x 128 deck against the results the reference shipped, and through the CLI."""
import functools
import os
import subprocess

import numpy as np
import pytest

import f64_ref
from test_f64 import U, _bits, _deck, _random_state, _synthetic, big_grid_case, big_grid_compare
from test_f64 import sum_bound as step_sum_bound

pytestmark = pytest.mark.gpu

BUILT_K = (2, 3, 4)                 # every K the kernel is built for (lbm_geometry.h)
TX, TY, LANES = 32, 16, 512         # the tile and the lanes of a block


@pytest.fixture(scope="module")
def f64(lbm):
    from mpilattice_boltzmann_amd import f64 as mod
    mod.load_library()
    return mod


def _force(monkeypatch, K):
    """A context reads the knobs when it is made.  The tests choose the kernel by shape, not by the measured minimum size."""
    monkeypatch.setenv("LBM_TUNE_MULTI64_K", str(K))
    monkeypatch.setenv("LBM_TUNE_MULTI64_MIN", "0")
    monkeypatch.delenv("LBM_TUNE_TILE64_MAX", raising=False)
    monkeypatch.delenv("LBM_TUNE_TILE64_GEOM", raising=False)


def multi_sum_bound(tiles):
    """Relative error of one av_vels entry of a run of lbm_multi_kernel_f64 against the exactly rounded sum times 1.0 / free_cells: (the
    longest chain of additions a term passes through + 2) * 2^-53, from the tree include/lbm_d2q9_f64.h states.  Every term is
    non-negative and the same double on both sides, so each addition errs by at most 2^-53 of its result, which is at most the total.
      in the tile's block (512 lanes)   2        a lane adds the owned cells it meets in that sub-step: at most two (the x-pair of
                                                 sub-step 1, the two items of a frame sub-step)
                                        6        butterfly levels over the 64 lanes of a wave
                                        7        one lane adds the eight waves' sums serially
      in the fold (F lanes)             ceil(tiles / F) + 6 + F/64 - 1; F = 512 in block 0 of the next launch, 256 in the last fold of a
                                        run: the larger of the two
      2                                 the product with 1.0 / free_cells, on this side and on the reference's."""
    in_tile = 2 + 6 + LANES // 64 - 1
    fold = max(-(-tiles // F) + 6 + F // 64 - 1 for F in (LANES, 256))
    return (in_tile + fold + 2) * U


def _av_err(av, exact, obst):
    ref = f64_ref.av_vels(exact, obst)
    assert av.shape == ref.shape
    # (a deck whose accelerated row is blocked stays at rest: every entry is 0 on both sides, and the error is taken absolutely)
    return float(np.max(np.abs(av - ref) / ref)) if np.all(ref > 0) else float(np.max(np.abs(av - ref)))


def _check_av_multi(av, exact, obst, K, tiles):
    err, bound = _av_err(av, exact, obst), multi_sum_bound(tiles)
    print(f"  av_vels <{K}> on {tiles} tiles: {err / U:.2f} x 2^-53 against a bound of {bound / U:.0f} x 2^-53")
    assert bound <= 64 * U           # a loose bound would hide a miscounted ring cell (an error of about 1 / cells >> 1e-14)
    assert err <= bound


# ---- references, each computed once and never written to --------------------------------------------------------------------

_CASES = {}


@functools.lru_cache(maxsize=None)
def _reference(key):
    """key: a deck name or (nx, ny).  37 steps from rest, and 12 steps from the rest state x U[0.8, 1.2)."""
    p, obst = _CASES[key]
    rest = f64_ref.run(p, obst, 37)
    state = _random_state(p)
    rand = f64_ref.run(p, obst, 12, cells0=state)
    for a in (obst, state, rest[0], rest[2], rand[0], rand[2]):
        a.setflags(write=False)
    return p, obst, rest, state, rand


def _case(key, p, obst):
    _CASES.setdefault(key, (p, obst))
    return _reference(key)


@functools.lru_cache(maxsize=None)
def _run_reference(key, seed, steps):
    p, obst = _CASES[key]
    state = _random_state(p, seed=seed)
    cells, _, exact = f64_ref.run(p, obst, steps, cells0=state)
    for a in (state, cells, exact):
        a.setflags(write=False)
    return state, cells, exact


def _kernel_name(K, nt=False):
    return f"lbm_multi_kernel_f64<{K},nt>" if nt else f"lbm_multi_kernel_f64<{K}>"


def _parity_multi(f64, ref, K, flags=None, nt=False):
    """tests/test_f64.py's _parity with the flag: 37 steps from rest (full launches and, for K = 2, 3 and 4, a 1-step tail), then
    run(5) + run(7) from a random positive state against 12 steps."""
    p, obst, (ref37, _, exact37), state, (ref12, _, exact12) = ref
    tiles = (p.nx // TX) * (p.ny // TY)
    with f64.Grid64(p, obst, flags=f64.FLAG_MULTI_STEPS if flags is None else flags) as g:
        desc = g.describe()
        assert desc["kernel"] == _kernel_name(K, nt) and desc["blocks"] == tiles and desc["cells_per_block"] == TX * TY, desc
        av = g.run(37)
        assert g.last_run_kernel_ms()[1] == -(-37 // K)
        assert np.array_equal(_bits(g.get_cells()), _bits(ref37)), f"{p.nx}x{p.ny} 37 steps from rest: {desc}"
        _check_av_multi(av, exact37, obst, K, tiles)
        g.set_cells(state)
        av = np.concatenate([g.run(5), g.run(7)])
        assert g.last_run_kernel_ms()[1] == -(-7 // K)
        assert np.array_equal(_bits(g.get_cells()), _bits(ref12)), f"{p.nx}x{p.ny} run(5) + run(7) from a random state: {desc}"
        assert ref12.min() > 0.0                         # the premise of the bound: positive densities, non-negative terms
        _check_av_multi(av, exact12, obst, K, tiles)
    return desc


SHAPES = [(32, 16), (64, 16), (32, 32), (96, 48)]
DECKS = ["accelrow_blocked_32x16", "strongaccel_32x16", "dense_32x32", "rand_64x48"]


@pytest.mark.parametrize("K", BUILT_K)
@pytest.mark.parametrize("nx,ny", SHAPES)
def test_bit_parity_shapes(lbm, f64, monkeypatch, nx, ny, K):
    """32 x 16: one tile, whose frame wraps onto itself in x and in y and holds row ny-2 twice; 64 x 16 and 32 x 32: two tiles wide /
    tall; 96 x 48: 3 x 3 tiles, every neighbour of the middle one distinct."""
    p, obst = _synthetic(lbm, nx, ny, seed=nx + ny)
    _force(monkeypatch, K)
    _parity_multi(f64, _case((nx, ny), p, obst), K)


@pytest.mark.parametrize("K", BUILT_K)
@pytest.mark.parametrize("name", DECKS)
def test_bit_parity_decks(f64, digests, monkeypatch, name, K):
    p, obst = _deck(f64, digests, name)
    assert p.nx % TX == 0 and p.ny % TY == 0
    _force(monkeypatch, K)
    _parity_multi(f64, _case(name, p, obst), K)


@pytest.mark.parametrize("K", BUILT_K)
def test_every_tail(f64, digests, monkeypatch, K):
    """run(k) for k = 1 .. K-1 (n < K: one launch that is not FULL, after the accelerate pre-pass and with no accelerate after its last
    sub-step), run(K) (one FULL launch), and run(2K + k): every tail length after full launches.  Each from a fresh random state."""
    name = "rand_64x48"
    p, obst = _deck(f64, digests, name)
    _case(name, p, obst)
    tiles = (p.nx // TX) * (p.ny // TY)
    _force(monkeypatch, K)
    with f64.Grid64(p, obst, flags=f64.FLAG_MULTI_STEPS) as g:
        assert g.describe()["kernel"] == _kernel_name(K)
        for n in list(range(1, K + 1)) + [2 * K + k for k in range(1, K)]:
            state, ref_cells, exact = _run_reference(name, 100 + n, n)
            g.set_cells(state)
            av = g.run(n)
            assert g.last_run_kernel_ms()[1] == -(-n // K)
            assert np.array_equal(_bits(g.get_cells()), _bits(ref_cells)), f"run({n}) under K = {K}"
            assert ref_cells.min() > 0.0
            _check_av_multi(av, exact, obst, K, tiles)


@pytest.mark.parametrize("K", BUILT_K)
@pytest.mark.parametrize("flag,nt", [("FLAG_NT_STORES", True), ("FLAG_NO_NT_STORES", False)])
def test_both_store_forms(f64, digests, monkeypatch, flag, nt, K):
    p, obst = _deck(f64, digests, "rand_64x48")
    _force(monkeypatch, K)
    _parity_multi(f64, _case("rand_64x48", p, obst), K, flags=f64.FLAG_MULTI_STEPS | getattr(f64, flag), nt=nt)


@pytest.mark.parametrize("K", BUILT_K)
def test_flag_on_against_flag_off(f64, digests, monkeypatch, K):
    p, obst = _deck(f64, digests, "rand_64x48")
    _force(monkeypatch, K)
    state = _random_state(p, seed=21)
    out = {}
    for flags in (0, f64.FLAG_MULTI_STEPS):
        with f64.Grid64(p, obst, flags=flags) as g:
            g.set_cells(state)
            out[flags] = (g.describe(), np.concatenate([g.run(11), g.run(2 * K)]), g.get_cells())
    (d_off, av_off, cells_off), (d_on, av_on, cells_on) = out[0], out[f64.FLAG_MULTI_STEPS]
    assert d_off["kernel"] == "lbm_step_kernel_f64<2>" and d_on["kernel"] == _kernel_name(K)
    assert np.array_equal(_bits(cells_on), _bits(cells_off))
    assert cells_off.min() > 0.0
    bound = step_sum_bound(d_off) + multi_sum_bound(d_on["blocks"])
    assert float(np.max(np.abs(av_on - av_off) / av_off)) <= bound


def test_with_the_tile_flag_too(f64, digests, monkeypatch):
    """512 | 1024: the tiled kernel where it takes the grid, the new one above its size cap."""
    p, obst = _deck(f64, digests, "rand_64x48")
    _force(monkeypatch, 3)
    with f64.Grid64(p, obst, flags=f64.FLAG_TILE_STEPS | f64.FLAG_MULTI_STEPS) as g:
        assert g.describe()["kernel"].startswith("lbm_tile_kernel_f64<")
    monkeypatch.setenv("LBM_TUNE_TILE64_MAX", str(64 * 48 - 1))
    _parity_multi(f64, _case("rand_64x48", p, obst), 3, flags=f64.FLAG_TILE_STEPS | f64.FLAG_MULTI_STEPS)


def _step_kernel_exactly_as_without_the_flag(f64, ref):
    p, obst, (ref37, _, exact37), state, (ref12, _, exact12) = ref
    with f64.Grid64(p, obst, flags=0) as g:
        off = (g.describe(), g.run(37), g.get_cells(), g.last_run_kernel_ms()[1])
    with f64.Grid64(p, obst, flags=f64.FLAG_MULTI_STEPS) as g:
        desc = g.describe()
        assert desc == off[0] and desc["kernel"] == f"lbm_step_kernel_f64<{2 if p.nx % 2 == 0 else 1}>", desc
        av = g.run(37)
        assert g.last_run_kernel_ms()[1] == off[3] == 37
        assert np.array_equal(_bits(g.get_cells()), _bits(off[2])) and np.array_equal(_bits(off[2]), _bits(ref37))
        assert np.array_equal(_bits(av), _bits(off[1]))
        g.set_cells(state)
        av = np.concatenate([g.run(5), g.run(7)])
        assert np.array_equal(_bits(g.get_cells()), _bits(ref12))
        assert ref12.min() > 0.0 and _av_err(av, exact12, obst) <= step_sum_bound(desc)


@pytest.mark.parametrize("shape", [(40, 24), (258, 33)])
def test_fallbacks_with_the_flag(lbm, f64, monkeypatch, shape):
    """Grids the tiles do not cover run lbm_step_kernel_f64 exactly as without the flag."""
    _force(monkeypatch, 3)
    p, obst = _synthetic(lbm, *shape)
    _step_kernel_exactly_as_without_the_flag(f64, _case(shape, p, obst))


def test_a_grid_below_the_minimum_falls_back(f64, digests, monkeypatch):
    p, obst = _deck(f64, digests, "rand_64x48")
    _force(monkeypatch, 3)
    monkeypatch.setenv("LBM_TUNE_MULTI64_MIN", str(64 * 48 + 1))
    _step_kernel_exactly_as_without_the_flag(f64, _case("rand_64x48", p, obst))
    monkeypatch.setenv("LBM_TUNE_MULTI64_MIN", str(64 * 48))
    with f64.Grid64(p, obst, flags=f64.FLAG_MULTI_STEPS) as g:
        assert g.describe()["kernel"] == _kernel_name(3)


def test_the_float_path_ignores_the_bit(lbm, f64, digests):
    """lbm_create of lbm_d2q9.h: the same kernel, launch and bits with 1024 as with 0, as with 512."""
    p, obst = _deck(f64, digests, "rand_64x48")
    out = {}
    for flags in (0, f64.FLAG_MULTI_STEPS):
        q = lbm.Partition(p, lbm.count_free_cells(obst), obst, flags=flags)
        try:
            out[flags] = (q.describe(), q.run(9), q.get_cells())
        finally:
            q.close()
    assert out[0][0] == out[f64.FLAG_MULTI_STEPS][0]
    assert np.array_equal(out[0][1], out[f64.FLAG_MULTI_STEPS][1])
    assert np.array_equal(out[0][2].view(np.uint32), out[f64.FLAG_MULTI_STEPS][2].view(np.uint32))


def test_read_outs_after_a_multi_step_run(f64, digests, monkeypatch):
    p, obst = _deck(f64, digests, "rand_64x48")
    _force(monkeypatch, 3)
    with f64.Grid64(p, obst, flags=f64.FLAG_MULTI_STEPS) as g:
        assert g.describe()["kernel"] == _kernel_name(3)
        g.set_cells(_random_state(p, seed=9))
        g.run(19)
        cells, obs, tot, re = g.get_cells(), g.get_observables(), g.av_velocity_sum(), g.reynolds()
    ref_cells, _, _ = f64_ref.run(p, obst, 19, cells0=_random_state(p, seed=9))
    assert np.array_equal(_bits(cells), _bits(ref_cells))
    assert np.array_equal(_bits(obs), _bits(f64_ref.observables(ref_cells)))
    assert re == f64_ref.reynolds(p, ref_cells, obst)
    n = p.nx * p.ny
    blocks = min(-(-n // 256), 1024)
    exact = f64_ref.velocity_sum_exact(ref_cells, obst)
    assert abs(tot - exact) <= (-(-n // (blocks * 256)) + 9 + blocks) * U * exact       # tests/test_f64.py: lbm64_av_velocity_sum's own tree


# ---- the kernel at its own sizes ----------------------------------------------------------------------------------------------------

def _no_knobs(monkeypatch):
    for k in [k for k in os.environ if k.startswith("LBM_TUNE_")]:
        monkeypatch.delenv(k)


@pytest.mark.parametrize("K", (4, 3))
@pytest.mark.parametrize("nx,ny", [(1024, 144), (1024, 272)])
def test_folds_that_take_a_second_stride(lbm, f64, monkeypatch, nx, ny, K):
    """More tiles than a fold has lanes.  1024 x 144 is 288 tiles: the last fold of a run (lbm64_fold_kernel, 256 lanes) takes a second
    stride for 32 of its lanes.  1024 x 272 is 544 tiles: the fold block of the next launch (512 lanes) does too, over a ragged
    remainder of 32, and the last fold takes three.  20 % obstacles, a random state, run(K + 1) then run(2 K): a full launch and a tail,
    then two full launches; the sums of every launch but the last of each run pass through the fold block, the last through the fold kernel."""
    p, obst = _synthetic(lbm, nx, ny, seed=nx + ny)
    tiles = (nx // TX) * (ny // TY)
    assert tiles > 256 and (ny != 272 or tiles > LANES) and tiles % 256 != 0
    _force(monkeypatch, K)
    state = _random_state(p, seed=17)
    ref_mid, _, exact_mid = f64_ref.run(p, obst, K + 1, cells0=state, nthreads=16)
    ref_end, _, exact_end = f64_ref.run(p, obst, 2 * K, cells0=ref_mid, nthreads=16)
    with f64.Grid64(p, obst, flags=f64.FLAG_MULTI_STEPS) as g:
        desc = g.describe()
        assert desc["kernel"] == _kernel_name(K) and desc["blocks"] == tiles, desc
        g.set_cells(state)
        av_mid = g.run(K + 1)
        assert g.last_run_kernel_ms()[1] == 2
        assert np.array_equal(_bits(g.get_cells()), _bits(ref_mid)), f"{nx}x{ny} run({K + 1}): {desc}"
        av_end = g.run(2 * K)
        assert g.last_run_kernel_ms()[1] == 2
        assert np.array_equal(_bits(g.get_cells()), _bits(ref_end)), f"{nx}x{ny} run({K + 1}) + run({2 * K}): {desc}"
    assert ref_end.min() > 0.0
    _check_av_multi(np.concatenate([av_mid, av_end]), np.concatenate([exact_mid, exact_end]), obst, K, tiles)


def test_default_plan_on_the_1024x1024_deck(f64, digests, monkeypatch):
    """The flag alone, no knob in the environment: what a user of LBM64_FLAG_MULTI_STEPS gets at the size the default begins at.
    K = 4 on 2048 tiles, 11 steps (two full launches and a 3-step tail) from a state that differs from cell to cell."""
    _no_knobs(monkeypatch)
    p, obst = _deck(f64, digests, "1024x1024_t200")
    y, x = np.arange(p.ny, dtype=np.float64)[:, None, None], np.arange(p.nx, dtype=np.float64)[None, :, None]
    state = f64_ref.initial_cells(p)[0, 0][None, None, :] * (1.0 + 0.05 * np.sin(0.37 * x + 0.11 * y) + 0.01 * np.arange(9)[None, None, :])
    with f64.Grid64(p, obst, flags=f64.FLAG_MULTI_STEPS) as g:
        desc = g.describe()
        assert desc["kernel"] in (_kernel_name(4, nt=True), _kernel_name(4)) and desc["blocks"] == (1024 // TX) * (1024 // TY) == 2048, desc
        g.set_cells(state)
        av = g.run(11)
        assert g.last_run_kernel_ms()[1] == 3
        cells = g.get_cells()
    ref_cells, _, exact = f64_ref.run(p, obst, 11, cells0=state, nthreads=16)
    assert np.array_equal(_bits(cells), _bits(ref_cells)), desc
    assert ref_cells.min() > 0.0
    _check_av_multi(av, exact, obst, 4, desc["blocks"])


def test_bit_parity_8192x7296_planes_beyond_4_gib_with_the_flag(lbm, f64, monkeypatch):
    """tests/test_f64.py's grid beyond 4 GiB under the multi-step kernel, the flag alone and no knob set: the same state, K + 1 steps (a
    full launch and a tail), the same comparison by row blocks.  A 32-bit byte offset in the kernel's pulls, its frame or its stores
    shows in the ninth plane.  116 736 tiles: the bound of the tree is 482 x 2^-53 = 5.4e-14 (the fold kernel's lanes add 456 sums each),
    so the 64 x 2^-53 cap of the small grids does not apply; a miscounted cell would be 1 / cells = 1.7e-8.
    Needs about 13 GB of host memory and is host-bound: with tests/test_f64.py's test of this grid one of the two above a few seconds.
    Measured side by side in one session on an MI355X (profiles/r12/pytest_gpu.log): 3.7 s for this test's 5 steps, 2.9 s for that
    one's 2; less than twice, so the step count stays K + 1."""
    _no_knobs(monkeypatch)
    nx, ny = 8192, 7296
    p, obst, cells = big_grid_case(lbm, max(BUILT_K) + 1)
    with f64.Grid64(p, obst, flags=f64.FLAG_MULTI_STEPS) as g:
        desc = g.describe()
        assert desc["kernel"].startswith("lbm_multi_kernel_f64<") and desc["state_bytes"] == 2 * 9 * nx * ny * 8, desc
        K = int(desc["kernel"][len("lbm_multi_kernel_f64<")])
        assert K in BUILT_K and desc["blocks"] == (nx // TX) * (ny // TY) == 116736
        g.set_cells(cells)
        av = g.run(K + 1)
        assert g.last_run_kernel_ms()[1] == 2
        got = g.get_cells()
    exact = big_grid_compare(p, obst, cells, got, K + 1)
    err, bound = _av_err(av, exact, obst), multi_sum_bound(desc["blocks"])
    print(f"  av_vels {desc['kernel']} on {desc['blocks']} tiles: {err / U:.2f} x 2^-53 against a bound of {bound / U:.0f} x 2^-53")
    assert bound < 0.01 / (nx * ny)          # far below one miscounted cell
    assert err <= bound


# ---- the whole 128 x 128 deck ----------------------------------------------------------------------------------------------------

def test_whole_128x128_deck_with_the_flag(lbm, f64, monkeypatch):
    """40 000 steps with the library's default K, only the minimum size lowered: populations bit for bit, av_vels within the bound of
    the tree, and both within the CPU test's limits of what the reference shipped."""
    for k in ("LBM_TUNE_TILE64_MAX", "LBM_TUNE_TILE64_GEOM", "LBM_TUNE_MULTI64_K"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("LBM_TUNE_MULTI64_MIN", "0")
    p, obst, ref_cells, serial, exact = f64_ref.deck_run("128x128")
    p64 = f64.read_params64(os.path.join(f64_ref.GOLDEN, "decks", "input_128x128.params"))
    with f64.Grid64(p64, obst, flags=f64.FLAG_MULTI_STEPS) as g:
        desc = g.describe()
        assert desc["kernel"].startswith("lbm_multi_kernel_f64<"), desc
        K = int(desc["kernel"][len("lbm_multi_kernel_f64<"):-1])
        av = g.run(p64.max_iters)
        ms, launches = g.last_run_kernel_ms()
        cells, obs, re = g.get_cells(), g.get_observables(), g.reynolds()
    assert K in BUILT_K and launches == -(-p64.max_iters // K) and desc["blocks"] == (128 // TX) * (128 // TY)
    print(f"  128x128, {p64.max_iters} steps with {desc['kernel']}: {ms:.1f} ms in {launches} launches")
    assert np.array_equal(_bits(cells), _bits(ref_cells)), "populations after 40 000 steps"
    _check_av_multi(av, exact, obst, K, desc["blocks"])
    golden_av = f64_ref.golden_av_vels("128x128")
    av_rel = float(np.max(np.abs(av - golden_av) / np.abs(golden_av)))
    values = obs.copy()
    values[obst != 0] = (0.0, 0.0, 0.0, p.density * (1.0 / 3.0))
    fs_abs = float(np.max(np.abs(values.reshape(-1, 4) - f64_ref.golden_final_state("128x128"))))
    pub = float(f64_ref.published()["reynolds"]["128x128"]["value"])
    print(f"  against the shipped results: av_vels {av_rel:.3e} rel, final_state {fs_abs:.3e} abs, Reynolds {re!r}")
    assert av_rel <= f64_ref.AV_VELS_LIMIT + multi_sum_bound(desc["blocks"])
    assert fs_abs <= f64_ref.FINAL_STATE_LIMIT
    assert abs(re - pub) / pub <= f64_ref.REYNOLDS_LIMIT


def test_cli_double_precision_with_the_flag(lbm, f64, tmp_path):
    """LBM_PRECISION=double LBM_FLAGS=1024 bin/d2q9-bgk on the 128 x 128 deck (the minimum size lowered to take it): final_state.dat
    byte-identical to the restatement's."""
    p, obst, ref_cells, serial, exact = f64_ref.deck_run("128x128")
    decks = os.path.join(f64_ref.GOLDEN, "decks")
    cmd = [lbm.CLI_PATH, os.path.join(decks, "input_128x128.params"), os.path.join(decks, "obstacles_128x128.dat")]
    env = {k: v for k, v in os.environ.items() if not k.startswith("LBM_")}
    env.update(LBM_PRECISION="double", LBM_FLAGS="1024", LBM_DESCRIBE="1", LBM_TUNE_MULTI64_MIN="0")      # K: the library's default
    r = subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    ran = [line for line in r.stderr.splitlines() if line.startswith("kernel: ")]
    assert len(ran) == 1 and ran[0].startswith("kernel: lbm_multi_kernel_f64<"), r.stderr                  # the new kernel ran, not the fallback
    K = int(ran[0][len("kernel: lbm_multi_kernel_f64<"):ran[0].index(">")])
    assert K in BUILT_K and ran[0] == f"kernel: lbm_multi_kernel_f64<{K}>, {-(-p.max_iters // K)} launches", r.stderr
    lines = r.stdout.splitlines()
    assert lines[0] == "==done==" and lines[1].split("\t")[-1] == "%.12E" % f64_ref.reynolds(p, ref_cells, obst)
    assert (tmp_path / "final_state.dat").read_text() == f64_ref.final_state_text(p, ref_cells, obst)
    av_lines = (tmp_path / "av_vels.dat").read_text().splitlines()
    assert len(av_lines) == p.max_iters and av_lines[0].startswith("0:\t") and av_lines[-1].startswith(f"{p.max_iters - 1}:\t")
