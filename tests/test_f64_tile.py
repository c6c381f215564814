"""LBM64_FLAG_TILE_STEPS on the GPU: lbm_tile_kernel_f64<T, H> (csrc/kernels/tile64.h), several steps per launch of the double-precision
mode, held to the CPU restatement tests/f64_ref.c with tests/test_f64.py's recipe: populations bit for bit in every geometry, on grids
smaller than a region, for every length of the last launch of a run; av_vels within the bound of the tiled launch's summation tree;
the fallbacks; the read-outs; the whole 128 x 128 deck against the results the reference shipped, and through the CLI."""
import functools
import os
import subprocess

import numpy as np
import pytest

import f64_ref
from test_f64 import U, _bits, _deck, _random_state, _synthetic
from test_f64 import sum_bound as step_sum_bound

pytestmark = pytest.mark.gpu

GEOMS = [(8, 4), (8, 8), (16, 4), (16, 8)]          # every geometry kept (profiles/r08/f64_tile.txt: <8,4> and <16,8> are the defaults by size)
TILE_MAX = str(1 << 20)                             # the tests choose the kernel by shape, not by the size cap


@pytest.fixture(scope="module")
def f64(lbm):
    from mpilattice_boltzmann_amd import f64 as mod
    mod.load_library()
    return mod


def _force(monkeypatch, T, H):
    """A context reads the knobs when it is made."""
    monkeypatch.setenv("LBM_TUNE_TILE64_GEOM", str(T * 10 + H))
    monkeypatch.setenv("LBM_TUNE_TILE64_MAX", TILE_MAX)


def tile_block(T, H):
    return 256 if (T, H) == (8, 4) else 512          # lanes of a block (lbm_geometry.h tile64_block)


def tile_sum_bound(T, H, tiles):
    """Relative error of one av_vels entry of a tiled run against the exactly rounded sum times 1.0 / free_cells: (the longest chain of
    additions a term passes through + 2) * 2^-53, from the tree include/lbm_d2q9_f64.h states.  Every term is non-negative and the same
    double on both sides, so each addition errs by at most 2^-53 of its result, which is at most the total.
      in the tile's block (B lanes)   1 or 2   a lane adds the owned cells it meets in that sub-step: one per pass, and a sub-step takes two
                                               passes where its region, at most (T + 2 (H - 1))^2 cells, has more than B of them
                                      6        butterfly levels over the 64 lanes of a wave
                                      B/64 - 1 one lane adds the waves' sums serially
      in the fold (F lanes)           ceil(tiles / F) + 6 + F/64 - 1; F = B in block 0 of the next launch, 256 in the last fold of a run:
                                      the larger of the two
      2                               the product with 1.0 / free_cells, on this side and on the reference's."""
    B = tile_block(T, H)
    passes = 2 if (T + 2 * (H - 1)) ** 2 > B else 1
    in_tile = passes + 6 + B // 64 - 1
    fold = max(-(-tiles // F) + 6 + F // 64 - 1 for F in (B, 256))
    return (in_tile + fold + 2) * U


def _av_err(av, exact, obst):
    ref = f64_ref.av_vels(exact, obst)
    assert av.shape == ref.shape
    # (a deck whose accelerated row is blocked stays at rest: every entry is 0 on both sides, and the error is taken absolutely)
    return float(np.max(np.abs(av - ref) / ref)) if np.all(ref > 0) else float(np.max(np.abs(av - ref)))


def _check_av_tiled(av, exact, obst, T, H, tiles):
    err, bound = _av_err(av, exact, obst), tile_sum_bound(T, H, tiles)
    print(f"  av_vels <{T},{H}> on {tiles} tiles: {err / U:.2f} x 2^-53 against a bound of {bound / U:.0f} x 2^-53")
    assert bound <= 64 * U           # a loose bound would hide a miscounted ghost cell (an error of about 1 / cells >> 1e-14)
    assert err <= bound


# ---- references, each computed once and never written to --------------------------------------------------------------------

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


_CASES = {}


def _case(key, p, obst):
    _CASES.setdefault(key, (p, obst))
    return _reference(key)


def _parity_tiled(f64, ref, T, H, flags=None):
    """tests/test_f64.py's _parity with the flag: 37 steps from rest (at H = 8 four full launches and a 5-step tail), then run(5) +
    run(7) from a random positive state against 12 steps."""
    p, obst, (ref37, _, exact37), state, (ref12, _, exact12) = ref
    tiles = (p.nx // T) * (p.ny // T)
    with f64.Grid64(p, obst, flags=f64.FLAG_TILE_STEPS if flags is None else flags) as g:
        desc = g.describe()
        assert desc["kernel"] == f"lbm_tile_kernel_f64<{T}, {H}>" and desc["blocks"] == tiles and desc["cells_per_block"] == T * T, desc
        av = g.run(37)
        assert g.last_run_kernel_ms()[1] == -(-37 // H)
        assert np.array_equal(_bits(g.get_cells()), _bits(ref37)), f"{p.nx}x{p.ny} 37 steps from rest: {desc}"
        _check_av_tiled(av, exact37, obst, T, H, tiles)
        g.set_cells(state)
        av = np.concatenate([g.run(5), g.run(7)])
        assert np.array_equal(_bits(g.get_cells()), _bits(ref12)), f"{p.nx}x{p.ny} run(5) + run(7) from a random state: {desc}"
        assert ref12.min() > 0.0                         # the premise of the bound: positive densities, non-negative terms
        _check_av_tiled(av, exact12, obst, T, H, tiles)
    return desc


DECKS = ["accelrow_blocked_32x16", "strongaccel_32x16", "dense_32x32", "rand_64x48", "walls_40x24", "wide_256x8", "tall_8x256"]
DECK_T16 = {"accelrow_blocked_32x16", "strongaccel_32x16", "dense_32x32", "rand_64x48"}       # edges that 16 divides
DECK_CASES = [(name, T, H) for name in DECKS for (T, H) in GEOMS if T == 8 or name in DECK_T16]


@pytest.mark.parametrize("name,T,H", DECK_CASES)
def test_bit_parity_decks_every_geometry(f64, digests, monkeypatch, name, T, H):
    """wide_256x8 and tall_8x256: one tile tall / wide, and a region (16 or 24 cells) that wraps the 8-cell edge two or three times."""
    p, obst = _deck(f64, digests, name)
    assert p.nx % T == 0 and p.ny % T == 0
    _force(monkeypatch, T, H)
    _parity_tiled(f64, _case(name, p, obst), T, H)


SMALL = [(8, 8, 8), (16, 8, 8), (8, 16, 8), (16, 16, 16), (16, 16, 8), (24, 40, 8), (48, 32, 16)]      # nx, ny, T


@pytest.mark.parametrize("nx,ny,T,H", [(nx, ny, T, H) for (nx, ny, T) in SMALL for H in (4, 8)])
def test_bit_parity_smallest_grids(lbm, f64, monkeypatch, nx, ny, T, H):
    """8 x 8 under <8,8>: one tile whose 24 x 24 region holds the grid three times each way; 24 x 40: 3 x 5 tiles."""
    p, obst = _synthetic(lbm, nx, ny, seed=nx + ny)
    _force(monkeypatch, T, H)
    _parity_tiled(f64, _case((nx, ny), p, obst), T, H)


@functools.lru_cache(maxsize=None)
def _tail_reference(name, seed, steps):
    p, obst = _CASES[name]
    state = _random_state(p, seed=seed)
    cells, _, exact = f64_ref.run(p, obst, steps, cells0=state)
    for a in (state, cells, exact):
        a.setflags(write=False)
    return state, cells, exact


@pytest.mark.parametrize("T,H", GEOMS)
def test_every_tail(f64, digests, monkeypatch, T, H):
    """run(k) for k = 1 .. H, each from a fresh random state: every length of a launch that is not FULL, each after the accelerate
    pre-pass and with no accelerate after its last sub-step.  Then run(H) + run(1) + run(H + 1) against 2H + 2 steps."""
    name = "strongaccel_32x16"
    p, obst = _deck(f64, digests, name)
    _case(name, p, obst)
    tiles = (p.nx // T) * (p.ny // T)
    _force(monkeypatch, T, H)
    with f64.Grid64(p, obst, flags=f64.FLAG_TILE_STEPS) as g:
        assert g.describe()["kernel"] == f"lbm_tile_kernel_f64<{T}, {H}>"
        for k in range(1, H + 1):
            state, ref_cells, exact = _tail_reference(name, 100 + k, k)
            g.set_cells(state)
            av = g.run(k)
            assert g.last_run_kernel_ms()[1] == 1
            assert np.array_equal(_bits(g.get_cells()), _bits(ref_cells)), f"run({k}) under <{T},{H}>"
            assert ref_cells.min() > 0.0
            _check_av_tiled(av, exact, obst, T, H, tiles)
        state, ref_cells, exact = _tail_reference(name, 99, 2 * H + 2)
        g.set_cells(state)
        av = np.concatenate([g.run(H), g.run(1), g.run(H + 1)])
        assert g.last_run_kernel_ms()[1] == 2
        assert np.array_equal(_bits(g.get_cells()), _bits(ref_cells)), f"run({H}) + run(1) + run({H + 1}) under <{T},{H}>"
        assert ref_cells.min() > 0.0
        _check_av_tiled(av, exact, obst, T, H, tiles)


@pytest.mark.parametrize("T,H", GEOMS)
def test_flag_on_against_flag_off(f64, digests, monkeypatch, T, H):
    p, obst = _deck(f64, digests, "rand_64x48")
    _force(monkeypatch, T, H)
    state = _random_state(p, seed=21)
    out = {}
    for flags in (0, f64.FLAG_TILE_STEPS):
        with f64.Grid64(p, obst, flags=flags) as g:
            g.set_cells(state)
            out[flags] = (g.describe(), np.concatenate([g.run(11), g.run(2 * H)]), g.get_cells())
    (d_off, av_off, cells_off), (d_on, av_on, cells_on) = out[0], out[f64.FLAG_TILE_STEPS]
    assert d_off["kernel"] == "lbm_step_kernel_f64<2>" and d_on["kernel"] == f"lbm_tile_kernel_f64<{T}, {H}>"
    assert np.array_equal(_bits(cells_on), _bits(cells_off))
    assert cells_off.min() > 0.0
    bound = step_sum_bound(d_off) + tile_sum_bound(T, H, d_on["blocks"])
    assert float(np.max(np.abs(av_on - av_off) / av_off)) <= bound


@pytest.mark.parametrize("shape", ["tiny_8x3", (7, 5), (258, 33)])
def test_fallbacks_with_the_flag(lbm, f64, digests, monkeypatch, shape):
    """Grids the tiled kernel does not take run lbm_step_kernel_f64 exactly as without the flag."""
    monkeypatch.setenv("LBM_TUNE_TILE64_MAX", TILE_MAX)
    p, obst = _deck(f64, digests, shape) if isinstance(shape, str) else _synthetic(lbm, *shape)
    p, obst, (ref37, _, exact37), state, (ref12, _, exact12) = _case(shape, p, obst)
    with f64.Grid64(p, obst, flags=f64.FLAG_TILE_STEPS) as g:
        desc = g.describe()
        assert desc["kernel"] == f"lbm_step_kernel_f64<{2 if p.nx % 2 == 0 else 1}>" and desc["blocks"] == -(-(p.nx * p.ny // (2 - p.nx % 2)) // 256), desc
        av = g.run(37)
        assert g.last_run_kernel_ms()[1] == 37
        assert np.array_equal(_bits(g.get_cells()), _bits(ref37))
        assert _av_err(av, exact37, obst) <= step_sum_bound(desc)
        g.set_cells(state)
        av = np.concatenate([g.run(5), g.run(7)])
        assert np.array_equal(_bits(g.get_cells()), _bits(ref12))
        assert ref12.min() > 0.0 and _av_err(av, exact12, obst) <= step_sum_bound(desc)


def test_a_grid_above_the_cap_falls_back(f64, digests, monkeypatch):
    p, obst = _deck(f64, digests, "rand_64x48")
    monkeypatch.setenv("LBM_TUNE_TILE64_MAX", str(64 * 48 - 1))
    with f64.Grid64(p, obst, flags=f64.FLAG_TILE_STEPS) as g:
        assert g.describe()["kernel"] == "lbm_step_kernel_f64<2>"
    monkeypatch.setenv("LBM_TUNE_TILE64_MAX", str(64 * 48))
    with f64.Grid64(p, obst, flags=f64.FLAG_TILE_STEPS | f64.FLAG_NT_STORES) as g:
        assert g.describe()["kernel"].startswith("lbm_tile_kernel_f64<")


def test_read_outs_after_a_tiled_run(f64, digests, monkeypatch):
    p, obst = _deck(f64, digests, "rand_64x48")
    monkeypatch.setenv("LBM_TUNE_TILE64_MAX", TILE_MAX)
    with f64.Grid64(p, obst, flags=f64.FLAG_TILE_STEPS) as g:
        assert g.describe()["kernel"].startswith("lbm_tile_kernel_f64<")
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


# ---- the whole 128 x 128 deck ----------------------------------------------------------------------------------------------------

def test_whole_128x128_deck_with_the_flag(lbm, f64, monkeypatch):
    """40 000 steps in the geometry the library picks for the deck, no knob set: populations bit for bit, av_vels within the tiled
    bound, and both within the CPU test's limits of what the reference shipped."""
    for k in ("LBM_TUNE_TILE64_MAX", "LBM_TUNE_TILE64_GEOM"):
        monkeypatch.delenv(k, raising=False)
    p, obst, ref_cells, serial, exact = f64_ref.deck_run("128x128")
    p64 = f64.read_params64(os.path.join(f64_ref.GOLDEN, "decks", "input_128x128.params"))
    with f64.Grid64(p64, obst, flags=f64.FLAG_TILE_STEPS) as g:
        desc = g.describe()
        assert desc["kernel"].startswith("lbm_tile_kernel_f64<"), desc
        T, H = (int(v) for v in desc["kernel"][len("lbm_tile_kernel_f64<"):-1].split(","))
        av = g.run(p64.max_iters)
        ms, launches = g.last_run_kernel_ms()
        cells, obs, re = g.get_cells(), g.get_observables(), g.reynolds()
    assert launches == -(-p64.max_iters // H) and desc["blocks"] == (128 // T) ** 2
    print(f"  128x128, {p64.max_iters} steps with {desc['kernel']}: {ms:.1f} ms in {launches} launches")
    assert np.array_equal(_bits(cells), _bits(ref_cells)), "populations after 40 000 steps"
    _check_av_tiled(av, exact, obst, T, H, desc["blocks"])
    golden_av = f64_ref.golden_av_vels("128x128")
    av_rel = float(np.max(np.abs(av - golden_av) / np.abs(golden_av)))
    values = obs.copy()
    values[obst != 0] = (0.0, 0.0, 0.0, p.density * (1.0 / 3.0))
    fs_abs = float(np.max(np.abs(values.reshape(-1, 4) - f64_ref.golden_final_state("128x128"))))
    pub = float(f64_ref.published()["reynolds"]["128x128"]["value"])
    print(f"  against the shipped results: av_vels {av_rel:.3e} rel, final_state {fs_abs:.3e} abs, Reynolds {re!r}")
    assert av_rel <= f64_ref.AV_VELS_LIMIT + tile_sum_bound(T, H, desc["blocks"])
    assert fs_abs <= f64_ref.FINAL_STATE_LIMIT
    assert abs(re - pub) / pub <= f64_ref.REYNOLDS_LIMIT


def test_cli_double_precision_with_the_flag(lbm, f64, tmp_path):
    """LBM_PRECISION=double LBM_FLAGS=512 bin/d2q9-bgk on the 128 x 128 deck: final_state.dat byte-identical to the restatement's."""
    p, obst, ref_cells, serial, exact = f64_ref.deck_run("128x128")
    decks = os.path.join(f64_ref.GOLDEN, "decks")
    cmd = [lbm.CLI_PATH, os.path.join(decks, "input_128x128.params"), os.path.join(decks, "obstacles_128x128.dat")]
    env = {k: v for k, v in os.environ.items() if not k.startswith("LBM_")}
    env.update(LBM_PRECISION="double", LBM_FLAGS="512", LBM_DESCRIBE="1")          # no knob: the command line of the README
    r = subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    ran = [line for line in r.stderr.splitlines() if line.startswith("kernel: ")]
    assert ran == [f"kernel: lbm_tile_kernel_f64<8, 4>, {p.max_iters // 4} launches"], r.stderr      # the tiled kernel ran, not the fallback
    lines = r.stdout.splitlines()
    assert lines[0] == "==done==" and lines[1].split("\t")[-1] == "%.12E" % f64_ref.reynolds(p, ref_cells, obst)
    assert (tmp_path / "final_state.dat").read_text() == f64_ref.final_state_text(p, ref_cells, obst)
    av_lines = (tmp_path / "av_vels.dat").read_text().splitlines()
    assert len(av_lines) == p.max_iters and av_lines[0].startswith("0:\t") and av_lines[-1].startswith(f"{p.max_iters - 1}:\t")
    env["LBM_GPUS"] = "2"
    r = subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "double precision runs on one GPU" in r.stderr
