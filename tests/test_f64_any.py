"""LBM64_FLAG_MULTI_ANY_SIZE on the GPU: the edge-tile form of lbm_multi_kernel_f64 (csrc/kernels/multi64.h, EDGE), several steps per
launch on grids that 32 x 16 tiles do not cover exactly: a tile that would hang over the grid's edge is shifted back inside it and owns
only the strip its neighbour does not.  Held to the CPU restatement tests/f64_ref.c with tests/test_f64_multi.py's recipe: populations
bit for bit, av_vels within the bound of the tree over ceil(nx / 32) * ceil(ny / 16) tiles; every run length and both store forms;
flag on against flag off by row digests on large grids; the same tree on exactly tiled grids; the fallbacks; the read-outs; the CLI."""
import os
import subprocess

import numpy as np
import pytest

import f64_ref
from test_f64 import U, _bits, _random_state
from test_f64 import sum_bound as step_sum_bound
from test_f64_multi import BUILT_K, TX, TY, _av_err, _case, _check_av_multi, _run_reference, multi_sum_bound

pytestmark = pytest.mark.gpu


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


def _tiles(nx, ny):
    return -(-nx // TX) * -(-ny // TY)


def _ragged(lbm, nx, ny, seed=None):
    """A random map (20 % blocked) with blocked cells on row ny-2 and in the strips that two tiles cover: the columns from nx - 32 to
    the last multiple of 32, the rows from ny - 16 to the last multiple of 16."""
    p = lbm.Params(nx=nx, ny=ny, max_iters=10, reynolds_dim=10, density=0.1, accel=0.005, omega=1.85)
    obst = lbm.synthetic_obstacles(nx, ny, p=0.2, seed=nx + ny if seed is None else seed, walls=False)
    obst[ny - 2, 1::5] = 1
    x_lo, x_hi = max(nx - TX, 0), (nx - 1) // TX * TX
    y_lo, y_hi = max(ny - TY, 0), (ny - 1) // TY * TY
    obst[2::3, x_lo:x_hi:4] = 1
    obst[y_lo:y_hi:2, 3::7] = 1
    obst[ny // 2, :3] = 0                              # free cells, some of them on row ny-2
    obst[ny - 2, 0::5] = 0
    assert obst[ny - 2].any() and not obst[ny - 2].all() and (x_hi == x_lo or obst[:, x_lo:x_hi].any()) and (y_hi == y_lo or obst[y_lo:y_hi].any())
    return p, obst


def _kernel_name(K, nt=False):
    return f"lbm_multi_kernel_f64<{K},nt,edge>" if nt else f"lbm_multi_kernel_f64<{K},edge>"


def _parity_any(f64, ref, K, flags=None, nt=False):
    """tests/test_f64_multi.py's _parity_multi under the new flag: 37 steps from rest, then run(5) + run(7) from a random positive state
    against 12 steps."""
    p, obst, (ref37, _, exact37), state, (ref12, _, exact12) = ref
    tiles = _tiles(p.nx, p.ny)
    with f64.Grid64(p, obst, flags=f64.FLAG_MULTI_ANY_SIZE if flags is None else flags) as g:
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


SHAPES = [(34, 16), (32, 17), (34, 18), (62, 31), (66, 35), (96, 50), (258, 34)]


@pytest.mark.parametrize("K", BUILT_K)
@pytest.mark.parametrize("nx,ny", SHAPES)
def test_bit_parity_shapes(lbm, f64, monkeypatch, nx, ny, K):
    """34 x 16: two tile columns overlapping by 30, the last owns 2 columns; the frame wraps onto itself in y.  32 x 17: the second tile
    row owns one row; row ny-2 = 15 lies in both tiles and is owned by the first.  34 x 18: row ny-2 = 16 is inside the owned sliver of
    the shifted tile.  62 x 31 and 66 x 35: 2 x 2 and 3 x 3 tiles, ragged both ways, an interior tile in the latter.  96 x 50: ragged in
    y only.  258 x 34: nine tile columns."""
    p, obst = _ragged(lbm, nx, ny)
    _force(monkeypatch, K)
    _parity_any(f64, _case(("any", nx, ny), p, obst), K)


@pytest.mark.parametrize("K", BUILT_K)
@pytest.mark.parametrize("flag,nt", [("FLAG_NT_STORES", True), ("FLAG_NO_NT_STORES", False)])
@pytest.mark.parametrize("nx,ny", [(34, 18), (66, 35)])
def test_every_run_length_and_both_store_forms(lbm, f64, monkeypatch, nx, ny, flag, nt, K):
    """run(n) for n = 1 .. 2K + 1: every tail length, n < K (one launch that is not FULL; n = 1 stores straight from sub-step 1), full
    launches alone.  Each from a fresh random state.  Then two runs back to back: run(K + 1) + run(K) against 2K + 1 steps."""
    p, obst = _ragged(lbm, nx, ny)
    key = ("any", nx, ny)
    _case(key, p, obst)
    tiles = _tiles(nx, ny)
    _force(monkeypatch, K)
    with f64.Grid64(p, obst, flags=f64.FLAG_MULTI_ANY_SIZE | getattr(f64, flag)) as g:
        assert g.describe()["kernel"] == _kernel_name(K, nt)
        for n in range(1, 2 * K + 2):
            state, ref_cells, exact = _run_reference(key, 100 + n, n)
            g.set_cells(state)
            av = g.run(n)
            assert g.last_run_kernel_ms()[1] == -(-n // K)
            assert np.array_equal(_bits(g.get_cells()), _bits(ref_cells)), f"run({n}) under K = {K}"
            assert ref_cells.min() > 0.0
            _check_av_multi(av, exact, obst, K, tiles)
        n = 2 * K + 1
        state, ref_cells, exact = _run_reference(key, 100 + n, n)
        g.set_cells(state)
        av = np.concatenate([g.run(K + 1), g.run(K)])
        assert np.array_equal(_bits(g.get_cells()), _bits(ref_cells)), f"run({K + 1}) + run({K}) under K = {K}"
        _check_av_multi(av, exact, obst, K, tiles)


def test_with_the_other_step_flags(lbm, f64, monkeypatch):
    """4096 with 512 and with 1024: the edge form where the tiled kernel does not take the grid."""
    p, obst = _ragged(lbm, 66, 35)
    _force(monkeypatch, 3)
    ref = _case(("any", 66, 35), p, obst)
    _parity_any(f64, ref, 3, flags=f64.FLAG_MULTI_ANY_SIZE | f64.FLAG_TILE_STEPS)
    _parity_any(f64, ref, 3, flags=f64.FLAG_MULTI_ANY_SIZE | f64.FLAG_MULTI_STEPS)


def _smooth_state(p):
    """A positive state that differs from cell to cell, made without a random draw per value (the large grids)."""
    y, x = np.arange(p.ny, dtype=np.float64)[:, None, None], np.arange(p.nx, dtype=np.float64)[None, :, None]
    return f64_ref.initial_cells(p)[0, 0][None, None, :] * (1.0 + 0.05 * np.sin(0.37 * x + 0.11 * y) + 0.01 * np.arange(9)[None, None, :])


def _on_against_off_by_digests(lbm, f64, nx, ny, steps, K):
    p, obst = _ragged(lbm, nx, ny)
    state = _smooth_state(p)
    out = {}
    for flags in (0, f64.FLAG_MULTI_ANY_SIZE):
        with f64.Grid64(p, obst, flags=flags) as g:
            g.set_cells(state)
            av = g.run(steps)
            out[flags] = (g.describe(), av, g.digest(), g.last_run_kernel_ms()[1])
    (d_off, av_off, (rows_off, sum_off), n_off), (d_on, av_on, (rows_on, sum_on), n_on) = out[0], out[f64.FLAG_MULTI_ANY_SIZE]
    assert d_off["kernel"].startswith("lbm_step_kernel_f64<2") and n_off == steps
    assert d_on["kernel"] in (_kernel_name(K), _kernel_name(K, nt=True)) and d_on["blocks"] == _tiles(nx, ny) and n_on == -(-steps // K), d_on
    differ = np.nonzero(rows_on != rows_off)[0]
    assert differ.size == 0 and sum_on == sum_off, f"{nx}x{ny}: rows that differ after {steps} steps: {differ[:16]}"
    assert np.all(av_off > 0.0)
    bound = step_sum_bound(d_off) + multi_sum_bound(d_on["blocks"])
    err = float(np.max(np.abs(av_on - av_off) / av_off))
    print(f"  {nx}x{ny} av_vels on against off: {err / U:.2f} x 2^-53 against a bound of {bound / U:.0f} x 2^-53")
    assert bound < 0.01 / (nx * ny) and err <= bound          # far below one miscounted cell


@pytest.mark.parametrize("K", BUILT_K)
def test_flag_on_against_flag_off_1000x600(lbm, f64, monkeypatch, K):
    """32 x 38 tiles, the last column owning 8 columns and the last row 8 rows; 2K + 1 steps: two full launches and a 1-step tail.  The
    state never comes back to the host: one 64-bit digest per row does (lbm_digest64_grid)."""
    _force(monkeypatch, K)
    _on_against_off_by_digests(lbm, f64, 1000, 600, 2 * K + 1, K)


def test_flag_on_against_flag_off_4098x2050(lbm, f64, monkeypatch):
    """129 x 129 tiles whose last column and row own two cells' width: wide planes, many tiles, the library's own K and minimum size."""
    for k in [k for k in os.environ if k.startswith("LBM_TUNE_")]:
        monkeypatch.delenv(k)
    _on_against_off_by_digests(lbm, f64, 4098, 2050, 5, 4)


def test_the_same_tree_on_exactly_tiled_grids(f64, digests, monkeypatch):
    """64 x 48: under 4096 the kernel, the name and every bit of av_vels are those of 1024."""
    from test_f64 import _deck
    p, obst = _deck(f64, digests, "rand_64x48")
    _force(monkeypatch, 3)
    state = _random_state(p, seed=21)
    out = {}
    for flags in (f64.FLAG_MULTI_STEPS, f64.FLAG_MULTI_ANY_SIZE, f64.FLAG_MULTI_ANY_SIZE | f64.FLAG_MULTI_STEPS):
        with f64.Grid64(p, obst, flags=flags) as g:
            g.set_cells(state)
            out[flags] = (g.describe(), np.concatenate([g.run(11), g.run(6)]), g.get_cells())
    d_1024, av_1024, cells_1024 = out[f64.FLAG_MULTI_STEPS]
    assert d_1024["kernel"] == "lbm_multi_kernel_f64<3>"
    for flags in (f64.FLAG_MULTI_ANY_SIZE, f64.FLAG_MULTI_ANY_SIZE | f64.FLAG_MULTI_STEPS):
        d, av, cells = out[flags]
        assert d == d_1024
        assert np.array_equal(_bits(av), _bits(av_1024)) and np.array_equal(_bits(cells), _bits(cells_1024))


@pytest.mark.parametrize("nx,ny", [(33, 16), (32, 15)])
def test_fallbacks_with_the_flag(lbm, f64, monkeypatch, nx, ny):
    """Odd nx and ny < 16 run lbm_step_kernel_f64 exactly as without the flag: the name, the launch, every bit."""
    _force(monkeypatch, 3)
    p, obst = _ragged(lbm, nx, ny)
    state = _random_state(p, seed=5)
    out = {}
    for flags in (0, f64.FLAG_MULTI_ANY_SIZE):
        with f64.Grid64(p, obst, flags=flags) as g:
            g.set_cells(state)
            out[flags] = (g.describe(), np.concatenate([g.run(5), g.run(7)]), g.get_cells(), g.last_run_kernel_ms()[1])
    off, on = out[0], out[f64.FLAG_MULTI_ANY_SIZE]
    assert on[0] == off[0] and on[0]["kernel"] == f"lbm_step_kernel_f64<{2 if nx % 2 == 0 else 1}>" and on[3] == off[3] == 7
    assert np.array_equal(_bits(on[1]), _bits(off[1])) and np.array_equal(_bits(on[2]), _bits(off[2]))
    ref_cells, _, _ = f64_ref.run(p, obst, 12, cells0=state)
    assert np.array_equal(_bits(on[2]), _bits(ref_cells))


def test_read_outs_after_an_edge_form_run(lbm, f64, monkeypatch):
    p, obst = _ragged(lbm, 66, 35)
    _force(monkeypatch, 3)
    state = _random_state(p, seed=9)
    with f64.Grid64(p, obst, flags=f64.FLAG_MULTI_ANY_SIZE) as g:
        assert g.describe()["kernel"] == _kernel_name(3)
        g.set_cells(state)
        g.run(19)
        cells, obs, tot, re = g.get_cells(), g.get_observables(), g.av_velocity_sum(), g.reynolds()
        rows, total = g.digest()
    ref_cells, _, _ = f64_ref.run(p, obst, 19, cells0=state)
    assert np.array_equal(_bits(cells), _bits(ref_cells))
    assert np.array_equal(_bits(obs), _bits(f64_ref.observables(ref_cells)))
    assert re == f64_ref.reynolds(p, ref_cells, obst)
    host_rows, host_total = f64.digest_host(ref_cells, p.nx)
    assert np.array_equal(rows, host_rows) and total == host_total
    n = p.nx * p.ny
    blocks = min(-(-n // 256), 1024)
    exact = f64_ref.velocity_sum_exact(ref_cells, obst)
    assert abs(tot - exact) <= (-(-n // (blocks * 256)) + 9 + blocks) * U * exact       # tests/test_f64.py: lbm64_av_velocity_sum's own tree


def test_cli_double_precision_with_the_flag(lbm, f64, tmp_path):
    """LBM_PRECISION=double bin/d2q9-bgk on a ragged 66 x 35 deck made here: final_state.dat under LBM_FLAGS=4096 is byte for byte that
    of LBM_FLAGS=0, and the LBM_DESCRIBE=1 line names the edge form."""
    from mpilattice_boltzmann_amd import decks
    p, obst = _ragged(lbm, 66, 35)
    steps = 23
    (tmp_path / "input.params").write_text(f"{p.nx}\n{p.ny}\n{steps}\n{p.reynolds_dim}\n{p.density}\n{p.accel}\n{p.omega}\n")
    decks.write_obstacles(str(tmp_path / "obstacles.dat"), obst)
    base = {k: v for k, v in os.environ.items() if not k.startswith("LBM_")}
    out = {}
    for flags in ("0", "4096"):
        cwd = tmp_path / flags
        cwd.mkdir()
        env = dict(base, LBM_PRECISION="double", LBM_FLAGS=flags, LBM_DESCRIBE="1", LBM_TUNE_MULTI64_MIN="0")      # K: the library's default
        r = subprocess.run([lbm.CLI_PATH, str(tmp_path / "input.params"), str(tmp_path / "obstacles.dat")], cwd=cwd, env=env,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        ran = [line for line in r.stderr.splitlines() if line.startswith("kernel: ")]
        assert len(ran) == 1, r.stderr
        out[flags] = (ran[0], (cwd / "final_state.dat").read_bytes(), (cwd / "av_vels.dat").read_text().splitlines(), r.stdout.splitlines())
    assert out["0"][0] == f"kernel: lbm_step_kernel_f64<2>, {steps} launches"
    K = int(out["4096"][0][len("kernel: lbm_multi_kernel_f64<")])
    assert K in BUILT_K and out["4096"][0] == f"kernel: {_kernel_name(K)}, {-(-steps // K)} launches", out["4096"][0]
    assert out["4096"][1] == out["0"][1] and len(out["0"][1]) > 0
    ref_cells, _, _ = f64_ref.run(p, obst, steps)
    assert out["4096"][1].decode() == f64_ref.final_state_text(p, ref_cells, obst)
    assert len(out["4096"][2]) == steps and out["4096"][3][0] == "==done==" and out["4096"][3][1] == out["0"][3][1]      # the Reynolds number line
