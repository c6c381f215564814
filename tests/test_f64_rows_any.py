"""LBM_ROWS64_FLAG_MULTI_ANY_SIZE on the GPU: the edge-tile form of lbm_rows_multi_kernel_f64 (csrc/kernels/rows_multi64.h, EDGE; the
host loop in csrc/lbm_rows64.hip), K steps per launch and exchange on ranks that 32 x 16 tiles do not cover exactly, uneven ranks among
them: a tile that would hang over the rank's last column or owned row is shifted back inside and owns only the strip its neighbour
does not.  Held to the CPU restatement tests/f64_ref.c with tests/test_f64_rows_multi.py's recipe: populations bit for bit, av_vels
within the bound of the summation tree; every run length and both store forms; flag on against flag off by row digests on large grids;
the exactly tiled deck, which runs as under LBM_ROWS64_FLAG_MULTI_STEPS; the fallbacks; the read-outs; the CLI.  All ranks run on
device 0; one test switches itself on where there are two GPUs or more.  Every run asserts the kernel's name, so that a fallback to
the one-step kernel cannot pass for the kernel.

THE av_vels BOUND is tests/test_f64_rows_multi.py's with the new tile count: a rank's sum of a step is lbm_multi_kernel_f64's tree over
the rank's ceil(nx / 32) * ceil(nyl / 16) tiles (a shifted tile adds exact zeros for the cells it does not own: no rounding), the rank
with the most tiles has the longest chain of additions, and the host adds the ranks' sums in rank order:
multi_sum_bound(tiles of the largest rank) + (nranks - 1) * 2^-53."""
import os
import subprocess

import numpy as np
import pytest

import f64_ref
from test_f64_any import _ragged, _smooth_state
from test_f64_multi import BUILT_K, _case, _run_reference
from test_f64_rows import U, _bits, _deck, _random_state
from test_f64_rows import sum_bound as rows_step_sum_bound
from test_f64_rows_multi import _check_av, _force, rows_multi_sum_bound

pytestmark = pytest.mark.gpu

TX, TY = 32, 16


@pytest.fixture(scope="module")
def f64(lbm):
    from mpilattice_boltzmann_amd import f64 as mod
    mod.load_rows_library()
    return mod


def _kernel_name(K, nt=False):
    return f"lbm_rows_multi_kernel_f64<{K},nt,edge>" if nt else f"lbm_rows_multi_kernel_f64<{K},edge>"


def _ragged_rows(lbm, nx, ny, nranks, rows=None):
    """tests/test_f64_any.py's _ragged map (20 % blocked; blocked and free cells on row ny-2; blocked cells in the columns from nx - 32
    to the last multiple of 32) with blocked cells in the rows that two tiles of a RANK cover as well: per rank, its owned rows from
    nyl - 16 to the last multiple of 16."""
    p, obst = _ragged(lbm, nx, ny)
    nyls, dis = lbm.decompose(ny, nranks)
    assert rows is None or list(nyls) == rows
    for nyl, y0 in zip(nyls, dis):
        lo, hi = y0 + max(nyl - TY, 0), y0 + (nyl - 1) // TY * TY
        obst[lo:hi:2, 3::7] = 1
        obst[lo:hi:3, 5::11] = 1
        assert hi == lo or obst[lo:hi].any()
    obst[ny - 2, 1::5] = 1
    obst[ny - 2, 0::5] = 0
    obst[ny // 2, :3] = 0
    assert obst[ny - 2].any() and not obst[ny - 2].all()
    return p, obst, list(nyls)


def _tiles(nx, nyls):
    return -(-nx // TX) * max(-(-n // TY) for n in nyls)


def _check_desc(desc, p, nyls, K, nt=False):
    nranks = len(nyls)
    tiles = _tiles(p.nx, nyls)
    assert desc["kernel"] == _kernel_name(K, nt), desc
    assert desc["nranks"] == nranks and desc["blocks"] == tiles and desc["cells_per_block"] == TX * TY, desc
    assert desc["state_bytes"] == 2 * 9 * 8 * p.nx * (p.ny + 2 * K * nranks), desc
    return tiles


def _parity_any(f64, ref, nyls, K, flags=None, nt=False, devices=None):
    """tests/test_f64_rows_multi.py's _parity under the new flag: 37 steps from rest (at K = 4 nine full launches and a one-step tail, the
    direct-store form), then run(5) + run(7) from a random positive state against 12 steps."""
    p, obst, (ref37, _, exact37), state, (ref12, _, exact12) = ref
    nranks = len(nyls)
    with f64.Rows64(p, obst, nranks, devices=devices if devices is not None else [0] * nranks,
                    flags=f64.FLAG_ROWS_MULTI_ANY_SIZE if flags is None else flags) as g:
        desc = g.describe()
        tiles = _check_desc(desc, p, nyls, K, nt)
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

# 34 x 18 on 1: the rank is its own neighbour; two tile columns overlapping by 30; row ny-2 = 16 inside the shifted tile's owned sliver.
# 32 x 33 on 2: ragged in y on one rank only, unequal tile counts, both neighbours the same rank.  34 x 35 on 2: row 33 lies in both
# tiles of rank 1 and is owned by the first.  66 x 50 on 3: three neighbours with different nyl and plane strides, an interior tile
# column.  62 x 31 on 1: 2 x 2 tiles, ragged both ways.  96 x 52 on 3: ragged in y only.  258 x 34 on 2: nine tile columns.
SHAPES = [(34, 18, [18]), (32, 33, [17, 16]), (34, 35, [18, 17]), (66, 50, [17, 17, 16]), (62, 31, [31]), (96, 52, [18, 17, 17]),
          (258, 34, [17, 17])]


def _key(nx, ny, nranks):
    return ("rows any", nx, ny, nranks)


@pytest.mark.parametrize("K", BUILT_K)
@pytest.mark.parametrize("nx,ny,rows", SHAPES)
def test_bit_parity_shapes(lbm, f64, monkeypatch, nx, ny, rows, K):
    p, obst, nyls = _ragged_rows(lbm, nx, ny, len(rows), rows)
    _force(monkeypatch, K)
    _parity_any(f64, _case(_key(nx, ny, len(rows)), p, obst), nyls, K)


@pytest.mark.parametrize("K", BUILT_K)
@pytest.mark.parametrize("flag,nt", [("FLAG_NT_STORES", True), ("FLAG_NO_NT_STORES", False)])
@pytest.mark.parametrize("nx,ny,nranks", [(34, 35, 2), (66, 50, 3)])
def test_every_run_length_and_both_store_forms(lbm, f64, monkeypatch, nx, ny, nranks, flag, nt, K):
    """run(n) for n = 1 .. 2K + 1: every tail length, n < K (one launch that is not FULL; n = 1 stores straight from sub-step 1), full
    launches alone.  Each from a fresh random state.  Then two runs back to back: run(K + 1) + run(K) against 2K + 1 steps."""
    p, obst, nyls = _ragged_rows(lbm, nx, ny, nranks)
    key = _key(nx, ny, nranks)
    _case(key, p, obst)
    _force(monkeypatch, K)
    with f64.Rows64(p, obst, nranks, devices=[0] * nranks, flags=f64.FLAG_ROWS_MULTI_ANY_SIZE | getattr(f64, flag)) as g:
        tiles = _check_desc(g.describe(), p, nyls, K, nt)
        for n in range(1, 2 * K + 2):
            state, ref_cells, exact = _run_reference(key, 100 + n, n)
            g.set_cells(state)
            av = g.run(n)
            assert g.last_run_ms()[1] == -(-n // K) * nranks
            assert np.array_equal(_bits(g.get_cells()), _bits(ref_cells)), f"run({n}) under K = {K}"
            assert ref_cells.min() > 0.0
            _check_av(av, exact, obst, tiles, nranks)
        n = 2 * K + 1
        state, ref_cells, exact = _run_reference(key, 100 + n, n)
        g.set_cells(state)
        av = np.concatenate([g.run(K + 1), g.run(K)])
        assert np.array_equal(_bits(g.get_cells()), _bits(ref_cells)), f"run({K + 1}) + run({K}) under K = {K}"
        _check_av(av, exact, obst, tiles, nranks)


def test_with_the_other_rows_flag(lbm, f64, monkeypatch):
    """8192 with 2048: the edge form, as under 8192 alone."""
    p, obst, nyls = _ragged_rows(lbm, 66, 50, 3)
    _force(monkeypatch, 3)
    _parity_any(f64, _case(_key(66, 50, 3), p, obst), nyls, 3, flags=f64.FLAG_ROWS_MULTI_ANY_SIZE | f64.FLAG_ROWS_MULTI_STEPS)


def test_the_exactly_tiled_deck_runs_as_under_2048(f64, digests, monkeypatch):
    """rand_64x48 on 3 ranks of 16 rows: under 8192 the kernel, describe() and every bit of av_vels and of the cells are those of 2048."""
    p, obst = _deck(f64, digests, "rand_64x48")
    _force(monkeypatch, 3)
    state = _random_state(p, seed=21)
    out = {}
    for flags in (f64.FLAG_ROWS_MULTI_STEPS, f64.FLAG_ROWS_MULTI_ANY_SIZE, f64.FLAG_ROWS_MULTI_ANY_SIZE | f64.FLAG_ROWS_MULTI_STEPS):
        with f64.Rows64(p, obst, 3, devices=[0] * 3, flags=flags) as g:
            g.set_cells(state)
            out[flags] = (g.describe(), np.concatenate([g.run(11), g.run(6)]), g.get_cells(), g.last_run_ms()[1])
    d_2048, av_2048, cells_2048, n_2048 = out[f64.FLAG_ROWS_MULTI_STEPS]
    assert d_2048["kernel"] == "lbm_rows_multi_kernel_f64<3>" and n_2048 == 2 * 3
    for flags in (f64.FLAG_ROWS_MULTI_ANY_SIZE, f64.FLAG_ROWS_MULTI_ANY_SIZE | f64.FLAG_ROWS_MULTI_STEPS):
        d, av, cells, n = out[flags]
        assert d == d_2048 and n == n_2048
        assert np.array_equal(_bits(av), _bits(av_2048)) and np.array_equal(_bits(cells), _bits(cells_2048))


@pytest.mark.parametrize("nx,ny,nranks", [(33, 32, 2), (30, 32, 2), (64, 47, 3)])
def test_fallbacks_with_the_flag(lbm, f64, monkeypatch, nx, ny, nranks):
    """Odd nx, nx < 32 and a rank of 15 rows (16, 16, 15) run lbm_rows_kernel_f64 exactly as without the flag: the name, the ghost
    rows and state bytes, the launches, every bit."""
    _force(monkeypatch, 3)
    p, obst, nyls = _ragged_rows(lbm, nx, ny, nranks)
    if ny == 47:
        assert nyls == [16, 16, 15]
    state = _random_state(p, seed=5)
    out = {}
    for flags in (0, f64.FLAG_ROWS_MULTI_ANY_SIZE):
        with f64.Rows64(p, obst, nranks, devices=[0] * nranks, flags=flags) as g:
            g.set_cells(state)
            out[flags] = (g.describe(), np.concatenate([g.run(5), g.run(7)]), g.get_cells(), g.last_run_ms()[1])
    off, on = out[0], out[f64.FLAG_ROWS_MULTI_ANY_SIZE]
    assert on[0] == off[0] and on[0]["kernel"] == f"lbm_rows_kernel_f64<{2 if nx % 2 == 0 else 1}>" and on[3] == off[3] == 7 * nranks
    assert on[0]["state_bytes"] == 2 * 9 * 8 * nx * (ny + 2 * nranks)
    assert np.array_equal(_bits(on[1]), _bits(off[1])) and np.array_equal(_bits(on[2]), _bits(off[2]))
    ref_cells, _, _ = f64_ref.run(p, obst, 12, cells0=state)
    assert np.array_equal(_bits(on[2]), _bits(ref_cells))


# ---- flag on against flag off by per-row digests: the state never comes to the host ------------------------------------------------------

def _on_against_off_by_digests(lbm, f64, nx, ny, nranks, rows, steps, K):
    p, obst, nyls = _ragged_rows(lbm, nx, ny, nranks, rows)
    state = _smooth_state(p)
    out = {}
    for flags in (0, f64.FLAG_ROWS_MULTI_ANY_SIZE):
        with f64.Rows64(p, obst, nranks, devices=[0] * nranks, flags=flags) as g:
            g.set_cells(state)
            av = g.run(steps)
            out[flags] = (g.describe(), av, g.digest(), g.last_run_ms()[1])
    (d_off, av_off, (rows_off, sum_off), n_off), (d_on, av_on, (rows_on, sum_on), n_on) = out[0], out[f64.FLAG_ROWS_MULTI_ANY_SIZE]
    assert d_off["kernel"].startswith("lbm_rows_kernel_f64<2") and n_off == steps * nranks
    assert d_on["kernel"] in (_kernel_name(K), _kernel_name(K, nt=True)) and d_on["blocks"] == _tiles(nx, nyls) and n_on == -(-steps // K) * nranks, d_on
    assert d_on["state_bytes"] == 2 * 9 * 8 * nx * (ny + 2 * K * nranks)
    differ = np.nonzero(rows_on != rows_off)[0]
    assert differ.size == 0 and sum_on == sum_off, f"{nx}x{ny} on {nranks} ranks: rows that differ after {steps} steps: {differ[:16]}"
    assert np.all(av_off > 0.0)
    bound = rows_step_sum_bound(d_off) + rows_multi_sum_bound(d_on["blocks"], nranks)
    err = float(np.max(np.abs(av_on - av_off) / av_off))
    print(f"  {nx}x{ny} on {nranks} ranks, av_vels on against off: {err / U:.2f} x 2^-53 against a bound of {bound / U:.0f} x 2^-53")
    assert bound < 0.01 / (nx * ny) and err <= bound          # far below one miscounted cell


@pytest.mark.parametrize("K", BUILT_K)
def test_flag_on_against_flag_off_1000x600_on_4_ranks(lbm, f64, monkeypatch, K):
    """Ranks of 150 rows: 32 x 10 tiles a rank, the last column owning 8 columns and the last row 6 rows; 2K + 1 steps: two full
    launches and a 1-step tail."""
    _force(monkeypatch, K)
    _on_against_off_by_digests(lbm, f64, 1000, 600, 4, [150] * 4, 2 * K + 1, K)


def test_flag_on_against_flag_off_4098x2050_on_8_ranks(lbm, f64, monkeypatch):
    """Rows 257, 257, 256 x 6: uneven ranks, 129 x 17 tiles on the first two (their last tile row owns one row, every last tile column
    two columns) and 129 x 16 on the others; the smallest rank has 2^20 cells and more, above the rows' default minimum of 2^17: the
    library's own K and minimum size, no knob set."""
    for k in [k for k in os.environ if k.startswith("LBM_TUNE_")]:
        monkeypatch.delenv(k)
    _on_against_off_by_digests(lbm, f64, 4098, 2050, 8, [257, 257] + [256] * 6, 5, 4)


# ---- read-outs, devices, the CLI ------------------------------------------------------------------------------------------------------

def test_read_outs_after_an_edge_form_run(lbm, f64, monkeypatch):
    p, obst, nyls = _ragged_rows(lbm, 66, 50, 3)
    _force(monkeypatch, 3)
    state = _random_state(p, seed=9)
    with f64.Rows64(p, obst, 3, devices=[0] * 3, flags=f64.FLAG_ROWS_MULTI_ANY_SIZE) as g:
        _check_desc(g.describe(), p, nyls, 3)
        g.set_cells(state)
        g.run(19)
        cells, obs, tot, re = g.get_cells(), g.get_observables(), g.av_velocity_sum(), g.reynolds()
        rows, total = g.digest()
        part = g.digest(15, 36)                          # rows of all three ranks
    ref_cells, _, _ = f64_ref.run(p, obst, 19, cells0=state)
    assert np.array_equal(_bits(cells), _bits(ref_cells))
    assert np.array_equal(_bits(obs), _bits(f64_ref.observables(ref_cells)))
    assert re == f64_ref.reynolds(p, ref_cells, obst)
    host_rows, host_total = f64.digest_host(ref_cells, p.nx)
    assert np.array_equal(rows, host_rows) and total == host_total and np.array_equal(part[0], host_rows[15:36])
    # tests/test_f64_rows.py: lbm_rows64_av_velocity_sum's own tree
    rank_cells = [n * p.nx for n in nyls]
    blocks = [min(-(-n // 256), 1024) for n in rank_cells]
    bound = (max(-(-n // (b * 256)) for n, b in zip(rank_cells, blocks)) + 9 + sum(blocks)) * U
    exact = f64_ref.velocity_sum_exact(ref_cells, obst)
    assert abs(tot - exact) <= bound * exact


def test_one_gpu_per_rank(lbm, f64, monkeypatch):
    """Switches itself on where there are at least 2 GPUs: 66 x 50 on 3 ranks over devices 0, 1, 0, so that the K rows of a push between
    ranks of different nyl and plane stride travel as stores over a real link."""
    import torch
    count = torch.cuda.device_count()
    if count < 2:
        pytest.skip(f"needs 2 GPUs, this box has {count}")
    _force(monkeypatch, 4)
    p, obst, nyls = _ragged_rows(lbm, 66, 50, 3)
    _parity_any(f64, _case(_key(66, 50, 3), p, obst), nyls, 4, devices=[0, 1, 0])


def test_cli_row_blocks_with_the_flag(lbm, f64, tmp_path):
    """LBM_PRECISION=double LBM64_RANKS=3 bin/d2q9-bgk on a ragged 66 x 50 deck made here, 23 steps: final_state.dat and the digest line
    under LBM_FLAGS=8192 are those of LBM_FLAGS=0 and of the restatement, and LBM_DESCRIBE's line names the edge form and its launches."""
    from mpilattice_boltzmann_amd import decks
    p, obst, _ = _ragged_rows(lbm, 66, 50, 3)
    steps = 23
    (tmp_path / "input.params").write_text(f"{p.nx}\n{p.ny}\n{steps}\n{p.reynolds_dim}\n{p.density}\n{p.accel}\n{p.omega}\n")
    decks.write_obstacles(str(tmp_path / "obstacles.dat"), obst)
    base = {k: v for k, v in os.environ.items() if not k.startswith("LBM_")}
    out = {}
    for flags in ("0", "8192"):
        cwd = tmp_path / flags
        cwd.mkdir()
        env = dict(base, LBM_PRECISION="double", LBM64_RANKS="3", LBM_DEVICES="0,0,0", LBM_FLAGS=flags, LBM_DESCRIBE="1", LBM_DIGEST="1",
                   LBM_TUNE_MULTI64_MIN="0")                                                    # K: the library's default
        r = subprocess.run([lbm.CLI_PATH, str(tmp_path / "input.params"), str(tmp_path / "obstacles.dat")], cwd=cwd, env=env,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        ran = [line for line in r.stderr.splitlines() if line.startswith("kernel: ")]
        digest = [line for line in r.stderr.splitlines() if line.startswith("state digest: ")]
        assert len(ran) == 1 and len(digest) == 1, r.stderr
        out[flags] = (ran[0], (cwd / "final_state.dat").read_bytes(), digest[0], r.stdout.splitlines())
    assert out["0"][0] == f"kernel: lbm_rows_kernel_f64<2> on 3 ranks, {steps * 3} launches"
    K = int(out["8192"][0][len("kernel: lbm_rows_multi_kernel_f64<")])
    assert K in BUILT_K and out["8192"][0] == f"kernel: {_kernel_name(K)} on 3 ranks, {-(-steps // K) * 3} launches", out["8192"][0]
    assert out["8192"][1] == out["0"][1] and len(out["0"][1]) > 0
    assert out["8192"][2] == out["0"][2]
    ref_cells, _, _ = f64_ref.run(p, obst, steps)
    assert out["8192"][1].decode() == f64_ref.final_state_text(p, ref_cells, obst)
    assert out["8192"][2] == f"state digest: {f64.digest_host(ref_cells, p.nx)[1]:016x}"
    assert out["8192"][3][0] == "==done==" and out["8192"][3][1] == out["0"][3][1]              # the Reynolds number line
