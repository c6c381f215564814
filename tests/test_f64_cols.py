"""Column-partitioned double-precision runs on the GPU (include/lbm_d2q9_f64_cols.h, csrc/lbm_cols64.hip, csrc/kernels/cols64.h) held to
the CPU restatement tests/f64_ref.c by tests/test_f64_rows.py's protocol and references: populations bit for bit for every rank count
and K, av_vels within the bound of the ranks' summation trees plus the host's additions over the ranks, the read-outs, the digest, the
whole 128 x 128 deck against the results the reference shipped, the CLI.  All ranks run on device 0 (ranks may share a device); one test
switches itself on where there are two GPUs or more.

The bound on av_vels.  A rank's sum of a step is lbm_multi_kernel_f64's tree over the rank's tiles, so its relative error against the
exactly rounded sum is tests/test_f64_multi.py's multi_sum_bound(tiles); the host then adds the nranks ranks' sums in rank order,
nranks - 1 more additions of non-negative terms: multi_sum_bound(tiles of the largest rank) + (nranks - 1) * 2^-53."""
import os
import subprocess

import numpy as np
import pytest

import f64_ref
from conftest import deck_paths
from test_f64_multi import multi_sum_bound
from test_f64_rows import BLOCK, U, _bits, _deck, _random_state, _reference, _synthetic

pytestmark = pytest.mark.gpu

TX, TY = 32, 16


@pytest.fixture(scope="module")
def f64(lbm):
    from mpilattice_boltzmann_amd import f64 as mod
    mod.load_cols_library()
    mod.load_digest_library()
    return mod


def _force(monkeypatch, K=None):
    """A run reads the knobs when it is made.  K None: the default."""
    if K is None:
        monkeypatch.delenv("LBM_TUNE_MULTI64_K", raising=False)
    else:
        monkeypatch.setenv("LBM_TUNE_MULTI64_K", str(K))
    monkeypatch.setenv("LBM_TUNE_MULTI64_MIN", "0")          # for the Rows64 and Grid64 runs beside it
    monkeypatch.delenv("LBM_TUNE_MAXBLOCKS", raising=False)


def _columns(nx, nranks):
    """lbm_decompose_columns: whole x-pairs, the spare pairs to the first ranks."""
    pairs, spare = divmod(nx // 2, nranks)
    return [2 * (pairs + (1 if r < spare else 0)) for r in range(nranks)]


def _kernel_name(K, nt=False, edge=False):
    return f"lbm_cols_multi_kernel_f64<{K}" + (",nt" if nt else "") + (",edge" if edge else "") + ">"


def cols_sum_bound(tiles, nranks):
    """The module docstring's bound."""
    return multi_sum_bound(tiles) + (nranks - 1) * U


def _check_av(av, exact, obst, tiles, nranks):
    ref = f64_ref.av_vels(exact, obst)
    assert av.shape == ref.shape
    # (a deck whose accelerated row is blocked stays at rest: every entry is 0 on both sides, and the error is taken absolutely)
    err = float(np.max(np.abs(av - ref) / ref)) if np.all(ref > 0) else float(np.max(np.abs(av - ref)))
    bound = cols_sum_bound(tiles, nranks)
    print(f"  av_vels on {nranks} column ranks of {tiles} tiles: {err / U:.2f} x 2^-53 against a bound of {bound / U:.0f} x 2^-53")
    assert err <= bound


def _check_desc(desc, p, nranks, K, nt=False):
    """The kernel's name, the tiles of the largest rank and the bytes of every rank's two grids, ghost columns included."""
    widest = max(_columns(p.nx, nranks))
    tiles = -(-widest // TX) * -(-p.ny // TY)
    edge = widest % TX != 0 or p.ny % TY != 0
    G = 2 * -(-K // 2)
    assert desc["kernel"] == _kernel_name(K, nt, edge), desc
    assert desc["nranks"] == nranks and desc["blocks"] == tiles and desc["cells_per_block"] == TX * TY, desc
    assert desc["state_bytes"] == 2 * 9 * 8 * p.ny * (p.nx + 2 * G * nranks), desc
    return tiles


def _parity(f64, key, p, obst, nranks, K, flags=0, nt=False, devices=None):
    """tests/test_f64_rows.py's protocol and its references (computed once per deck, shared with that file's tests).  37 steps from
    rest: at K = 4 nine full launches and a one-step tail, the direct-store form.  Then run(5) + run(7) from a random positive state
    against 12 steps: the accelerate that run(5) skipped after its last step is run(7)'s pre-pass, whose cells push -1 then sends."""
    ref37, exact37, state, ref12, exact12 = _reference(key, p, obst)
    with f64.Cols64(p, obst, nranks, devices=devices if devices is not None else [0] * nranks, flags=flags) as g:
        desc = g.describe()
        tiles = _check_desc(desc, p, nranks, K, nt)
        av = g.run(37)
        assert g.last_run_ms()[1] == -(-37 // K) * nranks
        assert np.array_equal(_bits(g.get_cells()), _bits(ref37)), f"{p.nx}x{p.ny} on {nranks} column ranks, 37 steps from rest: {desc}"
        _check_av(av, exact37, obst, tiles, nranks)
        g.set_cells(state)
        av = np.concatenate([g.run(5), g.run(7)])
        assert g.last_run_ms()[1] == -(-7 // K) * nranks
        assert np.array_equal(_bits(g.get_cells()), _bits(ref12)), f"{p.nx}x{p.ny} on {nranks} column ranks, run(5) + run(7) from a random state: {desc}"
        assert ref12.min() > 0.0                         # the premise of the bound: positive densities, non-negative terms
        _check_av(av, exact12, obst, tiles, nranks)
    return desc


# ---- the smallest shapes at which each thing can go wrong ---------------------------------------------------------------------------

# 32 x 16 on 1 rank: one tile; the rank fills its own ghost columns.  64 x 16 on 2: both neighbours are the same rank; K = 3 is the case
# G = 4 > K.  96 x 16 on 3: three distinct neighbours.  64 x 32 on 1: two tile rows and columns inside a block, the ring wraps in y.
# 68 x 16 on 2: blocks of 34, tiles shifted in x.  64 x 18 on 2: tiles shifted in y across the wrap.  70 x 18 on 2: blocks of 36 and 34
# (two pitches), both shifts.
SHAPES = [(32, 16, 1, 4), (64, 16, 2, 2), (64, 16, 2, 3), (64, 16, 2, 4), (96, 16, 3, 4), (64, 32, 1, 4), (68, 16, 2, 4), (64, 18, 2, 4),
          (70, 18, 2, 4)]


@pytest.mark.parametrize("nx,ny,nranks,K", SHAPES)
def test_bit_parity_shapes(lbm, f64, monkeypatch, nx, ny, nranks, K):
    p, obst = _synthetic(lbm, nx, ny)
    _force(monkeypatch, K)
    if (nx, nranks) == (70, 2):
        assert _columns(nx, nranks) == [36, 34]
    desc = _parity(f64, ("shape", nx, ny), p, obst, nranks, K)
    assert ("edge" in desc["kernel"]) == ((nx, ny) in ((68, 16), (64, 18), (70, 18)))


# rand_64x48 and open_64x48 on 2 ranks of 32 columns and three tile rows; the others on 1 rank: walls_40x24 (both shifts, walls on the
# block's edge columns), dense_32x32 (most cells blocked), the two 32 x 16 decks (blocked cells and strong forcing on the accelerated row,
# whose copies sit in the rank's own ghost columns and in the frame's ring).
DECKS = [("rand_64x48", 2, 2), ("rand_64x48", 2, 3), ("rand_64x48", 2, 4), ("open_64x48", 2, 4), ("walls_40x24", 1, 4), ("dense_32x32", 1, 4),
         ("accelrow_blocked_32x16", 1, 4), ("strongaccel_32x16", 1, 4)]


@pytest.mark.parametrize("name,nranks,K", DECKS)
def test_bit_parity_decks(f64, digests, monkeypatch, name, nranks, K):
    p, obst = _deck(f64, digests, name)
    _force(monkeypatch, K)
    _parity(f64, name, p, obst, nranks, K)


@pytest.mark.parametrize("flag,nt", [("FLAG_NT_STORES", True), ("FLAG_NO_NT_STORES", False)])
def test_bit_parity_under_the_nt_flags(f64, digests, monkeypatch, flag, nt):
    p, obst = _deck(f64, digests, "rand_64x48")
    _force(monkeypatch, 4)
    _parity(f64, "rand_64x48", p, obst, 2, 4, flags=getattr(f64, flag), nt=nt)


def test_the_four_ways_to_run_a_grid_give_the_same_populations(f64, digests, monkeypatch):
    """12 steps from one random state: Cols64, Rows64, Rows64 with FLAG_ROWS_MULTI_ANY_SIZE, Grid64."""
    p, obst = _deck(f64, digests, "rand_64x48")
    _force(monkeypatch)
    state = _random_state(p, seed=21)
    got = {}
    for tag, make in (("cols", lambda: f64.Cols64(p, obst, 2, devices=[0] * 2)),
                      ("rows", lambda: f64.Rows64(p, obst, 3, devices=[0] * 3)),
                      ("rows any", lambda: f64.Rows64(p, obst, 2, devices=[0] * 2, flags=f64.FLAG_ROWS_MULTI_ANY_SIZE)),
                      ("grid", lambda: f64.Grid64(p, obst))):
        with make() as g:
            kernel = g.describe()["kernel"]
            g.set_cells(state)
            g.run(12)
            got[tag] = (kernel, _bits(g.get_cells()))
    assert got["cols"][0].startswith("lbm_cols_multi_kernel_f64<") and got["rows"][0] == "lbm_rows_kernel_f64<2>"
    assert got["rows any"][0].startswith("lbm_rows_multi_kernel_f64<") and "edge" in got["rows any"][0] and got["grid"][0] == "lbm_step_kernel_f64<2>"
    for tag in ("rows", "rows any", "grid"):
        assert np.array_equal(got["cols"][1], got[tag][1]), tag


def test_two_identical_runs_give_identical_av_vels(f64, digests, monkeypatch):
    p, obst = _deck(f64, digests, "rand_64x48")
    _force(monkeypatch)
    state = _random_state(p, seed=3)
    got = []
    for _ in range(2):
        with f64.Cols64(p, obst, 2, devices=[0, 0]) as g:
            assert g.describe()["kernel"].startswith("lbm_cols_multi_kernel_f64<")
            g.set_cells(state)
            got.append((g.run(22), g.get_cells()))
    assert np.array_equal(_bits(got[0][0]), _bits(got[1][0])) and np.array_equal(_bits(got[0][1]), _bits(got[1][1]))
    assert np.all(got[0][0] > 0)


def test_cells_round_trip_keeps_every_bit(lbm, f64, monkeypatch):
    """get_cells(set_cells(x)) == x as bit patterns on 2 ranks of 36 and 34 columns: NaNs with payloads, both zeros, denormals,
    infinities, spread over both ranks' columns; with a chunk of one row and with the default chunk."""
    _force(monkeypatch)
    p, obst = _synthetic(lbm, 70, 18)
    state = _random_state(p)
    special = np.array([0x7FF8000000000001, 0xFFF4000000ABCDEF, 0x7FF0000000000001, 0x0000000000000000, 0x8000000000000000,
                        0x0000000000000001, 0x800FFFFFFFFFFFFF, 0x7FF0000000000000, 0xFFF0000000000000], np.uint64)
    flat = _bits(state).reshape(-1)
    flat[:special.size * 307:307] = special            # 307 doubles apart: cells 34 apart, on both sides of column 36
    assert {(i * 307 // 9) % 70 >= 36 for i in range(special.size)} == {False, True}
    for chunk in ("1", None):
        if chunk:
            monkeypatch.setenv("LBM_TUNE_OBS_CHUNK_CELLS", chunk)
        else:
            monkeypatch.delenv("LBM_TUNE_OBS_CHUNK_CELLS", raising=False)
        with f64.Cols64(p, obst, 2, devices=[0, 0]) as g:
            assert g.describe()["kernel"] == _kernel_name(4, edge=True)
            g.set_cells(state)
            assert np.array_equal(_bits(g.get_cells()), _bits(state)), chunk


def test_observables_velocity_sum_and_reynolds(lbm, f64, digests, monkeypatch):
    """lbm_cols64_get_observables bit for bit against the numpy restatement of write_values' arithmetic; lbm_cols64_av_velocity_sum
    against the exactly rounded sum of av_velocity's terms, within the bound of ITS order of additions: on rank r of n_r = nxl_r * ny
    cells and b_r = min(ceil(n_r / 256), 1024) blocks a lane adds ceil(n_r / (b_r * 256)) terms serially, block_sum's nine, then the host
    adds the ranks' b_r block sums serially, rank after rank; Cols64.reynolds sums on the host in the reference's cell order: Grid64's bits."""
    _force(monkeypatch)
    for (p, obst), nranks in ((_deck(f64, digests, "rand_64x48"), 2), (_synthetic(lbm, 70, 18), 2), (_synthetic(lbm, 700, 600, p_block=0.05), 3)):
        state = _random_state(p, seed=9)
        with f64.Cols64(p, obst, nranks, devices=[0] * nranks) as g:
            _check_desc(g.describe(), p, nranks, 4)
            g.set_cells(state)
            g.run(3)
            cells = g.get_cells()
            obs = g.get_observables()
            tot = g.av_velocity_sum()
            re = g.reynolds()
        with f64.Grid64(p, obst) as g:
            g.set_cells(state)
            g.run(3)
            re_whole = g.reynolds()
            assert np.array_equal(_bits(g.get_cells()), _bits(cells)), (p.nx, p.ny)
        assert np.array_equal(_bits(obs), _bits(f64_ref.observables(cells))), (p.nx, p.ny)
        rank_cells = [nxl * p.ny for nxl in _columns(p.nx, nranks)]
        blocks = [min(-(-n // BLOCK), 1024) for n in rank_cells]
        bound = (max(-(-n // (b * BLOCK)) for n, b in zip(rank_cells, blocks)) + 9 + sum(blocks)) * U
        exact = f64_ref.velocity_sum_exact(cells, obst)
        print(f"  {p.nx}x{p.ny} on {nranks} column ranks, velocity sum: {abs(tot - exact) / exact / U:.2f} x 2^-53 against {bound / U:.0f} x 2^-53")
        assert abs(tot - exact) <= bound * exact
        assert re == f64_ref.reynolds(p, cells, obst)
        assert re == re_whole


def test_digest_row_by_row_and_between_two_runs(lbm, f64, monkeypatch):
    """70 x 18 on 2 ranks: digest() row by row equals f64.digest_host(get_cells()) and Grid64.digest() of the same state, for the whole
    grid and for a range of rows; and a digest between two runs leaves both runs' results as they are without it."""
    _force(monkeypatch)
    p, obst = _synthetic(lbm, 70, 18)
    state = _random_state(p, seed=5)
    with f64.Grid64(p, obst) as g:
        g.set_cells(state)
        g.run(5)
        g.run(7)
        want_rows, want_sum = g.digest()
        want_cells = _bits(g.get_cells())
    with f64.Cols64(p, obst, 2, devices=[0, 0]) as g:
        assert g.describe()["kernel"] == _kernel_name(4, edge=True)
        g.set_cells(state)
        rows0, sum0 = g.digest()
        host0 = f64.digest_host(state, p.nx)
        assert np.array_equal(rows0, host0[0]) and sum0 == host0[1]
        av_a = g.run(5)
        mid_rows, mid_sum = g.digest()
        assert np.array_equal(mid_rows, f64.digest_host(g.get_cells(), p.nx)[0])
        av_b = g.run(7)
        rows, total = g.digest()
        cells = g.get_cells()
        part_rows, part_sum = g.digest(3, 11)
        assert g.digest(4, 4)[1] == 0
        with pytest.raises(lbm.LbmError, match="rows outside the grid"):
            g.digest(0, p.ny + 1)
    host_rows, host_sum = f64.digest_host(cells, p.nx)
    assert np.array_equal(rows, host_rows) and total == host_sum
    assert np.array_equal(rows, want_rows) and total == want_sum and np.array_equal(_bits(cells), want_cells)
    assert np.array_equal(part_rows, rows[3:11]) and part_sum == int(np.sum(rows[3:11], dtype=np.uint64))
    assert mid_sum != total and mid_sum != sum0
    with f64.Cols64(p, obst, 2, devices=[0, 0]) as g:       # the same two runs with no digest between them
        assert g.describe()["kernel"] == _kernel_name(4, edge=True)
        g.set_cells(state)
        av_plain = np.concatenate([g.run(5), g.run(7)])
        assert np.array_equal(_bits(g.get_cells()), _bits(cells))
    assert np.array_equal(_bits(np.concatenate([av_a, av_b])), _bits(av_plain))


def test_a_refused_create_leaves_no_hip_error_behind(lbm, f64, digests, monkeypatch):
    """A create that fails in its first HIP call (a device ordinal no machine has) reports that call, and the next create of the same
    thread is none the worse for it: the failed call's error is read where it is reported (csrc/lbm_hip_try.h), not left as the thread's
    last HIP error for the hipGetLastError() after the next launch to find."""
    _force(monkeypatch)
    p, obst = _deck(f64, digests, "rand_64x48")
    for make in (lambda d: f64.Cols64(p, obst, 2, devices=[d, d]), lambda d: f64.Rows64(p, obst, 2, devices=[d, d]), lambda d: f64.Grid64(p, obst, device=d)):
        with pytest.raises(lbm.LbmError, match="hipSetDevice"):
            make(4096)
        with make(0) as g:
            assert g.describe()["kernel"]
            assert np.all(g.run(4) > 0)
    with f64.Cols64(p, obst, 2, devices=[0, 0]) as g:
        assert g.describe()["kernel"] == _kernel_name(4)


def test_whole_128x128_deck_on_4_column_ranks_bits_and_shipped_results(lbm, f64, monkeypatch):
    """40 000 steps on 4 ranks of 32 columns, the library's default K: about a second on the device.  The restatement's run is
    f64_ref.deck_run's, once per process."""
    _force(monkeypatch)
    p, obst, ref_cells, serial, exact = f64_ref.deck_run("128x128")
    p64 = f64.read_params64(os.path.join(f64_ref.GOLDEN, "decks", "input_128x128.params"))
    assert (p64.density, p64.accel, p64.omega) == (p.density, p.accel, p.omega)
    with f64.Cols64(p64, obst, 4, devices=[0] * 4) as g:
        desc = g.describe()
        assert desc["kernel"].startswith("lbm_cols_multi_kernel_f64<"), desc
        K = int(desc["kernel"][len("lbm_cols_multi_kernel_f64<"):-1])
        tiles = _check_desc(desc, p64, 4, K)
        av = g.run(p64.max_iters)
        ms, launches = g.last_run_ms()
        cells = g.get_cells()
        obs = g.get_observables()
        re = g.reynolds()
    assert launches == -(-p64.max_iters // K) * 4
    print(f"  128x128 on 4 column ranks, {p64.max_iters} steps with {desc['kernel']}: {ms:.1f} ms in {launches} launches")
    assert np.array_equal(_bits(cells), _bits(ref_cells)), "populations after 40 000 steps"
    _check_av(av, exact, obst, tiles, 4)
    # against what the reference shipped: check.py's rule — the CPU test's limits (f64_ref) — plus the summation bound
    golden_av = f64_ref.golden_av_vels("128x128")
    av_rel = float(np.max(np.abs(av - golden_av) / np.abs(golden_av)))
    values = obs.copy()
    values[obst != 0] = (0.0, 0.0, 0.0, p.density * (1.0 / 3.0))
    fs_abs = float(np.max(np.abs(values.reshape(-1, 4) - f64_ref.golden_final_state("128x128"))))
    pub = float(f64_ref.published()["reynolds"]["128x128"]["value"])
    print(f"  against the shipped results: av_vels {av_rel:.3e} rel, final_state {fs_abs:.3e} abs, Reynolds {re!r}")
    assert av_rel <= f64_ref.AV_VELS_LIMIT + cols_sum_bound(tiles, 4)
    assert fs_abs <= f64_ref.FINAL_STATE_LIMIT
    assert abs(re - pub) / pub <= f64_ref.REYNOLDS_LIMIT


def test_cli_column_blocks(lbm, f64, digests, tmp_path):
    """LBM_PRECISION=double LBM64_COLS=2 bin/d2q9-bgk on rand_64x48: final_state.dat, the Reynolds line and the state digest are those
    of LBM_PRECISION=double alone, and LBM_DESCRIBE's line names the kernel with 2 * ceil(max_iters / K) launches."""
    ppath, opath = deck_paths("rand_64x48", digests)
    p, _ = _deck(f64, digests, "rand_64x48")
    env = {k: v for k, v in os.environ.items() if not k.startswith("LBM")}
    env.update(LBM_PRECISION="double", LBM_DIGEST="1")
    out = {}
    for tag, extra in (("whole", {}), ("cols", dict(LBM64_COLS="2", LBM_DEVICES="0,0", LBM_DESCRIBE="1"))):
        cwd = tmp_path / tag
        cwd.mkdir()
        r = subprocess.run([lbm.CLI_PATH, ppath, opath], cwd=cwd, env={**env, **extra}, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        out[tag] = (r.stdout.splitlines(), (cwd / "final_state.dat").read_bytes(), r.stderr)
    lines = out["cols"][0]
    assert lines[0] == "==done==" and lines[5].endswith("(2 column ranks, double precision)")
    assert lines[1].startswith("Reynolds number:\t\t") and lines[1] == out["whole"][0][1]
    assert out["cols"][1] == out["whole"][1]
    digest = [[line for line in out[tag][2].splitlines() if line.startswith("state digest: ")] for tag in ("whole", "cols")]
    assert len(digest[0]) == 1 and digest[0] == digest[1] and len(digest[0][0]) == len("state digest: ") + 16
    ran = [line for line in out["cols"][2].splitlines() if line.startswith("kernel: ")]
    assert len(ran) == 1 and ran[0].startswith("kernel: lbm_cols_multi_kernel_f64<"), out["cols"][2]
    K = int(ran[0][len("kernel: lbm_cols_multi_kernel_f64<"):ran[0].index(">")])
    assert K in (2, 3, 4) and ran[0] == f"kernel: lbm_cols_multi_kernel_f64<{K}> on 2 column ranks, {2 * -(-p.max_iters // K)} launches", ran[0]


def test_one_gpu_per_rank(f64, digests, monkeypatch):
    """Switches itself on where there are at least 2 GPUs: the G columns of a push then travel as stores over a real link.  The
    rand_64x48 parity on devices 0 and 1."""
    import torch
    count = torch.cuda.device_count()
    if count < 2:
        pytest.skip(f"needs 2 GPUs, this box has {count}")
    _force(monkeypatch, 4)
    p, obst = _deck(f64, digests, "rand_64x48")
    _parity(f64, "rand_64x48", p, obst, 2, 4, devices=[0, 1])
