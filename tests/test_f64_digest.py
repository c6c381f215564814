"""The state digests of the double-precision mode on the GPU (include/lbm_d2q9_f64_digest.h; lbm64_row_digest_kernel of
csrc/kernels/step64.h through lbm_digest64_grid and lbm_digest64_rows) held to the numpy restatement tests/digest64_ref.py and to
lbm_digest64_host on the state get_cells returns: every storage layout (a whole grid, a rank with one ghost row, a rank with K), every
kernel family that advances them, rows wider than a block, edge values, sub-ranges across ranks, and that a digest leaves the next run
as it would have been.  All ranks run on device 0; one test switches itself on where there are two GPUs or more."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import digest64_ref as ref
import f64_ref
from conftest import deck_paths

pytestmark = pytest.mark.gpu

MASK = ref.MASK


@pytest.fixture(scope="module")
def f64(lbm):
    from mpilattice_boltzmann_amd import f64 as mod
    mod.load_digest_library()
    return mod


def _synthetic(lbm, nx, ny, seed=11):
    p = lbm.Params(nx=nx, ny=ny, max_iters=10, reynolds_dim=10, density=0.1, accel=0.005, omega=1.85)
    obst = lbm.synthetic_obstacles(nx, ny, p=0.2, seed=seed, walls=False)
    obst.flat[obst.size // 2] = 0                      # at least one free cell
    return p, obst


def _deck(f64, digests, name):
    ppath, opath = deck_paths(name, digests)
    p = f64.read_params64(ppath)
    return p, f64_ref.read_obstacles(opath, p.nx, p.ny)


def _random_state(p, seed=7):
    """tests/test_f64.py's: each population of the rest state times a factor from [0.8, 1.2)."""
    return f64_ref.initial_cells(p) * np.random.default_rng(seed).uniform(0.8, 1.2, (p.ny, p.nx, 9))


def _force_multi(monkeypatch, K=None):
    """tests/test_f64_multi.py's and tests/test_f64_rows_multi.py's _force: the tests choose the kernel by shape, not by the minimum size."""
    monkeypatch.setenv("LBM_TUNE_MULTI64_MIN", "0")
    if K is None:
        monkeypatch.delenv("LBM_TUNE_MULTI64_K", raising=False)
    else:
        monkeypatch.setenv("LBM_TUNE_MULTI64_K", str(K))
    for k in ("LBM_TUNE_TILE64_MAX", "LBM_TUNE_TILE64_GEOM", "LBM_TUNE_MAXBLOCKS"):
        monkeypatch.delenv(k, raising=False)


def _check(f64, g, what=""):
    """g.digest() against the restatement and the host form on g.get_cells(); returns the row digests."""
    nx, ny = g.params.nx, g.params.ny
    rows, total = g.digest()
    cells = g.get_cells()
    want = ref.row_digests(cells, nx)
    assert rows.dtype == np.uint64 and rows.shape == (ny,)
    assert np.array_equal(rows, want), (what, [int(y) for y in np.nonzero(rows != want)[0]])
    host_rows, host_total = f64.digest_host(cells, nx)
    assert np.array_equal(rows, host_rows) and total == host_total == sum(int(v) for v in rows) & MASK, what
    return rows


# ---- whole grids --------------------------------------------------------------------------------------------------------------------
# (nx, ny, flag, kernel named by describe(), steps of the first run, steps of the second)
WHOLE = [(7, 5, None, "lbm_step_kernel_f64<1>", 1, 5),            # one cell per lane; rows far narrower than a block
         (8, 3, None, "lbm_step_kernel_f64<2>", 1, 5),            # the tiny_8x3 deck
         (300, 3, None, "lbm_step_kernel_f64<2>", 1, 5),          # a row wider than a block, with a tail of 44 lanes
         (8, 8, "FLAG_TILE_STEPS", "lbm_tile_kernel_f64", 1, 5),  # the smallest grid 8 x 8 tiles cover
         (64, 32, "FLAG_MULTI_STEPS", "lbm_multi_kernel_f64", 4, 1)]   # after one launch (4 steps) and after two (5)


@pytest.mark.parametrize("nx,ny,flag,kernel,first,second", WHOLE)
def test_whole_grids(lbm, f64, digests, monkeypatch, nx, ny, flag, kernel, first, second):
    _force_multi(monkeypatch, 4 if flag == "FLAG_MULTI_STEPS" else None)
    p, obst = _deck(f64, digests, "tiny_8x3") if (nx, ny) == (8, 3) else _synthetic(lbm, nx, ny)
    assert (p.nx, p.ny) == (nx, ny)
    with f64.Grid64(p, obst, flags=getattr(f64, flag) if flag else 0) as g:
        assert g.describe()["kernel"].startswith(kernel), g.describe()
        g.set_cells(_random_state(p))
        before = _check(f64, g, "before any step")
        g.run(first)
        after_first = _check(f64, g, f"after {first} steps")
        g.run(second)
        after_second = _check(f64, g, f"after {first + second} steps")
        assert not np.array_equal(before, after_first) and not np.array_equal(after_first, after_second)


def test_ranges_and_refusals_on_a_whole_grid(lbm, f64):
    p, obst = _synthetic(lbm, 300, 7)
    with f64.Grid64(p, obst) as g:
        g.set_cells(_random_state(p))
        g.run(2)
        rows, total = g.digest()
        for lo, hi in ((0, 7), (0, 1), (6, 7), (2, 5), (3, 3), (7, 7), (0, 0)):
            part, t = g.digest(lo, hi)
            assert np.array_equal(part, rows[lo:hi]) and t == sum(int(v) for v in rows[lo:hi]) & MASK, (lo, hi)
        for lo, hi in ((-1, 3), (0, 8), (5, 4), (8, 8)):
            with pytest.raises(lbm.LbmError, match="lbm_digest64_grid: rows outside the grid"):
                g.digest(lo, hi)
        lib = f64.load_digest_library()
        assert lib.lbm_digest64_grid(g._ctx, 0, 7, None, None) != 0
        assert "both output pointers are null" in lbm.load_library().lbm_last_error().decode()
        only = C.c_ulonglong(0)
        assert lib.lbm_digest64_grid(g._ctx, 0, 7, None, C.byref(only)) == 0 and only.value == total
        assert np.array_equal(g.digest()[0], rows)        # and the state is as it was


# ---- row blocks, the one-step kernel ------------------------------------------------------------------------------------------------
_WHOLE_RUNS = {}


def _whole_run(f64, key, p, obst, state, steps):
    """Grid64's row digests and cells after `steps` steps from `state`, once per key and never written to."""
    if key not in _WHOLE_RUNS:
        with f64.Grid64(p, obst) as g:
            g.set_cells(state)
            g.run(steps)
            rows = _check(f64, g, key)
            cells = g.get_cells()
        rows.setflags(write=False)
        cells.setflags(write=False)
        _WHOLE_RUNS[key] = (rows, cells)
    return _WHOLE_RUNS[key]


@pytest.mark.parametrize("nranks", [1, 2, 3, 8])
def test_row_blocks_rand_64x48(lbm, f64, digests, nranks):
    p, obst = _deck(f64, digests, "rand_64x48")
    state = _random_state(p, seed=21)
    want, cells = _whole_run(f64, "rand_64x48/5", p, obst, state, 5)
    owned, displs = lbm.decompose(p.ny, nranks)
    with f64.Rows64(p, obst, nranks, devices=[0] * nranks) as g:
        assert g.describe()["kernel"] == "lbm_rows_kernel_f64<2>"
        g.set_cells(state)
        g.run(5)
        rows = _check(f64, g, f"{nranks} ranks")
        assert np.array_equal(rows, want) and np.array_equal(ref.bits(g.get_cells()), ref.bits(cells))
        # sub-ranges: inside one rank (that rank alone is launched on: the others' rows are not in the answer), from the middle of one
        # rank to the middle of another, whole ranks, single rows at both ends of the grid and at both sides of every cut, none
        ranges = {(0, p.ny), (0, 1), (p.ny - 1, p.ny), (5, 41), (17, 30), (20, 20), (p.ny, p.ny)}
        for r in range(nranks):
            lo, hi = displs[r], displs[r] + owned[r]
            ranges |= {(lo, hi), (lo, lo + 1), (hi - 1, hi), (max(lo - 1, 0), min(lo + 1, p.ny)), (lo + 1, hi - 1)}
        for lo, hi in sorted(ranges):
            part, t = g.digest(lo, hi)
            assert np.array_equal(part, want[lo:hi]) and t == sum(int(v) for v in want[lo:hi]) & MASK, (nranks, lo, hi)
        for lo, hi in ((-1, 3), (0, p.ny + 1), (5, 4)):
            with pytest.raises(lbm.LbmError, match="lbm_digest64_rows: rows outside the grid"):
                g.digest(lo, hi)
        assert f64.load_digest_library().lbm_digest64_rows(g._run, 0, p.ny, None, None) != 0
        assert "both output pointers are null" in lbm.load_library().lbm_last_error().decode()


@pytest.mark.parametrize("nx", [7, 8])
def test_row_blocks_of_two_two_and_three_rows(lbm, f64, nx):
    p, obst = _synthetic(lbm, nx, 7)
    assert lbm.decompose(7, 3)[0] == [2, 2, 3]
    state = _random_state(p, seed=4)
    want, _ = _whole_run(f64, f"{nx}x7/5", p, obst, state, 5)
    with f64.Rows64(p, obst, 3, devices=[0, 0, 0]) as g:
        g.set_cells(state)
        g.run(5)
        assert np.array_equal(_check(f64, g), want)
        for lo, hi in ((1, 3), (1, 6), (3, 4), (4, 7)):
            assert np.array_equal(g.digest(lo, hi)[0], want[lo:hi]), (lo, hi)


# ---- row blocks, several steps per exchange: K ghost rows a side --------------------------------------------------------------------
@pytest.mark.parametrize("nx,ny,nranks", [(32, 32, 2), (64, 48, 3)])
def test_row_blocks_under_the_multi_steps_flag(lbm, f64, monkeypatch, nx, ny, nranks):
    _force_multi(monkeypatch, 4)
    p, obst = _synthetic(lbm, nx, ny)
    state = _random_state(p, seed=6)
    runs = {}
    for tag, make in (("whole", lambda: f64.Grid64(p, obst)),
                      ("rows", lambda: f64.Rows64(p, obst, nranks, devices=[0] * nranks)),
                      ("rows multi", lambda: f64.Rows64(p, obst, nranks, devices=[0] * nranks, flags=f64.FLAG_ROWS_MULTI_STEPS))):
        with make() as g:
            if tag == "rows multi":
                assert g.describe()["kernel"] == "lbm_rows_multi_kernel_f64<4>", g.describe()
            g.set_cells(state)
            g.run(4)
            after4 = _check(f64, g, f"{tag}, 4 steps")        # one launch of the multi-step kernel
            g.run(1)
            after5 = _check(f64, g, f"{tag}, 5 steps")        # and its one-step tail, from the other grid
            mid = g.digest(ny // nranks - 3, ny // nranks + 5)[0]
            runs[tag] = (after4, after5, mid)
    for tag in ("rows", "rows multi"):
        for a, b in zip(runs[tag], runs["whole"]):
            assert np.array_equal(a, b), tag
    assert np.array_equal(runs["whole"][2], runs["whole"][1][ny // nranks - 3:ny // nranks + 5])


# ---- edge values through the device -------------------------------------------------------------------------------------------------
def test_edge_values_before_any_step(lbm, f64):
    nx, ny = 16, 8
    p, obst = _synthetic(lbm, nx, ny)
    state = ref.edge_state(nx, ny, seed=2)
    held = set(int(v) for v in ref.bits(state).reshape(-1))
    assert held >= set(int(v) for v in ref.EDGE_BITS)
    want = ref.row_digests(state, nx)
    for make in (lambda: f64.Grid64(p, obst), lambda: f64.Rows64(p, obst, 2, devices=[0, 0])):
        with make() as g:
            g.set_cells(state)
            rows, total = g.digest()
            assert np.array_equal(rows, want), [int(y) for y in np.nonzero(rows != want)[0]]
            assert total == ref.digest(state, nx)
            assert np.array_equal(ref.bits(g.get_cells()), ref.bits(state))


# ---- localisation -------------------------------------------------------------------------------------------------------------------
def test_differing_rows_finds_the_row(f64, digests):
    p, obst = _deck(f64, digests, "rand_64x48")
    state = _random_state(p, seed=8)
    other = state.copy()
    ref.bits(other).reshape(p.ny, p.nx, 9)[17, 63, 7] ^= np.uint64(1) << np.uint64(20)
    with f64.Grid64(p, obst) as a, f64.Grid64(p, obst) as b, f64.Rows64(p, obst, 3, devices=[0, 0, 0]) as c:
        a.set_cells(state)
        b.set_cells(other)
        c.set_cells(other)
        assert f64.differing_rows(a, a) == [] and f64.differing_rows(b, c) == []
        assert f64.differing_rows(a, b) == [17] == f64.differing_rows(a, c) == f64.differing_rows(c, a)
        for g in (a, b, c):
            g.run(1)
        rows = f64.differing_rows(a, b)
        assert rows and set(rows) <= {16, 17, 18}, rows
        assert f64.differing_rows(a, c) == rows and f64.differing_rows(b, c) == []


# ---- no side effect -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["whole", "tiled", "3 row blocks"])
def test_a_digest_between_two_runs_changes_nothing(f64, digests, monkeypatch, how):
    """run(3), digest, run(5) against run(3), run(5): the same cells and the same 8 av_vels bits.  The first entry of the second run
    is folded by block 0 of its second launch from the partials of its first, and the last by the fold after the loop, from the
    counter the first run left: a digest launch that wrote to any of them would show here.  Nor do the last run's events move."""
    _force_multi(monkeypatch)
    p, obst = _deck(f64, digests, "rand_64x48")
    state = _random_state(p, seed=12)
    make = {"whole": lambda: f64.Grid64(p, obst), "tiled": lambda: f64.Grid64(p, obst, flags=f64.FLAG_TILE_STEPS),
            "3 row blocks": lambda: f64.Rows64(p, obst, 3, devices=[0, 0, 0])}[how]
    got = {}
    for with_digest in (False, True):
        with make() as g:
            if how == "tiled":
                assert g.describe()["kernel"].startswith("lbm_tile_kernel_f64")
            g.set_cells(state)
            av = [g.run(3)]
            if with_digest:
                timed = g.last_run_kernel_ms() if how != "3 row blocks" else g.last_run_ms()
                first = g.digest()
                g.digest(1, 2)
                assert np.array_equal(g.digest()[0], first[0])
                assert (g.last_run_kernel_ms() if how != "3 row blocks" else g.last_run_ms()) == timed
            av.append(g.run(5))
            got[with_digest] = (np.concatenate(av), g.get_cells())
    assert got[True][0].shape == (8,) and np.all(got[True][0] > 0)
    assert np.array_equal(ref.bits(got[True][0]), ref.bits(got[False][0]))
    assert np.array_equal(ref.bits(got[True][1]), ref.bits(got[False][1]))


# ---- the CLI ------------------------------------------------------------------------------------------------------------------------
def test_cli_prints_the_digest(lbm, f64, digests, tmp_path):
    ppath, opath = deck_paths("rand_64x48", digests)
    p, obst = _deck(f64, digests, "rand_64x48")
    env = {k: v for k, v in os.environ.items() if not k.startswith("LBM")}
    printed = {}
    for tag, extra in (("whole", {}), ("rows", dict(LBM64_RANKS="3", LBM_DEVICES="0,0,0"))):
        cwd = tmp_path / tag
        cwd.mkdir()
        r = subprocess.run([lbm.CLI_PATH, ppath, opath], cwd=cwd, env={**env, "LBM_PRECISION": "double", "LBM_DIGEST": "1", **extra},
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        lines = [l for l in r.stderr.splitlines() if l.startswith("state digest: ")]
        assert len(lines) == 1 and re.fullmatch(r"state digest: [0-9a-f]{16}", lines[0]), r.stderr
        assert "state digest" not in r.stdout
        printed[tag] = lines[0]
    with f64.Grid64(p, obst) as g:
        g.run(p.max_iters)
        _, total = g.digest()
    assert printed["whole"] == printed["rows"] == f"state digest: {total:016x}"
    r = subprocess.run([lbm.CLI_PATH, ppath, opath], cwd=tmp_path, env={**env, "LBM_DIGEST": "1"}, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "LBM_DIGEST: the state digest is the double-precision mode's, it needs LBM_PRECISION=double" in r.stderr


# ---- two GPUs -----------------------------------------------------------------------------------------------------------------------
def test_one_gpu_per_rank(f64, digests):
    """Switches itself on where there are at least 2 GPUs: each rank then digests its rows on its own device, side by side."""
    import torch
    count = torch.cuda.device_count()
    if count < 2:
        pytest.skip(f"needs 2 GPUs, this box has {count}")
    p, obst = _deck(f64, digests, "rand_64x48")
    state = _random_state(p, seed=21)
    want, _ = _whole_run(f64, "rand_64x48/5", p, obst, state, 5)
    with f64.Rows64(p, obst, 2, devices=[0, 1]) as g:
        g.set_cells(state)
        g.run(5)
        assert np.array_equal(_check(f64, g, "devices 0 and 1"), want)
        assert np.array_equal(g.digest(20, 30)[0], want[20:30])
