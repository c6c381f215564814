"""The double-precision mode on the GPU (include/lbm_d2q9_f64.h, csrc/lbm_f64.hip) held to its CPU restatement tests/f64_ref.c:
populations bit for bit, av_vels within the bound of the launch's summation tree, read-outs, the whole 128 x 128 deck against the
results the reference shipped, the CLI, and a grid whose planes pass 4 GiB."""
import os
import subprocess

import numpy as np
import pytest

import f64_ref
from conftest import deck_paths

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
BLOCK = 256
MAXBLOCKS = 16384        # LBM_TUNE_MAXBLOCKS: the most work blocks of a step launch; beyond 16384 * 256 units a block strides over 2, 4, ... chunks


@pytest.fixture(scope="module")
def f64(lbm):
    from mpilattice_boltzmann_amd import f64 as mod
    mod.load_library()
    return mod


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _synthetic(lbm, nx, ny, density=0.1, accel=0.005, omega=1.85, p_block=0.2, seed=11):
    p = lbm.Params(nx=nx, ny=ny, max_iters=10, reynolds_dim=10, density=density, accel=accel, omega=omega)
    obst = lbm.synthetic_obstacles(nx, ny, p=p_block, seed=seed, walls=False)
    obst.flat[obst.size // 2] = 0                      # at least one free cell
    return p, obst


def _deck(f64, digests, name):
    ppath, opath = deck_paths(name, digests)
    p = f64.read_params64(ppath)
    return p, f64_ref.read_obstacles(opath, p.nx, p.ny)


def _random_state(p, seed=7):
    """A random positive state that stays one: each population of the rest state times a factor from [0.8, 1.2).  (Nine unrelated values
    per cell are positive too, but at omega = 1.85 such a state diverges within a few steps; densities turn negative, and with them the
    sum|u| terms, whose sum then cancels: the bound below is for non-negative terms.)"""
    return f64_ref.initial_cells(p) * np.random.default_rng(seed).uniform(0.8, 1.2, (p.ny, p.nx, 9))


def sum_bound(desc):
    """Relative error of one av_vels entry against the exactly rounded sum times 1.0 / free_cells, from the launch shape lbm64_describe
    reports.  Every term is non-negative and the same double on both sides, so each addition errs by at most 2^-53 of its result, which
    is at most the total; the longest chain of additions a term goes through:
      cells_per_block / 256   serial additions in its lane (a pair's two terms, then one addition per unit of the lane),
      9                       block_sum: six butterfly levels of the wave, then the four waves' sums added serially,
      ceil(blocks / 256)      serial additions in a lane of the fold block (block 0 of the next launch, or the last fold),
      9                       its block_sum,
      2                       the product with 1.0 / free_cells, on this side and on the reference's."""
    return (desc["cells_per_block"] // BLOCK + 9 + -(-desc["blocks"] // BLOCK) + 9 + 2) * U


def _check_av(av, exact, obst, desc):
    ref = f64_ref.av_vels(exact, obst)
    assert av.shape == ref.shape
    err = float(np.max(np.abs(av - ref) / ref)) if np.all(ref > 0) else float(np.max(np.abs(av - ref)))
    print(f"  av_vels: {err / U:.2f} x 2^-53 against a bound of {sum_bound(desc) / U:.0f} x 2^-53 ({desc})")
    assert err <= sum_bound(desc)


PAIR_DECKS = ["tiny_8x3", "accelrow_blocked_32x16", "strongaccel_32x16", "walls_40x24", "dense_32x32", "rand_64x48", "wide_256x8"]
PAIR_SHAPES = [(2, 3), (258, 33)]          # 258 x 33: more than one block (4257 pairs), a ragged last one
SINGLE_SHAPES = [(1, 3), (7, 5), (257, 33)]


def _parity(f64, p, obst, flags=0, expect_kernel=None):
    """From the rest state: 37 steps.  From a random positive state: run(5) then run(7) against 12 steps (an odd and an even number
    of launches; the accelerate that run(5) skipped on its last step is run(7)'s pre-pass)."""
    with f64.Grid64(p, obst, flags=flags) as g:
        desc = g.describe()
        if expect_kernel:
            assert desc["kernel"] == expect_kernel, desc
        av = g.run(37)
        ref_cells, _, exact = f64_ref.run(p, obst, 37)
        assert np.array_equal(_bits(g.get_cells()), _bits(ref_cells)), f"{p.nx}x{p.ny} 37 steps from rest: {desc}"
        _check_av(av, exact, obst, desc)
        state = _random_state(p)
        g.set_cells(state)
        av = np.concatenate([g.run(5), g.run(7)])
        ref_cells, _, exact = f64_ref.run(p, obst, 12, cells0=state)
        assert np.array_equal(_bits(g.get_cells()), _bits(ref_cells)), f"{p.nx}x{p.ny} run(5) + run(7) from a random state: {desc}"
        assert ref_cells.min() > 0.0                     # the premise of the bound: positive densities, non-negative terms
        _check_av(av, exact, obst, desc)
    return desc


@pytest.mark.parametrize("name", PAIR_DECKS)
def test_bit_parity_pair_form_decks(f64, digests, name):
    p, obst = _deck(f64, digests, name)
    assert p.nx % 2 == 0
    _parity(f64, p, obst, expect_kernel="lbm_step_kernel_f64<2>")


@pytest.mark.parametrize("nx,ny", PAIR_SHAPES)
def test_bit_parity_pair_form_shapes(lbm, f64, nx, ny):
    p, obst = _synthetic(lbm, nx, ny)
    desc = _parity(f64, p, obst, expect_kernel="lbm_step_kernel_f64<2>")
    assert desc["blocks"] == -(-(nx * ny // 2) // BLOCK)


@pytest.mark.parametrize("nx,ny", SINGLE_SHAPES)
def test_bit_parity_single_form(lbm, f64, nx, ny):
    p, obst = _synthetic(lbm, nx, ny)
    _parity(f64, p, obst, expect_kernel="lbm_step_kernel_f64<1>")


@pytest.mark.parametrize("flag,kernel", [("FLAG_NT_STORES", "lbm_step_kernel_f64<2,nt>"), ("FLAG_NO_NT_STORES", "lbm_step_kernel_f64<2>")])
def test_bit_parity_under_the_nt_flags(f64, digests, flag, kernel):
    p, obst = _deck(f64, digests, "rand_64x48")
    _parity(f64, p, obst, flags=getattr(f64, flag), expect_kernel=kernel)


def test_other_flags_are_refused(lbm, f64, digests):
    p, obst = _deck(f64, digests, "tiny_8x3")
    for flags in (lbm._capi.FLAG_FUSED_ARITH, lbm._capi.FLAG_GRAPH, lbm._capi.FLAG_FORCE_HALO, 1 | 64):
        with pytest.raises(lbm.LbmError, match="LBM_FLAG_NT_STORES"):
            f64.Grid64(p, obst, flags=flags)


@pytest.mark.parametrize("nx,ny,maxblocks", [(258, 33, 3), (257, 33, 5), (64, 48, 1)])
def test_stride_loop_with_a_lowered_block_cap(lbm, f64, monkeypatch, nx, ny, maxblocks):
    """LBM_TUNE_MAXBLOCKS lowered (the context reads it when it is made): every block strides over several 256-unit chunks, the last
    chunk ragged, on shapes small enough to check all of it."""
    monkeypatch.setenv("LBM_TUNE_MAXBLOCKS", str(maxblocks))
    p, obst = _synthetic(lbm, nx, ny, seed=3)
    desc = _parity(f64, p, obst)
    assert desc["cells_per_block"] > BLOCK * 2 and desc["blocks"] * desc["cells_per_block"] >= nx * ny


def test_stride_loop_beyond_the_default_block_cap(lbm, f64):
    """4096 x 2050: 4 198 400 x-pairs, more than MAXBLOCKS * 256 = 4 194 304, so a block takes two chunks and the launch has 8200 blocks.
    3 steps from a state that differs from cell to cell."""
    nx, ny = 4096, 2050
    p, obst = _synthetic(lbm, nx, ny, p_block=0.02, seed=5)
    assert nx * ny // 2 > MAXBLOCKS * BLOCK
    y, x = np.arange(ny, dtype=np.float64)[:, None, None], np.arange(nx, dtype=np.float64)[None, :, None]
    state = f64_ref.initial_cells(p)[0, 0][None, None, :] * (1.0 + 0.05 * np.sin(0.37 * x + 0.11 * y) + 0.01 * np.arange(9)[None, None, :])
    with f64.Grid64(p, obst) as g:
        desc = g.describe()
        assert desc["kernel"] == "lbm_step_kernel_f64<2,nt>" and desc["cells_per_block"] == 2 * 2 * BLOCK and desc["blocks"] == 8200, desc
        g.set_cells(state)
        av = g.run(3)
        cells = g.get_cells()
    ref_cells, _, exact = f64_ref.run(p, obst, 3, cells0=state, nthreads=16)
    assert np.array_equal(_bits(cells), _bits(ref_cells))
    _check_av(av, exact, obst, desc)


def test_bit_parity_1024x1024_deck_8_steps(f64, digests):
    p, obst = _deck(f64, digests, "1024x1024_t200")
    with f64.Grid64(p, obst) as g:
        desc = g.describe()
        av = g.run(8)
        cells = g.get_cells()
    ref_cells, _, exact = f64_ref.run(p, obst, 8, nthreads=16)
    assert np.array_equal(_bits(cells), _bits(ref_cells)), desc
    _check_av(av, exact, obst, desc)


def test_cells_round_trip_keeps_every_bit(lbm, f64):
    """get_cells(set_cells(x)) == x as bit patterns: NaNs with payloads, both zeros, denormals, infinities."""
    p, obst = _synthetic(lbm, 10, 7)
    state = _random_state(p)
    special = np.array([0x7FF8000000000001, 0xFFF4000000ABCDEF, 0x7FF0000000000001, 0x0000000000000000, 0x8000000000000000,
                        0x0000000000000001, 0x800FFFFFFFFFFFFF, 0x7FF0000000000000, 0xFFF0000000000000], np.uint64)
    _bits(state).reshape(-1)[:special.size * 5:5] = special
    with f64.Grid64(p, obst) as g:
        g.set_cells(state)
        assert np.array_equal(_bits(g.get_cells()), _bits(state))


def test_observables_and_velocity_sum(lbm, f64, digests):
    """lbm64_get_observables bit for bit against the numpy restatement of write_values' arithmetic; lbm64_av_velocity_sum against the
    exactly rounded sum of av_velocity's terms, within the bound of ITS order of additions (kernels/step64.h: a lane adds
    ceil(n / (blocks * 256)) terms serially, block_sum's nine, then the host adds the min(ceil(n / 256), 1024) block sums serially)."""
    for p, obst in (_deck(f64, digests, "rand_64x48"), _synthetic(lbm, 257, 33), _synthetic(lbm, 700, 600, p_block=0.05)):
        with f64.Grid64(p, obst) as g:
            g.set_cells(_random_state(p, seed=9))
            g.run(3)
            cells = g.get_cells()
            obs = g.get_observables()
            tot = g.av_velocity_sum()
            re = g.reynolds()
        assert np.array_equal(_bits(obs), _bits(f64_ref.observables(cells))), (p.nx, p.ny)
        n = p.nx * p.ny
        blocks = min(-(-n // BLOCK), 1024)
        bound = (-(-n // (blocks * BLOCK)) + 9 + blocks) * U
        exact = f64_ref.velocity_sum_exact(cells, obst)
        print(f"  {p.nx}x{p.ny} velocity sum: {abs(tot - exact) / exact / U:.2f} x 2^-53 against {bound / U:.0f} x 2^-53")
        assert abs(tot - exact) <= bound * exact
        assert re == f64_ref.reynolds(p, cells, obst)        # Grid64.reynolds sums on the host in the reference's cell order: the same bits


@pytest.fixture(scope="module")
def deck128_device(f64):
    """The whole 128 x 128 deck on the device, once."""
    p, obst, ref_cells, serial, exact = f64_ref.deck_run("128x128")
    p64 = f64.read_params64(os.path.join(f64_ref.GOLDEN, "decks", "input_128x128.params"))
    assert (p64.density, p64.accel, p64.omega) == (p.density, p.accel, p.omega)
    with f64.Grid64(p64, obst) as g:
        desc = g.describe()
        av = g.run(p64.max_iters)
        cells = g.get_cells()
        obs = g.get_observables()
        re = g.reynolds()
    return dict(p=p64, obst=obst, desc=desc, av=av, cells=cells, obs=obs, re=re)


def test_whole_128x128_deck_bits_and_shipped_results(lbm, f64, deck128_device, tmp_path):
    d = deck128_device
    p, obst, ref_cells, serial, exact = f64_ref.deck_run("128x128")
    assert np.array_equal(_bits(d["cells"]), _bits(ref_cells)), "populations after 40 000 steps"
    _check_av(d["av"], exact, obst, d["desc"])
    # against what the reference shipped: the CPU test's limit (twice the restatement's own distance) plus the summation bound
    golden_av = f64_ref.golden_av_vels("128x128")
    av_rel = float(np.max(np.abs(d["av"] - golden_av) / np.abs(golden_av)))
    values = d["obs"].copy()
    values[obst != 0] = (0.0, 0.0, 0.0, p.density * (1.0 / 3.0))
    fs_abs = float(np.max(np.abs(values.reshape(-1, 4) - f64_ref.golden_final_state("128x128"))))
    pub = float(f64_ref.published()["reynolds"]["128x128"]["value"])
    print(f"  device, 128x128: av_vels {av_rel:.3e} rel, final_state {fs_abs:.3e} abs, Reynolds {d['re']!r}")
    assert av_rel <= f64_ref.AV_VELS_LIMIT + sum_bound(d["desc"])
    assert fs_abs <= f64_ref.FINAL_STATE_LIMIT          # the populations are the restatement's bits: no summation in these columns
    assert abs(d["re"] - pub) / pub <= f64_ref.REYNOLDS_LIMIT
    # check.py's rule on the files the mode writes
    fs_path, av_path = str(tmp_path / "final_state.dat"), str(tmp_path / "av_vels.dat")
    f64.write_final_state_obs64(fs_path, d["p"], d["obs"], obst)
    f64.write_av_vels64(av_path, d["av"])
    check = os.path.join(f64_ref.GOLDEN, "check")
    rep = lbm.checker.check_files(os.path.join(check, "128x128.av_vels.dat.gz"), os.path.join(check, "128x128.final_state.dat.gz"), av_path, fs_path)
    assert rep.ok, rep.message
    assert open(fs_path).read() == f64_ref.final_state_text(p, ref_cells, obst)


def test_cli_double_precision(lbm, f64, tmp_path):
    """LBM_PRECISION=double bin/d2q9-bgk on the 128 x 128 deck: final_state.dat byte-identical to the restatement's, the Reynolds line
    within the CPU limit of the published value; with LBM_GPUS=2 it refuses."""
    p, obst, ref_cells, serial, exact = f64_ref.deck_run("128x128")
    decks = os.path.join(f64_ref.GOLDEN, "decks")
    cmd = [lbm.CLI_PATH, os.path.join(decks, "input_128x128.params"), os.path.join(decks, "obstacles_128x128.dat")]
    env = {k: v for k, v in os.environ.items() if not k.startswith("LBM_")}
    env["LBM_PRECISION"] = "double"
    r = subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert lines[0] == "==done==" and lines[1].startswith("Reynolds number:\t\t") and lines[2].startswith("Elapsed time:\t\t\t")
    assert lines[3].startswith("Elapsed user CPU time:\t\t") and lines[4].startswith("Elapsed system CPU time:\t")
    re = float(lines[1].split("\t")[-1])
    pub = float(f64_ref.published()["reynolds"]["128x128"]["value"])
    assert abs(re - pub) / pub <= f64_ref.REYNOLDS_LIMIT
    assert lines[1].split("\t")[-1] == "%.12E" % f64_ref.reynolds(p, ref_cells, obst)
    assert (tmp_path / "final_state.dat").read_text() == f64_ref.final_state_text(p, ref_cells, obst)
    av_lines = (tmp_path / "av_vels.dat").read_text().splitlines()
    assert len(av_lines) == p.max_iters and av_lines[0].startswith("0:\t") and av_lines[-1].startswith(f"{p.max_iters - 1}:\t")
    env["LBM_GPUS"] = "2"
    r = subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "double precision runs on one GPU" in r.stderr


BIG = (8192, 7296)       # the smallest shape of whole 32 x 16 tiles whose ninth plane lies beyond 4 GiB


def big_grid_case(lbm, steps):
    """The deck and the state of the tests beyond 4 GiB (here and in tests/test_f64_multi.py): 0.5 % obstacles inside walls, and a state
    that differs from cell to cell, made in place: rest * (1 + a small separable pattern)."""
    nx, ny = BIG
    p = lbm.Params(nx=nx, ny=ny, max_iters=steps, reynolds_dim=10, density=0.1, accel=0.005, omega=1.85)
    assert 9 * nx * ny * 8 > 1 << 32
    obst = lbm.synthetic_obstacles(nx, ny, p=0.005, seed=42, walls=True)
    cells = f64_ref.initial_cells(p)
    cells *= (1.0 + 0.03 * np.sin(0.013 * np.arange(ny)))[:, None, None]
    cells *= (1.0 + 0.03 * np.cos(0.007 * np.arange(nx)))[None, :, None]
    return p, obst, cells


def big_grid_compare(p, obst, cells, got, steps):
    """`steps` steps of the restatement on `cells`, IN PLACE, then the bits by row blocks (no whole-grid temporaries).  Returns exact."""
    exact = np.zeros(steps)
    rc = f64_ref.lib().f64_ref_run(p.nx, p.ny, p.density, p.accel, p.omega, obst.ctypes.data_as(f64_ref.C.POINTER(f64_ref.C.c_int)), f64_ref._dp(cells),
                                   steps, 16, None, f64_ref._dp(exact))
    assert rc == 0
    for y0 in range(0, p.ny, 512):
        assert np.array_equal(_bits(got[y0:y0 + 512]), _bits(cells[y0:y0 + 512])), f"rows {y0}..{y0 + 511}"
    return exact


def test_bit_parity_8192x7296_planes_beyond_4_gib(lbm, f64):
    """8192 x 7296, 2 steps: a plane is 478 MB and the nine planes 4.3 GB, so a 32-bit byte offset anywhere in the step kernel, the
    copies or the read-outs shows.  Needs about 13 GB of host memory and is host-bound (about 10 s): one of the two tests above a few
    seconds (the other: tests/test_f64_multi.py, the same grid under the multi-step kernel)."""
    nx, ny = BIG
    p, obst, cells = big_grid_case(lbm, 2)
    with f64.Grid64(p, obst) as g:
        desc = g.describe()
        assert desc["state_bytes"] == 2 * 9 * nx * ny * 8 and desc["kernel"] == "lbm_step_kernel_f64<2,nt>"
        g.set_cells(cells)
        av = g.run(2)
        got = g.get_cells()
    exact = big_grid_compare(p, obst, cells, got, 2)
    _check_av(av, exact, obst, desc)
