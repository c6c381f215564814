"""Row-partitioned double-precision runs on the GPU (include/lbm_d2q9_f64_rows.h, csrc/lbm_rows64.hip) held to the CPU restatement
tests/f64_ref.c: populations bit for bit for every rank count, av_vels within the bound of the ranks' summation trees plus the host's
additions over the ranks, read-outs, the whole 128 x 128 deck against the results the reference shipped, the CLI.  All ranks run on
device 0 (ranks may share a device); one test switches itself on where there are two GPUs or more."""
import os
import subprocess

import numpy as np
import pytest

import f64_ref
from conftest import deck_paths

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
BLOCK = 256


@pytest.fixture(scope="module")
def f64(lbm):
    from mpilattice_boltzmann_amd import f64 as mod
    mod.load_rows_library()
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
    """tests/test_f64.py's: each population of the rest state times a factor from [0.8, 1.2) — positive, and it stays positive."""
    return f64_ref.initial_cells(p) * np.random.default_rng(seed).uniform(0.8, 1.2, (p.ny, p.nx, 9))


def sum_bound(desc):
    """Relative error of one av_vels entry against the exactly rounded sum times 1.0 / free_cells, from the launch shape
    lbm_rows64_describe reports.  Every term is non-negative and the same double on both sides, so each addition errs by at most 2^-53
    of its result, which is at most the total; the longest chain of additions a term goes through is that of tests/test_f64.py
    sum_bound on the rank with the most blocks, and one level more:
      cells_per_block / 256   serial additions in its lane,
      9                       block_sum: six butterfly levels of the wave, then the four waves' sums added serially,
      ceil(blocks / 256)      serial additions in a lane of the rank's fold block,
      9                       its block_sum,
      nranks - 1              the ranks' sums added on the host in rank order,
      2                       the product with 1.0 / free_cells, on this side and on the reference's."""
    return (desc["cells_per_block"] // BLOCK + 9 + -(-desc["blocks"] // BLOCK) + 9 + (desc["nranks"] - 1) + 2) * U


def _check_av(av, exact, obst, desc):
    ref = f64_ref.av_vels(exact, obst)
    assert av.shape == ref.shape
    err = float(np.max(np.abs(av - ref) / ref)) if np.all(ref > 0) else float(np.max(np.abs(av - ref)))
    print(f"  av_vels: {err / U:.2f} x 2^-53 against a bound of {sum_bound(desc) / U:.0f} x 2^-53 ({desc})")
    assert err <= sum_bound(desc)


_REFERENCES = {}


def _reference(key, p, obst):
    """The restatement's side of the parity protocol for one deck, computed once and shared by every rank count: never written to."""
    if key not in _REFERENCES:
        ref37, _, exact37 = f64_ref.run(p, obst, 37)
        state = _random_state(p)
        ref12, _, exact12 = f64_ref.run(p, obst, 12, cells0=state)
        for a in (ref37, exact37, state, ref12, exact12):
            a.setflags(write=False)
        _REFERENCES[key] = (ref37, exact37, state, ref12, exact12)
    return _REFERENCES[key]


def _parity(f64, key, p, obst, nranks, flags=0, expect_kernel=None, devices=None):
    """tests/test_f64.py's protocol.  From the rest state: 37 steps.  From a random positive state: run(5) then run(7) against 12 steps
    (an odd and an even number of steps; the accelerate that run(5) skipped on its last step is run(7)'s pre-pass, and run(7)'s first
    push sends the edge rows run(5) left)."""
    ref37, exact37, state, ref12, exact12 = _reference(key, p, obst)
    with f64.Rows64(p, obst, nranks, devices=devices if devices is not None else [0] * nranks, flags=flags) as g:
        desc = g.describe()
        assert desc["nranks"] == nranks
        if expect_kernel:
            assert desc["kernel"] == expect_kernel, desc
        av = g.run(37)
        assert np.array_equal(_bits(g.get_cells()), _bits(ref37)), f"{p.nx}x{p.ny} on {nranks} ranks, 37 steps from rest: {desc}"
        _check_av(av, exact37, obst, desc)
        g.set_cells(state)
        av = np.concatenate([g.run(5), g.run(7)])
        assert np.array_equal(_bits(g.get_cells()), _bits(ref12)), f"{p.nx}x{p.ny} on {nranks} ranks, run(5) + run(7) from a random state: {desc}"
        assert ref12.min() > 0.0                         # the premise of the bound: positive densities, non-negative terms
        _check_av(av, exact12, obst, desc)
    return desc


# the smallest shapes at which something can go wrong: (nx, ny, ranks, rows per rank)
SHAPES = [(1, 3, 1, [3]),                 # the rank is its own neighbour, one cell per lane
          (2, 6, 3, [2, 1, 3]),           # a one-row rank sends its row both ways; both x wraps fall on one lane
          (7, 5, 2, [2, 3]),              # odd nx
          (258, 33, 4, [9, 8, 8, 8]),     # several blocks per rank, a ragged last one
          (257, 33, 2, [17, 16])]


@pytest.mark.parametrize("nx,ny,nranks,rows", SHAPES)
def test_bit_parity_shapes(lbm, f64, nx, ny, nranks, rows):
    assert lbm.decompose(ny, nranks)[0] == rows
    p, obst = _synthetic(lbm, nx, ny)
    cells = 2 if nx % 2 == 0 else 1
    desc = _parity(f64, ("shape", nx, ny), p, obst, nranks, expect_kernel=f"lbm_rows_kernel_f64<{cells}>")
    assert desc["blocks"] == -(-(nx * max(rows) // cells) // BLOCK) and desc["cells_per_block"] == BLOCK * cells
    assert desc["state_bytes"] == 2 * 9 * 8 * nx * (ny + 2 * nranks)


# accelrow_blocked / strongaccel on 5 ranks: rows 4, 3, 3, 3, 3 — in the three-row last rank the accelerated row sits between two edge
# rows, one of which crosses the periodic seam to rank 0
DECKS = [("tiny_8x3", 1), ("accelrow_blocked_32x16", 2), ("accelrow_blocked_32x16", 5), ("strongaccel_32x16", 2), ("strongaccel_32x16", 5),
         ("rand_64x48", 2), ("rand_64x48", 3), ("rand_64x48", 8), ("wide_256x8", 2)]


@pytest.mark.parametrize("name,nranks", DECKS)
def test_bit_parity_decks(lbm, f64, digests, name, nranks):
    p, obst = _deck(f64, digests, name)
    assert p.nx % 2 == 0
    if name.endswith("32x16") and nranks == 5:
        assert lbm.decompose(p.ny, 5)[0] == [4, 3, 3, 3, 3]
    if name == "wide_256x8":
        assert lbm.decompose(p.ny, 2)[0] == [4, 4]
    _parity(f64, name, p, obst, nranks, expect_kernel="lbm_rows_kernel_f64<2>")


@pytest.mark.parametrize("flag,kernel", [("FLAG_NT_STORES", "lbm_rows_kernel_f64<2,nt>"), ("FLAG_NO_NT_STORES", "lbm_rows_kernel_f64<2>")])
def test_bit_parity_under_the_nt_flags(f64, digests, flag, kernel):
    p, obst = _deck(f64, digests, "rand_64x48")
    _parity(f64, "rand_64x48", p, obst, 2, flags=getattr(f64, flag), expect_kernel=kernel)


def test_populations_do_not_depend_on_the_rank_count(f64, digests):
    p, obst = _deck(f64, digests, "rand_64x48")
    state = _random_state(p, seed=21)
    with f64.Grid64(p, obst) as g:
        g.set_cells(state)
        g.run(12)
        want = _bits(g.get_cells())
    for nranks in (1, 2, 3, 8):
        with f64.Rows64(p, obst, nranks, devices=[0] * nranks) as g:
            g.set_cells(state)
            g.run(12)
            assert np.array_equal(_bits(g.get_cells()), want), nranks


def test_cells_round_trip_keeps_every_bit(lbm, f64):
    """get_cells(set_cells(x)) == x as bit patterns on 3 ranks (rows 2, 2, 3): NaNs with payloads, both zeros, denormals, infinities."""
    p, obst = _synthetic(lbm, 10, 7)
    state = _random_state(p)
    special = np.array([0x7FF8000000000001, 0xFFF4000000ABCDEF, 0x7FF0000000000001, 0x0000000000000000, 0x8000000000000000,
                        0x0000000000000001, 0x800FFFFFFFFFFFFF, 0x7FF0000000000000, 0xFFF0000000000000], np.uint64)
    flat = _bits(state).reshape(-1)
    flat[:special.size * 71:71] = special              # spread over the rows of all three ranks
    assert lbm.decompose(7, 3)[0] == [2, 2, 3] and special.size * 71 > 4 * 10 * 9
    with f64.Rows64(p, obst, 3, devices=[0, 0, 0]) as g:
        g.set_cells(state)
        assert np.array_equal(_bits(g.get_cells()), _bits(state))


def test_observables_velocity_sum_and_reynolds(lbm, f64, digests):
    """lbm_rows64_get_observables bit for bit against the numpy restatement of write_values' arithmetic; lbm_rows64_av_velocity_sum
    against the exactly rounded sum of av_velocity's terms, within the bound of ITS order of additions: on rank r of n_r cells and
    b_r = min(ceil(n_r / 256), 1024) blocks a lane adds ceil(n_r / (b_r * 256)) terms serially, block_sum's nine, then the host adds
    the ranks' b_r block sums serially, rank after rank; Rows64.reynolds sums on the host in the reference's cell order: Grid64's bits."""
    for (p, obst), nranks in ((_deck(f64, digests, "rand_64x48"), 3), (_synthetic(lbm, 257, 33), 2), (_synthetic(lbm, 700, 600, p_block=0.05), 1)):
        state = _random_state(p, seed=9)
        with f64.Rows64(p, obst, nranks, devices=[0] * nranks) as g:
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
        assert np.array_equal(_bits(obs), _bits(f64_ref.observables(cells))), (p.nx, p.ny)
        rank_cells = [rows * p.nx for rows in lbm.decompose(p.ny, nranks)[0]]
        blocks = [min(-(-n // BLOCK), 1024) for n in rank_cells]
        bound = (max(-(-n // (b * BLOCK)) for n, b in zip(rank_cells, blocks)) + 9 + sum(blocks)) * U
        exact = f64_ref.velocity_sum_exact(cells, obst)
        print(f"  {p.nx}x{p.ny} on {nranks} ranks, velocity sum: {abs(tot - exact) / exact / U:.2f} x 2^-53 against {bound / U:.0f} x 2^-53")
        assert abs(tot - exact) <= bound * exact
        assert re == f64_ref.reynolds(p, cells, obst)
        assert re == re_whole


def test_two_identical_runs_give_identical_av_vels(f64, digests):
    p, obst = _deck(f64, digests, "rand_64x48")
    state = _random_state(p, seed=3)
    got = []
    for _ in range(2):
        with f64.Rows64(p, obst, 3, devices=[0, 0, 0]) as g:
            g.set_cells(state)
            got.append((g.run(20), g.get_cells()))
    assert np.array_equal(_bits(got[0][0]), _bits(got[1][0])) and np.array_equal(_bits(got[0][1]), _bits(got[1][1]))
    assert np.all(got[0][0] > 0)


@pytest.fixture(scope="module")
def deck1024(f64, digests):
    """The 1024 x 1024 deck and 8 steps of the restatement on it, once."""
    p, obst = _deck(f64, digests, "1024x1024_t200")
    ref_cells, _, exact = f64_ref.run(p, obst, 8, nthreads=16)
    return p, obst, ref_cells, exact


def _run_1024(f64, deck1024, devices):
    p, obst, ref_cells, exact = deck1024
    with f64.Rows64(p, obst, len(devices), devices=devices) as g:
        desc = g.describe()
        av = g.run(8)
        cells = g.get_cells()
        ms, launches = g.last_run_ms()
    assert np.array_equal(_bits(cells), _bits(ref_cells)), desc
    _check_av(av, exact, obst, desc)
    assert launches == 8 * len(devices) and ms > 0.0


def test_bit_parity_1024x1024_deck_8_steps_on_8_ranks(f64, deck1024):
    _run_1024(f64, deck1024, [0] * 8)


def test_whole_128x128_deck_on_4_ranks_bits_and_shipped_results(lbm, f64):
    """40 000 steps on 4 ranks of 32 rows: 1.6 s on the device (40 us per step: on a grid this small the exchange is most of a step).
    The restatement's run is f64_ref.deck_run's, once per process (6 s where this test is the first to ask for it)."""
    p, obst, ref_cells, serial, exact = f64_ref.deck_run("128x128")
    p64 = f64.read_params64(os.path.join(f64_ref.GOLDEN, "decks", "input_128x128.params"))
    assert (p64.density, p64.accel, p64.omega) == (p.density, p.accel, p.omega)
    with f64.Rows64(p64, obst, 4, devices=[0] * 4) as g:
        desc = g.describe()
        av = g.run(p64.max_iters)
        cells = g.get_cells()
        obs = g.get_observables()
        re = g.reynolds()
    assert np.array_equal(_bits(cells), _bits(ref_cells)), "populations after 40 000 steps"
    _check_av(av, exact, obst, desc)
    # against what the reference shipped: the CPU test's limit (twice the restatement's own distance) plus the summation bound
    golden_av = f64_ref.golden_av_vels("128x128")
    av_rel = float(np.max(np.abs(av - golden_av) / np.abs(golden_av)))
    values = obs.copy()
    values[obst != 0] = (0.0, 0.0, 0.0, p.density * (1.0 / 3.0))
    fs_abs = float(np.max(np.abs(values.reshape(-1, 4) - f64_ref.golden_final_state("128x128"))))
    pub = float(f64_ref.published()["reynolds"]["128x128"]["value"])
    print(f"  4 ranks, 128x128: av_vels {av_rel:.3e} rel, final_state {fs_abs:.3e} abs, Reynolds {re!r}")
    assert av_rel <= f64_ref.AV_VELS_LIMIT + sum_bound(desc)
    assert fs_abs <= f64_ref.FINAL_STATE_LIMIT
    assert abs(re - pub) / pub <= f64_ref.REYNOLDS_LIMIT


def test_cli_row_blocks(lbm, f64, digests, tmp_path):
    """LBM_PRECISION=double LBM64_RANKS=3 bin/d2q9-bgk on rand_64x48: final_state.dat and the Reynolds line are those of
    LBM_PRECISION=double alone; av_vels.dat within the bound of three ranks' sums plus its 13 printed digits."""
    ppath, opath = deck_paths("rand_64x48", digests)
    p, obst = _deck(f64, digests, "rand_64x48")
    env = {k: v for k, v in os.environ.items() if not k.startswith("LBM")}
    env["LBM_PRECISION"] = "double"
    out = {}
    for tag, extra in (("whole", {}), ("rows", dict(LBM64_RANKS="3", LBM_DEVICES="0,0,0", LBM_DESCRIBE="1"))):
        cwd = tmp_path / tag
        cwd.mkdir()
        r = subprocess.run([lbm.CLI_PATH, ppath, opath], cwd=cwd, env={**env, **extra}, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        out[tag] = (r.stdout.splitlines(), (cwd / "final_state.dat").read_bytes(), (cwd / "av_vels.dat").read_text(), r.stderr)
    lines = out["rows"][0]
    assert lines[0] == "==done==" and lines[1].startswith("Reynolds number:\t\t") and lines[2].startswith("Elapsed time:\t\t\t")
    assert lines[3].startswith("Elapsed user CPU time:\t\t") and lines[4].startswith("Elapsed system CPU time:\t")
    assert lines[5].startswith("MLUPS:\t\t\t\t") and lines[5].endswith("(3 ranks, double precision)")
    assert lines[1] == out["whole"][0][1]
    assert out["rows"][1] == out["whole"][1]
    assert f"kernel: lbm_rows_kernel_f64<2> on 3 ranks, {3 * p.max_iters} launches" in out["rows"][3]
    _, _, exact = f64_ref.run(p, obst, p.max_iters)
    ref = f64_ref.av_vels(exact, obst)
    av_lines = out["rows"][2].splitlines()
    assert [l.split(":")[0] for l in av_lines] == [str(t) for t in range(p.max_iters)]
    av = np.array([float(l.split("\t")[1]) for l in av_lines])
    with f64.Rows64(p, obst, 3, devices=[0, 0, 0]) as g:
        desc = g.describe()
    err = float(np.max(np.abs(av - ref) / ref))
    print(f"  av_vels.dat: {err:.3e} relative against {sum_bound(desc) + 2e-12:.3e}")
    assert err <= sum_bound(desc) + 2e-12               # %.12E: 13 significant digits, half a unit of the last is 5e-13 relative at most


def test_one_gpu_per_rank(f64, digests, deck1024):
    """Switches itself on where there are at least 2 GPUs: the edge rows then travel as stores over a real link.  The rand_64x48 parity
    on devices 0 and 1, and the 1024 x 1024 deck's 8 steps on one rank per device, 8 at most."""
    import torch
    count = torch.cuda.device_count()
    if count < 2:
        pytest.skip(f"needs 2 GPUs, this box has {count}")
    p, obst = _deck(f64, digests, "rand_64x48")
    _parity(f64, "rand_64x48", p, obst, 2, devices=[0, 1], expect_kernel="lbm_rows_kernel_f64<2>")
    _run_1024(f64, deck1024, list(range(min(count, 8))))
