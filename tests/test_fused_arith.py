"""GPU suite of the fused arithmetic (LBM_FLAG_FUSED_ARITH): every kernel family a context can run must give the bits of the host
restatement tests/fused_ref.c (pinned and measured by tests/test_fused_ref.py) — populations bit for bit, per-step sums to 1e-12
relative (the device adds the same double terms in another order; lbm_multi_kernel forms them as compensated float sums of relative
error ~2^-44 = 6e-14).  Each case asserts through lbm_describe's kernel name that the intended family ran.  A library that ignores
the flag returns the exact arithmetic's bits and fails every comparison here.

Shapes: the smallest that reach each family by lbm_create's rules: lbm_tile_kernel up to 131 072 cells on edges
that are multiples of 16; lbm_multi_kernel<3> below 768 x 768 cells, <4> from there, on 64 x 24 tiles from 2^20 cells; the one-step
kernels where nx is below 128 and no multiple of 64 — one cell per lane up to 65 536 cells or where 4 does not divide nx
(lbm_step_kernel_narrow), four above (lbm_step_kernel: 100 x 700; a 128 x 64 grid is below that threshold, with or without
LBM_FLAG_ONE_STEP) — and in the one-step loops of a partition (LBM_FLAG_ONE_STEP, the RCCL case below).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import fused_ref
from conftest import GOLDEN, ROOT, deck_paths

pytestmark = pytest.mark.gpu

SUMS_RTOL = 1e-12


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def shipped(oracle, digests, name):
    ppath, opath = deck_paths(name, digests)
    p = oracle.read_params(ppath)
    obst, _ = oracle.read_obstacles(opath, p.nx, p.ny)
    return p, obst


def synthetic(lbm, nx, ny, steps, seed=3, block_accel_row=False):
    p = lbm.Params(nx=nx, ny=ny, max_iters=steps, reynolds_dim=10, density=0.1, accel=0.005, omega=1.85)
    obst = lbm.synthetic_obstacles(nx, ny, p=0.02, seed=seed, walls=True)
    if block_accel_row:
        obst[ny - 2, 5:11] = 1
        obst[ny - 2, nx // 2] = 1
    return p, obst


def fused_context(lbm, p, obst, flags=0):
    return lbm.Partition(p, lbm.count_free_cells(obst), obst, flags=flags | lbm._capi.FLAG_FUSED_ARITH)


def assert_equals_restatement(part, p, obst, runs, ref=None):
    """`runs` calls of lbm_run on `part`; populations and per-step sums against fused_ref (or `ref` = its (cells, sums))."""
    sums = []
    for n in runs:
        part.run(n)
        sums.append(part.step_collect(n))
    sums = np.concatenate(sums)
    ref_cells, ref_sums = fused_ref.run(p, obst, sum(runs), mode="fused") if ref is None else ref
    rel = float(np.max(np.abs(sums - ref_sums) / ref_sums))
    differing = int(np.count_nonzero(bits(part.get_cells()) != bits(ref_cells)))
    print(f"{part.describe()['kernel']}: {differing} differing population words, per-step sums off by {rel:.3e}")
    assert differing == 0
    assert rel < SUMS_RTOL


FAMILIES = [   # id, deck, steps, kernel name prefix
    ("tile_kernel", ("shipped", "128x128"), 37, "lbm_tile_kernel_fused<"),                       # a multiple of 8 plus a tail
    ("multi3_64x16", ("synthetic", 512, 384), 10, "lbm_multi_kernel<3, 6> (fused arithmetic)"),      # 3 + 3 + 4
    ("multi4_64x13", ("synthetic", 1024, 640), 11, "lbm_multi_kernel<4, 6> (fused arithmetic)"),     # 4 + 4 + 3
    ("multi4_tall", ("shipped", "1024x1024"), 11, "lbm_multi_kernel<4, 6> (fused arithmetic)"),
    ("multi_nx_130", ("synthetic", 130, 1024), 8, "lbm_multi_kernel<3, 6> (fused arithmetic)"),      # nx no multiple of 64
    ("step_narrow", ("synthetic", 126, 40), 5, "lbm_step_kernel_narrow_fused<"),
    ("step_quad", ("synthetic", 100, 700), 5, "lbm_step_kernel_fused<"),
]


@pytest.mark.parametrize("case", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_every_kernel_family_gives_the_restatement_bits(lbm, oracle, digests, case):
    _, deck, steps, kernel = case
    if deck[0] == "shipped":
        p, obst = shipped(oracle, digests, deck[1])
    else:
        p, obst = synthetic(lbm, deck[1], deck[2], steps, block_accel_row=deck[1] in (512, 126))
    part = fused_context(lbm, p, obst)
    d = part.describe()
    assert d["kernel"].startswith(kernel) and d["fused_arith"], d
    assert_equals_restatement(part, p, obst, [steps])
    part.close()


# ---- every row of the library's kernel tables that no case above launches --------------------------------------------------------
# lbm_tile_kernel: one row per (geometry, full-H launch or shorter, form of the terms).  A 32 x 32 grid is the smallest that all four
# geometries tile into more than one block; geometry 88 is the default of the 128 x 128 cases.  Runs of 11 then 5 steps: launches of
# 8 + 3, then 5 steps at H = 8 and of 4 + 4 + 3, then 4 + 1 at H = 4 — a full-H launch and a shorter one each.
TILE_GEOMS = ["168", "164", "84"]
AV_EXACT_RTOL = 1e-6      # av_vels against the oracle's exact per-step sums, as tests/test_gpu_parity.py holds LBM_FLAG_FAST_AVVELS to


@pytest.fixture(scope="module")
def tile_deck(lbm, oracle):
    """The 32 x 32 deck with both references for 16 steps, computed once: (p, obst, fused_ref's (cells, sums), the oracle's (cells, exact av_vels))."""
    p, obst = synthetic(lbm, 32, 32, 16, block_accel_row=True)
    ref_cells, _, ref_exact = oracle.run(p, obst, 16)
    return p, obst, fused_ref.run(p, obst, 16, mode="fused"), (ref_cells, ref_exact)


@pytest.mark.parametrize("geom", TILE_GEOMS)
def test_tile_geometries_with_the_fused_arithmetic(lbm, tile_deck, monkeypatch, geom):
    monkeypatch.setenv("LBM_TUNE_TILE_GEOM", geom)     # T*10 + H: owned tile edge, ghost ring / steps per launch
    p, obst, ref, _ = tile_deck
    part = fused_context(lbm, p, obst)
    assert part.describe()["kernel"] == f"lbm_tile_kernel_fused<{int(geom) // 10}, {int(geom) % 10}>"
    assert_equals_restatement(part, p, obst, [11, 5], ref=ref)
    part.close()


@pytest.mark.parametrize("geom", TILE_GEOMS)
def test_tile_geometries_with_float_av_vels_terms(lbm, tile_deck, monkeypatch, geom):
    """LBM_FLAG_FAST_AVVELS on the same grid and geometries: the exact arithmetic's populations bit for bit, av_vels to 1e-6."""
    monkeypatch.setenv("LBM_TUNE_TILE_GEOM", geom)
    p, obst, _, (ref_cells, ref_exact) = tile_deck
    sim = lbm.Simulation(p, obst, flags=lbm._capi.FLAG_FAST_AVVELS)
    assert sim.partition.describe()["kernel"] == f"lbm_tile_kernel<{int(geom) // 10}, {int(geom) % 10}, fast av_vels>"
    av = np.concatenate([sim.run(11), sim.run(5)])
    cells = sim.local_cells()
    sim.close()
    rel = float(np.max(np.abs(av - ref_exact) / ref_exact))
    differing = int(np.count_nonzero(bits(cells) != bits(ref_cells)))
    print(f"geometry {geom}: {differing} differing population words, av_vels off by {rel:.3e}")
    assert differing == 0
    assert rel < AV_EXACT_RTOL


# The one-step kernels with non-temporal stores (LBM_FLAG_NT_STORES; by default only grids beyond the Infinity Cache take them): one
# cell per lane at 126 x 40, four at 100 x 700, in both arithmetics.
NT_SHAPES = [("narrow", 126, 40, "lbm_step_kernel_narrow"), ("quad", 100, 700, "lbm_step_kernel")]


@pytest.mark.parametrize("shape", NT_SHAPES, ids=[s[0] for s in NT_SHAPES])
def test_non_temporal_one_step_kernels_in_both_arithmetics(lbm, oracle, shape):
    _, nx, ny, family = shape
    p, obst = synthetic(lbm, nx, ny, 5, block_accel_row=True)
    exact = lbm.Partition(p, lbm.count_free_cells(obst), obst, flags=lbm._capi.FLAG_NT_STORES)
    assert exact.describe()["kernel"] == f"{family}<true>"
    exact.run(5)
    ref_cells, _, _ = oracle.run(p, obst, 5)
    differing = int(np.count_nonzero(bits(exact.get_cells()) != bits(ref_cells)))
    print(f"{family}<true>: {differing} population words differ from the oracle's")
    assert differing == 0
    exact.close()
    fused = fused_context(lbm, p, obst, flags=lbm._capi.FLAG_NT_STORES)
    assert fused.describe()["kernel"] == f"{family}_fused<true>"
    assert_equals_restatement(fused, p, obst, [5])
    fused.close()


def test_set_cells_of_a_random_state_then_four_fused_steps(lbm):
    rng = np.random.default_rng(11)
    p, obst = synthetic(lbm, 256, 128, 4, seed=9, block_accel_row=True)
    cells0 = (rng.random((128, 256, 9), dtype=np.float32) * 0.02 + 0.004).astype(np.float32)
    part = fused_context(lbm, p, obst)
    part.set_cells(cells0)
    assert_equals_restatement(part, p, obst, [4], ref=fused_ref.run(p, obst, 4, mode="fused", cells0=cells0))
    part.close()


def test_a_run_split_over_two_calls_equals_one(lbm):
    p, obst = synthetic(lbm, 512, 384, 11, block_accel_row=True)
    ref = fused_ref.run(p, obst, 11, mode="fused")
    for runs in ([11], [5, 6]):
        part = fused_context(lbm, p, obst)
        assert_equals_restatement(part, p, obst, runs, ref=ref)
        part.close()


def test_graph_replay_of_the_fused_one_step_kernel(lbm):
    """LBM_FLAG_GRAPH with the flag (an accepted combination): lbm_run replays a captured block of 64 one-step launches; 70 steps =
    one direct launch, one replay, five direct launches.  The captured launches must be the fused ones."""
    p, obst = synthetic(lbm, 126, 40, 70, block_accel_row=True)
    part = fused_context(lbm, p, obst, flags=lbm._capi.FLAG_GRAPH)
    assert part.describe()["kernel"].startswith("lbm_step_kernel_narrow_fused<")
    assert_equals_restatement(part, p, obst, [70])
    part.close()


def test_a_default_context_still_equals_the_oracle(lbm, oracle):
    """Flag hygiene: without the flag nothing moved (same deck as the K = 3 family above), and the two arithmetics do differ on it."""
    p, obst = synthetic(lbm, 512, 384, 10, block_accel_row=True)
    part = lbm.Partition(p, lbm.count_free_cells(obst), obst)
    d = part.describe()
    assert d["kernel"] == "lbm_multi_kernel<3>" and d["fused_arith"] is False
    part.run(10)
    ref_cells, _, _ = oracle.run(p, obst, 10, nthreads=4)
    assert np.array_equal(bits(part.get_cells()), bits(ref_cells))
    part.close()
    fused_cells, _ = fused_ref.run(p, obst, 10, mode="fused")
    assert not np.array_equal(bits(fused_cells), bits(ref_cells))


@pytest.mark.parametrize("other", ["FLAG_FAST_AVVELS", "FLAG_EXACT_AVVELS"])
def test_refused_flag_combinations(lbm, other):
    p, obst = synthetic(lbm, 128, 128, 4)
    with pytest.raises(lbm.LbmError, match="LBM_FLAG_FUSED_ARITH cannot be combined"):
        fused_context(lbm, p, obst, flags=getattr(lbm._capi, other))


@pytest.mark.parametrize("one_step", [False, True], ids=["k_step_loop", "one_step_loop"])
def test_rccl_loop_as_a_ring_of_one_rank(lbm, one_step):
    """The RCCL step loop with the flag: K-step launches with ghost rows, and (LBM_FLAG_ONE_STEP) the split-phase one-step kernels
    with their halo rows — lbm_step_kernel, four cells per lane, on a rank of more than 65 536 cells."""
    p, obst = synthetic(lbm, 512, 160, 9, block_accel_row=True)
    flags = lbm._capi.FLAG_FORCE_HALO | lbm._capi.FLAG_FUSED_ARITH | (lbm._capi.FLAG_ONE_STEP if one_step else 0)
    sim = lbm.Simulation(p, obst, flags=flags, exchange="rccl", strict=True)
    d = sim.describe()
    kernel = sim.partition.describe()["kernel"]
    assert d["loop"] == "rccl" and d["fused_arith"] and (d["macro_k"] == 0) == one_step, d
    assert kernel.startswith("lbm_step_kernel_fused<" if one_step else "lbm_multi_kernel<4, 6> (fused arithmetic)"), kernel
    av = np.concatenate([sim.run(5), sim.run(4)])
    cells = sim.local_cells()
    sim.close()
    ref_cells, ref_sums = fused_ref.run(p, obst, 9, mode="fused")
    assert np.array_equal(bits(cells), bits(ref_cells))
    # the loop reports av_vels as floats: (float)(sum * (double)free_cells_inv), i.e. the restatement's value to 2^-24 (the float's
    # rounding) on top of the sums' 1e-12
    assert av.dtype == np.float32
    ref_av = ref_sums * np.float64(fused_ref.free_cells_inv(obst))
    assert np.max(np.abs(av.astype(np.float64) - ref_av) / ref_av) <= 2.0 ** -24 + SUMS_RTOL


PARTITIONS = [
    ("ring_of_2_rows", ["rows", "1024", "256", "2", "19"]),          # two groups of launches and a tail
    ("ring_of_3_uneven_rows", ["rows", "256", "190", "3", "13"]),    # 63 + 63 + 64 rows
    ("tiles_2x2", ["tiles", "512", "256", "2", "2", "11"]),
    ("column_blocks_2x1", ["tiles", "512", "256", "2", "1", "11"]),
]


@pytest.mark.parametrize("case", PARTITIONS, ids=[c[0] for c in PARTITIONS])
def test_partitions_in_one_process_equal_a_single_fused_context(lbm, case):
    """Peer-to-peer rings of row blocks and tile grids (tests/fused_partition_worker.py, a fresh process with a hardware queue per
    rank): the ranks' state digests add up to a single fused context's, and not to the exact arithmetic's."""
    env = dict(os.environ, GPU_MAX_HW_QUEUES="16", LBM_P2P_TIMEOUT_MS="10000")
    for k in ("LBM_TUNE_MACRO_K", "LBM_TUNE_MACRO_GHOST", "LBM_TUNE_MACRO_GROUP", "LBM_P2P_SCHEDULE", "LBM_TUNE_TILE_GHOST_ROWS"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fused_partition_worker.py"), *case[1]], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "FUSED PARTITIONS ok" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])


def test_cli_with_lbm_flags_256_on_the_shipped_128x128_deck(lbm, oracle, digests, tmp_path):
    """LBM_FLAGS=256 bin/d2q9-bgk: passes check.py's rule, and writes the final_state.dat the restatement's state gives."""
    ppath, opath = deck_paths("128x128", digests)
    p, obst = shipped(oracle, digests, "128x128")
    r = subprocess.run([lbm.CLI_PATH, ppath, opath], cwd=tmp_path, capture_output=True, text=True, timeout=300, env=dict(os.environ, LBM_FLAGS="256"))
    assert r.returncode == 0 and r.stdout.splitlines()[0] == "==done==", (r.stdout, r.stderr)
    rep = lbm.checker.check_files(os.path.join(GOLDEN, "check", "128x128.av_vels.dat.gz"), os.path.join(GOLDEN, "check", "128x128.final_state.dat.gz"),
                                  str(tmp_path / "av_vels.dat"), str(tmp_path / "final_state.dat"))
    assert rep.ok and "Both tests passed!" in rep.message, rep.message
    ref_cells, _ = fused_ref.run(p, obst, p.max_iters, mode="fused", nthreads=min(os.cpu_count() or 4, 16))
    oracle.write_final_state(str(tmp_path / "expected_final_state.dat"), p, ref_cells, obst)
    with open(tmp_path / "final_state.dat", "rb") as got, open(tmp_path / "expected_final_state.dat", "rb") as want:
        assert got.read() == want.read()
