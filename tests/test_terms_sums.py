"""The per-step double sums of every float kernel (lbm_step_collect after lbm_run, or after the in-process K-step partition loop) against
the exactly rounded sum of the reference's per-cell terms (tests/terms_ref.py StepSums: oracle_exact_sum over the oracle's terms, or over
tests/fused_ref.c's for LBM_FLAG_FUSED_ARITH).  A census: every case starts from a random state in which every free cell carries a term
of ordinary size, so a cell dropped or counted twice anywhere moves the sum by orders of magnitude more than the bound
(tests/test_terms_ref.py test_census_self_check); each case asserts, from the reference alone, that at most 0.1 % of the free cells have
a term below 8 x the asserted absolute bound.

Per step:  |dev - exact| <= rel_bound(family, form) * exact,  rel_bound = (D + 2) * 2^-53 + E_form.

D, the most additions a term passes through on its way into sums[t] (every term is non-negative, so each addition errs by at most
2^-53 of its result, which is at most the total), read off the code per family:
  step   lbm_step_kernel (kernels/step.h).  finish_quad adds a lane's four terms onto 0.0: 4; the kernel adds that onto its accumulator
         once per 1024-cell chunk of the block, and pick_iters (lbm_plan.cpp) leaves one chunk up to 16 384 blocks: 1; block_sum
         (kernels/common.h): six butterfly levels and the four waves' sums added serially: 9; the fold (block 0 of the next launch,
         fold_previous; lbm_fold_kernel after the last one): a lane adds ceil(blocks / 256) = 1 partials (at most 7 blocks here), then
         block_sum: 9.  D = 4 + 1 + 9 + 1 + 9 = 24.  The narrow form adds one term per lane instead of four: 20.
  tile   lbm_tile_kernel (kernels/tile.h).  A lane holds one pair's term per sub-step (t0 + t1: 1; one cell's in the late sub-steps);
         wave_sum_vec8 / wave_sum_vec4: two halving swaps, then four or one + three lane stages: 6; one lane adds the block's waves
         serially, at most 8 (blocks of 512, 320, 512, 128 lanes for the geometries 168, 164, 88, 84): 8; the fold in block 0 of the next
         launch: ceil(tiles / block) = 1 (at most 32 tiles here) + wave_sum 6 + its waves 8 = 15 (lbm_fold_kernel after the last launch:
         1 + 9).  D = 1 + 6 + 8 + 15 = 30.
  multi  lbm_multi_kernel (kernels/multi.h).  The pair: (double)p.x + (double)p.y, or t0 + t1: 1; k_substeps deals a region's pairs in
         passes of the block and adds each onto the lane's accumulator of that sub-step: at most 2 (the largest region, 36 x 19 pairs of
         K = 4 or 34 x 20 of K = 3, on 512 lanes); the compensated form widens the lane's float lo sum onto it once: 1 (the tall
         geometry's finish_pair adds hi + (double)lo per pair and deals a lane one pair per sub-step: 2 in all); wave_sum_vec4 or
         wave_sum: 6; one lane adds the block's 8 or 12 waves: 12; the fold in block 0 of the next launch: a lane adds
         ceil(tiles / lanes) <= 2 partials (1024 tiles of the K = 3 launch at 1024 x 1024, 512 lanes) + wave_sum 6 + its waves 12 = 20;
         after the last launch lbm_fold_kernel over < 1024 partials: ceil(n / 256) <= 4, + 9 = 13, or from 1024 partials
         lbm_fold_slices_kernel (64 slices of 16: 1 + 9) and lbm_fold_kernel over the 64 slice sums (1 + 9): 20.
         D = 1 + 2 + 1 + 6 + 12 + 20 = 42.
  parts  K-step row partitions: lbm_multi_kernel's tree per partition, and the test adds the 2 or 3 partitions' sums on the host: 44.

E_form: 0 for the double form (every term is the reference's double, tests/test_terms_cells.py).  Compensated form: B_COMP per term
(test_terms_cells.py's derivation; every term of these states has msq far above 2^-104, asserted from the reference) plus the float
additions of the lo parts — a pair's two (one rounding), then onto the lane's float accumulator, at most twice per sub-step (the first
onto 0.0f is exact): 3 roundings of 2^-24 of at most the lane's sum of |lo| <= 2^-22 (1 + 2^-19) of its terms: LANE_LO = 3 * 2^-46 (1 +
2^-18).  Together 8.125 * 2^-46 + 44 * 2^-53 < 2^-42.8, below the 2^-40 every double and compensated case must stay under.
Float form (LBM_FLAG_FAST_AVVELS): B_FLOAT per term and one float addition per pair: B_FLOAT + 2^-24 (1 + 2^-20), about 2^-22; a
cell's share of the sum on the grids it runs on here is above 2^-12.

The slow decks (density 0.1, accel 1e-17 and 1e-22, from the initial state) are held per cell: the double form to the tree bound, the
compensated default to the sum over the free cells of test_terms_cells.py's per-cell bound for the cell's own msq (its low-range bounds
where msq is below 2^-104), plus LANE_LO and the tree.  What the reference shows of these decks stands in the test's docstring."""
import math
import os

import numpy as np
import pytest

import terms_ref
import test_terms_cells as tc
from conftest import ARTIFACTS          # where tests leave what they record

U = 2.0 ** -53
OMEGA = 1.4              # a random state of unrelated populations stays positive for the steps run here (checked from the reference)
TREE_DEPTH = {"step": 24, "tile": 30, "multi": 42, "parts": 44}
LANE_LO = 3 * 2.0 ** -46 * (1 + 2.0 ** -18)
B_FAST = tc.B_FLOAT + tc.U32 * (1 + 2.0 ** -20)
E_FORM = {"double": 0.0, "compensated": tc.B_COMP + LANE_LO, "float": B_FAST}


def _pow2(x):
    return f"2^{math.log2(x):.2f}" if x > 0 else "0"


def rel_bound(family, form):
    return (TREE_DEPTH[family] + 2) * U + E_FORM[form]


def census_obstacles(nx, ny, seed, xgeom=None, ygeom=None, extra_rows=()):
    """Random, 30 % blocked; blocked cells forced on row ny - 2, in column 0 and column nx - 1, and on both sides of every tile and frame
    edge: xgeom = (tile width, frame growth) puts edges at k * width and k * width -+ growth, ygeom the same for rows; extra_rows are
    further row edges (partition boundaries).  A forced cell every fourth position along the edge, so free cells sit there too."""
    rng = np.random.default_rng(seed)
    obst = (rng.random((ny, nx)) < 0.3).astype(np.int32)
    obst[ny - 2, ::3] = 1
    obst[1::3, 0] = 1
    obst[2::3, nx - 1] = 1
    xs, ys = set(), set(extra_rows)
    if xgeom:
        for k in range(0, nx + xgeom[0], xgeom[0]):
            xs.update((k, k - xgeom[1], k + xgeom[1]))
    if ygeom:
        for k in range(0, ny + ygeom[0], ygeom[0]):
            ys.update((k, k - ygeom[1], k + ygeom[1]))
    for e in xs:
        obst[0::4, (e - 1) % nx] = 1
        obst[2::4, e % nx] = 1
    for e in ys:
        obst[(e - 1) % ny, 1::4] = 1
        obst[e % ny, 3::4] = 1
    obst[ny // 2, nx // 2] = 0              # never everything
    return obst


_refs = {}


def reference(lbm, nx, ny, steps, fused, obst_key, accel=0.005):
    """(p, obst, cells0, StepSums) of a case, computed once per process and shared; obst_key = (seed, xgeom, ygeom, extra_rows)."""
    key = (nx, ny, fused, obst_key, accel)
    if key not in _refs or _refs[key][4] < steps:
        p = lbm.Params(nx, ny, steps, 4, 0.1, accel, OMEGA)
        obst = census_obstacles(nx, ny, *obst_key)
        cells0 = terms_ref.random_state(ny, nx, 1000 + nx * 7 + ny)
        _refs[key] = (p, obst, cells0, terms_ref.StepSums(p, obst, cells0, steps, fused=fused), steps)
    return _refs[key][:4]


def check(dev, ref, n, family, form, what):
    """The assertion of the module docstring over the first n steps, the census condition, and the figures printed."""
    rel = rel_bound(family, form)
    assert form == "float" or rel < 2.0 ** -40
    exact = ref.sums[:n]
    assert dev.shape == exact.shape and np.all(exact > 0)
    worst = 0.0
    for t in range(n):
        terms = ref.terms[t][ref.free]
        assert np.all(terms >= 0), "the bound is for non-negative terms"
        share = ref.share_below(t, 8 * rel * exact[t])
        assert share <= 0.001, (what, t, share)
        worst = max(worst, abs(dev[t] - exact[t]) / exact[t])
    print(f"  {what}: largest |dev - exact| / exact = {worst / U:.2f} x 2^-53 = {_pow2(worst)}; bound {_pow2(rel)} ({family}, {form})")
    assert np.all(np.abs(dev - exact) <= rel * exact), what


def run_whole(lbm, p, obst, cells0, n, flags=0):
    """lbm_run on one context from cells0; returns the per-step double sums (lbm_step_collect: lbm_run advances run_done through
    after_launch in every family, the one-step kernels included), the kernel's name and the final state."""
    part = lbm.Partition(p, lbm.count_free_cells(obst), obst, flags=flags)
    try:
        part.set_cells(cells0)
        kernel = part.describe()["kernel"]
        av = part.run(n)
        sums = part.step_collect(n)
        cells = part.get_cells()
    finally:
        part.close()
    inv = np.float64(np.float32(1.0) / np.float32(lbm.count_free_cells(obst)))
    assert np.array_equal(av, (sums * inv).astype(np.float32)), "av_vels are these sums times free_cells_inv"
    return sums, kernel, cells


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _flags(lbm, form):
    return {"default": 0, "exact": lbm._capi.FLAG_EXACT_AVVELS, "fused": lbm._capi.FLAG_FUSED_ARITH, "fast": lbm._capi.FLAG_FAST_AVVELS}[form]


def _one_step_env(monkeypatch, vector):
    if vector:
        monkeypatch.setenv("LBM_TUNE_NARROW_MAX", "0")
    monkeypatch.setenv("LBM_TUNE_TILE_MAX", "0")
    monkeypatch.setenv("LBM_TUNE_MULTI_K", "0")
    monkeypatch.setenv("LBM_TUNE_MACRO_K", "0")


STEP_CASES = [(nx, ny, vector, form) for nx, ny, vector in ((48, 20, True), (1028, 6, True), (12, 7, False), (7, 9, False))
              for form in ("default", "fused", "fast") if form != "fast" or (nx, ny) == (48, 20)]


@pytest.mark.gpu
@pytest.mark.parametrize("nx,ny,vector,form", STEP_CASES)
def test_one_step_kernels(lbm, monkeypatch, nx, ny, vector, form):
    """lbm_step_kernel (vector form: four cells per lane) and its narrow form (one cell per lane; odd nx), 5 steps.  The terms are
    doubles whatever the flag: LBM_FLAG_FAST_AVVELS changes nothing in this family, and is held to the double form's bound."""
    _one_step_env(monkeypatch, vector)
    p, obst, cells0, ref = reference(lbm, nx, ny, 5, form == "fused", (nx + ny, None, None, ()))
    sums, kernel, cells = run_whole(lbm, p, obst, cells0, 5, _flags(lbm, form))
    assert kernel.startswith("lbm_step_kernel" + ("" if vector else "_narrow") + ("_fused<" if form == "fused" else "<")), kernel
    assert np.array_equal(_bits(cells), _bits(ref.cells))
    check(sums, ref, 5, "step", "double", f"{kernel} {nx}x{ny}")


# the float form (LBM_FLAG_FAST_AVVELS) runs on one grid per geometry
TILE_CASES = [(geom, nx, ny, form) for geom in ("168", "164", "88", "84") for nx, ny in ((16, 16), (32, 16), (64, 32))
              for form in ("default", "fused", "fast") if form != "fast" or (nx, ny) == (32, 16)]


@pytest.mark.gpu
@pytest.mark.parametrize("geom,nx,ny,form", TILE_CASES)
def test_tile_kernel(lbm, monkeypatch, geom, nx, ny, form):
    """lbm_tile_kernel, 9 steps: a full launch of the 8-step geometries and a 1-step tail, 4 + 4 + 1 of the others.  LBM_FLAG_FAST_AVVELS
    (float terms) on one grid per geometry."""
    monkeypatch.setenv("LBM_TUNE_TILE_MAX", str(1 << 30))
    monkeypatch.setenv("LBM_TUNE_TILE_GEOM", geom)
    T, H = int(geom[:-1]), int(geom[-1])
    p, obst, cells0, ref = reference(lbm, nx, ny, 9, form == "fused", (nx + ny, (T, H), (T, H), ()))
    sums, kernel, cells = run_whole(lbm, p, obst, cells0, 9, _flags(lbm, form))
    assert kernel.startswith("lbm_tile_kernel_fused<" if form == "fused" else "lbm_tile_kernel<") and ("fast av_vels" in kernel) == (form == "fast"), kernel
    assert np.array_equal(_bits(cells), _bits(ref.cells))
    check(sums, ref, 9, "tile", "float" if form == "fast" else "double", f"{kernel} {nx}x{ny}")


MULTI_FORM = {"default": "compensated", "exact": "double", "fused": "compensated", "fast": "float"}


def _multi_case(lbm, nx, ny, n, form, obst_key, expect_k):
    p, obst, cells0, ref = reference(lbm, nx, ny, n, form == "fused", obst_key)
    sums, kernel, cells = run_whole(lbm, p, obst, cells0, n, _flags(lbm, form))
    assert kernel.startswith(f"lbm_multi_kernel<{expect_k}"), kernel
    assert ("double-precision av_vels terms" in kernel) == (form == "exact") and ("fused arithmetic" in kernel) == (form == "fused") and ("fast av_vels" in kernel) == (form == "fast"), kernel
    assert np.array_equal(_bits(cells), _bits(ref.cells))
    term_floor = min(float(t[ref.free].min()) for t in ref.terms[:n])
    assert term_floor > 2.0 ** -40, "term = sqrt(msq) / rho with rho above 2^-5: msq above 2^-90, far from the compensated form's low range (below 2^-104)"
    check(sums, ref, n, "multi", MULTI_FORM[form], f"{kernel} {nx}x{ny} {n} steps")


# the float form (LBM_FLAG_FAST_AVVELS) runs on the ragged grid's long run only: one case per K and tile width
MULTI_CASES = [(K, tile, nx, ny, long_run, form) for K in (2, 3, 4) for tile in (64, 32) for nx, ny in ((128, 32), (130, 34), (448, 112))
               for long_run in (False, True) for form in ("default", "exact", "fused", "fast")
               if form != "fast" or ((nx, ny) == (130, 34) and long_run)]


@pytest.mark.gpu
@pytest.mark.parametrize("K,tile,nx,ny,long_run,form", MULTI_CASES)
def test_multi_kernel(lbm, monkeypatch, K, tile, nx, ny, long_run, form):
    """lbm_multi_kernel<K> on 64- and 32-wide tiles: one tile row, a ragged grid, a grid with inner tiles; K + 1 steps (a full launch
    and a tail, or one launch of 4 at K = 3) and 2 K + 3 steps.  LBM_FLAG_FAST_AVVELS on the ragged grid's long run only."""
    monkeypatch.setenv("LBM_TUNE_MULTI_K", str(K))
    monkeypatch.setenv("LBM_TUNE_MULTI_TILE", str(tile))
    monkeypatch.setenv("LBM_TUNE_TILE_MAX", "0")
    ty = 13 if K == 4 else 16
    ex = 2 * (K // 2)                                     # multi_ex(K - 1)
    n = 2 * K + 3 if long_run else K + 1
    _multi_case(lbm, nx, ny, n, form, (nx + ny + K, (tile, ex), (ty, K - 1), ()), K)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["default", "exact", "fused"])
@pytest.mark.parametrize("geom,nx,ny", [("0", 322, 140), ("1", 322, 140), ("2", 322, 140), ("0", 128, 57), ("1", 128, 57), ("2", 128, 57), (None, 1024, 1024)])
def test_multi_kernel_four_steps_geometries(lbm, monkeypatch, geom, nx, ny, form):
    """The three launch geometries of lbm_multi_kernel<4> (standard 64 x 13, narrow 32 x 13, tall 64 x 24 on 768 lanes with a fixed owned
    pair per lane) on ragged grids, and the library's own plan at 1024 x 1024 (the tall geometry from 2^20 cells); 11 steps = 4 + 4 + 3."""
    if geom is not None:
        monkeypatch.setenv("LBM_TUNE_TILE_MAX", "0")
        monkeypatch.setenv("LBM_TUNE_MULTI_K", "4")
        monkeypatch.setenv("LBM_TUNE_MULTI_GEOM", geom)
    tx, ty = (32 if geom == "1" else 64), (24 if geom in ("2", None) else 13)
    _multi_case(lbm, nx, ny, 11, form, (nx + ny, (tx, 4), (ty, 3), ()), 4)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["default", "exact"])
@pytest.mark.parametrize("K", [3, 4])
@pytest.mark.parametrize("nx,ny,size", [(256, 200, 2), (256, 200, 3), (130, 100, 2), (130, 100, 3)])
def test_k_step_row_partitions_in_process(lbm, monkeypatch, nx, ny, size, K, form):
    """2 and 3 row partitions of one grid as contexts of one process, ghost rows exchanged by device copies
    (tests/test_gpu_parity.py _k_step_partitions_in_process, which returns the partitions' double sums added up); 11 steps."""
    import test_gpu_parity as gp
    monkeypatch.setenv("LBM_TUNE_MACRO_K", str(K))
    n = 11
    ny_local, displs = lbm.decompose(ny, size)
    ty = 13 if K == 4 else 16
    p, obst, cells0, ref = reference(lbm, nx, ny, n, False, (nx + ny + size, (64, 2 * (K // 2)), (ty, K - 1), tuple(displs)))
    free = lbm.count_free_cells(obst)
    parts = [lbm.Partition(p, free, obst[displs[r]:displs[r] + ny_local[r]], displs[r], obstacles_global=obst, flags=_flags(lbm, form)) for r in range(size)]
    try:
        assert all(part.macro_steps == K for part in parts), [part.macro_steps for part in parts]
        for r, part in enumerate(parts):
            part.set_cells(cells0[displs[r]:displs[r] + ny_local[r]])
        sums = gp._k_step_partitions_in_process(lbm, parts, n, K)
        cells = np.concatenate([part.get_cells() for part in parts], axis=0)
    finally:
        for part in parts:
            part.close()
    assert np.array_equal(_bits(cells), _bits(ref.cells))
    check(sums, ref, n, "parts", MULTI_FORM[form], f"{size} partitions of {nx}x{ny}, K = {K}, {form}")


def _slow_reference(lbm, oracle, nx, ny, accel, n):
    """The deck from its initial state: per step the exact sum, the (ny, nx) terms, and msq, rinv of every cell."""
    import ctypes as C
    p = lbm.Params(nx, ny, n, 4, 0.1, accel, 1.7)
    obst = census_obstacles(nx, ny, nx + ny, (64, 2), (16, 2))
    cells = np.empty((ny, nx, 9), np.float32)
    oracle.lib().oracle_init_cells(C.byref(oracle.cparams(p)), oracle._f(cells), ny)
    ref = terms_ref.StepSums(p, obst, cells, n)
    per_cell = []
    state = cells
    for t in range(n):
        term, msq, rinv = terms_ref.cell_terms(terms_ref.pulled(terms_ref.accelerated(p, obst, state)))
        assert np.array_equal(np.where(obst != 0, 0.0, term), ref.terms[t])
        per_cell.append((msq, rinv, term))
        state, _ = oracle.run_from(p, obst, state, 1)
    return p, obst, cells, ref, per_cell


@pytest.mark.gpu
@pytest.mark.parametrize("accel", [1e-17, 1e-22])
@pytest.mark.parametrize("nx,ny,multi", [(64, 32, False), (128, 32, True)])
def test_slow_decks(lbm, oracle, monkeypatch, nx, ny, multi, accel):
    """Density 0.1, accel 1e-17 and 1e-22, from the initial state; 64 x 32 on the library's own choice (lbm_tile_kernel, double terms) and
    128 x 32 through lbm_multi_kernel<3> with its default (compensated) and its double form.  What the reference shows: at these
    accelerations w1 = density * accel / 9 is below half an ulp of every population, accelerate_flow changes no bit, the state stays the
    initial one, and every free cell carries the same term 6.585e-9 from msq = 2^-61 = 4.34e-19 — the residue of the rest state's own
    roundings in ((((w1 + w2) + w2) - w1) - w2) - w2 — in every step.  That is inside the compensated form's accurate range (msq >=
    2^-104): these decks never reach the low range, and the per-cell bound summed below is B_COMP throughout.  The low range itself is
    held per cell in tests/test_terms_cells.py (class S)."""
    n = 8
    if multi:
        monkeypatch.setenv("LBM_TUNE_TILE_MAX", "0")
        monkeypatch.setenv("LBM_TUNE_MULTI_K", "3")
    p, obst, cells0, ref, per_cell = _slow_reference(lbm, oracle, nx, ny, accel, n)
    free = obst == 0
    lines = []
    for form in (("default", "exact") if multi else ("default",)):
        sums, kernel, cells = run_whole(lbm, p, obst, cells0, n, _flags(lbm, form))
        family = "multi" if multi else "tile"
        assert kernel.startswith("lbm_multi_kernel<3" if multi else "lbm_tile_kernel<"), kernel
        assert np.array_equal(_bits(cells), _bits(ref.cells))
        compensated = multi and form == "default"
        worst = 0.0
        for t in range(n):
            msq, rinv, term = per_cell[t]
            tree = (TREE_DEPTH[family] + 2) * U * ref.sums[t]
            if compensated:
                lo_b, hi_b, covered, rest, low, main = tc._comp_interval(msq.reshape(-1, 1), rinv.reshape(-1, 1), term.reshape(-1, 1), free.reshape(-1, 1))
                assert covered.all()
                lo_b, hi_b = lo_b.sum() - LANE_LO * ref.sums[t] - tree, hi_b.sum() + LANE_LO * ref.sums[t] + tree
            else:
                lo_b, hi_b = ref.sums[t] - tree, ref.sums[t] + tree
            assert lo_b <= sums[t] <= hi_b, (kernel, t, sums[t], ref.sums[t], lo_b, hi_b)
            if ref.sums[t] > 0:
                worst = max(worst, abs(sums[t] - ref.sums[t]) / ref.sums[t])
        inv = np.float64(np.float32(1.0) / np.float32(int(free.sum())))
        av = (sums * inv).astype(np.float32)
        av_ref = (ref.sums * inv).astype(np.float32)
        lines.append(f"accel {accel:g} {nx}x{ny} {kernel}: msq of the free cells in [{min(float(m[free].min()) for m, _, _ in per_cell):.3e}, "
                     f"{max(float(m[free].max()) for m, _, _ in per_cell):.3e}]; largest |dev - exact| / exact = {_pow2(worst)}; "
                     f"av_vels floats that differ from the exact sum's: {int(np.sum(av != av_ref))} of {n}")
    print("\n".join("  " + l for l in lines))
    os.makedirs(ARTIFACTS, exist_ok=True)
    with open(os.path.join(ARTIFACTS, f"slow_deck_{accel:g}_{nx}x{ny}.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")
