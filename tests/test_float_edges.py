"""Every float kernel family on states a lattice run never holds, against the oracle (tests/oracle_lib.py) and, for
LBM_FLAG_FUSED_ARITH, against tests/fused_ref.c: exponents that sweep from the denormals to 2^120 across the grid, random signs, 3 x 3
patches of 0, 2^-149, 2^123 and -0.0, a row ny - 2 written at the edges of accelerate_flow's three tests, and special bit patterns that
stream into blocked cells.  tests/test_f64_edges.py is the pattern; the float kernels carry more machinery that depends on the values of
a whole wave (recip_exact's ballots, finish_pair_lo's obstacle ballot, the block-uniform tile_accel), so the forms are forced one by one
as their own test modules force them, named by describe()["kernel"] and by the launches launch_profile() reports, on the smallest
grids at which each can still go wrong.  No reference value comes from the device.

States (float32, (ny, nx, 9); _state): W1 positive sweep 2^-124 .. 2^40, the five blocked corner cells denormal; W2 signed sweep
2^-149 .. 2^120; "W2 long" the signed sweep of W1's range with two crest columns at 2^120; "blocks" the four patches on a benign state;
"recip" (RECIP_SCALES: patches of the benign state scaled to densities outside the short reciprocal); "accel"; "moved".  W2 starts the runs of up to 5 steps (3 on the two smallest grids), "W2 long" the longer ones (state_for); the 9-step
tile runs of 32 x 16 are not run from either (63 % of the free cells would hold a NaN; 64 x 32 holds those runs).

Populations (_compare_cells): equal sets of NaN places; equal bits wherever the reference holds a number; after ONE step every bit at
the blocked cells, NaN payloads and signs included (nothing but moves happened to them; in later steps a blocked cell may receive a NaN
that a free cell computed, whose payload is the processor's own).

Per-step sums (lbm_step_collect; av_vels are these times free_cells_inv, asserted), by the step's terms in the reference (_compare_sums):
  a NaN term, or infinite terms of both signs    the device's entry is a NaN;
  infinite terms of one sign only                the device's entry is not finite;
  every term finite, double form                 the one-step kernels, lbm_tile_kernel, lbm_multi_kernel with LBM_FLAG_EXACT_AVVELS:
                                                 |dev - exact| <= (TREE_DEPTH + 2) 2^-53 of the sum of the terms' MAGNITUDES
                                                 (tests/test_terms_sums.py's tree depths; exact = the exactly rounded sum, math.fsum);
  every term finite, compensated form            lbm_multi_kernel's default: the sum over the free cells of test_terms_cells.py's
                                                 interval of the cell's own msq and rinv (_comp_interval: exactly 0 at msq = 0, an
                                                 under-estimate between 0 and the term below msq = 2^-126, B_COMP and comp_abs above),
                                                 widened by (LANE_LO + tree) of the magnitudes;
  every term finite, float form                  LBM_FLAG_FAST_AVVELS on lbm_multi_kernel: B_FAST per term where msq >= 2^-126 and the
                                                 term is a normal float, exactly 0 below (the instruction flushes its argument: pinned
                                                 in test_terms_cells.py), plus the tree.
The compensated and the float form state no bound for a cell whose reciprocal is a denormal or an infinity or whose term is outside the
normal floats; a step that holds such a free cell is counted as "not held" for these two forms and only the populations are checked
there.  W1 and "blocks" must have every finite step held (asserted); W2, "W2 long", "accel" and "moved" hold what they hold.

Where accelerate_flow's three tests are met.  The row ny - 2 that "accel" writes is the INITIAL state's, and the acceleration before
the first step of a run is lbm_accelerate_kernel's (kernels/aux.h), in every family: that kernel is what the exact zeros, the ulp, the
lone NaNs and the +inf of "accel" hold.  The tests folded into the step kernels (accelerate_cell, and the one-step and multi-step
kernels' own copies) see only what a step has just produced.  A free cell's nine results share rho, so a NaN among the streamed-in
populations makes all nine NaN, and the NaNs that arithmetic makes from numbers (inf - inf in "a m - msq", 0 inf in "h d") come with
magnitudes of 2^63 and more or with infinite partners, where adding w1 = 5.6e-5 changes no bit: whether such a cell is accelerated
cannot be seen in the populations.  What the folded tests do decide, and what W1, W2 and "accel" hold in runs of two steps and more,
is the sign of each of the three differences (profiles/r17/float_edges_mutants.txt, mutants 2, 2b and 2c).

What the states reach is counted from the reference alone in test_states_reach_what_they_are_for (no GPU)."""
import functools
import math
from types import SimpleNamespace

import numpy as np
import pytest

import fused_ref
import oracle_lib
import terms_ref
import test_terms_cells as tc
from test_terms_sums import B_FAST, LANE_LO, TREE_DEPTH, U

DX = (0, 1, 0, -1, 0, 1, -1, -1, 1)
DY = (0, 0, 1, 0, -1, 1, 1, -1, -1)
BACK = (0, 3, 4, 1, 2, 7, 8, 5, 6)
SEED = 7


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- decks and states, from numpy alone ------------------------------------------------------------------------------------------

def _patches(nx, ny):
    """Top-left cells of the four 3 x 3 patches, none on row ny - 2.  The first starts at an odd x (an x-pair then holds one patch cell
    and one benign cell); the second straddles the column seam of every tiling the grid can have (x = 63, 31 or 15: tiles are 64, 32,
    16 or 8 wide); the lower two straddle the row seam at y = 8 where the grid has eleven rows or more."""
    seam = next(x for x in (63, 31, 15) if x + 6 < nx)
    if ny >= 11:
        return ((1, 3), (1, seam), (6, 8), (6, 21))
    return ((0, 3), (0, seam), (0, 100), (0, 121))          # 1028 x 6: rows 0 .. 2, row 4 is the accelerated one


PATCH_BITS = (0x7D000000, 0x00000000, 0x00000001, 0x80000000)          # 2^123 (at the odd x), 0.0, 2^-149, -0.0


@functools.lru_cache(maxsize=None)
def _deck(nx, ny):
    """density 0.1, accel 0.005, omega 1.85; 10 % random obstacles, cleared around the patches; the five cells of column 0 where the
    sweeps are lowest blocked: they keep the denormals W1 gives them and stream them into free cells in every step."""
    p = SimpleNamespace(nx=nx, ny=ny, max_iters=16, reynolds_dim=4, density=0.1, accel=0.005, omega=1.85)
    obst = (np.random.default_rng(1000 * nx + ny).random((ny, nx)) < 0.10).astype(np.int32)
    for y, x in _patches(nx, ny):
        obst[np.ix_(np.arange(y - 1, y + 4) % ny, np.arange(x - 1, x + 4) % nx)] = 0
    obst[[ny - 2, ny - 1, 0, 1, 2], 0] = 1
    obst.setflags(write=False)
    return p, obst


def _tri(n):
    """The periodic triangle 1 - |2 i / n - 1|."""
    return 1.0 - np.abs(2.0 * np.arange(n) / n - 1.0)


def _make(e, sig, neg=None):
    """Floats 2^e (1 + sig / 2^23); below 2^-126 the denormal nearest below (at least 2^-149)."""
    e = np.asarray(e, np.int64)
    sig = np.asarray(sig, np.int64)
    normal = ((np.clip(e, -126, 127) + 127) << 23) | sig
    den = np.maximum(((1 << 23) | sig) >> np.clip(-126 - e, 0, 24), 1)
    b = np.where(e >= -126, normal, den).astype(np.uint32)
    if neg is not None:
        b = b | (np.asarray(neg, np.uint32) << np.uint32(31))
    return b.view(np.float32)


def _wide(nx, ny, lo, hi, signs, seed=SEED):
    """One exponent per cell, rint(lo + (hi - lo) (0.8 tri(x) + 0.2 tri(y))); each population within 2 binades of it, a random significand."""
    rng = np.random.default_rng(seed)
    e = np.rint(lo + (hi - lo) * (0.8 * _tri(nx)[None, :] + 0.2 * _tri(ny)[:, None])).astype(np.int64)
    e = e[:, :, None] + rng.integers(-2, 3, (ny, nx, 9))
    sig = rng.integers(0, 1 << 23, (ny, nx, 9))
    neg = rng.integers(0, 2, (ny, nx, 9)) if signs else None
    return _make(e, sig, neg).copy()


def _benign(p, seed):
    rest = np.array([4.0 / 9.0] + [1.0 / 9.0] * 4 + [1.0 / 36.0] * 4) * p.density
    return (rest * np.random.default_rng(seed).uniform(0.8, 1.2, (p.ny, p.nx, 9))).astype(np.float32)


MOVED = np.array([0x7FA0ABCD, 0xFF900123, 0x7F800001, 0x00000001, 0x807FFFFF, 0x00000ABC, 0x80000000, 0x7F800000, 0xFF800000], np.uint32)
# signalling NaNs with payloads, denormals, -0.0, +-inf


def _sources_of_blocked(p, obst):
    """(y, x, k, ys, xs, i): population k of blocked cell (y, x) streams in from cell (ys, xs) and is fed MOVED[i]; sources on the
    accelerated row are left out (accelerate_flow may rewrite them before the step)."""
    out = []
    for n, (y, x) in enumerate(np.argwhere(obst != 0)):
        for k in range(9):
            ys, xs = (y - DY[k]) % p.ny, (x - DX[k]) % p.nx
            if ys != p.ny - 2:
                out.append((int(y), int(x), k, int(ys), int(xs), (k + n) % MOVED.size))
    return out


def accel_weights(p):
    """w1, w2 of accelerate_flow as the reference forms them in float: density * accel / 9 and / 36."""
    da = np.float32(p.density) * np.float32(p.accel)
    return da / np.float32(9.0), da / np.float32(36.0)


ACCEL_KINDS = ("p3 == w1", "p6 == w2", "p7 == w2 + ulp", "p3 < 0", "p6 < 0", "p7 < 0", "p3 NaN", "p6 NaN", "p7 NaN", "p3 +inf")
ACCEL_TAKEN = (False, False, True, False, False, False, False, False, False, True)
ACCEL_RUN = 3                        # cells per run: odd, so the runs meet both components of the x-pairs


def _accel_kind(x):
    return (x // ACCEL_RUN) % len(ACCEL_KINDS)


def _accel_row(p, row):
    w1, w2 = accel_weights(p)
    inf = np.float32(np.inf)
    for x in range(p.nx):
        k = _accel_kind(x)
        if k == 0: row[x, 3] = w1
        elif k == 1: row[x, 6] = w2
        elif k == 2: row[x, 7] = np.nextafter(w2, inf)
        elif k in (3, 4, 5): row[x, (3, 6, 7)[k - 3]] *= np.float32(-1.0)
        elif k in (6, 7, 8): row[x, (3, 6, 7)[k - 6]] = np.float32(np.nan)
        else: row[x, 3] = inf


# "recip": a recip_exact without its fallback survived W2 on the smallest grids (profiles/r17/float_edges_mutants.txt), and "blocks" cannot show it: the centres of its
# patches have msq = 0 and rinv = inf or a reciprocal that multiplies zeros only): the four patches as the benign state scaled.  Two
# by 2^-123: the centre's density is a denormal near 2^-126.3, outside the short reciprocal, its true reciprocal and every result finite.
# Two by 2^130: the density is above 2^126, the true reciprocal a denormal, msq infinite, and population 0 is -inf, not a NaN, only
# while h = 0.5 rinv 3 is not zero.  The first patch starts at an odd x: the centre's x-pair holds one such cell and one benign cell.
RECIP_SCALES = (2.0 ** -123, 2.0 ** -123, 2.0 ** 130, 2.0 ** 130)
LONG_BAND = 2                        # columns at the crest of "W2 long" that hold W2's own exponents


@functools.lru_cache(maxsize=None)
def _state(name, nx, ny):
    p, obst = _deck(nx, ny)
    if name == "W1":
        s = _wide(nx, ny, -124, 40, False)
        corner = ([ny - 2, ny - 1, 0, 1, 2], 0)
        rng = np.random.default_rng(SEED + 1)
        s[corner] = _make(rng.integers(-149, -129, (5, 9)), rng.integers(0, 1 << 23, (5, 9)))
    elif name == "W2":
        s = _wide(nx, ny, -149, 120, True)
    elif name == "W2 long":
        s = _wide(nx, ny, -124, 40, True)
        x0 = nx // 2 - LONG_BAND // 2
        rng = np.random.default_rng(SEED + 2)
        shape = (ny, LONG_BAND, 9)
        s[:, x0:x0 + LONG_BAND] = _make(120 + rng.integers(-2, 3, shape), rng.integers(0, 1 << 23, shape), rng.integers(0, 2, shape))
    elif name == "blocks":
        s = _benign(p, 33)
        for (y, x), b in zip(_patches(nx, ny), PATCH_BITS):
            _bits(s)[y:y + 3, x:x + 3, :] = np.uint32(b)
    elif name == "recip":
        s = _benign(p, 36)
        for i, (y, x) in enumerate(_patches(nx, ny)):
            s[y:y + 3, x:x + 3, :] = (s[y:y + 3, x:x + 3, :].astype(np.float64) * RECIP_SCALES[i]).astype(np.float32)
    elif name == "accel":
        s = _benign(p, 35)
        _accel_row(p, s[ny - 2])
    elif name == "moved":
        s = _benign(p, 34)
        for (y, x, k, ys, xs, i) in _sources_of_blocked(p, obst):
            _bits(s)[ys, xs, k] = MOVED[i]
    else:
        raise KeyError(name)
    assert s.dtype == np.float32 and s.shape == (ny, nx, 9)
    s.setflags(write=False)
    return s


STATES = ("W1", "W2", "blocks", "recip", "accel", "moved")
W2_MAX = {(32, 16): 3, (30, 11): 3}          # steps W2 itself runs for (5 elsewhere): beyond them more than half of the free cells hold a NaN
W2_LONG_MAX = {(32, 16): 5, (30, 11): 5}     # steps "W2 long" runs for on the two smallest grids: 2 + 2 * 5 of their 32 / 30 columns


def state_for(state, nx, ny, n):
    """The state a run of n steps starts from; None where neither W2 nor "W2 long" stays below the cap on NaNs (another grid holds that run)."""
    if state != "W2":
        return state
    if n <= W2_MAX.get((nx, ny), 5):
        return "W2"
    return "W2 long" if n <= W2_LONG_MAX.get((nx, ny), 1 << 30) else None


@functools.lru_cache(maxsize=None)
def _reference(name, nx, ny, steps, fused=False):
    """(cells, terms): the final populations and the per-step (ny, nx) double terms, computed once per (grid, state, steps, arithmetic)
    for the module and never written to."""
    p, obst = _deck(nx, ny)
    cells0 = _state(name, nx, ny)
    with np.errstate(all="ignore"):
        if not fused:
            cells, _, terms = oracle_lib.run_from(p, obst, cells0, steps, keep_terms=True)
        else:
            cells, _ = fused_ref.run(p, obst, steps, mode="fused", cells0=cells0)
            state, terms = np.array(cells0), []
            for _ in range(steps):
                state, _, t = fused_ref.step_terms(p, obst, state, "fused")
                terms.append(t)
            assert np.array_equal(_bits(state), _bits(cells)), "fused_ref.run and fused_ref.step_terms step alike"
    cells.setflags(write=False)
    for t in terms:
        t.setflags(write=False)
    return cells, tuple(terms)


@functools.lru_cache(maxsize=None)
def _inputs(name, nx, ny, step, fused=False):
    """msq, rinv (float32, (ny, nx)) of step `step` (0-based) of the run from the state: from the populations that stream into each
    cell after accelerate_flow, through fused_ref.cells_msq_rinv."""
    p, obst = _deck(nx, ny)
    state = _state(name, nx, ny) if step == 0 else _reference(name, nx, ny, step, fused)[0]
    with np.errstate(all="ignore"):
        t = terms_ref.pulled(terms_ref.accelerated(p, obst, state))
        return fused_ref.cells_msq_rinv(t, mode="fused" if fused else "exact")


# ---- the comparisons ---------------------------------------------------------------------------------------------------------------

def _compare_cells(got, ref, what, obst=None, every_bit_blocked=False):
    nan_ref, nan_got = np.isnan(ref), np.isnan(got)
    assert np.array_equal(nan_ref, nan_got), f"{what}: {int(np.sum(nan_ref != nan_got))} NaNs misplaced, first at {tuple(np.argwhere(nan_ref != nan_got)[0])}"
    differ = ~nan_ref & (_bits(got) != _bits(ref))
    assert not differ.any(), f"{what}: {int(differ.sum())} numbers differ, first at {tuple(np.argwhere(differ)[0])}"
    if every_bit_blocked:
        blocked = obst != 0
        differ = _bits(got)[blocked] != _bits(ref)[blocked]
        assert not differ.any(), f"{what}: {int(differ.sum())} words of blocked cells differ (NaN payloads and signs count)"


def _float_interval(msq, rinv, term):
    """Per free cell the interval of the float form's term (test_terms_cells.py FLOAT FORM) and whether a bound is stated for the cell."""
    with np.errstate(all="ignore"):
        aref = np.abs(term)
        normal_rinv = np.isfinite(rinv) & (np.abs(rinv) >= tc.MIN_NORMAL)
        zero = (msq >= 0) & (msq < tc.MIN_NORMAL) & (np.isfinite(rinv) if tc.FLOAT_ROOT_OF_A_DENORMAL_IS_ZERO else (msq == 0))
        main = np.isfinite(msq) & (msq >= tc.MIN_NORMAL) & normal_rinv & (aref >= 2.0 ** -125) & (aref <= 2.0 ** 126)
        b = np.where(main, B_FAST * aref, 0.0)
        lo = np.where(zero, 0.0, term - b)
        hi = np.where(zero, 0.0, term + b)
    return lo, hi, zero | main


def _comp_cells(msq, rinv, term):
    """Per free cell the interval of the compensated form's hi + lo (test_terms_cells._comp_interval, one counted cell per row) and
    whether a bound is stated for the cell.  That function states its low range for a positive reciprocal; every operation of the form
    that involves rinv (p = s rinv, e = fma(s, rinv, -p), lo = fma(c, rinv, e)) is odd in it and rounding to nearest is symmetric, so a
    negative reciprocal gives exactly the negated parts: the interval of |rinv|, mirrored."""
    col = lambda a: a.reshape(-1, 1)
    neg = np.signbit(rinv)
    lo, hi, covered, _, _, _ = tc._comp_interval(col(msq), col(np.abs(rinv)), col(np.abs(term)), np.ones((term.size, 1), bool))
    return np.where(neg, -hi, lo), np.where(neg, -lo, hi), covered


def _compare_sums(dev, terms, obst, family, form, what, inputs=None, extra=0):
    """The module docstring's cases, per step.  form: "double", "compensated" or "float"; inputs(t) gives msq, rinv of step t (the two
    float forms); extra: additions beyond the family's tree (partitions' sums added up).  Returns (entries held to NaN, to "not finite", to a bound, finite entries the form states no bound for)."""
    free = obst == 0
    assert dev.shape == (len(terms),)
    tree = (TREE_DEPTH[family] + 2 + extra) * U
    n_nan = n_inf = n_held = n_not = 0
    for t, full in enumerate(terms):
        term = full[free]
        if np.isnan(term).any() or (np.isposinf(term).any() and np.isneginf(term).any()):
            n_nan += 1
            assert np.isnan(dev[t]), f"{what}: sums[{t}] = {dev[t]!r} where a term is a NaN or infinities of both signs meet"
            continue
        if np.isinf(term).any():
            n_inf += 1
            assert not np.isfinite(dev[t]), f"{what}: sums[{t}] = {dev[t]!r} where a term is infinite"
            continue
        mags = math.fsum(np.abs(term).tolist())
        if form == "double":
            exact = math.fsum(term.tolist())
            lo_b, hi_b = exact - tree * mags, exact + tree * mags
        else:
            msq, rinv = (a[free] for a in inputs(t))
            assert np.array_equal(terms_ref.term_of(msq, rinv), term, equal_nan=True), "msq and rinv are the ones the reference's term came from"
            if form == "compensated":
                lo_c, hi_c, covered = _comp_cells(msq, rinv, term)
                slack = (LANE_LO + tree) * mags
            else:
                lo_c, hi_c, covered = _float_interval(msq, rinv, term)
                slack = tree * mags
            if not covered.all():
                n_not += 1
                continue
            lo_b, hi_b = math.fsum(lo_c.tolist()) - slack, math.fsum(hi_c.tolist()) + slack
        n_held += 1
        assert lo_b <= dev[t] <= hi_b, f"{what}: sums[{t}] = {dev[t]!r} outside [{lo_b!r}, {hi_b!r}] ({family}, {form})"
    print(f"  {what}: sums {n_nan} NaN on both sides, {n_inf} held to 'not finite', {n_held} inside their interval ({family}, {form}), {n_not} finite without a stated bound")
    return n_nan, n_inf, n_held, n_not


# ---- the forms ---------------------------------------------------------------------------------------------------------------------

KNOBS = ("LBM_TUNE_NARROW_MAX", "LBM_TUNE_TILE_MAX", "LBM_TUNE_TILE_GEOM", "LBM_TUNE_MULTI_K", "LBM_TUNE_MULTI_GEOM", "LBM_TUNE_MULTI_TILE",
         "LBM_TUNE_MACRO_K", "LBM_TUNE_TILE_SINGLE_MAX")
ONE_STEP = {"LBM_TUNE_TILE_MAX": "0", "LBM_TUNE_MULTI_K": "0", "LBM_TUNE_MACRO_K": "0"}
FLAG_BITS = {"nt": 1, "no_nt": 2, "fast": 64, "exact": 128, "fused": 256}          # include/lbm_d2q9.h; checked against lbm._capi in _context


def _form(env, kernel, family, terms, shapes, steps, flags=(), k=1):
    return dict(env=env, kernel=kernel, family=family, terms=terms, shapes=shapes, steps=steps, flags=flags, k=k)


def _multi_env(K, tile=None, geom=None):
    env = {"LBM_TUNE_TILE_MAX": "0", "LBM_TUNE_MULTI_K": str(K)}
    if tile is not None:
        env["LBM_TUNE_MULTI_TILE"] = str(tile)
    if geom is not None:
        env["LBM_TUNE_MULTI_GEOM"] = str(geom)
    return env


def _multi_name(K, flags):
    if "fused" in flags:
        return f"lbm_multi_kernel<{K}, 6> (fused arithmetic)"
    return f"lbm_multi_kernel<{K}, fast av_vels>" if "fast" in flags else f"lbm_multi_kernel<{K}, double-precision av_vels terms>" if "exact" in flags else f"lbm_multi_kernel<{K}>"


def _multi_terms(flags):
    return "float" if "fast" in flags else "double" if "exact" in flags else "compensated"


VECTOR = dict(ONE_STEP, LBM_TUNE_NARROW_MAX="0")
VECTOR_GRIDS, NARROW_GRIDS, TILE_GRIDS, MULTI_GRIDS, TALL_GRIDS, FIVE_GRIDS = (((64, 32), (1028, 6)), ((30, 11), (257, 33)), ((32, 16), (64, 32)),
                                                                              ((128, 32), (130, 34)), ((194, 77), (256, 83)), ((256, 83), (128, 16)))
FORMS = {"vector": _form(VECTOR, "lbm_step_kernel<", "step", "double", VECTOR_GRIDS, (1, 3)),
         "vector,nt": _form(VECTOR, "lbm_step_kernel<", "step", "double", VECTOR_GRIDS, (1, 3), ("nt",)),
         "vector,no_nt": _form(VECTOR, "lbm_step_kernel<", "step", "double", VECTOR_GRIDS, (1, 3), ("no_nt",)),
         "vector,fused": _form(VECTOR, "lbm_step_kernel_fused<", "step", "double", ((64, 32),), (1, 3), ("fused",)),
         "narrow": _form(ONE_STEP, "lbm_step_kernel_narrow<", "step", "double", NARROW_GRIDS, (1, 3)),
         "narrow,fused": _form(ONE_STEP, "lbm_step_kernel_narrow_fused<", "step", "double", ((257, 33),), (1, 3), ("fused",))}
for _g in ("168", "164", "88", "84"):
    _T, _H = int(_g[:-1]), int(_g[-1])
    _env = {"LBM_TUNE_TILE_MAX": str(1 << 30), "LBM_TUNE_TILE_GEOM": _g}
    FORMS[f"tile<{_T},{_H}>"] = _form(_env, f"lbm_tile_kernel<{_T}, {_H}>", "tile", "double", TILE_GRIDS, (1, _H + 1), k=_H)
# 8-wide tiles of 8 steps deal one cell per lane in every sub-step at the default LBM_TUNE_TILE_SINGLE_MAX (bounce_or_relax, the scalar
# recip_exact); with 0 every sub-step deals x-pairs (finish_pair, the packed one)
FORMS["tile<8,8>,pairs"] = _form({"LBM_TUNE_TILE_MAX": str(1 << 30), "LBM_TUNE_TILE_GEOM": "88", "LBM_TUNE_TILE_SINGLE_MAX": "0"}, "lbm_tile_kernel<8, 8>",
                                 "tile", "double", TILE_GRIDS, (1, 9), k=8)
FORMS["tile<16,4>,fused"] = _form({"LBM_TUNE_TILE_MAX": str(1 << 30), "LBM_TUNE_TILE_GEOM": "164"}, "lbm_tile_kernel_fused<16, 4>", "tile", "double",
                                  ((64, 32),), (1, 5), ("fused",), k=4)
for _K in (2, 3, 4):
    for _tile in (64, 32):
        FORMS[f"multi<{_K}>,{_tile}"] = _form(_multi_env(_K, _tile), _multi_name(_K, ()), "multi", "compensated", MULTI_GRIDS, (1, _K, _K + 3), k=_K)
for _f in ("exact", "fast", "fused"):
    FORMS[f"multi<4>,64,{_f}"] = _form(_multi_env(4, 64), _multi_name(4, (_f,)), "multi", _multi_terms((_f,)), ((130, 34),), (1, 7), (_f,), k=4)
FORMS["tall<4>"] = _form(_multi_env(4, geom=2), _multi_name(4, ()), "multi", "compensated", TALL_GRIDS, (1, 4, 7), k=4)
FORMS["five"] = _form(_multi_env(5, geom=2), _multi_name(5, ()), "multi", "compensated", FIVE_GRIDS, (1, 5, 7, 11), k=5)
for _f in ("exact", "fast", "fused"):
    FORMS[f"tall<4>,{_f}"] = _form(_multi_env(4, geom=2), _multi_name(4, (_f,)), "multi", _multi_terms((_f,)), ((256, 83),), (1, 7), (_f,), k=4)
    FORMS[f"five,{_f}"] = _form(_multi_env(5, geom=2), _multi_name(5, (_f,)), "multi", _multi_terms((_f,)), ((256, 83),), (1, 7), (_f,), k=5)
CASES = [(form, nx, ny) for form, f in FORMS.items() for (nx, ny) in f["shapes"]]

# the partitioned runs: (grid, ranks, K, steps)
ROW_SPLIT = ((64, 48), 3, 0, 3)
ROW_K_STEP = (((130, 100), 2, 4, 9), ((256, 200), 3, 3, 9))
# tile ranks (nx, ny, px, py, K, ghost, steps): of tests/test_gpu_parity.py TILE_CASES the smallest grid whose ranks keep ghost rows and
# ghost columns, and the column blocks narrower than two tiles; 8 ghost rows / columns: a group of two launches (3 + 4), then 4
TILE_RANKS = ((512, 256, 2, 2, 4, 8, 11), (448, 256, 4, 1, 4, 8, 11))


def _runs():
    """Every (state, nx, ny, steps, fused) a GPU test compares against: what the reach test goes through."""
    out = set()
    for form, nx, ny in CASES:
        for n in FORMS[form]["steps"]:
            for state in STATES:
                name = state_for(state, nx, ny, n)
                if name is not None:
                    out.add((name, nx, ny, n, "fused" in FORMS[form]["flags"]))
    for (nx, ny), _, _, n in (ROW_SPLIT,) + ROW_K_STEP:
        for state in STATES:
            out.add((state_for(state, nx, ny, n), nx, ny, n, False))
    for nx, ny, _, _, _, _, n in TILE_RANKS:
        for state in STATES:
            out.add((state_for(state, nx, ny, n), nx, ny, n, False))
    return sorted(out)


FIVE_LAUNCHES = {1: [1], 5: [5], 7: [4, 3], 11: [5, 3, 3]}          # the five-step plan's tails (tests/test_multi5.py, tests/test_plan_k5.py)


def expected_launches(lbm, form, n):
    """The steps of every launch of a run of n steps: one per step for the one-step kernels, H at a time and the rest for
    lbm_tile_kernel, lbm_plan_steps for lbm_multi_kernel."""
    f = FORMS[form]
    if f["family"] == "step":
        return [1] * n
    if f["family"] == "tile":
        return [f["k"]] * (n // f["k"]) + ([n % f["k"]] if n % f["k"] else [])
    if f["k"] == 5:
        return FIVE_LAUNCHES[n]
    return lbm.plan_steps(f["k"], n)


def _context(lbm, monkeypatch, form, nx, ny):
    f = FORMS[form]
    assert (lbm._capi.FLAG_NT_STORES, lbm._capi.FLAG_NO_NT_STORES, lbm._capi.FLAG_FAST_AVVELS, lbm._capi.FLAG_EXACT_AVVELS, lbm._capi.FLAG_FUSED_ARITH) == \
        tuple(FLAG_BITS[k] for k in ("nt", "no_nt", "fast", "exact", "fused"))
    for knob in KNOBS:
        monkeypatch.delenv(knob, raising=False)
    for knob, value in f["env"].items():
        monkeypatch.setenv(knob, value)
    p, obst = _deck(nx, ny)
    lp = lbm.Params(nx, ny, p.max_iters, p.reynolds_dim, p.density, p.accel, p.omega)
    part = lbm.Partition(lp, lbm.count_free_cells(obst), obst, flags=sum(FLAG_BITS[k] for k in f["flags"]))
    kernel = part.describe()["kernel"]
    if not (kernel.startswith(f["kernel"]) if f["kernel"].endswith("<") else kernel == f["kernel"]):          # a fallback cannot pass for the kernel
        part.close()
        raise AssertionError(f"{form} {nx}x{ny}: {kernel!r} was planned, not {f['kernel']!r}")
    if "nt" in f["flags"] or "no_nt" in f["flags"]:
        assert kernel.endswith("<true>") == ("nt" in f["flags"]), kernel
    return p, obst, part


def _run(part, state, n):
    """n steps from the state on the context: the final cells, the per-step double sums and the steps of every launch."""
    part.set_cells(state)
    part.set_profile(True)
    with np.errstate(all="ignore"):
        av = part.run(n)
        sums = part.step_collect(n)
        launches = [k for k, _ in part.launch_profile()]
        cells = part.get_cells()
        inv = np.float64(np.float32(1.0) / np.float32(part.free_cells))
        assert np.array_equal(av, (sums * inv).astype(np.float32), equal_nan=True), "av_vels are these sums times free_cells_inv"
    return cells, sums, launches


# ---- without a GPU -----------------------------------------------------------------------------------------------------------------

def _nan_share(cells, obst):
    return float(np.mean(np.isnan(cells).any(axis=2)[obst == 0]))


def _denormal(a):
    return (a != 0) & (np.abs(a) < tc.MIN_NORMAL)


def test_states_reach_what_they_are_for():
    """What a case may leave out, bounded from the reference alone (at most half of the free cells NaN, and so on), for every (grid, state, steps) a GPU test runs."""
    lines, failures = [], []

    def record(ok, line):
        lines.append(line)
        if not ok:
            failures.append(line)

    grids = set()
    for name, nx, ny, n, fused in _runs():
        p, obst = _deck(nx, ny)
        grids.add((nx, ny))
        cells, terms = _reference(name, nx, ny, n, fused)
        arith = "fused" if fused else "exact"
        if name == "W1":
            finite = bool(np.isfinite(cells).all())
            with np.errstate(all="ignore"):
                pulled = terms_ref.pulled(terms_ref.accelerated(p, obst, _state(name, nx, ny)))
            fed = int(np.sum(_denormal(pulled).any(axis=2) & (obst == 0)))
            record(finite and fed > 0 and all(np.isfinite(t).all() for t in terms),
                   f"W1 {nx}x{ny} {n} steps ({arith}): every population finite: {finite}; {fed} free cells pull a denormal in step 1; largest |population| 2^{math.log2(float(np.abs(cells).max())):.1f}")
        elif name in ("W2", "W2 long"):
            share = _nan_share(cells, obst)
            record(0 < share <= 0.5, f"{name} {nx}x{ny} {n} steps ({arith}): {share:.2%} of the free cells hold a NaN")
    for nx, ny in sorted(grids):
        p, obst = _deck(nx, ny)
        free = obst == 0
        # blocks, step 1: the three things the patches are for, each counted
        msq, rinv = _inputs("blocks", nx, ny, 0)
        after, _ = _reference("blocks", nx, ny, 1)
        fine = np.isfinite(after).all(axis=2)
        den_ok = int(np.sum(free & _denormal(rinv) & fine))
        inf_r = int(np.sum(free & np.isinf(rinv)))
        nans = int(np.sum(free & np.isnan(after).any(axis=2)))
        odd = sum(1 for (y, x) in _patches(nx, ny) if x % 2)
        record(den_ok > 0 and inf_r > 0 and nans > 0 and odd > 0 and all(y <= ny - 2 - 3 or y > ny - 2 for y, _ in _patches(nx, ny)),
               f"blocks {nx}x{ny}: {den_ok} free cells with a denormal reciprocal and a finite result, {inf_r} with an infinite reciprocal, {nans} NaN cells after step 1; {odd} patches start at an odd x")
        # recip, step 1: densities outside the short reciprocal whose results the reciprocal decides
        with np.errstate(all="ignore"):
            rho, _, _ = terms_ref.moments(terms_ref.pulled(terms_ref.accelerated(p, obst, _state("recip", nx, ny))))
            _, rinv = _inputs("recip", nx, ny, 0)
        after, _ = _reference("recip", nx, ny, 1)
        low = int(np.sum(free & _denormal(rho) & np.isfinite(rinv) & np.isfinite(after).all(axis=2)))
        high = int(np.sum(free & _denormal(rinv) & np.isneginf(after[:, :, 0])))
        record(low >= 2 and high >= 2, f"recip {nx}x{ny}: {low} free cells with a denormal density, a finite reciprocal and finite results, {high} with a denormal reciprocal and population 0 = -inf after step 1")
        # accel: every kind met on a free cell, accelerated or refused as listed; some of the cells blocked
        s = _state("accel", nx, ny)
        with np.errstate(all="ignore"):
            acc = terms_ref.accelerated(p, obst, s)
        changed = (_bits(acc)[ny - 2] != _bits(s)[ny - 2]).any(axis=1)
        kinds = np.array([_accel_kind(x) for x in range(nx)])
        row_free = free[ny - 2]
        counts, ok = [], True
        for k, taken in enumerate(ACCEL_TAKEN):
            sel = row_free & (kinds == k)
            counts.append(f"{ACCEL_KINDS[k]}: {int(changed[sel].sum())} of {int(sel.sum())}")
            ok = ok and sel.any() and bool(np.all(changed[sel] == taken))
        blocked = int(np.sum(~row_free))
        assert not changed[~row_free].any()
        record(ok and blocked > 0, f"accel {nx}x{ny}: accelerated cells per kind: {'; '.join(counts)}; {blocked} cells of the row blocked")
        # moved: every pattern into a blocked cell, and there after one step, bounced
        src = _sources_of_blocked(p, obst)
        s = _state("moved", nx, ny)
        after, _ = _reference("moved", nx, ny, 1)
        hit = np.zeros(MOVED.size, int)
        for (y, x, k, ys, xs, i) in src:
            assert _bits(s)[ys, xs, k] == MOVED[i] and _bits(after)[y, x, BACK[k]] == MOVED[i], (y, x, k)
            hit[i] += 1
        record(hit.min() > 0, f"moved {nx}x{ny}: patterns fed into blocked cells {hit.tolist()}")
    print("\n".join("  " + line for line in lines))
    assert not failures, failures


def test_compare_takes_each_case():
    """_compare_cells and _compare_sums on hand-made arrays: what each branch accepts and what it refuses."""
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    obst = np.array([[0, 1]], np.int32)
    ref = np.zeros((1, 2, 9), np.float32)
    ref[0, 0, :3] = (1.0, nan, -0.0)
    _bits(ref)[0, 1, 0] = 0x7FA0ABCD                      # a signalling NaN in the blocked cell
    quiet = ref.copy()
    _bits(quiet)[0, 1, 0] = 0x7FE0ABCD                    # the same NaN quieted
    other_nan = ref.copy()
    _bits(other_nan)[0, 0, 1] = 0xFFC00000                # a free cell's NaN with another sign and payload: the same place
    _compare_cells(ref.copy(), ref, "same", obst, True)
    _compare_cells(other_nan, ref, "NaN by place", obst, True)
    _compare_cells(quiet, ref, "quieted, later steps", obst, False)
    moved_nan, plus_zero, last_bit = ref.copy(), ref.copy(), ref.copy()
    moved_nan[0, 0, 1], moved_nan[0, 0, 3] = 0.0, nan
    plus_zero[0, 0, 2] = 0.0
    _bits(last_bit)[0, 0, 0] += 1
    for bad, every in ((quiet, True), (moved_nan, False), (plus_zero, False), (last_bit, False)):
        with pytest.raises(AssertionError):
            _compare_cells(bad, ref, "refused", obst, every)

    free2 = np.zeros((1, 2), np.int32)
    D = (TREE_DEPTH["step"] + 2) * U

    def sums(dev, *terms, form="double", inputs=None):
        return _compare_sums(np.array(dev, np.float64), [np.array([t], np.float64) for t in terms], free2, "step", form, "hand-made", inputs)

    assert sums([np.nan], [1.0, np.nan]) == (1, 0, 0, 0)
    assert sums([np.nan], [np.inf, -np.inf]) == (1, 0, 0, 0)
    assert sums([np.inf], [np.inf, 1.0]) == (0, 1, 0, 0)
    assert sums([np.nan], [np.inf, 1.0]) == (0, 1, 0, 0)             # finite partial sums may have met it the other way round
    assert sums([3.0 * (1 + D / 2)], [1.0, 2.0]) == (0, 0, 1, 0)
    assert sums([4.0 * D], [2.0, -2.0]) == (0, 0, 1, 0)              # signed terms that cancel: relative to the magnitudes
    for dev, terms in (([np.inf], [1.0, np.nan]), ([1.0], [np.inf, -np.inf]), ([1.0], [np.inf, 1.0]), ([3.0 * (1 + 2 * D)], [1.0, 2.0]),
                       ([8.0 * D], [2.0, -2.0]), ([np.nan], [1.0, 2.0])):
        with pytest.raises(AssertionError):
            sums(dev, terms)
    # the two float forms: msq = 2^-20, rinv = 4 and 8 (terms 2^-8, 2^-7); msq a denormal: an under-estimate / exactly 0
    msq = np.array([[2.0 ** -20, 2.0 ** -20]], np.float32)
    rinv = np.array([[4.0, 8.0]], np.float32)
    term = terms_ref.term_of(msq, rinv)[0]
    total = float(term.sum())
    give = lambda m, r: (lambda t: (m, r))
    assert sums([total * (1 + tc.B_COMP / 2)], term, form="compensated", inputs=give(msq, rinv)) == (0, 0, 1, 0)
    assert sums([total * (1 + B_FAST / 2)], term, form="float", inputs=give(msq, rinv)) == (0, 0, 1, 0)
    low = np.array([[2.0 ** -130, 2.0 ** -130]], np.float32)
    low_term = terms_ref.term_of(low, rinv)[0]
    assert sums([float(low_term.sum()) / 2], low_term, form="compensated", inputs=give(low, rinv)) == (0, 0, 1, 0)
    assert sums([0.0], low_term, form="float", inputs=give(low, rinv)) == (0, 0, 1, 0)
    assert sums([-float(low_term.sum()) / 2], -low_term, form="compensated", inputs=give(low, -rinv)) == (0, 0, 1, 0)          # mirrored
    with pytest.raises(AssertionError):
        sums([float(low_term.sum()) / 2], -low_term, form="compensated", inputs=give(low, -rinv))
    tiny = np.array([[2.0 ** -140, 8.0]], np.float32)                  # a denormal reciprocal: no bound stated
    tiny_term = terms_ref.term_of(msq, tiny)[0]
    assert sums([float(tiny_term.sum())], tiny_term, form="compensated", inputs=give(msq, tiny)) == (0, 0, 0, 1)
    for dev, m, t, form in (([total * (1 + 2 * tc.B_COMP)], msq, term, "compensated"), ([total * (1 + 2 * B_FAST)], msq, term, "float"),
                            ([float(low_term.sum()) * 1.01], low, low_term, "compensated"), ([float(low_term.sum())], low, low_term, "float")):
        with pytest.raises(AssertionError):
            sums(dev, t, form=form, inputs=give(m, rinv))


def test_launch_plans_of_the_cases(lbm):
    """Every lbm_multi_kernel case's longest runs are more than one launch (a full launch and a tail), by the host-only plan."""
    for form, f in FORMS.items():
        if f["family"] == "multi":
            split = expected_launches(lbm, form, f["steps"][-1])
            assert len(split) >= 2 and sum(split) == f["steps"][-1] and max(split) <= max(f["k"], 4), (form, split)
            assert expected_launches(lbm, form, 1) == [1]


# ---- the kernels -------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("form,nx,ny", CASES)
def test_kernels_on_edge_states(lbm, monkeypatch, form, nx, ny, state):
    """One step, then the form's longer runs (a full launch, a full launch and a tail), each from the state of that step count."""
    f = FORMS[form]
    fused = "fused" in f["flags"]
    p, obst, part = _context(lbm, monkeypatch, form, nx, ny)
    with part:
        for n in f["steps"]:
            name = state_for(state, nx, ny, n)
            if name is None:
                continue
            ref, terms = _reference(name, nx, ny, n, fused)
            cells, sums, launches = _run(part, _state(name, nx, ny), n)
            what = f"{form} {nx}x{ny} {name} {n} steps"
            assert launches == expected_launches(lbm, form, n), (what, launches)
            _compare_cells(cells, ref, what, obst, every_bit_blocked=(n == 1))
            counts = _compare_sums(sums, terms, obst, f["family"], f["terms"], what, functools.partial(_inputs, name, nx, ny, fused=fused))
            if name in ("W1", "blocks"):
                assert counts[3] == 0, f"{what}: every finite step of this state has a stated bound"
            if name == "W1":
                assert counts == (0, 0, n, 0)


def _assemble_rows(parts):
    return np.concatenate([part.get_cells() for part in parts], axis=0)


@pytest.mark.gpu
@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("vector", [True, False])
def test_row_partitions_split_phase(lbm, monkeypatch, vector, state):
    """Three row partitions of 64 x 48 stepped through the split-phase calls (interior, boundary, halo buffers), exchanged by device
    copies as tests/test_gpu_parity.py test_row_partitioned_stepping_equals_single_partition does; the assembled rows against the
    whole-grid reference.  The 1024 cells of a partition take the narrow form by default, the vector form with LBM_TUNE_NARROW_MAX=0."""
    import torch
    import test_gpu_parity as gp
    (nx, ny), size, _, steps = ROW_SPLIT
    for knob in KNOBS:
        monkeypatch.delenv(knob, raising=False)
    if vector:
        monkeypatch.setenv("LBM_TUNE_NARROW_MAX", "0")
    p, obst = _deck(nx, ny)
    name = state_for(state, nx, ny, steps)
    cells0 = _state(name, nx, ny)
    ref, terms = _reference(name, nx, ny, steps)
    lp = lbm.Params(nx, ny, p.max_iters, p.reynolds_dim, p.density, p.accel, p.omega)
    free = lbm.count_free_cells(obst)
    ny_local, displs = lbm.decompose(ny, size)
    dev = torch.device("cuda", 0)
    parts = []
    try:
        for r in range(size):
            part = lbm.Partition(lp, free, obst[displs[r]:displs[r] + ny_local[r]], displs[r])
            part.bind_halo_tensors(dev)
            part.set_cells(cells0[displs[r]:displs[r] + ny_local[r]])
            parts.append(part)
        assert all(part.describe()["kernel"].startswith("lbm_step_kernel<" if vector else "lbm_step_kernel_narrow<") for part in parts), parts[0].describe()
        torch.cuda.synchronize()
        tstream = torch.cuda.Stream(dev)
        stream = tstream.cuda_stream
        with torch.cuda.stream(tstream), np.errstate(all="ignore"):
            for part in parts:
                part.step_prepare(steps, stream)
            for _ in range(steps):
                gp._ring_exchange(parts)
                for part in parts:
                    part.step_interior(stream)
                    part.step_boundary(stream)
                    part.step_finish(stream)
            per_part = [part.step_collect(steps, stream) for part in parts]
        tstream.synchronize()
        cells = _assemble_rows(parts)
    finally:
        for part in parts:
            part.close()
    what = f"{size} row partitions of {nx}x{ny}, split phase, {name} {steps} steps"
    _compare_cells(cells, ref, what)
    with np.errstate(all="ignore"):
        sums = sum(per_part)
    counts = _compare_sums(sums, terms, obst, "step", "double", what, extra=size - 1)          # the partitions' sums added on the host
    if name == "W1":
        assert counts == (0, 0, steps, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("grid,size,K,steps", ROW_K_STEP)
def test_k_step_row_partitions(lbm, monkeypatch, grid, size, K, steps, state):
    """K-step row partitions as contexts of one process: ghost rows, grouped launches (tests/test_gpu_parity.py
    _k_step_partitions_in_process); the assembled rows against the whole-grid reference."""
    import test_gpu_parity as gp
    nx, ny = grid
    for knob in KNOBS:
        monkeypatch.delenv(knob, raising=False)
    monkeypatch.setenv("LBM_TUNE_MACRO_K", str(K))
    p, obst = _deck(nx, ny)
    name = state_for(state, nx, ny, steps)
    cells0 = _state(name, nx, ny)
    ref, terms = _reference(name, nx, ny, steps)
    lp = lbm.Params(nx, ny, p.max_iters, p.reynolds_dim, p.density, p.accel, p.omega)
    free = lbm.count_free_cells(obst)
    ny_local, displs = lbm.decompose(ny, size)
    parts = [lbm.Partition(lp, free, obst[displs[r]:displs[r] + ny_local[r]], displs[r], obstacles_global=obst) for r in range(size)]
    try:
        assert all(part.macro_steps == K for part in parts), [part.macro_steps for part in parts]
        assert all(part.describe()["kernel"] == f"lbm_multi_kernel<{K}>" for part in parts), parts[0].describe()
        for r, part in enumerate(parts):
            part.set_cells(cells0[displs[r]:displs[r] + ny_local[r]])
        with np.errstate(all="ignore"):
            sums = gp._k_step_partitions_in_process(lbm, parts, steps, K)
        cells = _assemble_rows(parts)
    finally:
        for part in parts:
            part.close()
    what = f"{size} K-step row partitions of {nx}x{ny}, K = {K}, {name} {steps} steps"
    _compare_cells(cells, ref, what)
    counts = _compare_sums(sums, terms, obst, "parts", "compensated", what, functools.partial(_inputs, name, nx, ny))
    if name in ("W1", "blocks"):
        assert counts[3] == 0
    if name == "W1":
        assert counts == (0, 0, steps, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("case", TILE_RANKS)
def test_tile_ranks_in_one_process(lbm, case):
    """The ranks of a tile decomposition as contexts of one process (tests/float_edges_tile_worker.py, a fresh process with a hardware
    queue per rank as tests/test_gpu_parity.py test_tile_decomposition_in_one_process starts its worker): ghost columns, and ghost
    rows where py > 1; every state, the blocks set with set_cells, assembled and compared with the whole-grid reference."""
    import os
    import subprocess
    import sys
    from conftest import ROOT
    env = dict(os.environ, GPU_MAX_HW_QUEUES="16", LBM_P2P_TIMEOUT_MS="10000")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "float_edges_tile_worker.py"), *(str(v) for v in case)],
                       capture_output=True, text=True, timeout=600, env=env)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "EDGE TILES ok" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
