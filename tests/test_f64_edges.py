"""Every built kernel of the double-precision mode on states a lattice run never holds: exponents that sweep from the denormals to the
largest doubles across the grid, random signs, patches of zeros, of the smallest denormal, of 2^1020 and of -0.0, and special bit
patterns that stream into blocked cells.  tests/test_f64_cells.py holds the per-cell function to the restatement in a kernel of its
own; here the shipped kernels run, each forced as its own test file forces it and named by describe(), for one step and for a full
launch plus a tail, against tests/f64_ref.c.  The nine steps of the H = 8 tile geometries start from sweeps with a lower crest
(state_for), so that what the states are meant to reach holds after every step count that is run.

The comparison rule is that of tests/test_f64_cells.py: equal sets of NaNs; equal bits wherever the reference holds a number; every bit
at blocked cells.  It is sound over several steps: the update has no min, max or abs and every comparison with a NaN is false on both
sides, so the set of NaN cells propagates identically.

av_vels, by what f64_ref.run_report says of the step's terms:
  some term a NaN, or infinities of both signs   the device's entry is a NaN (whatever the order of additions);
  infinite terms of one sign only                the device's entry is not finite (a sum cannot return from an infinity).  The restatement's
                                                 compensated sum is a NaN here, the device's plain sum an infinity: counted as "left out";
  every density positive, every term finite      the bound of the launch's summation tree, relative to the sum: the terms are non-negative;
  every term finite, some density not positive   terms of both signs: the same chain of additions errs by at most the same multiple of
                                                 2^-53 of the sum of the terms' MAGNITUDES (each addition by 2^-53 of its result, which is
                                                 at most that sum).  No new tolerance: the same bound without the premise of one sign.

What the states reach is counted from the reference alone in test_states_reach_what_they_are_for (no GPU)."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import f64_ref
from test_f64 import U
from test_f64 import sum_bound as step_sum_bound
from test_f64_cells import _bits, _denormal, _make
from test_f64_multi import _force as force_multi
from test_f64_multi import _kernel_name as multi_kernel_name
from test_f64_multi import multi_sum_bound
from test_f64_tile import GEOMS
from test_f64_tile import _force as force_tile
from test_f64_tile import tile_sum_bound

DX = (0, 1, 0, -1, 0, 1, -1, -1, 1)
DY = (0, 0, 1, 0, -1, 1, 1, -1, -1)
BACK = (0, 3, 4, 1, 2, 7, 8, 5, 6)


@pytest.fixture(scope="module")
def f64(lbm):
    from mpilattice_boltzmann_amd import f64 as mod
    mod.load_library()
    return mod


# ---- decks and states, from numpy alone ------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _deck(nx, ny):
    """density 0.1, accel 0.005, omega 1.85; 10 % random obstacles, cleared where the patches of the "blocks" state go."""
    p = SimpleNamespace(nx=nx, ny=ny, max_iters=10, reynolds_dim=10, density=0.1, accel=0.005, omega=1.85)
    obst = (np.random.default_rng(1000 * nx + ny).random((ny, nx)) < 0.10).astype(np.int32)
    for y, x in PATCHES:
        obst[y - 1:y + 4, x - 1:x + 4] = 0
    # The corner where W1's and W2's exponents are lowest: blocked, these five cells keep the denormal rest populations they start with
    # (a free cell's populations take the scale of its largest neighbour within a step), so denormals stream out of them in every step.
    # The denormals the reach test counts are these: held or streamed, not made by arithmetic in a free cell.
    obst[[ny - 2, ny - 1, 0, 1, 2], 0] = 1
    obst.setflags(write=False)
    return p, obst


PATCHES = ((2, 2), (2, 12), (9, 20), (9, 27))         # top-left cells of the 3 x 3 patches (rows 2..4 and 9..11: not the accelerated row)
PATCH_BITS = (0x0000000000000000, 0x0000000000000001, 0x7FB0000000000000, 0x8000000000000000)    # 0.0, 5e-324, 2^1020, -0.0


def _tri(n):
    """The periodic triangle 1 - |2 i / n - 1|: 0 at i = 0, 1 at i = n / 2, and back, so that the wrap is smooth."""
    return 1.0 - np.abs(2.0 * np.arange(n) / n - 1.0)


def _wide(nx, ny, lo, hi, signs, seed):
    """One exponent per cell, rint(lo + (hi - lo) * (0.8 tri(x) + 0.2 tri(y))); each population within 2 binades of it, a random significand."""
    rng = np.random.default_rng(seed)
    e = np.rint(lo + (hi - lo) * (0.8 * _tri(nx)[None, :] + 0.2 * _tri(ny)[:, None])).astype(np.int64)
    e = e[:, :, None] + rng.integers(-2, 3, (ny, nx, 9))
    sig = rng.integers(0, 1 << 52, (ny, nx, 9), dtype=np.uint64)
    neg = rng.integers(0, 2, (ny, nx, 9)) if signs else None
    return _make(e, sig, neg)


# W1 and W2 are the issue's states, with its figures for runs of up to 5 steps.  The H = 8 tile geometries run H + 1 = 9 steps, where W1
# (hi = 500) overflows in a few cells and W2's NaNs, which spread by one cell per step from wherever the exponents pass 2^511, cover
# 84 % of a 32 x 16 grid.  Runs of more than LONG steps therefore start from the same recipes with the upper exponent lowered to
# LONG_HI = 300, at which nine steps stay finite (measured with f64_ref.run: every hi from 300 down to -300 does, 500 does not); "W2
# long" keeps W2's own values, up to 2^1010, in the LONG_BAND = 2 columns at the crest of the triangle, so that its NaNs start there
# and after nine steps cover 2 + 2 * 9 = 20 columns: 62.5 % of 32, 31 % of 64.
LONG, LONG_HI, LONG_BAND = 5, 300, 2


def state_for(state, n):
    """The state a run of n steps starts from."""
    return f"{state} long" if state in ("W1", "W2") and n > LONG else state


def _benign(p, seed):
    return f64_ref.initial_cells(p) * np.random.default_rng(seed).uniform(0.8, 1.2, (p.ny, p.nx, 9))


MOVED = np.array([0x7FF4000000ABCDEF, 0xFFF0000012345678 | 1 << 50, 0x7FF0000000000001, 0x0000000000000001, 0x800FFFFFFFFFFFFF,
                  0x0000000000000ABC, 0x8000000000000000, 0x7FF0000000000000, 0xFFF0000000000000], np.uint64)
# signalling NaNs with payloads (0x7FF4..., 0xFFF4..., 0x7FF0...01), denormals, -0.0, +-inf


def _sources_of_blocked(p, obst):
    """(y, x, k, ys, xs): population k of blocked cell (y, x) streams in from cell (ys, xs); sources on the accelerated row are left out
    (accelerate_flow may rewrite them before the step)."""
    out = []
    for y, x in np.argwhere(obst != 0):
        for k in range(9):
            ys, xs = (y - DY[k]) % p.ny, (x - DX[k]) % p.nx
            if ys != p.ny - 2:
                out.append((int(y), int(x), k, int(ys), int(xs)))
    return out


@functools.lru_cache(maxsize=None)
def _state(name, nx, ny):
    p, obst = _deck(nx, ny)
    if name == "W1":
        s = _wide(nx, ny, -1060, 500, False, 31)
    elif name == "W2":
        s = _wide(nx, ny, -1060, 1010, True, 32)
    elif name == "W1 long":
        s = _wide(nx, ny, -1060, LONG_HI, False, 31)
    elif name == "W2 long":
        s = _wide(nx, ny, -1060, LONG_HI, True, 32).copy()
        x0 = nx // 2 - LONG_BAND // 2
        s[:, x0:x0 + LONG_BAND] = _wide(nx, ny, -1060, 1010, True, 32)[:, x0:x0 + LONG_BAND]
    elif name == "blocks":
        s = _benign(p, 33)
        for (y, x), b in zip(PATCHES, PATCH_BITS):
            _bits(s)[y:y + 3, x:x + 3, :] = np.uint64(b)
    elif name == "moved":
        s = _benign(p, 34)
        for i, (y, x, k, ys, xs) in enumerate(_sources_of_blocked(p, obst)):
            _bits(s)[ys, xs, k] = MOVED[i % MOVED.size]
    else:
        raise KeyError(name)
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def _reference(name, nx, ny, steps):
    p, obst = _deck(nx, ny)
    with np.errstate(all="ignore"):
        cells, exact, status, mags = f64_ref.run_report(p, obst, steps, cells0=_state(name, nx, ny))
    assert np.array_equal(np.isnan(exact), (status & ~f64_ref.POSITIVE) != 0)
    for a in (cells, exact, status, mags):
        a.setflags(write=False)
    return cells, (exact, status, mags)


def _left_out(report):
    """av_vels entries that can only be held to "not finite": infinite terms of one sign and no NaN."""
    exact, status, mags = report
    inf = status & (f64_ref.POS_INF_TERM | f64_ref.NEG_INF_TERM)
    return int(np.sum(((inf == f64_ref.POS_INF_TERM) | (inf == f64_ref.NEG_INF_TERM)) & (status & f64_ref.NAN_TERM == 0)))


# ---- the forms ---------------------------------------------------------------------------------------------------------------------

def _step_form(flag, kernel, shapes):
    return dict(kind="step", flag=flag, kernel=kernel, shapes=shapes, steps=(1, 5))


FORMS = {"step<1>": _step_form(None, "lbm_step_kernel_f64<1>", ((33, 16),)),
         "step<2>": _step_form("FLAG_NO_NT_STORES", "lbm_step_kernel_f64<2>", ((32, 16), (64, 48))),
         "step<2,nt>": _step_form("FLAG_NT_STORES", "lbm_step_kernel_f64<2,nt>", ((32, 16), (64, 48)))}
for _T, _H in GEOMS:
    FORMS[f"tile<{_T},{_H}>"] = dict(kind="tile", geom=(_T, _H), kernel=f"lbm_tile_kernel_f64<{_T}, {_H}>", shapes=((32, 16), (64, 48)), steps=(1, _H + 1))
for _K in (2, 3, 4):
    FORMS[f"multi<{_K}>"] = dict(kind="multi", K=_K, kernel=multi_kernel_name(_K), shapes=((32, 16), (64, 48)), steps=(1, _K + 1))
CASES = [(form, nx, ny) for form, f in FORMS.items() for (nx, ny) in f["shapes"]]
STEP_COUNTS = {shape: sorted({n for f in FORMS.values() if shape in f["shapes"] for n in f["steps"]}) for shape in ((33, 16), (32, 16), (64, 48))}


def _grid(f64, monkeypatch, form, nx, ny):
    f = FORMS[form]
    p, obst = _deck(nx, ny)
    for knob in ("LBM_TUNE_TILE64_MAX", "LBM_TUNE_TILE64_GEOM", "LBM_TUNE_MULTI64_K", "LBM_TUNE_MULTI64_MIN", "LBM_TUNE_MAXBLOCKS"):
        monkeypatch.delenv(knob, raising=False)
    if f["kind"] == "step":
        flags = 0 if f["flag"] is None else getattr(f64, f["flag"])
    elif f["kind"] == "tile":
        force_tile(monkeypatch, *f["geom"])
        flags = f64.FLAG_TILE_STEPS
    else:
        force_multi(monkeypatch, f["K"])
        flags = f64.FLAG_MULTI_STEPS
    g = f64.Grid64(p, obst, flags=flags)
    desc = g.describe()
    assert desc["kernel"] == f["kernel"], desc             # a fallback cannot pass for the kernel
    if f["kind"] == "step":
        bound = step_sum_bound(desc)
    elif f["kind"] == "tile":
        bound = tile_sum_bound(*f["geom"], desc["blocks"])
    else:
        bound = multi_sum_bound(desc["blocks"])
    return p, obst, g, bound


def _compare_cells(got, ref, what):
    nan_ref, nan_got = np.isnan(ref), np.isnan(got)
    assert np.array_equal(nan_ref, nan_got), f"{what}: {int(np.sum(nan_ref != nan_got))} NaNs misplaced"
    differ = ~nan_ref & (_bits(got) != _bits(ref))
    assert not differ.any(), f"{what}: {int(differ.sum())} numbers differ, first at {tuple(np.argwhere(differ)[0])}"


def _compare_av(av, report, obst, bound, what):
    """The module docstring's four cases.  Returns how many entries fell under each."""
    exact, status, mags = report
    ref = f64_ref.av_vels(exact, obst)
    scale = f64_ref.av_vels(mags, obst)
    assert av.shape == ref.shape == status.shape
    both = f64_ref.POS_INF_TERM | f64_ref.NEG_INF_TERM
    n_nan = n_inf = n_pos = n_signed = 0
    worst = 0.0
    for t, st in enumerate(status.tolist()):
        if st & f64_ref.NAN_TERM or st & both == both:
            n_nan += 1
            assert np.isnan(av[t]), f"{what}: av_vels[{t}] = {av[t]!r} where a term is a NaN"
        elif st & both:
            n_inf += 1
            assert not np.isfinite(av[t]), f"{what}: av_vels[{t}] = {av[t]!r} where a term is infinite"
        else:
            positive = st == f64_ref.POSITIVE
            n_pos, n_signed = n_pos + positive, n_signed + (not positive)
            against = ref[t] if positive else scale[t]
            err = abs(av[t] - ref[t]) / against if against > 0 else abs(av[t] - ref[t])
            worst = max(worst, err)
            assert err <= bound, f"{what}: av_vels[{t}] off by {err / U:.2f} x 2^-53, bound {bound / U:.0f} x 2^-53 ({'non-negative' if positive else 'signed'} terms)"
    print(f"  {what}: av_vels {n_nan} NaN on both sides, {n_pos} + {n_signed} (non-negative + signed terms) within {worst / U:.2f} of {bound / U:.0f} x 2^-53, {n_inf} held to 'not finite' only")
    assert n_inf == _left_out(report)
    return n_nan, n_pos, n_signed, n_inf


# ---- what the states reach (no GPU) ------------------------------------------------------------------------------------------------

def test_states_reach_what_they_are_for():
    """After every step count a kernel test runs, from the state that run starts from (state_for).  W1: every cell finite, at least
    0.1 % of the cells holding a denormal, no av_vels entry left out.  W2: between 15 % and 65 % of the cells holding a NaN, at most
    half of the av_vels entries left out.
    (The denormals counted here sit in the blocked cells of the low corner (_deck) and in what streams out of them: a free cell's
    populations take the scale of its largest neighbour within a step.  Denormals made BY arithmetic are tests/test_f64_cells.py's
    classes B, C and the two with denormal weights.)"""
    lines, failures = [], []
    for (nx, ny), counts in STEP_COUNTS.items():
        for n in counts:
            name = state_for("W1", n)
            cells, report = _reference(name, nx, ny, n)
            finite = float(np.mean(np.isfinite(cells).all(axis=2)))
            den = float(np.mean(_denormal(cells).any(axis=2)))
            left = _left_out(report)
            lines.append(f"{name} {nx}x{ny} {n} steps: {finite:.4%} of cells finite, {den:.3%} hold a denormal (in or streamed from the blocked corner), "
                         f"{int(np.isnan(report[0]).sum())} av_vels entries not numbers, {left} of {n} left out")
            if not (finite == 1.0 and den >= 0.001 and left == 0):
                failures.append(lines[-1])
            name = state_for("W2", n)
            cells, report = _reference(name, nx, ny, n)
            nan = float(np.mean(np.isnan(cells).any(axis=2)))
            left = _left_out(report)
            lines.append(f"{name} {nx}x{ny} {n} steps: {nan:.2%} of cells hold a NaN, {left} of {n} av_vels entries left out")
            if not (0.15 <= nan <= 0.65 and 2 * left <= n):
                failures.append(lines[-1])
    print("\n".join("  " + line for line in lines))
    assert not failures, failures


def test_compare_av_takes_each_case():
    """_compare_av's four cases on hand-made reports, the one no recorded run reaches (infinite terms of one sign) among them: what
    each accepts and what it refuses."""
    obst = np.zeros((2, 2), np.int32)                       # 4 free cells: av_vels = sum * 0.25
    P, N, PI, NI = f64_ref.POSITIVE, f64_ref.NAN_TERM, f64_ref.POS_INF_TERM, f64_ref.NEG_INF_TERM
    inf, nan = np.inf, np.nan

    def report(exact, status, mags):
        return np.array(exact), np.array(status, np.int32), np.array(mags)

    good = [(report([nan], [P | N], [nan]), [nan]),                      # a NaN term
            (report([nan], [PI | NI], [inf]), [nan]),                    # infinities of both signs
            (report([nan], [P | PI], [inf]), [inf]),                     # +inf alone: the plain sum is +inf
            (report([nan], [P | PI], [inf]), [nan]),                     # ... or a NaN, had finite partial sums overflowed the other way
            (report([4.0], [P], [4.0]), [1.0 + 8 * U]),                  # non-negative terms, within the bound of the sum
            (report([0.0], [0], [4.0]), [8 * U])]                        # signed terms that cancel: within the bound of the magnitudes
    for rep, av in good:
        _compare_av(np.array(av), rep, obst, 8 * U, "hand-made")
    bad = [(report([nan], [P | N], [nan]), [inf]), (report([nan], [PI | NI], [inf]), [inf]), (report([nan], [P | PI], [inf]), [1.0]),
           (report([4.0], [P], [4.0]), [1.0 + 16 * U]), (report([0.0], [0], [4.0]), [16 * U]), (report([4.0], [P], [4.0]), [nan])]
    for rep, av in bad:
        with pytest.raises(AssertionError):
            _compare_av(np.array(av), rep, obst, 8 * U, "hand-made")
    assert _left_out(report([nan, nan, 4.0], [P | PI, PI | NI, P], [inf, inf, 4.0])) == 1


def test_moved_state_is_what_it_says():
    """The "moved" state: every population that streams into a blocked cell from outside the accelerated row is one of MOVED."""
    for nx, ny in STEP_COUNTS:
        p, obst = _deck(nx, ny)
        s, src = _state("moved", nx, ny), _sources_of_blocked(p, obst)
        assert len(src) > 9 * MOVED.size and all(_bits(s)[ys, xs, k] in MOVED for (_, _, k, ys, xs) in src)
        ref, _ = _reference("moved", nx, ny, 1)
        hit = np.zeros(MOVED.size, int)
        for (y, x, k, ys, xs) in src:
            assert _bits(ref)[y, x, BACK[k]] == _bits(s)[ys, xs, k]
            hit[int(np.flatnonzero(MOVED == _bits(s)[ys, xs, k])[0])] += 1
        assert hit.min() > 0


# ---- the kernels -------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("state", ["W1", "W2", "blocks"])
@pytest.mark.parametrize("form,nx,ny", CASES)
def test_kernels_on_edge_states(f64, monkeypatch, form, nx, ny, state):
    """One step, then a full launch plus a tail: H + 1 or K + 1 steps, 5 for the one-step kernel; each from the state of that step
    count (state_for: beyond 5 steps W1 and W2 with their upper exponents lowered)."""
    p, obst, g, bound = _grid(f64, monkeypatch, form, nx, ny)
    with g:
        for n in FORMS[form]["steps"]:
            name = state_for(state, n)
            ref, report = _reference(name, nx, ny, n)
            g.set_cells(_state(name, nx, ny))
            with np.errstate(all="ignore"):
                av = g.run(n)
            what = f"{form} {nx}x{ny} {name} {n} steps"
            _compare_cells(g.get_cells(), ref, what)
            left = _compare_av(av, report, obst, bound, what)[3]
            if state == "W1":
                assert left == 0
            if state == "W2":
                assert 2 * left <= n
            if state == "blocks":
                assert np.isnan(ref).any() and not np.isnan(ref).all()


@pytest.mark.gpu
@pytest.mark.parametrize("form,nx,ny", CASES)
def test_blocked_cells_move_bits(f64, monkeypatch, form, nx, ny):
    """After one step a blocked cell holds exactly the bit patterns that streamed in, permuted by the bounce-back: signalling NaNs keep
    their payloads and stay signalling, denormals, -0.0 and the infinities arrive as they left.  Free cells beside them by the rule."""
    p, obst, g, bound = _grid(f64, monkeypatch, form, nx, ny)
    state = _state("moved", nx, ny)
    ref, report = _reference("moved", nx, ny, 1)
    with g:
        g.set_cells(state)
        with np.errstate(all="ignore"):
            av = g.run(1)
        got = g.get_cells()
    for (y, x, k, ys, xs) in _sources_of_blocked(p, obst):
        assert _bits(got)[y, x, BACK[k]] == _bits(state)[ys, xs, k], (y, x, k)
    blocked = obst != 0
    assert np.array_equal(_bits(got)[blocked], _bits(ref)[blocked])            # every bit, NaNs included: no arithmetic happened
    _compare_cells(got, ref, f"{form} {nx}x{ny} moved")
    _compare_av(av, report, obst, bound, f"{form} {nx}x{ny} moved")
