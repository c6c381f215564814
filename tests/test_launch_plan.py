"""What every launch of a run covers — checked on a CPU through the planning unit's launch entry points (csrc/lbm_plan.cpp: lbm_plan_launch,
lbm_plan_run_launches, declared in csrc/lbm_internal.h).

Two checks.  The properties: every LaunchPlan of every group of runs of 1, 4, 7, 11 and 20 steps against a brute-force restatement, tile
by tile, written here from the tile heights, the column reach of a sub-step and the owned rectangle — not taken from the planner.  The
recording: the kernel name, grid and workgroup each LaunchPlan stands for against tests/golden/launches_parent.json, the dispatches
tests/launch_cases.py traced on an MI355X at the commit named inside the file."""
import ctypes as C
import json
import os

import pytest

import launch_cases
import plan_cases
from test_plan import CPlan, ROOT, planner  # noqa: F401  (planner: the fixture that declares the lbm_plan_* context entry points)
from test_tile_split_phase import LAYOUTS

GOLDEN = os.path.join(ROOT, "tests", "golden", "launches_parent.json")
RUNS = (1, 4, 7, 11, 20)
WHOLE, INTERIOR, EDGE = 0, 1, 2
SERIAL, SCHEDULE_EDGE = 0, 1
PART_PLAIN, PART_GHOST, PART_READY, PART_TILE = 0, 1, 2, 3
GEOM_STD, GEOM_NARROW, GEOM_TALL = 0, 1, 2
KNOBS = sorted(set(launch_cases.TUNE) | {knob for knob, _, _ in plan_cases.KNOBS})
TILE_BLOCK = {(8, 8): 512, (16, 8): 512, (16, 4): 320, (8, 4): 128}       # kernels/tile.h TileGeom<T, H>::block


class CRect(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("ty0", "tx0", "ntx", "count")]


class CLaunch(C.Structure):
    """struct LaunchPlan (csrc/lbm_internal.h), field for field."""

    _fields_ = ([(n, C.c_int) for n in ("k", "ext", "row_first", "rows_compute", "rows_storage", "count_first", "count_end",
                                        "cx0", "cx1", "keep_x0", "keep_x1", "y_periodic", "y0_global", "tiles_x", "ntiles_total",
                                        "tile_begin", "tile_count", "tile_begin2", "tile_count2", "nrect")] + [("rect", CRect * 4)] +
                [(n, C.c_int) for n in ("nblocks", "launched_blocks", "xcd_remap", "part", "row", "lanes", "full")])

    def key(self):
        return tuple(getattr(self, n) for n, t in self._fields_ if t is C.c_int) + tuple((r.ty0, r.tx0, r.ntx, r.count) for r in self.rect)


@pytest.fixture(scope="module")
def launcher(planner):
    lib, P = planner, C.POINTER
    lib.lbm_plan_launch_sizeof.restype, lib.lbm_plan_launch_sizeof.argtypes = C.c_int, []
    lib.lbm_plan_launch.restype, lib.lbm_plan_launch.argtypes = C.c_int, [P(CPlan), C.c_int, C.c_int, C.c_int, C.c_int, P(CLaunch)]
    lib.lbm_plan_run_launches.restype, lib.lbm_plan_run_launches.argtypes = C.c_int, [P(CPlan), C.c_int, C.c_int, P(CLaunch), C.c_int]
    lib.lbm_plan_edge_rows_suffice.restype, lib.lbm_plan_edge_rows_suffice.argtypes = C.c_int, [P(CPlan), C.c_int]
    assert lib.lbm_plan_launch_sizeof() == C.sizeof(CLaunch), "CLaunch above is not the library's LaunchPlan"
    return lib


@pytest.fixture
def no_knobs(monkeypatch):
    for knob in KNOBS:
        monkeypatch.delenv(knob, raising=False)
    return monkeypatch


# ---- the contexts ----------------------------------------------------------------------------------------------------------------

def _plan(lbm, lib, kind, p, env, monkeypatch, **kw):
    """The ContextPlan of a whole grid, a one-rank ring or a tile rank, made with `env` in the environment."""
    from mpilattice_boltzmann_amd import host
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cp, plan = host._cparams(p), CPlan()
    if kind == "whole":
        rc = lib.lbm_plan_whole(C.byref(cp), p.nx * p.ny, 0, p.ny, 0, 0, C.byref(plan))
    elif kind == "ring":
        rc = lib.lbm_plan_rank(C.byref(cp), p.nx * p.ny, 1, 0, lbm._capi.FLAG_FORCE_HALO, C.byref(plan))
    else:
        rc = lib.lbm_plan_tile(C.byref(cp), p.nx * p.ny, kw["px"], kw["py"], kw["rank"], 0, C.byref(plan))
    for k in env:
        monkeypatch.delenv(k)
    assert rc == 0, lib.lbm_last_error().decode()
    return plan


def contexts(lbm, lib, monkeypatch):
    """(label, ContextPlan, knobs) of the rings, tile ranks and multi-kernel whole grids of plan_cases and of every rank of LAYOUTS."""
    out = []
    for case in plan_cases.cases():
        if case["flags"] not in ([], ["FLAG_FORCE_HALO"]) or case["env"] or case["nx"] * case["ny"] > 2048 * 1024:
            continue
        kw = {k: case[k] for k in ("px", "py", "rank") if k in case}
        out.append((json.dumps(case), _plan(lbm, lib, case["kind"], plan_cases.params_of(lbm, case), {}, monkeypatch, **kw), {}))
    for name, (nx, ny, px, py, env, *_) in LAYOUTS.items():
        p = lbm.Params(nx, ny, 26, 4, 0.1, 0.01, 1.7)
        out += [(f"{name} rank {r}", _plan(lbm, lib, "tile", p, env, monkeypatch, px=px, py=py, rank=r), env) for r in range(px * py)]
    return [(label, plan, env) for label, plan, env in out if plan.multi_K > 0 and (plan.self_periodic or plan.ghost > 0)]


def plan_launch(lib, plan, k, ext, which, says_ready=False):
    l = CLaunch()
    assert lib.lbm_plan_launch(C.byref(plan), k, ext, which, 1 if says_ready else 0, C.byref(l)) == 0, lib.lbm_last_error().decode()
    return l


def run_groups(lbm, lib, plan, n_steps, schedule):
    """The launches of a run as lbm_plan_run_launches gives them, cut into groups by host.plan_groups / host.plan_steps: a list of groups,
    each a list of (index in the group, which, LaunchPlan, does it say ready).  Every entry must be the lbm_plan_launch of its (k, ext, which, says_ready)."""
    from mpilattice_boltzmann_amd import host
    buf = (CLaunch * 64)()
    n = lib.lbm_plan_run_launches(C.byref(plan), n_steps, schedule, buf, 64)
    assert 0 <= n <= 64, lib.lbm_last_error().decode()
    got = [buf[i] for i in range(n)]
    if plan.ghost == 0:                                               # lbm_run: one launch per "group", nothing exchanged
        steps = host.plan_steps(plan.multi_K, n_steps)
        assert [l.k for l in got] == steps and all(l.ext == 0 for l in got)
        for l in got:
            assert l.key() == plan_launch(lib, plan, l.k, 0, WHOLE).key()
        return [[(0, WHOLE, l, False)] for l in got]
    groups, pos, left = [], 0, n_steps
    for steps in host.plan_groups(plan.multi_K, plan.ghost, plan.group_max, n_steps):
        assert sum(steps) <= plan.ghost and len(steps) <= plan.group_max      # a group's steps fit the ghost rows
        left -= sum(steps)
        group = []
        for i, k in enumerate(steps):
            ext = sum(steps[i + 1:])                                  # the steps of the later launches of the group
            if i == 0 and schedule == SCHEDULE_EDGE:
                interior = plan_launch(lib, plan, k, ext, INTERIOR)
                want = ([(0, INTERIOR, interior, False)] if interior.nblocks > 0 else []) + [(0, EDGE, plan_launch(lib, plan, k, ext, EDGE), False)]
            else:
                ready = len(steps) > 1 and i == len(steps) - 1 and left > 0      # the last launch of a group of several, when another group follows
                want = [(i, WHOLE, plan_launch(lib, plan, k, ext, WHOLE, ready), ready)]
            for _, which, l, _ in want:
                assert pos < n and got[pos].key() == l.key(), (n_steps, schedule, steps, i, which)
                assert (l.k, l.ext) == (k, ext)
                pos += 1
            group += want
        groups.append(group)
    assert pos == n and left == 0
    return groups


# ---- the restatement -------------------------------------------------------------------------------------------------------------

def multi_ty(k, geom):
    return (24 if geom == GEOM_TALL else 13) if k >= 4 else 16


def multi_ex(ey):
    return 2 * ((ey + 1) // 2)


def tiles_of(plan, k, ext):
    """Every tile of a launch of k steps + ext as (tile row, tile column, is it in the rim).  A tile is in the rim when its first sub-step —
    which reads k rows and multi_ex(k - 1) + 1 columns beyond the tile on each side — reads a row that is not an owned row (a rank with
    ghost rows: those are the exchanged rows, whatever part of them this launch advances itself) or a column that is not an owned column
    (a rank with ghost columns).  Where no tile column lies inside the owned columns by that reach, every tile is in the rim by this rule already."""
    ty, tx = multi_ty(k, plan.multi_geom), 32 if plan.multi_geom == GEOM_NARROW else 64
    ext_y = ext if plan.ghost_rows > 0 else 0
    first, rows = plan.ghost_rows - ext_y, plan.nyl + 2 * ext_y
    nty, ntx = -(-rows // ty), -(-plan.nx // tx)
    lo, hi, xlo, xhi = plan.ghost_rows, plan.ghost_rows + plan.nyl, plan.ghost_x, plan.ghost_x + plan.nxl
    reach = multi_ex(k - 1) + 1
    out = []
    for j in range(nty):
        r0, r1 = first + j * ty, min(first + (j + 1) * ty, first + rows)
        row_rim = plan.ghost_rows > 0 and (r0 - k < lo or r1 - 1 + k >= hi)
        for i in range(ntx):
            col_rim = plan.ghost_x > 0 and (i * tx - reach < xlo or (i + 1) * tx - 1 + reach >= xhi)
            out.append((j, i, row_rim or col_rim, (r0, r1)))
    return out, ntx, nty


def covered(l, ntx):
    """The (tile row, tile column) pairs a LaunchPlan covers, with multiplicity."""
    out = []
    if l.nrect > 0:
        assert l.tile_count == 0 and l.tile_count2 == 0
        for r in list(l.rect)[:l.nrect]:
            assert r.ntx > 0 and r.count % r.ntx == 0 and r.count > 0
            out += [(r.ty0 + q // r.ntx, r.tx0 + q % r.ntx) for q in range(r.count)]
    for begin, count in ((l.tile_begin, l.tile_count), (l.tile_begin2, l.tile_count2)):
        out += [(t // ntx, t % ntx) for t in range(begin, begin + count)]
    return out


def check_launch(plan, env, which, l, says_ready):
    tile_rank = plan.ghost_x > 0
    tiles, ntx, nty = tiles_of(plan, l.k, l.ext)
    assert (l.tiles_x, l.ntiles_total) == (ntx, ntx * nty) and len(tiles) == l.ntiles_total
    want = sorted((j, i) for j, i, rim, _ in tiles if which == WHOLE or rim == (which == EDGE))
    got = covered(l, ntx)
    assert sorted(got) == want, (which, l.k, l.ext)
    assert l.nblocks == len(got)
    # rows and columns
    assert 0 <= l.row_first and l.row_first + l.rows_compute <= l.rows_storage == plan.nyl + 2 * plan.ghost_rows
    assert (l.count_first, l.count_end) == (plan.ghost_rows, plan.ghost_rows + plan.nyl)
    assert l.keep_x0 % 2 == 0 and l.keep_x1 % 2 == 0 and 0 <= l.keep_x0 <= l.cx0 < l.cx1 <= l.keep_x1 <= plan.nx
    assert (l.cx0, l.cx1) == (plan.ghost_x, plan.ghost_x + plan.nxl)
    assert l.y_periodic == (1 if plan.self_periodic or plan.ghost_rows == 0 else 0)
    assert l.y0_global == plan.y0 - (plan.ghost_rows - l.row_first)
    # the grid
    remap_knob, pad_knob = env.get("LBM_TUNE_MULTI_REMAP", "1") != "0", env.get("LBM_TUNE_TILE_PAD_GRID", "1") != "0"
    padded = tile_rank and remap_knob and pad_knob and l.nblocks >= 64
    assert l.launched_blocks == (-(-l.nblocks // 8) * 8 if padded else l.nblocks)
    if l.xcd_remap:
        assert l.launched_blocks % 8 == 0 and l.launched_blocks >= 64
    assert l.xcd_remap == (1 if remap_knob and l.launched_blocks % 8 == 0 and l.launched_blocks >= 64 else 0)
    # the kernel
    assert l.part == (PART_TILE if tile_rank else PART_GHOST if l.ext > 0 else PART_READY if says_ready else PART_PLAIN)
    assert l.lanes == (768 if l.k >= 4 and plan.multi_geom == GEOM_TALL else 512) and l.full == 0


def kernel_of(plan, l):
    """(instantiation name, grid in work-items, workgroup) of a LaunchPlan, from its table row."""
    if plan.tile_kernel:
        terms, full, h, t = l.row % 3, l.row // 3 % 2, 4 if l.row // 6 % 2 else 8, 8 if l.row // 12 else 16
        assert (t, h, full, l.k <= h) == (plan.tile_T, plan.tile_H, l.full, True)
        block = TILE_BLOCK[(t, h)]
        name = f"lbm_tile_kernel<{t}, {h}, {'true' if full else 'false'}, {4 if terms == 2 else terms}>((anonymous namespace)::TileArgs)"
        return "void (anonymous namespace)::" + name, (l.launched_blocks + 1) * block, block
    part, terms, k, geom = l.row % 4, l.row // 4 % 4, l.row // 16 % 4 + 1, l.row // 64
    assert (part, k) == (l.part, min(l.k, 4)) and geom == plan.multi_geom
    name = f"lbm_multi_kernel<{k}, {6 if terms == 3 else terms}, {GEOM_STD if geom == GEOM_TALL and k < 4 else geom}, {part}>((anonymous namespace)::MultiArgs)"
    return "void (anonymous namespace)::" + name, (l.launched_blocks + 1) * l.lanes, l.lanes


# ---- 1. the properties -------------------------------------------------------------------------------------------------------------

def test_every_launch_covers_what_the_restatement_says(lbm, launcher, no_knobs):
    seen = set()
    ctxs = contexts(lbm, launcher, no_knobs)
    assert len(ctxs) >= 40 and {p.ghost for _, p, _ in ctxs} >= {0, 4, 7, 8, 16, 32} and any(p.ghost_x > 0 and p.ghost_rows == 0 for _, p, _ in ctxs)
    for label, plan, env in ctxs:
        for knob, value in env.items():
            no_knobs.setenv(knob, value)
        for n_steps in RUNS:
            for schedule in (SERIAL, SCHEDULE_EDGE):
                for group in run_groups(lbm, launcher, plan, n_steps, schedule):
                    for i, which, l, says_ready in group:
                        key = (label, which, says_ready, l.key())
                        if key not in seen:                           # the same launch recurs from run to run
                            seen.add(key)
                            check_launch(plan, env, which, l, says_ready)
                    if schedule == SCHEDULE_EDGE and plan.ghost > 0:   # interior + edge together: every tile exactly once
                        first = [l for i, _, l, _ in group if i == 0]
                        ntx = first[0].tiles_x
                        both = sorted(t for l in first for t in covered(l, ntx))
                        assert both == [(j, i) for j in range(first[0].ntiles_total // ntx) for i in range(ntx)], label
        for knob in env:
            no_knobs.delenv(knob)
    assert len(seen) > 300


def test_ready_is_said_by_the_last_launch_of_a_group_that_another_follows(lbm, launcher, no_knobs):
    plan = _plan(lbm, launcher, "ring", lbm.Params(1024, 64, 20, 10, 0.1, 0.005, 1.85), {}, no_knobs)
    assert (plan.multi_K, plan.ghost, plan.ghost_x) == (4, 8, 0)
    parts = [[l.part for _, _, l, _ in g] for g in run_groups(lbm, launcher, plan, 20, SERIAL)]
    assert parts == [[PART_GHOST, PART_READY], [PART_GHOST, PART_READY], [PART_PLAIN]]


def test_the_grid_is_padded_for_tile_ranks_with_both_knobs_only(lbm, launcher, no_knobs):
    p = lbm.Params(1024, 512, 20, 10, 0.1, 0.005, 1.85)
    for env in ({}, {"LBM_TUNE_TILE_PAD_GRID": "0"}, {"LBM_TUNE_MULTI_REMAP": "0"}):
        plan = _plan(lbm, launcher, "tile", p, env, no_knobs, px=2, py=2, rank=3)
        for knob, value in env.items():
            no_knobs.setenv(knob, value)
        groups = run_groups(lbm, launcher, plan, 20, SCHEDULE_EDGE)
        launches = [l for g in groups for _, _, l, _ in g]
        for _, which, l, says_ready in [t for g in groups for t in g]:
            check_launch(plan, env, which, l, says_ready)
        assert any(l.nblocks >= 64 and l.nblocks % 8 for l in launches)
        assert any(l.launched_blocks != l.nblocks for l in launches) == (env == {})
        for knob in env:
            no_knobs.delenv(knob)


def test_the_push_overtakes_the_interior_only_where_the_edge_rows_hold_its_rows(lbm, launcher, no_knobs):
    from mpilattice_boltzmann_amd import host
    yes = 0
    one = {"LBM_TUNE_MACRO_GROUP": "1"}                                # one launch per exchange: the groups whose push may overtake
    ring = ("1024 x 128 ring, one launch per exchange", _plan(lbm, launcher, "ring", lbm.Params(1024, 128, 20, 10, 0.1, 0.005, 1.85), one, no_knobs), one)
    for label, plan, env in contexts(lbm, launcher, no_knobs) + [ring]:
        if plan.ghost == 0:
            continue
        for knob, value in env.items():
            no_knobs.setenv(knob, value)
        for n_steps in RUNS:
            groups, left = host.plan_groups(plan.multi_K, plan.ghost, plan.group_max, n_steps), n_steps
            for g, steps in enumerate(groups):
                suffice = launcher.lbm_plan_edge_rows_suffice(C.byref(plan), left)
                left -= sum(steps)
                if not suffice:
                    continue
                yes += 1
                assert g + 1 < len(groups) and len(steps) == 1 and plan.ghost_x == 0, label
                rows, lo, hi = sum(groups[g + 1]), plan.ghost_rows, plan.ghost_rows + plan.nyl
                tiles, _, _ = tiles_of(plan, steps[0], 0)
                edge_rows = {r for _, _, rim, (r0, r1) in tiles if rim for r in range(r0, r1)}
                assert set(range(lo, lo + rows)) | set(range(hi - rows, hi)) <= edge_rows, label
        for knob in env:
            no_knobs.delenv(knob)
    assert yes > 0


def test_bad_arguments_are_refused(lbm, launcher, no_knobs):
    plan, l = _plan(lbm, launcher, "whole", lbm.Params(512, 512, 11, 10, 0.1, 0.005, 1.85), {}, no_knobs), CLaunch()
    for k, ext, which in ((0, 0, WHOLE), (5, 0, WHOLE), (4, -1, WHOLE), (4, 0, 3)):
        assert launcher.lbm_plan_launch(C.byref(plan), k, ext, which, 0, C.byref(l)) == 1
        assert launcher.lbm_last_error().decode() == "lbm_plan_launch: bad argument"
    assert launcher.lbm_plan_run_launches(C.byref(plan), -1, SERIAL, None, 0) == -1
    assert launcher.lbm_plan_run_launches(C.byref(plan), 11, 2, None, 0) == -1
    assert launcher.lbm_plan_run_launches(C.byref(plan), 11, SERIAL, None, 0) == 3           # the count alone
    step = _plan(lbm, launcher, "whole", lbm.Params(100, 100, 11, 10, 0.1, 0.005, 1.85), {}, no_knobs)
    assert launcher.lbm_plan_run_launches(C.byref(step), 11, SERIAL, None, 0) == 0           # the one-step kernels: not planned here


# ---- 2. the recording ----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


def test_the_recorded_table_is_the_recorder_s(golden):
    assert golden["steps"] == launch_cases.STEPS and len(golden["commit"]) >= 7
    assert [{k: r[k] for k in c} for r, c in zip(golden["rows"], launch_cases.cases())] == launch_cases.cases()
    assert len(golden["rows"]) == len(launch_cases.cases()) and sum(len(r["dispatches"]) for r in golden["rows"]) > 60


def test_launch_plans_reproduce_the_recorded_dispatches(lbm, launcher, golden, no_knobs):
    for row in golden["rows"]:
        what = json.dumps({k: v for k, v in row.items() if k != "dispatches"})
        p, env = launch_cases.params_of(lbm, row), {k: v for k, v in row["env"].items() if k.startswith("LBM_TUNE")}
        ranks = [dict(px=row["px"], py=row["py"], rank=r) for r in range(row["contexts"])] if row["kind"] == "tiles" else [{}]
        plans = [_plan(lbm, launcher, "tile" if row["kind"] == "tiles" else row["kind"], p, env, no_knobs, **kw) for kw in ranks]
        for knob, value in env.items():
            no_knobs.setenv(knob, value)
        recorded = [tuple(d) for d in row["dispatches"]]
        if not (plans[0].multi_K > 0 and (plans[0].self_periodic or plans[0].ghost > 0)) and not plans[0].tile_kernel:
            assert recorded == [], what                               # the one-step kernels
        elif row["kind"] == "whole":
            buf = (CLaunch * 64)()
            n = launcher.lbm_plan_run_launches(C.byref(plans[0]), launch_cases.STEPS, SERIAL, buf, 64)
            assert [kernel_of(plans[0], buf[i]) for i in range(n)] == recorded, what
        else:
            # rings: the peer-to-peer loop under its schedule; tile grids: every rank through interior + edge, then every rank's later launches
            schedule = SCHEDULE_EDGE if row["kind"] == "tiles" or row["schedule"] == "edge" else SERIAL
            per_rank = [run_groups(lbm, launcher, plan, launch_cases.STEPS, schedule) for plan in plans]
            pos = 0
            for g in range(len(per_rank[0])):
                first = [kernel_of(plan, l) for plan, groups in zip(plans, per_rank) for i, _, l, _ in groups[g] if i == 0]
                rest = [kernel_of(plan, l) for plan, groups in zip(plans, per_rank) for i, _, l, _ in groups[g] if i > 0]
                got = recorded[pos:pos + len(first) + len(rest)]
                pos += len(got)
                if row["kind"] == "ring" and schedule == SCHEDULE_EDGE:      # two streams: in order of their start, whichever came first
                    assert sorted(got) == sorted(first + rest), (what, g)
                else:
                    assert got == first + rest, (what, g)
            assert pos == len(recorded), what
        for knob in env:
            no_knobs.delenv(knob)
