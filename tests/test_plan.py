"""Which kernel, geometry and sizes a context gets — checked on a CPU through the library's planning entry points (csrc/lbm_plan.cpp,
declared in csrc/lbm_internal.h) against tests/golden/plans_parent.json, which tests/plan_cases.py recorded from live contexts on an
MI355X at the commit named inside the file.  The one GPU test records again and compares row for row."""
import ctypes as C
import json
import os

import pytest

import plan_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "plans_parent.json")
KNOB_NAMES = [knob for knob, _, _ in plan_cases.KNOBS]
GEOM_STD, GEOM_NARROW, GEOM_TALL = 0, 1, 2


class CPlan(C.Structure):
    """struct ContextPlan (csrc/lbm_internal.h), field for field."""

    _fields_ = ([(n, C.c_int) for n in ("nx", "y0", "nyl")] + [("flags", C.c_uint)] +
                [(n, C.c_int) for n in ("self_periodic", "accel_row", "use_graph")] +
                [(n, C.c_float) for n in ("accel_w1", "accel_w2", "free_cells_inv")] +
                [(n, C.c_int) for n in ("multi_K", "ghost", "ghost_rows", "group_max",
                                        "ghost_x", "x0", "nxl", "nx_global", "tiles_px", "tiles_py", "tile_rx", "tile_ry")] +
                [(n, C.c_longlong) for n in ("ncells", "ncells_storage", "ps", "grid_floats")] +
                [(n, C.c_int) for n in ("mask_words", "nxp", "nt_stores", "lane_cells", "fast_avvels", "fused", "multi_terms", "multi_tail4",
                                        "tile_T", "tile_H", "tile_single_max", "n_tiles", "tile_kernel",
                                        "multi_geom", "multi_tx", "multi_tiles_x",
                                        "iters_full", "iters_interior", "n_part_full", "n_part_interior", "n_part_boundary", "partials_cap")] +
                [(n, C.c_longlong) for n in ("pack_floats", "pack_floats_x", "pack_alloc_floats")])


@pytest.fixture(scope="module")
def planner(lbm):
    lib = lbm.load_library()
    P, CP = C.POINTER, lbm._capi.CParams
    lib.lbm_plan_sizeof.restype, lib.lbm_plan_sizeof.argtypes = C.c_int, []
    lib.lbm_plan_whole.restype, lib.lbm_plan_whole.argtypes = C.c_int, [P(CP), C.c_int, C.c_int, C.c_int, C.c_uint, C.c_int, P(CPlan)]
    lib.lbm_plan_rank.restype, lib.lbm_plan_rank.argtypes = C.c_int, [P(CP), C.c_int, C.c_int, C.c_int, C.c_uint, P(CPlan)]
    lib.lbm_plan_tile.restype, lib.lbm_plan_tile.argtypes = C.c_int, [P(CP), C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint, P(CPlan)]
    lib.lbm_plan_kernel_name.restype, lib.lbm_plan_kernel_name.argtypes = C.c_int, [P(CPlan), C.c_char_p, C.c_size_t]
    assert lib.lbm_plan_sizeof() == C.sizeof(CPlan), "CPlan above is not the library's ContextPlan"
    return lib


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


@pytest.fixture
def no_knobs(monkeypatch):
    for knob in KNOB_NAMES:
        monkeypatch.delenv(knob, raising=False)
    return monkeypatch


def plan_of(lbm, lib, case, status=0):
    """The plan of a case of plan_cases.cases() (its knobs must already be in the environment) and the kernel name it spells."""
    from mpilattice_boltzmann_amd import host
    p = plan_cases.params_of(lbm, case)
    cp, flags, free, plan = host._cparams(p), plan_cases.flags_of(lbm, case), p.nx * p.ny, CPlan()
    if case["kind"] == "whole":
        rc = lib.lbm_plan_whole(C.byref(cp), free, 0, p.ny, flags, 0, C.byref(plan))
    elif case["kind"] == "ring":
        rc = lib.lbm_plan_rank(C.byref(cp), free, 1, 0, flags, C.byref(plan))
    else:
        rc = lib.lbm_plan_tile(C.byref(cp), free, case["px"], case["py"], case["rank"], flags, C.byref(plan))
    assert rc == status, lib.lbm_last_error().decode()
    name = C.create_string_buffer(256)
    if rc == 0:
        assert lib.lbm_plan_kernel_name(C.byref(plan), name, 256) == 0
    return plan, name.value.decode()


def whole(nx, ny, *flags):
    return {"kind": "whole", "nx": nx, "ny": ny, "flags": list(flags), "env": {}}


def launches_of(lbm, plan, name):
    """The steps per launch of an lbm_run of plan_cases.STEPS steps."""
    from mpilattice_boltzmann_amd import host
    n = plan_cases.STEPS
    if name.startswith("lbm_multi_kernel"):
        return host.plan_steps(plan.multi_K, n)
    if name.startswith("lbm_tile_kernel"):
        return [min(plan.tile_H, n - t) for t in range(0, n, plan.tile_H)]
    return [1] * n


def test_the_table_is_the_recorded_one(golden):
    rows = golden["rows"]
    assert golden["steps"] == plan_cases.STEPS and len(golden["commit"]) >= 7
    assert [{k: r[k] for k in c} for r, c in zip(rows, plan_cases.cases())] == plan_cases.cases() and len(rows) == len(plan_cases.cases())


def test_plans_reproduce_the_recorded_contexts(lbm, planner, golden, no_knobs):
    for row in golden["rows"]:
        for knob, value in row["env"].items():
            no_knobs.setenv(knob, value)
        plan, name = plan_of(lbm, planner, row)
        for knob in row["env"]:
            no_knobs.delenv(knob)
        what = json.dumps({k: row[k] for k in ("kind", "nx", "ny", "flags", "env")})
        assert name == row["kernel"], what
        assert plan.ncells == row["cells_per_launch"], what
        assert 2 * 9 * plan.ncells * 4 + plan.ncells // 8 == row["state_bytes"], what
        assert 3 * plan.nxp == row["halo_floats"], what
        assert plan.pack_floats == row["macro_pack_floats"] and plan.pack_floats_x == row["macro_pack_floats_x"], what
        if row["kind"] == "tile":
            assert {"px": plan.tiles_px, "py": plan.tiles_py, "rx": plan.tile_rx, "ry": plan.tile_ry, "x0": plan.x0, "nx_local": plan.nxl,
                    "y0": plan.y0, "ny_local": plan.nyl, "macro_k": plan.multi_K if plan.ghost > 0 else 0, "ghost": plan.ghost,
                    "group": plan.group_max, "ghost_x": plan.ghost_x, "ghost_y": plan.ghost_rows} == row["tile_info"], what
            assert plan.nx == plan.nxl + 2 * plan.ghost_x, what
        if row["kind"] == "whole":
            assert launches_of(lbm, plan, name) == row["launch_steps"], what


@pytest.mark.parametrize("nx, ny, kernel, details", [
    (128, 128, "lbm_tile_kernel<8, 8>", {}),
    (256, 256, "lbm_tile_kernel<16, 8>", {}),
    (512, 256, "lbm_tile_kernel<16, 8>", {}),
    (512, 512, "lbm_multi_kernel<3>", {"multi_geom": GEOM_STD}),
    (768, 768, "lbm_multi_kernel<4>", {"multi_geom": GEOM_STD}),
    (1024, 1024, "lbm_multi_kernel<4>", {"multi_geom": GEOM_TALL}),
    (130, 100, "lbm_multi_kernel<3>", {"multi_geom": GEOM_NARROW, "multi_tx": 32, "lane_cells": 1}),
    (100, 100, "lbm_step_kernel_narrow<false>", {}),
    (127, 64, "lbm_step_kernel_narrow<false>", {}),
    (96, 2048, "lbm_step_kernel<false>", {}),
    (100, 40000, "lbm_step_kernel<true>", {}),
])
def test_which_kernel_a_whole_grid_gets(lbm, planner, no_knobs, nx, ny, kernel, details):
    plan, name = plan_of(lbm, planner, whole(nx, ny))
    assert name == kernel
    assert {k: getattr(plan, k) for k in details} == details


def test_each_knob_moves_the_plan(lbm, planner, no_knobs):
    def with_knob(knob, value, nx, ny):
        no_knobs.setenv(knob, value)
        out = plan_of(lbm, planner, whole(nx, ny))
        no_knobs.delenv(knob)
        return out
    plan, name = with_knob("LBM_TUNE_MULTI_K", "3", 1024, 1024)          # K by knob; the geometry is still chosen by size
    assert (name, plan.multi_K, plan.multi_geom) == ("lbm_multi_kernel<3>", 3, GEOM_TALL)
    assert with_knob("LBM_TUNE_MULTI_K", "3", 256, 256)[1] == "lbm_tile_kernel<16, 8>"       # not a multi-kernel grid: untouched
    plan, name = with_knob("LBM_TUNE_TILE_GEOM", "164", 256, 256)        # T * 10 + H
    assert (name, plan.tile_T, plan.tile_H, plan.n_tiles) == ("lbm_tile_kernel<16, 4>", 16, 4, 256)
    assert with_knob("LBM_TUNE_TILE_GEOM", "164", 128, 128)[1] == "lbm_tile_kernel<16, 4>"
    assert with_knob("LBM_TUNE_TILE_GEOM", "164", 512, 512)[1] == "lbm_multi_kernel<3>"
    plan, name = with_knob("LBM_TUNE_MULTI_GEOM", "0", 1024, 1024)       # the whole choice of geometry
    assert (name, plan.multi_geom, plan.multi_tx) == ("lbm_multi_kernel<4>", GEOM_STD, 64)
    plan, name = with_knob("LBM_TUNE_MULTI_GEOM", "0", 130, 100)
    assert (plan.multi_geom, plan.multi_tx, plan.multi_tiles_x) == (GEOM_STD, 64, 3)
    plan, name = with_knob("LBM_TUNE_NARROW_MAX", "0", 100, 100)         # no grid is "small" for the one-step kernel: four cells per lane
    assert (name, plan.lane_cells) == ("lbm_step_kernel<false>", 4)
    assert with_knob("LBM_TUNE_NARROW_MAX", "0", 127, 64)[1] == "lbm_step_kernel_narrow<false>"      # nx % 4 != 0 stays narrow
    for nx, ny in ((256, 256), (128, 128), (64, 16)):                   # no grid is small enough for lbm_tile_kernel: 64 x 16 tiles take them
        plan, name = with_knob("LBM_TUNE_TILE_MAX", "0", nx, ny)
        assert (name, plan.tile_kernel, plan.multi_K) == ("lbm_multi_kernel<3>", 0, 3)
    plan, name = plan_of(lbm, planner, whole(64, 16))                   # (without the knob: a tile-kernel grid)
    assert name == "lbm_tile_kernel<8, 8>"


def test_refusals_keep_their_words(lbm, planner, no_knobs):
    from mpilattice_boltzmann_amd import host
    lib, K = planner, lbm._capi

    def refused(call):
        assert call() == 1
        return lib.lbm_last_error().decode()
    plan = CPlan()
    cp = host._cparams(plan_cases.params_of(lbm, whole(512, 512)))
    for other in (K.FLAG_FAST_AVVELS, K.FLAG_EXACT_AVVELS):
        assert refused(lambda: lib.lbm_plan_whole(C.byref(cp), 512 * 512, 0, 512, K.FLAG_FUSED_ARITH | other, 0, C.byref(plan))) == \
            "lbm_create: LBM_FLAG_FUSED_ARITH cannot be combined with LBM_FLAG_FAST_AVVELS or LBM_FLAG_EXACT_AVVELS (the fused kernels carry each family's default sum|u| terms only)"
    assert refused(lambda: lib.lbm_plan_whole(C.byref(cp), 512 * 512, 0, 512, K.FLAG_KERNEL_LDS, 0, C.byref(plan))) == \
        "lbm_create: LBM_FLAG_KERNEL_LDS is retired (the LDS-staged one-step kernel was never faster and is no longer built)"
    # row ny-2 as the first or the last row of a partition
    for y0, rows in ((0, 511), (510, 2)):
        assert refused(lambda: lib.lbm_plan_whole(C.byref(cp), 512 * 512, y0, rows, 0, 0, C.byref(plan))) == \
            "lbm_create: the partition holding row ny-2 needs >= 3 rows (d2q9-bgk.c:848-849)"
    big = host._cparams(plan_cases.params_of(lbm, whole(65536, 40000)))
    assert refused(lambda: lib.lbm_plan_whole(C.byref(big), 1, 0, 40000, 0, 0, C.byref(plan))) == \
        "lbm_create: partition too large for 32-bit cell indices"
    # the layouts' refusals come first, in their own words
    small = host._cparams(plan_cases.params_of(lbm, whole(64, 2)))
    assert refused(lambda: lib.lbm_plan_rank(C.byref(small), 128, 1, 0, K.FLAG_FORCE_HALO, C.byref(plan))) == "lbm_rank_layout: grid too small for this many ranks"
    assert refused(lambda: lib.lbm_plan_tile(C.byref(cp), 512 * 512, 2, 1, 0, K.FLAG_ONE_STEP, C.byref(plan))).startswith(
        "lbm_tile_layout_of: the tile decomposition runs in K-step mode only:")
    assert refused(lambda: lib.lbm_plan_whole(C.byref(cp), 0, 0, 512, 0, 0, C.byref(plan))) == "lbm_create: free_cells must be positive"


def test_a_one_step_ring_plans_no_ghost_rows(lbm, planner, no_knobs):
    """A one-rank ring of 31 rows is below K-step mode's 32: the plan keeps no ghost rows and names the one-step kernel."""
    plan, name = plan_of(lbm, planner, {"kind": "ring", "nx": 1024, "ny": 31, "flags": ["FLAG_FORCE_HALO"], "env": {}})
    assert (plan.multi_K, plan.ghost, plan.ghost_rows, plan.self_periodic, plan.pack_floats) == (0, 0, 0, 0, 0)
    assert name.startswith("lbm_step_kernel")
    plan, name = plan_of(lbm, planner, {"kind": "ring", "nx": 1024, "ny": 128, "flags": ["FLAG_FORCE_HALO"], "env": {}})
    assert plan.multi_K == 4 and plan.ghost == plan.ghost_rows and plan.ghost % 4 == 0 and plan.pack_floats == 9 * plan.ghost * 1024
    assert plan.ncells_storage == 1024 * (128 + 2 * plan.ghost_rows) and plan.mask_words == (plan.ncells_storage + 31) // 32 + 4


@pytest.mark.gpu
def test_live_contexts_agree_with_the_recorded_plans(lbm, golden):
    """The recorder again, on this build, row for row against the recording."""
    for case, row in zip(plan_cases.cases(), golden["rows"]):
        assert plan_cases.record_case(lbm, case) == row
