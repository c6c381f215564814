"""The plan of a double-precision context (csrc/lbm_plan.cpp plan64_whole, Plan64 of lbm_internal.h) through the lbm_plan64_* entry
points: what lbm64_create decides, without a GPU.  Without LBM64_FLAG_TILE_STEPS every shape tests/test_f64.py runs plans as that file
asserts; with it, which grids lbm_tile_kernel_f64 takes, in which geometry, and how a run is cut into launches."""
import ctypes as C

import pytest

BLOCK = 256
FLAG_NT, FLAG_NO_NT, FLAG_TILE = 1, 2, 512
GEOMS = [(8, 4), (8, 8), (16, 4), (16, 8)]          # every geometry lbm_tile_kernel_f64 is built for
LDS_PER_WORKGROUP = 160 * 1024


class Plan64(C.Structure):
    """struct Plan64 (lbm_internal.h), field for field."""

    _fields_ = [("flags", C.c_uint), ("nt_stores", C.c_int), ("lane_cells", C.c_int), ("units", C.c_uint), ("iters", C.c_int), ("blocks", C.c_int),
                ("tile_kernel", C.c_int), ("tile_T", C.c_int), ("tile_H", C.c_int), ("n_tiles", C.c_int), ("tiles_x", C.c_int),
                ("tile_block", C.c_int), ("tile_lds_bytes", C.c_int), ("partials_cap", C.c_int),
                ("ps", C.c_longlong), ("grid_doubles", C.c_longlong)]


@pytest.fixture(scope="module")
def api(lbm):
    from mpilattice_boltzmann_amd import f64
    lib = lbm.load_library()
    lib.lbm_plan64_sizeof.restype, lib.lbm_plan64_sizeof.argtypes = C.c_int, []
    lib.lbm_plan64_whole.restype, lib.lbm_plan64_whole.argtypes = C.c_int, [C.POINTER(f64.CParams64), C.c_uint, C.POINTER(Plan64)]
    lib.lbm_plan64_kernel_name.restype, lib.lbm_plan64_kernel_name.argtypes = C.c_int, [C.POINTER(Plan64), C.c_char_p, C.c_size_t]
    lib.lbm_plan64_run_launches.restype = C.c_int
    lib.lbm_plan64_run_launches.argtypes = [C.POINTER(Plan64), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int]
    assert lib.lbm_plan64_sizeof() == C.sizeof(Plan64)
    return lib, f64


@pytest.fixture(autouse=True)
def _no_knobs(monkeypatch):
    for k in ("LBM_TUNE_TILE64_MAX", "LBM_TUNE_TILE64_GEOM", "LBM_TUNE_MAXBLOCKS", "LBM_TUNE_SKEW"):
        monkeypatch.delenv(k, raising=False)


def _plan(api, nx, ny, flags=0):
    lib, f64 = api
    cp = f64.CParams64(nx, ny, 10, 10, 0.1, 0.005, 1.85)
    plan = Plan64()
    assert lib.lbm_plan64_whole(C.byref(cp), flags, C.byref(plan)) == 0
    name = C.create_string_buffer(128)
    assert lib.lbm_plan64_kernel_name(C.byref(plan), name, 128) == 0
    return plan, name.value.decode()


def _launches(api, plan, n):
    lib, _ = api
    cap = n + 1
    steps, full = (C.c_int * cap)(), (C.c_int * cap)()
    count = lib.lbm_plan64_run_launches(C.byref(plan), n, steps, full, cap)
    assert 0 <= count <= cap
    return list(steps[:count]), list(full[:count])


PAIR = [(8, 3), (32, 16), (40, 24), (32, 32), (64, 48), (256, 8), (2, 3), (258, 33), (1024, 1024)]
SINGLE = [(1, 3), (7, 5), (257, 33)]


@pytest.mark.parametrize("nx,ny", PAIR + SINGLE)
def test_without_the_flag_the_one_step_plan_is_what_test_f64_asserts(api, nx, ny):
    plan, name = _plan(api, nx, ny)
    cells = 2 if nx % 2 == 0 else 1
    assert name == f"lbm_step_kernel_f64<{cells}>" and plan.tile_kernel == 0
    assert (plan.lane_cells, plan.nt_stores, plan.iters) == (cells, 0, 1)
    assert plan.units == nx * ny // cells and plan.blocks == -(-plan.units // BLOCK)
    assert plan.partials_cap == plan.blocks + 1
    assert plan.ps % 2 == 0 and plan.ps >= nx * ny + 64 and plan.grid_doubles == 9 * plan.ps + 128
    for flag, want in ((FLAG_NT, f"lbm_step_kernel_f64<{cells},nt>"), (FLAG_NO_NT, f"lbm_step_kernel_f64<{cells}>")):
        assert _plan(api, nx, ny, flag)[1] == want


def test_without_the_flag_large_grids(api):
    plan, name = _plan(api, 4096, 2050)
    assert name == "lbm_step_kernel_f64<2,nt>" and (plan.iters, plan.blocks, plan.units) == (2, 8200, 4096 * 2050 // 2)
    plan, name = _plan(api, 8192, 7296)
    assert name == "lbm_step_kernel_f64<2,nt>" and plan.tile_kernel == 0


@pytest.mark.parametrize("nx,ny,maxblocks", [(258, 33, 3), (257, 33, 5), (64, 48, 1)])
def test_without_the_flag_a_lowered_block_cap(api, monkeypatch, nx, ny, maxblocks):
    monkeypatch.setenv("LBM_TUNE_MAXBLOCKS", str(maxblocks))
    plan, _ = _plan(api, nx, ny)
    per_block = BLOCK * plan.iters * plan.lane_cells
    assert per_block > BLOCK * 2 and plan.blocks * per_block >= nx * ny and plan.blocks == -(-(nx * ny) // per_block)


def test_refusals(api):
    lib, f64 = api
    plan = Plan64()
    for nx, ny, flags in ((0, 4, 0), (8, 2, 0), (8, 8, 256), (8, 8, 4), (8, 8, FLAG_TILE | 64)):
        cp = f64.CParams64(nx, ny, 10, 10, 0.1, 0.005, 1.85)
        assert lib.lbm_plan64_whole(C.byref(cp), flags, C.byref(plan)) == 1
    assert lib.lbm_plan64_run_launches(C.byref(plan), -1, None, None, 0) == -1


def test_eligibility_with_the_flag(api, monkeypatch):
    monkeypatch.setenv("LBM_TUNE_TILE64_MAX", str(1 << 20))       # eligibility by shape, whatever cap the measurements set
    for nx, ny in ((128, 128), (128, 256), (256, 256)):
        plan, name = _plan(api, nx, ny, FLAG_TILE)
        assert plan.tile_kernel == 1 and name == f"lbm_tile_kernel_f64<{plan.tile_T}, {plan.tile_H}>", (nx, ny, name)
        assert plan.tiles_x == nx // plan.tile_T and plan.n_tiles == (nx // plan.tile_T) * (ny // plan.tile_T)
        assert plan.partials_cap == max(plan.blocks, plan.tile_H * plan.n_tiles) + 1
        # the one-step plan is still there, unchanged
        plain, _ = _plan(api, nx, ny)
        assert (plan.lane_cells, plan.nt_stores, plan.units, plan.iters, plan.blocks, plan.ps) == (plain.lane_cells, plain.nt_stores, plain.units, plain.iters, plain.blocks, plain.ps)
    for nx, ny in ((8, 3), (7, 5), (258, 33)):
        plan, name = _plan(api, nx, ny, FLAG_TILE)
        assert plan.tile_kernel == 0 and name == _plan(api, nx, ny)[1] and name.startswith("lbm_step_kernel_f64<")
        assert plan.partials_cap == plan.blocks + 1
    monkeypatch.setenv("LBM_TUNE_TILE64_GEOM", "88")
    plan, name = _plan(api, 40, 24, FLAG_TILE)
    assert plan.tile_kernel == 1 and name == "lbm_tile_kernel_f64<8, 8>" and (plan.tiles_x, plan.n_tiles) == (5, 15)
    monkeypatch.setenv("LBM_TUNE_TILE64_GEOM", "164")
    plan, name = _plan(api, 40, 24, FLAG_TILE)
    assert plan.tile_kernel == 0 and name == "lbm_step_kernel_f64<2>"


def test_the_size_cap(api, monkeypatch):
    monkeypatch.setenv("LBM_TUNE_TILE64_GEOM", "84")
    monkeypatch.setenv("LBM_TUNE_TILE64_MAX", str(64 * 64))
    assert _plan(api, 64, 64, FLAG_TILE)[0].tile_kernel == 1
    assert _plan(api, 64, 72, FLAG_TILE)[0].tile_kernel == 0         # one row of tiles above the cap
    monkeypatch.setenv("LBM_TUNE_TILE64_MAX", str(64 * 64 + 63))
    assert _plan(api, 64, 72, FLAG_TILE)[0].tile_kernel == 0
    monkeypatch.setenv("LBM_TUNE_TILE64_MAX", "0")
    plan, name = _plan(api, 64, 64, FLAG_TILE)
    assert plan.tile_kernel == 0 and name == "lbm_step_kernel_f64<2>"


def test_defaults_are_the_measured_ones(api):
    """No knob set (profiles/r08/f64_tile.txt): the flag takes every measured deck, in the geometry that was fastest on it, and nothing
    above the largest size measured."""
    fastest = {(128, 128): (8, 4), (128, 256): (16, 8), (256, 256): (16, 8), (512, 512): (8, 4), (1024, 1024): (8, 4)}
    for (nx, ny), geom in fastest.items():
        plan, name = _plan(api, nx, ny, FLAG_TILE)
        assert plan.tile_kernel == 1 and (plan.tile_T, plan.tile_H) == geom, (nx, ny, name)
    plan, name = _plan(api, 1024, 1024 + 16, FLAG_TILE)
    assert plan.tile_kernel == 0 and name == "lbm_step_kernel_f64<2>"
    assert _plan(api, 1024, 1024)[0].tile_kernel == 0                        # and nothing without the flag


@pytest.mark.parametrize("T,H", GEOMS)
def test_forced_geometries_and_their_blocks(api, monkeypatch, T, H):
    monkeypatch.setenv("LBM_TUNE_TILE64_MAX", str(1 << 20))
    monkeypatch.setenv("LBM_TUNE_TILE64_GEOM", str(T * 10 + H))
    plan, name = _plan(api, 128, 128, FLAG_TILE)
    assert (plan.tile_kernel, plan.tile_T, plan.tile_H) == (1, T, H) and name == f"lbm_tile_kernel_f64<{T}, {H}>"
    R = T + 2 * H
    assert 2 * 9 * R * R * 8 + R * R <= plan.tile_lds_bytes <= LDS_PER_WORKGROUP      # two buffers and the flag bytes at least
    assert plan.tile_block <= 1024 and plan.tile_block % 64 == 0 and plan.tile_block >= T * T
    assert plan.n_tiles == (128 // T) ** 2 and plan.partials_cap == H * plan.n_tiles + 1


@pytest.mark.parametrize("value", ["87", "0", "-1", "abc", "1680", "48", "168x"])
def test_malformed_geometry_gets_the_default(api, monkeypatch, value):
    monkeypatch.setenv("LBM_TUNE_TILE64_MAX", str(1 << 20))
    default, _ = _plan(api, 128, 128, FLAG_TILE)
    monkeypatch.setenv("LBM_TUNE_TILE64_GEOM", value)
    plan, _ = _plan(api, 128, 128, FLAG_TILE)
    if value == "168x":                              # atoi reads the leading number
        assert (plan.tile_T, plan.tile_H) == (16, 8)
    else:
        assert (plan.tile_T, plan.tile_H) == (default.tile_T, default.tile_H)
    assert (default.tile_T, default.tile_H) in GEOMS


@pytest.mark.parametrize("T,H", GEOMS)
def test_run_launches(api, monkeypatch, T, H):
    monkeypatch.setenv("LBM_TUNE_TILE64_MAX", str(1 << 20))
    monkeypatch.setenv("LBM_TUNE_TILE64_GEOM", str(T * 10 + H))
    plan, _ = _plan(api, 64, 64, FLAG_TILE)
    assert plan.tile_kernel == 1
    assert _launches(api, plan, 0) == ([], [])
    for n in range(1, 3 * H + 2):
        steps, full = _launches(api, plan, n)
        assert sum(steps) == n and all(1 <= k <= H for k in steps)
        assert full == [int(k == H) for k in steps]
        assert sum(1 for f in full if not f) <= 1 and len(steps) == -(-n // H)
        assert all(f for f in full[:-1])                                 # the short launch, if any, is the tail
    # a context of the one-step kernel: n launches of one step
    plain, _ = _plan(api, 64, 64)
    assert _launches(api, plain, 5) == ([1] * 5, [0] * 5)


def test_code_object_holds_both_kernels(lbm):
    blob = open(lbm.LIB_PATH, "rb").read()
    assert b"lbm_tile_kernel_f64" in blob and b"lbm_step_kernel_f64" in blob
