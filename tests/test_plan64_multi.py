"""The plan of a double-precision context under LBM64_FLAG_MULTI_STEPS (csrc/lbm_plan.cpp plan64_multi, PlanMulti64 of lbm_internal.h)
through the lbm_plan64_multi* entry points, without a GPU: which grids lbm_multi_kernel_f64 takes, after which other kernel, with how
many steps per launch, and how a run is cut into launches; and that Plan64 and everything without the flag stay what they were."""
import ctypes as C

import pytest

from test_plan64 import FLAG_NO_NT, FLAG_NT, FLAG_TILE, LDS_PER_WORKGROUP, Plan64

FLAG_MULTI = 1024
TX, TY = 32, 16                 # the tile (lbm_geometry.h kMulti64TX, kMulti64TY)
BUILT_K = (2, 3, 4)             # every K lbm_multi_kernel_f64 is built for
DEFAULT_K, DEFAULT_MIN = 4, 1 << 20      # set by the measurement: test_defaults_are_the_measured_ones


class PlanMulti64(C.Structure):
    """struct PlanMulti64 (lbm_internal.h), field for field."""

    _fields_ = [("multi_kernel", C.c_int), ("K", C.c_int), ("TX", C.c_int), ("TY", C.c_int), ("tiles_x", C.c_int), ("n_tiles", C.c_int),
                ("block", C.c_int), ("lds_bytes", C.c_int), ("nt_stores", C.c_int), ("partials_cap", C.c_int)]


def frame_cells(K):
    return (TX + 4 * (K // 2)) * (TY + 2 * (K - 1))      # multi_ex(K - 1) = 2 ceil((K - 1) / 2) = 2 (K // 2) columns a side, K - 1 rows


@pytest.fixture(scope="module")
def api(lbm):
    from mpilattice_boltzmann_amd import f64
    lib = lbm.load_library()
    lib.lbm_plan64_sizeof.restype, lib.lbm_plan64_sizeof.argtypes = C.c_int, []
    lib.lbm_plan64_whole.restype, lib.lbm_plan64_whole.argtypes = C.c_int, [C.POINTER(f64.CParams64), C.c_uint, C.POINTER(Plan64)]
    lib.lbm_plan64_kernel_name.restype, lib.lbm_plan64_kernel_name.argtypes = C.c_int, [C.POINTER(Plan64), C.c_char_p, C.c_size_t]
    lib.lbm_plan64_multi_sizeof.restype, lib.lbm_plan64_multi_sizeof.argtypes = C.c_int, []
    lib.lbm_plan64_multi.restype, lib.lbm_plan64_multi.argtypes = C.c_int, [C.POINTER(f64.CParams64), C.c_uint, C.POINTER(PlanMulti64)]
    lib.lbm_plan64_multi_kernel_name.restype, lib.lbm_plan64_multi_kernel_name.argtypes = C.c_int, [C.POINTER(PlanMulti64), C.c_char_p, C.c_size_t]
    lib.lbm_plan64_multi_run_launches.restype = C.c_int
    lib.lbm_plan64_multi_run_launches.argtypes = [C.POINTER(PlanMulti64), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int]
    return lib, f64


@pytest.fixture(autouse=True)
def _no_knobs(monkeypatch):
    for k in ("LBM_TUNE_TILE64_MAX", "LBM_TUNE_TILE64_GEOM", "LBM_TUNE_MAXBLOCKS", "LBM_TUNE_SKEW", "LBM_TUNE_MULTI64_K", "LBM_TUNE_MULTI64_MIN"):
        monkeypatch.delenv(k, raising=False)


def _whole(api, nx, ny, flags):
    lib, f64 = api
    cp = f64.CParams64(nx, ny, 10, 10, 0.1, 0.005, 1.85)
    plan = Plan64()
    assert lib.lbm_plan64_whole(C.byref(cp), flags, C.byref(plan)) == 0
    name = C.create_string_buffer(128)
    assert lib.lbm_plan64_kernel_name(C.byref(plan), name, 128) == 0
    return plan, name.value.decode()


def _multi(api, nx, ny, flags=FLAG_MULTI):
    lib, f64 = api
    cp = f64.CParams64(nx, ny, 10, 10, 0.1, 0.005, 1.85)
    plan = PlanMulti64()
    assert lib.lbm_plan64_multi(C.byref(cp), flags, C.byref(plan)) == 0
    name = C.create_string_buffer(128)
    assert lib.lbm_plan64_multi_kernel_name(C.byref(plan), name, 128) == 0
    return plan, name.value.decode()


def _launches(api, plan, n):
    lib, _ = api
    cap = n + 1
    steps, full = (C.c_int * cap)(), (C.c_int * cap)()
    count = lib.lbm_plan64_multi_run_launches(C.byref(plan), n, steps, full, cap)
    assert 0 <= count <= cap
    return list(steps[:count]), list(full[:count])


def test_the_mirror_has_the_struct_s_size(api):
    assert api[0].lbm_plan64_multi_sizeof() == C.sizeof(PlanMulti64)
    assert api[0].lbm_plan64_sizeof() == C.sizeof(Plan64)                    # and Plan64 is what tests/test_plan64.py mirrors


def test_eligibility_by_shape(api, monkeypatch):
    monkeypatch.setenv("LBM_TUNE_MULTI64_MIN", "0")
    for nx, ny in ((TX, TY), (2 * TX, TY), (96, 48)):
        plan, name = _multi(api, nx, ny)
        assert plan.multi_kernel == 1 and name == f"lbm_multi_kernel_f64<{plan.K}>", (nx, ny, name)
        assert (plan.TX, plan.TY, plan.tiles_x, plan.n_tiles) == (TX, TY, nx // TX, (nx // TX) * (ny // TY))
        assert _multi(api, nx, ny, FLAG_MULTI | FLAG_NT)[1] == f"lbm_multi_kernel_f64<{plan.K},nt>"
        assert _multi(api, nx, ny, FLAG_MULTI | FLAG_NO_NT)[1] == f"lbm_multi_kernel_f64<{plan.K}>"
        for flags in (0, FLAG_NT, FLAG_TILE):                             # nothing without the flag
            plan, name = _multi(api, nx, ny, flags)
            assert plan.multi_kernel == 0 and name == ""
    for nx, ny in ((40, 24), (258, 33), (7, 5)):
        plan, name = _multi(api, nx, ny)
        assert plan.multi_kernel == 0 and name == "" and plan.n_tiles == 0, (nx, ny)


def test_non_temporal_stores_follow_the_one_step_rule(api, monkeypatch):
    monkeypatch.setenv("LBM_TUNE_MULTI64_MIN", "0")
    for nx, ny in ((1024, 1024), (4096, 2048), (8192, 7296)):
        whole, _ = _whole(api, nx, ny, 0)
        plan, name = _multi(api, nx, ny)
        assert plan.nt_stores == whole.nt_stores and name.endswith(",nt>") == bool(whole.nt_stores)
    assert _multi(api, 8192, 7296)[0].nt_stores == 1 and _multi(api, 1024, 1024)[0].nt_stores == 0


def test_the_tiled_kernel_comes_first(api, monkeypatch):
    monkeypatch.setenv("LBM_TUNE_MULTI64_MIN", "0")
    whole, name = _whole(api, 128, 128, FLAG_TILE | FLAG_MULTI)
    assert whole.tile_kernel == 1 and name.startswith("lbm_tile_kernel_f64<")
    assert _multi(api, 128, 128, FLAG_TILE | FLAG_MULTI)[0].multi_kernel == 0
    assert _multi(api, 128, 128, FLAG_MULTI)[0].multi_kernel == 1
    # an eligible grid above LBM_TUNE_TILE64_MAX (1024 x 1024 by default): the one-step kernel with 512 alone, the new one with both
    whole, name = _whole(api, 1024, 1040, FLAG_TILE | FLAG_MULTI)
    assert whole.tile_kernel == 0 and name == "lbm_step_kernel_f64<2>"
    plan, name = _multi(api, 1024, 1040, FLAG_TILE | FLAG_MULTI)
    assert plan.multi_kernel == 1 and name == f"lbm_multi_kernel_f64<{plan.K}>"
    assert _multi(api, 1024, 1040, FLAG_TILE)[0].multi_kernel == 0


def test_the_minimum_size(api, monkeypatch):
    monkeypatch.setenv("LBM_TUNE_MULTI64_MIN", str(64 * 64))
    assert _multi(api, 64, 64 - TY)[0].multi_kernel == 0                    # one tile row below
    assert _multi(api, 64, 64)[0].multi_kernel == 1
    monkeypatch.setenv("LBM_TUNE_MULTI64_MIN", str(64 * 64 + 1))
    assert _multi(api, 64, 64)[0].multi_kernel == 0
    monkeypatch.setenv("LBM_TUNE_MULTI64_MIN", "0")
    assert _multi(api, TX, TY)[0].multi_kernel == 1


@pytest.mark.parametrize("value", ["0", "1", "5", "-3", "abc", "33", "3x"])
def test_malformed_steps_per_launch_get_the_default(api, monkeypatch, value):
    monkeypatch.setenv("LBM_TUNE_MULTI64_MIN", "0")
    default, _ = _multi(api, 96, 48)
    assert default.K == DEFAULT_K and default.K in BUILT_K
    monkeypatch.setenv("LBM_TUNE_MULTI64_K", value)
    plan, name = _multi(api, 96, 48)
    assert plan.K == (3 if value == "3x" else default.K)                   # atoi reads the leading number
    assert plan.multi_kernel == 1 and name == f"lbm_multi_kernel_f64<{plan.K}>"


@pytest.mark.parametrize("K", BUILT_K)
def test_every_built_k_and_its_block(api, monkeypatch, K):
    monkeypatch.setenv("LBM_TUNE_MULTI64_MIN", "0")
    monkeypatch.setenv("LBM_TUNE_MULTI64_K", str(K))
    plan, name = _multi(api, 96, 48)
    assert (plan.multi_kernel, plan.K) == (1, K) and name == f"lbm_multi_kernel_f64<{K}>"
    assert plan.block % 64 == 0 and plan.block <= 1024 and plan.block >= TX * TY
    assert 9 * 8 * frame_cells(K) <= plan.lds_bytes <= LDS_PER_WORKGROUP
    assert plan.n_tiles == 9 and plan.partials_cap == K * plan.n_tiles + 1


@pytest.mark.parametrize("K", BUILT_K)
def test_run_launches(api, monkeypatch, K):
    monkeypatch.setenv("LBM_TUNE_MULTI64_MIN", "0")
    monkeypatch.setenv("LBM_TUNE_MULTI64_K", str(K))
    plan, _ = _multi(api, 64, 48)
    assert plan.multi_kernel == 1
    assert _launches(api, plan, 0) == ([], [])
    for n in range(1, 3 * K + 2):
        steps, full = _launches(api, plan, n)
        assert sum(steps) == n and all(1 <= k <= K for k in steps)
        assert full == [int(k == K) for k in steps]
        assert all(f for f in full[:-1])                                  # the short launch, if any, is the tail
        assert sum(1 for f in full if not f) <= 1 and len(steps) == -(-n // K)
    assert api[0].lbm_plan64_multi_run_launches(C.byref(plan), -1, None, None, 0) == -1


@pytest.mark.parametrize("nx,ny", [(8, 3), (7, 5), (32, 16), (40, 24), (64, 48), (258, 33), (1024, 1024), (1024, 1040), (8192, 7296)])
def test_plan64_does_not_change_with_the_flag(api, monkeypatch, nx, ny):
    fields = [f for f, _ in Plan64._fields_ if f != "flags"]
    for base in (0, FLAG_NT, FLAG_NO_NT, FLAG_TILE, FLAG_TILE | FLAG_NT):
        for minimum in (None, "0"):
            if minimum is None:
                monkeypatch.delenv("LBM_TUNE_MULTI64_MIN", raising=False)
            else:
                monkeypatch.setenv("LBM_TUNE_MULTI64_MIN", minimum)
            off, name_off = _whole(api, nx, ny, base)
            on, name_on = _whole(api, nx, ny, base | FLAG_MULTI)
            assert on.flags == base | FLAG_MULTI and name_on == name_off
            assert [getattr(on, f) for f in fields] == [getattr(off, f) for f in fields]


def test_refusals(api):
    """tests/test_plan64.py's refused arguments, with and without the new bit, at both entry points."""
    lib, f64 = api
    plan, multi = Plan64(), PlanMulti64()
    for nx, ny, flags in ((0, 4, 0), (8, 2, 0), (8, 8, 256), (8, 8, 4), (8, 8, FLAG_TILE | 64)):
        for extra in (0, FLAG_MULTI):
            cp = f64.CParams64(nx, ny, 10, 10, 0.1, 0.005, 1.85)
            assert lib.lbm_plan64_whole(C.byref(cp), flags | extra, C.byref(plan)) == 1
            assert lib.lbm_plan64_multi(C.byref(cp), flags | extra, C.byref(multi)) == 1
    cp = f64.CParams64(64, 64, 10, 10, 0.1, 0.005, 1.85)
    assert lib.lbm_plan64_multi(C.byref(cp), FLAG_MULTI | 2048, C.byref(multi)) == 1
    assert lib.lbm_plan64_multi(C.byref(cp), FLAG_MULTI, None) == 1


def test_defaults_are_the_measured_ones(api):
    """No knob set (profiles/r11/f64_multi.txt): K = 4 is the fastest at 8192 x 8192 (624.3 us per step against 706.3 at K = 3 and 1039.8
    at K = 2); the flag takes the smallest measured size that beats the one-step kernel by more than the two max - min spreads
    together, 1024 x 1024 (11.99 against 23.46 us per step, spreads 0.05 us; the tiled kernel there: 20.67), and nothing smaller."""
    plan, name = _multi(api, 8192, 8192)
    assert plan.multi_kernel == 1 and plan.K == DEFAULT_K and name == f"lbm_multi_kernel_f64<{DEFAULT_K},nt>"
    side = int(DEFAULT_MIN ** 0.5)
    assert side * side == DEFAULT_MIN and side % TX == 0
    assert _multi(api, side, side)[0].multi_kernel == 1
    assert _multi(api, side, side - TY)[0].multi_kernel == 0
    assert _multi(api, 128, 128)[0].multi_kernel == 0


def test_code_object_holds_the_kernel(lbm):
    blob = open(lbm.LIB_PATH, "rb").read()
    assert b"lbm_multi_kernel_f64" in blob and b"lbm_tile_kernel_f64" in blob and b"lbm_step_kernel_f64" in blob
