"""The plan of a double-precision context under LBM64_FLAG_MULTI_ANY_SIZE (csrc/lbm_plan.cpp plan64_multi_any, PlanMultiAny64 of
lbm_internal.h) through the lbm_plan64_multi_any* entry points, without a GPU: which grids the edge-tile form of lbm_multi_kernel_f64
takes, which keep the existing form and which the one-step kernel; the tiles, where the last ones start and which cells each owns;
how a run is cut into launches; and that Plan64, PlanMulti64 and the row partitions stay what they were."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_plan64 import FLAG_NO_NT, FLAG_NT, FLAG_TILE, LDS_PER_WORKGROUP, Plan64
from test_plan64_multi import BUILT_K, DEFAULT_K, DEFAULT_MIN, FLAG_MULTI, TX, TY, PlanMulti64, frame_cells

FLAG_ANY = 4096
EDGE_SHAPES = [(34, 16), (32, 17), (40, 24), (62, 31), (258, 34)]          # tiles do not cover them; nx even and >= 32, ny >= 16
EXACT_SHAPES = [(32, 16), (96, 48)]
ONE_STEP_SHAPES = [(33, 16), (30, 16), (32, 15), (7, 5)]                   # odd nx, nx < 32, ny < 16
# 258 x 33, which LBM64_FLAG_MULTI_STEPS leaves to the one-step kernel (tests/test_plan64_multi.py), meets every condition of the edge
# form (nx even and >= 32, ny >= 16, not covered): it is an edge shape, with an odd ny and a last tile row that owns one row.
EDGE_SHAPES_ODD_NY = [(258, 33)]


class PlanMultiAny64(C.Structure):
    """struct PlanMultiAny64 (lbm_internal.h), field for field."""

    _fields_ = [("multi_kernel", C.c_int), ("edge", C.c_int), ("K", C.c_int), ("TX", C.c_int), ("TY", C.c_int),
                ("tiles_x", C.c_int), ("tiles_y", C.c_int), ("n_tiles", C.c_int), ("last_x0", C.c_int), ("last_y0", C.c_int),
                ("block", C.c_int), ("lds_bytes", C.c_int), ("nt_stores", C.c_int), ("partials_cap", C.c_int)]


@pytest.fixture(scope="module")
def api(lbm):
    from mpilattice_boltzmann_amd import f64
    lib = lbm.load_library()
    cp = C.POINTER(f64.CParams64)
    lib.lbm_plan64_sizeof.restype, lib.lbm_plan64_sizeof.argtypes = C.c_int, []
    lib.lbm_plan64_whole.restype, lib.lbm_plan64_whole.argtypes = C.c_int, [cp, C.c_uint, C.POINTER(Plan64)]
    lib.lbm_plan64_kernel_name.restype, lib.lbm_plan64_kernel_name.argtypes = C.c_int, [C.POINTER(Plan64), C.c_char_p, C.c_size_t]
    lib.lbm_plan64_multi_sizeof.restype, lib.lbm_plan64_multi_sizeof.argtypes = C.c_int, []
    lib.lbm_plan64_multi.restype, lib.lbm_plan64_multi.argtypes = C.c_int, [cp, C.c_uint, C.POINTER(PlanMulti64)]
    lib.lbm_plan64_multi_kernel_name.restype, lib.lbm_plan64_multi_kernel_name.argtypes = C.c_int, [C.POINTER(PlanMulti64), C.c_char_p, C.c_size_t]
    lib.lbm_plan64_multi_any_sizeof.restype, lib.lbm_plan64_multi_any_sizeof.argtypes = C.c_int, []
    lib.lbm_plan64_multi_any.restype, lib.lbm_plan64_multi_any.argtypes = C.c_int, [cp, C.c_uint, C.POINTER(PlanMultiAny64)]
    lib.lbm_plan64_multi_any_kernel_name.restype = C.c_int
    lib.lbm_plan64_multi_any_kernel_name.argtypes = [C.POINTER(PlanMultiAny64), C.c_char_p, C.c_size_t]
    lib.lbm_plan64_multi_any_run_launches.restype = C.c_int
    lib.lbm_plan64_multi_any_run_launches.argtypes = [C.POINTER(PlanMultiAny64), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int]
    lib.lbm_plan64_rows.restype, lib.lbm_plan64_rows.argtypes = C.c_int, [cp, C.c_int, C.c_int, C.c_uint, C.c_void_p]
    lib.lbm_plan64_rows_multi.restype, lib.lbm_plan64_rows_multi.argtypes = C.c_int, [cp, C.c_int, C.c_int, C.c_uint, C.c_void_p]
    return lib, f64


@pytest.fixture(autouse=True)
def _no_knobs(monkeypatch):
    for k in ("LBM_TUNE_TILE64_MAX", "LBM_TUNE_TILE64_GEOM", "LBM_TUNE_MAXBLOCKS", "LBM_TUNE_SKEW", "LBM_TUNE_MULTI64_K", "LBM_TUNE_MULTI64_MIN"):
        monkeypatch.delenv(k, raising=False)


def _params(api, nx, ny):
    return api[1].CParams64(nx, ny, 10, 10, 0.1, 0.005, 1.85)


def _any(api, nx, ny, flags=FLAG_ANY):
    lib = api[0]
    plan = PlanMultiAny64()
    assert lib.lbm_plan64_multi_any(C.byref(_params(api, nx, ny)), flags, C.byref(plan)) == 0, lib.lbm_last_error()
    name = C.create_string_buffer(128)
    assert lib.lbm_plan64_multi_any_kernel_name(C.byref(plan), name, 128) == 0
    return plan, name.value.decode()


def _whole(api, nx, ny, flags):
    lib = api[0]
    plan = Plan64()
    assert lib.lbm_plan64_whole(C.byref(_params(api, nx, ny)), flags, C.byref(plan)) == 0, lib.lbm_last_error()
    name = C.create_string_buffer(128)
    assert lib.lbm_plan64_kernel_name(C.byref(plan), name, 128) == 0
    return plan, name.value.decode()


def _multi(api, nx, ny, flags):
    lib = api[0]
    plan = PlanMulti64()
    assert lib.lbm_plan64_multi(C.byref(_params(api, nx, ny)), flags, C.byref(plan)) == 0, lib.lbm_last_error()
    name = C.create_string_buffer(128)
    assert lib.lbm_plan64_multi_kernel_name(C.byref(plan), name, 128) == 0
    return plan, name.value.decode()


def _values(s):
    return [getattr(s, f) for f, _ in s._fields_]


def _launches(api, plan, n):
    cap = n + 1
    steps, full = (C.c_int * cap)(), (C.c_int * cap)()
    count = api[0].lbm_plan64_multi_any_run_launches(C.byref(plan), n, steps, full, cap)
    assert 0 <= count <= cap
    return list(steps[:count]), list(full[:count])


def test_the_mirror_has_the_struct_s_size(api):
    assert api[0].lbm_plan64_multi_any_sizeof() == C.sizeof(PlanMultiAny64) == 14 * 4
    assert api[0].lbm_plan64_multi_sizeof() == C.sizeof(PlanMulti64)           # and the two beside it are what their tests mirror
    assert api[0].lbm_plan64_sizeof() == C.sizeof(Plan64)


def test_eligibility_by_shape(api, monkeypatch):
    monkeypatch.setenv("LBM_TUNE_MULTI64_MIN", "0")
    for nx, ny in EDGE_SHAPES + EDGE_SHAPES_ODD_NY:
        plan, name = _any(api, nx, ny)
        assert (plan.multi_kernel, plan.edge) == (1, 1) and name == f"lbm_multi_kernel_f64<{plan.K},edge>", (nx, ny, name)
        assert _any(api, nx, ny, FLAG_ANY | FLAG_NT)[1] == f"lbm_multi_kernel_f64<{plan.K},nt,edge>"
        assert _any(api, nx, ny, FLAG_ANY | FLAG_NO_NT)[1] == f"lbm_multi_kernel_f64<{plan.K},edge>"
        assert _any(api, nx, ny, FLAG_ANY | FLAG_MULTI)[1] == name
        for flags in (0, FLAG_NT, FLAG_TILE, FLAG_MULTI, FLAG_MULTI | FLAG_TILE):     # nothing without the flag, 1024 included
            plan, name = _any(api, nx, ny, flags)
            assert (plan.multi_kernel, plan.edge, name) == (0, 0, ""), (nx, ny, flags)
    for nx, ny in EXACT_SHAPES:
        for flags in (FLAG_ANY, FLAG_MULTI, FLAG_ANY | FLAG_MULTI):
            plan, name = _any(api, nx, ny, flags)
            assert (plan.multi_kernel, plan.edge) == (1, 0) and name == f"lbm_multi_kernel_f64<{plan.K}>", (nx, ny, flags, name)
            assert name == _multi(api, nx, ny, FLAG_MULTI)[1]
        assert _any(api, nx, ny, FLAG_ANY | FLAG_NT)[1] == f"lbm_multi_kernel_f64<{plan.K},nt>"
        assert _any(api, nx, ny, 0)[0].multi_kernel == 0
    for nx, ny in ONE_STEP_SHAPES:
        plan, name = _any(api, nx, ny)
        assert (plan.multi_kernel, plan.edge, plan.n_tiles, name) == (0, 0, 0, ""), (nx, ny)
        assert _whole(api, nx, ny, FLAG_ANY)[1] == _whole(api, nx, ny, 0)[1] == f"lbm_step_kernel_f64<{2 if nx % 2 == 0 else 1}>"


def test_the_tiled_kernel_comes_first(api, monkeypatch):
    monkeypatch.setenv("LBM_TUNE_MULTI64_MIN", "0")
    whole, name = _whole(api, 136, 136, FLAG_TILE | FLAG_ANY)                   # 8 x 8 tiles of the tiled kernel cover it, 32 x 16 do not
    assert whole.tile_kernel == 1 and name.startswith("lbm_tile_kernel_f64<")
    assert _any(api, 136, 136, FLAG_TILE | FLAG_ANY)[0].multi_kernel == 0
    assert _any(api, 136, 136, FLAG_ANY)[0].edge == 1
    monkeypatch.setenv("LBM_TUNE_TILE64_MAX", str(136 * 136 - 1))
    assert _any(api, 136, 136, FLAG_TILE | FLAG_ANY)[0].edge == 1


def test_the_minimum_size(api, monkeypatch):
    """The knob and the default are lbm_multi_kernel_f64's (profiles/r20/f64_multi_any.txt: the edge form clears the bar at every
    measured size, so it keeps them)."""
    monkeypatch.setenv("LBM_TUNE_MULTI64_MIN", str(66 * 64))
    assert _any(api, 66, 63)[0].multi_kernel == 0
    assert _any(api, 66, 64)[0].edge == 1
    monkeypatch.setenv("LBM_TUNE_MULTI64_MIN", str(66 * 64 + 1))
    assert _any(api, 66, 64)[0].multi_kernel == 0
    monkeypatch.delenv("LBM_TUNE_MULTI64_MIN")
    assert DEFAULT_MIN == 1 << 20
    assert _any(api, 1026, 1022)[0].multi_kernel == 0                          # 1 048 572 cells
    assert _any(api, 1026, 1023)[0].edge == 1
    plan, name = _any(api, 8190, 8190)
    assert (plan.edge, plan.K) == (1, DEFAULT_K) and name == f"lbm_multi_kernel_f64<{DEFAULT_K},nt,edge>"
    assert _any(api, 1000, 1000)[0].multi_kernel == 0 and _any(api, 1000, 1050)[0].edge == 1


@pytest.mark.parametrize("value", ["0", "1", "5", "-3", "abc", "33", "3x"])
def test_malformed_steps_per_launch_get_the_default(api, monkeypatch, value):
    monkeypatch.setenv("LBM_TUNE_MULTI64_MIN", "0")
    monkeypatch.setenv("LBM_TUNE_MULTI64_K", value)
    plan, name = _any(api, 62, 31)
    assert plan.K == (3 if value == "3x" else DEFAULT_K)                       # atoi reads the leading number
    assert plan.edge == 1 and name == f"lbm_multi_kernel_f64<{plan.K},edge>"


@pytest.mark.parametrize("K", BUILT_K)
def test_every_built_k_and_its_block(api, monkeypatch, K):
    monkeypatch.setenv("LBM_TUNE_MULTI64_MIN", "0")
    monkeypatch.setenv("LBM_TUNE_MULTI64_K", str(K))
    plan, name = _any(api, 66, 35)
    exact = _multi(api, 96, 48, FLAG_MULTI)[0]
    assert (plan.multi_kernel, plan.edge, plan.K) == (1, 1, K) and name == f"lbm_multi_kernel_f64<{K},edge>"
    assert (plan.TX, plan.TY, plan.block, plan.lds_bytes) == (TX, TY, exact.block, exact.lds_bytes)      # the frame and block of the existing form
    assert plan.block == TX * TY == 512 and 9 * 8 * frame_cells(K) <= plan.lds_bytes <= LDS_PER_WORKGROUP
    assert plan.n_tiles == 9 and plan.partials_cap == K * plan.n_tiles + 1


@pytest.mark.parametrize("K", BUILT_K)
def test_run_launches(api, monkeypatch, K):
    monkeypatch.setenv("LBM_TUNE_MULTI64_MIN", "0")
    monkeypatch.setenv("LBM_TUNE_MULTI64_K", str(K))
    for shape in ((66, 35), (64, 48)):
        plan, _ = _any(api, *shape)
        assert plan.multi_kernel == 1
        assert _launches(api, plan, 0) == ([], [])
        for n in range(1, 3 * K + 2):
            steps, full = _launches(api, plan, n)
            assert sum(steps) == n and all(1 <= k <= K for k in steps)
            assert full == [int(k == K) for k in steps]
            assert all(f for f in full[:-1])                                  # the short launch, if any, is the tail
            assert sum(1 for f in full if not f) <= 1 and len(steps) == -(-n // K)
        assert api[0].lbm_plan64_multi_any_run_launches(C.byref(plan), -1, None, None, 0) == -1


@pytest.mark.parametrize("nx,ny", EDGE_SHAPES + EDGE_SHAPES_ODD_NY + EXACT_SHAPES + [(66, 35), (8190, 4100)])
def test_tile_counts_and_last_tile_starts(api, monkeypatch, nx, ny):
    monkeypatch.setenv("LBM_TUNE_MULTI64_MIN", "0")
    plan, _ = _any(api, nx, ny)
    assert (plan.tiles_x, plan.tiles_y) == (-(-nx // TX), -(-ny // TY)) and plan.n_tiles == plan.tiles_x * plan.tiles_y
    assert (plan.last_x0, plan.last_y0) == (nx - TX, ny - TY)
    assert plan.last_x0 % 2 == 0 and 0 <= plan.last_x0 and 0 <= plan.last_y0
    assert plan.last_x0 <= TX * (plan.tiles_x - 1) and plan.last_y0 <= TY * (plan.tiles_y - 1)      # the last tiles reach back, never forward
    assert plan.partials_cap == plan.K * plan.n_tiles + 1
    whole, _ = _whole(api, nx, ny, FLAG_ANY)
    assert plan.nt_stores == whole.nt_stores


def owners(nx, ny, tiles_x, tiles_y, last_x0, last_y0):
    """The kernel's ownership rule restated: tile (tx, ty) starts at (min(TX tx, last_x0), min(TY ty, last_y0)) and owns its cells
    at tile-local x >= TX tx - x0, y >= TY ty - y0.  Returns how many tiles own each cell, and the x bounds."""
    count = np.zeros((ny, nx), np.int32)
    bounds = []
    for ty in range(tiles_y):
        for tx in range(tiles_x):
            x0, y0 = min(TX * tx, last_x0), min(TY * ty, last_y0)
            own_x, own_y = TX * tx - x0, TY * ty - y0
            assert 0 <= x0 and x0 + TX <= nx and 0 <= y0 and y0 + TY <= ny    # the tile lies inside the grid
            assert 0 <= own_x < TX and 0 <= own_y < TY                        # and owns at least one column and row
            count[y0 + own_y:y0 + TY, x0 + own_x:x0 + TX] += 1
            bounds.append((x0, own_x))
    return count, bounds


@pytest.mark.parametrize("nx,ny", EDGE_SHAPES + EDGE_SHAPES_ODD_NY + [(66, 35), (96, 50), (34, 18), (1000, 600)])
def test_every_cell_has_exactly_one_owner(api, monkeypatch, nx, ny):
    monkeypatch.setenv("LBM_TUNE_MULTI64_MIN", "0")
    plan, _ = _any(api, nx, ny)
    assert plan.edge == 1
    count, bounds = owners(nx, ny, plan.tiles_x, plan.tiles_y, plan.last_x0, plan.last_y0)
    assert count.min() == 1 and count.max() == 1
    assert all(x0 % 2 == 0 and own_x % 2 == 0 for x0, own_x in bounds)         # x-pairs are aligned and owned whole


@pytest.mark.parametrize("nx,ny", [(8, 3), (7, 5), (32, 16), (40, 24), (64, 48), (258, 33), (258, 34), (1024, 1024), (1024, 1040), (8192, 7296)])
def test_existing_plans_with_the_bit(api, monkeypatch, nx, ny):
    """Plan64 does not change with the bit (but for .flags, which records it).  PlanMulti64 under 4096 is PlanMulti64 under 1024 on a
    grid the tiles cover, and "no multi kernel" on any other."""
    fields = [f for f, _ in Plan64._fields_ if f != "flags"]
    for base in (0, FLAG_NT, FLAG_NO_NT, FLAG_TILE, FLAG_TILE | FLAG_NT):
        for minimum in (None, "0"):
            if minimum is None:
                monkeypatch.delenv("LBM_TUNE_MULTI64_MIN", raising=False)
            else:
                monkeypatch.setenv("LBM_TUNE_MULTI64_MIN", minimum)
            off, name_off = _whole(api, nx, ny, base)
            for bits in (FLAG_ANY, FLAG_ANY | FLAG_MULTI):
                on, name_on = _whole(api, nx, ny, base | bits)
                assert on.flags == base | bits and name_on == name_off
                assert [getattr(on, f) for f in fields] == [getattr(off, f) for f in fields]
                m_on, m_name_on = _multi(api, nx, ny, base | bits)
                m_1024, m_name_1024 = _multi(api, nx, ny, base | FLAG_MULTI)
                assert _values(m_on) == _values(m_1024) and m_name_on == m_name_1024
                if nx % TX or ny % TY:
                    assert m_on.multi_kernel == 0 and m_name_on == ""
                # and where the existing form runs, the new plan says what PlanMulti64 says
                a, a_name = _any(api, nx, ny, base | bits)
                if m_on.multi_kernel:
                    assert a.edge == 0 and a_name == m_name_on
                    assert (a.multi_kernel, a.K, a.TX, a.TY, a.tiles_x, a.n_tiles, a.block, a.lds_bytes, a.nt_stores, a.partials_cap) == tuple(_values(m_on))


def test_refusals(api):
    lib, _ = api
    plan = PlanMultiAny64()
    for nx, ny, flags in ((0, 4, 0), (8, 2, 0), (8, 8, 256), (8, 8, 4), (8, 8, FLAG_TILE | 64), (64, 64, 2048), (64, 64, 8192)):
        for extra in (0, FLAG_ANY):
            assert lib.lbm_plan64_multi_any(C.byref(_params(api, nx, ny)), flags | extra, C.byref(plan)) == 1
    assert lib.lbm_plan64_multi_any(C.byref(_params(api, 64, 64)), FLAG_ANY, None) == 1
    assert lib.lbm_plan64_multi_any_kernel_name(None, C.create_string_buffer(8), 8) == 1


def test_row_partitions_keep_refusing_the_flag(lbm, api):
    lib, f64 = api
    room = C.create_string_buffer(256)
    for flags in (FLAG_ANY, FLAG_ANY | 2048, FLAG_ANY | FLAG_NT):
        for fn in (lib.lbm_plan64_rows, lib.lbm_plan64_rows_multi):
            assert fn(C.byref(_params(api, 34, 34)), 2, 0, flags, room) == 1
            assert "LBM_FLAG_NT_STORES or LBM_FLAG_NO_NT_STORES only" in lib.lbm_last_error().decode()
    p = lbm.Params(nx=34, ny=34, max_iters=1, reynolds_dim=1, density=0.1, accel=0.005, omega=1.85)
    with pytest.raises(lbm.LbmError, match="LBM_FLAG_NT_STORES or LBM_FLAG_NO_NT_STORES only"):
        f64.Rows64(p, np.zeros((34, 34), np.int32), 2, devices=[4096, 4096], flags=FLAG_ANY)


def test_create_accepts_the_flag_before_any_hip_call(lbm, api):
    """With a device ordinal that no machine has, the first HIP call fails: the flag was accepted before it, wherever 1024 is."""
    f64 = api[1]
    assert f64.FLAG_MULTI_ANY_SIZE == FLAG_ANY
    p = lbm.Params(nx=34, ny=18, max_iters=1, reynolds_dim=1, density=0.1, accel=0.005, omega=1.85)
    obst = np.zeros((18, 34), np.int32)
    for flags in (FLAG_ANY, FLAG_ANY | FLAG_NT, FLAG_ANY | FLAG_NO_NT, FLAG_ANY | FLAG_TILE, FLAG_ANY | FLAG_MULTI, FLAG_ANY | FLAG_TILE | FLAG_MULTI | FLAG_NT):
        with pytest.raises(lbm.LbmError, match="hipSetDevice"):
            f64.Grid64(p, obst, device=4096, flags=flags)
    for flags in (FLAG_ANY | 2048, FLAG_ANY | 256, FLAG_ANY | 8192):
        with pytest.raises(lbm.LbmError, match="lbm64_create: the double-precision mode takes"):
            f64.Grid64(p, obst, device=4096, flags=flags)


def test_a_c99_caller_sees_the_macro(lbm, tmp_path):
    src = tmp_path / "caller.c"
    src.write_text('''
#include <stdio.h>
#include "lbm_d2q9_f64.h"
int main(void)
{
  lbm64_params p = {34, 18, 10, 10, 0.1, 0.005, 1.85};
  static int obstacles[34 * 18];
  lbm64_ctx* ctx = NULL;
  if (LBM64_FLAG_MULTI_ANY_SIZE != 4096u || LBM64_ABI_VERSION != 1 || lbm64_abi_version() != 1) return 2;
  if ((LBM64_FLAG_MULTI_ANY_SIZE & (LBM_FLAG_NT_STORES | LBM_FLAG_NO_NT_STORES | LBM64_FLAG_TILE_STEPS | LBM64_FLAG_MULTI_STEPS)) != 0u) return 3;
  if (lbm64_create(&ctx, &p, 34 * 18, obstacles, 4096, LBM64_FLAG_MULTI_ANY_SIZE | LBM_FLAG_NT_STORES) != 1 || ctx != NULL) return 4;
  printf("%s\\n", lbm_last_error());
  return lbm64_destroy(NULL);
}
''')
    exe = tmp_path / "caller"
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-L",
                        os.path.dirname(lbm.LIB_PATH), "-llbm_d2q9", f"-Wl,-rpath,{os.path.dirname(lbm.LIB_PATH)}", "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "hipSetDevice" in r.stdout, (r.returncode, r.stdout, r.stderr)


def test_cli_takes_the_flag(lbm, digests, tmp_path):
    """LBM_PRECISION=double LBM_FLAGS=4096, alone and with 1, 2, 512 and 1024, reaches lbm64_create, which accepts it."""
    from conftest import deck_paths
    ppath, opath = deck_paths("rand_64x48", digests)
    base = {k: v for k, v in os.environ.items() if not k.startswith("LBM")}
    for flags in ("4096", "4097", "4098", "4608", "5120", "5633"):
        r = subprocess.run([lbm.CLI_PATH, ppath, opath], cwd=tmp_path, env={**base, "LBM_PRECISION": "double", "LBM_FLAGS": flags, "LBM_DEVICE": "4096"},
                           capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "hipSetDevice" in r.stderr and "the double-precision mode takes" not in r.stderr, (flags, r.stderr)


def test_exports_and_code_object(lbm):
    import re
    nm = subprocess.run(["nm", "-D", "--defined-only", lbm.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert {"lbm_plan64_multi_any", "lbm_plan64_multi_any_sizeof", "lbm_plan64_multi_any_kernel_name",
            "lbm_plan64_multi_any_run_launches"} <= set(re.findall(r" T (lbm_plan64_[a-z_0-9]+)", nm))
    from mpilattice_boltzmann_amd import f64
    assert set(re.findall(r" T (lbm64_[a-z_0-9]+)", nm)) == set(f64.EXPORTS) and len(f64.EXPORTS) == 15
    assert f64.load_library().lbm64_abi_version() == 1
