"""The plan of a row-partitioned double-precision run under LBM_ROWS64_FLAG_MULTI_ANY_SIZE (csrc/lbm_plan.cpp plan64_rows_multi_any,
PlanRowsMultiAny64 of lbm_internal.h) through the lbm_plan64_rows_multi_any* entry points, without a GPU: which runs take the edge-tile
form of lbm_rows_multi_kernel_f64 and with what tiles on each rank; that every owned cell of a rank has one owning tile and that
sub-step 1 stays inside a rank's storage rows, worked out in numpy from the plan's fields alone; the exactly covered runs, which are
PlanRowsMulti64's; the fallbacks; the refusals; the header's macro from C99; the exported symbols; the CLI's switches."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from test_f64_rows_host import PlanRows64
from test_plan64_rows_multi import BUILT_K, DEFAULT_K, DEFAULT_MIN, LANES, TX, TY, PlanRowsMulti64, multi64_lds_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAG_NT, FLAG_NO_NT, FLAG_TILE, FLAG_MULTI, FLAG_ROWS_MULTI, FLAG_ANY, FLAG_ROWS_ANY = 1, 2, 512, 1024, 2048, 4096, 8192


class PlanRowsMultiAny64(C.Structure):
    """struct PlanRowsMultiAny64 (lbm_internal.h), field for field."""

    _fields_ = [("multi_kernel", C.c_int), ("edge", C.c_int), ("K", C.c_int), ("ghost", C.c_int),
                ("tiles_x", C.c_int), ("tiles_y", C.c_int), ("n_tiles", C.c_int), ("last_x0", C.c_int), ("last_y0", C.c_int),
                ("block", C.c_int), ("lds_bytes", C.c_int), ("nt_stores", C.c_int), ("mask_words", C.c_int), ("partials_cap", C.c_int),
                ("ps", C.c_longlong), ("grid_doubles", C.c_longlong)]


@pytest.fixture(scope="module")
def f64(lbm):
    from mpilattice_boltzmann_amd import f64 as mod
    mod.load_rows_library()
    return mod


@pytest.fixture(scope="module")
def api(lbm, f64):
    lib = lbm.load_library()
    P = C.POINTER
    lib.lbm_plan64_rows_sizeof.restype, lib.lbm_plan64_rows_sizeof.argtypes = C.c_int, []
    lib.lbm_plan64_rows.restype, lib.lbm_plan64_rows.argtypes = C.c_int, [P(f64.CParams64), C.c_int, C.c_int, C.c_uint, P(PlanRows64)]
    lib.lbm_plan64_rows_kernel_name.restype, lib.lbm_plan64_rows_kernel_name.argtypes = C.c_int, [P(PlanRows64), C.c_char_p, C.c_size_t]
    lib.lbm_plan64_rows_multi_sizeof.restype, lib.lbm_plan64_rows_multi_sizeof.argtypes = C.c_int, []
    lib.lbm_plan64_rows_multi.restype = C.c_int
    lib.lbm_plan64_rows_multi.argtypes = [P(f64.CParams64), C.c_int, C.c_int, C.c_uint, P(PlanRowsMulti64)]
    lib.lbm_plan64_rows_multi_kernel_name.restype, lib.lbm_plan64_rows_multi_kernel_name.argtypes = C.c_int, [P(PlanRowsMulti64), C.c_char_p, C.c_size_t]
    lib.lbm_plan64_rows_multi_any_sizeof.restype, lib.lbm_plan64_rows_multi_any_sizeof.argtypes = C.c_int, []
    lib.lbm_plan64_rows_multi_any.restype = C.c_int
    lib.lbm_plan64_rows_multi_any.argtypes = [P(f64.CParams64), C.c_int, C.c_int, C.c_uint, P(PlanRowsMultiAny64)]
    lib.lbm_plan64_rows_multi_any_kernel_name.restype = C.c_int
    lib.lbm_plan64_rows_multi_any_kernel_name.argtypes = [P(PlanRowsMultiAny64), C.c_char_p, C.c_size_t]
    lib.lbm_plan64_rows_multi_any_run_launches.restype = C.c_int
    lib.lbm_plan64_rows_multi_any_run_launches.argtypes = [P(PlanRowsMultiAny64), C.c_int, P(C.c_int), P(C.c_int), C.c_int]
    return lib


@pytest.fixture(autouse=True)
def _no_knobs(monkeypatch):
    for k in ("LBM_TUNE_MAXBLOCKS", "LBM_TUNE_SKEW", "LBM_TUNE_MULTI64_K", "LBM_TUNE_MULTI64_MIN"):
        monkeypatch.delenv(k, raising=False)


def _params(f64, nx, ny):
    return f64.CParams64(nx, ny, 10, 10, 0.1, 0.005, 1.85)


def _rows(api, f64, nx, ny, nranks, rank, flags):
    plan, name = PlanRows64(), C.create_string_buffer(128)
    rc = api.lbm_plan64_rows(C.byref(_params(f64, nx, ny)), nranks, rank, flags, C.byref(plan))
    if rc == 0:
        assert api.lbm_plan64_rows_kernel_name(C.byref(plan), name, 128) == 0
    return rc, plan, name.value.decode()


def _multi(api, f64, nx, ny, nranks, rank, flags):
    plan, name = PlanRowsMulti64(), C.create_string_buffer(128)
    rc = api.lbm_plan64_rows_multi(C.byref(_params(f64, nx, ny)), nranks, rank, flags, C.byref(plan))
    if rc == 0:
        assert api.lbm_plan64_rows_multi_kernel_name(C.byref(plan), name, 128) == 0
    return rc, plan, name.value.decode()


def _any(api, f64, nx, ny, nranks, rank, flags=FLAG_ROWS_ANY):
    plan, name = PlanRowsMultiAny64(), C.create_string_buffer(128)
    rc = api.lbm_plan64_rows_multi_any(C.byref(_params(f64, nx, ny)), nranks, rank, flags, C.byref(plan))
    if rc == 0:
        assert api.lbm_plan64_rows_multi_any_kernel_name(C.byref(plan), name, 128) == 0
    return rc, plan, name.value.decode()


def _values(plan):
    return [getattr(plan, f) for f, _ in plan._fields_]


def test_layout_mirror(api):
    assert api.lbm_plan64_rows_multi_any_sizeof() == C.sizeof(PlanRowsMultiAny64) == 14 * 4 + 2 * 8
    assert api.lbm_plan64_rows_multi_sizeof() == C.sizeof(PlanRowsMulti64)        # the two plans beside it are what they were
    assert api.lbm_plan64_rows_sizeof() == C.sizeof(PlanRows64)


# (nx, ny, ranks, rows per rank): the shapes of tests/test_f64_rows_any.py, then 8190 x 8190 on 8 and the reference's own uneven rule
EDGE_SHAPES = [(34, 18, 1, [18]), (32, 33, 2, [17, 16]), (34, 35, 2, [18, 17]), (66, 50, 3, [17, 17, 16]), (62, 31, 1, [31]),
               (96, 52, 3, [18, 17, 17]), (258, 34, 2, [17, 17]), (1000, 600, 4, [150] * 4), (4098, 2050, 8, [257, 257] + [256] * 6),
               (8190, 8190, 8, [1024] * 6 + [1023] * 2), (1024, 190, 6, [32, 32, 32, 32, 31, 31])]


@pytest.mark.parametrize("K", [None, 2, 3])
@pytest.mark.parametrize("nx,ny,nranks,rows", EDGE_SHAPES)
def test_edge_form_geometry(lbm, api, f64, monkeypatch, nx, ny, nranks, rows, K):
    monkeypatch.setenv("LBM_TUNE_MULTI64_MIN", "0")
    if K is not None:
        monkeypatch.setenv("LBM_TUNE_MULTI64_K", str(K))
    K = DEFAULT_K if K is None else K
    nyls, dis = lbm.decompose(ny, nranks)
    assert list(nyls) == rows and min(rows) >= TY
    plans = []
    for r in range(nranks):
        nyl = rows[r]
        rc, a, name = _any(api, f64, nx, ny, nranks, r)
        assert rc == 0, lbm.load_library().lbm_last_error()
        storage = nx * (nyl + 2 * K)
        nt = 2 * 9 * 8 * storage > 192 << 20                              # plan64_whole's rule on the rank's two grids
        assert (a.multi_kernel, a.edge, a.K, a.ghost) == (1, 1, K, K)
        assert (a.tiles_x, a.tiles_y, a.n_tiles) == (-(-nx // TX), -(-nyl // TY), -(-nx // TX) * -(-nyl // TY))
        assert (a.last_x0, a.last_y0) == (nx - TX, nyl - TY)
        assert a.block == LANES and a.lds_bytes == multi64_lds_bytes(K) and a.lds_bytes <= 65536
        assert a.nt_stores == int(nt) and name == (f"lbm_rows_multi_kernel_f64<{K},nt,edge>" if nt else f"lbm_rows_multi_kernel_f64<{K},edge>")
        assert a.ps % 2 == 0 and a.ps >= storage + 64 and a.grid_doubles == 9 * a.ps + 128
        assert a.mask_words * 32 >= storage and a.partials_cap == K * a.n_tiles + 1
        assert _any(api, f64, nx, ny, nranks, r, FLAG_ROWS_ANY | FLAG_NT)[2] == f"lbm_rows_multi_kernel_f64<{K},nt,edge>"
        assert _any(api, f64, nx, ny, nranks, r, FLAG_ROWS_ANY | FLAG_NO_NT)[2] == f"lbm_rows_multi_kernel_f64<{K},edge>"
        assert _values(_any(api, f64, nx, ny, nranks, r, FLAG_ROWS_ANY | FLAG_ROWS_MULTI)[1]) == _values(a)      # 8192 means 2048
        # the storage is PlanRowsMulti64's; without the new flag nothing runs the kernel here
        for flags in (0, FLAG_NT, FLAG_ROWS_MULTI):
            rc, off, name_off = _any(api, f64, nx, ny, nranks, r, flags)
            assert rc == 0 and (off.multi_kernel, off.edge) == (0, 0) and name_off == ""
        _, m, m_name = _multi(api, f64, nx, ny, nranks, r, FLAG_ROWS_ANY)
        assert (m.multi_kernel, m.n_tiles, m_name) == (0, 0, "")
        assert (m.K, m.ghost, m.block, m.lds_bytes, m.nt_stores, m.mask_words, m.ps, m.grid_doubles) == \
               (a.K, a.ghost, a.block, a.lds_bytes, a.nt_stores, a.mask_words, a.ps, a.grid_doubles)
        # PlanRows64 is the one-step plan whatever the flag says
        _, off, name_off = _rows(api, f64, nx, ny, nranks, r, 0)
        _, on, name_on = _rows(api, f64, nx, ny, nranks, r, FLAG_ROWS_ANY)
        assert on.flags == FLAG_ROWS_ANY and name_on == name_off
        assert _values(on)[1:] == _values(off)[1:]
        plans.append(a)
    # one decision for all ranks: they agree on these and may differ in the rest
    assert len({(a.multi_kernel, a.edge, a.K, a.ghost, a.tiles_x, a.last_x0, a.block, a.lds_bytes) for a in plans}) == 1
    if len(set(rows)) > 1:
        assert len({(a.last_y0, a.mask_words, a.ps) for a in plans}) > 1


@pytest.mark.parametrize("nx,ny,nranks", [(32, 16, 1), (64, 48, 3), (1024, 1024, 8), (8192, 8192, 8)])
def test_exactly_covered_runs_are_the_2048_plan(api, f64, monkeypatch, nx, ny, nranks):
    """Where 32 x 16 tiles cover every rank, 8192 gives what 2048 gives: edge == 0, PlanRowsMulti64's values and its kernel name."""
    monkeypatch.setenv("LBM_TUNE_MULTI64_MIN", "0")
    for r in range(nranks):
        _, m, m_name = _multi(api, f64, nx, ny, nranks, r, FLAG_ROWS_MULTI)
        assert m.multi_kernel == 1 and m_name.startswith("lbm_rows_multi_kernel_f64<") and "edge" not in m_name
        nyl = ny // nranks
        for flags in (FLAG_ROWS_ANY, FLAG_ROWS_MULTI, FLAG_ROWS_ANY | FLAG_ROWS_MULTI):
            rc, a, name = _any(api, f64, nx, ny, nranks, r, flags)
            assert rc == 0 and (a.multi_kernel, a.edge) == (1, 0) and name == m_name
            assert (a.K, a.ghost, a.tiles_x, a.n_tiles, a.block, a.lds_bytes, a.nt_stores, a.mask_words, a.partials_cap, a.ps, a.grid_doubles) == \
                   (m.K, m.ghost, m.tiles_x, m.n_tiles, m.block, m.lds_bytes, m.nt_stores, m.mask_words, m.partials_cap, m.ps, m.grid_doubles)
            assert (a.tiles_y, a.last_x0, a.last_y0) == (nyl // TY, nx - TX, nyl - TY)
        _, m_any, m_any_name = _multi(api, f64, nx, ny, nranks, r, FLAG_ROWS_ANY)              # and PlanRowsMulti64 itself under the new flag
        assert _values(m_any) == _values(m) and m_any_name == m_name
        assert _any(api, f64, nx, ny, nranks, r, 0)[1].multi_kernel == 0


def test_ownership_and_bounds_from_the_plan_alone(lbm, api, f64, monkeypatch):
    """For every run of the sweep that the plan gives the edge form, from the plan's fields and the kernel's two rules (tile (tx, ty)
    starts at x0 = min(32 tx, last_x0), owned row y0 = min(16 ty, last_y0); it owns its cells at tile-local x >= 32 tx - x0 and
    y >= 16 ty - y0): every owned cell of every rank has exactly one owning tile, and a launch of k = 1 .. K steps reads, in sub-step 1
    (the region grown by e = k - 1 rows, whose pull reads one row further), storage rows within [0, nyl + 2 K)."""
    monkeypatch.setenv("LBM_TUNE_MULTI64_MIN", "0")
    seen = {"edge": 0, "exact": 0, "fallback": 0, "uneven": 0}
    for K in BUILT_K:
        monkeypatch.setenv("LBM_TUNE_MULTI64_K", str(K))
        for nx in (32, 34, 62, 64, 66, 258):
            for ny in range(16, 71):
                for nranks in range(1, 5):
                    try:
                        nyls, _ = lbm.decompose(ny, nranks)
                    except Exception:
                        continue
                    if min(nyls) < 1 or nyls[-1] < 3:
                        continue
                    plans = [_any(api, f64, nx, ny, nranks, r) for r in range(nranks)]
                    assert all(rc == 0 for rc, _, _ in plans)
                    assert len({(a.multi_kernel, a.edge) for _, a, _ in plans}) == 1
                    a0 = plans[0][1]
                    assert a0.multi_kernel == int(min(nyls) >= TY) and a0.edge == int(a0.multi_kernel and not (nx % TX == 0 and all(n % TY == 0 for n in nyls)))
                    seen["edge" if a0.edge else "exact" if a0.multi_kernel else "fallback"] += 1
                    if not a0.edge:
                        continue
                    seen["uneven"] += len(set(nyls)) > 1
                    for r, (_, a, _) in enumerate(plans):
                        nyl = nyls[r]
                        assert a.K == a.ghost == K
                        owners = np.zeros((nyl, nx), np.int32)
                        for ty in range(a.tiles_y):
                            y0 = min(TY * ty, a.last_y0)
                            assert 0 <= y0 <= nyl - TY
                            for tx in range(a.tiles_x):
                                x0 = min(TX * tx, a.last_x0)
                                assert 0 <= x0 <= nx - TX and x0 % 2 == 0
                                owners[TY * ty:y0 + TY, TX * tx:x0 + TX] += 1           # tile-local x >= 32 tx - x0, y >= 16 ty - y0
                            for k in range(1, K + 1):
                                e = k - 1
                                lo, hi = a.ghost + y0 - e - 1, a.ghost + y0 + TY + e - 1 + 1     # the rows pulled from, one further each way
                                assert 0 <= lo and hi < nyl + 2 * K, (nx, ny, nranks, r, ty, k)
                        assert owners.min() == 1 and owners.max() == 1, (nx, ny, nranks, r)
    assert seen["edge"] > 1000 and seen["exact"] > 0 and seen["fallback"] > 0 and seen["uneven"] > 100, seen


# odd nx; nx < 32; a rank of 15 rows (16, 16, 15); and, with no knob set, a smallest rank below the default minimum
FALLBACKS = [(33, 32, 2, True), (30, 32, 2, True), (64, 47, 3, True), (1022, 250, 2, False)]


@pytest.mark.parametrize("nx,ny,nranks,force", FALLBACKS)
def test_fallback_plans(lbm, api, f64, monkeypatch, nx, ny, nranks, force):
    if force:
        monkeypatch.setenv("LBM_TUNE_MULTI64_MIN", "0")
    else:
        assert nx * min(lbm.decompose(ny, nranks)[0]) < DEFAULT_MIN
    if (nx, ny, nranks) == (64, 47, 3):
        assert list(lbm.decompose(ny, nranks)[0]) == [16, 16, 15]
    fields = [f for f, _ in PlanRows64._fields_ if f != "flags"]
    for r in range(nranks):
        for extra in (0, FLAG_ROWS_MULTI):
            rc, a, name = _any(api, f64, nx, ny, nranks, r, FLAG_ROWS_ANY | extra)
            assert rc == 0 and (a.multi_kernel, a.edge) == (0, 0) and name == ""
        for base in (0, FLAG_NT, FLAG_NO_NT):
            rc_off, off, name_off = _rows(api, f64, nx, ny, nranks, r, base)
            rc_on, on, name_on = _rows(api, f64, nx, ny, nranks, r, base | FLAG_ROWS_ANY)
            assert rc_off == rc_on == 0 and on.flags == base | FLAG_ROWS_ANY and off.flags == base
            lane = 2 if nx % 2 == 0 else 1
            assert name_on == name_off == (f"lbm_rows_kernel_f64<{lane},nt>" if base == FLAG_NT else f"lbm_rows_kernel_f64<{lane}>")
            assert [getattr(on, f) for f in fields] == [getattr(off, f) for f in fields]


def test_the_minimum_size_is_the_smallest_rank_s(api, f64, monkeypatch):
    """66 x 50 on 3 ranks: rows 17, 17, 16."""
    monkeypatch.setenv("LBM_TUNE_MULTI64_MIN", str(66 * 16))
    assert [_any(api, f64, 66, 50, 3, r)[1].edge for r in range(3)] == [1, 1, 1]
    monkeypatch.setenv("LBM_TUNE_MULTI64_MIN", str(66 * 16 + 1))
    assert [_any(api, f64, 66, 50, 3, r)[1].multi_kernel for r in range(3)] == [0, 0, 0]
    assert _any(api, f64, 66, 50, 1, 0)[1].edge == 1


def test_defaults_without_the_knobs(api, f64):
    """The default minimum is plan64_rows_multi's, 2^17 cells of the smallest rank, and the default K its 4: 4098 x 2050 on 8 ranks
    (the smallest rank 256 rows, 2^20 cells and more) and 8190 x 8190 on 8 take the edge form."""
    for nx, ny in ((4098, 2050), (8190, 8190)):
        for r in (0, 7):
            rc, a, name = _any(api, f64, nx, ny, 8, r)
            assert rc == 0 and (a.multi_kernel, a.edge, a.K) == (1, 1, DEFAULT_K) and name.endswith("edge>")
    assert _any(api, f64, 8190, 8190, 8, 0)[2] == f"lbm_rows_multi_kernel_f64<{DEFAULT_K},nt,edge>"
    assert _any(api, f64, 1022, 2 * (DEFAULT_MIN // 1022 + 1), 2, 0)[1].edge == 1
    assert _any(api, f64, 1022, 2 * (DEFAULT_MIN // 1022), 2, 0)[1].multi_kernel == 0


@pytest.mark.parametrize("K", BUILT_K)
def test_run_launches(api, f64, monkeypatch, K):
    monkeypatch.setenv("LBM_TUNE_MULTI64_MIN", "0")
    monkeypatch.setenv("LBM_TUNE_MULTI64_K", str(K))
    _, plan, _ = _any(api, f64, 66, 50, 3, 2)
    assert plan.edge == 1
    for n in range(0, 3 * K + 2):
        cap = n + 1
        steps, full = (C.c_int * cap)(), (C.c_int * cap)()
        count = api.lbm_plan64_rows_multi_any_run_launches(C.byref(plan), n, steps, full, cap)
        steps, full = list(steps[:count]), list(full[:count])
        assert count == -(-n // K) and sum(steps) == n and full == [int(k == K) for k in steps] and all(full[:-1])
    assert api.lbm_plan64_rows_multi_any_run_launches(C.byref(plan), -1, None, None, 0) == -1


def test_refusals_and_acceptances(lbm, api, f64):
    lib = lbm.load_library()
    for flags in (FLAG_ROWS_ANY, FLAG_ROWS_ANY | FLAG_ROWS_MULTI, FLAG_ROWS_ANY | FLAG_NT, FLAG_ROWS_ANY | FLAG_NO_NT):
        assert _rows(api, f64, 34, 35, 2, 0, flags)[0] == 0 and _any(api, f64, 34, 35, 2, 0, flags)[0] == 0
    for flags in (FLAG_ROWS_ANY | FLAG_TILE, FLAG_ROWS_ANY | FLAG_MULTI, FLAG_ROWS_ANY | FLAG_ROWS_MULTI | FLAG_MULTI):
        for fn in (_rows, _any):
            assert fn(api, f64, 34, 35, 2, 0, flags)[0] == 1
            assert "several steps per exchange are not built" in lib.lbm_last_error().decode()
    for flags in (FLAG_ROWS_ANY | FLAG_ANY, FLAG_ANY, FLAG_ROWS_ANY | 256, FLAG_ROWS_ANY | 16384):
        for fn in (_rows, _any):
            assert fn(api, f64, 34, 35, 2, 0, flags)[0] == 1
            assert "LBM_FLAG_NT_STORES or LBM_FLAG_NO_NT_STORES only" in lib.lbm_last_error().decode()
    assert api.lbm_plan64_rows_multi_any(C.byref(_params(f64, 34, 35)), 2, 0, FLAG_ROWS_ANY, None) == 1
    for nx, ny, nranks in ((0, 16, 2), (8, 2, 1), (8, 5, 3), (8, 3, 3), (8, 16, 0), (8, 16, 65)):
        assert _any(api, f64, nx, ny, nranks, 0)[0] == 1


def test_whole_grids_keep_refusing_the_flag(lbm, f64):
    p = lbm.Params(nx=34, ny=18, max_iters=1, reynolds_dim=1, density=0.1, accel=0.005, omega=1.85)
    for flags in (FLAG_ROWS_ANY, FLAG_ROWS_ANY | FLAG_ANY):
        with pytest.raises(lbm.LbmError, match="lbm64_create: the double-precision mode takes"):
            f64.Grid64(p, np.zeros((18, 34), np.int32), device=4096, flags=flags)


def test_create_accepts_the_flag_before_any_hip_call(lbm, f64):
    """With a device ordinal that no machine has, the first HIP call fails: the flag was accepted before it.  The whole grid's flags
    beside it are refused before it."""
    assert f64.FLAG_ROWS_MULTI_ANY_SIZE == FLAG_ROWS_ANY and "FLAG_ROWS_MULTI_ANY_SIZE" in f64.__all__
    p = lbm.Params(nx=34, ny=35, max_iters=1, reynolds_dim=1, density=0.1, accel=0.005, omega=1.85)
    obst = np.zeros((35, 34), np.int32)
    for flags in (FLAG_ROWS_ANY, FLAG_ROWS_ANY | FLAG_ROWS_MULTI, FLAG_ROWS_ANY | FLAG_NT, FLAG_ROWS_ANY | FLAG_NO_NT):
        with pytest.raises(lbm.LbmError, match="hipSetDevice"):
            f64.Rows64(p, obst, 2, devices=[4096, 4096], flags=flags)
    for flags in (FLAG_ROWS_ANY | FLAG_TILE, FLAG_ROWS_ANY | FLAG_MULTI):
        with pytest.raises(lbm.LbmError, match="several steps per exchange are not built"):
            f64.Rows64(p, obst, 2, devices=[4096, 4096], flags=flags)
    with pytest.raises(lbm.LbmError, match="LBM_FLAG_NT_STORES or LBM_FLAG_NO_NT_STORES only"):
        f64.Rows64(p, obst, 2, devices=[4096, 4096], flags=FLAG_ROWS_ANY | FLAG_ANY)


def test_a_c99_caller_sees_the_macro(lbm, tmp_path):
    src = tmp_path / "caller.c"
    src.write_text('''
#include <stdio.h>
#include "lbm_d2q9_f64_rows.h"
int main(void)
{
  lbm64_params p = {34, 35, 10, 10, 0.1, 0.005, 1.85};
  static int obstacles[34 * 35];
  lbm_rows64* run = NULL;
  const unsigned flags = LBM_ROWS64_FLAG_MULTI_ANY_SIZE | LBM64_FLAG_MULTI_ANY_SIZE;
  if (LBM_ROWS64_FLAG_MULTI_ANY_SIZE != 8192u || LBM_ROWS64_FLAG_MULTI_STEPS != 2048u || LBM_ROWS64_ABI_VERSION != 1) return 2;
  if ((LBM_ROWS64_FLAG_MULTI_ANY_SIZE & (LBM_FLAG_NT_STORES | LBM_FLAG_NO_NT_STORES | LBM64_FLAG_TILE_STEPS | LBM64_FLAG_MULTI_STEPS |
                                         LBM64_FLAG_MULTI_ANY_SIZE | LBM_ROWS64_FLAG_MULTI_STEPS)) != 0u) return 3;
  if (lbm_rows64_create(&run, &p, 34 * 35, obstacles, 2, NULL, flags) != 1 || run != NULL) return 4;
  printf("%s\\n", lbm_last_error());
  return lbm_rows64_destroy(NULL);
}
''')
    exe = tmp_path / "caller"
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-L",
                        os.path.dirname(lbm.LIB_PATH), "-llbm_d2q9", f"-Wl,-rpath,{os.path.dirname(lbm.LIB_PATH)}", "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "LBM_FLAG_NT_STORES or LBM_FLAG_NO_NT_STORES only" in r.stdout, (r.returncode, r.stdout, r.stderr)


def test_exports_and_code_object(lbm, f64):
    """No lbm_rows64_* or lbm64_* symbol more, the versions as they were, the four plan entry points, the kernel in the code object."""
    nm = subprocess.run(["nm", "-D", "--defined-only", lbm.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(re.findall(r" T (lbm_rows64_[a-z_0-9]+)", nm)) == set(f64.ROWS_EXPORTS) and len(f64.ROWS_EXPORTS) == 10
    assert set(re.findall(r" T (lbm64_[a-z_0-9]+)", nm)) == set(f64.EXPORTS) and len(f64.EXPORTS) == 15
    assert f64.load_rows_library().lbm_rows64_abi_version() == 1
    assert {"lbm_plan64_rows_multi_any", "lbm_plan64_rows_multi_any_sizeof", "lbm_plan64_rows_multi_any_kernel_name",
            "lbm_plan64_rows_multi_any_run_launches"} <= set(re.findall(r" T (lbm_plan64_[a-z_0-9]+)", nm))
    assert b"lbm_rows_multi_kernel_f64" in open(lbm.LIB_PATH, "rb").read()


def test_cli_switches(lbm, digests, tmp_path):
    from conftest import deck_paths
    ppath, opath = deck_paths("rand_64x48", digests)
    base = {k: v for k, v in os.environ.items() if not k.startswith("LBM")}

    def cli(**env):
        return subprocess.run([lbm.CLI_PATH, ppath, opath], cwd=tmp_path, env={**base, **env}, capture_output=True, text=True, timeout=60)

    for flags in ("8192", "8193", "8194", "10240"):
        r = cli(LBM_PRECISION="double", LBM64_RANKS="1", LBM_DEVICES="4096", LBM_FLAGS=flags)
        assert r.returncode != 0 and "hipSetDevice" in r.stderr and "LBM_FLAGS" not in r.stderr, (flags, r.stderr)
    for flags in ("8195", "8704", "9216", "12288"):
        r = cli(LBM_PRECISION="double", LBM64_RANKS="1", LBM_DEVICES="4096", LBM_FLAGS=flags)
        assert r.returncode != 0 and "LBM_FLAGS: with LBM64_RANKS expected 0, 1" in r.stderr and "8192" in r.stderr, (flags, r.stderr)
    # without LBM64_RANKS the flag goes to lbm64_create, which refuses it
    r = cli(LBM_PRECISION="double", LBM_FLAGS="8192", LBM_DEVICE="4096")
    assert r.returncode != 0 and "lbm64_create: the double-precision mode takes" in r.stderr, r.stderr
