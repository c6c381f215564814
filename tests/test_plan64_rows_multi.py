"""The plan of a row-partitioned double-precision run under LBM_ROWS64_FLAG_MULTI_STEPS (csrc/lbm_plan.cpp plan64_rows_multi,
PlanRowsMulti64 of lbm_internal.h) through the lbm_plan64_rows_multi* entry points, without a GPU: which runs
lbm_rows_multi_kernel_f64 takes, with how many steps per launch and on what storage; the fallbacks, in which lbm_plan64_rows returns
what it returns without the flag; the refusals; the header's macro from C99; the CLI's switches."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from test_f64_rows_host import PlanRows64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAG_NT, FLAG_NO_NT, FLAG_TILE, FLAG_MULTI, FLAG_ROWS_MULTI = 1, 2, 512, 1024, 2048
TX, TY, LANES = 32, 16, 512
BUILT_K, DEFAULT_K = (2, 3, 4), 4
DEFAULT_MIN = 1 << 17            # LBM_TUNE_MULTI64_MIN's default for ranks, cells of the smallest rank: measured (test_threshold_without_the_knob)


class PlanRowsMulti64(C.Structure):
    """struct PlanRowsMulti64 (lbm_internal.h), field for field."""

    _fields_ = [("multi_kernel", C.c_int), ("K", C.c_int), ("ghost", C.c_int), ("tiles_x", C.c_int), ("n_tiles", C.c_int),
                ("block", C.c_int), ("lds_bytes", C.c_int), ("nt_stores", C.c_int), ("mask_words", C.c_int), ("partials_cap", C.c_int),
                ("ps", C.c_longlong), ("grid_doubles", C.c_longlong)]


def multi64_lds_bytes(K):
    """lbm_geometry.h: the frame of (TX + 2 multi_ex(K-1)) x (TY + 2 (K-1)) cells of nine doubles and a flag byte, and 4 x 8 doubles."""
    return (TX + 4 * (K // 2)) * (TY + 2 * (K - 1)) * (9 * 8 + 1) + 8 * 4 * (LANES // 64)


@pytest.fixture(scope="module")
def f64(lbm):
    from mpilattice_boltzmann_amd import f64 as mod
    mod.load_rows_library()
    return mod


@pytest.fixture(scope="module")
def api(lbm, f64):
    lib = lbm.load_library()
    lib.lbm_plan64_rows_sizeof.restype, lib.lbm_plan64_rows_sizeof.argtypes = C.c_int, []
    lib.lbm_plan64_rows.restype = C.c_int
    lib.lbm_plan64_rows.argtypes = [C.POINTER(f64.CParams64), C.c_int, C.c_int, C.c_uint, C.POINTER(PlanRows64)]
    lib.lbm_plan64_rows_kernel_name.restype, lib.lbm_plan64_rows_kernel_name.argtypes = C.c_int, [C.POINTER(PlanRows64), C.c_char_p, C.c_size_t]
    lib.lbm_plan64_rows_multi_sizeof.restype, lib.lbm_plan64_rows_multi_sizeof.argtypes = C.c_int, []
    lib.lbm_plan64_rows_multi.restype = C.c_int
    lib.lbm_plan64_rows_multi.argtypes = [C.POINTER(f64.CParams64), C.c_int, C.c_int, C.c_uint, C.POINTER(PlanRowsMulti64)]
    lib.lbm_plan64_rows_multi_kernel_name.restype = C.c_int
    lib.lbm_plan64_rows_multi_kernel_name.argtypes = [C.POINTER(PlanRowsMulti64), C.c_char_p, C.c_size_t]
    lib.lbm_plan64_rows_multi_run_launches.restype = C.c_int
    lib.lbm_plan64_rows_multi_run_launches.argtypes = [C.POINTER(PlanRowsMulti64), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int]
    assert lib.lbm_plan64_rows_multi_sizeof() == C.sizeof(PlanRowsMulti64)
    assert lib.lbm_plan64_rows_sizeof() == C.sizeof(PlanRows64)              # and PlanRows64 is what tests/test_f64_rows_host.py mirrors
    return lib


@pytest.fixture(autouse=True)
def _no_knobs(monkeypatch):
    for k in ("LBM_TUNE_MAXBLOCKS", "LBM_TUNE_SKEW", "LBM_TUNE_MULTI64_K", "LBM_TUNE_MULTI64_MIN"):
        monkeypatch.delenv(k, raising=False)


def _rows(api, f64, nx, ny, nranks, rank, flags):
    cp = f64.CParams64(nx, ny, 10, 10, 0.1, 0.005, 1.85)
    plan = PlanRows64()
    rc = api.lbm_plan64_rows(C.byref(cp), nranks, rank, flags, C.byref(plan))
    name = C.create_string_buffer(128)
    if rc == 0:
        assert api.lbm_plan64_rows_kernel_name(C.byref(plan), name, 128) == 0
    return rc, plan, name.value.decode()


def _multi(api, f64, nx, ny, nranks, rank, flags=FLAG_ROWS_MULTI):
    cp = f64.CParams64(nx, ny, 10, 10, 0.1, 0.005, 1.85)
    plan = PlanRowsMulti64()
    rc = api.lbm_plan64_rows_multi(C.byref(cp), nranks, rank, flags, C.byref(plan))
    name = C.create_string_buffer(128)
    if rc == 0:
        assert api.lbm_plan64_rows_multi_kernel_name(C.byref(plan), name, 128) == 0
    return rc, plan, name.value.decode()


ELIGIBLE = [(32, 16, 1), (32, 32, 2), (64, 48, 3), (1024, 1024, 8), (8192, 8192, 8)]


@pytest.mark.parametrize("K", [None, 2, 3])
@pytest.mark.parametrize("nx,ny,nranks", ELIGIBLE)
def test_eligible_plans(lbm, api, f64, monkeypatch, nx, ny, nranks, K):
    monkeypatch.setenv("LBM_TUNE_MULTI64_MIN", "0")
    if K is not None:
        monkeypatch.setenv("LBM_TUNE_MULTI64_K", str(K))
    K = DEFAULT_K if K is None else K
    nyls, dis = lbm.decompose(ny, nranks)
    assert all(n % TY == 0 for n in nyls)
    for r in range(nranks):
        nyl = nyls[r]
        rc, m, name = _multi(api, f64, nx, ny, nranks, r)
        assert rc == 0, lbm.load_library().lbm_last_error()
        storage = nx * (nyl + 2 * K)
        nt = 2 * 9 * 8 * storage > 192 << 20                              # plan64_whole's rule on the rank's two grids
        assert (m.multi_kernel, m.K, m.ghost) == (1, K, K)
        assert (m.tiles_x, m.n_tiles) == (nx // TX, (nx // TX) * (nyl // TY))
        assert m.block == LANES and m.lds_bytes == multi64_lds_bytes(K) and m.lds_bytes <= 65536
        assert m.nt_stores == int(nt) and name == (f"lbm_rows_multi_kernel_f64<{K},nt>" if nt else f"lbm_rows_multi_kernel_f64<{K}>")
        assert m.ps % 2 == 0 and m.ps >= storage + 64 and m.grid_doubles == 9 * m.ps + 128
        assert m.mask_words * 32 >= storage                                   # the window covers every storage row
        assert m.partials_cap == K * m.n_tiles + 1
        assert _multi(api, f64, nx, ny, nranks, r, FLAG_ROWS_MULTI | FLAG_NT)[2] == f"lbm_rows_multi_kernel_f64<{K},nt>"
        assert _multi(api, f64, nx, ny, nranks, r, FLAG_ROWS_MULTI | FLAG_NO_NT)[2] == f"lbm_rows_multi_kernel_f64<{K}>"
        # PlanRows64 is the one-step plan whatever the flag says
        _, off, name_off = _rows(api, f64, nx, ny, nranks, r, 0)
        _, on, name_on = _rows(api, f64, nx, ny, nranks, r, FLAG_ROWS_MULTI)
        assert on.flags == FLAG_ROWS_MULTI and name_on == name_off
        assert [getattr(on, f) for f, _ in PlanRows64._fields_ if f != "flags"] == [getattr(off, f) for f, _ in PlanRows64._fields_ if f != "flags"]
        # nothing without the flag
        for flags in (0, FLAG_NT, FLAG_NO_NT):
            rc, m, name = _multi(api, f64, nx, ny, nranks, r, flags)
            assert rc == 0 and m.multi_kernel == 0 and name == ""


@pytest.mark.parametrize("value", ["0", "1", "5", "abc"])
def test_malformed_steps_per_launch_get_the_default(api, f64, monkeypatch, value):
    monkeypatch.setenv("LBM_TUNE_MULTI64_MIN", "0")
    monkeypatch.setenv("LBM_TUNE_MULTI64_K", value)
    rc, m, name = _multi(api, f64, 64, 48, 3, 1)
    assert rc == 0 and (m.multi_kernel, m.K, m.ghost) == (1, DEFAULT_K, DEFAULT_K) and name == f"lbm_rows_multi_kernel_f64<{DEFAULT_K}>"


# nx not a multiple of 32 (twice); 24 rows a rank; uneven ranks (17, 16)
FALLBACKS = [(8, 16, 2), (30, 32, 2), (32, 48, 2), (32, 33, 2)]


@pytest.mark.parametrize("nx,ny,nranks", FALLBACKS)
def test_fallbacks(api, f64, monkeypatch, nx, ny, nranks):
    monkeypatch.setenv("LBM_TUNE_MULTI64_MIN", "0")
    fields = [f for f, _ in PlanRows64._fields_ if f != "flags"]
    for r in range(nranks):
        rc, m, name = _multi(api, f64, nx, ny, nranks, r)
        assert rc == 0 and m.multi_kernel == 0 and m.n_tiles == 0 and name == ""
        for base in (0, FLAG_NT, FLAG_NO_NT):
            rc_off, off, name_off = _rows(api, f64, nx, ny, nranks, r, base)
            rc_on, on, name_on = _rows(api, f64, nx, ny, nranks, r, base | FLAG_ROWS_MULTI)
            assert rc_off == rc_on == 0 and on.flags == base | FLAG_ROWS_MULTI and off.flags == base
            assert name_on == name_off and name_on.startswith("lbm_rows_kernel_f64<")
            assert [getattr(on, f) for f in fields] == [getattr(off, f) for f in fields]


def test_the_minimum_size_is_the_smallest_rank_s(api, f64, monkeypatch):
    monkeypatch.setenv("LBM_TUNE_MULTI64_MIN", str(64 * 16))
    assert _multi(api, f64, 64, 48, 3, 0)[1].multi_kernel == 1                # 64 x 16 a rank
    monkeypatch.setenv("LBM_TUNE_MULTI64_MIN", str(64 * 16 + 1))
    assert [_multi(api, f64, 64, 48, 3, r)[1].multi_kernel for r in range(3)] == [0, 0, 0]
    assert _multi(api, f64, 64, 48, 1, 0)[1].multi_kernel == 1                # one rank of 64 x 48


def test_threshold_without_the_knob(api, f64):
    """The issue's assertion was "1024 x 1024 on 8 ranks (2^17 cells a rank) falls back under the existing default of 2^20, 8192 x 8192
    on 8 ranks does not; if the measurement moves the default, this assertion moves with it".  The measurement moved it
    (profiles/r18/f64_rows_multi.txt, us per step unflagged | flagged, all ranks on one MI355X): 1024 x 1024 on 8 ranks 96.90 | 31.14, a
    gain of 65.76 us against the two max - min spreads together of 3.88 us; that is the smallest rank size measured, so by
    plan64_multi's rule the default for ranks is 2^17 cells of the smallest rank.  Now: 1024 x 1024 on 8 ranks runs the kernel, one tile
    row of it less a rank does not, 8192 x 8192 on 8 ranks does; and the whole grid's default stays 2^20 cells."""
    assert 1024 * 1024 // 8 == DEFAULT_MIN
    for r in (0, 7):
        rc, m, name = _multi(api, f64, 1024, 1024, 8, r)
        assert rc == 0 and m.multi_kernel == 1 and m.K == DEFAULT_K and name == f"lbm_rows_multi_kernel_f64<{DEFAULT_K}>"
        rc, m, name = _multi(api, f64, 1024, 1024 - 8 * TY, 8, r)              # 112 rows a rank
        assert rc == 0 and m.multi_kernel == 0 and m.n_tiles > 0 and name == ""
        rc, m, name = _multi(api, f64, 8192, 8192, 8, r)
        assert rc == 0 and m.multi_kernel == 1 and m.K == DEFAULT_K and name == f"lbm_rows_multi_kernel_f64<{DEFAULT_K},nt>"
    assert _multi(api, f64, 1024, 512, 8, 0)[1].multi_kernel == 0              # 2^16 cells a rank
    # lbm64_create's default is what it was: a whole 1024 x 1008 grid runs the one-step kernel with LBM64_FLAG_MULTI_STEPS
    lib = api
    from test_plan64_multi import PlanMulti64
    lib.lbm_plan64_multi.restype, lib.lbm_plan64_multi.argtypes = C.c_int, [C.POINTER(f64.CParams64), C.c_uint, C.POINTER(PlanMulti64)]
    whole = PlanMulti64()
    assert lib.lbm_plan64_multi(C.byref(f64.CParams64(1024, 1024, 10, 10, 0.1, 0.005, 1.85)), FLAG_MULTI, C.byref(whole)) == 0 and whole.multi_kernel == 1
    assert lib.lbm_plan64_multi(C.byref(f64.CParams64(1024, 1008, 10, 10, 0.1, 0.005, 1.85)), FLAG_MULTI, C.byref(whole)) == 0 and whole.multi_kernel == 0


@pytest.mark.parametrize("K", BUILT_K)
def test_run_launches(api, f64, monkeypatch, K):
    monkeypatch.setenv("LBM_TUNE_MULTI64_MIN", "0")
    monkeypatch.setenv("LBM_TUNE_MULTI64_K", str(K))
    _, plan, _ = _multi(api, f64, 64, 48, 3, 0)
    for n in range(0, 3 * K + 2):
        cap = n + 1
        steps, full = (C.c_int * cap)(), (C.c_int * cap)()
        count = api.lbm_plan64_rows_multi_run_launches(C.byref(plan), n, steps, full, cap)
        steps, full = list(steps[:count]), list(full[:count])
        assert count == -(-n // K) and sum(steps) == n and full == [int(k == K) for k in steps] and all(full[:-1])
    assert api.lbm_plan64_rows_multi_run_launches(C.byref(plan), -1, None, None, 0) == -1


def test_refusals(lbm, api, f64):
    lib = lbm.load_library()
    for flags in (FLAG_ROWS_MULTI | FLAG_TILE, FLAG_ROWS_MULTI | FLAG_MULTI, FLAG_ROWS_MULTI | FLAG_NT | FLAG_MULTI):
        for fn in (_rows, _multi):
            assert fn(api, f64, 32, 32, 2, 0, flags)[0] == 1
            assert "several steps per exchange are not built" in lib.lbm_last_error().decode()
    for flags in (FLAG_ROWS_MULTI | 256, FLAG_ROWS_MULTI | 8, 4096):
        assert _rows(api, f64, 32, 32, 2, 0, flags)[0] == 1
        assert "LBM_FLAG_NT_STORES or LBM_FLAG_NO_NT_STORES only" in lib.lbm_last_error().decode()
    for flags in (FLAG_ROWS_MULTI, FLAG_ROWS_MULTI | FLAG_NT, FLAG_ROWS_MULTI | FLAG_NO_NT):
        assert _rows(api, f64, 32, 32, 2, 0, flags)[0] == 0
    assert api.lbm_plan64_rows_multi(C.byref(f64.CParams64(32, 32, 10, 10, 0.1, 0.005, 1.85)), 2, 0, FLAG_ROWS_MULTI, None) == 1
    # the arguments plan64_rows refuses, with the flag as without it
    for nx, ny, nranks in ((0, 16, 2), (8, 2, 1), (8, 5, 3), (8, 3, 3), (8, 16, 0), (8, 16, 65)):
        assert _multi(api, f64, nx, ny, nranks, 0)[0] == 1


def test_whole_grids_keep_refusing_the_flag(lbm, f64):
    p = lbm.Params(nx=32, ny=16, max_iters=1, reynolds_dim=1, density=0.1, accel=0.005, omega=1.85)
    for flags in (FLAG_ROWS_MULTI, FLAG_ROWS_MULTI | FLAG_MULTI):
        with pytest.raises(lbm.LbmError, match="lbm64_create: the double-precision mode takes"):
            f64.Grid64(p, np.zeros((16, 32), np.int32), device=4096, flags=flags)


def test_create_accepts_the_flag_before_any_hip_call(lbm, f64):
    """With a device ordinal that no machine has, the first HIP call fails: the flag was accepted before it.  512 and 1024 beside it
    are refused before it."""
    assert f64.FLAG_ROWS_MULTI_STEPS == FLAG_ROWS_MULTI
    p = lbm.Params(nx=32, ny=32, max_iters=1, reynolds_dim=1, density=0.1, accel=0.005, omega=1.85)
    obst = np.zeros((32, 32), np.int32)
    for flags in (FLAG_ROWS_MULTI, FLAG_ROWS_MULTI | FLAG_NT, FLAG_ROWS_MULTI | FLAG_NO_NT):
        with pytest.raises(lbm.LbmError, match="hipSetDevice"):
            f64.Rows64(p, obst, 2, devices=[4096, 4096], flags=flags)
    for flags in (FLAG_ROWS_MULTI | FLAG_TILE, FLAG_ROWS_MULTI | FLAG_MULTI):
        with pytest.raises(lbm.LbmError, match="several steps per exchange are not built"):
            f64.Rows64(p, obst, 2, devices=[4096, 4096], flags=flags)


def test_a_c99_caller_sees_the_macro(lbm, tmp_path):
    src = tmp_path / "caller.c"
    src.write_text('''
#include <stdio.h>
#include "lbm_d2q9_f64_rows.h"
int main(void)
{
  lbm64_params p = {32, 32, 10, 10, 0.1, 0.005, 1.85};
  static int obstacles[32 * 32];
  lbm_rows64* run = NULL;
  const unsigned flags = LBM_ROWS64_FLAG_MULTI_STEPS | LBM64_FLAG_MULTI_STEPS;
  if (LBM_ROWS64_FLAG_MULTI_STEPS != 2048u || LBM_ROWS64_ABI_VERSION != 1) return 2;
  if ((LBM_ROWS64_FLAG_MULTI_STEPS & (LBM_FLAG_NT_STORES | LBM_FLAG_NO_NT_STORES | LBM64_FLAG_TILE_STEPS | LBM64_FLAG_MULTI_STEPS)) != 0u) return 3;
  if (lbm_rows64_create(&run, &p, 1024, obstacles, 2, NULL, flags) != 1 || run != NULL) return 4;
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
    assert r.returncode == 0 and "several steps per exchange are not built" in r.stdout, (r.returncode, r.stdout, r.stderr)


def test_exports_and_code_object(lbm, f64):
    """No lbm_rows64_* symbol more, the version as it was, the new kernels in the code object."""
    nm = subprocess.run(["nm", "-D", "--defined-only", lbm.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(re.findall(r" T (lbm_rows64_[a-z_0-9]+)", nm)) == set(f64.ROWS_EXPORTS) and len(f64.ROWS_EXPORTS) == 10
    assert f64.load_rows_library().lbm_rows64_abi_version() == 1
    assert {"lbm_plan64_rows_multi", "lbm_plan64_rows_multi_sizeof", "lbm_plan64_rows_multi_kernel_name",
            "lbm_plan64_rows_multi_run_launches"} <= set(re.findall(r" T (lbm_plan64_[a-z_0-9]+)", nm))
    blob = open(lbm.LIB_PATH, "rb").read()
    assert b"lbm_rows_multi_kernel_f64" in blob and b"lbm64_push_ghost_rows_kernel" in blob


def test_cli_switches(lbm, digests, tmp_path):
    from conftest import deck_paths
    ppath, opath = deck_paths("rand_64x48", digests)
    base = {k: v for k, v in os.environ.items() if not k.startswith("LBM")}

    def cli(**env):
        return subprocess.run([lbm.CLI_PATH, ppath, opath], cwd=tmp_path, env={**base, **env}, capture_output=True, text=True, timeout=60)

    for flags in ("2048", "2049", "2050"):
        r = cli(LBM_PRECISION="double", LBM64_RANKS="1", LBM_DEVICES="4096", LBM_FLAGS=flags)
        assert r.returncode != 0 and "hipSetDevice" in r.stderr and "LBM_FLAGS" not in r.stderr, (flags, r.stderr)
    for flags in ("2051", "2560", "3072", "4096"):
        r = cli(LBM_PRECISION="double", LBM64_RANKS="1", LBM_DEVICES="4096", LBM_FLAGS=flags)
        assert r.returncode != 0 and "LBM_FLAGS: with LBM64_RANKS expected 0, 1" in r.stderr, (flags, r.stderr)
    # without LBM64_RANKS the flag goes to lbm64_create, which refuses it
    r = cli(LBM_PRECISION="double", LBM_FLAGS="2048", LBM_DEVICE="4096")
    assert r.returncode != 0 and "lbm64_create: the double-precision mode takes" in r.stderr, r.stderr
