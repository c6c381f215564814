"""Host half of the row-partitioned double-precision runs (include/lbm_d2q9_f64_rows.h; csrc/lbm_plan.cpp plan64_rows, PlanRows64 of
lbm_internal.h): the plan of every rank, the refusals, the header, the exports, what lbm_rows64_create says without a GPU, and the
CLI's switches.  No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK = 256
FLAG_NT, FLAG_NO_NT = 1, 2


class PlanRows64(C.Structure):
    """struct PlanRows64 (lbm_internal.h), field for field."""

    _fields_ = [("flags", C.c_uint), ("nranks", C.c_int), ("rank", C.c_int), ("y0", C.c_int), ("ny_local", C.c_int),
                ("nt_stores", C.c_int), ("lane_cells", C.c_int), ("units", C.c_uint), ("iters", C.c_int), ("blocks", C.c_int),
                ("partials_cap", C.c_int), ("mask_words", C.c_int), ("accel_rank", C.c_int), ("accel_row", C.c_int),
                ("ps", C.c_longlong), ("grid_doubles", C.c_longlong)]


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
    assert lib.lbm_plan64_rows_sizeof() == C.sizeof(PlanRows64)
    return lib


@pytest.fixture(autouse=True)
def _no_knobs(monkeypatch):
    for k in ("LBM_TUNE_MAXBLOCKS", "LBM_TUNE_SKEW"):
        monkeypatch.delenv(k, raising=False)


def _plan(api, f64, nx, ny, nranks, rank, flags=0):
    cp = f64.CParams64(nx, ny, 10, 10, 0.1, 0.005, 1.85)
    plan = PlanRows64()
    rc = api.lbm_plan64_rows(C.byref(cp), nranks, rank, flags, C.byref(plan))
    name = C.create_string_buffer(128)
    if rc == 0:
        assert api.lbm_plan64_rows_kernel_name(C.byref(plan), name, 128) == 0
    return rc, plan, name.value.decode()


ROWS = {(6, 3): [2, 1, 3], (8, 3): [3, 2, 3], (33, 4): [9, 8, 8, 8], (16, 5): None, (48, 8): None, (3, 1): [3]}


@pytest.mark.parametrize("ny,nranks", list(ROWS))
def test_plan_rows_are_the_reference_decomposition(lbm, api, f64, ny, nranks):
    nyl, dis = lbm.decompose(ny, nranks)
    if ROWS[(ny, nranks)] is not None:
        assert nyl == ROWS[(ny, nranks)]
    assert sum(nyl) == ny and dis == [sum(nyl[:r]) for r in range(nranks)]
    for nx in (8, 7):
        for r in range(nranks):
            rc, plan, name = _plan(api, f64, nx, ny, nranks, r)
            assert rc == 0, lbm.load_library().lbm_last_error()
            assert (plan.nranks, plan.rank, plan.y0, plan.ny_local) == (nranks, r, dis[r], nyl[r])
            # row ny-2 lies in the last rank, and is neither its first nor its last row
            assert plan.accel_rank == nranks - 1 and plan.accel_row == ny - 2 - dis[-1] and 0 < plan.accel_row < nyl[-1] - 1
            cells = 2 if nx % 2 == 0 else 1
            assert plan.lane_cells == cells and name == f"lbm_rows_kernel_f64<{cells}>" and plan.nt_stores == 0
            assert plan.units == nx * nyl[r] // cells and plan.iters == 1 and plan.blocks == -(-plan.units // BLOCK)
            assert plan.partials_cap == plan.blocks + 1 and plan.mask_words * 32 >= nx * nyl[r]
            # two ghost rows in every plane, the guards of the shifted loads, 16-byte accesses
            assert plan.ps % 2 == 0 and plan.ps >= nx * (nyl[r] + 2) + 64 and plan.grid_doubles == 9 * plan.ps + 128


def test_plan_blocks_flags_and_the_store_rule(api, f64):
    nyl = [9, 8, 8, 8]
    for r in range(4):
        rc, plan, name = _plan(api, f64, 258, 33, 4, r)
        assert rc == 0 and plan.units == 129 * nyl[r] and plan.blocks == -(-plan.units // BLOCK) and plan.blocks > 1
        assert plan.units % BLOCK != 0                                       # a ragged last block
    assert _plan(api, f64, 258, 33, 4, 0, FLAG_NT)[2] == "lbm_rows_kernel_f64<2,nt>"
    assert _plan(api, f64, 257, 33, 2, 1, FLAG_NT)[2] == "lbm_rows_kernel_f64<1,nt>"
    assert _plan(api, f64, 258, 33, 4, 0, FLAG_NO_NT)[2] == "lbm_rows_kernel_f64<2>"
    # non-temporal stores by default once the RANK's two grids pass 192 MiB: 8192 x 8192 on 8 ranks (1.2 GB a rank), not 1024 x 1024
    assert _plan(api, f64, 8192, 8192, 8, 3)[1].nt_stores == 1 and _plan(api, f64, 8192, 8192, 8, 3, FLAG_NO_NT)[1].nt_stores == 0
    assert _plan(api, f64, 1024, 1024, 8, 3)[1].nt_stores == 0
    # 4096 x 1200 on one rank passes it (708 MB), on 8 ranks (150 rows, 89 MB a rank) it does not
    assert _plan(api, f64, 4096, 1200, 1, 0)[1].nt_stores == 1 and _plan(api, f64, 4096, 1200, 8, 0)[1].nt_stores == 0


def test_plan_with_a_lowered_block_cap(api, f64, monkeypatch):
    monkeypatch.setenv("LBM_TUNE_MAXBLOCKS", "2")
    rc, plan, _ = _plan(api, f64, 258, 33, 4, 0)
    per_block = BLOCK * plan.iters * plan.lane_cells
    assert rc == 0 and plan.iters > 1 and plan.blocks == -(-(258 * 9) // per_block) and plan.partials_cap == plan.blocks + 1


REFUSALS = [
    (dict(ny=5, nranks=3), "the last rank fewer than 3 rows"),            # 2, 1, 2
    (dict(ny=3, nranks=3), "without a row"),                              # 1, 0, 2
    (dict(nranks=0), r"nranks must be 1\.\.64"),
    (dict(nranks=65), r"nranks must be 1\.\.64"),
    (dict(flags=512), "several steps per exchange are not built"),       # LBM64_FLAG_TILE_STEPS
    (dict(flags=1024), "several steps per exchange are not built"),      # LBM64_FLAG_MULTI_STEPS
    (dict(flags=1 | 1024), "several steps per exchange are not built"),
    (dict(flags=256), "LBM_FLAG_NT_STORES or LBM_FLAG_NO_NT_STORES only"),   # LBM_FLAG_FUSED_ARITH
    (dict(flags=8), "LBM_FLAG_NT_STORES or LBM_FLAG_NO_NT_STORES only"),
    (dict(nx=0), "nx must be positive"),
    (dict(ny=2, nranks=1), "ny must be >= 3"),
    (dict(nx=65536, ny=32768), "grid too large for 32-bit cell indices"),
]


@pytest.mark.parametrize("case,text", REFUSALS)
def test_plan_refusals(lbm, api, f64, case, text):
    args = dict(nx=8, ny=16, nranks=2, flags=0)
    args.update(case)
    rc, _, _ = _plan(api, f64, args["nx"], args["ny"], args["nranks"], 0, args["flags"])
    message = lbm.load_library().lbm_last_error().decode()
    assert rc == 1 and re.search(text, message), message


@pytest.mark.parametrize("case,text", [c for c in REFUSALS if c[0].get("nx", 8) < 65536])      # (not the 2^31-cell map)
def test_create_refuses_the_same_before_any_hip_call(lbm, f64, case, text):
    """The arguments are checked before the devices: a device ordinal that no machine has would be reported otherwise."""
    args = dict(nx=8, ny=16, nranks=2, flags=0)
    args.update(case)
    p = lbm.Params(nx=args["nx"], ny=args["ny"], max_iters=1, reynolds_dim=1, density=0.1, accel=0.005, omega=1.85)
    with pytest.raises(lbm.LbmError, match=text):
        f64.Rows64(p, np.zeros((p.ny, p.nx), np.int32), args["nranks"], devices=[4096] * max(args["nranks"], 0), flags=args["flags"])


def test_create_without_a_gpu_fails_with_a_message(lbm, f64):
    """On a machine with no GPU lbm_rows64_create reports the HIP error instead of crashing (with one, the device ordinal is out of range)."""
    p = lbm.Params(nx=8, ny=4, max_iters=1, reynolds_dim=1, density=0.1, accel=0.005, omega=1.85)
    with pytest.raises(lbm.LbmError) as e:
        f64.Rows64(p, np.zeros((4, 8), np.int32), 1, devices=[4096])
    assert "hipSetDevice" in str(e.value)
    with pytest.raises(lbm.LbmError, match="free_cells must be positive"):
        f64.Rows64(p, np.ones((4, 8), np.int32), 1, devices=[4096])
    with pytest.raises(ValueError, match="one device per rank"):
        f64.Rows64(p, np.zeros((4, 8), np.int32), 2, devices=[0])


def test_header_is_c99_and_a_c_caller_links(lbm, tmp_path):
    src = tmp_path / "caller.c"
    src.write_text('''
#include <stdio.h>
#include "lbm_d2q9_f64_rows.h"
int main(void)
{
  lbm64_params p = {8, 5, 10, 10, 0.1, 0.005, 1.85};
  int obstacles[40] = {0};
  lbm_rows64* run = NULL;
  if (lbm_rows64_abi_version() != LBM_ROWS64_ABI_VERSION || LBM_ROWS64_ABI_VERSION != 1 || LBM_ROWS64_MAX_RANKS != 64) return 2;
  if (lbm64_abi_version() != 1 || LBM_ABI_VERSION != 5) return 3;
  if (lbm_rows64_create(&run, &p, 40, obstacles, 3, NULL, 0) != 1 || run != NULL) return 4;      /* 5 rows on 3 ranks: 2, 1, 2 */
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
    assert r.returncode == 0 and "the last rank fewer than 3 rows" in r.stdout, (r.returncode, r.stdout, r.stderr)


def test_library_exports_every_declared_rows_symbol(lbm, f64):
    header = open(os.path.join(ROOT, "include", "lbm_d2q9_f64_rows.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(lbm_rows64_[a-z_0-9]+)\s*\(", header))
    assert len(declared) == 10
    nm = subprocess.run(["nm", "-D", "--defined-only", lbm.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (lbm_rows64_[a-z_0-9]+)", nm))
    assert declared == exported, declared ^ exported
    assert declared == set(f64.ROWS_EXPORTS)
    assert f64.load_rows_library().lbm_rows64_abi_version() == 1 == f64.ROWS_ABI_VERSION
    # the ABIs beside it are as they were
    assert f64.load_library().lbm64_abi_version() == 1 == f64.ABI_VERSION and len(f64.EXPORTS) == 15
    assert not set(f64.EXPORTS) & set(f64.ROWS_EXPORTS)
    assert lbm.load_library().lbm_abi_version() == 5
    blob = open(lbm.LIB_PATH, "rb").read()
    assert b"lbm_rows_kernel_f64" in blob and b"lbm64_push_rows_kernel" in blob


def test_cli_switches(lbm, digests, tmp_path):
    from conftest import deck_paths
    ppath, opath = deck_paths("tiny_8x3", digests)
    base = {k: v for k, v in os.environ.items() if not k.startswith("LBM")}

    def cli(**env):
        return subprocess.run([lbm.CLI_PATH, ppath, opath], cwd=tmp_path, env={**base, **env}, capture_output=True, text=True, timeout=60)

    r = cli(LBM64_RANKS="2")
    assert r.returncode != 0 and "LBM64_RANKS: row blocks in double precision need LBM_PRECISION=double" in r.stderr
    r = cli(LBM64_RANKS="2", LBM_PRECISION="float")
    assert r.returncode != 0 and "need LBM_PRECISION=double" in r.stderr
    r = cli(LBM_PRECISION="double", LBM_GPUS="2")
    assert r.returncode != 0 and "double precision runs on one GPU" in r.stderr
    r = cli(LBM_PRECISION="double", LBM_GPUS="2", LBM64_RANKS="2")
    assert r.returncode != 0 and "double precision runs on one GPU" in r.stderr
    for bad in ("0", "65", "-1", "x"):
        r = cli(LBM_PRECISION="double", LBM64_RANKS=bad)
        assert r.returncode != 0 and "LBM64_RANKS: expected 1 to 64 ranks" in r.stderr, bad
    for flags in ("3", "512", "1024", "256"):
        r = cli(LBM_PRECISION="double", LBM64_RANKS="1", LBM_FLAGS=flags)
        assert r.returncode != 0 and "LBM_FLAGS: with LBM64_RANKS expected 0, 1" in r.stderr, flags
    # 3 rows on 2 ranks: 1, 2 — refused by the plan, before any device is touched
    r = cli(LBM_PRECISION="double", LBM64_RANKS="2", LBM_DEVICES="4096,4096")
    assert r.returncode != 0 and "the last rank fewer than 3 rows" in r.stderr
    r = cli(LBM_PRECISION="double", LBM64_RANKS="1", LBM_DEVICES="4096")
    assert r.returncode != 0 and "hipSetDevice" in r.stderr
