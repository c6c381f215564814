"""Column-partitioned double-precision runs, what can be checked without a GPU (include/lbm_d2q9_f64_cols.h, csrc/lbm_cols64.hip): the
declared names against the library's exports and the binding's table, the header from a C99 caller, the refusals of lbm_cols64_create
before its first HIP call, the CLI's refusals, the kernels in the code object."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lbm_d2q9_f64_cols.h")
NO_DEVICE = 4096          # an ordinal no machine has: the first HIP call of a create that got that far fails


@pytest.fixture(scope="module")
def f64(lbm):
    from mpilattice_boltzmann_amd import f64 as mod
    mod.load_cols_library()
    return mod


def test_declared_names_are_the_exports_and_the_binding(lbm, f64):
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(lbm_cols64_[a-z_0-9]+)\s*\(", header))
    assert declared == {"lbm_cols64_" + n for n in ("abi_version", "create", "destroy", "run", "get_cells", "set_cells", "get_observables",
                                                    "av_velocity_sum", "last_run_ms", "describe", "digest")}
    nm = subprocess.run(["nm", "-D", "--defined-only", lbm.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(re.findall(r" T (lbm_cols64_[a-z_0-9]+)", nm)) == declared == set(f64.COLS_EXPORTS)
    assert {"lbm_plan64_cols", "lbm_plan64_cols_sizeof", "lbm_plan64_cols_kernel_name", "lbm_plan64_cols_run_launches"} <= set(re.findall(r" T (lbm_plan64_[a-z_0-9]+)", nm))
    # the names that were there stay what they were
    assert set(re.findall(r" T (lbm64_[a-z_0-9]+)", nm)) == set(f64.EXPORTS) and len(f64.EXPORTS) == 15
    assert set(re.findall(r" T (lbm_rows64_[a-z_0-9]+)", nm)) == set(f64.ROWS_EXPORTS) and len(f64.ROWS_EXPORTS) == 10
    assert set(re.findall(r" T (lbm_digest64_[a-z_0-9]+)", nm)) == set(f64.DIGEST_EXPORTS) and len(f64.DIGEST_EXPORTS) == 4
    lib = f64.load_cols_library()
    assert lib.lbm_cols64_abi_version() == 1 == f64.COLS_ABI_VERSION
    assert lib.lbm_abi_version() == 5 and lib.lbm64_abi_version() == 1 and f64.load_digest_library().lbm_digest64_abi_version() == 1
    assert f64.load_rows_library().lbm_rows64_abi_version() == 1
    for name in ("Cols64", "COLS_EXPORTS", "COLS_ABI_VERSION", "load_cols_library"):
        assert name in f64.__all__


def test_the_kernels_are_in_the_code_object(lbm):
    blob = open(lbm.LIB_PATH, "rb").read()
    assert b"lbm_cols_multi_kernel_f64" in blob and b"lbm64_push_ghost_cols_kernel" in blob


def test_the_header_compiles_as_c99_and_a_c_caller_is_refused_with_the_message(lbm, tmp_path):
    src = tmp_path / "caller.c"
    src.write_text('''
#include <stdio.h>
#include "lbm_d2q9_f64_cols.h"
int main(void)
{
  lbm64_params p = {62, 16, 10, 10, 0.1, 0.005, 1.85};
  static int obstacles[62 * 16];
  lbm_cols64* run = NULL;
  unsigned long long d = 0;
  if (LBM_COLS64_ABI_VERSION != 1 || LBM_COLS64_MAX_RANKS != 64 || lbm_cols64_abi_version() != LBM_COLS64_ABI_VERSION) return 2;
  if (lbm_cols64_create(&run, &p, 62 * 16, obstacles, 2, NULL, 0u) != 1 || run != NULL) return 3;
  printf("%s\\n", lbm_last_error());
  if (lbm_cols64_run(NULL, 1, NULL) != 1 || lbm_cols64_digest(NULL, 0, 0, NULL, &d) != 1) return 4;
  return lbm_cols64_destroy(NULL);
}
''')
    exe = tmp_path / "caller"
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-L",
                        os.path.dirname(lbm.LIB_PATH), "-llbm_d2q9", f"-Wl,-rpath,{os.path.dirname(lbm.LIB_PATH)}", "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "leaves rank 1 30 columns" in r.stdout and "row partition" in r.stdout, (r.returncode, r.stdout, r.stderr)


def _params(lbm, nx, ny):
    return lbm.Params(nx=nx, ny=ny, max_iters=1, reynolds_dim=1, density=0.1, accel=0.005, omega=1.85)


def test_create_refuses_before_any_hip_call(lbm, f64, digests):
    """With a device ordinal that no machine has, the first HIP call of an accepted run fails (hipSetDevice); every refusal below comes
    with its own message instead: it was made before that call."""
    from conftest import deck_paths
    dev = lambda n: [NO_DEVICE] * n
    for flags in (0, f64.FLAG_NT_STORES, f64.FLAG_NO_NT_STORES):
        with pytest.raises(lbm.LbmError, match="hipSetDevice"):
            f64.Cols64(_params(lbm, 70, 18), np.zeros((18, 70), np.int32), 2, devices=dev(2), flags=flags)
    for nx, ny, nranks, text in ((63, 16, 1, "nx must be even"), (62, 16, 2, "leaves rank 1 30 columns"), (64, 15, 2, "ny = 15 is fewer than 16 rows")):
        with pytest.raises(lbm.LbmError, match=text) as e:
            f64.Cols64(_params(lbm, nx, ny), np.zeros((ny, nx), np.int32), nranks, devices=dev(nranks))
        assert "row partition" in str(e.value)
    ppath, opath = deck_paths("column_24x20", digests)
    p = f64.read_params64(ppath)
    obst, _ = lbm.read_obstacles(opath, p.nx, p.ny)
    with pytest.raises(lbm.LbmError, match="leaves rank 0 24 columns"):
        f64.Cols64(p, obst, 1, devices=dev(1))
    with pytest.raises(lbm.LbmError, match="nranks must be 1..64"):
        f64.Cols64(_params(lbm, 65 * 32, 16), np.zeros((16, 65 * 32), np.int32), 65, devices=dev(65))
    for flags in (512, 1024, 2048, 4096, 8192, 256):
        with pytest.raises(lbm.LbmError, match="LBM_FLAG_NT_STORES or LBM_FLAG_NO_NT_STORES only"):
            f64.Cols64(_params(lbm, 64, 16), np.zeros((16, 64), np.int32), 2, devices=dev(2), flags=flags)
    with pytest.raises(lbm.LbmError, match="free_cells must be positive"):
        f64.Cols64(_params(lbm, 64, 16), np.ones((16, 64), np.int32), 2, devices=dev(2))


def test_cli_refusals(lbm, digests, tmp_path):
    from conftest import deck_paths
    ppath, opath = deck_paths("rand_64x48", digests)
    base = {k: v for k, v in os.environ.items() if not k.startswith("LBM")}

    def cli(**env):
        return subprocess.run([lbm.CLI_PATH, ppath, opath], cwd=tmp_path, env={**base, **env}, capture_output=True, text=True, timeout=60)

    r = cli(LBM64_COLS="2")
    assert r.returncode != 0 and "LBM64_COLS: column blocks in double precision need LBM_PRECISION=double" in r.stderr
    r = cli(LBM_PRECISION="double", LBM64_COLS="2", LBM64_RANKS="2")
    assert r.returncode != 0 and "LBM64_COLS: column blocks and row blocks (LBM64_RANKS) exclude each other" in r.stderr
    r = cli(LBM_PRECISION="double", LBM64_COLS="2", LBM_GPUS="2")
    assert r.returncode != 0 and "LBM64_COLS: the column blocks of one process take their devices from LBM_DEVICES" in r.stderr
    for n in ("0", "65", "-1"):
        r = cli(LBM_PRECISION="double", LBM64_COLS=n)
        assert r.returncode != 0 and "LBM64_COLS: expected 1 to 64 column blocks" in r.stderr, (n, r.stderr)
    for flags in ("3", "512", "2048", "8192", "-1"):
        r = cli(LBM_PRECISION="double", LBM64_COLS="2", LBM_DEVICES="4096,4096", LBM_FLAGS=flags)
        assert r.returncode != 0 and "LBM_FLAGS: with LBM64_COLS expected 0, 1" in r.stderr, (flags, r.stderr)
    # accepted as far as the first HIP call: flags 0, 1, 2 on two blocks of 32 columns
    for flags in ("0", "1", "2"):
        r = cli(LBM_PRECISION="double", LBM64_COLS="2", LBM_DEVICES="4096,4096", LBM_FLAGS=flags)
        assert r.returncode != 0 and "hipSetDevice" in r.stderr, (flags, r.stderr)
    # three blocks of a 64-wide deck: 22, 22, 20 columns — the library's refusal, with the alternative
    r = cli(LBM_PRECISION="double", LBM64_COLS="3", LBM_DEVICES="4096,4096,4096")
    assert r.returncode != 0 and "leaves rank 0 22 columns" in r.stderr and "row partition" in r.stderr
    assert not (tmp_path / "final_state.dat").exists()
