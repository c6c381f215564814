"""Host half of the double-precision mode (include/lbm_d2q9_f64.h; lbm_host.cpp): parser, writers, header, exports, and what
lbm64_create says on a machine without a GPU.  No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def f64(lbm):
    from mpilattice_boltzmann_amd import f64 as mod
    mod.load_library()
    return mod


def test_read_params_parses_doubles_and_reports_the_reference_messages(lbm, f64, tmp_path):
    path = tmp_path / "in.params"
    path.write_text("128\n64\n100\n10\n0.1\n0.005\n1.85\n")
    p = f64.read_params64(str(path))
    assert (p.nx, p.ny, p.max_iters, p.reynolds_dim) == (128, 64, 100, 10)
    assert p.density == 0.1 and p.accel == 0.005 and p.omega == 1.85           # the doubles themselves ...
    assert p.density != float(np.float32(0.1)) and p.omega != float(np.float32(1.85))   # ... not widened floats
    assert lbm.read_params(str(path)).density == float(np.float32(0.1))        # which is what the float parser gives
    tokens = ["128", "64", "100", "10", "0.1", "0.005", "1.85"]
    names = ["nx", "ny", "maxIters", "reynolds_dim", "density", "accel", "omega"]
    for i, name in enumerate(names):                                            # d2q9-bgk.c:781-800, one die() text per field
        path.write_text("\n".join(tokens[:i]) + ("\n" if i else ""))
        with pytest.raises(lbm.LbmError, match=f"^could not read param file: {name}$"):
            f64.read_params64(str(path))
        path.write_text("\n".join(tokens[:i] + ["x"]) + "\n")
        with pytest.raises(lbm.LbmError, match=f"^could not read param file: {name}$"):
            f64.read_params64(str(path))
    with pytest.raises(lbm.LbmError, match="^could not open input parameter file: "):
        f64.read_params64(str(tmp_path / "absent.params"))


def _awkward_doubles():
    rng = np.random.default_rng(12)
    vals = list(rng.uniform(-1.0, 1.0, 300)) + list(10.0 ** rng.uniform(-300, 300, 300) * rng.choice([-1.0, 1.0], 300))
    # the 13th digit rounds up across a power of ten: 9.9999999999996 -> 1.000000000000E+01, and its neighbours that do not
    vals += [9.9999999999996, 9.99999999999949, 9.9999999999995, 0.99999999999996, 9.9999999999996e-5, 9.9999999999996e99, 9.9999999999996e-100,
             -9.9999999999996e7, 1.0000000000005, 1.00000000000049999, 2.5000000000005, 1.2345678901235e-3, 0.1, 1.0 / 3.0, 0.0, -0.0,
             5e-324, 2.2250738585072014e-308, 1.7976931348623157e308, float("inf"), float("-inf"), float("nan")]
    return np.array(vals, np.float64)


def test_writers_are_byte_identical_to_percent_12E(lbm, f64, tmp_path):
    vals = _awkward_doubles()
    assert "%.12E" % 9.9999999999996 == "1.000000000000E+01"
    av_path = tmp_path / "av_vels.dat"
    f64.write_av_vels64(str(av_path), vals)
    assert av_path.read_text() == "".join("%d:\t%.12E\n" % (i, v) for i, v in enumerate(vals.tolist()))
    # final_state: a 1-row-per-4-values grid, obstacle cells print 0 0 0 density / 3
    n = vals.size // 4
    nx, ny = 4, n // 4
    obs = vals[:nx * ny * 4].reshape(ny, nx, 4).copy()
    obst = np.zeros((ny, nx), np.int32)
    obst[::3, 1] = 1
    p = lbm.Params(nx=nx, ny=ny, max_iters=1, reynolds_dim=1, density=0.1, accel=0.005, omega=1.85)
    fs_path = tmp_path / "final_state.dat"
    f64.write_final_state_obs64(str(fs_path), p, obs, obst)
    want = []
    for y in range(ny):
        for x in range(nx):
            a, b, c, d = (0.0, 0.0, 0.0, 0.1 * (1.0 / 3.0)) if obst[y, x] else obs[y, x].tolist()
            want.append("%d %d %.12E %.12E %.12E %.12E %d\n" % (x, y, a, b, c, d, obst[y, x]))
    assert fs_path.read_text() == "".join(want)


def test_host_reductions(f64):
    lib = f64.load_library()
    rng = np.random.default_rng(4)
    nx, ny = 13, 9
    obs = rng.uniform(-0.1, 0.1, (ny, nx, 4))
    obst = (rng.uniform(size=(ny, nx)) < 0.3).astype(np.int32)
    cp = f64.CParams64(nx, ny, 5, 10, 0.1, 0.005, 1.85)
    tot = lib.lbm64_av_velocity_obs(C.byref(cp), obs.ctypes.data_as(C.POINTER(C.c_double)), obst.ctypes.data_as(C.POINTER(C.c_int)), ny)
    want = 0.0
    for y in range(ny):
        for x in range(nx):
            if not obst[y, x]:
                ux, uy = float(obs[y, x, 0]), float(obs[y, x, 1])
                want += float(np.sqrt(np.float64((ux * ux) + (uy * uy))))
    assert tot == want
    assert lib.lbm64_reynolds(C.byref(cp), 0.0123) == 0.0123 * 10 / (1.0 / 6.0 * (2.0 / 1.85 - 1.0))      # d2q9-bgk.c:1005-1007 in double


def test_header_is_c99_and_a_c_caller_links(lbm, tmp_path):
    src = tmp_path / "caller.c"
    src.write_text('''
#include <stdio.h>
#include "lbm_d2q9_f64.h"
int main(void)
{
  lbm64_params p = {128, 128, 10, 10, 0.1, 0.005, 1.85};
  lbm64_ctx* ctx = NULL;
  if (lbm64_abi_version() != LBM64_ABI_VERSION || LBM64_ABI_VERSION != 1 || LBM_ABI_VERSION != 5) return 2;
  printf("%.17g %p\\n", lbm64_reynolds(&p, 0.5), (void*)ctx);
  return 0;
}
''')
    exe = tmp_path / "caller"
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-L",
                        os.path.dirname(lbm.LIB_PATH), "-llbm_d2q9", f"-Wl,-rpath,{os.path.dirname(lbm.LIB_PATH)}", "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    assert float(r.stdout.split()[0]) == 0.5 * 10 / (1.0 / 6.0 * (2.0 / 1.85 - 1.0))


def test_library_exports_every_declared_lbm64_symbol(lbm, f64):
    header = open(os.path.join(ROOT, "include", "lbm_d2q9_f64.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(lbm64_[a-z_0-9]+)\s*\(", header))
    assert len(declared) == 15
    nm = subprocess.run(["nm", "-D", "--defined-only", lbm.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (lbm64_[a-z_0-9]+)", nm))
    assert declared == exported, declared ^ exported
    assert declared == set(f64.EXPORTS)
    assert f64.load_library().lbm64_abi_version() == 1 == f64.ABI_VERSION
    assert lbm.load_library().lbm_abi_version() == 5                       # the float ABI is as it was


def test_create_without_a_gpu_fails_with_a_message(lbm, f64):
    """On a machine with no GPU lbm64_create reports the HIP error instead of crashing (with one, the device ordinal is out of range)."""
    p = lbm.Params(nx=8, ny=4, max_iters=1, reynolds_dim=1, density=0.1, accel=0.005, omega=1.85)
    with pytest.raises(lbm.LbmError) as e:
        f64.Grid64(p, np.zeros((4, 8), np.int32), device=4096)
    assert "hipSetDevice" in str(e.value)
    for bad, text in ((dict(nx=8, ny=2), "ny must be >= 3"), (dict(nx=0, ny=4), "nx must be positive")):
        q = lbm.Params(max_iters=1, reynolds_dim=1, density=0.1, accel=0.005, omega=1.85, **bad)
        with pytest.raises(lbm.LbmError, match=text):
            f64.Grid64(q, np.zeros((q.ny, q.nx), np.int32))
    with pytest.raises(lbm.LbmError, match="LBM_FLAG_NT_STORES or LBM_FLAG_NO_NT_STORES only"):
        f64.Grid64(p, np.zeros((4, 8), np.int32), flags=256)


def test_cli_refuses_double_precision_on_several_gpus(lbm, digests, tmp_path):
    from conftest import deck_paths
    ppath, opath = deck_paths("tiny_8x3", digests)
    env = {k: v for k, v in os.environ.items() if not k.startswith("LBM_")}
    env.update(LBM_PRECISION="double", LBM_GPUS="2")
    r = subprocess.run([lbm.CLI_PATH, ppath, opath], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "double precision runs on one GPU" in r.stderr
    env.update(LBM_PRECISION="quad", LBM_GPUS="1")
    r = subprocess.run([lbm.CLI_PATH, ppath, opath], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "LBM_PRECISION: expected float or double" in r.stderr
