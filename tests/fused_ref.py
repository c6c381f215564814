"""ctypes wrapper of tests/fused_ref.c — the CPU restatement of a lattice step in the fused arithmetic of
LBM_FLAG_FUSED_ARITH (mode "fused") and in the exact one (mode "exact", pinned to the oracle by tests/test_fused_ref.py).

TEST INFRASTRUCTURE: no GPU, no call into liblbm_d2q9.so.  The C file is compiled on first use with
`gcc -std=c99 -O2 -ffp-contract=off -lm` into tests/_build/ (git-ignored).  Two options are tried first for speed only, and left out
if that compile fails: -fopenmp (rows shared among threads; every sum is added in row order either way) and, where the CPU has it,
-mfma (fmaf is correctly rounded whether libm computes it or the CPU's own instruction does).
"""
from __future__ import annotations

import ctypes as C
import os
import shutil
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "fused_ref.c")
BUILD_DIR = os.path.join(HERE, "_build")
LIB_PATH = os.path.join(BUILD_DIR, "libfused_ref.so")
MODES = {"exact": 0, "fused": 1}

_lib = None


def _cpu_has_fma() -> bool:
    try:
        with open("/proc/cpuinfo") as fh:
            for line in fh:
                if line.startswith("flags"):
                    return " fma " in line + " "
    except OSError:
        pass
    return False


def build() -> str:
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        raise RuntimeError("no C compiler (gcc / cc) for tests/fused_ref.c")
    os.makedirs(BUILD_DIR, exist_ok=True)
    tmp = f"{LIB_PATH}.{os.getpid()}.tmp"
    base = [cc, "-std=c99", "-O2", "-ffp-contract=off"]
    tail = ["-fPIC", "-shared", SRC, "-o", tmp, "-lm"]
    speed = ["-fopenmp"] + (["-mfma"] if _cpu_has_fma() else [])
    if subprocess.run(base + speed + tail, capture_output=True).returncode != 0:
        # no libgomp (or no -mfma) here: the plain build of the header comment; one thread, fmaf from libm, the same bits
        subprocess.run(base + tail, check=True, capture_output=True)
    os.replace(tmp, LIB_PATH)          # atomic: test processes running side by side build the same file
    return LIB_PATH


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH) or os.path.getmtime(SRC) > os.path.getmtime(LIB_PATH):
            build()
        L = C.CDLL(LIB_PATH)
        fp, ip, dp = C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_double)
        L.fused_ref_init.argtypes = [C.c_int, C.c_int, C.c_float, fp]
        L.fused_ref_init.restype = None
        L.fused_ref_run.argtypes = [C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, ip, fp, C.c_int, C.c_int, C.c_int, dp]
        L.fused_ref_run.restype = C.c_int
        L.fused_ref_cells.argtypes = [C.c_size_t, fp, C.c_float, C.c_int, fp, fp]
        L.fused_ref_cells.restype = None
        L.fused_ref_step_terms.argtypes = [C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, ip, fp, C.c_int, C.c_int, dp, dp]
        L.fused_ref_step_terms.restype = C.c_int
        _lib = L
    return _lib


def initial_cells(p) -> np.ndarray:
    """The rest state every run starts from: (ny, nx, 9) float32."""
    cells = np.empty((p.ny, p.nx, 9), np.float32)
    lib().fused_ref_init(p.nx, p.ny, p.density, cells.ctypes.data_as(C.POINTER(C.c_float)))
    return cells


def run(p, obstacles: np.ndarray, n_steps: int, mode: str = "fused", cells0: np.ndarray | None = None, nthreads: int = 4):
    """n_steps steps of the deck (p: anything with nx, ny, density, accel, omega) from the rest state, or from cells0.
    Returns cells (ny, nx, 9) float32 and sums (n_steps,) float64: per step the sum over the free cells of
    sqrt((double)msq) * (double)rinv, not yet divided by the number of free cells.  The thread count changes no bit."""
    obstacles = np.ascontiguousarray(obstacles, np.int32)
    assert obstacles.shape == (p.ny, p.nx)
    cells = initial_cells(p) if cells0 is None else np.array(cells0, dtype=np.float32, order="C").reshape(p.ny, p.nx, 9)
    sums = np.zeros(max(n_steps, 1), np.float64)
    rc = lib().fused_ref_run(p.nx, p.ny, p.density, p.accel, p.omega, obstacles.ctypes.data_as(C.POINTER(C.c_int)),
                             cells.ctypes.data_as(C.POINTER(C.c_float)), n_steps, MODES[mode], nthreads, sums.ctypes.data_as(C.POINTER(C.c_double)))
    if rc != 0:
        raise MemoryError("fused_ref_run")
    return cells, sums[:n_steps]


def cells_msq_rinv(t: np.ndarray, mode: str = "fused", omega: float = 1.0):
    """msq and rinv (float32) of cells given by their nine streamed-in populations, t of shape (..., 9): relax_exact / relax_fused."""
    t = np.ascontiguousarray(t, np.float32)
    assert t.shape[-1] == 9
    msq = np.empty(t.shape[:-1], np.float32)
    rinv = np.empty(t.shape[:-1], np.float32)
    fp = C.POINTER(C.c_float)
    lib().fused_ref_cells(msq.size, t.ctypes.data_as(fp), omega, MODES[mode], msq.ctypes.data_as(fp), rinv.ctypes.data_as(fp))
    return msq, rinv


def step_terms(p, obstacles: np.ndarray, cells: np.ndarray, mode: str = "fused", nthreads: int = 4):
    """One step from `cells`.  Returns the new cells, the step's sum as fused_ref_run adds it, and the (ny, nx) velocity terms of the
    step (0 at blocked cells)."""
    obstacles = np.ascontiguousarray(obstacles, np.int32)
    cells = np.array(cells, dtype=np.float32, order="C").reshape(p.ny, p.nx, 9)
    total = np.zeros(1, np.float64)
    terms = np.zeros((p.ny, p.nx), np.float64)
    rc = lib().fused_ref_step_terms(p.nx, p.ny, p.density, p.accel, p.omega, obstacles.ctypes.data_as(C.POINTER(C.c_int)),
                                    cells.ctypes.data_as(C.POINTER(C.c_float)), MODES[mode], nthreads,
                                    total.ctypes.data_as(C.POINTER(C.c_double)), terms.ctypes.data_as(C.POINTER(C.c_double)))
    if rc != 0:
        raise MemoryError("fused_ref_step_terms")
    return cells, float(total[0]), terms


def free_cells_inv(obstacles: np.ndarray) -> np.float32:
    """1 / (number of free cells) as the reference and the library form it: a float division."""
    return np.float32(1.0) / np.float32(int(obstacles.size - np.count_nonzero(obstacles)))


def av_vels(sums: np.ndarray, obstacles: np.ndarray) -> np.ndarray:
    """Per-step average velocities as lbm_run reports them: (float)(sum * (double)free_cells_inv)."""
    return (np.asarray(sums, np.float64) * np.float64(free_cells_inv(obstacles))).astype(np.float32)
