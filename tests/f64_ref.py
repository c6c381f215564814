"""ctypes wrapper of tests/f64_ref.c — the CPU restatement of the double-precision mode (include/lbm_d2q9_f64.h) — and, in numpy, the
end-of-run pieces of that mode: av_velocity, calc_reynolds, the write_values arithmetic and the two output files.

TEST INFRASTRUCTURE: no GPU, no call into liblbm_d2q9.so.  The C file is compiled on first use with
`gcc -std=c99 -O2 -ffp-contract=off -lm` into tests/_build/ (git-ignored); -fopenmp is tried first for speed only (rows shared among
threads; every sum is added by one thread in a fixed order either way).

tests/test_f64_ref.py pins this to the results the reference published; tests/test_f64.py holds the kernels to it.
"""
from __future__ import annotations

import ctypes as C
import gzip
import json
import math
import os
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "f64_ref.c")
BUILD_DIR = os.path.join(HERE, "_build")
LIB_PATH = os.path.join(BUILD_DIR, "libf64_ref.so")
GOLDEN = os.path.join(HERE, "golden")

_lib = None
_deck_cache: dict = {}

# Distances of THIS restatement from the results the reference shipped for the 128 x 128 deck (tests/test_f64_ref.py measures them
# again and prints them; DESIGN.md section 5 lists the other decks).  The arithmetic is deterministic: what is left is the printing of
# both sides to 13 significant digits.  The tests assert at twice the measured value.
MEASURED_AV_VELS_REL = 6.87e-13        # largest relative difference of av_vels over the 40 000 steps
MEASURED_FINAL_STATE_ABS = 1.26e-14    # largest absolute difference of final_state columns 3..6
MEASURED_REYNOLDS_REL = 1.21e-13       # 9.763598020524826 against the printed 9.763598020526E+00
AV_VELS_LIMIT, FINAL_STATE_LIMIT, REYNOLDS_LIMIT = 2 * MEASURED_AV_VELS_REL, 2 * MEASURED_FINAL_STATE_ABS, 2 * MEASURED_REYNOLDS_REL


def build() -> str:
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        raise RuntimeError("no C compiler (gcc / cc) for tests/f64_ref.c")
    os.makedirs(BUILD_DIR, exist_ok=True)
    tmp = f"{LIB_PATH}.{os.getpid()}.tmp"
    base = [cc, "-std=c99", "-O2", "-ffp-contract=off"]
    tail = ["-fPIC", "-shared", SRC, "-o", tmp, "-lm"]
    if subprocess.run(base + ["-fopenmp"] + tail, capture_output=True).returncode != 0:
        subprocess.run(base + tail, check=True, capture_output=True)       # no libgomp here: one thread, the same bits
    os.replace(tmp, LIB_PATH)          # atomic: test processes running side by side build the same file
    return LIB_PATH


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH) or os.path.getmtime(SRC) > os.path.getmtime(LIB_PATH):
            build()
        L = C.CDLL(LIB_PATH)
        ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
        L.f64_ref_init.argtypes = [C.c_int, C.c_int, C.c_double, dp]
        L.f64_ref_init.restype = None
        L.f64_ref_run.argtypes = [C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, ip, dp, C.c_int, C.c_int, dp, dp]
        L.f64_ref_run.restype = C.c_int
        L.f64_ref_run_report.argtypes = L.f64_ref_run.argtypes + [ip, dp]
        L.f64_ref_run_report.restype = C.c_int
        L.f64_ref_accel_weights.argtypes = [C.c_double, C.c_double, dp, dp]
        L.f64_ref_accel_weights.restype = None
        L.f64_ref_cells.argtypes = [C.c_size_t, dp, ip, ip, C.c_double, C.c_double, C.c_double, dp, dp]
        L.f64_ref_cells.restype = None
        L.f64_ref_cells_moments.argtypes = L.f64_ref_cells.argtypes + [dp]
        L.f64_ref_cells_moments.restype = None
        _lib = L
    return _lib


def _dp(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def read_params(path: str) -> SimpleNamespace:
    """The seven tokens of a parameter file, the three reals as doubles (Python's float() is strtod: what %lf reads)."""
    tok = open(path).read().split()
    return SimpleNamespace(nx=int(tok[0]), ny=int(tok[1]), max_iters=int(tok[2]), reynolds_dim=int(tok[3]),
                           density=float(tok[4]), accel=float(tok[5]), omega=float(tok[6]))


def read_obstacles(path: str, nx: int, ny: int) -> np.ndarray:
    obst = np.zeros((ny, nx), np.int32)
    for line in open(path):
        t = line.split()
        if t:
            obst[int(t[1]), int(t[0])] = 1
    return obst


def initial_cells(p) -> np.ndarray:
    """The rest state every run starts from: (ny, nx, 9) float64."""
    cells = np.empty((p.ny, p.nx, 9), np.float64)
    lib().f64_ref_init(p.nx, p.ny, p.density, _dp(cells))
    return cells


def run(p, obstacles: np.ndarray, n_steps: int, cells0: np.ndarray | None = None, nthreads: int = 8):
    """n_steps steps of the deck (p: anything with nx, ny, density, accel, omega as Python floats) from the rest state, or from cells0.
    Returns cells (ny, nx, 9) float64, serial (n_steps,) and exact (n_steps,): per step the sum over the free cells of
    sqrt(msq) * rinv in the reference's order of additions, and exactly rounded; neither divided by the number of free cells.
    The thread count changes no bit."""
    obstacles = np.ascontiguousarray(obstacles, np.int32)
    assert obstacles.shape == (p.ny, p.nx)
    cells = initial_cells(p) if cells0 is None else np.array(cells0, dtype=np.float64, order="C").reshape(p.ny, p.nx, 9)
    serial = np.zeros(max(n_steps, 1), np.float64)
    exact = np.zeros(max(n_steps, 1), np.float64)
    rc = lib().f64_ref_run(p.nx, p.ny, p.density, p.accel, p.omega, obstacles.ctypes.data_as(C.POINTER(C.c_int)), _dp(cells), n_steps, nthreads,
                           _dp(serial), _dp(exact))
    if rc != 0:
        raise MemoryError("f64_ref_run")
    return cells, serial[:n_steps], exact[:n_steps]


POSITIVE, NAN_TERM, POS_INF_TERM, NEG_INF_TERM = 1, 2, 4, 8        # f64_ref.c's F64_REF_* status bits


def run_report(p, obstacles: np.ndarray, n_steps: int, cells0: np.ndarray | None = None, nthreads: int = 8):
    """run(), and what decides how each step's sum can be compared: cells, exact, status, abs_exact.
    status (n_steps,) int32: POSITIVE where every free cell had a positive density in that step; NAN_TERM, POS_INF_TERM, NEG_INF_TERM
    where some term was one.  abs_exact (n_steps,): the exactly rounded sum of the terms' magnitudes."""
    obstacles = np.ascontiguousarray(obstacles, np.int32)
    assert obstacles.shape == (p.ny, p.nx)
    cells = initial_cells(p) if cells0 is None else np.array(cells0, dtype=np.float64, order="C").reshape(p.ny, p.nx, 9)
    m = max(n_steps, 1)
    serial, exact, abs_exact, status = np.zeros(m), np.zeros(m), np.zeros(m), np.zeros(m, np.int32)
    rc = lib().f64_ref_run_report(p.nx, p.ny, p.density, p.accel, p.omega, obstacles.ctypes.data_as(C.POINTER(C.c_int)), _dp(cells), n_steps,
                                  nthreads, _dp(serial), _dp(exact), status.ctypes.data_as(C.POINTER(C.c_int)), _dp(abs_exact))
    if rc != 0:
        raise MemoryError("f64_ref_run_report")
    return cells, exact[:n_steps], status[:n_steps], abs_exact[:n_steps]


def benign(status: np.ndarray) -> np.ndarray:
    """Steps whose terms are all non-negative numbers: the premise of the summation bounds (tests/test_f64.py sum_bound and its kin)."""
    return np.asarray(status) == POSITIVE


def accel_weights(density: float, accel: float):
    """(w1, w2): accelerate_flow's axis and diagonal weights as the restatement forms them (d2q9-bgk.c:445-446)."""
    w1, w2 = C.c_double(0.0), C.c_double(0.0)
    lib().f64_ref_accel_weights(density, accel, C.byref(w1), C.byref(w2))
    return w1.value, w2.value


def cells_each(pops: np.ndarray, blocked: np.ndarray, accel: np.ndarray, omega: float, w1: float, w2: float, moments: bool = False):
    """f64_ref_cells: n cells without neighbours.  pops (n, 9) = what streamed in; returns out (n, 9) after bounce-back or relaxation
    and, where accel is set on a free cell, the next step's accelerate_flow, and term (n,).  With moments=True also mom (n, 2) =
    {density, squared momentum} as collide() formed them."""
    pops = np.ascontiguousarray(pops, np.float64)
    n = pops.shape[0]
    assert pops.shape == (n, 9)
    blocked = np.ascontiguousarray(blocked, np.int32)
    accel = np.ascontiguousarray(accel, np.int32)
    assert blocked.shape == accel.shape == (n,)
    out, term = np.empty((n, 9), np.float64), np.empty(n, np.float64)
    ip = C.POINTER(C.c_int)
    if moments:
        mom = np.empty((n, 2), np.float64)
        lib().f64_ref_cells_moments(n, _dp(pops), blocked.ctypes.data_as(ip), accel.ctypes.data_as(ip), omega, w1, w2, _dp(out), _dp(term), _dp(mom))
        return out, term, mom
    lib().f64_ref_cells(n, _dp(pops), blocked.ctypes.data_as(ip), accel.ctypes.data_as(ip), omega, w1, w2, _dp(out), _dp(term))
    return out, term


def free_cells(obstacles: np.ndarray) -> int:
    return int(obstacles.size - np.count_nonzero(obstacles))


def av_vels(sums: np.ndarray, obstacles: np.ndarray) -> np.ndarray:
    """Per-step average velocities: sum * (1.0 / free_cells), d2q9-bgk.c:367 and :950 in double."""
    return np.asarray(sums, np.float64) * (1.0 / free_cells(obstacles))


def _moments(cells: np.ndarray):
    """rho, u_x, u_y per cell with the reference's operation order (d2q9-bgk.c:724-746, and the same :1084-1107): nine additions onto
    0.0, left to right; each numerator (a + b + c) - (d + e + f)."""
    f = [cells[..., k] for k in range(9)]
    rho = np.zeros(cells.shape[:-1], np.float64)
    for k in range(9):
        rho = rho + f[k]
    ux = (((f[1] + f[5]) + f[8]) - ((f[3] + f[6]) + f[7])) / rho
    uy = (((f[2] + f[5]) + f[6]) - ((f[4] + f[7]) + f[8])) / rho
    return rho, ux, uy


def observables(cells: np.ndarray) -> np.ndarray:
    """lbm64_get_observables: (ny, nx, 4) = {u_x, u_y, u, pressure} as write_values computes them for a fluid cell (:1084-1111)."""
    cells = np.ascontiguousarray(cells, np.float64)
    out = np.empty(cells.shape[:-1] + (4,), np.float64)
    with np.errstate(all="ignore"):
        rho, ux, uy = _moments(cells)
        out[..., 0] = ux
        out[..., 1] = uy
        out[..., 2] = np.sqrt((ux * ux) + (uy * uy))
        out[..., 3] = rho * (1.0 / 3.0)
    return out


def velocity_terms(cells: np.ndarray) -> np.ndarray:
    with np.errstate(all="ignore"):
        _, ux, uy = _moments(np.ascontiguousarray(cells, np.float64))
        return np.sqrt((ux * ux) + (uy * uy))


def velocity_sum_serial(cells: np.ndarray, obstacles: np.ndarray) -> float:
    """av_velocity()'s accumulator (:716-751): the free cells' terms added in cell order."""
    terms = velocity_terms(cells)[np.asarray(obstacles) == 0]
    s = 0.0
    for v in terms.tolist():
        s += v
    return s


def velocity_sum_exact(cells: np.ndarray, obstacles: np.ndarray) -> float:
    return math.fsum(velocity_terms(cells)[np.asarray(obstacles) == 0].tolist())


def reynolds(p, cells: np.ndarray, obstacles: np.ndarray) -> float:
    """calc_reynolds (:1005-1007) on av_velocity (:753)."""
    av = velocity_sum_serial(cells, obstacles) * (1.0 / free_cells(obstacles))
    viscosity = 1.0 / 6.0 * (2.0 / p.omega - 1.0)
    return av * p.reynolds_dim / viscosity


def final_state_values(p, cells: np.ndarray, obstacles: np.ndarray) -> np.ndarray:
    """What write_values prints per cell: (ny, nx, 4); an obstacle cell prints 0, 0, 0, density * (1.0 / 3.0) (:1076-1080)."""
    obs = observables(cells)
    blocked = np.asarray(obstacles) != 0
    obs[blocked] = (0.0, 0.0, 0.0, p.density * (1.0 / 3.0))
    return obs


def final_state_text(p, cells: np.ndarray, obstacles: np.ndarray) -> str:
    """final_state.dat (:1115), formatted by Python's own %-operator."""
    v = final_state_values(p, cells, obstacles)
    lines = []
    for y in range(p.ny):
        for x in range(p.nx):
            a, b, c, d = v[y, x].tolist()
            lines.append("%d %d %.12E %.12E %.12E %.12E %d\n" % (x, y, a, b, c, d, int(obstacles[y, x])))
    return "".join(lines)


def av_vels_text(av: np.ndarray) -> str:
    return "".join("%d:\t%.12E\n" % (i, v) for i, v in enumerate(np.asarray(av, np.float64).tolist()))


# ---- the reference's published results -----------------------------------------------------------------------------------------

def published() -> dict:
    with open(os.path.join(GOLDEN, "f64_published.json")) as fh:
        return json.load(fh)


def golden_av_vels(deck: str) -> np.ndarray:
    with gzip.open(os.path.join(GOLDEN, "check", f"{deck}.av_vels.dat.gz"), "rt") as fh:
        return np.array([float(line.split()[1]) for line in fh], np.float64)


def golden_final_state(deck: str) -> np.ndarray:
    """Columns 3..6 (1-based) of the shipped final_state file, (cells, 4), in file order (y outer, x inner)."""
    with gzip.open(os.path.join(GOLDEN, "check", f"{deck}.final_state.dat.gz"), "rt") as fh:
        return np.loadtxt(fh, usecols=(2, 3, 4, 5), dtype=np.float64)


def deck(name: str):
    p = read_params(os.path.join(GOLDEN, "decks", f"input_{name}.params"))
    return p, read_obstacles(os.path.join(GOLDEN, "decks", f"obstacles_{name}.dat"), p.nx, p.ny)


def deck_run(name: str = "128x128", nthreads: int = 8):
    """The whole deck through the restatement, once per process (6 s for 128x128 on 8 threads): p, obstacles, cells, serial, exact."""
    if name not in _deck_cache:
        p, obst = deck(name)
        _deck_cache[name] = (p, obst) + run(p, obst, p.max_iters, nthreads=nthreads)
    return _deck_cache[name]
