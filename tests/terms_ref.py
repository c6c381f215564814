"""The sum|u| term of a cell, sqrt((double)msq) * (double)rinv (d2q9-bgk.c:667), restated in numpy from the cell's nine streamed-in
populations, and the per-step exactly rounded sums of those terms that the device's per-step double sums are held to.

TEST INFRASTRUCTURE: no GPU, no call into liblbm_d2q9.so.  Two arithmetics, as the library has them:
  exact   msq and rinv in float32, every operation rounded on its own, in relax_core's order (kernels/common.h) — which is the
          oracle's (oracle/d2q9_oracle.c relax_row): rho = ((t0 + t1) + t2) + ... + t8, mx = ((((t1 + t5) + t8) - t3) - t6) - t7,
          my = ((((t2 + t5) + t6) - t4) - t7) - t8, msq = mx * mx + my * my, rinv = 1 / rho.  numpy's float32 operations are IEEE ones.
  fused   the same moments, msq = fma(my, my, mx * mx): numpy has no fused multiply-add, so msq and rinv come from tests/fused_ref.c
          (fused_ref_cells), whose exact mode tests/test_fused_ref.py pins to the oracle.
The term is np.sqrt(float64(msq)) * float64(rinv) in both: a correctly rounded double root and one double product."""
from __future__ import annotations

import numpy as np

import fused_ref
import oracle_lib


def moments(t: np.ndarray):
    """rho, mx, my (float32) of cells t[..., 9] in relax_core's order of additions."""
    t = np.asarray(t, np.float32)
    assert t.dtype == np.float32 and t.shape[-1] == 9
    with np.errstate(all="ignore"):
        rho = t[..., 0] + t[..., 1]
        for k in range(2, 9):
            rho = rho + t[..., k]
        mx = t[..., 1] + t[..., 5]
        mx = mx + t[..., 8]
        mx = mx - t[..., 3]
        mx = mx - t[..., 6]
        mx = mx - t[..., 7]
        my = t[..., 2] + t[..., 5]
        my = my + t[..., 6]
        my = my - t[..., 4]
        my = my - t[..., 7]
        my = my - t[..., 8]
    assert rho.dtype == np.float32 and mx.dtype == np.float32 and my.dtype == np.float32
    return rho, mx, my


def msq_rinv(t: np.ndarray, fused: bool = False):
    """msq and rinv (float32) of cells t[..., 9]."""
    if fused:
        return fused_ref.cells_msq_rinv(t, "fused")
    rho, mx, my = moments(t)
    with np.errstate(all="ignore"):
        msq = mx * mx + my * my                    # two float32 products, one float32 sum: numpy rounds each
        rinv = np.float32(1.0) / rho
    assert msq.dtype == np.float32 and rinv.dtype == np.float32
    return msq, rinv


def term_of(msq: np.ndarray, rinv: np.ndarray) -> np.ndarray:
    """sqrt((double)msq) * (double)rinv."""
    with np.errstate(all="ignore"):
        return np.sqrt(np.asarray(msq, np.float32).astype(np.float64)) * np.asarray(rinv, np.float32).astype(np.float64)


def cell_terms(t: np.ndarray, fused: bool = False):
    """term (float64), msq, rinv (float32) of cells t[..., 9]."""
    msq, rinv = msq_rinv(t, fused)
    return term_of(msq, rinv), msq, rinv


def pulled(cells: np.ndarray) -> np.ndarray:
    """The nine populations that stream into every cell of a periodic (ny, nx, 9) grid (d2q9-bgk.c:526-538): population k comes from
    the neighbour at (x - dx[k], y - dy[k])."""
    dx = (0, 1, 0, -1, 0, 1, -1, -1, 1)
    dy = (0, 0, 1, 0, -1, 1, 1, -1, -1)
    cells = np.asarray(cells, np.float32)
    return np.stack([np.roll(cells[..., k], (dy[k], dx[k]), axis=(0, 1)) for k in range(9)], axis=-1)


def accelerated(p, obstacles: np.ndarray, cells: np.ndarray) -> np.ndarray:
    """A copy of the state with accelerate_flow applied to row ny - 2 (oracle_accelerate_row), as every step begins."""
    import ctypes as C
    out = np.array(cells, dtype=np.float32, order="C")
    obst = np.ascontiguousarray(obstacles, np.int32)
    cp = oracle_lib.cparams(p)
    row = np.ascontiguousarray(out[p.ny - 2])
    oracle_lib.lib().oracle_accelerate_row(C.byref(cp), oracle_lib._f(row), oracle_lib._i(np.ascontiguousarray(obst[p.ny - 2])))
    out[p.ny - 2] = row
    return out


def step_terms(p, obstacles: np.ndarray, cells: np.ndarray, fused: bool = False) -> np.ndarray:
    """(ny, nx) terms of the step that starts from `cells`, 0 at blocked cells: accelerate, pull, cell_terms."""
    terms, _, _ = cell_terms(pulled(accelerated(p, obstacles, cells)), fused)
    return np.where(np.asarray(obstacles) != 0, 0.0, terms)


class StepSums:
    """What a run of n steps from cells0 must give: .cells (the final state), .sums (n,) the exactly rounded per-step sums of the free
    cells' terms (not divided by the number of free cells), .terms a list of n (ny, nx) term arrays (0 at blocked cells).
    exact arithmetic: the oracle (oracle_lib.run_from); fused arithmetic: tests/fused_ref.c step by step, the sum by oracle_exact_sum."""

    def __init__(self, p, obstacles: np.ndarray, cells0: np.ndarray, n_steps: int, fused: bool = False):
        obstacles = np.ascontiguousarray(obstacles, np.int32)
        if not fused:
            self.cells, _, self.sums, self.terms = oracle_lib.run_from(p, obstacles, cells0, n_steps, sums=True, keep_terms=True)
        else:
            cells, sums, self.terms = np.asarray(cells0, np.float32), [], []
            for _ in range(n_steps):
                cells, _, terms = fused_ref.step_terms(p, obstacles, cells, "fused")
                self.terms.append(terms)
                sums.append(oracle_lib.exact_sum(terms, obstacles))
            self.cells, self.sums = cells, np.asarray(sums, np.float64)
        self.free = obstacles == 0
        self.sums.setflags(write=False)

    def smallest_free_term(self, step: int) -> float:
        return float(self.terms[step][self.free].min())

    def share_below(self, step: int, threshold: float) -> float:
        """Share of the free cells whose term of that step is below the threshold."""
        return float(np.mean(self.terms[step][self.free] < threshold))


def random_state(ny: int, nx: int, seed: int) -> np.ndarray:
    """Populations 0.004 - 0.024, nine unrelated values per cell (tests/test_gpu_parity.py test_set_cells_random_state): every free cell
    carries a term of ordinary size from the first step on."""
    rng = np.random.default_rng(seed)
    return (rng.random((ny, nx, 9), dtype=np.float32) * np.float32(0.02) + np.float32(0.004)).astype(np.float32)
