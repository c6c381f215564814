"""Plain numpy restatements of what the read-out entry points report about a state: lbm_state_checksum, lbm_av_velocity_sum and
lbm_get_observables (include/lbm_d2q9.h; the kernels' documentation in csrc/kernels/aux.h).

TEST INFRASTRUCTURE: no GPU, no library call.  Written from the documented formulas, so that the device's answers are held to
something that is not the device: tests/test_readout_ref.py pins these functions (known answers as literals, additivity,
sensitivity), tests/test_readout.py holds the kernels to them.

A block of cells is a (rows, ncol, 9) float32 array in the reference's AoS layout (t_speed, d2q9-bgk.c:95-98), row-major, x fastest.
"""
from __future__ import annotations

import math

import numpy as np

GOLDEN = np.uint64(0x9E3779B97F4A7C15)
MIX1 = np.uint64(0xBF58476D1CE4E5B9)
MIX2 = np.uint64(0x94D049BB133111EB)
GENERATED_NAN = np.uint32(0xFFC00000)      # the NaN x86 generates (0/0, inf - inf): sign set, quiet, no payload — printed "-NAN"


def _block(cells) -> np.ndarray:
    cells = np.ascontiguousarray(cells, dtype=np.float32)
    if cells.ndim != 3 or cells.shape[2] != 9:
        raise ValueError("cells must be (rows, ncol, 9)")
    return cells


def digest(cells, global_cell0: int = 0, nx_global: int | None = None) -> int:
    """lbm_state_checksum of a block whose first cell has global index `global_cell0` (= y0 * nx_global + x0) in a grid
    `nx_global` cells wide (default: the block's own width, i.e. whole rows):

        sum over cells and k = 0..8 of mix(bits(f[cell][k]) ^ (global_index(cell) * 9 + k) * 0x9E3779B97F4A7C15)   (mod 2^64)
        mix(z): z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;  z = (z ^ z >> 27) * 0x94D049BB133111EB;  z ^ z >> 31

    with all arithmetic in wrap-around uint64 and bits(f) the float's 32 bits zero-extended."""
    cells = _block(cells)
    rows, ncol, _ = cells.shape
    if rows == 0 or ncol == 0:
        return 0
    nxg = ncol if nx_global is None else int(nx_global)
    if nxg < ncol:
        raise ValueError("nx_global is narrower than the block")
    gc = (np.uint64(global_cell0 % (1 << 64))
          + np.arange(rows, dtype=np.uint64)[:, None] * np.uint64(nxg) + np.arange(ncol, dtype=np.uint64)[None, :])
    idx = gc[:, :, None] * np.uint64(9) + np.arange(9, dtype=np.uint64)[None, None, :]
    z = cells.view(np.uint32).astype(np.uint64) ^ (idx * GOLDEN)
    z = (z ^ (z >> np.uint64(30))) * MIX1
    z = (z ^ (z >> np.uint64(27))) * MIX2
    z ^= z >> np.uint64(31)
    return int(z.sum(dtype=np.uint64))


def digest_rows(cells, global_cell0: int = 0, nx_global: int | None = None, chunk_rows: int = 256) -> int:
    """`digest` taken `chunk_rows` rows at a time and added up (the digest is additive over disjoint sets of cells): the temporaries
    are those of one chunk — 256 rows of 8192 cells: 151 MB per uint64 array — whatever the block's size."""
    cells = _block(cells)
    if chunk_rows < 1:
        raise ValueError("chunk_rows must be positive")
    nxg = cells.shape[1] if nx_global is None else int(nx_global)
    total = 0
    for r in range(0, cells.shape[0], chunk_rows):
        total += digest(cells[r:r + chunk_rows], global_cell0 + r * nxg, nxg)
    return total % (1 << 64)


def _moments(cells):
    """rho, u_x, u_y per cell in float32 with the reference's operation order (d2q9-bgk.c:724-746 and, the same, :1084-1107): the
    density is nine additions onto 0.0f, strictly left to right; each numerator is (a + b + c) - (d + e + f)."""
    f = [cells[..., k] for k in range(9)]
    rho = np.zeros(cells.shape[:-1], dtype=np.float32)
    rho = rho + f[0]
    rho = rho + f[1]
    rho = rho + f[2]
    rho = rho + f[3]
    rho = rho + f[4]
    rho = rho + f[5]
    rho = rho + f[6]
    rho = rho + f[7]
    rho = rho + f[8]
    ux = (((f[1] + f[5]) + f[8]) - ((f[3] + f[6]) + f[7])) / rho
    uy = (((f[2] + f[5]) + f[6]) - ((f[4] + f[7]) + f[8])) / rho
    assert rho.dtype == ux.dtype == uy.dtype == np.float32
    return rho, ux, uy


def velocity_terms(cells) -> np.ndarray:
    """av_velocity()'s per-cell term (d2q9-bgk.c:724-748): sqrt((double)(u_x * u_x + u_y * u_y)), the argument formed in float32 —
    returned as float64, shape (rows, ncol), for every cell (the caller leaves the blocked ones out)."""
    cells = _block(cells)
    with np.errstate(all="ignore"):
        _, ux, uy = _moments(cells)
        return np.sqrt(((ux * ux) + (uy * uy)).astype(np.float64))


def velocity_sum(cells, obstacles) -> float:
    """lbm_av_velocity_sum: the sum of `velocity_terms` over the cells with obstacles == 0, exactly rounded (math.fsum) — whatever a
    summation order costs is then the error of the thing compared with this, not of this."""
    terms = velocity_terms(cells)
    free = np.asarray(obstacles).reshape(terms.shape) == 0
    return math.fsum(terms[free].tolist())


def velocity_sum_bound(n_cells: int, block: int = 256, max_blocks: int = 1024) -> float:
    """Relative error a sum of n_cells NON-NEGATIVE doubles may have when it is added up as lbm_av_velocity_sum does it: each lane adds
    at most ceil(n / (blocks * block)) terms serially, a tree of depth log2(block) joins the lanes of a block, the host adds the
    `blocks` partials serially (blocks = min(ceil(n / block), max_blocks)).  Every addition of non-negative numbers errs by at most
    2^-53 of its result, which is at most the total: (terms per lane + log2(block) + blocks) * 2^-53.  (block_sum joins the four waves
    of a block with three serial additions after six shuffle levels, nine on its longest path where a binary tree has eight; the bound
    is kept as the tree's — the tighter of the two — and the errors observed, a few 2^-53, are well inside it.)"""
    blocks = max(1, min(-(-n_cells // block), max_blocks))
    per_lane = -(-n_cells // (blocks * block))
    return (per_lane + int(math.log2(block)) + blocks) * 2.0 ** -53


def observables(cells) -> np.ndarray:
    """lbm_get_observables: (rows, ncol, 4) float32 = {u_x, u_y, u, pressure} as write_values() computes them for a fluid cell
    (d2q9-bgk.c:1084-1111): u = (float)sqrt((double)(u_x * u_x + u_y * u_y)), pressure = rho * (1.0f / 3.0f).  A NaN that comes out of
    a cell none of whose nine populations is a NaN (rho = 0, infinities) has the bits 0xFFC00000, as lbm_observables_kernel
    documents; what a cell WITH a NaN population gives is a NaN whose bits nothing specifies."""
    cells = _block(cells)
    out = np.empty(cells.shape[:-1] + (4,), dtype=np.float32)
    with np.errstate(all="ignore"):
        rho, ux, uy = _moments(cells)
        out[..., 0] = ux
        out[..., 1] = uy
        out[..., 2] = np.sqrt(((ux * ux) + (uy * uy)).astype(np.float64)).astype(np.float32)
        out[..., 3] = rho * (np.float32(1.0) / np.float32(3.0))
    generated = np.isnan(out) & ~np.isnan(cells).any(axis=-1)[..., None]
    out.view(np.uint32)[generated] = GENERATED_NAN
    return out
