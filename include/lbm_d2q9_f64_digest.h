/*
 * lbm_d2q9_f64_digest.h — C ABI of the STATE DIGESTS of the double-precision mode (liblbm_d2q9.so): one 64-bit digest per ROW of a
 * grid of doubles, for a whole grid (lbm_d2q9_f64.h), for every rank of a row-partitioned run (lbm_d2q9_f64_rows.h) and for a state
 * that lies in host memory.  The counterpart of lbm_state_checksum of lbm_d2q9.h, under names of its own: nothing of the other
 * headers changes with it.
 *
 * Every faster way to advance a double-precision grid is held to "the same populations bit for bit".  The digests answer "is this
 * the whole grid's state, and if not, in which rows does it differ" with one pass over the state on the device and 8 * rows bytes
 * to the host, where lbm64_get_cells / lbm_rows64_get_cells move 72 bytes per cell.
 *
 * THE DEFINITION.  For the cell at global column x, global row y of a grid nx cells wide, and population k in 0..8, with f the
 * population's value and all arithmetic unsigned, modulo 2^64:
 *
 *     idx  = (y * nx + x) * 9 + k
 *     z    = bits64(f) ^ (idx * 0x9E3779B97F4A7C15)        bits64: the double's object representation, unchanged
 *     z    = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9
 *     z    = (z ^ (z >> 27)) * 0x94D049BB133111EB
 *     term = z ^ (z >> 31)
 *
 * (lbm_state_checksum's mixer with the 64 value bits in place of 32.)  row_digest[y] is the wrap-around sum of `term` over the
 * row's nx cells and nine populations; the digest of a row range is the wrap-around sum of its rows' digests; an empty range has
 * digest 0.  So a digest depends on where a value sits, adds up over disjoint rows, and does not depend on who holds the rows or in
 * what storage: the ranks' digests of a partitioned run add up to the whole grid's.  It tells -0.0 from +0.0 and one NaN payload
 * from another.  Obstacle cells count like any other; ghost rows never do.  Two states that differ in one row differ in that row's
 * digest with probability 1 - 2^-64.
 *
 * ON THE DEVICE: lbm64_row_digest_kernel (csrc/kernels/step64.h), one block of 256 lanes per row, the lanes striding along x through
 * the nine planes read as 64-bit integers (no value passes through a floating-point register), joined by the wave's butterfly and
 * through LDS; no atomics.  It reads the CURRENT grid and writes nothing but its own output array: not the populations, not the
 * partial sums a later launch folds, not the step counter, not the events of lbm64_last_run_kernel_ms / lbm_rows64_last_run_ms.  A
 * run of n steps, a digest, a run of m steps leave the populations and av_vels of the two runs without the digest.
 * Measured on one MI355X (profiles/r19/f64_digest.txt): at 8192 x 8192 the kernel takes 772 us, 6.26 TB/s of state read (0.68 of
 * lbm64_observables_kernel's 1137 us for the same grid, which moves 104 B per cell to this one's 72); the whole call 0.97 ms beside
 * 290 ms of lbm64_get_cells, on 8 ranks of one GPU 1.26 ms beside 294 ms of lbm_rows64_get_cells; at 1024 x 1024 0.17 ms beside 4.6 ms.
 *
 * Conventions are those of lbm_d2q9.h: 0 on success, otherwise lbm_last_error() has the message for the calling thread.  Refused,
 * with a message and before the first HIP call: a null context or run; both output pointers null; y_begin < 0, y_end > ny or
 * y_begin > y_end; for the host form a null state with rows > 0, nx < 1, rows < 0 or y0 < 0.  y_begin == y_end succeeds with digest 0
 * and launches nothing.
 *
 * NOT HERE: the digest of a column-partitioned run, whose ranks each hold a PART of every row.  It is lbm_cols64_digest of
 * lbm_d2q9_f64_cols.h: the ranks' parts of a row, added wrap-around, are this header's row digest by the definition above.
 */
#ifndef LBM_D2Q9_F64_DIGEST_H
#define LBM_D2Q9_F64_DIGEST_H

#include "lbm_d2q9_f64_rows.h"      /* lbm64_ctx, lbm_rows64, lbm_last_error */

#ifdef __cplusplus
extern "C" {
#endif

#define LBM_DIGEST64_ABI_VERSION 1

int lbm_digest64_abi_version(void);

/* Host only, no GPU: `rows` rows of AoS cells (9 doubles per cell, x fastest) that are global rows [y0, y0 + rows) of a grid nx cells
 * wide — a state read from anywhere (lbm64_get_cells, a CPU restatement, a file).  row_digests: `rows` entries, or NULL; digest: their
 * wrap-around sum, or NULL; not both NULL. */
int lbm_digest64_host(const double* cells_aos, int nx, int rows, long long y0, unsigned long long* row_digests, unsigned long long* digest);

/* The current state of a whole grid, global rows [y_begin, y_end).  row_digests: y_end - y_begin entries, or NULL; digest: their
 * wrap-around sum, or NULL; not both NULL. */
int lbm_digest64_grid(lbm64_ctx* ctx, int y_begin, int y_end, unsigned long long* row_digests, unsigned long long* digest);

/* The same of a row-partitioned run: every rank that owns rows of the range digests them on its device and stream, all ranks
 * enqueued before any is waited for; row y of the whole grid lands in row_digests[y - y_begin] whichever rank owns it.  A range
 * inside one rank launches on that rank only. */
int lbm_digest64_rows(lbm_rows64* run, int y_begin, int y_end, unsigned long long* row_digests, unsigned long long* digest);

#ifdef __cplusplus
}
#endif

#endif /* LBM_D2Q9_F64_DIGEST_H */
