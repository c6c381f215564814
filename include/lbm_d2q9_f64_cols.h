/*
 * lbm_d2q9_f64_cols.h — C ABI of COLUMN-PARTITIONED runs of the double-precision mode (liblbm_d2q9.so, csrc/lbm_cols64.hip): a whole
 * periodic nx x ny grid dealt to `nranks` column blocks over one or several GPUs of one process, in the arithmetic lbm_d2q9_f64.h
 * states, K steps per launch and exchange.  Opt-in, under names of its own: nothing of lbm_d2q9_f64.h, lbm_d2q9_f64_rows.h or
 * lbm_d2q9_f64_digest.h changes with it.  It is for grids much wider than tall, where a row block (lbm_d2q9_f64_rows.h) is a few thin
 * rows under as many ghost rows and pushes 72 nx doubles per launch: a column block owns every row, wraps in y as a whole grid does,
 * keeps a few ghost columns and pushes 18 G ny doubles.
 *
 * LAYOUT.  One object, lbm_cols64, is the whole run; one host thread drives it.  The columns are dealt by lbm_decompose_columns
 * (lbm_d2q9.h: whole x-pairs, the spare pairs to the first ranks); rank r owns columns [x0_r, x0_r + nxl_r) of every row, on the device
 * it was given — ranks may share a device.  K = LBM_TUNE_MULTI64_K (2..4, default 4: the knob of the whole grid's and the row
 * partition's multi-step kernels), G = 2 * ceil(K / 2) ghost columns on each side (the ghost rounded up to even).  A rank's two grids
 * are nine planes of ny storage rows of pitch nxl_r + 2 G doubles; owned column x is storage column G + x.  The pitch is even: every
 * x-pair stays 16-byte aligned and a pair's two obstacle bits sit in one word.  There are no ghost rows: y wraps on ny.  The obstacle
 * mask of a rank is a window bitfield over its storage cells, bit c of storage cell c = y * pitch + sx, covering the whole grid's
 * columns x0_r - G .. x0_r + nxl_r + G - 1, periodic in x.
 *
 * WHO RUNS.  A run is taken if and only if nx is even, every rank has nxl_r >= 32 and ny >= 16.  Everything else is refused by
 * lbm_cols64_create, with a message that names the row partition as the alternative: there is no one-step fallback and no size
 * threshold.  Rank r launches ceil(nxl_r / 32) x ceil(ny / 16) tiles of lbm_cols_multi_kernel_f64<K, NT, FULL, EDGE>
 * (csrc/kernels/cols64.h), the column-block form of lbm_multi_kernel_f64 (lbm_d2q9_f64.h: the same tile, LDS frame, sub-steps, cell
 * update and sums).  Where the tiles do not cover the block exactly the kernel's edge-tile form applies, as lbm_d2q9_f64.h describes
 * it: tile (tx, ty) starts at x0 = min(32 tx, nxl_r - 32), y0 = min(16 ty, ny - 16), and a shifted tile owns — stores and counts —
 * only the cells its neighbour does not.
 *
 * EXCHANGE AND ORDER.  After its launch a rank runs lbm64_push_ghost_cols_kernel, which stores all nine planes, every row, of its first
 * G owned columns into the east ghost columns of the rank to its west and of its last G owned columns into the west ghost columns of
 * the rank to its east (the ring is periodic; with one rank the rank is its own neighbour, with two both neighbours are the other
 * rank), formed from the neighbour's own pitch and plane stride: ranks may differ in width.  Between devices these are plain 16-byte
 * vector stores into the peer's memory (peer access, xGMI).  Everything is ordered by stream events at kernel boundaries: no kernel
 * waits for another one, there is no flag, no spin and no time-out on the device.  Per launch t, in rank order, the host enqueues on
 * the rank's stream: a wait for both neighbours' push events of launch t-1, the kernel, the push, the record of this rank's push
 * event of launch t.  With A the source and B the destination grid of launch t:
 *   - kernel t of rank r reads A's ghost columns: the neighbours' pushes t-1 wrote them, and kernel t waited for exactly those.
 *   - push t of rank r writes the ghost columns of a neighbour's B.  The last reader of those was the neighbour's kernel t-1 (B was
 *     its source).  Rank r's kernel t waited for that neighbour's push t-1, which follows the neighbour's kernel t-1 on its stream,
 *     and push t follows kernel t on r's stream: the neighbour's kernel t-1 has finished.  The neighbour's kernel t reads A, not B;
 *     its kernel t+1, which reads B, waits for this very push.  So a push into a neighbour's grid never meets a launch of that
 *     neighbour reading the same grid.
 *   - kernel t of rank r writes B's owned columns.  Their readers were r's own kernel t-1 and push t-2, earlier on the same stream;
 *     no other rank ever reads them (the exchange is push only).  The neighbours' pushes t write B's ghost columns: other cells.
 *   - an event is recorded again two launches later; every wait on its earlier record was enqueued before that.
 * A run of n steps is floor(n / K) launches of K steps and at most one shorter launch, the last.  Before the first launch of every
 * run comes the accelerate pre-pass on the rank's owned cells of row ny-2 and then, on the same stream, a push of the current grid
 * ("push -1"): the ghost columns a launch reads are therefore right after create, after set_cells and between runs.  Inside a launch
 * the kernel accelerates every copy of row ny-2 (owned, ghost column, ring) between its sub-steps, and after its last sub-step
 * exactly when another step of the run follows, before the push on the same stream.  A launch of k steps consumes k of the G ghost
 * columns on each side; the G columns pushed after it are whole again.  Sources of a push are owned columns and targets ghost
 * columns: disjoint even where a rank is its own neighbour, because nxl_r >= 32 > 2 G.
 *
 * WHAT IS COMPUTED.  The populations are the bits lbm64_run gives on the whole grid, for EVERY rank count.  av_vels[t]: per rank the
 * tree lbm_d2q9_f64.h states for lbm_multi_kernel_f64 over the rank's tiles, then nranks - 1 host additions in rank order, times
 * 1.0 / free_cells.  No atomics: the same state and the same rank count give the same bits in every run.
 *
 * Conventions are those of lbm_d2q9_f64_rows.h: 0 on success, otherwise lbm_last_error() has the message for the calling thread;
 * cells cross the boundary as AoS, 9 doubles per cell of the WHOLE grid, row-major, x fastest; obstacles as the reference's int map
 * of the whole grid.  The host half of lbm_d2q9_f64.h serves these runs as it is.
 *
 * OUT OF SCOPE: px x py tiles with py > 1; a one-step column kernel; odd nx or blocks narrower than 32; ranks in separate
 * processes; more than one launch per exchange; overlap of interior tiles with the push.
 */
#ifndef LBM_D2Q9_F64_COLS_H
#define LBM_D2Q9_F64_COLS_H

#include <stddef.h>

#include "lbm_d2q9_f64.h"           /* lbm64_params, LBM_FLAG_NT_STORES / LBM_FLAG_NO_NT_STORES, lbm_last_error */

#ifdef __cplusplus
extern "C" {
#endif

#define LBM_COLS64_ABI_VERSION 1
#define LBM_COLS64_MAX_RANKS 64

typedef struct lbm_cols64 lbm_cols64;   /* opaque: the device state of every rank of one run */

int lbm_cols64_abi_version(void);

/* A whole periodic nx x ny grid in the initial state of d2q9-bgk.c:880-902, its columns dealt to `nranks` ranks.
 * obstacles_all = ny*nx ints, the whole grid's map.  devices = nranks HIP ordinals, or NULL: rank r on device r % (device count).
 * Ranks may share a device.  flags: 0, LBM_FLAG_NT_STORES or LBM_FLAG_NO_NT_STORES (non-temporal stores of the output grid: by default
 * once a RANK's two grids exceed the Infinity Cache).
 * Refused, with a message and before the first HIP call: nranks outside 1..LBM_COLS64_MAX_RANKS; odd nx; a rank of fewer than 32
 * columns; ny < 16; free_cells < 1; any other flag; a rank whose storage has 2^31 - 4096 cells or more (the kernels' cell indices are
 * 32-bit).  Refused after it: two ranks on distinct devices that hipDeviceCanAccessPeer denies. */
int lbm_cols64_create(lbm_cols64** run, const lbm64_params* params, int free_cells, const int* obstacles_all, int nranks,
                      const int* devices, unsigned flags);
int lbm_cols64_destroy(lbm_cols64* run);

/* n_steps iterations of d2q9-bgk.c:315-394 on every rank; av_vels[t] (may be NULL) as described above.  May be called repeatedly; the
 * state it leaves is the post-step state, NOT yet accelerated for a next step, exactly as lbm64_run.  Returns when every rank is
 * idle. */
int lbm_cols64_run(lbm_cols64* run, int n_steps, double* av_vels);

/* The state of the whole grid, AoS: ny*nx*9 doubles, gathered from / scattered to the ranks' owned columns in chunks of rows, with no
 * second copy of the state.  Bits travel unchanged both ways (NaN payloads, signed zeros, denormals). */
int lbm_cols64_get_cells(lbm_cols64* run, double* cells_aos);
int lbm_cols64_set_cells(lbm_cols64* run, const double* cells_aos);

/* {u_x, u_y, u, pressure} per cell of the whole grid as lbm64_get_observables gives them: ny*nx*4 doubles. */
int lbm_cols64_get_observables(lbm_cols64* run, double* obs);

/* av_velocity()'s sum over the free cells (d2q9-bgk.c:716-751) of the current state: each rank sums its block as
 * lbm64_av_velocity_sum does (per lane, per block of lanes), the host adds the blocks' sums, rank after rank. */
int lbm_cols64_av_velocity_sum(lbm_cols64* run, double* tot_u);

/* Device time of the last lbm_cols64_run: events around each rank's launches and pushes, the largest span over the ranks; and the
 * number of launches of the run, ceil(n_steps / K) * nranks. */
int lbm_cols64_last_run_ms(lbm_cols64* run, double* ms, int* launches);

/* What a launch looks like: the kernel's name ("lbm_cols_multi_kernel_f64<K>", "<K,nt>", "<K,edge>" or "<K,nt,edge>"), the rank
 * count, and of the rank with the most tiles: those tiles (one more block folds the previous launch's sums) and the 512 cells a
 * block advances; the bytes of all ranks' grids, ghost columns included: 2 * 9 * 8 * ny * (nx + 2 * G * nranks). */
int lbm_cols64_describe(const lbm_cols64* run, char* kernel_name, size_t len, int* nranks, long long* blocks, long long* cells_per_block,
                        long long* state_bytes);

/* The state digest of lbm_d2q9_f64_digest.h for the whole grid's rows [y_begin, y_end) of the current state, with lbm_digest64_rows'
 * contract and refusals: row_digests (y_end - y_begin entries) and digest (their wrap-around sum) may each be NULL, not both;
 * 0 <= y_begin <= y_end <= ny.  Every rank digests its columns of those rows on its device; the host adds the ranks' parts of a row
 * wrap-around, which is that row's digest by lbm_digest64_host's definition.  Leaves the run as it was. */
int lbm_cols64_digest(lbm_cols64* run, int y_begin, int y_end, unsigned long long* row_digests, unsigned long long* digest);

#ifdef __cplusplus
}
#endif

#endif /* LBM_D2Q9_F64_COLS_H */
