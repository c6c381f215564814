/*
 * lbm_d2q9_f64_rows.h — C ABI of ROW-PARTITIONED runs of the double-precision mode (liblbm_d2q9.so, csrc/lbm_rows64.hip): the
 * reference's row decomposition with a halo exchange (d2q9-bgk.c:244-251, 295-313, 326-328, 364, 834-862) over one or several GPUs of
 * one process, in the arithmetic lbm_d2q9_f64.h states.  Opt-in, under names of its own: nothing of lbm_d2q9_f64.h changes with it.
 *
 * One object, lbm_rows64, is the whole run; one host thread drives it.  The rows are dealt to `nranks` ranks by lbm_decompose (the
 * reference's rule, :834-862); rank r keeps its rows on the device it was given — ranks may share a device — as two grids of
 * ny_local + 2 storage rows: a ghost row below the owned rows and one above.  A step of a rank is one launch of
 * lbm_rows_kernel_f64<CELLS, NT> (csrc/kernels/rows64.h), the partition form of lbm_step_kernel_f64: the same lane forms (an x-pair per
 * lane where nx is even, else a cell), the same cell update, the same chunks of 256 units per block — over rows that do not wrap:
 * the rows above and below an edge row are the ghost rows.  After its step kernel a rank runs lbm64_push_rows_kernel, which stores
 * the three populations that cross each cut into the neighbours' ghost rows of the grid just written: populations 4, 7, 8 of its
 * first owned row into the ghost row above the rank below, populations 2, 5, 6 of its last owned row into the ghost row below the rank
 * above (the ring is periodic; with one rank the rank is its own neighbour, with two both neighbours are the other rank; a rank of
 * one row sends that row both ways).  Between devices these are plain vector stores into the peer's memory (peer access, xGMI).  The
 * other six planes of a ghost row are never read and never written.
 *
 * ORDER.  Everything is ordered by stream events at kernel boundaries: no kernel waits for another one, there is no flag, no spin
 * and no time-out on the device.  Per step t, in rank order, the host enqueues on the rank's stream: a wait for both neighbours'
 * push events of step t-1, the step kernel, the push, the record of this rank's push event of step t.  The price is a serial chain
 * kernel -> push -> neighbour's kernel per step: next to a rank kernel of hundreds of microseconds it is small, on a tiny grid it
 * is most of the step (DESIGN.md section 5 has the measured figures): this mode is for grids too large or too slow for one GPU.
 *
 * WHAT IS COMPUTED.  The populations are the bits lbm64_run gives on the whole grid, for EVERY rank count.  av_vels[t] is the sum
 * over the ranks, in rank order on the host, of each rank's sum of step t, times 1.0 / free_cells.  A rank's sum is formed as
 * lbm_d2q9_f64.h describes for lbm_step_kernel_f64 (per-lane sums, a fixed tree per block, block 0 of the next launch folds the
 * blocks' sums); adding the ranks' sums is one more serial level of that tree, nranks - 1 additions.  No atomics: the same state and
 * the same rank count give the same bits in every run.
 *
 * Conventions are those of lbm_d2q9.h: 0 on success, otherwise lbm_last_error() has the message for the calling thread; cells cross
 * the boundary as AoS, 9 doubles per cell of the WHOLE grid, row-major, x fastest; obstacles as the reference's int map of the whole
 * grid.  The host half of lbm_d2q9_f64.h (lbm64_read_params, lbm64_av_velocity_obs, lbm64_reynolds, the writers) serves these runs as
 * it is.
 *
 * SEVERAL STEPS PER EXCHANGE (LBM_ROWS64_FLAG_MULTI_STEPS, opt-in).  Where 32 x 16 tiles cover every rank exactly (nx % 32 == 0 and
 * every rank's rows a multiple of 16: ny % (16 * nranks) == 0) and the smallest rank owns at least LBM_TUNE_MULTI64_MIN cells, a rank
 * keeps K = LBM_TUNE_MULTI64_K (2..4, default 4) ghost rows on each side instead of one, advances up to K steps per launch of
 * lbm_rows_multi_kernel_f64<K, NT, FULL> (csrc/kernels/rows_multi64.h), the partition form of lbm_multi_kernel_f64 (lbm_d2q9_f64.h:
 * the same tile, LDS frame, sub-steps, cell update and sums), and exchanges once per launch: lbm64_push_ghost_rows_kernel stores all
 * nine planes of its first K owned rows into the upper ghost rows of the rank below and of its last K owned rows into the lower ghost
 * rows of the rank above.  A run of n steps is floor(n / K) launches of K steps and at most one shorter one, the last.  The ORDER is the
 * one above with "launch" for "step"; row ny-2 is now among the pushed rows (rank 0's lower ghost rows hold a copy of it, which the
 * kernel accelerates between its sub-steps as it does the owned one), so the accelerate pre-pass and a launch's accelerating epilogue
 * come before the push on the same stream.  The populations are the same bits.  av_vels[t]: per rank the tree lbm_d2q9_f64.h states
 * for lbm_multi_kernel_f64 over the rank's tiles (a lane's at most two owned cells of a sub-step, the wave's halving butterflies, one
 * lane over the eight waves, the fold over the tiles' sums by block 0 of the next launch or by the last fold of a run), then the
 * nranks - 1 host additions in rank order: the same bits in every run.  On any other run the flag changes nothing: the one-step kernel,
 * one ghost row, the same name from lbm_rows64_describe and the same av_vels bits as without it.
 *
 * ... ON RANKS OF ANY SIZE (LBM_ROWS64_FLAG_MULTI_ANY_SIZE, opt-in; alone, with a store form, or with LBM_ROWS64_FLAG_MULTI_STEPS, which
 * it means).  A run that 32 x 16 tiles cover on every rank runs precisely as under LBM_ROWS64_FLAG_MULTI_STEPS: the same kernel, name
 * and bits.  Any other run whose nx is even and >= 32, whose EVERY rank owns >= 16 rows (lbm_decompose; the ranks may be uneven) and
 * whose smallest rank owns at least LBM_TUNE_MULTI64_MIN cells advances up to K steps per launch and exchange too, with the EDGE-TILE
 * form of lbm_rows_multi_kernel_f64 (the edge-tile form of lbm_d2q9_f64.h on a rank's rows): rank r launches ceil(nx / 32) *
 * ceil(nyl / 16) tiles, nyl its own rows; a tile of its last column or row is shifted back inside the rank's owned rows, over its
 * neighbour, and owns — stores and counts — only the cells the neighbour does not.  K ghost rows, the exchange, the ORDER and the cut
 * of a run into launches are those above; the decision is one for all ranks.  The populations are the same bits.  av_vels[t]: per
 * rank the tree of lbm_multi_kernel_f64 over the rank's ceil(nx / 32) * ceil(nyl / 16) tiles (a shifted tile adds zeros for the cells
 * it does not own), then the nranks - 1 host additions in rank order.  On any other run (odd nx, nx < 32, a rank of fewer than 16 rows,
 * a smallest rank below the minimum) the flag changes nothing, as above.
 *
 * OUT OF SCOPE: tiles of a 2-D decomposition with more than one block in each direction (column blocks, for grids much wider than
 * tall, are lbm_d2q9_f64_cols.h, an object of its own); ranks in separate processes, over IPC or RCCL; more than one launch per exchange; odd nx
 * under either flag (such runs take the one-step kernel); overlap of a rank's interior rows or tiles with the exchange.
 * The whole grid's LBM64_FLAG_TILE_STEPS and LBM64_FLAG_MULTI_STEPS are refused, and so is its LBM64_FLAG_MULTI_ANY_SIZE: the row
 * partition's own bit for ranks that 32 x 16 tiles do not cover exactly is LBM_ROWS64_FLAG_MULTI_ANY_SIZE.
 */
#ifndef LBM_D2Q9_F64_ROWS_H
#define LBM_D2Q9_F64_ROWS_H

#include <stddef.h>

#include "lbm_d2q9_f64.h"           /* lbm64_params, LBM_FLAG_NT_STORES / LBM_FLAG_NO_NT_STORES, lbm_last_error */

#ifdef __cplusplus
extern "C" {
#endif

#define LBM_ROWS64_ABI_VERSION 1
#define LBM_ROWS64_MAX_RANKS 64     /* MPI_PROCS, d2q9-bgk.c:67 */
#define LBM_ROWS64_FLAG_MULTI_STEPS 2048u   /* K steps per launch and exchange on K ghost rows where every rank is eligible; else no effect */
#define LBM_ROWS64_FLAG_MULTI_ANY_SIZE 8192u   /* LBM_ROWS64_FLAG_MULTI_STEPS, and the same by the kernel's edge-tile form where nx is even and >= 32 and every rank owns >= 16 rows */

typedef struct lbm_rows64 lbm_rows64;   /* opaque: the device state of every rank of one run */

int lbm_rows64_abi_version(void);

/* A whole periodic nx x ny grid (ny >= 3) in the initial state of d2q9-bgk.c:880-902, its rows dealt to `nranks` ranks.
 * obstacles_all = ny*nx ints, the whole grid's map.  devices = nranks HIP ordinals, or NULL: rank r on device r % (device count).
 * Ranks may share a device.  flags: 0, LBM_FLAG_NT_STORES or LBM_FLAG_NO_NT_STORES (non-temporal stores of the output grid: by default
 * once a RANK's two grids exceed the Infinity Cache), each with or without LBM_ROWS64_FLAG_MULTI_STEPS and
 * LBM_ROWS64_FLAG_MULTI_ANY_SIZE (several steps per exchange, above; accepted, like the store forms, before the first HIP call).
 * Refused, with a message and before the first HIP call: nranks outside 1..LBM_ROWS64_MAX_RANKS; a decomposition that leaves a rank
 * without a row, or the last rank fewer than 3 (d2q9-bgk.c:848-849; ny = 5 on 3 ranks is 2, 1, 2); the shapes lbm64_create refuses;
 * free_cells < 1; any other flag — LBM64_FLAG_TILE_STEPS, LBM64_FLAG_MULTI_STEPS and LBM64_FLAG_MULTI_ANY_SIZE among them, with or without
 * the two flags above: they are the whole grid's.  Refused after it: two ranks on distinct devices that hipDeviceCanAccessPeer
 * denies. */
int lbm_rows64_create(lbm_rows64** run, const lbm64_params* params, int free_cells, const int* obstacles_all, int nranks,
                      const int* devices, unsigned flags);
int lbm_rows64_destroy(lbm_rows64* run);

/* n_steps iterations of d2q9-bgk.c:315-394 on every rank; av_vels[t] (may be NULL) as described above.  May be called repeatedly; the
 * state it leaves is the post-step state, NOT yet accelerated for a next step, exactly as lbm64_run.  Returns when every rank is
 * idle. */
int lbm_rows64_run(lbm_rows64* run, int n_steps, double* av_vels);

/* The state of the whole grid, AoS: ny*nx*9 doubles, gathered from / scattered to the ranks' owned rows in chunks of rows.  Bits
 * travel unchanged both ways (NaN payloads, signed zeros, denormals). */
int lbm_rows64_get_cells(lbm_rows64* run, double* cells_aos);
int lbm_rows64_set_cells(lbm_rows64* run, const double* cells_aos);

/* {u_x, u_y, u, pressure} per cell of the whole grid as lbm64_get_observables gives them: ny*nx*4 doubles. */
int lbm_rows64_get_observables(lbm_rows64* run, double* obs);

/* av_velocity()'s sum over the free cells (d2q9-bgk.c:716-751) of the current state: each rank sums its rows as
 * lbm64_av_velocity_sum does (per lane, per block), the host adds the blocks' sums, rank after rank. */
int lbm_rows64_av_velocity_sum(lbm_rows64* run, double* tot_u);

/* Device time of the last lbm_rows64_run: events around each rank's step and push launches, the largest span over the ranks; and
 * the number of step launches of the run (n_steps * nranks; under lbm_rows_multi_kernel_f64 ceil(n_steps / K) * nranks). */
int lbm_rows64_last_run_ms(lbm_rows64* run, double* ms, int* launches);

/* What a step looks like: the kernel's name ("lbm_rows_kernel_f64<2>", "lbm_rows_kernel_f64<1>", or with non-temporal stores
 * "lbm_rows_kernel_f64<2,nt>"), the rank count, and of the rank with the most work blocks: those blocks (one more block folds the
 * previous step's sums) and the cells a block advances; the bytes of all ranks' grids, ghost rows included.  Under
 * LBM_ROWS64_FLAG_MULTI_STEPS on an eligible run: "lbm_rows_multi_kernel_f64<K>" or "<K,nt>", the tiles of the rank with the most,
 * 512 cells, and 2 * 9 * 8 * nx * (ny + 2 * K * nranks) bytes.  Under LBM_ROWS64_FLAG_MULTI_ANY_SIZE on a run that takes the edge-tile
 * form: "lbm_rows_multi_kernel_f64<K,edge>" or "<K,nt,edge>" and the same three figures. */
int lbm_rows64_describe(const lbm_rows64* run, char* kernel_name, size_t len, int* nranks, long long* blocks, long long* cells_per_block,
                        long long* state_bytes);

#ifdef __cplusplus
}
#endif

#endif /* LBM_D2Q9_F64_ROWS_H */
