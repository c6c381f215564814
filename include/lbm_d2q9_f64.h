/*
 * lbm_d2q9_f64.h — C ABI of the DOUBLE-PRECISION mode of the D2Q9-BGK timestep path (liblbm_d2q9.so, csrc/lbm_f64.hip).
 *
 * The reference's shipped results (the files under check/, the Reynolds numbers of its README) came from the double-precision original of
 * its code; its float path, which include/lbm_d2q9.h reproduces bit for bit, sits 0.08 - 0.24 % away from them.  This mode is the
 * reference's arithmetic with every float object a double: the EXACT, non-fused cell update in the reference's operation order
 * (kernels/common.h relax_core; d2q9-bgk.c:546-666), the initial state (:880-902), accelerate_flow (:442-478), av_velocity
 * (:716-753), calc_reynolds (:1005-1007) and the write_values arithmetic (:1076-1111), where
 *   - every float literal is the same decimal literal read as a double, sqrtf is sqrt;
 *   - free_cells_inv is 1.0 / free_cells; density, accel and omega are parsed as doubles (%lf);
 *   - nothing is contracted (-ffp-contract=off, no fast-math); division and square root are correctly rounded;
 *   - av_vels[t] = (sum over the free cells of sqrt(msq) * rinv, in double) * free_cells_inv.  Only the ORDER of that sum differs
 *     from a serial loop's (per-lane partial sums, a fixed tree per block, block 0 of the next launch folds the blocks' sums).
 *     With LBM64_FLAG_TILE_STEPS on an eligible grid (lbm_tile_kernel_f64<T, H>, blocks of B = 256 lanes for <8, 4> and 512 otherwise)
 *     the tree of one entry is: a lane adds the terms of the owned cells it meets in that sub-step (one per pass: 1 addition, 2 where
 *     the sub-step's region has more than B cells), six butterfly levels join the 64 lanes of a wave, one lane adds the B / 64 waves'
 *     sums serially: the tile's sum.  The fold then adds the tiles' sums: a lane ceil(tiles / F) of them serially, six butterfly
 *     levels, F / 64 waves' sums serially, where F = B in block 0 of the next launch and F = 256 in the last fold of a run.
 *     With LBM64_FLAG_MULTI_STEPS on an eligible grid (lbm_multi_kernel_f64<K>, 32 x 16 tiles, blocks of 512 lanes) the tree of one
 *     entry is: a lane adds the terms of the owned cells it meets in that sub-step (at most two — the x-pair it pulls in the first
 *     sub-step of a launch, the two cells it is dealt where a sub-step's region has more than 512 — so 2 additions), six butterfly
 *     levels join the 64 lanes of a wave, one lane adds the eight waves' sums serially (7 additions): the tile's sum.  The fold then adds
 *     the tiles' sums exactly as above: a lane ceil(tiles / F) of them serially, six butterfly levels, F / 64 waves' sums serially,
 *     where F = 512 in block 0 of the next launch and F = 256 in the last fold of a run.
 *     No atomics: the same state, grid and geometry give the same bits in every run.
 * tests/f64_ref.c restates it on a CPU; DESIGN.md section 5 gives the measured distances to the reference's shipped results.
 *
 * Conventions are those of lbm_d2q9.h: 0 on success, otherwise lbm_last_error() has the message for the calling thread; cells cross
 * the boundary as AoS, 9 doubles per cell, row-major, x fastest; obstacles as the reference's int map.  lbm_read_obstacles and
 * lbm_last_error of lbm_d2q9.h serve this mode as they are.
 *
 * OUT OF SCOPE of this mode (use lbm_d2q9.h; for row blocks in double precision inside one process, lbm_d2q9_f64_rows.h; for column
 * blocks, lbm_d2q9_f64_cols.h): row or tile
 * partitions and every halo transport (peer-to-peer, RCCL, split-phase calls)
 * — a context is a whole periodic grid on one GPU (several steps per launch are opt-in: LBM64_FLAG_TILE_STEPS for small grids,
 * LBM64_FLAG_MULTI_STEPS for large ones that 32 x 16 tiles cover, LBM64_FLAG_MULTI_ANY_SIZE for large ones of any even width; without
 * them, and on every grid they do not take, every step is one launch of lbm_step_kernel_f64); the
 * fused arithmetic (LBM_FLAG_FUSED_ARITH); hipGraph replay (LBM_FLAG_GRAPH).  The state digest of doubles, lbm_state_checksum's
 * counterpart, is lbm_digest64_grid of lbm_d2q9_f64_digest.h: one digest per row, under names of its own.
 */
#ifndef LBM_D2Q9_F64_H
#define LBM_D2Q9_F64_H

#include <stddef.h>

#include "lbm_d2q9.h"               /* LBM_NSPEEDS, LBM_FLAG_NT_STORES / LBM_FLAG_NO_NT_STORES, lbm_read_obstacles, lbm_last_error */

#ifdef __cplusplus
extern "C" {
#endif

#define LBM64_ABI_VERSION 1

/* lbm64_create flag, beside LBM_FLAG_NT_STORES / LBM_FLAG_NO_NT_STORES: advance a small whole grid several steps per launch with the
 * temporally blocked kernel lbm_tile_kernel_f64<T, H> (T x T tiles, up to H steps per launch; csrc/kernels/tile64.h).  Taken where
 * nx and ny are multiples of T and nx * ny is at most LBM_TUNE_TILE64_MAX (scripts/README.md; by default 1024 x 1024 cells);
 * every other grid runs lbm_step_kernel_f64 exactly as without the flag.  Populations are the same bits either way; av_vels differs in
 * the order of its additions only (above).  lbm_create of lbm_d2q9.h ignores this bit. */
#define LBM64_FLAG_TILE_STEPS 512u

/* lbm64_create flag, alone or with the flags above: advance a large whole grid several steps per launch with lbm_multi_kernel_f64<K>
 * (32 x 16 tiles, an in-place LDS frame, K steps per launch; csrc/kernels/multi64.h).  Taken where nx is a multiple of 32, ny a
 * multiple of 16, nx * ny is at least LBM_TUNE_MULTI64_MIN and LBM64_FLAG_TILE_STEPS does not take the grid for the tiled kernel;
 * K is LBM_TUNE_MULTI64_K (scripts/README.md has both knobs and their measured defaults).  Every other grid runs exactly as without
 * this flag.  A run of n steps is floor(n / K) launches of K steps and at most one shorter launch, the last.  Populations are the
 * same bits either way; av_vels differs in the order of its additions only (above).  lbm_create of lbm_d2q9.h ignores this bit. */
#define LBM64_FLAG_MULTI_STEPS 1024u

/* lbm64_create flag, wherever LBM64_FLAG_MULTI_STEPS is taken (alone, with a store form, with the two flags above): it means
 * LBM64_FLAG_MULTI_STEPS, and takes the large grids that 32 x 16 tiles do NOT cover exactly as well.  A grid the tiles cover runs
 * precisely as under LBM64_FLAG_MULTI_STEPS (the same kernel, name and av_vels bits).  Any other grid with nx even and >= 32, ny >= 16
 * and at least LBM_TUNE_MULTI64_MIN cells, which the tiled kernel does not take, advances K steps per launch with the EDGE-TILE form of
 * lbm_multi_kernel_f64: ceil(nx / 32) x ceil(ny / 16) tiles, tile (tx, ty) starting at x0 = min(32 tx, nx - 32), y0 = min(16 ty,
 * ny - 16) — a tile that would hang over the edge is shifted back inside the grid, over its neighbour — and OWNING (storing, and
 * counting in the sums) only its cells at tile-local x >= 32 tx - x0 and y >= 16 ty - y0: every cell of the grid has exactly one
 * owner.  The frame, the sub-steps, the cell update and the recomputed ring are the kernel's as they are.  The av_vels tree is the
 * one stated above for lbm_multi_kernel_f64, over the ceil(nx / 32) * ceil(ny / 16) tiles.  Odd nx, nx < 32 and ny < 16 run
 * lbm_step_kernel_f64 exactly as without the flag.  Populations are the same bits either way.  Row partitions (lbm_d2q9_f64_rows.h)
 * refuse this bit (their own, for ranks the tiles do not cover, is LBM_ROWS64_FLAG_MULTI_ANY_SIZE there); lbm_create of lbm_d2q9.h
 * ignores it. */
#define LBM64_FLAG_MULTI_ANY_SIZE 4096u

/* t_param (d2q9-bgk.c:79-90) with its three floats as doubles. */
typedef struct lbm64_params {
  int nx, ny;
  int max_iters;
  int reynolds_dim;
  double density, accel, omega;
} lbm64_params;

typedef struct lbm64_ctx lbm64_ctx;   /* opaque: device state of one whole grid */

int lbm64_abi_version(void);

/* ---- host side (no GPU needed) ------------------------------------------------------------------------------------------- */

/* d2q9-bgk.c:772-803 with %lf for density, accel and omega: "0.1" becomes the double 0.1, not (double)0.1f.  On failure the message
 * is the reference's die() text ("could not read param file: nx", ...). */
int lbm64_read_params(const char* paramfile, lbm64_params* out);

/* av_velocity()'s sum (d2q9-bgk.c:716-751) from lbm64_get_observables output: the sum over the free cells, in the reference's cell
 * order, of sqrt(u_x * u_x + u_y * u_y), a double accumulator.  Multiply by 1.0 / free_cells for the average (:753). */
double lbm64_av_velocity_obs(const lbm64_params* p, const double* obs, const int* obstacles, int rows);

/* calc_reynolds (d2q9-bgk.c:1005-1007): av_velocity * reynolds_dim / (1.0 / 6.0 * (2.0 / omega - 1.0)). */
double lbm64_reynolds(const lbm64_params* p, double av_velocity);

/* write_values (d2q9-bgk.c:1054-1120) from lbm64_get_observables output, "%d %d %.12E %.12E %.12E %.12E %d\n" per cell; an obstacle
 * cell prints 0, 0, 0 and density * (1.0 / 3.0).  Same bytes as fprintf gives. */
int lbm64_write_final_state_obs(const char* path, const lbm64_params* p, const double* obs, const int* obstacles, int rows, int displ, int append);

/* d2q9-bgk.c:1127-1139: "%d:\t%.12E\n" per step. */
int lbm64_write_av_vels(const char* path, const double* av_vels, int n);

/* ---- device state ---------------------------------------------------------------------------------------------------------- */

/* A whole periodic nx x ny grid (ny >= 3) on GPU `device`, in the initial state of d2q9-bgk.c:880-902.  obstacles = ny*nx ints.
 * flags: 0, LBM_FLAG_NT_STORES or LBM_FLAG_NO_NT_STORES (non-temporal stores of the output grid: by default once the two grids
 * exceed the Infinity Cache), each with or without LBM64_FLAG_TILE_STEPS and LBM64_FLAG_MULTI_STEPS (with both, the tiled kernel where
 * it takes the grid, otherwise lbm_multi_kernel_f64 where that does) and LBM64_FLAG_MULTI_ANY_SIZE (LBM64_FLAG_MULTI_STEPS, and its
 * edge-tile form where the tiles do not cover the grid); any other flag is refused. */
int lbm64_create(lbm64_ctx** ctx, const lbm64_params* params, int free_cells, const int* obstacles, int device, unsigned flags);
int lbm64_destroy(lbm64_ctx* ctx);

/* n_steps iterations of d2q9-bgk.c:315-394 (accelerate_flow, then the step); av_vels[t] (may be NULL) as described above.  May be
 * called repeatedly; the state it leaves is the post-step state, NOT yet accelerated for a next step, exactly as lbm_run. */
int lbm64_run(lbm64_ctx* ctx, int n_steps, double* av_vels);

/* The state, AoS: ny*nx*9 doubles.  Bits travel unchanged both ways (NaN payloads, signed zeros, denormals). */
int lbm64_get_cells(lbm64_ctx* ctx, double* cells_aos);
int lbm64_set_cells(lbm64_ctx* ctx, const double* cells_aos);

/* {u_x, u_y, u, pressure} per cell as write_values computes them for a FLUID cell (d2q9-bgk.c:1084-1111): ny*nx*4 doubles, computed
 * on the device, copied in chunks of rows (no second copy of the state). */
int lbm64_get_observables(lbm64_ctx* ctx, double* obs);

/* av_velocity()'s sum over the free cells (d2q9-bgk.c:716-751) of the current state, summed on the device (order: per lane, per
 * block, then the blocks' sums on the host). */
int lbm64_av_velocity_sum(lbm64_ctx* ctx, double* tot_u);

/* Device time of the step launches of the last lbm64_run (events around them), and their number (tiled and multi-step kernels:
 * launches, not steps — ceil(n / K) for lbm_multi_kernel_f64<K>). */
int lbm64_last_run_kernel_ms(lbm64_ctx* ctx, double* ms, int* launches);

/* What a step launch looks like: the kernel's name, its work blocks (one more block folds the previous step's sums), the cells
 * a block advances (256 lanes x cells per lane x units per lane) and the bytes of the two grids.  A context that
 * LBM64_FLAG_TILE_STEPS advances with the tiled kernel: "lbm_tile_kernel_f64<T, H>", the tiles, T * T.  One that LBM64_FLAG_MULTI_STEPS
 * advances with the multi-step kernel: "lbm_multi_kernel_f64<K>" ("lbm_multi_kernel_f64<K,nt>" with non-temporal stores), the tiles,
 * 32 * 16.  One that LBM64_FLAG_MULTI_ANY_SIZE advances with the edge-tile form: "lbm_multi_kernel_f64<K,edge>" ("<K,nt,edge>"),
 * ceil(nx / 32) * ceil(ny / 16), 512 (the cells a block computes in its last sub-step; it owns fewer where it is shifted). */
int lbm64_describe(const lbm64_ctx* ctx, char* kernel_name, size_t len, long long* blocks, long long* cells_per_block, long long* state_bytes);

#ifdef __cplusplus
}
#endif

#endif /* LBM_D2Q9_F64_H */
