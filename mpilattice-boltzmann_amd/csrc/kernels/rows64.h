// rows64.h — row-partitioned runs of the double-precision mode: lbm_rows_kernel_f64<CELLS, NT>, the partition form of
// lbm_step_kernel_f64 (one step of one rank per launch), and lbm64_push_rows_kernel, which stores a rank's edge rows into its
// neighbours' ghost rows.  Part of the translation unit lbm_rows64.hip (device code of liblbm_d2q9.so, gfx950 only);
// include/lbm_d2q9_f64_rows.h states the contract.  From step64.h it takes pull_pair_f64, finish_cell_f64, the loads and stores and the
// small kernels as they are; from common.h kBlock and block_sum.
#pragma once
#include "step64.h"

namespace {

// Layout of a rank: nine planes of (nyl + 2) * nx doubles at plane stride `ps`, two grids swapped per step.  Owned row y (0 <= y < nyl)
// is storage row y + 1; storage rows 0 and nyl + 1 are the ghost rows, which the neighbours' pushes fill.  The obstacle bitfield covers
// the owned rows only: bit c of the owned-cell index c = y * nx + x.
struct RowsStep64Args {
  const double* src;           // source grid, plane 0 STORAGE row 0
  double* dst;                 // destination grid
  const uint32_t* mask;        // obstacle bitfield of the owned rows
  size_t ps;                   // plane stride in doubles (even)
  uint32_t nx;                 // row length
  uint32_t units;              // x-pairs (CELLS = 2) or cells (CELLS = 1) of the owned rows: nyl * nx cells
  int iters;                   // 256-unit chunks per block
  double omega;
  double accel_w1, accel_w2;   // d2q9-bgk.c:445-446 in double
  int accel_row;               // the OWNED-row index of row ny-2 of the grid on the rank that owns it while a step follows; else -1
  double* partials_out;        // this launch's per-block sums
  const double* prev_partials; // previous step's per-block sums, folded by block 0 of this launch
  int n_prev;
  double* sums;                // this rank's per-step totals of this run
  int* counter;                // index of the next entry of sums
};

// Rows that owned row y pulls from (d2q9-bgk.c:511-512 on a rank: no wrap, the halo rows are rows of the grid), as element offsets of
// their first cell in a plane.
__device__ __forceinline__ Rows64 rows_of_rank(uint32_t nx, uint32_t y)
{
  Rows64 r;
  r.south = static_cast<size_t>(y) * nx;
  r.here = r.south + nx;
  r.north = r.here + nx;
  return r;
}

// The x-pair form (nx even): step_pair_f64 on a rank's rows.
template <bool NT>
__device__ __forceinline__ double rows_pair_f64(const RowsStep64Args& a, uint32_t pair)
{
  const uint32_t c = pair * kPairCells;
  const uint32_t y = c / a.nx;
  const uint32_t x0 = c - y * a.nx;
  const size_t ps = a.ps;
  const Rows64 r = rows_of_rank(a.nx, y);
  d2 p[9];
  pull_pair_f64(a.src, ps, a.nx, r, x0, p);
  const uint32_t mbits = (a.mask[c >> 5] >> (c & 31u)) & 3u;   // c is even: both bits in one word
  const bool accel = static_cast<int>(y) == a.accel_row;
  d2 out[9];
  double acc = 0.0;
#pragma unroll
  for (int j = 0; j < kPairCells; ++j) {
    double t[9], q[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) t[k] = p[k][j];
    const double term = finish_cell_f64(t, (mbits >> j) & 1u, a.omega, accel, a.accel_w1, a.accel_w2, q);
#pragma unroll
    for (int k = 0; k < 9; ++k) out[k][j] = q[k];
    acc = j == 0 ? term : acc + term;
  }
  double* d = a.dst + r.here + x0;
#pragma unroll
  for (int k = 0; k < 9; ++k) store2<NT>(d + k * ps, out[k]);
  return acc;
}

// One cell per lane (odd nx): step_cell_f64 on a rank's rows.
template <bool NT>
__device__ __forceinline__ double rows_cell_f64(const RowsStep64Args& a, uint32_t cell)
{
  const uint32_t y = cell / a.nx;
  const uint32_t x = cell - y * a.nx;
  const size_t ps = a.ps;
  const Rows64 r = rows_of_rank(a.nx, y);
  const size_t xe = (x + 1 >= a.nx) ? 0 : x + 1;                       // :527-528
  const size_t xw = (x == 0) ? a.nx - 1 : x - 1;                       // :529
  const double* g = a.src;
  double t[9], out[9];
  t[0] = g[r.here + x];            t[1] = g[ps + r.here + xw];       t[2] = g[2 * ps + r.south + x];    // :530-532
  t[3] = g[3 * ps + r.here + xe];  t[4] = g[4 * ps + r.north + x];   t[5] = g[5 * ps + r.south + xw];   // :533-535
  t[6] = g[6 * ps + r.south + xe]; t[7] = g[7 * ps + r.north + xe];  t[8] = g[8 * ps + r.north + xw];   // :536-538
  const bool blocked = (a.mask[cell >> 5] >> (cell & 31u)) & 1u;
  const double term = finish_cell_f64(t, blocked, a.omega, static_cast<int>(y) == a.accel_row, a.accel_w1, a.accel_w2, out);
  double* d = a.dst + r.here + x;
#pragma unroll
  for (int k = 0; k < 9; ++k) store1<NT>(d + k * ps, out[k]);
  return term;
}

// fold_previous_f64 for a rank: block 0 folds the PREVIOUS step's per-block sums of this rank into its sums[counter++].
__device__ __forceinline__ void fold_previous_rows_f64(const RowsStep64Args& a, double* red)
{
  if (a.n_prev <= 0) return;
  double s = 0.0;
  for (int i = threadIdx.x; i < a.n_prev; i += kBlock) s += a.prev_partials[i];
  s = block_sum(s, red);
  if (threadIdx.x == 0) {
    const int t = *a.counter;
    a.sums[t] = s;
    *a.counter = t + 1;
  }
}

// One step of one rank, one definition for its four instantiations (kRows64Kernels, lbm_rows64.hip): the grid, the block shape and the
// lane summation of lbm_step_kernel_f64 — one fold block (block 0), then ceil(units / (256 * iters)) work blocks of 256 lanes; work
// block b owns `iters` consecutive 256-unit chunks; a lane adds its units' terms serially, block_sum joins the lanes in a fixed tree.
template <int CELLS, bool NT>
__global__ void __launch_bounds__(kBlock) lbm_rows_kernel_f64(const RowsStep64Args a)
{
  static_assert(CELLS == 1 || CELLS == kPairCells, "one cell or one x-pair per lane");
  __shared__ double red[kBlock / 64];
  if (blockIdx.x == 0) { fold_previous_rows_f64(a, red); return; }
  const uint32_t wblock = blockIdx.x - 1;   // work block index
  double acc = 0.0;
  const uint32_t base = wblock * static_cast<uint32_t>(a.iters) * kBlock + threadIdx.x;    // < units + 256 * iters < 2^31 + 2^18
  for (int i = 0; i < a.iters; ++i) {
    const uint32_t unit = base + static_cast<uint32_t>(i) * kBlock;
    if (unit < a.units) {
      if constexpr (CELLS == 1) acc += rows_cell_f64<NT>(a, unit);
      else acc += rows_pair_f64<NT>(a, unit);
    }
  }
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) a.partials_out[wblock] = acc;
}

// The exchange of one rank after its step: the populations that cross each cut, from the grid just written into the neighbours' ghost
// rows of THEIR grid of the same parity.  Southwards (d2q9-bgk.c:326-328's send to the rank below): populations 4, 7, 8 of the first
// owned row into the ghost row above the rank below (its storage row down_nyl + 1).  Northwards: populations 2, 5, 6 of the last owned
// row into the ghost row below the rank above (its storage row 0).  The other six planes of a ghost row are never read.  A neighbour's
// grid may be another device's memory (peer access): plain vector stores, 16 bytes each where nx is even (WIDE), else 8.
struct RowsPush64Args {
  const double* grid;          // this rank's grid just written, plane 0 storage row 0
  size_t ps;
  uint32_t nx, nyl;
  double* down;                // the rank below: the same grid of it, its plane stride and owned rows
  size_t down_ps;
  uint32_t down_nyl;
  double* up;                  // the rank above
  size_t up_ps;
};

template <bool WIDE>
__global__ void __launch_bounds__(kBlock) lbm64_push_rows_kernel(const RowsPush64Args a)
{
  constexpr uint32_t W = WIDE ? kPairCells : 1;
  const uint32_t per_row = a.nx / W;                                   // accesses per row of a plane
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;                // < 6 * per_row + 256
  if (i >= 6u * per_row) return;
  const uint32_t j = i / per_row;                                      // 0..2: southwards planes 4, 7, 8; 3..5: northwards planes 2, 5, 6
  const size_t x = static_cast<size_t>(i - j * per_row) * W;
  const bool north = j >= 3u;
  const uint32_t k = north ? (j == 3u ? 2u : j == 4u ? 5u : 6u) : (j == 0u ? 4u : j == 1u ? 7u : 8u);
  const size_t nx = a.nx;
  const double* from = a.grid + k * a.ps + (north ? static_cast<size_t>(a.nyl) * nx : nx) + x;
  double* to = north ? a.up + k * a.up_ps + x : a.down + k * a.down_ps + (static_cast<size_t>(a.down_nyl) + 1) * nx + x;
  if constexpr (WIDE) *reinterpret_cast<d2*>(to) = load2(from);
  else *to = *from;
}

}  // namespace
