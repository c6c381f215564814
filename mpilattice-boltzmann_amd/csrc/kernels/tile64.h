// tile64.h — lbm_tile_kernel_f64<T, H, FULL>: up to H steps per launch of the double-precision mode, for the small whole grids whose
// one-step launches are bound by the kernel boundary.  Part of the translation unit lbm_f64.hip (gfx950 only, -ffp-contract=off).
//
// lbm_tile_kernel's scheme (kernels/tile.h) with every float object a double.  A block owns a T x T tile and loads the R x R region
// around it, R = T + 2H, periodic in x and in y, into LDS; a grid smaller than the region simply appears in it several times (8 x 8
// under <8,8>: three times each way).  Sub-step s of k recomputes the owned tile grown by k - s cells from the LDS copy sub-step
// s - 1 left (two buffers, one barrier per sub-step); ghost cells are recomputed by the neighbouring blocks with the same
// arithmetic, so no block waits for another.  The cell update is finish_cell_f64 of step64.h, called as it is: the bits do not
// depend on the kernel, the geometry, the cut of a run into launches or the lane that computed a cell.
//
// accelerate_flow between sub-steps is finish_cell_f64's `accel` on every region copy of row ny-2 (flag bit 2), ghost copies
// included, and after the last sub-step exactly when another step of the run follows (accel_last), as accel_row of the one-step launch.
//
// Lanes: there is no packed double arithmetic, so a lane takes ONE cell and the cells of the current region are dealt anew in every
// sub-step, cell i to lane i % block: live lanes fill whole waves from wave 0 up, the rest of the block goes to the barrier.
//
// sum|u|: a term counts for owned, unblocked cells only; a lane keeps one accumulator per sub-step (a lane meets at most one owned
// cell per pass), the wave's halving butterflies (common.h wave_sum_vec4 / wave_sum_vec8) join the lanes, one lane per sub-step adds
// the waves' sums serially and writes partials_out[step][tile].  Block 0 does no lattice work: it folds the PREVIOUS launch's vectors
// into sums[counter ...].  No atomics anywhere: the order of additions is fixed (include/lbm_d2q9_f64.h states the tree).
#pragma once
#include "step64.h"

namespace {

struct Tile64Args {
  const double* src;
  double* dst;
  const uint32_t* mask;
  size_t ps;
  int nx, ny;
  int tiles_x;                 // nx / T
  int ksteps;                  // 1..H steps in this launch (FULL: H)
  double omega, accel_w1, accel_w2;
  int accel_row;               // ny-2
  int accel_last;              // apply accelerate_flow after the LAST sub-step too (another step follows)
  double* partials_out;        // [ksteps][tiles]
  const double* prev_partials; // previous launch: [n_prev_vecs][n_prev]
  int n_prev, n_prev_vecs;
  double* sums;
  int* counter;
};

// FULL: the launch makes exactly H steps, so every region size is a compile-time constant.
template <int T, int H, bool FULL>
__global__ void __launch_bounds__(tile64_block(T, H)) lbm_tile_kernel_f64(const Tile64Args a)
{
  static_assert(tile64_geom_ok(T, H), "unsupported tile geometry");
  constexpr int R = tile64_region(T, H), RP = R / 2, kCells = R * R, kLanes = tile64_block(T, H), kWaves = kLanes / 64;
  extern __shared__ __attribute__((aligned(16))) double lds64[];     // [2][9][R*R] doubles, reduction scratch, flag bytes
  double* red = lds64 + 2 * 9 * kCells;                               // [H][kWaves]
  uint8_t* cell_flags = reinterpret_cast<uint8_t*>(red + H * kWaves);  // per region cell: bit 0 obstacle, 1 owned, 2 on row ny-2
  const int tid = threadIdx.x;

  if (blockIdx.x == 0) {
    // fold block: the previous launch's per-tile sums, one vector per step, into sums[counter ...]
    const int first = tid == 0 ? *a.counter : 0;                      // lane 0 alone reads and writes it
    for (int v = 0; v < a.n_prev_vecs; ++v) {
      double s = 0.0;
      for (int i = tid; i < a.n_prev; i += kLanes) s += a.prev_partials[static_cast<size_t>(v) * a.n_prev + i];
      s = wave_sum(s);
      lds_barrier();
      if ((tid & 63) == 0) red[tid >> 6] = s;
      lds_barrier();
      if (tid == 0) {
        double t = red[0];
        for (int w = 1; w < kWaves; ++w) t += red[w];
        a.sums[first + v] = t;
      }
    }
    if (tid == 0 && a.n_prev_vecs > 0) *a.counter = first + a.n_prev_vecs;
    return;
  }

  const int tile = blockIdx.x - 1;
  const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;

  // ---- load: an aligned x-pair of the region per lane and pass, periodic (d2q9-bgk.c:527-529 in x, :511-512 in y).  nx, T and H are
  // even, so a pair never straddles the wrap and its first cell has an even index: 16-byte loads, both obstacle bits in one word.
  for (int i = tid; i < RP * R; i += kLanes) {
    const int ry = i / RP, rx = 2 * (i - ry * RP);
    int gx = (tx * T - H + rx) % a.nx; if (gx < 0) gx += a.nx;
    int gy = (ty * T - H + ry) % a.ny; if (gy < 0) gy += a.ny;
    const uint32_t cell = static_cast<uint32_t>(gy) * static_cast<uint32_t>(a.nx) + static_cast<uint32_t>(gx);
    const uint32_t mbits = (a.mask[cell >> 5] >> (cell & 31u)) & 3u;
    const uint32_t common = ((rx >= H && rx < H + T && ry >= H && ry < H + T) ? 2u : 0u) | (gy == a.accel_row ? 4u : 0u);
    const int c = ry * R + rx;
#pragma unroll
    for (int k = 0; k < 9; ++k) *reinterpret_cast<d2*>(lds64 + k * kCells + c) = load2(a.src + k * a.ps + cell);
    *reinterpret_cast<uint16_t*>(cell_flags + c) = static_cast<uint16_t>(((mbits & 1u) | common) | ((((mbits >> 1) & 1u) | common) << 8));
  }
  lds_barrier();

  double acc[H];
#pragma unroll
  for (int i = 0; i < H; ++i) acc[i] = 0.0;

  const int k_total = FULL ? H : a.ksteps;
  // One sub-step; S is a compile-time constant (the sub-steps are unrolled: buffer roles and the accumulator slot fold).
  auto substep = [&](auto sc) __attribute__((always_inline)) {
    constexpr int S = decltype(sc)::value;
    const double* bufA = lds64 + ((S & 1) ? 0 : 9 * kCells);
    double* bufB = lds64 + ((S & 1) ? 9 * kCells : 0);
    const int e = k_total - S;                   // cells still needed after this sub-step: the owned tile grown by e
    const int side = T + 2 * e;
    const bool last = S == k_total;
    const bool accel_now = !last || a.accel_last;
    for (int i = tid; i < side * side; i += kLanes) {
      const int ry = FULL ? i / side : small_div(i, side), rx = i - ry * side;
      const int c = (H - e + ry) * R + (H - e + rx);
      const uint32_t fl = cell_flags[c];
      double t[9], out[9];                                                           // d2q9-bgk.c:530-538
      t[0] = bufA[0 * kCells + c];         t[1] = bufA[1 * kCells + c - 1];     t[2] = bufA[2 * kCells + c - R];
      t[3] = bufA[3 * kCells + c + 1];     t[4] = bufA[4 * kCells + c + R];     t[5] = bufA[5 * kCells + c - R - 1];
      t[6] = bufA[6 * kCells + c - R + 1]; t[7] = bufA[7 * kCells + c + R + 1]; t[8] = bufA[8 * kCells + c + R - 1];
      const double term = finish_cell_f64(t, (fl & 1u) != 0u, a.omega, accel_now && (fl & 4u) != 0u, a.accel_w1, a.accel_w2, out);
      acc[S - 1] += (fl & 2u) ? term : 0.0;                                          // owned cells only (:667); a blocked cell's term is 0
      if (!last) {
#pragma unroll
        for (int k = 0; k < 9; ++k) bufB[k * kCells + c] = out[k];
      } else {
        // last sub-step: the region is the owned tile, inside the grid
        const size_t cell = static_cast<size_t>(ty * T + ry) * a.nx + tx * T + rx;
#pragma unroll
        for (int k = 0; k < 9; ++k) a.dst[k * a.ps + cell] = out[k];
      }
    }
    if (!last) lds_barrier();
  };
  if (1 <= k_total) substep(std::integral_constant<int, 1>{});
  if (2 <= k_total) substep(std::integral_constant<int, 2>{});
  if (3 <= k_total) substep(std::integral_constant<int, 3>{});
  if (4 <= k_total) substep(std::integral_constant<int, 4>{});
  if constexpr (H >= 8) {
    if (5 <= k_total) substep(std::integral_constant<int, 5>{});
    if (6 <= k_total) substep(std::integral_constant<int, 6>{});
    if (7 <= k_total) substep(std::integral_constant<int, 7>{});
    if (8 <= k_total) substep(std::integral_constant<int, 8>{});
  }

  // per-step sums over the owned cells of this tile: one halving butterfly per wave (common.h), then one lane per step over the waves
  const int ntiles = gridDim.x - 1;
  if constexpr (H == 8) {
    const double w = wave_sum_vec8(acc);
    if ((tid & 7) == 0) red[wave_sum_slot<8>(tid & 63) * kWaves + (tid >> 6)] = w;
  } else {
    const double w = wave_sum_vec4(acc[0], acc[1], acc[2], acc[3]);
    if ((tid & 15) == 0) red[wave_sum_slot<4>(tid & 63) * kWaves + (tid >> 6)] = w;
  }
  lds_barrier();                 // LDS only: no wait for the tile's global stores
  if (tid < k_total) {
    double t = red[tid * kWaves];
    for (int w = 1; w < kWaves; ++w) t += red[tid * kWaves + w];
    a.partials_out[static_cast<size_t>(tid) * ntiles + tile] = t;
  }
}

}  // namespace
