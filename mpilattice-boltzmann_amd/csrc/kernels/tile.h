// tile.h — lbm_tile_kernel<T,H>: up to H steps per launch for the launch-latency-bound small grids
// Part of the single translation unit lbm_kernels.hip (device code of liblbm_d2q9.so, gfx950 only).
#pragma once
#include "common.h"

namespace {

// ------------------------------------------------------------------------------------------------
// Temporally blocked form for launch-latency-bound grids (the three small shipped decks).
//
// A step of a <= 64 K-cell grid takes less time to compute than a kernel boundary costs, so one
// launch here advances the lattice by up to H steps: a block loads an R x R region (R = T + 2H: a T x T
// owned tile + an H-cell ghost ring, periodic in x and y) into LDS, and sub-step s recomputes the
// region shrunk by s cells from the LDS copy of sub-step s-1 (two buffers, one barrier per sub-step).
// Ghost cells are computed redundantly by neighbouring blocks with the same arithmetic, so no block
// ever waits for another.  Per-step sum|u| is taken over owned cells only; accelerate_flow is applied
// to row ny-2 (ghost copies too) between sub-steps exactly as between launches of the one-step
// kernels.  Results are bit-identical to the one-step kernels (same relax_core, same order of steps).
//
// Work per sub-step is what bounds this kernel (one block = one CU: its 4 SIMDs issue every wave
// that holds a live lane), so the lanes are dealt anew in every sub-step: lane i takes the i-th
// x-pair of the CURRENT region (packed arithmetic: finish_pair), live lanes fill whole waves from
// wave 0 up, and the rest of the block skips the sub-step.  <16,8>: 39 wave-passes per 8 steps instead
// of 52 with a fixed lane -> cell assignment (and 104 with one cell per lane).  The region's left edge
// alternates between even and odd x, so LDS accesses are pairs of dwords rather than 8-byte words.
// What a lane needs to know about its cells it reads from a flag byte per region cell.
// ------------------------------------------------------------------------------------------------
// Geometry is a template parameter pair: T = owned tile edge, H = ghost ring = max steps per launch
// (both even); the block has R*R/2 lanes (the load phase: one aligned x-pair per lane).
constexpr int kMaxTileSteps = 8;

// Diagnostic builds only (scripts/build_variant.sh tile_stamps -DLBM_TILE_STAMPS=1, scripts/tile_stamps.py): shader-clock
// stamps of block 1, lane 0 at the phase boundaries of a launch.  No stamp executes in the product build.
#ifndef LBM_TILE_STAMPS
#define LBM_TILE_STAMPS 0
#endif
#ifndef LBM_TILE88_BLOCK
#define LBM_TILE88_BLOCK 512      // lanes of a <8,8> block: 320 would do for its 288 load-phase lanes (1.045 vs 1.009 us/step at 128 x 128; 448: 1.016)
#endif
#if LBM_TILE_STAMPS
__device__ unsigned long long g_tile_stamps[16];
#define LBM_STAMP(i) do { if (blockIdx.x == 1 && threadIdx.x == 0) g_tile_stamps[i] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define LBM_STAMP(i) do { } while (0)
#endif

template <int T, int H>
struct TileGeom {
  static constexpr int R = T + 2 * H;
  static constexpr int RP = R / 2;                  // aligned pairs per region row
  static constexpr int cells = R * R;
  // (a lane per region CELL, R*R lanes, so that every sub-step can deal one cell per lane, was measured and dropped:
  // 256x256 deck 0.142 -> 0.204 s, 128x128 0.0529 -> 0.0554 — sixteen-wave blocks pay more at the barriers than the
  // shorter chains of the early sub-steps save)
  static constexpr int lanes = RP * R;
  // launched size: whole waves, so that the wave-level sums see 64 active lanes; <8,8> gets 512 lanes rather than the
  // 320 its load phase needs, so that ALL its sub-steps (regions of 484 cells and less) deal one cell per lane.
  static constexpr int block = (T == 8 && H == 8 && LBM_TILE88_BLOCK > 64 * ((lanes + 63) / 64)) ? LBM_TILE88_BLOCK : 64 * ((lanes + 63) / 64);
  static constexpr int waves = block / 64;
  static constexpr size_t lds_bytes = sizeof(float) * 2 * 9 * cells + sizeof(double) * H * waves + cells;   // + flag bytes
  static_assert(lanes <= 1024 && H <= kMaxTileSteps && T % 2 == 0 && H % 2 == 0, "unsupported tile geometry");
};

struct TileArgs {
  const float* src;
  float* dst;
  const uint32_t* mask;
  size_t ps;
  int nx, ny;
  int tiles_x;                 // nx / T
  int ksteps;                  // 1..H steps in this launch
  int single_max;              // sub-steps whose region holds at most this many cells deal ONE cell per lane (0: always x-pairs)
  float omega, accel_w1, accel_w2;
  int accel_row;               // ny-2
  int accel_last;              // apply accelerate_flow after the LAST sub-step too (another step follows)
  double* partials_out;        // [ksteps][ntiles]
  const double* prev_partials; // previous launch: [n_prev_vecs][n_prev]
  int n_prev, n_prev_vecs;
  double* sums;
  int* counter;
};

// The kernel is defined from ONE text, kernels/tile_kernel_def.h, included once per arithmetic: lbm_tile_kernel<T, H, FULL, FAST> (the exact
// arithmetic: its source, and with it its code, is what it was before the fused form existed) and lbm_tile_kernel_fused<T, H, FULL>
// (LBM_FLAG_FUSED_ARITH: relax_core's fused sequence, double-precision sum|u| terms; not in the experiment build).
#define LBM_TILE_FUSED 0
#include "tile_kernel_def.h"
#undef LBM_TILE_FUSED
#if !LBM_EXPERIMENTS
#define LBM_TILE_FUSED 1
#include "tile_kernel_def.h"
#undef LBM_TILE_FUSED
#endif

}  // namespace
