// step.h — one step per launch: lbm_step_kernel<CELLS, NT, FUSED> (4 cells per lane, or 1: the narrow form)
// Part of the single translation unit lbm_kernels.hip (device code of liblbm_d2q9.so, gfx950 only).
#pragma once
#include "common.h"

namespace {

// Everything after the pull for the 4 cells at (y, x0..x0+3), partition-local cell index c:
// relaxation / bounce-back select, next step's accelerate_flow on row ny-2, stores, outgoing halo
// rows.  p[k] = streamed-in population k of the four cells.  Returns their sum|u| contribution.
template <bool NT, bool FUSED = false>
__device__ __forceinline__ double finish_quad(const StepArgs& a, int c, int y, int x0, const f4 (&p)[9], uint32_t mbits)
{
  const size_t ps = a.ps;
  f4 out[9];
  double acc = 0.0;
#pragma unroll
  for (int j = 0; j < kCellsPerLane; ++j) {
    float t[9], o[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) t[k] = p[k][j];
    const double term = relax_cell<FUSED>(t, a.omega, o);
    const bool blocked = (mbits >> j) & 1u;
    // bounce-back (d2q9-bgk.c:687-695): out[opposite(k)] = t[k]
    out[0][j] = blocked ? t[0] : o[0];
    out[1][j] = blocked ? t[3] : o[1];
    out[2][j] = blocked ? t[4] : o[2];
    out[3][j] = blocked ? t[1] : o[3];
    out[4][j] = blocked ? t[2] : o[4];
    out[5][j] = blocked ? t[7] : o[5];
    out[6][j] = blocked ? t[8] : o[6];
    out[7][j] = blocked ? t[5] : o[7];
    out[8][j] = blocked ? t[6] : o[8];
    acc += blocked ? 0.0 : term;
  }

  // accelerate_flow for the NEXT step, applied to the freshly written row ny-2 (d2q9-bgk.c:457-469)
  if (y == a.accel_row) {
#pragma unroll
    for (int j = 0; j < kCellsPerLane; ++j) {
      const bool blocked = (mbits >> j) & 1u;
      if (!blocked && out[3][j] - a.accel_w1 > 0.0f && out[6][j] - a.accel_w2 > 0.0f &&
          out[7][j] - a.accel_w2 > 0.0f) {
        out[1][j] += a.accel_w1; out[5][j] += a.accel_w2; out[8][j] += a.accel_w2;
        out[3][j] -= a.accel_w1; out[6][j] -= a.accel_w2; out[7][j] -= a.accel_w2;
      }
    }
  }

  float* d = a.dst + c;
#pragma unroll
  for (int k = 0; k < 9; ++k) store4<NT>(d + k * ps, out[k]);

  // next step's outgoing halo rows (row-partitioned runs only)
  if (a.send_south != nullptr && y == 0) {
    float* s = a.send_south + kHaloGuard + x0;
    store4<false>(s, out[4]); store4<false>(s + a.nxp, out[7]); store4<false>(s + 2 * a.nxp, out[8]);
  }
  if (a.send_north != nullptr && y == a.nyl - 1) {
    float* s = a.send_north + kHaloGuard + x0;
    store4<false>(s, out[2]); store4<false>(s + a.nxp, out[5]); store4<false>(s + 2 * a.nxp, out[6]);
  }
  return acc;
}

// Direct-load form: processes the 4 cells starting at partition-local cell index 4*quad
// (nx % 4 == 0, so the four share a row).
template <bool NT, bool FUSED = false>
__device__ __forceinline__ double step_quad(const StepArgs& a, int quad)
{
  const int c = quad * kCellsPerLane;
  const int y = c / a.nx;
  const int x0 = c - y * a.nx;
  const size_t ps = a.ps;
  const int nx = a.nx;
  const RowPtrs r = source_rows(a, y);

  // pull (d2q9-bgk.c:530-538): aligned for x, dword-shifted for x-1 / x+1
  f4 p[9];
  p[0] = load4(r.here + x0);
  p[2] = load4(r.s2 + x0);
  p[4] = load4(r.n4 + x0);
  p[1] = load4u(r.here + ps + x0 - 1);
  p[5] = load4u(r.s5 + x0 - 1);
  p[8] = load4u(r.n8 + x0 - 1);
  p[3] = load4u(r.here + 3 * ps + x0 + 1);
  p[6] = load4u(r.s6 + x0 + 1);
  p[7] = load4u(r.n7 + x0 + 1);
  const uint32_t mword = a.mask[c >> 5];
  if (x0 == 0) {                       // x_w wraps to nx-1 (:529)
    p[1].x = r.here[ps + nx - 1];
    p[5].x = r.s5[nx - 1];
    p[8].x = r.n8[nx - 1];
  }
  if (x0 == nx - kCellsPerLane) {      // x_e wraps to 0 (:527-528)
    p[3].w = r.here[3 * ps];
    p[6].w = r.s6[0];
    p[7].w = r.n7[0];
  }
  const uint32_t mbits = (mword >> (c & 31)) & 0xFu;
  return finish_quad<NT, FUSED>(a, c, y, x0, p, mbits);
}

// One-cell-per-lane form: used for grids so small that a step is bound by the latency of one lane's
// dependent instruction chain rather than by bandwidth (4x more lanes, each with a quarter of the
// chain), and for row lengths that are not a multiple of 4.  `cell` = partition-local cell index.
template <bool NT, bool FUSED = false>
__device__ __forceinline__ double step_cell(const StepArgs& a, int cell)
{
  const int y = cell / a.nx;
  const int x = cell - y * a.nx;
  const size_t ps = a.ps;
  const int nx = a.nx;
  const RowPtrs r = source_rows(a, y);
  const int xe = (x + 1 >= nx) ? x + 1 - nx : x + 1;                   // :527-528
  const int xw = (x == 0) ? nx - 1 : x - 1;                             // :529
  float t[9], o[9];
  t[0] = r.here[x];            t[1] = r.here[ps + xw];      t[2] = r.s2[x];      // :530-532
  t[3] = r.here[3 * ps + xe];  t[4] = r.n4[x];              t[5] = r.s5[xw];     // :533-535
  t[6] = r.s6[xe];             t[7] = r.n7[xe];             t[8] = r.n8[xw];     // :536-538
  const bool blocked = (a.mask[cell >> 5] >> (cell & 31)) & 1u;
  const double term = relax_cell<FUSED>(t, a.omega, o);
  float out[9];
  out[0] = blocked ? t[0] : o[0];                                       // bounce-back :687-695
  out[1] = blocked ? t[3] : o[1];
  out[2] = blocked ? t[4] : o[2];
  out[3] = blocked ? t[1] : o[3];
  out[4] = blocked ? t[2] : o[4];
  out[5] = blocked ? t[7] : o[5];
  out[6] = blocked ? t[8] : o[6];
  out[7] = blocked ? t[5] : o[7];
  out[8] = blocked ? t[6] : o[8];
  if (y == a.accel_row && !blocked && out[3] - a.accel_w1 > 0.0f && out[6] - a.accel_w2 > 0.0f &&
      out[7] - a.accel_w2 > 0.0f) {                                     // next step's accelerate_flow :457-469
    out[1] += a.accel_w1; out[5] += a.accel_w2; out[8] += a.accel_w2;
    out[3] -= a.accel_w1; out[6] -= a.accel_w2; out[7] -= a.accel_w2;
  }
  float* d = a.dst + cell;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    if (NT) __builtin_nontemporal_store(out[k], d + k * ps);
    else d[k * ps] = out[k];
  }
  if (a.send_south != nullptr && y == 0) {
    float* s = a.send_south + kHaloGuard + x;
    s[0] = out[4]; s[a.nxp] = out[7]; s[2 * a.nxp] = out[8];
  }
  if (a.send_north != nullptr && y == a.nyl - 1) {
    float* s = a.send_north + kHaloGuard + x;
    s[0] = out[2]; s[a.nxp] = out[5]; s[2 * a.nxp] = out[6];
  }
  return blocked ? 0.0 : term;
}

// The one-step kernel, one definition for every instantiation (the host's kStepKernels table, lbm_kernels.hip): CELLS = cells per lane
// (kCellsPerLane: step_quad; 1: step_cell — the unit ranges of StepArgs are then cell ranges), NT = non-temporal stores, FUSED =
// LBM_FLAG_FUSED_ARITH.  lbm_describe still names the families lbm_step_kernel / lbm_step_kernel_narrow and *_fused.  That this text
// compiles to the code the per-family definitions gave is recorded in profiles/r06/isa_identity.txt.
// Grid: ceil(#units / (256*iters)) work blocks of 256 lanes (block b owns `iters` consecutive 256-unit chunks) after one fold
// block (block 0, dispatched first).
template <int CELLS, bool NT, bool FUSED>
__global__ void __launch_bounds__(kBlock) lbm_step_kernel(const StepArgs a)
{
  static_assert(CELLS == 1 || CELLS == kCellsPerLane, "one cell or one quad per lane");
  __shared__ double red[kBlock / 64];
  if (blockIdx.x == 0) { fold_previous(a, red); return; }
  const int wblock = blockIdx.x - 1;   // work block index
  double acc = 0.0;
  const int n1 = a.quad_end - a.quad_begin;
  const int n2 = a.quad_end2 > a.quad_begin2 ? a.quad_end2 - a.quad_begin2 : 0;
  const int base = wblock * a.iters * kBlock + threadIdx.x;
  for (int i = 0; i < a.iters; ++i) {
    const int r = base + i * kBlock;
    if (r < n1 + n2) {
      const int unit = r < n1 ? a.quad_begin + r : a.quad_begin2 + (r - n1);
      if constexpr (CELLS == 1) acc += step_cell<NT, FUSED>(a, unit);
      else acc += step_quad<NT, FUSED>(a, unit);
    }
  }
  acc = block_sum(acc, red);
  // boundary launch of a peer-to-peer run: the outgoing halo rows were stored straight into the neighbours' windows;
  // a full barrier drains every wave's stores (block_sum's barriers order LDS only), then one lane writes the XCD's L2
  // back towards the peers
  if (a.release_sends) __syncthreads();
  if (threadIdx.x == 0) {
    a.partials_out[wblock] = acc;
    if (a.release_sends) __atomic_thread_fence(__ATOMIC_RELEASE);
  }
}

__device__ __forceinline__ void fold_previous(const StepArgs& a, double* red)
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

}  // namespace
