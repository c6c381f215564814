// lbm_f64.hip — the double-precision mode of liblbm_d2q9.so: the device entry points of include/lbm_d2q9_f64.h and, through
// kernels/step64.h, its gfx950 kernels.  A translation unit of its own: the float path's code objects (lbm_kernels.hip) do not
// change with it.  The host-only half (parser, end-of-run reductions, writers) is in lbm_host.cpp.
//
// What one step does is what lbm_kernels.hip's header lists, with every float object a double (the contract: lbm_d2q9_f64.h):
// pull-stream, moments + equilibrium, BGK relaxation / bounce-back, the sum|u| terms into per-block partials, accelerate_flow as an
// epilogue on row ny-2 for the NEXT step, av_vels[t] folded by block 0 of the next launch.  lbm_step_kernel_f64<CELLS, NT> makes one
// step per launch; with LBM64_FLAG_TILE_STEPS a small grid is advanced by lbm_tile_kernel_f64<T, H, FULL> (kernels/tile64.h), up to H
// steps per launch; with LBM64_FLAG_MULTI_STEPS a large one by lbm_multi_kernel_f64<K, NT, FULL> (kernels/multi64.h), up to K, and with
// LBM64_FLAG_MULTI_ANY_SIZE by its edge-tile form where the tiles do not cover the grid.  Whole
// periodic grids on one GPU only (no partitions, no fused arithmetic, no hipGraph; the state digest is lbm_digest64_grid, at the end of
// this unit: include/lbm_d2q9_f64_digest.h).  What a context gets of all that
// is decided in lbm_plan.cpp (Plan64 and PlanMultiAny64, lbm_internal.h); this unit allocates and launches by the plans.  What it does
// with its grid as lbm_rows64.hip does with a rank's row block (allocation, chunked read-outs, the velocity sum) is in lbm_f64_slab.h.
//
// Layout in HBM: struct-of-arrays, 9 planes of ny*nx doubles at a padded, skewed plane stride (the float path's rule in elements: lbm_plan.cpp plane_stride_floats), two grids
// swapped per launch, the obstacle map as the float path's bitfield.  Compiled with -ffp-contract=off like the rest of the library:
// the post-step populations are the bits gcc -std=c99 gives the same statements (tests/f64_ref.c).
//
// gfx950 only: 64-wide wavefronts (block_sum).

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "lbm_d2q9_f64.h"
#include "lbm_d2q9_f64_digest.h"
#include "lbm_internal.h"
#include "lbm_knobs.h"
#include "kernels/step64.h"
#include "kernels/tile64.h"
#include "kernels/multi64.h"
#include "lbm_f64_slab.h"

struct lbm64_ctx {
  Knobs knobs;                       // the environment knobs as lbm64_create read them (lbm_knobs.h)
  lbm64_params p{};
  int free_cells = 0;
  double free_cells_inv = 0.0;
  lbm_internal::Plan64 plan{};       // kernels, launch shapes and sizes (lbm_plan.cpp plan64_whole): written once
  lbm_internal::PlanMultiAny64 multi{};   // lbm_multi_kernel_f64's part of them, the edge-tile form included (plan64_multi_any): written once
  Slab64 slab;                       // the whole grid on its device (lbm_f64_slab.h)
  int cur = 0;
  double accel_w1 = 0.0, accel_w2 = 0.0;
  int ev_launches = 0;
  bool ev_valid = false;
};

namespace {

using Step64Kernel = void (*)(Step64Args);
// every instantiation of the one-step kernel, by [one cell per lane][non-temporal stores]
constexpr Step64Kernel kStep64Kernels[2][2] = {
  {&lbm_step_kernel_f64<kPairCells, false>, &lbm_step_kernel_f64<kPairCells, true>},
  {&lbm_step_kernel_f64<1, false>, &lbm_step_kernel_f64<1, true>},
};

using Tile64Kernel = void (*)(Tile64Args);
// every instantiation of the tiled kernel, by tile64_row(T, H, FULL) (lbm_geometry.h, which also has their block sizes and LDS bytes)
constexpr Tile64Kernel kTile64Kernels[kTile64Rows] = {
  &lbm_tile_kernel_f64<16, 8, false>, &lbm_tile_kernel_f64<16, 8, true>, &lbm_tile_kernel_f64<16, 4, false>, &lbm_tile_kernel_f64<16, 4, true>,
  &lbm_tile_kernel_f64<8, 8, false>,  &lbm_tile_kernel_f64<8, 8, true>,  &lbm_tile_kernel_f64<8, 4, false>,  &lbm_tile_kernel_f64<8, 4, true>,
};
static_assert(tile64_row(16, 8, false) == 0 && tile64_row(16, 4, true) == 3 && tile64_row(8, 8, false) == 4 && tile64_row(8, 4, true) == 7, "the order of kTile64Kernels");

using Multi64Kernel = void (*)(Multi64Args);
// every instantiation of the multi-step kernel, by multi64_row(K, NT, FULL) (lbm_geometry.h, which also has the block size and LDS bytes)
#define LBM_MULTI64_ROWS(K) &lbm_multi_kernel_f64<K, false, false>, &lbm_multi_kernel_f64<K, false, true>, &lbm_multi_kernel_f64<K, true, false>, &lbm_multi_kernel_f64<K, true, true>
constexpr Multi64Kernel kMulti64Kernels[kMulti64Rows] = {LBM_MULTI64_ROWS(2), LBM_MULTI64_ROWS(3), LBM_MULTI64_ROWS(4)};
#undef LBM_MULTI64_ROWS
static_assert(kMulti64MinK == 2 && kMulti64MaxK == 4 && multi64_row(2, false, true) == 1 && multi64_row(3, true, false) == 6 && multi64_row(4, true, true) == 11, "the order of kMulti64Kernels");
// and every instantiation of its edge-tile form (LBM64_FLAG_MULTI_ANY_SIZE), in the same order
#define LBM_MULTI64_EDGE_ROWS(K) &lbm_multi_kernel_f64<K, false, false, true>, &lbm_multi_kernel_f64<K, false, true, true>, &lbm_multi_kernel_f64<K, true, false, true>, &lbm_multi_kernel_f64<K, true, true, true>
constexpr Multi64Kernel kMulti64EdgeKernels[kMulti64Rows] = {LBM_MULTI64_EDGE_ROWS(2), LBM_MULTI64_EDGE_ROWS(3), LBM_MULTI64_EDGE_ROWS(4)};
#undef LBM_MULTI64_EDGE_ROWS
// the instantiation a context launches for a launch of K steps (full) or fewer
Multi64Kernel multi64_kernel(const lbm_internal::PlanMultiAny64& m, bool full)
{
  return (m.edge ? kMulti64EdgeKernels : kMulti64Kernels)[multi64_row(m.K, m.nt_stores != 0, full)];
}

// The run loop of both frame kernels (lbm_tile_kernel_f64, lbm_multi_kernel_f64): next_steps(left) steps per launch of kernel_of(steps)
// over n_tiles blocks; block 0 of a launch folds the vectors of the launch before it.  Moves on *parity and c->cur; leaves the number
// of launches and the vectors of the last one.
template <typename Args, typename NextSteps, typename KernelOf>
int run_frames(lbm64_ctx* c, int n_steps, int tiles_x, int n_tiles, int block, int lds_bytes, NextSteps next_steps, KernelOf kernel_of,
               int* parity, int* launches, int* last_vecs)
{
  const Slab64& s = c->slab;
  Args a{};
  a.mask = s.mask;
  a.ps = s.ps;
  a.nx = c->p.nx; a.ny = c->p.ny;
  a.tiles_x = tiles_x;
  a.omega = c->p.omega;
  a.accel_w1 = c->accel_w1; a.accel_w2 = c->accel_w2;
  a.accel_row = c->p.ny - 2;
  a.n_prev = n_tiles;
  a.sums = s.sums;
  a.counter = s.counter;
  HIP_TRY(hipEventRecord(s.ev_begin, s.stream));
  for (int left = n_steps; left > 0;) {
    const int k = next_steps(left);
    left -= k;
    a.src = s.grid[c->cur];
    a.dst = s.grid[c->cur ^ 1];
    a.ksteps = k;
    a.accel_last = left > 0;
    a.partials_out = s.partials[*parity];
    a.prev_partials = s.partials[*parity ^ 1];
    a.n_prev_vecs = *last_vecs;
    kernel_of(k)<<<dim3(n_tiles + 1), dim3(block), static_cast<size_t>(lds_bytes), s.stream>>>(a);   // + the fold block
    *last_vecs = k;
    *parity ^= 1;
    c->cur ^= 1;
    ++*launches;
  }
  return 0;
}

}  // namespace

extern "C" {

int lbm64_destroy(lbm64_ctx* c)
{
  if (!c) return 0;
  slab64_destroy(c->slab);
  delete c;
  return 0;
}

int lbm64_create(lbm64_ctx** out, const lbm64_params* p, int free_cells, const int* obstacles, int device, unsigned flags)
{
  if (!out || !p || !obstacles) { lbm_internal::set_error("lbm64_create: null argument"); return 1; }
  *out = nullptr;
  if (p->nx < 1) { lbm_internal::set_error("lbm64_create: nx must be positive"); return 1; }
  if (p->ny < 3) { lbm_internal::set_error("lbm64_create: ny must be >= 3 (accelerate_flow works on row ny-2, d2q9-bgk.c:449)"); return 1; }
  if (free_cells <= 0) { lbm_internal::set_error("lbm64_create: free_cells must be positive"); return 1; }
  if ((flags & ~lbm_internal::kFlags64) != 0u) {
    lbm_internal::set_error("lbm64_create: the double-precision mode takes LBM_FLAG_NT_STORES or LBM_FLAG_NO_NT_STORES only, each with or without LBM64_FLAG_TILE_STEPS, LBM64_FLAG_MULTI_STEPS and LBM64_FLAG_MULTI_ANY_SIZE (whole grids, exact arithmetic)");
    return 1;
  }
  if (static_cast<long long>(p->nx) * p->ny > (1LL << 31) - 4096) { lbm_internal::set_error("lbm64_create: grid too large for 32-bit cell indices"); return 1; }

  HIP_TRY(hipSetDevice(device));
  lbm64_ctx* c = new lbm64_ctx();
  c->knobs = knobs_from_env();
  c->p = *p;
  c->free_cells = free_cells;
  c->free_cells_inv = 1.0 / free_cells;                                      // d2q9-bgk.c:950 in double
  c->accel_w1 = p->density * p->accel * 0.111111111111111111111111;         // d2q9-bgk.c:445
  c->accel_w2 = p->density * p->accel * 0.0277777777777777777777778;        // d2q9-bgk.c:446
  lbm_internal::plan64_whole(c->knobs, p, flags, &c->plan);
  const lbm_internal::Plan64& plan = c->plan;
  lbm_internal::plan64_multi_any(c->knobs, p, plan, &c->multi);
  const lbm_internal::PlanMultiAny64& multi = c->multi;
  Slab64& s = c->slab;
  s.device = device;
  s.ncells = static_cast<size_t>(p->nx) * p->ny;
  s.ps = static_cast<size_t>(plan.ps);

  auto fail = [&](void) { lbm64_destroy(c); return 1; };
  if (slab64_create(s, static_cast<size_t>(plan.grid_doubles), (s.ncells + 31) / 32 + 4,
                    static_cast<size_t>(std::max(plan.partials_cap, multi.multi_kernel ? multi.partials_cap : 0)), obstacles, p->density, p->max_iters))
    return fail();
  if (plan.tile_kernel && plan.tile_lds_bytes > 65536) {     // dynamic LDS above 64 KiB: raised once, for the two instantiations the context launches
    for (int full = 0; full < 2; ++full)
      HIP_TRY_OR(hipFuncSetAttribute(reinterpret_cast<const void*>(kTile64Kernels[tile64_row(plan.tile_T, plan.tile_H, full != 0)]),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, plan.tile_lds_bytes), return fail());
  }
  if (multi.multi_kernel && multi.lds_bytes > 65536) {
    for (int full = 0; full < 2; ++full)
      HIP_TRY_OR(hipFuncSetAttribute(reinterpret_cast<const void*>(multi64_kernel(multi, full != 0)),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, multi.lds_bytes), return fail());
  }
  HIP_TRY_OR(hipStreamSynchronize(s.stream), return fail());
  *out = c;
  return 0;
}

int lbm64_run(lbm64_ctx* c, int n_steps, double* av_vels)
{
  if (!c) { lbm_internal::set_error("lbm64_run: null context"); return 1; }
  if (n_steps < 0) { lbm_internal::set_error("lbm64_run: negative step count"); return 1; }
  if (n_steps == 0) return 0;
  Slab64& slab = c->slab;
  HIP_TRY(hipSetDevice(slab.device));
  hipStream_t s = slab.stream;
  if (slab64_ensure_sums(slab, n_steps, c->p.max_iters)) return 1;
  // accelerate_flow of the first step (d2q9-bgk.c:345-348): every later one is the epilogue of the step before it
  const uint32_t nx = static_cast<uint32_t>(c->p.nx), ny = static_cast<uint32_t>(c->p.ny);
  hipLaunchKernelGGL(lbm64_accelerate_kernel, dim3((nx + 255) / 256), dim3(256), 0, s, slab.grid[c->cur], slab.ps, slab.mask, nx, ny - 2, c->accel_w1, c->accel_w2);
  HIP_TRY(hipGetLastError());
  const lbm_internal::Plan64& plan = c->plan;
  const lbm_internal::PlanMultiAny64& multi = c->multi;
  int parity = 0, launches = 0;
  int last_n = 0, last_vecs = 0;        // the last launch's partials: vectors of last_n sums, one per step
  if (plan.tile_kernel) {
    // up to tile_H steps per launch (lbm_plan.cpp plan64_next_steps)
    if (run_frames<Tile64Args>(c, n_steps, plan.tiles_x, plan.n_tiles, plan.tile_block, plan.tile_lds_bytes,
                               [&](int left) { return lbm_internal::plan64_next_steps(plan, left); },
                               [&](int k) { return kTile64Kernels[tile64_row(plan.tile_T, plan.tile_H, k == plan.tile_H)]; },
                               &parity, &launches, &last_vecs)) return 1;
    last_n = plan.n_tiles;
  } else if (multi.multi_kernel) {
    // up to K steps per launch (lbm_plan.cpp plan64_multi_any_next_steps)
    if (run_frames<Multi64Args>(c, n_steps, multi.tiles_x, multi.n_tiles, multi.block, multi.lds_bytes,
                                [&](int left) { return lbm_internal::plan64_multi_any_next_steps(multi, left); },
                                [&](int k) { return multi64_kernel(multi, k == multi.K); },
                                &parity, &launches, &last_vecs)) return 1;
    last_n = multi.n_tiles;
  } else {
    Step64Args a{};
    a.mask = slab.mask;
    a.ps = slab.ps;
    a.nx = nx; a.ny = ny;
    a.units = plan.units;
    a.iters = plan.iters;
    a.omega = c->p.omega;
    a.accel_w1 = c->accel_w1; a.accel_w2 = c->accel_w2;
    a.sums = slab.sums;
    a.counter = slab.counter;
    const Step64Kernel kernel = kStep64Kernels[plan.lane_cells == 1][plan.nt_stores];
    HIP_TRY(hipEventRecord(slab.ev_begin, s));
    for (int t = 0; t < n_steps; ++t) {
      a.src = slab.grid[c->cur];
      a.dst = slab.grid[c->cur ^ 1];
      a.accel_row = t + 1 < n_steps ? static_cast<int>(ny) - 2 : -1;
      a.partials_out = slab.partials[parity];
      a.prev_partials = slab.partials[parity ^ 1];
      a.n_prev = t > 0 ? plan.blocks : 0;
      kernel<<<dim3(plan.blocks + 1), dim3(kBlock), 0, s>>>(a);               // + the fold block
      parity ^= 1;
      c->cur ^= 1;
    }
    launches = n_steps;
    last_n = plan.blocks; last_vecs = 1;
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(slab.ev_end, s));
  c->ev_launches = launches;
  c->ev_valid = true;
  hipLaunchKernelGGL(lbm64_fold_kernel, dim3(1), dim3(kBlock), 0, s, slab.partials[parity ^ 1], last_n, last_vecs, slab.sums, slab.counter);
  HIP_TRY(hipGetLastError());
  if (av_vels) {
    HIP_TRY(hipMemcpyAsync(av_vels, slab.sums, sizeof(double) * n_steps, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int t = 0; t < n_steps; ++t) av_vels[t] = av_vels[t] * c->free_cells_inv;          // d2q9-bgk.c:367
  } else {
    HIP_TRY(hipStreamSynchronize(s));
  }
  return 0;
}

int lbm64_get_cells(lbm64_ctx* c, double* cells_aos)
{
  if (!c || !cells_aos) { lbm_internal::set_error("lbm64_get_cells: null argument"); return 1; }
  HIP_TRY(hipSetDevice(c->slab.device));
  return slab64_get_cells(c->slab, c->cur, slab64_chunk_cells(c->slab, c->p.nx, c->knobs), cells_aos);
}

int lbm64_set_cells(lbm64_ctx* c, const double* cells_aos)
{
  if (!c || !cells_aos) { lbm_internal::set_error("lbm64_set_cells: null argument"); return 1; }
  HIP_TRY(hipSetDevice(c->slab.device));
  return slab64_set_cells(c->slab, c->cur, slab64_chunk_cells(c->slab, c->p.nx, c->knobs), cells_aos);
}

int lbm64_get_observables(lbm64_ctx* c, double* obs)
{
  if (!c || !obs) { lbm_internal::set_error("lbm64_get_observables: null argument"); return 1; }
  HIP_TRY(hipSetDevice(c->slab.device));
  return slab64_get_observables(c->slab, c->cur, slab64_chunk_cells(c->slab, c->p.nx, c->knobs), obs);
}

int lbm64_av_velocity_sum(lbm64_ctx* c, double* tot_u)
{
  if (!c || !tot_u) { lbm_internal::set_error("lbm64_av_velocity_sum: null argument"); return 1; }
  HIP_TRY(hipSetDevice(c->slab.device));
  double s = 0.0;
  if (slab64_add_velocity_sum(c->slab, c->cur, &s)) return 1;
  *tot_u = s;
  return 0;
}

int lbm64_last_run_kernel_ms(lbm64_ctx* c, double* ms, int* launches)
{
  if (!c || !ms) { lbm_internal::set_error("lbm64_last_run_kernel_ms: null argument"); return 1; }
  if (!c->ev_valid) { lbm_internal::set_error("lbm64_last_run_kernel_ms: no run yet"); return 1; }
  HIP_TRY(hipSetDevice(c->slab.device));
  float t = 0.f;
  HIP_TRY(hipEventElapsedTime(&t, c->slab.ev_begin, c->slab.ev_end));
  *ms = t;
  if (launches) *launches = c->ev_launches;
  return 0;
}

int lbm64_describe(const lbm64_ctx* c, char* kernel_name, size_t len, long long* blocks, long long* cells_per_block, long long* state_bytes)
{
  if (!c) { lbm_internal::set_error("lbm64_describe: null context"); return 1; }
  const lbm_internal::Plan64& plan = c->plan;
  const lbm_internal::PlanMultiAny64& multi = c->multi;
  if (multi.multi_kernel) {
    if (kernel_name && len > 0) lbm_internal::plan64_multi_any_kernel_name(multi, kernel_name, len);
    if (blocks) *blocks = multi.n_tiles;
    if (cells_per_block) *cells_per_block = static_cast<long long>(multi.TX) * multi.TY;
    if (state_bytes) *state_bytes = static_cast<long long>(2 * 9 * c->slab.ncells * sizeof(double));
    return 0;
  }
  if (kernel_name && len > 0) lbm_internal::plan64_kernel_name(plan, kernel_name, len);
  if (blocks) *blocks = plan.tile_kernel ? plan.n_tiles : plan.blocks;
  if (cells_per_block) *cells_per_block = plan.tile_kernel ? static_cast<long long>(plan.tile_T) * plan.tile_T : static_cast<long long>(kBlock) * plan.iters * plan.lane_cells;
  if (state_bytes) *state_bytes = static_cast<long long>(2 * 9 * c->slab.ncells * sizeof(double));
  return 0;
}

// include/lbm_d2q9_f64_digest.h: one digest per row of the current grid.  Reads the grid on the slab's stream and leaves the context as
// it was: cur, the partials, the counter and the events of the last run are not touched.
int lbm_digest64_grid(lbm64_ctx* c, int y_begin, int y_end, unsigned long long* row_digests, unsigned long long* digest)
{
  if (!c) { lbm_internal::set_error("lbm_digest64_grid: null context"); return 1; }
  if (!row_digests && !digest) { lbm_internal::set_error("lbm_digest64_grid: both output pointers are null"); return 1; }
  if (y_begin < 0 || y_end > c->p.ny || y_begin > y_end) { lbm_internal::set_error("lbm_digest64_grid: rows outside the grid (0 <= y_begin <= y_end <= ny)"); return 1; }
  const int rows = y_end - y_begin;
  if (rows == 0) { if (digest) *digest = 0; return 0; }
  std::vector<unsigned long long> own;
  if (!row_digests) { own.resize(static_cast<size_t>(rows)); row_digests = own.data(); }
  HIP_TRY(hipSetDevice(c->slab.device));
  unsigned long long* dev = nullptr;
  const int bad = slab64_enqueue_row_digests(c->slab, c->cur, c->p.nx, y_begin, rows, y_begin, &dev);
  if (slab64_collect_row_digests(c->slab, dev, rows, row_digests) || bad) return 1;
  if (digest) *digest = slab64_digest_sum(row_digests, rows);
  return 0;
}

}  // extern "C"
