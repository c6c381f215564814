// lbm_f64.hip — the double-precision mode of liblbm_d2q9.so: the device entry points of include/lbm_d2q9_f64.h and, through
// kernels/step64.h, its gfx950 kernels.  A translation unit of its own: the float path's code objects (lbm_kernels.hip) do not
// change with it.  The host-only half (parser, end-of-run reductions, writers) is in lbm_host.cpp.
//
// What one step does is what lbm_kernels.hip's header lists, with every float object a double (the contract: lbm_d2q9_f64.h):
// pull-stream, moments + equilibrium, BGK relaxation / bounce-back, the sum|u| terms into per-block partials, accelerate_flow as an
// epilogue on row ny-2 for the NEXT step, av_vels[t] folded by block 0 of the next launch.  lbm_step_kernel_f64<CELLS, NT> makes one
// step per launch; with LBM64_FLAG_TILE_STEPS a small grid is advanced by lbm_tile_kernel_f64<T, H, FULL> (kernels/tile64.h), up to H
// steps per launch; with LBM64_FLAG_MULTI_STEPS a large one by lbm_multi_kernel_f64<K, NT, FULL> (kernels/multi64.h), up to K.  Whole
// periodic grids on one GPU only (no partitions, no fused arithmetic, no hipGraph, no state digest).  What a context gets of all that
// is decided in lbm_plan.cpp (Plan64 and PlanMulti64, lbm_internal.h); this unit allocates and launches by the plans.
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
#include "lbm_internal.h"
#include "lbm_knobs.h"
#include "kernels/step64.h"
#include "kernels/tile64.h"
#include "kernels/multi64.h"

namespace {

#define HIP_TRY(expr)                                                                        \
  do {                                                                                       \
    hipError_t e_ = (expr);                                                                  \
    if (e_ != hipSuccess) {                                                                  \
      lbm_internal::set_error(std::string(#expr) + ": " + hipGetErrorString(e_));            \
      return 1;                                                                              \
    }                                                                                        \
  } while (0)

}  // namespace

struct lbm64_ctx {
  Knobs knobs;                       // the environment knobs as lbm64_create read them (lbm_knobs.h)
  lbm64_params p{};
  int free_cells = 0;
  double free_cells_inv = 0.0;
  int device = 0;
  lbm_internal::Plan64 plan{};       // kernels, launch shapes and sizes (lbm_plan.cpp plan64_whole): written once
  lbm_internal::PlanMulti64 multi{}; // lbm_multi_kernel_f64's part of them (plan64_multi): written once
  size_t ncells = 0, ps = 0;
  double* grid_alloc[2] = {nullptr, nullptr};
  double* grid[2] = {nullptr, nullptr};      // plane 0 row 0 (after the front guard)
  int cur = 0;
  uint32_t* mask = nullptr;
  double* partials[2] = {nullptr, nullptr};
  double* sums = nullptr;
  int sums_cap = 0;
  int* counter = nullptr;
  double accel_w1 = 0.0, accel_w2 = 0.0;
  hipStream_t stream = nullptr;
  hipEvent_t ev_begin = nullptr, ev_end = nullptr;
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

int ensure_sums(lbm64_ctx* c, int n)
{
  if (n <= c->sums_cap) return 0;
  n = std::max(n, std::max(c->p.max_iters, 4096));
  double* dev = nullptr;
  HIP_TRY(hipMalloc(&dev, sizeof(double) * static_cast<size_t>(n)));
  if (c->sums) (void)hipFree(c->sums);         // between runs: the stream is idle
  c->sums = dev;
  c->sums_cap = n;
  return 0;
}

// cells of whole rows that the chunked copies (cells, observables) move at a time
size_t chunk_cells(const lbm64_ctx* c)
{
  const size_t nx = static_cast<size_t>(c->p.nx);
  return std::min(c->ncells, std::max<size_t>(1, static_cast<size_t>(std::max(c->knobs.obs_chunk_cells, 1)) / nx) * nx);
}

}  // namespace

extern "C" {

int lbm64_destroy(lbm64_ctx* c)
{
  if (!c) return 0;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  for (int g = 0; g < 2; ++g) if (c->grid_alloc[g]) (void)hipFree(c->grid_alloc[g]);
  if (c->mask) (void)hipFree(c->mask);
  for (int i = 0; i < 2; ++i) if (c->partials[i]) (void)hipFree(c->partials[i]);
  if (c->sums) (void)hipFree(c->sums);
  if (c->counter) (void)hipFree(c->counter);
  if (c->ev_begin) (void)hipEventDestroy(c->ev_begin);
  if (c->ev_end) (void)hipEventDestroy(c->ev_end);
  if (c->stream) (void)hipStreamDestroy(c->stream);
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
    lbm_internal::set_error("lbm64_create: the double-precision mode takes LBM_FLAG_NT_STORES or LBM_FLAG_NO_NT_STORES only, each with or without LBM64_FLAG_TILE_STEPS and LBM64_FLAG_MULTI_STEPS (whole grids, exact arithmetic)");
    return 1;
  }
  if (static_cast<long long>(p->nx) * p->ny > (1LL << 31) - 4096) { lbm_internal::set_error("lbm64_create: grid too large for 32-bit cell indices"); return 1; }

  HIP_TRY(hipSetDevice(device));
  lbm64_ctx* c = new lbm64_ctx();
  c->knobs = knobs_from_env();
  c->p = *p;
  c->free_cells = free_cells;
  c->free_cells_inv = 1.0 / free_cells;                                      // d2q9-bgk.c:950 in double
  c->device = device;
  c->accel_w1 = p->density * p->accel * 0.111111111111111111111111;         // d2q9-bgk.c:445
  c->accel_w2 = p->density * p->accel * 0.0277777777777777777777778;        // d2q9-bgk.c:446
  c->ncells = static_cast<size_t>(p->nx) * p->ny;
  lbm_internal::plan64_whole(c->knobs, p, flags, &c->plan);
  const lbm_internal::Plan64& plan = c->plan;
  lbm_internal::plan64_multi(c->knobs, p, plan, &c->multi);
  const lbm_internal::PlanMulti64& multi = c->multi;
  c->ps = static_cast<size_t>(plan.ps);

  auto fail = [&](void) { lbm64_destroy(c); return 1; };
#define HIP_TRY_C(expr)                                                                      \
  do {                                                                                       \
    hipError_t e_ = (expr);                                                                  \
    if (e_ != hipSuccess) {                                                                  \
      lbm_internal::set_error(std::string(#expr) + ": " + hipGetErrorString(e_));            \
      return fail();                                                                         \
    }                                                                                        \
  } while (0)

  HIP_TRY_C(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  HIP_TRY_C(hipEventCreate(&c->ev_begin));
  HIP_TRY_C(hipEventCreate(&c->ev_end));
  for (int g = 0; g < 2; ++g) {
    HIP_TRY_C(hipMalloc(&c->grid_alloc[g], sizeof(double) * static_cast<size_t>(plan.grid_doubles)));
    HIP_TRY_C(hipMemsetAsync(c->grid_alloc[g], 0, sizeof(double) * static_cast<size_t>(plan.grid_doubles), c->stream));
    c->grid[g] = c->grid_alloc[g] + 64;
  }
  // obstacle bitfield: bit c of the cell index, as the float path's
  const size_t mwords = (c->ncells + 31) / 32 + 4;
  {
    std::vector<uint32_t> bits(mwords, 0u);
    for (size_t i = 0; i < c->ncells; ++i)
      if (obstacles[i]) bits[i >> 5] |= 1u << (i & 31);
    HIP_TRY_C(hipMalloc(&c->mask, sizeof(uint32_t) * mwords));
    HIP_TRY_C(hipMemcpy(c->mask, bits.data(), sizeof(uint32_t) * mwords, hipMemcpyHostToDevice));
  }
  for (int i = 0; i < 2; ++i) HIP_TRY_C(hipMalloc(&c->partials[i], sizeof(double) * static_cast<size_t>(std::max(plan.partials_cap, multi.multi_kernel ? multi.partials_cap : 0))));
  if (plan.tile_kernel && plan.tile_lds_bytes > 65536) {     // dynamic LDS above 64 KiB: raised once, for the two instantiations the context launches
    for (int full = 0; full < 2; ++full)
      HIP_TRY_C(hipFuncSetAttribute(reinterpret_cast<const void*>(kTile64Kernels[tile64_row(plan.tile_T, plan.tile_H, full != 0)]),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, plan.tile_lds_bytes));
  }
  if (multi.multi_kernel && multi.lds_bytes > 65536) {
    for (int full = 0; full < 2; ++full)
      HIP_TRY_C(hipFuncSetAttribute(reinterpret_cast<const void*>(kMulti64Kernels[multi64_row(multi.K, multi.nt_stores != 0, full != 0)]),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, multi.lds_bytes));
  }
  HIP_TRY_C(hipMalloc(&c->counter, sizeof(int)));
  HIP_TRY_C(hipMemsetAsync(c->counter, 0, sizeof(int), c->stream));
  if (ensure_sums(c, 1)) return fail();
  {
    const double w0 = p->density * 4.0 / 9.0, w1 = p->density / 9.0, w2 = p->density / 36.0;   // d2q9-bgk.c:880-882
    const unsigned blocks = static_cast<unsigned>((c->ncells + 255) / 256);
    hipLaunchKernelGGL(lbm64_init_kernel, dim3(blocks), dim3(256), 0, c->stream, c->grid[0], c->ps, c->ncells, w0, w1, w2);
    HIP_TRY_C(hipGetLastError());
  }
  HIP_TRY_C(hipStreamSynchronize(c->stream));
#undef HIP_TRY_C
  *out = c;
  return 0;
}

int lbm64_run(lbm64_ctx* c, int n_steps, double* av_vels)
{
  if (!c) { lbm_internal::set_error("lbm64_run: null context"); return 1; }
  if (n_steps < 0) { lbm_internal::set_error("lbm64_run: negative step count"); return 1; }
  if (n_steps == 0) return 0;
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  if (ensure_sums(c, n_steps)) return 1;
  // accelerate_flow of the first step (d2q9-bgk.c:345-348): every later one is the epilogue of the step before it
  const uint32_t nx = static_cast<uint32_t>(c->p.nx), ny = static_cast<uint32_t>(c->p.ny);
  hipLaunchKernelGGL(lbm64_accelerate_kernel, dim3((nx + 255) / 256), dim3(256), 0, s, c->grid[c->cur], c->ps, c->mask, nx, ny - 2, c->accel_w1, c->accel_w2);
  HIP_TRY(hipGetLastError());
  const lbm_internal::Plan64& plan = c->plan;
  int parity = 0, launches = 0;
  int last_n = 0, last_vecs = 0;        // the last launch's partials: vectors of last_n sums, one per step
  if (plan.tile_kernel) {
    // up to tile_H steps per launch (lbm_plan.cpp plan64_next_steps); block 0 of a launch folds the vectors of the launch before it
    Tile64Args a{};
    a.mask = c->mask;
    a.ps = c->ps;
    a.nx = static_cast<int>(nx); a.ny = static_cast<int>(ny);
    a.tiles_x = plan.tiles_x;
    a.omega = c->p.omega;
    a.accel_w1 = c->accel_w1; a.accel_w2 = c->accel_w2;
    a.accel_row = static_cast<int>(ny) - 2;
    a.n_prev = plan.n_tiles;
    a.sums = c->sums;
    a.counter = c->counter;
    HIP_TRY(hipEventRecord(c->ev_begin, s));
    for (int left = n_steps; left > 0;) {
      const int k = lbm_internal::plan64_next_steps(plan, left);
      left -= k;
      a.src = c->grid[c->cur];
      a.dst = c->grid[c->cur ^ 1];
      a.ksteps = k;
      a.accel_last = left > 0;
      a.partials_out = c->partials[parity];
      a.prev_partials = c->partials[parity ^ 1];
      a.n_prev_vecs = last_vecs;
      const Tile64Kernel kernel = kTile64Kernels[tile64_row(plan.tile_T, plan.tile_H, k == plan.tile_H)];
      kernel<<<dim3(plan.n_tiles + 1), dim3(plan.tile_block), static_cast<size_t>(plan.tile_lds_bytes), s>>>(a);   // + the fold block
      last_vecs = k;
      parity ^= 1;
      c->cur ^= 1;
      ++launches;
    }
    last_n = plan.n_tiles;
  } else if (c->multi.multi_kernel) {
    // up to K steps per launch (lbm_plan.cpp plan64_multi_next_steps); block 0 of a launch folds the vectors of the launch before it
    const lbm_internal::PlanMulti64& multi = c->multi;
    Multi64Args a{};
    a.mask = c->mask;
    a.ps = c->ps;
    a.nx = static_cast<int>(nx); a.ny = static_cast<int>(ny);
    a.tiles_x = multi.tiles_x;
    a.omega = c->p.omega;
    a.accel_w1 = c->accel_w1; a.accel_w2 = c->accel_w2;
    a.accel_row = static_cast<int>(ny) - 2;
    a.n_prev = multi.n_tiles;
    a.sums = c->sums;
    a.counter = c->counter;
    HIP_TRY(hipEventRecord(c->ev_begin, s));
    for (int left = n_steps; left > 0;) {
      const int k = lbm_internal::plan64_multi_next_steps(multi, left);
      left -= k;
      a.src = c->grid[c->cur];
      a.dst = c->grid[c->cur ^ 1];
      a.ksteps = k;
      a.accel_last = left > 0;
      a.partials_out = c->partials[parity];
      a.prev_partials = c->partials[parity ^ 1];
      a.n_prev_vecs = last_vecs;
      const Multi64Kernel kernel = kMulti64Kernels[multi64_row(multi.K, multi.nt_stores != 0, k == multi.K)];
      kernel<<<dim3(multi.n_tiles + 1), dim3(multi.block), static_cast<size_t>(multi.lds_bytes), s>>>(a);   // + the fold block
      last_vecs = k;
      parity ^= 1;
      c->cur ^= 1;
      ++launches;
    }
    last_n = multi.n_tiles;
  } else {
    Step64Args a{};
    a.mask = c->mask;
    a.ps = c->ps;
    a.nx = nx; a.ny = ny;
    a.units = plan.units;
    a.iters = plan.iters;
    a.omega = c->p.omega;
    a.accel_w1 = c->accel_w1; a.accel_w2 = c->accel_w2;
    a.sums = c->sums;
    a.counter = c->counter;
    const Step64Kernel kernel = kStep64Kernels[plan.lane_cells == 1][plan.nt_stores];
    HIP_TRY(hipEventRecord(c->ev_begin, s));
    for (int t = 0; t < n_steps; ++t) {
      a.src = c->grid[c->cur];
      a.dst = c->grid[c->cur ^ 1];
      a.accel_row = t + 1 < n_steps ? static_cast<int>(ny) - 2 : -1;
      a.partials_out = c->partials[parity];
      a.prev_partials = c->partials[parity ^ 1];
      a.n_prev = t > 0 ? plan.blocks : 0;
      kernel<<<dim3(plan.blocks + 1), dim3(kBlock), 0, s>>>(a);               // + the fold block
      parity ^= 1;
      c->cur ^= 1;
    }
    launches = n_steps;
    last_n = plan.blocks; last_vecs = 1;
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(c->ev_end, s));
  c->ev_launches = launches;
  c->ev_valid = true;
  hipLaunchKernelGGL(lbm64_fold_kernel, dim3(1), dim3(kBlock), 0, s, c->partials[parity ^ 1], last_n, last_vecs, c->sums, c->counter);
  HIP_TRY(hipGetLastError());
  if (av_vels) {
    HIP_TRY(hipMemcpyAsync(av_vels, c->sums, sizeof(double) * n_steps, hipMemcpyDeviceToHost, s));
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
  HIP_TRY(hipSetDevice(c->device));
  const size_t chunk = chunk_cells(c);
  unsigned long long* tmp = nullptr;
  HIP_TRY(hipMalloc(&tmp, sizeof(double) * 9 * chunk));
  hipError_t e = hipSuccess;
  for (size_t c0 = 0; c0 < c->ncells && e == hipSuccess; c0 += chunk) {
    const size_t n = std::min(chunk, c->ncells - c0);
    hipLaunchKernelGGL(lbm64_soa_to_aos_kernel, dim3(static_cast<unsigned>((n * 9 + 255) / 256)), dim3(256), 0, c->stream,
                       reinterpret_cast<const unsigned long long*>(c->grid[c->cur] + c0), tmp, c->ps, n);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(cells_aos + 9 * c0, tmp, sizeof(double) * 9 * n, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  }
  (void)hipFree(tmp);
  HIP_TRY(e);
  return 0;
}

int lbm64_set_cells(lbm64_ctx* c, const double* cells_aos)
{
  if (!c || !cells_aos) { lbm_internal::set_error("lbm64_set_cells: null argument"); return 1; }
  HIP_TRY(hipSetDevice(c->device));
  const size_t chunk = chunk_cells(c);
  unsigned long long* tmp = nullptr;
  HIP_TRY(hipMalloc(&tmp, sizeof(double) * 9 * chunk));
  hipError_t e = hipSuccess;
  for (size_t c0 = 0; c0 < c->ncells && e == hipSuccess; c0 += chunk) {
    const size_t n = std::min(chunk, c->ncells - c0);
    e = hipMemcpyAsync(tmp, cells_aos + 9 * c0, sizeof(double) * 9 * n, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(lbm64_aos_to_soa_kernel, dim3(static_cast<unsigned>((n * 9 + 255) / 256)), dim3(256), 0, c->stream,
                         tmp, reinterpret_cast<unsigned long long*>(c->grid[c->cur] + c0), c->ps, n);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  }
  (void)hipFree(tmp);
  HIP_TRY(e);
  return 0;
}

int lbm64_get_observables(lbm64_ctx* c, double* obs)
{
  if (!c || !obs) { lbm_internal::set_error("lbm64_get_observables: null argument"); return 1; }
  HIP_TRY(hipSetDevice(c->device));
  const size_t chunk = chunk_cells(c);
  double* tmp = nullptr;
  HIP_TRY(hipMalloc(&tmp, sizeof(double) * 4 * chunk));
  hipError_t e = hipSuccess;
  for (size_t c0 = 0; c0 < c->ncells && e == hipSuccess; c0 += chunk) {
    const size_t n = std::min(chunk, c->ncells - c0);
    hipLaunchKernelGGL(lbm64_observables_kernel, dim3(static_cast<unsigned>((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, c->stream,
                       c->grid[c->cur] + c0, c->ps, n, tmp);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(obs + 4 * c0, tmp, sizeof(double) * 4 * n, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  }
  (void)hipFree(tmp);
  HIP_TRY(e);
  return 0;
}

int lbm64_av_velocity_sum(lbm64_ctx* c, double* tot_u)
{
  if (!c || !tot_u) { lbm_internal::set_error("lbm64_av_velocity_sum: null argument"); return 1; }
  HIP_TRY(hipSetDevice(c->device));
  const int blocks = static_cast<int>(std::min<size_t>((c->ncells + kBlock - 1) / kBlock, 1024));
  double* part = nullptr;
  HIP_TRY(hipMalloc(&part, sizeof(double) * blocks));
  hipLaunchKernelGGL(lbm64_av_velocity_kernel, dim3(blocks), dim3(kBlock), 0, c->stream, c->grid[c->cur], c->ps, c->mask, c->ncells, part);
  std::vector<double> host(blocks);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(host.data(), part, sizeof(double) * blocks, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  (void)hipFree(part);
  HIP_TRY(e);
  double s = 0.0;
  for (double v : host) s += v;
  *tot_u = s;
  return 0;
}

int lbm64_last_run_kernel_ms(lbm64_ctx* c, double* ms, int* launches)
{
  if (!c || !ms) { lbm_internal::set_error("lbm64_last_run_kernel_ms: null argument"); return 1; }
  if (!c->ev_valid) { lbm_internal::set_error("lbm64_last_run_kernel_ms: no run yet"); return 1; }
  HIP_TRY(hipSetDevice(c->device));
  float t = 0.f;
  HIP_TRY(hipEventElapsedTime(&t, c->ev_begin, c->ev_end));
  *ms = t;
  if (launches) *launches = c->ev_launches;
  return 0;
}

int lbm64_describe(const lbm64_ctx* c, char* kernel_name, size_t len, long long* blocks, long long* cells_per_block, long long* state_bytes)
{
  if (!c) { lbm_internal::set_error("lbm64_describe: null context"); return 1; }
  const lbm_internal::Plan64& plan = c->plan;
  const lbm_internal::PlanMulti64& multi = c->multi;
  if (multi.multi_kernel) {
    if (kernel_name && len > 0) lbm_internal::plan64_multi_kernel_name(multi, kernel_name, len);
    if (blocks) *blocks = multi.n_tiles;
    if (cells_per_block) *cells_per_block = static_cast<long long>(multi.TX) * multi.TY;
    if (state_bytes) *state_bytes = static_cast<long long>(2 * 9 * c->ncells * sizeof(double));
    return 0;
  }
  if (kernel_name && len > 0) lbm_internal::plan64_kernel_name(plan, kernel_name, len);
  if (blocks) *blocks = plan.tile_kernel ? plan.n_tiles : plan.blocks;
  if (cells_per_block) *cells_per_block = plan.tile_kernel ? static_cast<long long>(plan.tile_T) * plan.tile_T : static_cast<long long>(kBlock) * plan.iters * plan.lane_cells;
  if (state_bytes) *state_bytes = static_cast<long long>(2 * 9 * c->ncells * sizeof(double));
  return 0;
}

}  // extern "C"
