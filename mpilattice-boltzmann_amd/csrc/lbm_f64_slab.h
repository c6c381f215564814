// lbm_f64_slab.h — one device's share of a double-precision grid and what lbm_f64.hip (the whole grid) and lbm_rows64.hip (a rank's
// row block) both do with it: allocate and free it, grow its sums, copy cells and observables in chunks, sum the velocities.  Host
// side only; included after kernels/step64.h, whose kernels it launches.  Every function wants the slab's device current.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

#include "lbm_hip_try.h"
#include "lbm_knobs.h"

namespace {

struct Slab64 {
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev_begin = nullptr, ev_end = nullptr;
  double* grid_alloc[2] = {nullptr, nullptr};
  double* grid[2] = {nullptr, nullptr};      // plane 0 row 0 of the storage (after the front guard of 64 doubles)
  size_t ps = 0;                             // plane stride
  size_t ncells = 0, first = 0;              // owned cells; doubles from grid[g] to the first of them (0: a whole grid, nx: a row block)
  uint32_t* mask = nullptr;
  double* partials[2] = {nullptr, nullptr};
  double* sums = nullptr;
  int sums_cap = 0;
  int* counter = nullptr;

  double* owned(int g) const { return grid[g] + first; }
};

int slab64_ensure_sums(Slab64& s, int n, int max_iters)
{
  if (n <= s.sums_cap) return 0;
  n = std::max(n, std::max(max_iters, 4096));
  double* dev = nullptr;
  HIP_TRY(hipMalloc(&dev, sizeof(double) * static_cast<size_t>(n)));
  if (s.sums) (void)hipFree(s.sums);         // between runs: the stream is idle
  s.sums = dev;
  s.sums_cap = n;
  return 0;
}

// Stream, events, both grids (zeroed), the obstacle bitfield of `obstacles` (the first owned cell's flag: bit c of the owned-cell index,
// as the float path's), partials, counter, sums, and the rest state on the owned cells (enqueued, not waited for).  device, ps, ncells
// and first are the caller's to set before.  On failure the caller destroys the slab.
int slab64_create(Slab64& s, size_t grid_doubles, size_t mask_words, size_t partials_cap, const int* obstacles, double density, int max_iters)
{
  HIP_TRY(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking));
  HIP_TRY(hipEventCreate(&s.ev_begin));
  HIP_TRY(hipEventCreate(&s.ev_end));
  for (int g = 0; g < 2; ++g) {
    HIP_TRY(hipMalloc(&s.grid_alloc[g], sizeof(double) * grid_doubles));
    HIP_TRY(hipMemsetAsync(s.grid_alloc[g], 0, sizeof(double) * grid_doubles, s.stream));
    s.grid[g] = s.grid_alloc[g] + 64;
  }
  {
    std::vector<uint32_t> bits(mask_words, 0u);
    for (size_t i = 0; i < s.ncells; ++i)
      if (obstacles[i]) bits[i >> 5] |= 1u << (i & 31);
    HIP_TRY(hipMalloc(&s.mask, sizeof(uint32_t) * mask_words));
    HIP_TRY(hipMemcpy(s.mask, bits.data(), sizeof(uint32_t) * mask_words, hipMemcpyHostToDevice));
  }
  for (int i = 0; i < 2; ++i) HIP_TRY(hipMalloc(&s.partials[i], sizeof(double) * partials_cap));
  HIP_TRY(hipMalloc(&s.counter, sizeof(int)));
  HIP_TRY(hipMemsetAsync(s.counter, 0, sizeof(int), s.stream));
  if (slab64_ensure_sums(s, 1, max_iters)) return 1;
  const double w0 = density * 4.0 / 9.0, w1 = density / 9.0, w2 = density / 36.0;   // d2q9-bgk.c:880-882
  const unsigned blocks = static_cast<unsigned>((s.ncells + 255) / 256);
  hipLaunchKernelGGL(lbm64_init_kernel, dim3(blocks), dim3(256), 0, s.stream, s.owned(0), s.ps, s.ncells, w0, w1, w2);
  HIP_TRY(hipGetLastError());
  return 0;
}

// Waits for the slab's stream, then frees whatever slab64_create got as far as making.
void slab64_destroy(Slab64& s)
{
  if (!s.stream) return;                     // never reached its device: the stream is the first thing made
  (void)hipSetDevice(s.device);
  (void)hipStreamSynchronize(s.stream);
  for (int g = 0; g < 2; ++g) if (s.grid_alloc[g]) (void)hipFree(s.grid_alloc[g]);
  if (s.mask) (void)hipFree(s.mask);
  for (int i = 0; i < 2; ++i) if (s.partials[i]) (void)hipFree(s.partials[i]);
  if (s.sums) (void)hipFree(s.sums);
  if (s.counter) (void)hipFree(s.counter);
  if (s.ev_begin) (void)hipEventDestroy(s.ev_begin);
  if (s.ev_end) (void)hipEventDestroy(s.ev_end);
  (void)hipStreamDestroy(s.stream);
}

// cells of whole rows that the chunked copies (cells, observables) move at a time
size_t slab64_chunk_cells(const Slab64& s, int nx, const Knobs& knobs)
{
  const size_t row = static_cast<size_t>(nx);
  return std::min(s.ncells, std::max<size_t>(1, static_cast<size_t>(std::max(knobs.obs_chunk_cells, 1)) / row) * row);
}

// The chunked copies between the owned cells of grid `g` and the caller's array, `chunk` cells at a time.  `cells_aos` and `obs` point
// at the slab's first owned cell.
int slab64_get_cells(const Slab64& s, int g, size_t chunk, double* cells_aos)
{
  unsigned long long* tmp = nullptr;
  HIP_TRY(hipMalloc(&tmp, sizeof(double) * 9 * chunk));
  hipError_t e = hipSuccess;
  for (size_t c0 = 0; c0 < s.ncells && e == hipSuccess; c0 += chunk) {
    const size_t n = std::min(chunk, s.ncells - c0);
    hipLaunchKernelGGL(lbm64_soa_to_aos_kernel, dim3(static_cast<unsigned>((n * 9 + 255) / 256)), dim3(256), 0, s.stream,
                       reinterpret_cast<const unsigned long long*>(s.owned(g) + c0), tmp, s.ps, n);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(cells_aos + 9 * c0, tmp, sizeof(double) * 9 * n, hipMemcpyDeviceToHost, s.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(s.stream);
  }
  (void)hipFree(tmp);
  HIP_TRY(e);
  return 0;
}

int slab64_set_cells(const Slab64& s, int g, size_t chunk, const double* cells_aos)
{
  unsigned long long* tmp = nullptr;
  HIP_TRY(hipMalloc(&tmp, sizeof(double) * 9 * chunk));
  hipError_t e = hipSuccess;
  for (size_t c0 = 0; c0 < s.ncells && e == hipSuccess; c0 += chunk) {
    const size_t n = std::min(chunk, s.ncells - c0);
    e = hipMemcpyAsync(tmp, cells_aos + 9 * c0, sizeof(double) * 9 * n, hipMemcpyHostToDevice, s.stream);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(lbm64_aos_to_soa_kernel, dim3(static_cast<unsigned>((n * 9 + 255) / 256)), dim3(256), 0, s.stream,
                         tmp, reinterpret_cast<unsigned long long*>(s.owned(g) + c0), s.ps, n);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s.stream);
  }
  (void)hipFree(tmp);
  HIP_TRY(e);
  return 0;
}

int slab64_get_observables(const Slab64& s, int g, size_t chunk, double* obs)
{
  double* tmp = nullptr;
  HIP_TRY(hipMalloc(&tmp, sizeof(double) * 4 * chunk));
  hipError_t e = hipSuccess;
  for (size_t c0 = 0; c0 < s.ncells && e == hipSuccess; c0 += chunk) {
    const size_t n = std::min(chunk, s.ncells - c0);
    hipLaunchKernelGGL(lbm64_observables_kernel, dim3(static_cast<unsigned>((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s.stream,
                       s.owned(g) + c0, s.ps, n, tmp);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(obs + 4 * c0, tmp, sizeof(double) * 4 * n, hipMemcpyDeviceToHost, s.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(s.stream);
  }
  (void)hipFree(tmp);
  HIP_TRY(e);
  return 0;
}

// The row digests (include/lbm_d2q9_f64_digest.h) of `rows` owned rows of grid `g` from the slab's row `local_row` on, which is row
// `global_row` of the whole grid.  In two halves, so that a caller with several slabs enqueues on all of them before it waits for one:
// slab64_enqueue_row_digests launches lbm64_row_digest_kernel on the slab's stream into a device array it allocates (*dev);
// slab64_collect_row_digests copies that array to `out`, waits for the stream and frees it (call it after a failed enqueue too:
// *dev may be set).  rows >= 1.  Ghost rows are never reached: local_row counts from s.owned(g).  Touches nothing else of the slab.
int slab64_enqueue_row_digests(const Slab64& s, int g, int nx, int local_row, int rows, long long global_row, unsigned long long** dev)
{
  HIP_TRY(hipMalloc(dev, sizeof(unsigned long long) * static_cast<size_t>(rows)));
  hipLaunchKernelGGL(lbm64_row_digest_kernel, dim3(static_cast<unsigned>(rows)), dim3(kBlock), 0, s.stream,
                     reinterpret_cast<const unsigned long long*>(s.owned(g) + static_cast<size_t>(local_row) * static_cast<size_t>(nx)), s.ps,
                     static_cast<uint32_t>(nx), static_cast<unsigned long long>(global_row), *dev);
  HIP_TRY(hipGetLastError());
  return 0;
}

int slab64_collect_row_digests(const Slab64& s, unsigned long long* dev, int rows, unsigned long long* out)
{
  if (!dev) return 0;
  hipError_t e = hipMemcpyAsync(out, dev, sizeof(unsigned long long) * static_cast<size_t>(rows), hipMemcpyDeviceToHost, s.stream);
  if (e == hipSuccess) e = hipStreamSynchronize(s.stream);
  (void)hipFree(dev);
  HIP_TRY(e);
  return 0;
}

// What both digest entry points return from the row digests of their range: the wrap-around sum.
unsigned long long slab64_digest_sum(const unsigned long long* row_digests, int rows)
{
  unsigned long long sum = 0;
  for (int i = 0; i < rows; ++i) sum += row_digests[i];
  return sum;
}

// av_velocity's sum over the owned free cells of grid `g`: each block's sum added to *total, in block order (no subtotal of the slab:
// a caller that passes one accumulator from slab to slab adds every block of every slab to it serially).
int slab64_add_velocity_sum(const Slab64& s, int g, double* total)
{
  const int blocks = static_cast<int>(std::min<size_t>((s.ncells + kBlock - 1) / kBlock, 1024));
  double* part = nullptr;
  HIP_TRY(hipMalloc(&part, sizeof(double) * blocks));
  hipLaunchKernelGGL(lbm64_av_velocity_kernel, dim3(blocks), dim3(kBlock), 0, s.stream, s.owned(g), s.ps, s.mask, s.ncells, part);
  std::vector<double> host(blocks);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(host.data(), part, sizeof(double) * blocks, hipMemcpyDeviceToHost, s.stream);
  if (e == hipSuccess) e = hipStreamSynchronize(s.stream);
  (void)hipFree(part);
  HIP_TRY(e);
  for (double v : host) *total += v;
  return 0;
}

}  // namespace
