// The SHIPPED per-cell function of the double-precision mode, finish_cell_f64 (kernels/step64.h, included below, not copied), on cells
// given in a file: one cell per lane, no streaming, no sums.  tests/test_f64_cells.py feeds it populations the lattice never produces
// (denormal, zero, negative, huge, infinite, NaN; densities that cancel; roots and quotients of every binade) and compares every bit
// with the CPU restatement's f64_ref_cells (tests/f64_ref.c).
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -std=c++17 -I include -I mpilattice-boltzmann_amd/csrc \
//         scripts/experiments/cell64_probe.hip -o /tmp/cell64_probe          (the library's flags for lbm_f64.hip: build.py COMMON)
//   /tmp/cell64_probe IN OUT [IN OUT ...]
// IN:  uint64 n, double omega, double w1, double w2, n x 9 doubles (the populations that streamed in), n bytes blocked, n bytes accel.
// OUT: n x 9 doubles (finish_cell_f64's out[]), n doubles (the term it returns).
// Exit status 0 only if every file was read, computed and written and no HIP call failed.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <vector>
#include "../../mpilattice-boltzmann_amd/csrc/kernels/step64.h"

#define HIP_OK(expr)                                                                                          \
  do {                                                                                                        \
    const hipError_t e_ = (expr);                                                                             \
    if (e_ != hipSuccess) {                                                                                   \
      std::fprintf(stderr, "cell64_probe: %s: %s (%s:%d)\n", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
      return 2;                                                                                               \
    }                                                                                                         \
  } while (0)

__global__ void __launch_bounds__(kBlock) cell64_probe_kernel(const double* in, const unsigned char* blocked, const unsigned char* accel, size_t n,
                                                              double omega, double w1, double w2, double* out, double* term)
{
  const size_t c = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (c >= n) return;
  double t[9], o[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) t[k] = in[c * 9 + k];
  term[c] = finish_cell_f64(t, blocked[c] != 0, omega, accel[c] != 0, w1, w2, o);
#pragma unroll
  for (int k = 0; k < 9; ++k) out[c * 9 + k] = o[k];
}

struct Header { uint64_t n; double omega, w1, w2; };

static int probe_file(const char* in_path, const char* out_path)
{
  std::FILE* f = std::fopen(in_path, "rb");
  if (!f) { std::fprintf(stderr, "cell64_probe: cannot open %s\n", in_path); return 1; }
  Header h;
  if (std::fread(&h, sizeof h, 1, f) != 1 || h.n == 0 || h.n > (1ull << 26)) {
    std::fprintf(stderr, "cell64_probe: %s: bad header\n", in_path);
    std::fclose(f);
    return 1;
  }
  const size_t n = static_cast<size_t>(h.n);
  std::vector<double> pops(n * 9), res(n * 10);
  std::vector<unsigned char> flags(n * 2);
  const bool read = std::fread(pops.data(), sizeof(double), n * 9, f) == n * 9 && std::fread(flags.data(), 1, n * 2, f) == n * 2;
  std::fclose(f);
  if (!read) { std::fprintf(stderr, "cell64_probe: %s: short file\n", in_path); return 1; }
  double *d_in = nullptr, *d_res = nullptr;
  unsigned char* d_flags = nullptr;
  HIP_OK(hipMalloc(&d_in, n * 9 * sizeof(double)));
  HIP_OK(hipMalloc(&d_res, n * 10 * sizeof(double)));
  HIP_OK(hipMalloc(&d_flags, n * 2));
  HIP_OK(hipMemcpy(d_in, pops.data(), n * 9 * sizeof(double), hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(d_flags, flags.data(), n * 2, hipMemcpyHostToDevice));
  HIP_OK(hipMemset(d_res, 0xff, n * 10 * sizeof(double)));
  const unsigned blocks = static_cast<unsigned>((n + kBlock - 1) / kBlock);
  cell64_probe_kernel<<<blocks, kBlock>>>(d_in, d_flags, d_flags + n, n, h.omega, h.w1, h.w2, d_res, d_res + n * 9);
  HIP_OK(hipGetLastError());
  HIP_OK(hipDeviceSynchronize());
  HIP_OK(hipMemcpy(res.data(), d_res, n * 10 * sizeof(double), hipMemcpyDeviceToHost));
  HIP_OK(hipFree(d_in));
  HIP_OK(hipFree(d_res));
  HIP_OK(hipFree(d_flags));
  std::FILE* g = std::fopen(out_path, "wb");
  if (!g) { std::fprintf(stderr, "cell64_probe: cannot write %s\n", out_path); return 1; }
  const bool wrote = std::fwrite(res.data(), sizeof(double), n * 10, g) == n * 10;
  if (std::fclose(g) != 0 || !wrote) { std::fprintf(stderr, "cell64_probe: %s: short write\n", out_path); return 1; }
  std::printf("cell64_probe: %s: %zu cells\n", in_path, n);
  return 0;
}

int main(int argc, char** argv)
{
  if (argc < 3 || argc % 2 != 1) {
    std::fprintf(stderr, "usage: %s IN OUT [IN OUT ...]\n", argv[0]);
    return 1;
  }
  for (int i = 1; i + 1 < argc; i += 2) {
    const int rc = probe_file(argv[i], argv[i + 1]);
    if (rc != 0) return rc;
  }
  return 0;
}
