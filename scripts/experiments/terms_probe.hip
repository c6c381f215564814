// The SHIPPED sum|u| term code of the float kernels, finish_pair_lo<TERMS> (kernels/common.h, included below, not copied), on x-pairs of
// cells given in a file: one pair per lane, no streaming, no reductions.  tests/test_terms_cells.py feeds it lattice-like states, momenta
// of every binade down to the smallest denormal msq, states at rest, huge, infinite and NaN values, every skip and obstacle code, and
// holds every form of the term to tests/terms_ref.py.
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -std=c++17 -I include -I mpilattice-boltzmann_amd/csrc \
//         scripts/experiments/terms_probe.hip -o /tmp/terms_probe            (the library's flags: build.py COMMON)
//   /tmp/terms_probe IN OUT [IN OUT ...]
// IN:  uint64 n (pairs), float omega, float pad; n x 9 x 2 floats (population k of the pair's two cells: p[k].x, p[k].y);
//      n bytes mbits (obstacle bits of the pair); n bytes skip (bit j drops cell j from the pair's term).
// OUT: uint32 denormals_kept (1: a float product of the kernel that is a denormal number came out as one; 0: as zero), uint32 0;
//      then for each of the five instantiations the library builds, in the order kTermsDouble, kTermsFloat, kTermsCompensated,
//      kTermsCompensated | kTermsFused, kTermsDouble | kTermsFused: n doubles (the term finish_pair_lo returns);
//      then for each of them n floats (lo_sum, started from 0);
//      then n x 2 floats each: msq, rinv of relax_core (exact arithmetic), msq, rinv of the fused arithmetic,
//      the raw v_sqrt_f32 and the raw v_rsq_f32 of the exact msq.
// With --owned as the first argument each OUT gets a second file OUT.owned: the term of finish_pair_owned (the form lbm_multi_kernel's tall
//      geometry relaxes with), n doubles for each of <kTermsCompensated, kPairTermOwned>, <kTermsCompensated | kTermsFused, kPairTermOwned>,
//      <kTermsCompensated, kPairTermGuarded>, <kTermsCompensated | kTermsFused, kPairTermGuarded>, with `clean` what owned_substeps passes:
//      no lane of the pair's wave (64 consecutive pairs) drops a cell.  OUT itself is the same with and without the option.
// Exit status 0 only if every file was read, computed and written and no HIP call failed.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>
#include "../../mpilattice-boltzmann_amd/csrc/kernels/common.h"

#define HIP_OK(expr)                                                                                          \
  do {                                                                                                        \
    const hipError_t e_ = (expr);                                                                             \
    if (e_ != hipSuccess) {                                                                                   \
      std::fprintf(stderr, "terms_probe: %s: %s (%s:%d)\n", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
      return 2;                                                                                               \
    }                                                                                                         \
  } while (0)

constexpr int kForms = 5;
constexpr int kFloatPlanes = 6;   // msq, rinv, fused msq, fused rinv, raw sqrt, raw rsq: n x 2 floats each

template <int TERMS>
__device__ __forceinline__ void one_form(const f2 (&t)[9], uint32_t mbits, float omega, uint32_t skip, double* term, float* lo, size_t c)
{
  f2 out[9];
  float lo_sum = 0.0f;
  term[c] = finish_pair_lo<TERMS>(t, mbits, omega, /*tile_accel=*/false, /*accel=*/false, 0.0f, 0.0f, skip, out, lo_sum);
  lo[c] = lo_sum;
}

__global__ void __launch_bounds__(kBlock) terms_probe_kernel(const float* in, const unsigned char* mbits_in, const unsigned char* skip_in, size_t n, float omega,
                                                             float tiny, uint32_t* flags, double* term, float* lo, float* planes)
{
  const size_t c = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (c >= n) return;
  if (c == 0) flags[0] = (tiny * 0.5f != 0.0f) ? 1u : 0u;      // tiny = 2^-126 from the host: the product is a denormal number
  f2 t[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) t[k] = f2{in[(c * 9 + k) * 2], in[(c * 9 + k) * 2 + 1]};
  const uint32_t mbits = mbits_in[c] & 3u, skip = skip_in[c] & 3u;
  one_form<kTermsDouble>(t, mbits, omega, skip, term + 0 * n, lo + 0 * n, c);
  one_form<kTermsFloat>(t, mbits, omega, skip, term + 1 * n, lo + 1 * n, c);
  one_form<kTermsCompensated>(t, mbits, omega, skip, term + 2 * n, lo + 2 * n, c);
  one_form<kTermsCompensated | kTermsFused>(t, mbits, omega, skip, term + 3 * n, lo + 3 * n, c);
  one_form<kTermsDouble | kTermsFused>(t, mbits, omega, skip, term + 4 * n, lo + 4 * n, c);
  f2 o[9], msq, rinv, msq_fused, rinv_fused;
  relax_core<f2, false>(t, omega, o, msq, rinv);
  relax_core<f2, true>(t, omega, o, msq_fused, rinv_fused);
  const f2 vals[kFloatPlanes] = {msq, rinv, msq_fused, rinv_fused,
                                 f2{__builtin_amdgcn_sqrtf(msq.x), __builtin_amdgcn_sqrtf(msq.y)},
                                 f2{__builtin_amdgcn_rsqf(msq.x), __builtin_amdgcn_rsqf(msq.y)}};
#pragma unroll
  for (int v = 0; v < kFloatPlanes; ++v) {
    planes[(v * n + c) * 2] = vals[v].x;
    planes[(v * n + c) * 2 + 1] = vals[v].y;
  }
}

constexpr int kOwnedForms = 4;

__global__ void __launch_bounds__(kBlock) terms_probe_owned_kernel(const float* in, const unsigned char* mbits_in, const unsigned char* skip_in, size_t n, float omega, double* term)
{
  const size_t c = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (c >= n) return;
  f2 t[9], out[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) t[k] = f2{in[(c * 9 + k) * 2], in[(c * 9 + k) * 2 + 1]};
  const uint32_t mbits = mbits_in[c] & 3u, skip = skip_in[c] & 3u;
  const bool clean = __builtin_amdgcn_ballot_w64(skip != 0u) == 0ull;
  term[0 * n + c] = finish_pair_owned<kTermsCompensated, kPairTermOwned>(t, mbits, omega, skip, clean, out);
  term[1 * n + c] = finish_pair_owned<kTermsCompensated | kTermsFused, kPairTermOwned>(t, mbits, omega, skip, clean, out);
  term[2 * n + c] = finish_pair_owned<kTermsCompensated, kPairTermGuarded>(t, mbits, omega, skip, clean, out);
  term[3 * n + c] = finish_pair_owned<kTermsCompensated | kTermsFused, kPairTermGuarded>(t, mbits, omega, skip, clean, out);
}

struct Header { uint64_t n; float omega, pad; };

static int probe_file(const char* in_path, const char* out_path, bool owned)
{
  std::FILE* f = std::fopen(in_path, "rb");
  if (!f) { std::fprintf(stderr, "terms_probe: cannot open %s\n", in_path); return 1; }
  Header h;
  if (std::fread(&h, sizeof h, 1, f) != 1 || h.n == 0 || h.n > (1ull << 24)) {
    std::fprintf(stderr, "terms_probe: %s: bad header\n", in_path);
    std::fclose(f);
    return 1;
  }
  const size_t n = static_cast<size_t>(h.n);
  std::vector<float> pops(n * 18);
  std::vector<unsigned char> codes(n * 2);
  const bool read = std::fread(pops.data(), sizeof(float), n * 18, f) == n * 18 && std::fread(codes.data(), 1, n * 2, f) == n * 2;
  std::fclose(f);
  if (!read) { std::fprintf(stderr, "terms_probe: %s: short file\n", in_path); return 1; }
  float *d_in = nullptr, *d_lo = nullptr, *d_planes = nullptr;
  double* d_term = nullptr;
  unsigned char* d_codes = nullptr;
  uint32_t* d_flags = nullptr;
  HIP_OK(hipMalloc(&d_in, n * 18 * sizeof(float)));
  HIP_OK(hipMalloc(&d_codes, n * 2));
  HIP_OK(hipMalloc(&d_flags, 2 * sizeof(uint32_t)));
  HIP_OK(hipMalloc(&d_term, kForms * n * sizeof(double)));
  HIP_OK(hipMalloc(&d_lo, kForms * n * sizeof(float)));
  HIP_OK(hipMalloc(&d_planes, kFloatPlanes * n * 2 * sizeof(float)));
  HIP_OK(hipMemcpy(d_in, pops.data(), n * 18 * sizeof(float), hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(d_codes, codes.data(), n * 2, hipMemcpyHostToDevice));
  HIP_OK(hipMemset(d_flags, 0, 2 * sizeof(uint32_t)));
  HIP_OK(hipMemset(d_term, 0xff, kForms * n * sizeof(double)));
  HIP_OK(hipMemset(d_lo, 0xff, kForms * n * sizeof(float)));
  HIP_OK(hipMemset(d_planes, 0xff, kFloatPlanes * n * 2 * sizeof(float)));
  const unsigned blocks = static_cast<unsigned>((n + kBlock - 1) / kBlock);
  terms_probe_kernel<<<blocks, kBlock>>>(d_in, d_codes, d_codes + n, n, h.omega, 0x1p-126f, d_flags, d_term, d_lo, d_planes);
  HIP_OK(hipGetLastError());
  HIP_OK(hipDeviceSynchronize());
  uint32_t flags[2] = {0, 0};
  std::vector<double> term(kForms * n);
  std::vector<float> lo(kForms * n), planes(kFloatPlanes * n * 2);
  HIP_OK(hipMemcpy(flags, d_flags, sizeof flags, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(term.data(), d_term, term.size() * sizeof(double), hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(lo.data(), d_lo, lo.size() * sizeof(float), hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(planes.data(), d_planes, planes.size() * sizeof(float), hipMemcpyDeviceToHost));
  std::vector<double> owned_term;
  if (owned) {
    double* d_owned = nullptr;
    HIP_OK(hipMalloc(&d_owned, kOwnedForms * n * sizeof(double)));
    HIP_OK(hipMemset(d_owned, 0xff, kOwnedForms * n * sizeof(double)));
    terms_probe_owned_kernel<<<blocks, kBlock>>>(d_in, d_codes, d_codes + n, n, h.omega, d_owned);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    owned_term.resize(kOwnedForms * n);
    HIP_OK(hipMemcpy(owned_term.data(), d_owned, owned_term.size() * sizeof(double), hipMemcpyDeviceToHost));
    HIP_OK(hipFree(d_owned));
  }
  HIP_OK(hipFree(d_in));
  HIP_OK(hipFree(d_codes));
  HIP_OK(hipFree(d_flags));
  HIP_OK(hipFree(d_term));
  HIP_OK(hipFree(d_lo));
  HIP_OK(hipFree(d_planes));
  std::FILE* g = std::fopen(out_path, "wb");
  if (!g) { std::fprintf(stderr, "terms_probe: cannot write %s\n", out_path); return 1; }
  const bool wrote = std::fwrite(flags, sizeof(uint32_t), 2, g) == 2 && std::fwrite(term.data(), sizeof(double), term.size(), g) == term.size() &&
                     std::fwrite(lo.data(), sizeof(float), lo.size(), g) == lo.size() &&
                     std::fwrite(planes.data(), sizeof(float), planes.size(), g) == planes.size();
  if (std::fclose(g) != 0 || !wrote) { std::fprintf(stderr, "terms_probe: %s: short write\n", out_path); return 1; }
  if (owned) {
    const std::string owned_path = std::string(out_path) + ".owned";
    std::FILE* o = std::fopen(owned_path.c_str(), "wb");
    if (!o) { std::fprintf(stderr, "terms_probe: cannot write %s\n", owned_path.c_str()); return 1; }
    const bool wrote_owned = std::fwrite(owned_term.data(), sizeof(double), owned_term.size(), o) == owned_term.size();
    if (std::fclose(o) != 0 || !wrote_owned) { std::fprintf(stderr, "terms_probe: %s: short write\n", owned_path.c_str()); return 1; }
  }
  std::printf("terms_probe: %s: %zu pairs, float denormals %s\n", in_path, n, flags[0] ? "kept" : "flushed");
  return 0;
}

int main(int argc, char** argv)
{
  const bool owned = argc > 1 && std::strcmp(argv[1], "--owned") == 0;
  const int first = owned ? 2 : 1;
  if (argc - first < 2 || (argc - first) % 2 != 0) {
    std::fprintf(stderr, "usage: %s [--owned] IN OUT [IN OUT ...]\n", argv[0]);
    return 1;
  }
  for (int i = first; i + 1 < argc; i += 2) {
    const int rc = probe_file(argv[i], argv[i + 1], owned);
    if (rc != 0) return rc;
  }
  return 0;
}
