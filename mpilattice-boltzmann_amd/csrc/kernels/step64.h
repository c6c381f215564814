// step64.h — the double-precision mode: lbm_step_kernel_f64<CELLS, NT> (one step per launch, an x-pair or one cell per lane) and its
// small kernels (accelerate pre-pass, initial state, AoS<->SoA, observables, av_velocity, the row digests, the last fold of a run).
// Part of the translation unit lbm_f64.hip (device code of liblbm_d2q9.so, gfx950 only); include/lbm_d2q9_f64.h states the contract
// (the digests': include/lbm_d2q9_f64_digest.h).
// From common.h it takes kBlock, wave_sum, block_sum and lds_barrier, nothing of the float path's arithmetic.
#pragma once
#include "common.h"

namespace {

// (kPairCells = 2, one 16-byte access per population per lane: lbm_geometry.h, through common.h)

typedef double d2 __attribute__((ext_vector_type(2)));
typedef double d2u __attribute__((ext_vector_type(2), aligned(8)));   // 8-byte-aligned 16-byte access

// Layout: nine planes of ny*nx doubles, plane stride `ps` doubles (plane_stride_floats in elements, lbm_plan.cpp), two grids swapped per launch,
// the obstacle map as the float path's bitfield (bit c of the cell index).  Cell indices are 32-bit (lbm64_create refuses grids of
// 2^31 cells or more); every ADDRESS is formed in 64 bits: the nine planes of an 8192 x 8192 grid are 4.8 GB.
struct Step64Args {
  const double* src;           // source grid, plane 0 row 0
  double* dst;                 // destination grid
  const uint32_t* mask;        // obstacle bitfield
  size_t ps;                   // plane stride in doubles (even: the pair form's aligned accesses)
  uint32_t nx, ny;
  uint32_t units;              // x-pairs (CELLS = 2) or cells (CELLS = 1) of the grid
  int iters;                   // 256-unit chunks per block
  double omega;
  double accel_w1, accel_w2;   // d2q9-bgk.c:445-446 in double
  int accel_row;               // ny-2, or -1 on a run's last step: epilogue accelerate_flow for the NEXT step
  double* partials_out;        // this launch's per-block sums
  const double* prev_partials; // previous step's per-block sums, folded by block 0 of this launch
  int n_prev;
  double* sums;                // per-step totals of this run
  int* counter;                // index of the next entry of sums
};

__device__ __forceinline__ d2 load2(const double* p) { return *reinterpret_cast<const d2*>(p); }
__device__ __forceinline__ d2 load2u(const double* p) { return *reinterpret_cast<const d2u*>(p); }

template <bool NT>
__device__ __forceinline__ void store2(double* p, d2 v)
{
  if (NT) __builtin_nontemporal_store(v, reinterpret_cast<d2*>(p));
  else *reinterpret_cast<d2*>(p) = v;
}

template <bool NT>
__device__ __forceinline__ void store1(double* p, double v)
{
  if (NT) __builtin_nontemporal_store(v, p);
  else *p = v;
}

// One cell: moments, equilibrium and relaxation (d2q9-bgk.c:546-666) with every object a double — relax_core's exact form
// (kernels/common.h) word for word: opposite directions share "u*ic_sq" (one is the other's negation), "u*u*ic_sq - u_sq" and its
// product with "0.5*densinv*ic_sq" (equal), and "rho - a" stands for "rho + (-a)".  Nothing is contracted (-ffp-contract=off);
// 1.0 / rho is hipcc's IEEE division and sqrt its correctly rounded sequence (exact_math.h describes it).
// Returns the cell's sum|u| term sqrt(msq) * rinv (:667).
__device__ __forceinline__ double relax_cell_f64(const double (&t)[9], double omega, double (&o)[9])
{
  const double csq_inv = 3.0;                                         // :497
  const double w0 = 4.0 / 9.0, w1 = 1.0 / 9.0, w2 = 1.0 / 36.0;         // :499-501
  double rho = t[0] + t[1];                                           // :546-554, :570-574, :576-580 side by side
  double mx = t[1] + t[5];
  double my = t[2] + t[5];
  rho += t[2]; mx += t[8]; my += t[6];
  rho += t[3]; mx -= t[3]; my -= t[4];
  rho += t[4]; mx -= t[6]; my -= t[7];
  rho += t[5]; mx -= t[7]; my -= t[8];
  rho += t[6];
  const double mxx = mx * mx, myy = my * my;
  const double e5 = mx + my, e8 = mx - my;                            // :600,603 (u[7] = -e5, u[6] = -e8)
  rho += t[7];
  const double msq = mxx + myy;                                       // :589
  const double a[4] = {mx * csq_inv, my * csq_inv, e5 * csq_inv, e8 * csq_inv};   // :610-617 for k = 1, 2, 5, 8
  rho += t[8];
  const double rinv = 1.0 / rho;                                      // :561
  double d[4] = {a[0] * mx, a[1] * my, a[2] * e5, a[3] * e8};         // :624-631
  const double h = 0.5 * rinv * csq_inv;                              // "0.5*densinv*ic_sq" of :638-646
#pragma unroll
  for (int i = 0; i < 4; ++i) d[i] = h * (d[i] - msq);
  double s[9];                                                        // :638-646
  s[0] = rho - h * msq;
  s[1] = rho + a[0]; s[3] = rho - a[0];
  s[2] = rho + a[1]; s[4] = rho - a[1];
  s[5] = rho + a[2]; s[7] = rho - a[2];
  s[8] = rho + a[3]; s[6] = rho - a[3];
  s[1] += d[0]; s[3] += d[0]; s[2] += d[1]; s[4] += d[1];
  s[5] += d[2]; s[7] += d[2]; s[8] += d[3]; s[6] += d[3];
  s[0] = w0 * s[0];
#pragma unroll
  for (int k = 1; k < 9; ++k) s[k] = ((k < 5) ? w1 : w2) * s[k];
#pragma unroll
  for (int k = 0; k < 9; ++k) o[k] = t[k] + omega * (s[k] - t[k]);    // :658-666
  return sqrt(msq) * rinv;                                            // :667
}

// Relaxation / bounce-back select (d2q9-bgk.c:687-695), then the NEXT step's accelerate_flow (:457-469) where `accel`.
__device__ __forceinline__ double finish_cell_f64(const double (&t)[9], bool blocked, double omega, bool accel, double w1, double w2, double (&out)[9])
{
  double o[9];
  const double term = relax_cell_f64(t, omega, o);
  out[0] = blocked ? t[0] : o[0];
  out[1] = blocked ? t[3] : o[1];
  out[2] = blocked ? t[4] : o[2];
  out[3] = blocked ? t[1] : o[3];
  out[4] = blocked ? t[2] : o[4];
  out[5] = blocked ? t[7] : o[5];
  out[6] = blocked ? t[8] : o[6];
  out[7] = blocked ? t[5] : o[7];
  out[8] = blocked ? t[6] : o[8];
  if (accel && !blocked && out[3] - w1 > 0.0 && out[6] - w2 > 0.0 && out[7] - w2 > 0.0) {
    out[1] += w1; out[5] += w2; out[8] += w2;
    out[3] -= w1; out[6] -= w2; out[7] -= w2;
  }
  return blocked ? 0.0 : term;
}

// Rows a destination row pulls from (d2q9-bgk.c:511-512 with one rank: periodic), as element offsets of their first cell.
struct Rows64 { size_t here, south, north; };
__device__ __forceinline__ Rows64 rows_of(uint32_t nx, uint32_t ny, uint32_t y)
{
  Rows64 r;
  r.here = static_cast<size_t>(y) * nx;
  r.south = static_cast<size_t>(y > 0 ? y - 1 : ny - 1) * nx;
  r.north = static_cast<size_t>(y + 1 < ny ? y + 1 : 0) * nx;
  return r;
}
__device__ __forceinline__ Rows64 rows_of(const Step64Args& a, uint32_t y) { return rows_of(a.nx, a.ny, y); }

// The pull of an x-pair (d2q9-bgk.c:530-538; nx even): the two cells at (y, x0), (y, x0 + 1), x0 even.  Populations 0, 2, 4 come by
// 16-byte aligned loads, the east- and west-moving ones by loads shifted one double; the pair at x0 == 0 fetches its west column from
// x = nx-1 and the pair at x0 == nx-2 its east column from x = 0, each lane for itself (nx = 2: both on the one lane of a row).
__device__ __forceinline__ void pull_pair_f64(const double* src, size_t ps, uint32_t nx, const Rows64& r, uint32_t x0, d2 (&p)[9])
{
  const double* here = src + r.here + x0;
  const double* south = src + r.south + x0;
  const double* north = src + r.north + x0;
  p[0] = load2(here);
  p[2] = load2(south + 2 * ps);
  p[4] = load2(north + 4 * ps);
  p[1] = load2u(here + ps - 1);
  p[5] = load2u(south + 5 * ps - 1);
  p[8] = load2u(north + 8 * ps - 1);
  p[3] = load2u(here + 3 * ps + 1);
  p[6] = load2u(south + 6 * ps + 1);
  p[7] = load2u(north + 7 * ps + 1);
  if (x0 == 0) {                               // x_w wraps to nx-1 (:529)
    const size_t last = nx - 1;
    p[1].x = src[ps + r.here + last];
    p[5].x = src[5 * ps + r.south + last];
    p[8].x = src[8 * ps + r.north + last];
  }
  if (x0 == nx - kPairCells) {                 // x_e wraps to 0 (:527-528)
    p[3].y = src[3 * ps + r.here];
    p[6].y = src[6 * ps + r.south];
    p[7].y = src[7 * ps + r.north];
  }
}

// The x-pair form (nx even): pull_pair_f64, then the two cells one after the other.
template <bool NT>
__device__ __forceinline__ double step_pair_f64(const Step64Args& a, uint32_t pair)
{
  const uint32_t c = pair * kPairCells;
  const uint32_t y = c / a.nx;
  const uint32_t x0 = c - y * a.nx;
  const size_t ps = a.ps;
  const Rows64 r = rows_of(a, y);
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

// One cell per lane (odd nx).
template <bool NT>
__device__ __forceinline__ double step_cell_f64(const Step64Args& a, uint32_t cell)
{
  const uint32_t y = cell / a.nx;
  const uint32_t x = cell - y * a.nx;
  const size_t ps = a.ps;
  const Rows64 r = rows_of(a, y);
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

// Block 0 of every step launch does no lattice work: it folds the PREVIOUS step's per-block sums into sums[counter++]
// (d2q9-bgk.c:367) while the other blocks stream (the float path's fold_previous, kernels/step.h).
__device__ __forceinline__ void fold_previous_f64(const Step64Args& a, double* red)
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

// The one-step kernel of the double-precision mode, one definition for its four instantiations (kStep64Kernels, lbm_f64.hip):
// CELLS = 2 (step_pair_f64) or 1 (step_cell_f64), NT = non-temporal stores.
// Grid: one fold block (block 0, dispatched first), then ceil(units / (256 * iters)) work blocks of 256 lanes; work block b owns
// `iters` consecutive 256-unit chunks.  A lane adds its units' terms serially, block_sum joins the lanes in a fixed tree.
template <int CELLS, bool NT>
__global__ void __launch_bounds__(kBlock) lbm_step_kernel_f64(const Step64Args a)
{
  static_assert(CELLS == 1 || CELLS == kPairCells, "one cell or one x-pair per lane");
  __shared__ double red[kBlock / 64];
  if (blockIdx.x == 0) { fold_previous_f64(a, red); return; }
  const uint32_t wblock = blockIdx.x - 1;   // work block index
  double acc = 0.0;
  const uint32_t base = wblock * static_cast<uint32_t>(a.iters) * kBlock + threadIdx.x;    // < units + 256 * iters < 2^31 + 2^18
  for (int i = 0; i < a.iters; ++i) {
    const uint32_t unit = base + static_cast<uint32_t>(i) * kBlock;
    if (unit < a.units) {
      if constexpr (CELLS == 1) acc += step_cell_f64<NT>(a, unit);
      else acc += step_pair_f64<NT>(a, unit);
    }
  }
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) a.partials_out[wblock] = acc;
}

// The last launch's partials, after the loop: one block.  nvecs vectors of n sums, one per step of that launch (the one-step kernel: 1;
// lbm_tile_kernel_f64: its steps), each summed as the one vector always was.
__global__ void __launch_bounds__(kBlock) lbm64_fold_kernel(const double* partials, int n, int nvecs, double* sums, int* counter)
{
  __shared__ double red[kBlock / 64];
  const int first = threadIdx.x == 0 ? *counter : 0;                 // lane 0 alone reads and writes it
  for (int v = 0; v < nvecs; ++v) {
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += kBlock) s += partials[static_cast<size_t>(v) * n + i];
    s = block_sum(s, red);
    if (threadIdx.x == 0) sums[first + v] = s;
  }
  if (threadIdx.x == 0) *counter = 0;                               // 0: the next run starts counting again
}

// accelerate_flow (d2q9-bgk.c:442-478) in place on one row: before the first step of a run.
__global__ void lbm64_accelerate_kernel(double* grid, size_t ps, const uint32_t* mask, uint32_t nx, uint32_t row, double w1, double w2)
{
  const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= nx) return;
  const uint32_t c = row * nx + x;
  if ((mask[c >> 5] >> (c & 31u)) & 1u) return;
  double* f = grid + c;
  const double f3 = f[3 * ps], f6 = f[6 * ps], f7 = f[7 * ps];
  if (f3 - w1 > 0.0 && f6 - w2 > 0.0 && f7 - w2 > 0.0) {
    f[1 * ps] += w1; f[5 * ps] += w2; f[8 * ps] += w2;
    f[3 * ps] = f3 - w1; f[6 * ps] = f6 - w2; f[7 * ps] = f7 - w2;
  }
}

// Initial state (d2q9-bgk.c:880-902).
__global__ void lbm64_init_kernel(double* grid, size_t ps, size_t ncells, double w0, double w1, double w2)
{
  const size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= ncells) return;
  grid[i] = w0;
#pragma unroll
  for (int k = 1; k < 5; ++k) grid[k * ps + i] = w1;
#pragma unroll
  for (int k = 5; k < 9; ++k) grid[k * ps + i] = w2;
}

// AoS (the reference's t_speed, doubles) <-> SoA planes, cells [0, n) of `grid` (already offset to the first cell wanted).  Bits are moved
// as 64-bit integers: no arithmetic instruction sees a NaN payload or a denormal.
__global__ void lbm64_aos_to_soa_kernel(const unsigned long long* aos, unsigned long long* grid, size_t ps, size_t n)
{
  const size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n * 9) return;
  const size_t c = i / 9;
  grid[(i - c * 9) * ps + c] = aos[i];
}

__global__ void lbm64_soa_to_aos_kernel(const unsigned long long* grid, unsigned long long* aos, size_t ps, size_t n)
{
  const size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n * 9) return;
  const size_t c = i / 9;
  aos[i] = grid[(i - c * 9) * ps + c];
}

// av_velocity (d2q9-bgk.c:716-751) in double; cell c of `grid` is bit c of the bitfield.
__global__ void __launch_bounds__(kBlock) lbm64_av_velocity_kernel(const double* grid, size_t ps, const uint32_t* mask, size_t ncells, double* partials)
{
  __shared__ double red[kBlock / 64];
  double acc = 0.0;
  for (size_t c = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x; c < ncells; c += static_cast<size_t>(gridDim.x) * kBlock) {
    if ((mask[c >> 5] >> (c & 31)) & 1u) continue;
    double f[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) f[k] = grid[k * ps + c];
    double rho = 0.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) rho += f[k];                                   // :724-729
    const double ux = (f[1] + f[5] + f[8] - (f[3] + f[6] + f[7])) / rho;       // :732-738
    const double uy = (f[2] + f[5] + f[6] - (f[4] + f[7] + f[8])) / rho;       // :740-746
    acc += sqrt((ux * ux) + (uy * uy));                                        // :748
  }
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) partials[blockIdx.x] = acc;
}

// write_values()' per-cell arithmetic for a fluid cell (d2q9-bgk.c:1084-1111) in double on cells [0, n) of `grid`:
// obs[4c..4c+3] = {u_x, u_y, u, pressure}.  As in the float path's lbm_observables_kernel, a NaN produced here from non-NaN inputs
// (rho = 0) gets the sign x86 gives a generated NaN, which is what the reference's fprintf shows ("-NAN").
__global__ void __launch_bounds__(kBlock) lbm64_observables_kernel(const double* grid, size_t ps, size_t n, double* obs)
{
  const size_t c = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (c >= n) return;
  double f[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) f[k] = grid[k * ps + c];
  double rho = 0.0;
  bool nan_in = false;
#pragma unroll
  for (int k = 0; k < 9; ++k) { rho += f[k]; nan_in |= (f[k] != f[k]); }        // :1084-1090
  double o[4];
  o[0] = (f[1] + f[5] + f[8] - (f[3] + f[6] + f[7])) / rho;                     // :1093-1099
  o[1] = (f[2] + f[5] + f[6] - (f[4] + f[7] + f[8])) / rho;                     // :1101-1107
  o[2] = sqrt((o[0] * o[0]) + (o[1] * o[1]));                                   // :1109
  o[3] = rho * (1.0 / 3.0);                                                     // :1111, c_sq of :1040
  if (!nan_in) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (o[j] != o[j]) o[j] = __longlong_as_double(static_cast<long long>(0xFFF8000000000000ull));
  }
  *reinterpret_cast<d2*>(obs + 4 * c) = d2{o[0], o[1]};
  *reinterpret_cast<d2*>(obs + 4 * c + 2) = d2{o[2], o[3]};
}

// The state digest of include/lbm_d2q9_f64_digest.h, one per row: block b digests the nx cells of row b of `grid` (already offset to
// the first cell of the first row wanted), which is row global_row0 + b of the whole grid, into row_digests[b].  The planes are read as
// 64-bit integers, like the AoS<->SoA kernels: no arithmetic instruction sees a NaN payload or a denormal.  Every index is formed in
// 64 bits: (row * nx + x) * 9 + k passes 2^32 long before the cell index does.  Lanes stride along x (coalesced per plane), the wave's
// lanes join by the butterfly, the waves' sums meet in LDS; integer sums do not depend on the order, and there is no atomic.  Reads
// the grid, writes row_digests, nothing else.
__global__ void __launch_bounds__(kBlock) lbm64_row_digest_kernel(const unsigned long long* grid, size_t ps, uint32_t nx, unsigned long long global_row0,
                                                                  unsigned long long* row_digests)
{
  __shared__ unsigned long long red[kBlock / 64];
  const unsigned long long* row = grid + static_cast<size_t>(blockIdx.x) * nx;
  const unsigned long long cell0 = (global_row0 + blockIdx.x) * static_cast<unsigned long long>(nx);   // the row's first cell in the whole grid
  unsigned long long h = 0;
  for (uint32_t x = threadIdx.x; x < nx; x += kBlock) {              // nx < 2^31: x + kBlock does not wrap
    unsigned long long f[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) f[k] = row[k * ps + x];
    const unsigned long long idx0 = (cell0 + x) * 9ull;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      unsigned long long z = f[k] ^ ((idx0 + static_cast<unsigned long long>(k)) * 0x9E3779B97F4A7C15ull);
      z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
      z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
      h += z ^ (z >> 31);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) h += __shfl_xor(h, off, 64);   // every lane of the wave is back here: the loop has ended
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = h;
  lds_barrier();
  if (threadIdx.x == 0) {
    unsigned long long t = red[0];
#pragma unroll
    for (int w = 1; w < kBlock / 64; ++w) t += red[w];
    row_digests[blockIdx.x] = t;
  }
}

}  // namespace
