// cols64.h — column-partitioned runs of the double-precision mode, several steps per exchange: lbm_cols_multi_kernel_f64<K, NT, FULL, EDGE>,
// the column-block form of lbm_multi_kernel_f64 (kernels/multi64.h: up to K steps of one rank per launch), lbm64_push_ghost_cols_kernel,
// which stores a rank's G first and G last owned columns into its neighbours' ghost columns, and the small kernels that read and write
// a block whose pitch is not its width (accelerate pre-pass, AoS <-> SoA, observables, av_velocity, partial row digests).
// Part of the translation unit lbm_cols64.hip (gfx950 only, -ffp-contract=off); include/lbm_d2q9_f64_cols.h states the contract.
//
// A FULL DEFINITION, not a shared body, as kernels/rows_multi64.h is and for the reason that file gives: a body shared with
// lbm_multi_kernel_f64 changes the device assembly of lbm_f64.hip.  multi64.h and rows_multi64.h stay as they are and this file restates
// the kernel a second time.  Whoever changes one of the three changes the others: tests/test_f64_cols.py holds all three to the same bits.
//
// What is lbm_multi_kernel_f64's, unchanged: the 32 x 16 tile per block of kMulti64Lanes lanes, the launch bounds, the in-place LDS frame
// with its reduction scratch and flag bytes (bit 0 obstacle, 1 owned, 2 on row ny-2), the sub-steps and their barriers, finish_cell_f64,
// one accumulator per sub-step, wave_sum_vec4, the fold block (block 0), the layout of partials_out and the DPP pair exchange of the
// final store.
//
// What differs, in sub-step 1, in the final store and in the mask index only:
//   storage         a rank's grids are nine planes of ny STORAGE rows of pitch = nxl + 2 G doubles, G = 2 ceil(K / 2) ghost columns on
//                   each side (K of a full launch; the ghost rounded up to even, so that pitch is even: every x-pair is 16-byte aligned
//                   and its two obstacle bits sit in one word).  Owned column x is storage column G + x.  There are no ghost rows.
//   columns do not wrap.  The pair (tile-local rx) of the tile at owned column x0, grown by gx = multi_ex(e), is storage column
//                   sx = G + x0 - gx + rx.
//   rows wrap on ny exactly as in lbm_multi_kernel_f64: rows_of(pitch, ny, y) on the global row y, which is the storage row.
//   row ny-2        is told by that row y, so every frame copy and ghost-column copy of it is accelerated between sub-steps.
//   obstacle bits   come from the rank's WINDOW bitfield over its storage cells (the whole grid's columns x0_r - G .. x0_r + nxl + G - 1,
//                   periodic in x): bit c of the storage cell c = y * pitch + sx.  pitch and sx are even: both bits in one word.
//   pull_pair_f64   is called with the pitch as its nx.
//
// THE BOUND ARGUMENT (e = k - 1 <= K - 1 the growth of sub-step 1 in a launch of k steps, gx = multi_ex(e) = e or e + 1, 0 <= x0 <= nxl - 32):
//   storage columns sx = G + x0 - gx + rx with 0 <= rx <= 30 + 2 gx, so G - gx <= sx <= nxl + G + gx - 2.  multi_ex(K - 1) = 2 for K = 2, 3 and
//                   4 for K = 4, G = 2, 4, 4: gx <= G for every K, hence 0 <= sx and sx + 1 <= pitch - 1: a pair lies inside its storage row.
//   what is needed  a cell that sub-step 1 must get right lies at distance <= e from the tile and pulls from distance <= e + 1 <= K <= G:
//                   from storage columns >= G - K >= 0 and <= nxl + G + K - 1 <= pitch - 1.  Every value that can reach an owned cell
//                   comes from a real storage cell, and the ghost columns it comes from were pushed whole (G >= K columns) before the launch.
//   what is not     where gx = e + 1 (e odd) the aligned pair also computes one cell at distance gx.  Only there — gx = G, a tile on the
//                   block's first or last column — its west read falls on storage column -1 or its east read on column pitch.
//                   pull_pair_f64's own wrap (x0 == 0, x0 == nx - 2 with nx = pitch) turns that into the other end of the same storage
//                   row, which is in bounds; the unconditional shifted loads beside it read one double before or behind the row, inside
//                   the planes' guards, exactly as the whole grid's kernel does.  That cell sits on the outermost column of the frame
//                   region of sub-step 1: sub-step 2 reads the region grown by e - 1 and one cell around it, which ends at distance e.
//                   It is never read again, never stored and never counted (multi_ex's comment in lbm_geometry.h says the same of the
//                   whole grid's kernel, whose outermost column is as dead).
//   rows            0 <= y < ny after one correction (ny >= 16 > e), and rows_of wraps the rows a pull reads: storage rows only.
//   stores          go to owned cells: storage rows y0 + ry < ny, storage columns G + x0 + rx in G .. G + nxl - 1.
//   cell indices    y * pitch + sx < ny * pitch, which the plan holds below 2^31 - 4096.
//
// EDGE: multi64.h's edge-tile form on a rank's block.  ceil(nxl / TX) x ceil(ny / TY) tiles on a block they do not cover exactly
// (nxl even and >= TX, ny >= TY).  Tile (tx, ty) starts at owned column x0 = min(TX tx, nxl - TX) and row y0 = min(TY ty, ny - TY) and
// owns only its cells at tile-local x >= TX tx - x0, y >= TY ty - y0.  x0 stays even and within 0 .. nxl - TX: the bounds above hold.
#pragma once
#include <type_traits>

#include "multi64.h"

namespace {

struct ColsMulti64Args {
  const double* src;           // source grid, plane 0 storage row 0 storage column 0
  double* dst;                 // destination grid
  const uint32_t* mask;        // the rank's window bitfield: bit c of the storage cell c
  size_t ps;
  int nxl, ny;                 // owned columns of the rank; rows (of the whole grid: every rank owns every row)
  int pitch;                   // doubles of a storage row: nxl + 2 ghost
  int ghost;                   // ghost columns on each side of the owned ones: G
  int tiles_x;                 // nxl / TX (EDGE: rounded up)
  int ksteps;                  // 1..K steps in this launch (FULL: K)
  double omega, accel_w1, accel_w2;
  int accel_row;               // ny-2
  int accel_last;              // apply accelerate_flow after the LAST sub-step too (another step follows)
  double* partials_out;        // [ksteps][tiles of this rank]
  const double* prev_partials; // previous launch: [n_prev_vecs][n_prev]
  int n_prev, n_prev_vecs;
  double* sums;                // this rank's per-step totals of this run
  int* counter;
};

// FULL: the launch makes exactly K steps, so every region size is a compile-time constant.
// EDGE: the edge-tile form described above.
template <int K, bool NT, bool FULL, bool EDGE>
__global__ void __launch_bounds__(kMulti64Lanes, kMulti64WavesPerSimd) lbm_cols_multi_kernel_f64(const ColsMulti64Args a)
{
  static_assert(multi64_k_ok(K), "unsupported steps per launch");
  constexpr int TX = kMulti64TX, TY = kMulti64TY, FX = multi64_frame_x(K), FY = multi64_frame_y(K), FC = FX * FY;
  constexpr int EX = multi_ex(K - 1), EY = K - 1, kLanes = kMulti64Lanes, kWaves = kLanes / 64;
  static_assert((TX / 2 + multi_ex(K - 1)) * FY <= kLanes, "sub-step 1 deals a lane at most one x-pair");
  static_assert(multi_ex(K - 1) <= 2 * ((K + 1) / 2), "the grown tile of sub-step 1 lies inside the ghost columns: gx <= G");
  extern __shared__ __attribute__((aligned(16))) double frame64[];     // [9][FC] doubles, reduction scratch, flag bytes
  double* red = frame64 + 9 * FC;                                       // [kMulti64Accs][kWaves]
  uint8_t* cell_flags = reinterpret_cast<uint8_t*>(red + kMulti64Accs * kWaves);   // per frame cell: bit 0 obstacle, 1 owned, 2 on row ny-2
  const int tid = threadIdx.x;

  if (blockIdx.x == 0) {
    // fold block: the previous launch's per-tile sums of this rank, one vector per step, into sums[counter ...]
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
  const int k_total = FULL ? K : a.ksteps;
  const size_t ps = a.ps;
  // the tile's first owned column and row (EDGE: shifted back inside the block)
  const int x0 = EDGE ? min(tx * TX, a.nxl - TX) : tx * TX, own_x = EDGE ? tx * TX - x0 : 0;
  const int y0 = EDGE ? min(ty * TY, a.ny - TY) : ty * TY, own_y = EDGE ? ty * TY - y0 : 0;

  double acc[kMulti64Accs];
#pragma unroll
  for (int i = 0; i < kMulti64Accs; ++i) acc[i] = 0.0;

  // ---- sub-step 1: an aligned x-pair of the grown tile per lane, pulled from the source grid.  pitch, ghost, TX and multi_ex are even,
  // so a pair's first storage cell has an even index.
  {
    const int e = k_total - 1, gx = multi_ex(e);
    const int wp = TX / 2 + gx, hy = TY + 2 * e;               // pairs per row, rows
    const bool last = !FULL && e == 0;
    if (tid < wp * hy) {
      const int ry = FULL ? tid / wp : small_div(tid, wp), rx = 2 * (tid - ry * wp);
      const int sx = a.ghost + x0 - gx + rx;                                               // storage column: ghost - gx .. pitch - ghost + gx - 2, and gx <= ghost: no wrap
      int y = y0 - e + ry;  if (y < 0) y += a.ny; else if (y >= a.ny) y -= a.ny;           // -e .. ny + e - 1, and ny >= TY > e
      const uint32_t cell = static_cast<uint32_t>(y) * static_cast<uint32_t>(a.pitch) + static_cast<uint32_t>(sx);
      const uint32_t mbits = (a.mask[cell >> 5] >> (cell & 31u)) & 3u;                       // cell is even: both bits in one word
      const bool on_row = y == a.accel_row;                                                  // the owned cells of row ny-2 and every ghost-column or ring copy of them
      const bool accel = on_row && (!last || a.accel_last);
      const bool owned = rx >= gx + own_x && rx < gx + TX && ry >= e + own_y && ry < e + TY;   // both cells of a pair, or neither
      d2 p[9];
      pull_pair_f64(a.src, ps, static_cast<uint32_t>(a.pitch), rows_of(static_cast<uint32_t>(a.pitch), static_cast<uint32_t>(a.ny), static_cast<uint32_t>(y)), static_cast<uint32_t>(sx), p);
      if (last) {
        d2 out[9];
#pragma unroll
        for (int j = 0; j < kPairCells; ++j) {
          double t[9], q[9];
#pragma unroll
          for (int k = 0; k < 9; ++k) t[k] = p[k][j];
          const double term = finish_cell_f64(t, (mbits >> j) & 1u, a.omega, accel, a.accel_w1, a.accel_w2, q);
          if (!EDGE || owned) acc[0] += term;                                                // e = 0: every cell is owned, except in a shifted tile
#pragma unroll
          for (int k = 0; k < 9; ++k) out[k][j] = q[k];
        }
        double* d = a.dst + cell;                                                            // e = 0: sx = ghost + x0 + rx, an owned column
        if (!EDGE || owned) {
#pragma unroll
          for (int k = 0; k < 9; ++k) store2<NT>(d + k * ps, out[k]);
        }
      } else {
        const int c = (EY - e + ry) * FX + (EX - gx + rx);
        const uint32_t common = (owned ? 2u : 0u) | (on_row ? 4u : 0u);
#pragma unroll
        for (int j = 0; j < kPairCells; ++j) {
          double t[9], q[9];
#pragma unroll
          for (int k = 0; k < 9; ++k) t[k] = p[k][j];
          const double term = finish_cell_f64(t, (mbits >> j) & 1u, a.omega, accel, a.accel_w1, a.accel_w2, q);
          if (owned) acc[0] += term;                                                         // owned cells only (:667); a blocked cell's term is 0
#pragma unroll
          for (int k = 0; k < 9; ++k) frame64[k * FC + c + j] = q[k];
        }
        *reinterpret_cast<uint16_t*>(cell_flags + c) = static_cast<uint16_t>(((mbits & 1u) | common) | ((((mbits >> 1) & 1u) | common) << 8));
      }
    }
    if (!last) lds_barrier();
  }

  // ---- sub-steps 2 .. k on the frame; S is a compile-time constant (the sub-steps are unrolled: the accumulator slot folds)
  auto substep = [&](auto sc) __attribute__((always_inline)) {
    constexpr int S = decltype(sc)::value;
    const int e = k_total - S;                   // cells still needed after this sub-step: the owned tile grown by e
    const int w = TX + 2 * e, n = w * (TY + 2 * e);
    const bool last = e == 0;
    const bool accel_now = !last || a.accel_last;
    double out[2][9];
    int at[2];
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int i = tid + it * kLanes;
      at[it] = -1;
      if (it == 0 ? (FULL || i < n) : (!last && i < n)) {              // item 0 of a FULL launch: n >= lanes
        const int ry = FULL ? i / w : small_div(i, w), rx = i - ry * w;
        const int c = (EY - e + ry) * FX + (EX - e + rx);
        const uint32_t fl = cell_flags[c];
        double t[9];                                                                   // d2q9-bgk.c:530-538
        t[0] = frame64[0 * FC + c];          t[1] = frame64[1 * FC + c - 1];      t[2] = frame64[2 * FC + c - FX];
        t[3] = frame64[3 * FC + c + 1];      t[4] = frame64[4 * FC + c + FX];     t[5] = frame64[5 * FC + c - FX - 1];
        t[6] = frame64[6 * FC + c - FX + 1]; t[7] = frame64[7 * FC + c + FX + 1]; t[8] = frame64[8 * FC + c + FX - 1];
        const double term = finish_cell_f64(t, (fl & 1u) != 0u, a.omega, accel_now && (fl & 4u) != 0u, a.accel_w1, a.accel_w2, out[it]);
        if (fl & 2u) acc[S - 1] += term;
        at[it] = c;
      }
    }
    if (!last) {
      lds_barrier();                             // every lane has read all its items: the frame may change
#pragma unroll
      for (int it = 0; it < 2; ++it) {
        if (at[it] >= 0) {
#pragma unroll
          for (int k = 0; k < 9; ++k) frame64[k * FC + at[it]] = out[it][k];
        }
      }
      lds_barrier();
    } else {
      // the owned tile, lane tid its cell tid: lanes 2m and 2m + 1 are x-neighbours.  The even lane stores the pair's populations
      // 0, 2, 4, 6, 8, the odd lane 1, 3, 5, 7: each sends the other the half it does not store (bits, by a DPP move).
      const int ry = tid / TX, rx = tid - ry * TX;
      const bool odd = (tid & 1) != 0;
      const bool stores = !EDGE || (rx >= own_x && ry >= own_y);      // owned (own_x is even: both lanes of a pair, or neither); every lane makes the exchange
      double* d = a.dst + (static_cast<size_t>(y0 + ry) * a.pitch + static_cast<size_t>(a.ghost + x0 + (rx & ~1)));   // owned column x0 + rx of row y0 + ry
#pragma unroll
      for (int j = 0; j < 5; ++j) {
        constexpr int kLastOdd = 7;
        const int ke = 2 * j, ko = j < 4 ? 2 * j + 1 : kLastOdd;
        const double mine = odd ? out[0][ko] : out[0][ke];
        const double send = odd ? out[0][ke] : out[0][ko];
        const double recv = dpp_full<0xB1>(send);                      // quad_perm [1,0,3,2]: lane l ^ 1
        const d2 v = odd ? d2{recv, mine} : d2{mine, recv};
        if ((j < 4 || !odd) && stores) store2<NT>(d + static_cast<size_t>(odd ? ko : ke) * ps, v);
      }
    }
  };
  if (2 <= k_total) substep(std::integral_constant<int, 2>{});
  if constexpr (K >= 3) { if (3 <= k_total) substep(std::integral_constant<int, 3>{}); }
  if constexpr (K >= 4) { if (4 <= k_total) substep(std::integral_constant<int, 4>{}); }

  // per-step sums over the owned cells of this tile: one halving butterfly per wave (common.h), then one lane per step over the waves
  const int ntiles = gridDim.x - 1;
  const double wsum = wave_sum_vec4(acc[0], acc[1], acc[2], acc[3]);
  if ((tid & 15) == 0) red[wave_sum_slot<4>(tid & 63) * kWaves + (tid >> 6)] = wsum;
  lds_barrier();                 // LDS only: no wait for the tile's global stores
  if (tid < k_total) {
    double t = red[tid * kWaves];
    for (int wv = 1; wv < kWaves; ++wv) t += red[tid * kWaves + wv];
    a.partials_out[static_cast<size_t>(tid) * ntiles + tile] = t;
  }
}

// The exchange of one rank after a launch: all nine planes, every row, of its first `ghost` owned columns (storage columns ghost ..
// 2 ghost - 1) into the EAST ghost columns of the rank to its west (that rank's storage columns ghost + west_nxl ..), and of its last
// `ghost` owned columns (storage columns nxl .. nxl + ghost - 1) into the WEST ghost columns of the rank to its east (its storage
// columns 0 .. ghost - 1), in the neighbour's grid of the same parity.  Sources are owned columns, targets ghost columns: disjoint even
// where the rank is its own neighbour (nxl >= 32 > 2 ghost).  Ranks may differ in width: the targets are formed from the NEIGHBOUR's
// pitch, plane stride and owned columns.  A neighbour's grid may be another device's memory (peer access): plain 16-byte vector stores
// (ghost, nxl and every pitch are even, so every access starts at an even double).  Nothing waits on the device.
struct ColsPushGhost64Args {
  const double* grid;          // this rank's grid just written, plane 0 storage row 0
  size_t ps;
  uint32_t pitch, nxl, ny, ghost;
  double* west;                // the rank to the west: the same grid of it, its plane stride, pitch and owned columns
  size_t west_ps;
  uint32_t west_pitch, west_nxl;
  double* east;                // the rank to the east
  size_t east_ps;
  uint32_t east_pitch;
};

// Grid: x over the ny * ghost / 2 accesses of one plane and way (< 2^31: ny * pitch is), y = 2 * plane + way.
__global__ void __launch_bounds__(kBlock) lbm64_push_ghost_cols_kernel(const ColsPushGhost64Args a)
{
  const uint32_t per_row = a.ghost / kPairCells;                       // accesses per row of a plane and way: 1 or 2
  const uint32_t m = blockIdx.x * kBlock + threadIdx.x;
  if (m >= a.ny * per_row) return;
  const uint32_t k = blockIdx.y >> 1;                                  // plane 0..8
  const bool to_east = (blockIdx.y & 1u) != 0u;
  const uint32_t row = m / per_row;                                    // 0 .. ny - 1
  const size_t x = static_cast<size_t>(m - row * per_row) * kPairCells; // 0 .. ghost - 2
  const double* from = a.grid + k * a.ps + static_cast<size_t>(row) * a.pitch + (to_east ? a.nxl : a.ghost) + x;
  double* to = to_east ? a.east + k * a.east_ps + static_cast<size_t>(row) * a.east_pitch + x
                       : a.west + k * a.west_ps + static_cast<size_t>(row) * a.west_pitch + (static_cast<size_t>(a.ghost) + a.west_nxl) + x;
  *reinterpret_cast<d2*>(to) = load2(from);
}

// ---- a block whose pitch is not its width: the counterparts of step64.h's small kernels ---------------------------------------------
// In the copies, the observables and the digest `grid` points at the first OWNED cell of the first row wanted (the caller adds the ghost
// columns): cell (row, x), 0 <= x < nxl, lies at grid[row * pitch + x], and a contiguous index c over the nxl * rows cells wanted is
// row = c / nxl, x = c - row * nxl.  The two kernels that read the window bitfield take plane 0's storage cell 0 and index both by the
// storage cell.

// accelerate_flow (d2q9-bgk.c:442-478) in place on the owned cells of one row: before the first step of a run.  `grid` is plane 0's
// storage cell 0, `mask` the window bitfield and `first` the storage cell of the row's first owned column.
__global__ void lbm64_cols_accelerate_kernel(double* grid, size_t ps, const uint32_t* mask, uint32_t first, uint32_t nxl, double w1, double w2)
{
  const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= nxl) return;
  const uint32_t c = first + x;
  if ((mask[c >> 5] >> (c & 31u)) & 1u) return;
  double* f = grid + c;
  const double f3 = f[3 * ps], f6 = f[6 * ps], f7 = f[7 * ps];
  if (f3 - w1 > 0.0 && f6 - w2 > 0.0 && f7 - w2 > 0.0) {
    f[1 * ps] += w1; f[5 * ps] += w2; f[8 * ps] += w2;
    f[3 * ps] = f3 - w1; f[6 * ps] = f6 - w2; f[7 * ps] = f7 - w2;
  }
}

// AoS <-> SoA of `n` cells (whole rows of the block): aos holds them contiguously, 9 words a cell.  Bits move as 64-bit integers.
__global__ void lbm64_cols_aos_to_soa_kernel(const unsigned long long* aos, unsigned long long* grid, size_t ps, size_t pitch, size_t nxl, size_t n)
{
  const size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n * 9) return;
  const size_t c = i / 9, row = c / nxl;
  grid[(i - c * 9) * ps + row * pitch + (c - row * nxl)] = aos[i];
}

__global__ void lbm64_cols_soa_to_aos_kernel(const unsigned long long* grid, unsigned long long* aos, size_t ps, size_t pitch, size_t nxl, size_t n)
{
  const size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n * 9) return;
  const size_t c = i / 9, row = c / nxl;
  aos[i] = grid[(i - c * 9) * ps + row * pitch + (c - row * nxl)];
}

// lbm64_observables_kernel's arithmetic (d2q9-bgk.c:1084-1111) on `n` cells of the block: obs[4c..4c+3] = {u_x, u_y, u, pressure}.
__global__ void __launch_bounds__(kBlock) lbm64_cols_observables_kernel(const double* grid, size_t ps, size_t pitch, size_t nxl, size_t n, double* obs)
{
  const size_t c = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (c >= n) return;
  const size_t row = c / nxl, at = row * pitch + (c - row * nxl);
  double f[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) f[k] = grid[k * ps + at];
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

// lbm64_av_velocity_kernel's sum (d2q9-bgk.c:716-751) over the nxl * ny owned cells: `grid` and the window bitfield are indexed by the
// STORAGE cell row * pitch + ghost + x.
__global__ void __launch_bounds__(kBlock) lbm64_cols_av_velocity_kernel(const double* grid, size_t ps, const uint32_t* mask, size_t pitch, size_t ghost, size_t nxl,
                                                                        size_t ncells, double* partials)
{
  __shared__ double red[kBlock / 64];
  double acc = 0.0;
  for (size_t c = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x; c < ncells; c += static_cast<size_t>(gridDim.x) * kBlock) {
    const size_t row = c / nxl, at = row * pitch + ghost + (c - row * nxl);
    if ((mask[at >> 5] >> (at & 31)) & 1u) continue;
    double f[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) f[k] = grid[k * ps + at];
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

// The block's PART of the row digests of include/lbm_d2q9_f64_digest.h: block b sums the digest terms of the nxl owned cells of row
// row0 + b, which are the whole grid's cells (row0 + b) * nx + x0 + x, into row_parts[b].  The terms are lbm64_row_digest_kernel's; the
// sum is wrap-around, so the parts of the ranks add up, in any order, to the row's digest.  `grid` points at row row0's first owned cell.
__global__ void __launch_bounds__(kBlock) lbm64_cols_row_digest_kernel(const unsigned long long* grid, size_t ps, size_t pitch, uint32_t nxl, uint32_t nx, uint32_t x0,
                                                                       unsigned long long row0, unsigned long long* row_parts)
{
  __shared__ unsigned long long red[kBlock / 64];
  const unsigned long long* row = grid + static_cast<size_t>(blockIdx.x) * pitch;
  const unsigned long long cell0 = (row0 + blockIdx.x) * static_cast<unsigned long long>(nx) + x0;   // the block's first cell of the row in the whole grid
  unsigned long long h = 0;
  for (uint32_t x = threadIdx.x; x < nxl; x += kBlock) {
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
    row_parts[blockIdx.x] = t;
  }
}

}  // namespace
