// multi64.h — lbm_multi_kernel_f64<K, NT, FULL, EDGE>: up to K steps per launch of the double-precision mode, for the large whole grids whose
// one-step launches are bound by HBM (144 B per cell-step).  Part of the translation unit lbm_f64.hip (gfx950 only, -ffp-contract=off).
//
// lbm_multi_kernel's scheme (kernels/multi.h) with every object a double.  A block of kMulti64Lanes lanes owns a TX x TY tile
// (lbm_geometry.h: 32 x 16).  Its LDS frame is ONE buffer of FX x FY cells of nine doubles, FX = TX + 2 multi_ex(K-1), FY = TY + 2 (K-1),
// updated in place; the owned tile sits at (multi_ex(K-1), K-1) in it.  A launch of k <= K steps:
//   sub-step 1      pulls the tile grown by e = k-1 rows and multi_ex(e) columns straight from the source grid, periodic in x and y on
//                   GLOBAL coordinates (a grid of one tile simply meets itself), an aligned x-pair per lane (pull_pair_f64 of step64.h:
//                   16-byte loads, both obstacle bits from one mask word), and writes the results and a flag byte per cell into the frame;
//   sub-step s > 1  works on the tile grown by e = k-s cells each way, one cell per lane and item: a lane reads the nine neighbours of ALL
//                   its items (at most two: a region has up to 2 x lanes cells) from the frame into registers and computes; then a
//                   barrier, the write-back, a barrier — otherwise one pass's results would feed another's neighbours;
//   the last one    covers the tile, one cell per lane, and stores to the destination grid: x-neighbouring lanes exchange halves
//                   (one DPP move per population pair) so that every store is 16 bytes, non-temporal where NT.
// k = 1 (a tail): sub-step 1 is the last and stores its pairs directly.
// Ring cells are recomputed by the neighbouring blocks with the same arithmetic, so no block waits for another.  The cell update is
// finish_cell_f64 of step64.h, called as it is: no bit depends on the kernel, K, the cut of a run into launches or the lane.
//
// accelerate_flow between sub-steps is finish_cell_f64's `accel` on every frame copy of global row ny-2 (flag bit 2), ring copies
// included, and after the last sub-step exactly when another step of the run follows (accel_last), as in tile64.h.
//
// sum|u|: a term counts for owned, unblocked cells only (ring items never read their term: its sqrt is dead there).  A lane keeps one
// accumulator per sub-step — it meets at most two owned cells in one: the pair of sub-step 1, the two items of a frame sub-step — the
// wave's halving butterflies (common.h wave_sum_vec4) join the lanes, one lane per step adds the waves' sums serially and writes
// partials_out[step][tile].  Block 0 does no lattice work: it folds the PREVIOUS launch's vectors into sums[counter ...].  No atomics
// anywhere: the order of additions is fixed (include/lbm_d2q9_f64.h states the tree).
//
// Addresses: cell indices are 32-bit (lbm64_create refuses grids of 2^31 cells), every address is formed in 64 bits with size_t plane
// offsets.  Bounds: a pull reads cells of the grid only, shifted by one double into the planes' guards at most, exactly as the one-step
// kernel; a frame sub-step reads one cell around a region grown by at most K-2, inside the frame; stores go to owned cells.
#pragma once
#include "step64.h"

namespace {

struct Multi64Args {
  const double* src;
  double* dst;
  const uint32_t* mask;
  size_t ps;
  int nx, ny;
  int tiles_x;                 // nx / TX (EDGE: rounded up)
  int ksteps;                  // 1..K steps in this launch (FULL: K)
  double omega, accel_w1, accel_w2;
  int accel_row;               // ny-2
  int accel_last;              // apply accelerate_flow after the LAST sub-step too (another step follows)
  double* partials_out;        // [ksteps][tiles]
  const double* prev_partials; // previous launch: [n_prev_vecs][n_prev]
  int n_prev, n_prev_vecs;
  double* sums;
  int* counter;
};

// Waves per SIMD the kernel is compiled for: two blocks of eight waves per CU, i.e. 128 registers a lane.  (The frames of K <= 3 leave
// LDS for a third block, which a kernel of 80 registers or fewer gets.)
constexpr int kMulti64WavesPerSimd = 2 * (kMulti64Lanes / 64) / 4;

// FULL: the launch makes exactly K steps, so every region size is a compile-time constant.
// EDGE (LBM64_FLAG_MULTI_ANY_SIZE): ceil(nx / TX) x ceil(ny / TY) tiles on a grid they do not cover exactly (nx even and >= TX, ny >= TY).
// Tile (tx, ty) starts at x0 = min(TX tx, nx - TX), y0 = min(TY ty, ny - TY): a tile of the last column or row is shifted back inside
// the grid, over its neighbour, and owns only its cells at tile-local x >= TX tx - x0, y >= TY ty - y0, so every cell of the grid has
// exactly one owner.  x0 and the x bound are even (nx is): pairs stay aligned and are owned whole.  A tile's cells it does not own
// are computed like ring cells, for their neighbours; only owned cells are stored and counted.  All else is the kernel as it is.
template <int K, bool NT, bool FULL, bool EDGE = false>
__global__ void __launch_bounds__(kMulti64Lanes, kMulti64WavesPerSimd) lbm_multi_kernel_f64(const Multi64Args a)
{
  static_assert(multi64_k_ok(K), "unsupported steps per launch");
  constexpr int TX = kMulti64TX, TY = kMulti64TY, FX = multi64_frame_x(K), FY = multi64_frame_y(K), FC = FX * FY;
  constexpr int EX = multi_ex(K - 1), EY = K - 1, kLanes = kMulti64Lanes, kWaves = kLanes / 64;
  static_assert((TX / 2 + multi_ex(K - 1)) * FY <= kLanes, "sub-step 1 deals a lane at most one x-pair");
  extern __shared__ __attribute__((aligned(16))) double frame64[];     // [9][FC] doubles, reduction scratch, flag bytes
  double* red = frame64 + 9 * FC;                                       // [kMulti64Accs][kWaves]
  uint8_t* cell_flags = reinterpret_cast<uint8_t*>(red + kMulti64Accs * kWaves);   // per frame cell: bit 0 obstacle, 1 owned, 2 on row ny-2
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
  const int k_total = FULL ? K : a.ksteps;
  const size_t ps = a.ps;
  // the tile's first cell (EDGE: shifted back inside the grid).  Formed where it is used, x before y, not here: the existing instantiations
  // then compile to the instructions they had before EDGE was a parameter (profiles/r20/device_asm_identical.txt).
  auto tile_x0 = [&]() __attribute__((always_inline)) { return EDGE ? min(tx * TX, a.nx - TX) : tx * TX; };
  auto tile_y0 = [&]() __attribute__((always_inline)) { return EDGE ? min(ty * TY, a.ny - TY) : ty * TY; };

  double acc[kMulti64Accs];
#pragma unroll
  for (int i = 0; i < kMulti64Accs; ++i) acc[i] = 0.0;

  // ---- sub-step 1: an aligned x-pair of the grown tile per lane, pulled from the source grid.  nx, TX and multi_ex are even, so a pair
  // never straddles the wrap and its first cell has an even index.
  {
    const int e = k_total - 1, gx = multi_ex(e);
    const int wp = TX / 2 + gx, hy = TY + 2 * e;               // pairs per row, rows
    const bool last = !FULL && e == 0;
    if (tid < wp * hy) {
      const int ry = FULL ? tid / wp : small_div(tid, wp), rx = 2 * (tid - ry * wp);
      const int x0 = tile_x0(), own_x = EDGE ? tx * TX - x0 : 0;
      int x = x0 - gx + rx; if (x < 0) x += a.nx; else if (x >= a.nx) x -= a.nx;           // -gx .. nx + gx - 2, and nx >= TX > gx
      const int y0 = tile_y0(), own_y = EDGE ? ty * TY - y0 : 0;
      int y = y0 - e + ry;  if (y < 0) y += a.ny; else if (y >= a.ny) y -= a.ny;           // -e .. ny + e - 1, and ny >= TY > e
      const uint32_t cell = static_cast<uint32_t>(y) * static_cast<uint32_t>(a.nx) + static_cast<uint32_t>(x);
      const uint32_t mbits = (a.mask[cell >> 5] >> (cell & 31u)) & 3u;                       // cell is even: both bits in one word
      const bool on_row = y == a.accel_row;
      const bool accel = on_row && (!last || a.accel_last);
      const bool owned = rx >= gx + own_x && rx < gx + TX && ry >= e + own_y && ry < e + TY;   // both cells of a pair, or neither
      d2 p[9];
      pull_pair_f64(a.src, ps, static_cast<uint32_t>(a.nx), rows_of(static_cast<uint32_t>(a.nx), static_cast<uint32_t>(a.ny), static_cast<uint32_t>(y)), static_cast<uint32_t>(x), p);
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
        double* d = a.dst + cell;
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
      const int x0 = tile_x0(), y0 = tile_y0(), own_x = EDGE ? tx * TX - x0 : 0, own_y = EDGE ? ty * TY - y0 : 0;
      const bool stores = !EDGE || (rx >= own_x && ry >= own_y);      // owned (own_x is even: both lanes of a pair, or neither); every lane makes the exchange
      double* d = a.dst + (static_cast<size_t>(y0 + ry) * a.nx + static_cast<size_t>(x0 + (rx & ~1)));
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

}  // namespace
