// rows_multi64.h — row-partitioned runs of the double-precision mode, several steps per exchange (LBM_ROWS64_FLAG_MULTI_STEPS,
// LBM_ROWS64_FLAG_MULTI_ANY_SIZE): lbm_rows_multi_kernel_f64<K, NT, FULL, EDGE>, the partition form of lbm_multi_kernel_f64 (kernels/multi64.h: up to K steps of one rank per
// launch), and lbm64_push_ghost_rows_kernel, which stores a rank's K first and K last owned rows into its neighbours' ghost rows.
// Part of the translation unit lbm_rows64.hip (gfx950 only, -ffp-contract=off); include/lbm_d2q9_f64_rows.h states the contract.
//
// A FULL DEFINITION, not a shared body.  Moving lbm_multi_kernel_f64's body into a function that both kernels call — with no other
// change — gives lbm_f64.hip other device assembly than the parent's (other register numbering and schedule in every instantiation:
// the callee is optimised before it is inlined, without the kernel's launch bounds, which clang accepts on kernels only), and
// profiles/r18/device_asm_identical.txt holds the existing units to the parent's assembly.  So multi64.h stays as it is and this file
// restates it.  Whoever changes one of the two changes the other: tests/test_f64_rows_multi.py holds both to the same bits.
//
// What is lbm_multi_kernel_f64's, unchanged: the 32 x 16 tile per block of kMulti64Lanes lanes, the in-place LDS frame with its
// reduction scratch and flag bytes (bit 0 obstacle, 1 owned, 2 on row ny-2), the sub-steps and their barriers, finish_cell_f64, one
// accumulator per sub-step, wave_sum_vec4, the fold block (block 0) and the layout of partials_out.
//
// What differs, in sub-step 1 and in the final store only:
//   rows do not wrap.  A rank's grids are nyl + 2 * ghost STORAGE rows (ghost = the K of a full launch); owned row y is storage row
//                   y + ghost.  Tile row ty's region grown by e starts at storage row ghost + ty * TY - e >= 1 (e <= K - 1 < ghost) and
//                   ends at ghost + nyl + e - 1 <= nyl + 2 ghost - 2: the pull reads one row further, storage rows 0 and
//                   nyl + 2 ghost - 1 at the most.  x wraps on nx as before.
//   row ny-2        is told by the WHOLE grid's row (row0 + storage row) mod ny, so the copies of it among a rank's ghost rows (rank 0's
//                   lower ones: the ring is periodic) and in the frames' rings are accelerated between sub-steps as the owned copy is.
//   obstacle bits   come from the rank's WINDOW bitfield over its storage rows (the whole grid's rows row0 .. row0 + nyl + 2 ghost - 1,
//                   periodic): bit c of the storage cell c.  nx is even, so a pair's two bits sit in one word.
//   sum|u| terms    count for owned cells, as before: ghost rows are ring cells of the edge tiles.
// Bounds: a pull reads storage cells only, shifted by one double into the planes' guards at most; stores go to owned cells.
//
// EDGE (LBM_ROWS64_FLAG_MULTI_ANY_SIZE): multi64.h's edge-tile form on a rank's rows.  ceil(nx / TX) x ceil(nyl / TY) tiles on a rank
// they do not cover exactly (nx even and >= TX, nyl >= TY; ranks of one run may differ in nyl).  Tile (tx, ty) starts at column
// x0 = min(TX tx, nx - TX) and OWNED row y0 = min(TY ty, nyl - TY): a tile of the last column or row is shifted back inside the rank's
// owned rows, over its neighbour, and owns only its cells at tile-local x >= TX tx - x0, y >= TY ty - y0, so every owned cell of the
// rank has exactly one owner.  Only owned cells are stored and counted; the others are computed like ring cells.  What the bounds
// above become:
//   rows            y0 <= nyl - TY, so the region grown by e spans storage rows ghost + y0 - e >= 1 to ghost + y0 + TY + e - 1 <=
//                   ghost + nyl + e - 1, as before; the pull reads one row further, inside the storage.
//   obstacle bits   x0 and gx are even (nx and TX are), so a pair's first cell is even and its two bits still sit in one word.
//   x wrap          nx >= TX = 32 > gx, and x0 - gx + rx lies in -gx .. nx + gx - 2: one correction suffices, as before.
//   row ny-2        by the whole grid's row of the storage row, which does not depend on the tile: unchanged.
#pragma once
#include <type_traits>

#include "multi64.h"

namespace {

struct RowsMulti64Args {
  const double* src;           // source grid, plane 0 STORAGE row 0
  double* dst;                 // destination grid
  const uint32_t* mask;        // the rank's window bitfield: bit c of the storage cell c
  size_t ps;
  int nx, ny;                  // of the WHOLE grid (ny: for the row-ny-2 flag alone)
  int ghost;                   // ghost rows on each side of the owned rows: the K of a full launch
  int row0;                    // the whole grid's row of storage row 0, y0 - ghost: -ghost .. ny - 1 - ghost
  int tiles_x;                 // nx / TX (EDGE: rounded up)
  int ksteps;                  // 1..K steps in this launch (FULL: K)
  double omega, accel_w1, accel_w2;
  int accel_row;               // ny-2, a row of the WHOLE grid
  int accel_last;              // apply accelerate_flow after the LAST sub-step too (another step follows)
  double* partials_out;        // [ksteps][tiles of this rank]
  const double* prev_partials; // previous launch: [n_prev_vecs][n_prev]
  int n_prev, n_prev_vecs;
  double* sums;                // this rank's per-step totals of this run
  int* counter;
};
// What the EDGE form takes: a type of its own, so that the kernel arguments of the other form (and with them the offsets of the
// hidden ones behind them) stay what they were.
struct RowsMulti64EdgeArgs : RowsMulti64Args {
  int last_y0;                 // the owned row at which the rank's last tile row starts: nyl - TY
};
template <bool EDGE> using RowsMulti64ArgsOf = std::conditional_t<EDGE, RowsMulti64EdgeArgs, RowsMulti64Args>;

// Rows that storage row sy pulls from: no wrap, its neighbours are rows of the storage (1 <= sy <= rows - 2).
__device__ __forceinline__ Rows64 rows_of_storage(uint32_t nx, uint32_t sy)
{
  Rows64 r;
  r.here = static_cast<size_t>(sy) * nx;
  r.south = r.here - nx;
  r.north = r.here + nx;
  return r;
}

// FULL: the launch makes exactly K steps, so every region size is a compile-time constant.
// EDGE: the edge-tile form described above.
template <int K, bool NT, bool FULL, bool EDGE = false>
__global__ void __launch_bounds__(kMulti64Lanes, kMulti64WavesPerSimd) lbm_rows_multi_kernel_f64(const RowsMulti64ArgsOf<EDGE> a)
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
  // the tile's first column and owned row (EDGE: shifted back inside the rank).  Formed where they are used, x before y, not here, as in
  // multi64.h: the existing instantiations then compile to the instructions they had before EDGE was a parameter
  // (profiles/r22/device_asm_identical.txt).
  auto tile_x0 = [&]() __attribute__((always_inline)) { return EDGE ? min(tx * TX, a.nx - TX) : tx * TX; };
  auto tile_y0 = [&]() __attribute__((always_inline)) { if constexpr (EDGE) return min(ty * TY, a.last_y0); else return ty * TY; };

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
      int x = x0 - gx + rx; if (x < 0) x += a.nx; else if (x >= a.nx) x -= a.nx;      // -gx .. nx + gx - 2, and nx >= TX > gx
      const int y0 = tile_y0(), own_y = EDGE ? ty * TY - y0 : 0;
      const int sy = a.ghost + y0 - e + ry;                                            // storage row: ghost - e .. ghost + nyl + e - 1, and ghost > e
      int gy = a.row0 + sy; if (gy < 0) gy += a.ny; else if (gy >= a.ny) gy -= a.ny;       // the whole grid's row: -e .. ny + e - 1 before, and ny >= TY > e
      const uint32_t cell = static_cast<uint32_t>(sy) * static_cast<uint32_t>(a.nx) + static_cast<uint32_t>(x);
      const uint32_t mbits = (a.mask[cell >> 5] >> (cell & 31u)) & 3u;                       // cell is even: both bits in one word
      const bool on_row = gy == a.accel_row;                                                 // the owned row ny-2 and every ghost or ring copy of it
      const bool accel = on_row && (!last || a.accel_last);
      const bool owned = rx >= gx + own_x && rx < gx + TX && ry >= e + own_y && ry < e + TY;   // both cells of a pair, or neither
      d2 p[9];
      pull_pair_f64(a.src, ps, static_cast<uint32_t>(a.nx), rows_of_storage(static_cast<uint32_t>(a.nx), static_cast<uint32_t>(sy)), static_cast<uint32_t>(x), p);
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
      double* d = a.dst + (static_cast<size_t>(a.ghost + y0 + ry) * a.nx + static_cast<size_t>(x0 + (rx & ~1)));   // owned row y0 + ry
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

// The exchange of one rank after a launch: all nine planes of its first `ghost` owned rows (storage rows ghost .. 2 ghost - 1) into the
// upper ghost rows of the rank below (its storage rows ghost + down_nyl ..), and of its last `ghost` owned rows (storage rows nyl ..
// nyl + ghost - 1) into the lower ghost rows of the rank above (its storage rows 0 .. ghost - 1), in the neighbour's grid of the same
// parity.  Sources are owned rows, targets ghost rows: disjoint even where the rank is its own neighbour (nyl >= 16 > 2 ghost).  Ranks of
// an uneven run (EDGE) differ in nyl and plane stride: the targets are formed from the NEIGHBOUR's down_nyl, down_ps and up_ps, and
// every rank owns >= 16 rows, so the same holds.
// A neighbour's grid may be another device's memory (peer access): plain 16-byte vector stores (nx is even, every row starts at an even
// double).  Nothing waits on the device.
struct RowsPushGhost64Args {
  const double* grid;          // this rank's grid just written, plane 0 storage row 0
  size_t ps;
  uint32_t nx, nyl, ghost;
  double* down;                // the rank below: the same grid of it, its plane stride and owned rows
  size_t down_ps;
  uint32_t down_nyl;
  double* up;                  // the rank above
  size_t up_ps;
};

// Grid: x over the ghost * nx / 2 accesses of one plane and way (< 2^28: nx * 16 <= 2^31), y = 2 * plane + way.
__global__ void __launch_bounds__(kBlock) lbm64_push_ghost_rows_kernel(const RowsPushGhost64Args a)
{
  const uint32_t per_row = a.nx / kPairCells;                          // accesses per row of a plane
  const uint32_t m = blockIdx.x * kBlock + threadIdx.x;                // < ghost * per_row + 256
  if (m >= a.ghost * per_row) return;
  const uint32_t k = blockIdx.y >> 1;                                  // plane 0..8
  const bool north = (blockIdx.y & 1u) != 0u;
  const uint32_t row = m / per_row;                                    // 0 .. ghost - 1
  const size_t x = static_cast<size_t>(m - row * per_row) * kPairCells;
  const size_t nx = a.nx;
  const double* from = a.grid + k * a.ps + (static_cast<size_t>(north ? a.nyl : a.ghost) + row) * nx + x;
  double* to = north ? a.up + k * a.up_ps + static_cast<size_t>(row) * nx + x
                     : a.down + k * a.down_ps + (static_cast<size_t>(a.ghost) + a.down_nyl + row) * nx + x;
  *reinterpret_cast<d2*>(to) = load2(from);
}

}  // namespace
