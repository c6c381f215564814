// multi.h — lbm_multi_kernel<K>: K steps per pass over HBM for the bandwidth-bound grids and for K-step row partitions
// Part of the single translation unit lbm_kernels.hip (device code of liblbm_d2q9.so, gfx950 only).
#pragma once
#include "common.h"

namespace {

// ------------------------------------------------------------------------------------------------
// K steps per pass over HBM for bandwidth-bound grids: lbm_multi_kernel<K>.
//
// The one-step kernel moves 72 B per cell-step and sits at ~90 % of what HBM delivers; the only way
// further up is to touch memory less often.  Here a block owns a TX x TY tile (MultiGeom below: 64 x 16 on
// 512 lanes for K <= 3; 64 x 13, 32 x 13 or, on 768 lanes, 64 x 24 for K = 4) and advances it
// by K steps per launch: sub-step 1 pulls straight from the source grid (as the one-step kernel
// does) for the tile plus a (K-1)-cell ring and keeps the result in LDS; sub-steps 2..K update that
// LDS frame in place (neighbours read into registers, barrier, results written back), each on a
// region one cell smaller; the last sub-step covers exactly the owned tile and writes the
// destination grid.  The ring is recomputed redundantly by the neighbouring blocks with the same
// arithmetic, so no block ever waits for another, and the results are bit-identical to K launches of
// the one-step kernel.  HBM traffic per K steps, on 64 x 16 tiles: (64+2K)(16+2K)/1024 x 36 B read + 36 B
// written (K = 2: 84 B instead of 144 B; K = 4: 97 B instead of 288 B).
//
// Dealing of lanes.  k_substeps deals each region's pairs row after row over the block, in passes of
// whole rows (sub-steps 1 - 3 of the tall K = 4 launch take two passes each), every pair with the
// sum|u| term code and a flag byte in LDS.  The tall K = 4 instantiation, whose 64 x 24 tile has one
// x-pair per lane, runs owned_substeps instead: each lane keeps its owned pair for the whole launch
// (flags and population 0 in registers), and the ring pairs are extra, term-free items on the first
// lanes, one per lane and sub-step, so that each in-LDS sub-step is a single read / barrier / write.
// What is not the dealing itself — the source pull, the kept / counted tests, the flag byte, the frame read,
// the destination index — is written once at kernel scope (pull, classify, pair_flag_bits, read_pair, kept_cell).
// K = 5 (whole periodic grids, tall geometry, plain form only) runs owned_substeps on the same tile with a 72 x 32 frame that
// holds populations 1 - 8: population 0 of a ring pair lives in a compact array by the pair's index in sub-step 1's ring
// (MultiGeom::compact0, ring0_at), which keeps the block at two per CU.
//
// Rows outside the partition: `y_periodic` wraps (self-contained domain); otherwise the storage has
// `ghost` extra rows below and above the owned rows, filled by the neighbours before the launch.
// ------------------------------------------------------------------------------------------------
// Tile shapes, block sizes and the steps a launch can make (kMTX ... kMaxGroup, kGeom*, geom_tx, multi_ty, multi_lanes, geom_for, multi_ex): lbm_geometry.h.
#if LBM_TILE_STAMPS      // diagnostic builds (tile.h, scripts/tile_stamps.py): stamps of one block in the middle of the launch, lane 0
#define LBM_MSTAMP(i) do { if (blockIdx.x == (gridDim.x >> 1) && threadIdx.x == 0) g_tile_stamps[i] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define LBM_MSTAMP(i) do { } while (0)
#endif

template <int K, int GEOM = kGeomStd>
struct MultiGeom {
  static constexpr int TX = geom_tx(GEOM);                          // owned columns of a tile
  static constexpr int TY = multi_ty(K, GEOM);                      // owned rows of a tile
  static constexpr int LANES = multi_lanes(K, GEOM);                // block size
  static constexpr int EY = K - 1, EX = multi_ex(K - 1);            // growth of the first sub-step
  static constexpr int W = TX + 2 * EX, H = TY + 2 * EY;            // LDS frame
  static constexpr int cells = W * H;
  // population 0 out of the frame (the five-step launch of whole grids, lbm_geometry.h multi_compact0): planes 1 - 8, then a float pair per ring pair of sub-step 1
  static constexpr bool compact0 = multi_compact0(K, GEOM);
  static constexpr int planes = compact0 ? 8 : 9, first_plane = compact0 ? 1 : 0;
  static constexpr int ring0_floats = compact0 ? 2 * multi_ring_pairs(K, GEOM, 1) : 0;
  static constexpr size_t lds_bytes = multi_lds_bytes(K, GEOM);     // planes (+ ring pairs' population 0) + reduction scratch + a flag byte per x-pair
  static_assert(lds_bytes == sizeof(float) * (planes * cells + ring0_floats) + sizeof(double) * K * (LANES / 64) + (K >= 2 ? cells / 2 : 0), "the kernel's layout and lbm_geometry.h agree");
  static_assert(W == multi_frame_w(K, GEOM) && H == multi_frame_h(K, GEOM), "the frame of lbm_geometry.h");
  // waves per SIMD the kernel is compiled for: what its LDS frame lets a CU hold, LBM_MWAVES at most
  static constexpr int blocks_per_cu = lds_bytes * 8 <= 160 * 1024 ? 8 : static_cast<int>(160 * 1024 / lds_bytes);
  static constexpr int waves_per_simd = blocks_per_cu * (LANES / 64) / 4 < LBM_MWAVES ? (blocks_per_cu * (LANES / 64) / 4 < 1 ? 1 : blocks_per_cu * (LANES / 64) / 4) : LBM_MWAVES;
  // lanes dealt one owned x-pair each for the whole launch (the tall geometry at K = 4 and K = 5: 32 x 24 pairs on 768 lanes; see owned_substeps)
  static constexpr bool owned_lanes = K >= 4 && GEOM == kGeomTall;
  // x-pairs of sub-step j's region outside the owned tile: ey rows below and above it, multi_ex(ey) / 2 pairs on each side of its rows
  static constexpr int ring_pairs(int j) { return multi_ring_pairs(K, GEOM, j); }
};

struct MultiArgs {
  const float* src;
  float* dst;
  const float* srck[9];        // src + k*ps, dst + k*ps: plane bases as kernel arguments, so that they are scalar
  float* dstk[9];              // loads at the point of use and never 64-bit vector arithmetic
  const uint32_t* mask;        // bit per STORAGE cell (ghost rows included)
  size_t ps;
  int nx;
  // Rows, all in STORAGE coordinates (row 0 = the first ghost row, or the first grid row of a whole periodic grid).  A launch
  // computes the rows [row_first, row_first + rows_compute): the owned rows, or — the first launches of a group that makes several
  // launches per halo exchange (lbm_p2p_impl.h) — the owned rows and `ext` ghost rows on each side, which the later launches of the
  // group then read instead of exchanged rows.  Only cells of the rows [count_first, count_end) — the rows the partition OWNS — enter the
  // per-step sums (the neighbours count theirs).
  int row_first, rows_compute;
  int rows_storage;            // owned rows + 2 x ghost rows
  int count_first, count_end;
  int y_periodic;
  int y0_global, ny_global;    // global row of storage row `row_first` (may be negative: a rank's bottom ghost rows wrap); global grid height
  int tiles_x;
  int tile_begin, tile_count, tile_begin2, tile_count2;   // tile ranges of this launch (second may be empty)
  int ntiles_total;            // stride of partials_out
  int xcd_remap;               // tile order: contiguous eighth per XCD (needs (tile_count+tile_count2) % 8 == 0)
  float omega, accel_w1, accel_w2;
  int accel_row;               // GLOBAL row ny-2
  int accel_last;
  double* partials_out;        // [ksteps][ntiles_total]
  const double* prev_partials; // previous launch: [n_prev_vecs][n_prev]
  int n_prev, n_prev_vecs;
  double* sums;
  int* counter;
  // peer-to-peer loop, the LAST launch of a group of several: "ready for epoch `ready_epoch`" to both neighbours (kernels/p2p.h
  // P2PWindowHeader::halo_ack), said by the fold block as the launch starts — this launch reads ghost rows of its source grid only and
  // writes owned rows, so the ghost rows of its destination grid, the next push's target, are free from here on.  0: nothing to say.
  unsigned long long* ready[2];  // [0] south, [1] north
  unsigned long long ready_epoch;
  // ... and, once the fold is done, waits until both neighbours have said the same to this rank (bounded; err is the transport's
  // host-mapped error word): the push kernel that follows this launch in the stream then stores without asking.  Every rank speaks
  // before it waits, so a ring of ranks cannot dead-lock here; the wait overlaps the launch's own tiles.
  const unsigned long long* wait_ready;  // this rank's halo_ack[2] (kPartTile: [4]), or null
  long long timeout_ticks;
  int* err;
  // Tile decomposition (kPartTile): the storage also has ghost COLUMNS on each side of the owned ones.  The launch computes every
  // column of its rows (the row wraps at the storage width: what the wrap feeds in is wrong by one more column per step and never
  // reaches a kept one before the next exchange), KEEPS — writes to the destination grid — the columns [keep_x0, keep_x1) only (owned +
  // the ghost columns the later launches of the group read; both even), and counts the owned columns [cx0, cx1).
  int keep_x0, keep_x1, cx0, cx1;
  unsigned long long* ready_x[2]; // ... and its ready words for the west and the east neighbour (this rank's: wait_ready[2], [3])
  // ... and the tiles of a launch as up to four RECTANGLES of the tile grid instead of two tile ranges (nrect > 0): the part of a group's first
  // launch that reads no exchanged row or column is one rectangle (tile rows x tile columns inside the rim), the rim the four around it.
  int nrect;
  struct Rect { int ty0, tx0, ntx, count; } rect[4];       // tile rows from ty0, tile columns [tx0, tx0 + ntx); count = rows x ntx blocks
  int nblocks;                     // kPartTile: tiles of this launch; the grid is padded to a multiple of 8 blocks so that the XCD-contiguous order
                                   // (xcd_remap) applies to any tile count — a tile rank's storage rows are never a multiple of 8 tiles wide
};

// A pair (x, x+1), x even, of population k into row `row` (a dword index) of an LDS frame of row stride W: interleaved
// for the populations pulled without an x shift, odd-x cells first then even-x cells for the others (see the reads).
template <int W>
__device__ __forceinline__ void store_pair(float* plane, int k, int row, int fx, f2 v)
{
  if (k == 0 || k == 2 || k == 4) {
    *reinterpret_cast<f2*>(plane + row + fx) = v;
  } else {
    plane[row + (fx >> 1)] = v.y;
    plane[row + (fx >> 1) + W / 2] = v.x;
  }
}

// finish_pair_lo's accelerate_flow (d2q9-bgk.c:457-469) on the pair's vector elements directly.  owned_substeps relaxes with
// tile_accel = false and applies this after: the same arithmetic, but no float[9] copy of each cell, which hipcc turned into
// strided vector loads of the result array and then kept that array in scratch.
__device__ __forceinline__ void accelerate_pair(f2 (&out)[9], uint32_t mbits, bool accel, float w1, float w2)
{
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const bool go = accel && !((mbits >> j) & 1u) && out[3][j] - w1 > 0.0f && out[6][j] - w2 > 0.0f && out[7][j] - w2 > 0.0f;
    out[1][j] = go ? out[1][j] + w1 : out[1][j]; out[5][j] = go ? out[5][j] + w2 : out[5][j]; out[8][j] = go ? out[8][j] + w2 : out[8][j];
    out[3][j] = go ? out[3][j] - w1 : out[3][j]; out[6][j] = go ? out[6][j] - w2 : out[6][j]; out[7][j] = go ? out[7][j] - w2 : out[7][j];
  }
}

// One launch = exactly K steps (every region size, pass count and accumulator slot is a compile-time
// constant).  A run whose step count K does not divide ends with a launch of the smaller instantiation
// lbm_multi_kernel<k>, k < K: its frame needs k-1 <= ghost rows around the tile, so it runs on the same storage.
// Launch forms (PART).  The first round-4 build had ONE kernel for grids and partitions — row-range arguments, a `counted` bit beside
// `owned` in every pair, the peer-to-peer loop's ready words in the fold block — and ran lbm_multi_kernel<4> on 64 x 23 tiles 3 % slower at
// 8192 x 8192 than round 3's library in the same process (294 against 285.5 us/step); without the counted test and the ready words still
// 1.2 % slower, with an instruction count equal to the old kernel's to five in 1 851: hipcc had scheduled the two bodies differently (110
// differing lines in the opcode sequence), and a launch at the socket power limit notices.  Hence: whole grids, and the launches of a
// partition that compute its owned rows only, compile without either and with their row arithmetic spelled as rounds 1 - 3 spelled it;
// a launch that also computes ghost rows takes the counted form only in the tiles that hold such rows (its first and last tile rows),
// chosen by a block-uniform branch; the ready words live in a third instantiation.  Whole grids: back to round 3's time; the 8192 x 1024-row
// ring 43.4 -> 42.9 us/step beside 40.3 - 41.0 for the same rows as one periodic grid (profiles/r04/ab_part_template.txt).
// PART = kPartPlain, kPartGhost, kPartReady or kPartTile (lbm_geometry.h; the forms above do not change for kPartTile).

// The flag byte of an x-pair of the frame, written by sub-step 1 and read by the in-LDS sub-steps (which then need no grid
// coordinates at all); bits 0-1 are the pair's obstacle bits.  0: the pair was not computed.
constexpr uint32_t kPairObstacles = 3u,
                   kPairKept = 4u,       // inside the owned tile and the grid: the last sub-step writes it to the destination grid
                   kPairAccelRow = 8u,   // on the global accelerate row ny - 2
                   kPairComputed = 16u,
                   kPairCounted = 32u;   // owned by this partition: enters the per-step sums (set in the COUNT form only: elsewhere kept pairs count)
__device__ __forceinline__ uint32_t pair_flag_bits(uint32_t mbits, bool kept, bool accel_row, bool counted)
{
  return mbits | (kept ? kPairKept : 0u) | (accel_row ? kPairAccelRow : 0u) | kPairComputed | (counted ? kPairCounted : 0u);
}

template <int K, int TERMS, int GEOM, int PART>   // TERMS: form of the sum|u| terms (kTermsCompensated by default; + kTermsFused: the fused arithmetic), see finish_pair_lo; GEOM: kGeomStd / Narrow / Tall
__global__ void __launch_bounds__((MultiGeom<K, GEOM>::LANES), (MultiGeom<K, GEOM>::waves_per_simd)) lbm_multi_kernel(const MultiArgs a)
{
  using G = MultiGeom<K, GEOM>;
  constexpr int TX = G::TX, EX = G::EX, EY = G::EY, W = G::W, WH = G::W / 2, kCells = G::cells, kLanes = G::LANES, kWaves = kLanes / 64, TY = G::TY;
  // plane k of the frame is lds + (k - kPl) * kCells: nine planes from population 0, or (G::compact0) eight from population 1 and
  // behind them ring0, population 0 of the ring pairs by their index in sub-step 1's ring
  constexpr int kPlanes = G::planes, kPl = G::first_plane;
  extern __shared__ __attribute__((aligned(16))) float lds[];      // [kPlanes][kCells] (+ ring0), then [K][kWaves] doubles
  double* red = reinterpret_cast<double*>(lds + kPlanes * kCells + G::ring0_floats);
  uint8_t* pair_flags = reinterpret_cast<uint8_t*>(red + K * kWaves);   // a flag byte (kPair*) per x-pair of the frame
  const int tid = threadIdx.x;

  if (blockIdx.x == 0) {
    constexpr int kReadyWords = PART == kPartTile ? 4 : PART == kPartReady ? 2 : 0;   // south, north (a.ready), west, east (a.ready_x)
    if constexpr (kReadyWords > 0) {
      if (a.ready_epoch != 0ull && tid == 0) {
#pragma unroll
        for (int d = 0; d < kReadyWords; ++d) __hip_atomic_store(d < 2 ? a.ready[d] : a.ready_x[d - 2], a.ready_epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      }
    }
    // fold block: the previous launch's per-tile sums, one vector per step, into sums[counter..]
    for (int v = 0; v < a.n_prev_vecs; ++v) {
      double s = 0.0;
      for (int i = tid; i < a.n_prev; i += kLanes) s += a.prev_partials[static_cast<size_t>(v) * a.n_prev + i];
      s = wave_sum(s);
      __syncthreads();
      if ((tid & 63) == 0) red[tid >> 6] = s;
      __syncthreads();
      if (tid == 0) {
        double t = 0.0;
        for (int w = 0; w < kWaves; ++w) t += red[w];
        a.sums[*a.counter + v] = t;
      }
    }
    __syncthreads();
    if (tid == 0 && a.n_prev_vecs > 0) *a.counter += a.n_prev_vecs;
    if constexpr (kReadyWords > 0) {
      if (a.wait_ready && tid == 0) p2p_wait_flags(a.wait_ready, nullptr, kReadyWords, a.ready_epoch, 0ull, a.timeout_ticks, a.err, /*acquire=*/false);
    }
    return;
  }

  LBM_MSTAMP(0);
  int b = blockIdx.x - 1;
  if (a.xcd_remap) {
    // blocks b, b+8, ... share an XCD (round-robin dispatch): give each XCD one contiguous eighth of
    // the launch so that tiles which overlap (x and y neighbours) meet in the same L2
    const int nb = gridDim.x - 1, per = nb >> 3;
    b = (b & 7) * per + (b >> 3);
  }
  if constexpr (PART == kPartTile) {
    if (b >= a.nblocks) return;                      // padding of the grid (block-uniform)
  }
  int tile_of_block = b < a.tile_count ? a.tile_begin + b : a.tile_begin2 + (b - a.tile_count);
  if constexpr (PART == kPartTile) {
    if (a.nrect > 0) {                               // block -> rectangle -> tile (block-uniform scalar work; constant indices: the arguments stay in SGPRs)
      int q = b, ty0 = a.rect[0].ty0, tx0 = a.rect[0].tx0, ntx = a.rect[0].ntx;
      if (a.nrect > 1 && q >= a.rect[0].count) {
        q -= a.rect[0].count; ty0 = a.rect[1].ty0; tx0 = a.rect[1].tx0; ntx = a.rect[1].ntx;
        if (a.nrect > 2 && q >= a.rect[1].count) {
          q -= a.rect[1].count; ty0 = a.rect[2].ty0; tx0 = a.rect[2].tx0; ntx = a.rect[2].ntx;
          if (a.nrect > 3 && q >= a.rect[2].count) { q -= a.rect[2].count; ty0 = a.rect[3].ty0; tx0 = a.rect[3].tx0; ntx = a.rect[3].ntx; }
        }
      }
      const int rr = q / ntx;
      tile_of_block = (ty0 + rr) * a.tiles_x + tx0 + (q - rr * ntx);
    }
  }
  const int tile = tile_of_block;
  const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
  const int x0 = tx * TX;
  const int sy0 = a.row_first + ty * TY;          // storage row of the tile's first row
  const int nx = a.nx;
  constexpr bool XR = PART == kPartTile;            // ghost columns: kept / counted column ranges
  const int rows_storage = (PART == kPartGhost || PART == kPartTile) ? a.rows_storage : a.rows_compute + 2 * a.row_first;   // (owned rows only: row_first ghost rows on each side)
  const int tile_row_base = sy0 * nx;               // block-uniform: a scalar multiply
  const int grid_cells = rows_storage * nx;
  constexpr int ksteps = K;
  double acc[K];
  float acc_lo[K];             // kTermsCompensated: the low parts of a lane's terms, widened once at the end
#pragma unroll
  for (int i = 0; i < K; ++i) { acc[i] = 0.0; acc_lo[i] = 0.0f; }

  // does the LDS frame of this tile meet the global accelerate row ny-2 at all ?  (block-uniform)
  bool tile_accel;
  {
    int d = (a.accel_row - (a.y0_global + ty * TY - EY)) % a.ny_global;     // frame row 0 is storage row row_first + ty*TY - EY
    if (d < 0) d += a.ny_global;
    tile_accel = d < G::H || a.ny_global < G::H;
  }
  // storage row (after any periodic wrap) -> does it hold the global accelerate row ny-2 ?
  auto on_accel_row = [&](int sr) __attribute__((always_inline)) {
    if (!tile_accel) return false;
    int g = a.y0_global + sr - a.row_first;
    if (g < 0) g += a.ny_global; else if (g >= a.ny_global) g -= a.ny_global;
    return g == a.accel_row;
  };

  // tiles whose frame (and its x -+ 1, y -+ 1 reads) lies inside the grid need none of the periodic
  // wraps and none of the partial-tile tests in sub-step 1: block-uniform fast path for all but the edge tiles
  const bool inner = x0 - EX >= 2 && x0 + TX + EX + 2 <= nx && sy0 - EY >= 1 && sy0 + TY + EY + 1 <= rows_storage &&
                     sy0 + TY <= a.row_first + a.rows_compute;

  // ---- what both dealings of the lanes (k_substeps, owned_substeps below) share: the pair at frame position (fx, fy), fx even

  // Sub-step 1's sources of the pair, pulled from the source grid: its nine populations, obstacle bits, storage row `sr` (after
  // any periodic wrap) and byte offset `o_here` within a plane.  false: a row past the storage (a row partition whose rows the
  // tile height does not divide: the last tile row sticks out past the ghost rows), outside every owned cell's dependency cone
  // and not computed.
  auto pull = [&](const int fx, const int fy, f2 (&p)[9], uint32_t& mbits, int& sr, uint32_t& o_here) __attribute__((always_inline)) -> bool {
    int gx = x0 + fx - EX;
    sr = sy0 + fy - EY;
    // One multiply per pair, and a 24-bit one (v_mul_lo_u32 and v_mad_u64_u32 issue at quarter rate: the three
    // products sr * nx, ys * nx, yn * nx were 48 cycles of a pass): the tile's first row is a scalar product, the row
    // inside the frame a small factor (nx < 2^23 is part of the kernel's eligibility), the rows above and below and
    // the periodic wraps are additions.
    int cell = tile_row_base + __mul24(fy - EY, nx) + gx;
    int d_south = -nx, d_north = nx;
    if (!inner) {
      if (gx < 0) { gx += nx; cell += nx; } else if (gx >= nx) { gx -= nx; cell -= nx; }      // periodic (:527-529)
      if (!a.y_periodic && sr + 1 >= rows_storage) return false;
      if (a.y_periodic) {                                                               // periodic (:245-247)
        if (sr < 0) { sr += rows_storage; cell += grid_cells; } else if (sr >= rows_storage) { sr -= rows_storage; cell -= grid_cells; }
        if (sr == 0) d_south = grid_cells - nx;
        if (sr + 1 >= rows_storage) d_north = nx - grid_cells;
      }
    }
    // three 32-bit byte offsets per lane on block-uniform plane bases (scalar base + vector offset
    // addressing: no 64-bit address arithmetic in the vector unit; the x -+ 1 shifts live in the bases)
    o_here = 4u * static_cast<uint32_t>(cell);
    const uint32_t o_south = 4u * static_cast<uint32_t>(cell + d_south);
    const uint32_t o_north = 4u * static_cast<uint32_t>(cell + d_north);
    p[0] = at_byte<f2>(a.srck[0], o_here);                                           // :530-538
    p[2] = at_byte<f2>(a.srck[2], o_south);
    p[4] = at_byte<f2>(a.srck[4], o_north);
    p[1] = at_byte<f2u>(a.srck[1] - 1, o_here);
    p[5] = at_byte<f2u>(a.srck[5] - 1, o_south);
    p[8] = at_byte<f2u>(a.srck[8] - 1, o_north);
    p[3] = at_byte<f2u>(a.srck[3] + 1, o_here);
    p[6] = at_byte<f2u>(a.srck[6] + 1, o_south);
    p[7] = at_byte<f2u>(a.srck[7] + 1, o_north);
    if (!inner) {
      if (gx == 0) {                        // x_w wraps to nx-1 (:529)
        p[1].x = at_byte<float>(a.srck[1] + nx - 1, o_here); p[5].x = at_byte<float>(a.srck[5] + nx - 1, o_south);
        p[8].x = at_byte<float>(a.srck[8] + nx - 1, o_north);
      }
      if (gx == nx - 2) {                   // x_e wraps to 0 (:527-528)
        p[3].y = at_byte<float>(a.srck[3] + 2 - nx, o_here); p[6].y = at_byte<float>(a.srck[6] + 2 - nx, o_south);
        p[7].y = at_byte<float>(a.srck[7] + 2 - nx, o_north);
      }
    }
    mbits = (at_byte<uint32_t>(a.mask, 4u * (static_cast<uint32_t>(cell) >> 5)) >> (cell & 31)) & 3u;
    return true;
  };
  // Is the pair kept (written to the destination grid) and counted (in the per-step sums) ?  kept = inside the owned tile (`own`)
  // AND inside the grid (the last tile column / row may stick out of a grid whose edges are not multiples of the tile: those
  // cells are periodic images, computed but not kept).  COUNT (see the forms below): the tile holds rows or columns that are
  // computed but not counted.  (The grid test behind `if (!inner)`: as one && chain it cost the K = 2 and K = 3 ghost-row
  // instantiations a 63rd VGPR.)
  auto classify = [&](auto count_c, const int fx, const int fy, const bool own, bool& kept, bool& counted) __attribute__((always_inline)) {
    constexpr bool COUNT = decltype(count_c)::value;
    const int srow = sy0 + fy - EY, gxo = x0 + fx - EX;               // the pair's storage row and column before any periodic wrap
    kept = own;
    if (!inner) kept = kept && gxo < nx && srow < a.row_first + a.rows_compute;
    counted = COUNT ? (kept && srow >= a.count_first && srow < a.count_end) : kept;
    if constexpr (XR && COUNT) {                                      // ghost columns: kept and counted column ranges (even bounds: whole pairs)
      kept = kept && gxo >= a.keep_x0 && gxo < a.keep_x1;
      counted = counted && kept && gxo >= a.cx0 && gxo < a.cx1;
    }
  };
  // Populations 1 - 8 of the pair from the frame as the in-LDS sub-step that reads it finds it: stored `rd` dwords lower.
  // Frame layout, per population: the three that are pulled without an x shift (0, 2, 4) keep their rows
  // interleaved — a pair is one aligned ds_read_b64.  The six that are pulled from x -+ 1 have their rows stored
  // DE-INTERLEAVED, odd-x cells first: a row is O[0..WH), E[0..WH) (WH = W/2).  For a pair (x, x+1), x = 2i, the
  // west pulls are O[i-1], E[i] and the east pulls O[i], E[i+1]: one ds_read2_b32 each, ascending addresses in
  // lane order (no register swap), lanes on consecutive dwords (interleaved, they were dword pairs at odd
  // addresses with lane stride 2, two-way bank conflicts in both passes of the instruction).
  auto read_pair = [&](const int rd, const int fx, const int fy, f2 (&p)[9]) __attribute__((always_inline)) {
    const int ci = fy * W + fx - rd;                                   // interleaved planes: cell (fx, fy)
    const int cs = fy * W + (fx >> 1) - rd;                            // split planes: O[i] of row fy; E[i] is WH further
    p[2] = *reinterpret_cast<const f2*>(lds + (2 - kPl) * kCells + ci - W);
    p[4] = *reinterpret_cast<const f2*>(lds + (4 - kPl) * kCells + ci + W);
    p[1] = f2{lds[(1 - kPl) * kCells + cs - 1], lds[(1 - kPl) * kCells + cs + WH]};
    p[5] = f2{lds[(5 - kPl) * kCells + cs - W - 1], lds[(5 - kPl) * kCells + cs - W + WH]};
    p[8] = f2{lds[(8 - kPl) * kCells + cs + W - 1], lds[(8 - kPl) * kCells + cs + W + WH]};
    p[3] = f2{lds[(3 - kPl) * kCells + cs], lds[(3 - kPl) * kCells + cs + WH + 1]};
    p[6] = f2{lds[(6 - kPl) * kCells + cs - W], lds[(6 - kPl) * kCells + cs - W + WH + 1]};
    p[7] = f2{lds[(7 - kPl) * kCells + cs + W], lds[(7 - kPl) * kCells + cs + W + WH + 1]};
  };
  // Cell index of a kept pair in the destination grid: it lies inside the grid, so its index needs no periodic wrap.
  auto kept_cell = [&](const int fx, const int fy) __attribute__((always_inline)) { return tile_row_base + __mul24(fy - EY, nx) + x0 + fx - EX; };

  // The K sub-steps, in two forms: COUNT = the tile holds rows that are computed but not counted (a launch that also advances ghost rows:
  // its first and last tile rows) — every pair then carries a `counted` bit beside `kept`; all other tiles, and every tile of the other
  // launches, take the form without it, whose schedule is the one rounds 1 - 3 measured (see PART above: the test costs 2 - 3 % when every
  // tile carries it).  The choice is block-uniform.
  auto k_substeps = [&](auto count_c) __attribute__((always_inline)) {
    constexpr bool COUNT = decltype(count_c)::value;
    // ---- sub-step 1: pull from the source grid; region = owned tile grown by (ksteps-1) rows / multi_ex(ksteps-1) columns
    {
      const int ey = ksteps - 1, ex = multi_ex(ey);
      const int wp = (TX + 2 * ex) / 2;                                 // pairs per region row
      const int np = wp * (TY + 2 * ey);
  #pragma unroll 1
      for (int i = tid; i < np; i += kLanes) {
        const int ry = i / wp, rp = i - ry * wp;
        const int fx = EX - ex + 2 * rp, fy = EY - ey + ry;               // LDS frame coordinates (fx even)
        f2 p[9], out[9];
        uint32_t mbits = 0, o_here = 0;
        int sr = 0;
        if (!pull(fx, fy, p, mbits, sr, o_here)) {
          if (ksteps > 1) pair_flags[(fy * W + fx) >> 1] = 0;
          continue;
        }
        bool kept, counted;
        classify(count_c, fx, fy, fx >= EX && fx < EX + TX && fy >= EY && fy < EY + TY, kept, counted);
        const bool accel_row_here = on_accel_row(sr);
        acc[0] += finish_pair_lo<TERMS>(p, mbits, a.omega, tile_accel, (ksteps > 1 || a.accel_last) && accel_row_here, a.accel_w1, a.accel_w2, counted ? mbits : 3u, out, acc_lo[0]);
        if (ksteps > 1) {
  #pragma unroll
          for (int k = 0; k < 9; ++k) store_pair<W>(lds + k * kCells, k, fy * W, fx, out[k]);
          pair_flags[(fy * W + fx) >> 1] = static_cast<uint8_t>(pair_flag_bits(mbits, kept, accel_row_here, COUNT && counted));
        } else if (kept) {
  #pragma unroll
          for (int k = 0; k < 9; ++k) __builtin_nontemporal_store(out[k], &at_byte<f2>(a.dstk[k], o_here));
        }
      }
    }
    LBM_MSTAMP(1);
    if constexpr (K >= 2) {
      __syncthreads();
      LBM_MSTAMP(2);
      // ---- sub-steps 2..ksteps: in place in the LDS frame, each on a region one row / zero or two columns smaller.
      // In place without holding a whole region in registers: sub-step j writes its row r where the
      // frame it read kept row r-1 (the frame creeps down one storage row per sub-step), and a region
      // of more than 512 pairs goes in passes of whole rows, bottom to top.  A pass reads, meets at a
      // barrier, then writes; what it overwrites (old rows up to its last row - 1) no later pass reads.
      auto in_lds_substep = [&](const int j) __attribute__((always_inline)) {
        const int ey = ksteps - j, ex = multi_ex(ey);
        const int wp = (TX + 2 * ex) / 2;                                // pairs per region row
        const int rows = TY + 2 * ey;
        const int rpp = kLanes / wp;                                       // whole rows per pass
        const bool last = j == ksteps;
        const int rd = (j - 2) * W, wr = (j - 1) * W;                      // storage shift of the frame read / written
        // lane t -> row t / wp of the pass.  (Round 4 tried rows dealt to ALIGNED 32-lane groups — LDS reads are served in 32-lane groups, and
        // nine groups of ten straddle two region rows here, a two-way bank conflict each: SQ_LDS_BANK_CONFLICT 90.5 M -> 29.0 M cycles per
        // launch, LDS-array cycles 240 M -> 179 M, and the launch time unchanged: profiles/r04/ab_lds_rowmap.txt.  Code not kept.)
        const int ry = tid / wp, rp = tid - ry * wp;
        const int fx = EX - ex + 2 * rp;
        for (int r0 = 0; r0 < rows; r0 += rpp) {        // one or two passes (compile-time count: unrolled)
          f2 outs[9];
          int slot = -1;
          const bool in_region = ry < rpp && r0 + ry < rows;
          // whole waves without work skip the pass; in the others every lane computes (an idle lane on the
          // region's first row) and only the write is predicated: no per-lane state to merge at the barrier
          if (__builtin_amdgcn_ballot_w64(in_region) != 0ull) {
            const int fy = EY - ey + (in_region ? r0 + ry : 0);
            const uint32_t fl = pair_flags[(fy * W + fx) >> 1];
            const bool lane_on = in_region && (fl & kPairComputed);
            f2 p[9];
            p[0] = *reinterpret_cast<const f2*>(lds + fy * W + fx - rd);
            read_pair(rd, fx, fy, p);
            const bool kept = lane_on && (fl & kPairKept);
            const bool counted = COUNT ? (lane_on && (fl & kPairCounted)) : kept;
            float term_lo = 0.0f;
            const double term = finish_pair_lo<TERMS>(p, fl & kPairObstacles, a.omega, tile_accel, (!last || a.accel_last) && (fl & kPairAccelRow), a.accel_w1, a.accel_w2,
                                                      counted ? (fl & kPairObstacles) : 3u, outs, term_lo);
  #pragma unroll
            for (int m = 1; m < K; ++m)
              if (m == j - 1) { acc[m] += term; acc_lo[m] += term_lo; }
            slot = !lane_on ? -1 : last ? (kept ? kept_cell(fx, fy) : -1) : fy * W - wr;   // in LDS: the row; fx is added below
          }
          if (!last) {
            __syncthreads();                     // every lane of the pass has read its neighbours
            if (slot >= 0) {
  #pragma unroll
              for (int k = 0; k < 9; ++k) store_pair<W>(lds + k * kCells, k, slot, fx, outs[k]);
            }
          } else if (slot >= 0) {
  #pragma unroll
            for (int k = 0; k < 9; ++k) __builtin_nontemporal_store(outs[k], &at_byte<f2>(a.dstk[k], 4u * static_cast<uint32_t>(slot)));
          }
        }
        if (!last) __syncthreads();
        LBM_MSTAMP(1 + j);
      };
      // compile-time sub-step index: region sizes, `last`, accumulator slot all fold
  #pragma unroll
      for (int j = 2; j <= K; ++j) in_lds_substep(j);
    }

  };

  // The same K sub-steps with the lanes dealt ONE OWNED x-pair each for the whole launch (G::owned_lanes: a tile of exactly as many
  // x-pairs as the block has lanes).  Lane t keeps pair (t mod TX/2, t / (TX/2)) of the tile: its flag bits (as pair_flags) and its
  // population 0, which never streams, live in registers, and its frame address is fixed — each sub-step moves it by a constant row.
  // The ring of each region (312 / 184 / 116 pairs at K = 4) is extra, term-free work on the first lanes: sub-step 1 runs one ring
  // item after the owned pass; sub-step j < K relaxes the owned pair and, on those lanes, reads one ring pair, meets at ONE barrier,
  // then relaxes the ring pair and writes both (the dealing above takes two passes for each of sub-steps 1 - 3, every pair with the
  // term code).  Each lane adds exactly one pair's term per sub-step: acc[j-1] is that term, its compensated low part already added.
  // Plane 0 and the flag byte are kept in LDS for ring pairs only (K = 5: no plane 0 at all, the ring pairs' population 0 in ring0).
  // Sub-step 1 has an interior form for tiles that are `inner` and hold no uncounted rows or columns (all but the edge tiles of a
  // launch), chosen by a block-uniform branch.  Every owned pair is then computed, kept and counted, no source wraps and no row is
  // missing, so it is two straight-line sections (the owned pair, then the ring pair of the first lanes) instead of one rolled body
  // that serves both: one vector offset per pair on nine block-uniform plane bases that hold the rows' -+ nx as well as the x -+ 1, the
  // owned pair's frame address the lane's fixed one, its flag bits constants.  The arithmetic of a pair is the same code in both forms,
  // and both forms share the in-LDS sub-steps: a second, specialised copy of those was 2 % faster at 8192 x 8192 and made the whole
  // kernel, the edge tiles' code included, 2.5 % slower at 1024 x 1024.
  auto owned_substeps = [&](auto count_c) __attribute__((always_inline)) {
    constexpr bool COUNT = decltype(count_c)::value;
    constexpr int TP = TX / 2;                                         // owned pairs per tile row
    static_assert(TP * TY == kLanes && G::ring_pairs(1) <= kLanes, "one owned pair and at most one ring pair per lane and sub-step");
    // ring pair i of sub-step j: the ey region rows below the tile, the ey above it, then per tile row the ex / 2 pairs on each side
    auto ring_pos = [&](auto jc, const int i, int& fx, int& fy) __attribute__((always_inline)) {
      constexpr int ey = K - decltype(jc)::value, ex = multi_ex(ey), ep = ex / 2, wp = TP + ep * 2, band = ey * wp;
      if (i < 2 * band) {
        const bool top = i >= band;
        const int q = top ? i - band : i, ry = q / wp, rp = q - ry * wp;
        fy = top ? EY + TY + ry : EY - ey + ry;
        fx = EX - ex + 2 * rp;
      } else {
        const int q = i - 2 * band, ry = q / (2 * ep), c = q - ry * (2 * ep);
        fy = EY + ry;
        fx = EX - ex + 2 * (c < ep ? c : c + TP);
      }
    };
    // G::compact0: where population 0 of the ring pair at frame position (fx, fy) lives — its index in sub-step 1's ring, the inverse of
    // ring_pos<1> (the later rings are subsets of the first).  Only the pair at the same position ever reads it back: population 0 does not stream.
    [[maybe_unused]] f2* const ring0 = reinterpret_cast<f2*>(lds + kPlanes * kCells);
    [[maybe_unused]] auto ring0_at = [&](const int fx, const int fy) __attribute__((always_inline)) -> f2* {
      constexpr int ep = EX / 2, wp = TP + ep * 2, band = EY * wp;        // sub-step 1: ey = EY, ex = EX
      const int rp = fx >> 1;
      const int i = fy < EY ? fy * wp + rp : fy >= EY + TY ? band + (fy - EY - TY) * wp + rp : 2 * band + (fy - EY) * (2 * ep) + (rp < ep ? rp : rp - TP);
      return ring0 + i;
    };
    // relaxation, bounce-back and accelerate_flow of one pair; returns its sum|u| term (0 where skip = 3).  term_c: kPairTermNone for
    // a ring pair, kPairTermOwned for the owned pair, kPairTermGuarded where one rolled body serves both (finish_pair_owned);
    // clean (wave-uniform): no lane of the wave drops a cell from its term, hence none holds an obstacle either
    auto relax = [&](auto term_c, const f2 (&p)[9], const uint32_t mbits, const bool accel, const uint32_t skip, const bool clean, f2 (&out)[9]) __attribute__((always_inline)) {
      const double term = finish_pair_owned<TERMS, decltype(term_c)::value>(p, mbits, a.omega, skip, clean, out);
      if (tile_accel) accelerate_pair(out, mbits, accel, a.accel_w1, a.accel_w2);
      return term;
    };
    constexpr std::integral_constant<int, kPairTermNone> ring_term{};
    constexpr std::integral_constant<int, kPairTermOwned> owned_term{};
    constexpr std::integral_constant<int, kPairTermGuarded> either_term{};
    const int py = tid / TP, ofx = EX + 2 * (tid - py * TP), ofy = EY + py;
    // The owned pair's frame accesses.  Its position is fixed for the launch and every plane, row and sub-step shift is a constant,
    // so each dword can be one ds_read_b32 / ds_write_b32 with a 16-bit immediate offset on a lane base that never changes.  Written
    // as plain loads and stores (read_pair, store_pair) hipcc pairs the two dwords of a split plane into ds_read2_b32 / ds_write2_b32,
    // whose 8-bit offsets do not span a plane, and builds a new base per plane and pass (12 v_add_u32 per in-frame sub-step).  A
    // relaxed wavefront-scope atomic access is the same LDS instruction and is left unpaired.  Three bases, byte offsets into the
    // frame, each set below everything a read or write of any sub-step reaches so that all immediates are >= 0: the interleaved
    // planes (2, 4), the split planes, and the last split plane, whose offsets pass 64 KB.  Sub-steps 2 .. K only: with the bases
    // alive through sub-step 1's pull as well the kernel needs more than its 80 VGPRs, so sub-step 1 stores through store_pair.
    constexpr int kLowI = (K - 1) * W, kLowS = (K - 1) * W + 1;       // dwords a sub-step reaches below the pair's own position
    constexpr int kImmDwords = 16384, kHiDwords = (kPlanes - 1) * kCells;
    static_assert((kPlanes - 2) * kCells + kLowS + W + WH + 1 < kImmDwords && kPlanes * kCells - kHiDwords < kImmDwords, "two split bases reach every plane");
    uint32_t own_bi = 0, own_bs = 0, own_bs_hi = 0;                    // set after sub-step 1
    auto own_split = [&](const int o) __attribute__((always_inline)) -> float* {          // dword o (a constant) above the split base
      return o < kImmDwords ? reinterpret_cast<float*>(reinterpret_cast<char*>(lds) + own_bs) + o
                            : reinterpret_cast<float*>(reinterpret_cast<char*>(lds) + own_bs_hi) + (o - kHiDwords);
    };
    auto own_inter = [&](const int o) __attribute__((always_inline)) -> unsigned long long* {
      return reinterpret_cast<unsigned long long*>(reinterpret_cast<float*>(reinterpret_cast<char*>(lds) + own_bi) + o);
    };
    auto ld1 = [&](const int o) __attribute__((always_inline)) { return __hip_atomic_load(own_split(o), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); };
    auto ld2 = [&](const int o) __attribute__((always_inline)) { return __builtin_bit_cast(f2, __hip_atomic_load(own_inter(o), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT)); };
    // read_pair(rd, ofx, ofy, p)
    auto read_pair_own = [&](const int rd, f2 (&p)[9]) __attribute__((always_inline)) {
      const int ci = kLowI - rd, cs = kLowS - rd;
      p[2] = ld2((2 - kPl) * kCells + ci - W);
      p[4] = ld2((4 - kPl) * kCells + ci + W);
      p[1] = f2{ld1((1 - kPl) * kCells + cs - 1), ld1((1 - kPl) * kCells + cs + WH)};
      p[5] = f2{ld1((5 - kPl) * kCells + cs - W - 1), ld1((5 - kPl) * kCells + cs - W + WH)};
      p[8] = f2{ld1((8 - kPl) * kCells + cs + W - 1), ld1((8 - kPl) * kCells + cs + W + WH)};
      p[3] = f2{ld1((3 - kPl) * kCells + cs), ld1((3 - kPl) * kCells + cs + WH + 1)};
      p[6] = f2{ld1((6 - kPl) * kCells + cs - W), ld1((6 - kPl) * kCells + cs - W + WH + 1)};
      p[7] = f2{ld1((7 - kPl) * kCells + cs + W), ld1((7 - kPl) * kCells + cs + W + WH + 1)};
    };
    // store_pair<W>(lds + (k - kPl) * kCells, k, ofy * W - wr, ofx, v[k]) for k = 1 .. 8
    auto store_pair_own = [&](const int wr, const f2 (&v)[9]) __attribute__((always_inline)) {
  #pragma unroll
      for (int k = 1; k < 9; ++k) {
        if (k == 2 || k == 4) {
          __hip_atomic_store(own_inter((k - kPl) * kCells + kLowI - wr), __builtin_bit_cast(unsigned long long, v[k]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        } else {
          __hip_atomic_store(own_split((k - kPl) * kCells + kLowS - wr), v[k].y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
          __hip_atomic_store(own_split((k - kPl) * kCells + kLowS - wr + WH), v[k].x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        }
      }
    };
    f2 own0 = f2{0.0f, 0.0f};                                          // population 0 of the owned pair
    uint32_t ofl = 0;                                                  // its flag bits; 0: not computed
    if (!COUNT && inner) {                                             // block-uniform
      // ---- sub-step 1, interior form: the owned pair, then a ring pair (the first G::ring_pairs(1) lanes)
      const float* const here0 = a.srck[0], * const here1 = a.srck[1] - 1, * const here3 = a.srck[3] + 1;
      const float* const south2 = a.srck[2] - nx, * const south5 = a.srck[5] - 1 - nx, * const south6 = a.srck[6] + 1 - nx;
      const float* const north4 = a.srck[4] + nx, * const north8 = a.srck[8] - 1 + nx, * const north7 = a.srck[7] + 1 + nx;
      // the mask's base is read here, with the plane bases, not between the loads of a pair behind a wait of its own; the address
      // space is named again because the compiler cannot see through the statement that holds the value in scalar registers
      typedef const __attribute__((address_space(1))) char* global_bytes;
      const uint32_t* mask_arg = a.mask;
      asm volatile("" : "+s"(mask_arg));
      const global_bytes mask = (global_bytes)mask_arg;
      auto pull_inner = [&](const int fx, const int fy, f2 (&p)[9], uint32_t& mbits) __attribute__((always_inline)) -> uint32_t {
        const int cell = tile_row_base + __mul24(fy - EY, nx) + x0 + fx - EX;
        const uint32_t o = 4u * static_cast<uint32_t>(cell);
        p[0] = at_byte<f2>(here0, o);                                                    // :530-538
        p[2] = at_byte<f2>(south2, o);
        p[4] = at_byte<f2>(north4, o);
        p[1] = at_byte<f2u>(here1, o);
        p[5] = at_byte<f2u>(south5, o);
        p[8] = at_byte<f2u>(north8, o);
        p[3] = at_byte<f2u>(here3, o);
        p[6] = at_byte<f2u>(south6, o);
        p[7] = at_byte<f2u>(north7, o);
        mbits = (*(const __attribute__((address_space(1))) uint32_t*)(mask + 4u * (static_cast<uint32_t>(cell) >> 5)) >> (cell & 31)) & 3u;
        return o;
      };
      {
        f2 p[9], out[9];
        uint32_t mbits;
        pull_inner(ofx, ofy, p, mbits);
        const bool accel_row_here = on_accel_row(sy0 + py);
        acc[0] = relax(owned_term, p, mbits, accel_row_here, mbits, __builtin_amdgcn_ballot_w64(mbits != 0u) == 0ull, out);
  #pragma unroll
        for (int k = 1; k < 9; ++k) store_pair<W>(lds + (k - kPl) * kCells, k, ofy * W, ofx, out[k]);
        own0 = out[0];
        ofl = pair_flag_bits(mbits, true, accel_row_here, false);
      }
      if (tid < G::ring_pairs(1)) {
        int fx, fy;
        ring_pos(std::integral_constant<int, 1>{}, tid, fx, fy);
        f2 p[9], out[9];
        uint32_t mbits;
        pull_inner(fx, fy, p, mbits);
        const bool accel_row_here = on_accel_row(sy0 + fy - EY);
        relax(ring_term, p, mbits, accel_row_here, 3u, false, out);
  #pragma unroll
        for (int k = kPl; k < 9; ++k) store_pair<W>(lds + (k - kPl) * kCells, k, fy * W, fx, out[k]);
        if constexpr (G::compact0) ring0[tid] = out[0];
        pair_flags[(fy * W + fx) >> 1] = static_cast<uint8_t>(pair_flag_bits(mbits, false, accel_row_here, false));
      }
    } else {
    // ---- sub-step 1: item 0 = the owned pair, item 1 = a ring pair (the first G::ring_pairs(1) lanes)
  #pragma unroll 1
    for (int item = 0; item < 2; ++item) {
      const bool own = item == 0;
      if (!own && tid >= G::ring_pairs(1)) break;
      int fx = ofx, fy = ofy;
      if (!own) ring_pos(std::integral_constant<int, 1>{}, tid, fx, fy);
      f2 p[9];
      uint32_t mbits = 0, fl = 0, o_here = 0;
      int sr = 0;
      if (pull(fx, fy, p, mbits, sr, o_here)) {
        bool kept, counted;
        classify(count_c, fx, fy, own, kept, counted);
        const bool accel_row_here = on_accel_row(sr);
        f2 out[9];
        const double term = relax(either_term, p, mbits, accel_row_here, counted ? mbits : 3u, false, out);
  #pragma unroll
        for (int k = 1; k < 9; ++k) store_pair<W>(lds + (k - kPl) * kCells, k, fy * W, fx, out[k]);
        fl = pair_flag_bits(mbits, kept, accel_row_here, COUNT && counted);
        if (own) {
          acc[0] = term;
          own0 = out[0];
        } else if constexpr (G::compact0) {
          ring0[tid] = out[0];
        } else {
          store_pair<W>(lds, 0, fy * W, fx, out[0]);
        }
      }
      if (own) ofl = fl;
      else pair_flags[(fy * W + fx) >> 1] = static_cast<uint8_t>(fl);
    }
    }
    LBM_MSTAMP(1);
    __syncthreads();
    LBM_MSTAMP(2);
    // the three bases, from here on in their registers: left to itself hipcc derives them again from the lane index in every sub-step
    own_bi = 4u * static_cast<uint32_t>(ofy * W + ofx - kLowI); own_bs = 4u * static_cast<uint32_t>(ofy * W + (ofx >> 1) - kLowS);
    own_bs_hi = own_bs + 4u * kHiDwords;
    asm volatile("" : "+v"(own_bi), "+v"(own_bs), "+v"(own_bs_hi));
    // the owned pair's flags do not change either: is this a wave in which every lane counts both its cells ?
    const bool own_clean = __builtin_amdgcn_ballot_w64(((ofl & (COUNT ? kPairCounted : kPairKept)) != 0u ? ofl & kPairObstacles : 3u) != 0u) == 0ull;
    // ---- sub-steps 2..K in place, the frame creeping down one row per sub-step as in k_substeps
    auto in_lds_substep = [&](auto jc) __attribute__((always_inline)) {
      constexpr int j = decltype(jc)::value;
      constexpr bool last = j == K;
      constexpr int rd = (j - 2) * W, wr = (j - 1) * W;                // storage shift of the frame read / written
      f2 p[9], outs[9];
      read_pair_own(rd, p);
      p[0] = own0;
      const uint32_t mbits = ofl & kPairObstacles;
      const bool counted = (ofl & (COUNT ? kPairCounted : kPairKept)) != 0u;
      acc[j - 1] = relax(owned_term, p, mbits, (!last || a.accel_last) && (ofl & kPairAccelRow), counted ? mbits : 3u, own_clean, outs);
      own0 = outs[0];
      if constexpr (!last) {
        // the ring pair's populations are READ before the barrier and relaxed after it, once the owned results are stored: a lane
        // never holds the results of one pair while it computes the other
        f2 q[9];
        int rfx = 0, rfy = 0;
        uint32_t rfl = 0;
        [[maybe_unused]] f2* r0 = nullptr;
        const bool ring = tid < G::ring_pairs(j);
        if (ring) {
          ring_pos(jc, tid, rfx, rfy);
          rfl = pair_flags[(rfy * W + rfx) >> 1];
          read_pair(rd, rfx, rfy, q);
          if constexpr (G::compact0) { r0 = ring0_at(rfx, rfy); q[0] = *r0; }
          else q[0] = *reinterpret_cast<const f2*>(lds + rfy * W + rfx - rd);
        }
        __syncthreads();                       // every lane has read its neighbours
        if (ofl & kPairComputed) store_pair_own(wr, outs);
        if (ring) {
          f2 routs[9];
          relax(ring_term, q, rfl & kPairObstacles, (rfl & kPairAccelRow) != 0u, 3u, false, routs);
          if (rfl & kPairComputed) {
  #pragma unroll
            for (int k = kPl; k < 9; ++k) store_pair<W>(lds + (k - kPl) * kCells, k, rfy * W - wr, rfx, routs[k]);
            if constexpr (G::compact0) *r0 = routs[0];
          }
        }
        __syncthreads();
      } else if (ofl & kPairKept) {
        const uint32_t o = 4u * static_cast<uint32_t>(kept_cell(ofx, ofy));
  #pragma unroll
        for (int k = 0; k < 9; ++k) __builtin_nontemporal_store(outs[k], &at_byte<f2>(a.dstk[k], o));
      }
      LBM_MSTAMP(1 + j);
    };
    in_lds_substep(std::integral_constant<int, 2>{});
    if constexpr (K >= 3) in_lds_substep(std::integral_constant<int, K >= 3 ? 3 : 2>{});
    if constexpr (K >= 4) in_lds_substep(std::integral_constant<int, K >= 4 ? 4 : 2>{});
    if constexpr (K >= 5) in_lds_substep(std::integral_constant<int, K >= 5 ? 5 : 2>{});
  };
  auto substeps = [&](auto count_c) __attribute__((always_inline)) {
    if constexpr (G::owned_lanes) owned_substeps(count_c);
    else k_substeps(count_c);
  };

  if constexpr (PART == kPartGhost) {
    if (sy0 >= a.count_first && sy0 + TY <= a.count_end) substeps(std::false_type{});       // every row of the tile counts
    else substeps(std::true_type{});
  } else if constexpr (PART == kPartTile) {
    if (sy0 >= a.count_first && sy0 + TY <= a.count_end && x0 >= a.cx0 && x0 + TX <= a.cx1) substeps(std::false_type{});   // ... and every column
    else substeps(std::true_type{});
  } else {
    substeps(std::false_type{});
  }

  // per-step sums over the owned cells of this tile
  if constexpr ((TERMS & ~kTermsFused) == kTermsCompensated && !G::owned_lanes) {
#pragma unroll
    for (int i = 0; i < K; ++i) acc[i] += static_cast<double>(acc_lo[i]);
  }
  if constexpr (K == 1) {
    const double w = wave_sum(acc[0]);
    if ((tid & 63) == 0) red[tid >> 6] = w;
  } else if constexpr (K <= 4) {
    const double w = wave_sum_vec4(acc[0], acc[1], K > 2 ? acc[2] : 0.0, K > 3 ? acc[K > 3 ? 3 : 0] : 0.0);
    const int q = wave_sum_slot<4>(tid & 63);
    if ((tid & 15) == 0 && q < K) red[q * kWaves + (tid >> 6)] = w;
  } else {
    static_assert(K <= 8, "wave_sum_vec8 carries eight steps");
    double acc8[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc8[i] = i < K ? acc[i < K ? i : 0] : 0.0;
    const double w = wave_sum_vec8(acc8);
    const int q = wave_sum_slot<8>(tid & 63);
    if ((tid & 7) == 0 && q < K) red[q * kWaves + (tid >> 6)] = w;
  }
  lds_barrier();                 // LDS only: the block does not wait for its own global stores to complete
  if (tid < ksteps) {
    double t = 0.0;
    for (int w = 0; w < kWaves; ++w) t += red[tid * kWaves + w];
    a.partials_out[static_cast<size_t>(tid) * a.ntiles_total + tile] = t;
  }
  LBM_MSTAMP(2 + K);
}

}  // namespace
