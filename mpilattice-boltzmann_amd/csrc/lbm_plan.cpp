// lbm_plan.cpp — the host-only planning unit of liblbm_d2q9.so: which kernel, which geometry and which buffer sizes a context
// gets, and what each launch of a run covers.  No HIP call and no device pointer anywhere in this file, so every rule here can be
// read, called and tested on a CPU (tests/test_plan.py and tests/test_launch_plan.py, through the lbm_plan_* exports at the end).
//
//   the rules        macro_eligible, macro_k_for, macro_ghost_for, macro_group_for, pick_geom, plane_stride_floats, pick_iters,
//                    blocks_for — each with the measurements behind it
//   the layouts      rank_layout (row blocks), tile_layout_of (tiles), lbm_choose_rank_grid (which of the two): one answer for all
//                    ranks of a run, from global quantities only
//   the plan         plan_context fills a ContextPlan (lbm_internal.h): everything lbm_create* decides that does not depend on
//                    a device pointer.  plan_whole / plan_rank / plan_tile are its three callers, one per way of creating a
//                    context; lbm_kernels.hip allocates, uploads and launches by the plan and never writes it
//   the names        family_of(plan) and plan_kernel_name(plan): the only place the kernel families' names are spelled
//   the launches     lbm_plan_next / lbm_plan_group_for cut a run into launches and groups; plan_launch fills a LaunchPlan: the rows,
//                    columns, tiles (macro_rows, macro_rects), grid and kernel-table row of one launch of lbm_multi_kernel
//                    (plan_tile_launch: of lbm_tile_kernel); edge_rows_suffice and plan_column_message are the exchange's two
//                    geometric rules.  No heap allocation anywhere on this path: it runs once per launch
//
// Refusals keep the words and the order lbm_create* always had: what was checked before the device was touched returns
// kPlanRefused, what was checked after it kPlanRefusedLate (the caller lets a bad device speak first).

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "lbm_d2q9.h"
#include "lbm_d2q9_f64_rows.h"
#include "lbm_d2q9_f64_cols.h"
#include "lbm_geometry.h"
#include "lbm_internal.h"
#include "lbm_knobs.h"

using lbm_internal::ContextPlan;
using lbm_internal::set_error;

namespace lbm_internal {

// Plane stride, in elements (floats here, doubles in lbm_f64.hip: the same rule): rows*nx elements + guard for the dword-shifted loads at both ends, rounded to 64 elements (256 B of floats),
// then skewed by an odd number of such units so the 9 planes (and the two grids) do not all start
// on the same HBM channel when rows*nx is a large power of two.
size_t plane_stride_floats(size_t ncells, int skew)
{
  size_t s = (ncells + 64 + 63) / 64 * 64;
  if ((s / 64) % 2 == 0) s += 64;
  // Skew between planes for large grids (planes of 8192 x 8192 floats are 2^28 bytes: nine streams on the same channels without one).
  // 24 x 256 B = 6 KiB.  Rounds 1-2 used 34 (tuned on the K = 3 launch, 64 x 16 tiles); scanned again on the K = 4 launch on 64 x 23 tiles,
  // 8192 x 8192, us/step for skews 0 / 8 / 16 / 24 / 33 / 34 / 40 / 48 / 68: K = 4 286.7 / 284.6 / 285.8 / 284.7 / 314.3 / 307.8 & 295.3 / 289.0 /
  // 285.1 / 286.6; K = 3 (the tails) 384.6 & 329.5 / 341.1 / 324.0 / 317.9 / 339.8 / 339.7 & 348.5 / 323.5 / 335.4 / 333.7 — 33 and 34 are the
  // two bad values for the tall tiles, 24 is best for both; other sizes (4096 x 4096 ... 16384 x 4096, partitions) do not care
  // (profiles/r03/ab_skew_scan.txt, ab_skew_sizes.txt).
  if (ncells >= (1u << 20)) s += 64 * static_cast<size_t>(skew);
  return s;
}

// max_blocks (LBM_TUNE_MAXBLOCKS): measured on 8192x8192, 16384 blocks x 4 chunks ~7 % faster than 4096 x 16
int pick_iters(long long quads, int max_blocks)
{
  // keep the grid at <= ~4096 blocks (16 per CU): fewer, longer blocks and a short partial vector
  long long chunks = (quads + kBlock - 1) / kBlock;
  int iters = 1;
  while (chunks / iters > max_blocks && iters < 1024) iters *= 2;
  return iters;
}

int blocks_for(long long quads, int iters)
{
  const long long per_block = static_cast<long long>(kBlock) * iters;
  return static_cast<int>((quads + per_block - 1) / per_block);
}

}  // namespace lbm_internal

namespace {

// What every launch of lbm_multi_kernel needs of the rows it works on, whole grid or partition: a plane addressed with 32-bit byte
// offsets (< 2^30 storage cells, the deepest ghost rows included) and 24-bit row multiplies (nx < 2^23).
bool multi_addressable(int nx, int rows)
{
  return static_cast<size_t>(nx) * (rows + 2 * kMaxGhost) < (size_t(1) << 30) && nx < (1 << 23);
}

// Is a row partition of `rows` rows eligible for K-step mode (lbm_multi_kernel with ghost rows) ?  At least 32 rows, and rows of whole
// 64-wide tiles or of any even width from 128 cells.
bool macro_eligible(const lbm_params* p, int rows, unsigned flags)
{
  return !(flags & LBM_FLAG_ONE_STEP) && rows >= 2 * kMTY && multi_addressable(p->nx, rows) && (p->nx % kMTX == 0 || (p->nx % 2 == 0 && p->nx >= 2 * kMTX));
}

// Does lbm_multi_kernel tile a whole periodic grid ?  Grids tiled exactly by 64x16, or any even nx >= 128 with ny >= 32, where the last
// tile column / row sticks out of the grid (periodic images: computed, not kept).  Not the partitions' rule: a whole grid of fewer than
// 32 rows that 64 x 16 tiles exactly is taken.
bool whole_grid_tiled(int nx, int ny)
{
  return multi_addressable(nx, ny) && ((nx % kMTX == 0 && ny % kMTY == 0) || (nx % 2 == 0 && nx >= 2 * kMTX && ny >= 2 * kMTY));
}

// K of the K-step partitions, whatever their size (LBM_TUNE_MACRO_K overrides).  Measured on a 1-rank ring with the packed exchange,
// us/step for K = 2 / 3 / 4 (one-step loop):
//   8192x4096 rows 243 / 182 / 199   8192x2048 rows 122 / 92.6 / 103   8192x1024 rows 66.2 / 52.5 / 55.9 (116)
//   1024x128 rows 26.1 / 18.8 / 14.7 (37)
// Round 3: with the 4-step launch on 64 x 13 tiles (three blocks per CU, kernels/multi.h) K = 4 wins at every size — 1-rank
// p2p rings, us/step for K = 3 / K = 4: 8192x4096 178.9 / 166.2, 8192x1024 51.3 / 48.5, 1024x128 4.40 / 4.04.
int macro_k_for(const Knobs& knobs)
{
  return std::min(std::max(knobs.macro_k, 0), kMaxMultiSteps);
}

// Ghost rows kept on each side of a K-step partition, and with them how often it exchanges: the launches between two exchanges (a
// GROUP) make at most `ghost` steps together.  Round 4: the first launch of a group also advances `ext` = (steps of the later ones)
// ghost rows on each side from the exchanged rows, so the later ones are launches over all tiles that read no exchanged row: no
// interior / edge split, no push, no wait, no join.  Rounds 1-3 kept K rows (4 at K = 3) and exchanged before every launch.
//   partitions that run the edge-stream schedule (>= 2 M cells): 2 K rows (8 at K = 3: 3 + 4, 4 + 4, 3 + 3), two launches per exchange —
//     1-rank ring of 8192 x 1024 rows, us/step at 20 / 200 steps per run for K, 8, 12, 16 rows: 48.1 / 45.7, 46.8 / 43.8, 46.5 / 43.7, 47.2 / 43.9
//     (profiles/r04/rings_p2p_final_build.txt: past two launches per exchange nothing more is gained, so the fewest ghost rows stay);
//   smaller ones (everything on one stream: each exchange is an exposed push + wait): as deep as their rows carry — 16 rows (four
//     launches per exchange) from 128 rows per rank, 8 from 64, K below (a 32-row rank would compute 56 rows in a group's first launch) —
//     1024 x 128 rows: 4.85 (K rows), 4.23 (8), 3.85 (12), 3.84 (16) us/step at 200 steps, 6.40 / 6.12 / 5.87 / 5.65 at 20
//     (profiles/r04/rings_p2p_small.txt; with the neighbours' "ready" awaited inside the push kernel, by every block or by block 0 with a
//     go word for the rest, 8 rows were no faster than K: 4.95 - 5.76 — the wait now sits in the fold block of the group's last launch).
// One answer for all ranks: from nx and the smallest / largest row count of the run.  LBM_TUNE_MACRO_GHOST overrides (0 or anything
// below K: K rows, one launch per exchange).  The exchange moves the rows the NEXT group needs (peer-to-peer loop) or all `ghost`
// rows (RCCL loop).
int macro_ghost_for(const Knobs& knobs, int k, int nx, int rows_min, int rows_max, bool row_blocks = true)
{
  if (k <= 0) return 0;
  const int classic = k == 3 ? 4 : k, two = k == 3 ? 8 : 2 * k;
  int by_size = two;
  if (static_cast<size_t>(nx) * rows_max < (size_t(1) << 21)) by_size = rows_min >= 128 ? std::max(16 / k * k, two) : rows_min >= 64 ? two : classic;
  // ... and deeper still for the smallest ranks (round 4, last: kMaxGhost 16 -> 32), whose launches are bound by latency, not by the rows they
  // compute: us/step for 16 / 24 / 32 ghost rows — 1024 x 128 rows 3.30 / 3.14 / 3.10, 1024 x 256 3.97 / 3.82 / 3.76, 512 x 512 3.86 / 3.70 / 3.63,
  // 2048 x 256 5.50 / 5.40 / 5.33; not for wider or larger ones: 4096 x 128 6.03 / 6.18 / 6.22, 8192 x 128 10.2 / 10.5 / 10.6, 2048 x 512 7.75 / 7.70 / 7.97,
  // 1024 x 1024 7.4 / 7.3 / 7.4, and 1024 x 192 3.40 / 3.43 / 3.55 (profiles/r04/ab_row_block_ghost_depth.txt): 24 rows from 128 rows per rank, 32 from 256,
  // for ranks of at most 2^19 cells in rows of at most 2048 cells
  if (row_blocks && nx <= 2048 && static_cast<size_t>(nx) * rows_max <= (size_t(1) << 19) && rows_min >= 128)     // (tile ranks: lbm_tile_layout_of has its own rule)
    by_size = std::max(by_size, std::min((rows_min >= 256 ? 32 : 24) / k * k, static_cast<int>(kMaxGhost)));
  return std::min(std::max(knob_or(knobs.macro_ghost, by_size), k), kMaxGhost);
}

// Most launches per exchange: what the ghost rows allow (LBM_TUNE_MACRO_GROUP caps it; 1 = rounds 1-3's loop on any number of ghost rows).
int macro_group_for(const Knobs& knobs, int k, int ghost)
{
  if (k <= 0) return 1;
  return std::min(std::max(knob_or(knobs.macro_group, std::max(ghost / k, 1)), 1), kMaxGroup);
}

// Geometry of lbm_multi_kernel's launches by partition size.  Width: 64 x 16 tiles for the bandwidth-bound grids; 32 x 16 where 64 x 16
// tiles would not even fill the chip once (256 CUs x 3 blocks), so that the launch is bound by one block's chain of
// sub-steps: half the work per block, twice the blocks.  Measured us/step for 64 / 32 wide tiles (K = 3, one GPU):
// 1024x128 3.22 / 2.53, 512x256 3.17 / 2.50, 512x512 3.42 / 3.44, 2048x256 4.94 / 5.05, 1024x1024 8.39 / 9.01.
// LBM_TUNE_MULTI_TILE = 64 / 32 overrides the width; LBM_TUNE_MULTI_GEOM = 0 / 1 / 2 the whole choice.
// The tall geometry (K = 4 on 64 x 24 tiles, 768-lane blocks, two per CU) from 2^20 cells up: where a launch is several rounds of
// blocks it is 4 - 10 % faster, at one round or less its 512 slots lose to 768 (kernels/multi.h).
// Row partitions (interior + edge launch per macro-step) follow the same rule.  Measured one ring per PROCESS, as ranks run (two rings in
// one process can share a hardware queue, which made the tall geometry look 20 % worse in a same-process A/B): standard / tall, us/step
// at 200 and 20 steps per run: 8192 x 1024 rows 46.5 / 45.5 and 48.2 / 48.1, 8192 x 2048 rows 86.9 / 82.4 and 88.9 / 84.2
// (profiles/r03/ab_fused_schedule.txt).
int pick_geom(const Knobs& knobs, size_t ncells)
{
  const int by_size = ncells <= static_cast<size_t>(knobs.narrow_tile_max) ? kMTXNarrow : kMTX;
  const int t = knob_or(knobs.multi_tile, by_size);
  int g = t == kMTXNarrow ? kGeomNarrow : ncells >= static_cast<size_t>(knobs.tall_tile_min) ? kGeomTall : kGeomStd;
  if (knobs.multi_geom >= kGeomStd && knobs.multi_geom <= kGeomTall) g = knobs.multi_geom;
  return g;
}

// One mode and one K for every rank of a run, from global quantities only (see the header).
int rank_layout(const Knobs& knobs, const lbm_params* p, int nranks, int rank, unsigned flags, lbm_layout* out)
{
  if (!p || !out || nranks < 1 || rank < 0 || rank >= nranks) { set_error("lbm_rank_layout: bad argument"); return 1; }
  if (p->nx < 1 || p->ny < 3 || p->ny < nranks) { set_error("lbm_rank_layout: grid too small for this many ranks"); return 1; }
  std::vector<int> nyl(nranks), dis(nranks);
  if (lbm_decompose(p->ny, nranks, nyl.data(), dis.data())) return 1;                 // d2q9-bgk.c:834-862
  const int lo = *std::min_element(nyl.begin(), nyl.end()), hi = *std::max_element(nyl.begin(), nyl.end());
  if (lo < 1) { set_error("lbm_rank_layout: a rank would own no rows"); return 1; }
  out->y0 = dis[rank];
  out->ny_local = nyl[rank];
  out->macro_k = 0;
  const bool partitioned = nranks > 1 || (flags & LBM_FLAG_FORCE_HALO);
  if (partitioned && macro_eligible(p, lo, flags) && macro_eligible(p, hi, flags))
    out->macro_k = macro_k_for(knobs);
  out->ghost = macro_ghost_for(knobs, out->macro_k, p->nx, lo, hi);
  out->group = macro_group_for(knobs, out->macro_k, out->ghost);
  return 0;
}

// ---- tile (2-D) decomposition: px x py ranks, rank = ry * px + rx ------------------------------------------------------------
// Rows by the reference's rule over py (d2q9-bgk.c:834-862), columns by lbm_decompose_columns over px.  Always K-step mode: ghost rows
// as a row partition of the same cells would keep, ghost columns the same number rounded up to even (x-pairs).
int tile_layout_of(const Knobs& knobs, const lbm_params* p, int px, int py, int rank, unsigned flags, lbm_tile_layout* out)
{
  if (!p || !out || px < 1 || py < 1 || rank < 0 || rank >= px * py) { set_error("lbm_tile_layout_of: bad argument"); return 1; }
  if (p->nx < 1 || p->ny < 3 || p->ny < py) { set_error("lbm_tile_layout_of: grid too small for this many ranks"); return 1; }
  std::vector<int> nyl(py), ydis(py), nxl(px), xdis(px);
  if (lbm_decompose(p->ny, py, nyl.data(), ydis.data())) return 1;
  if (lbm_decompose_columns(p->nx, px, nxl.data(), xdis.data())) return 1;
  const int rlo = *std::min_element(nyl.begin(), nyl.end()), rhi = *std::max_element(nyl.begin(), nyl.end());
  const int clo = *std::min_element(nxl.begin(), nxl.end()), chi = *std::max_element(nxl.begin(), nxl.end());
  if (rlo < 1) { set_error("lbm_tile_layout_of: a rank would own no rows"); return 1; }
  std::memset(out, 0, sizeof *out);
  out->px = px; out->py = py; out->rx = rank % px; out->ry = rank / px;
  out->x0 = xdis[out->rx]; out->nx_local = nxl[out->rx];
  out->y0 = ydis[out->ry]; out->ny_local = nyl[out->ry];
  const int k = macro_k_for(knobs);
  int ghost = macro_ghost_for(knobs, k, chi, rlo, rhi, /*row_blocks=*/false);
  // Column blocks (py = 1) below the edge-stream size: 32 ghost columns, eight launches per exchange.  Their ghost depth costs columns only (no
  // launch advances ghost rows), and their launches are bound by latency, not by the cells they compute: us/step for 16 / 24 / 32 ghost columns
  // 2048 x 512 8.05 / 8.00 / 7.85, 4096 x 256 8.40 / 8.21 / 8.18, 8192 x 128 8.77 / 8.58 / 8.46, 512 x 512 4.06 / 3.96 / 3.87, 256 x 512 3.32 / 3.20 / 3.14
  // (profiles/r04/ab_column_block_ghost_depth.txt).  LBM_TUNE_MACRO_GHOST still overrides.
  if (k > 0 && py == 1 && clo >= 256 && !knobs.tile_ghost_rows && static_cast<size_t>(chi) * rhi < (size_t(1) << 21) && knobs.macro_ghost < 0)   // (blocks of >= 256 columns: the measured range)
    ghost = std::max(ghost, std::min(32 / k * k, static_cast<int>(kMaxGhost)));
  int ghost_x = (ghost + 1) & ~1;
  ghost_x = std::min(std::max(knob_or(knobs.tile_ghost_x, ghost_x) & ~1, ghost_x), kMaxGhost);
  // every rank's storage rows (owned + ghost columns) must be ones the K-step kernels take, and its own columns at least the ghost
  // columns its neighbours need from it
  lbm_params narrow = *p, wide = *p;
  narrow.nx = clo + 2 * ghost_x; wide.nx = chi + 2 * ghost_x;
  if (k <= 0 || !macro_eligible(&narrow, rlo, flags) || !macro_eligible(&wide, rhi, flags) || !macro_eligible(&narrow, rhi, flags) || !macro_eligible(&wide, rlo, flags) ||
      clo < ghost_x || (py > 1 && rlo < ghost)) {
    set_error("lbm_tile_layout_of: the tile decomposition runs in K-step mode only: every rank needs >= 32 rows, an even number of columns with "
                            "at least 128 storage columns (owned + ghost) and LBM_FLAG_ONE_STEP clear — use the row decomposition (lbm_rank_layout)");
    return 1;
  }
  out->macro_k = k; out->ghost = ghost; out->ghost_x = ghost_x;
  out->group = macro_group_for(knobs, k, ghost);
  // column blocks (py = 1: every rank owns all rows) keep no ghost rows: their launches wrap in y like a whole grid's, and an exchange is the
  // column push alone.  LBM_TUNE_TILE_GHOST_ROWS=1 keeps them (a 1 x 1 ring then stands for a block of ANY tiling: the rank is its own south
  // and north neighbour through the row push, as it is its own west and east one)
  out->ghost_y = (py == 1 && !knobs.tile_ghost_rows) ? 0 : ghost;
  return 0;
}

// lbm_create_tile's part of a plan: `p->nx` is then the storage row width nxl + 2 ghost_x
struct TileSpec { int px, py, rx, ry, x0, nxl, ghost_x, nx_global, ghost_rows; };

// Launch geometry of a context that runs lbm_multi_kernel (K-step partitions and whole grids alike): the geometry by size, its tile width,
// and room for the partials of its longest launch (no ghost rows where the rows wrap).
void plan_multi(const Knobs& knobs, bool tile_rank, ContextPlan& c)
{
  c.multi_geom = pick_geom(knobs, static_cast<size_t>(c.ncells));
  if (tile_rank && c.ghost_rows == 0 && c.multi_geom == kGeomTall && knobs.multi_geom < 0) {
    // A column block's launches all cover exactly its ny rows: where 23-row tiles fit them badly the last tile row is mostly waste — 256 rows: 12
    // tile rows cover 276 (7.8 % over) against 260 on 13-row tiles; 128 rows: 138 against 130 — and the standard geometry wins by 10 % (us/step
    // tall / standard: 4096 x 256 8.96 / 8.11, 8192 x 128 9.40 / 8.37; 512 and 1024 rows fit: 2048 x 512 7.82 / 8.25, 1024 x 1024 8.20 / 8.60, 2048 x 1024
    // 13.8 / 14.1; profiles/r04/ab_column_block_geometry.txt).  Row blocks and whole grids compute different row counts from launch to launch (no rule).
    auto over = [&](int ty) { return static_cast<double>((c.nyl + ty - 1) / ty * ty) / c.nyl; };
    if (over(kMTY4Tall) - over(kMTY4) > 0.03) c.multi_geom = kGeomStd;
  }
  c.multi_tx = geom_tx(c.multi_geom);
  c.multi_tiles_x = (c.nx + c.multi_tx - 1) / c.multi_tx;
  // (a context of the five-step launch: five vectors, over the tiles of its shortest tail's geometry)
  const int vecs = c.multi_K > kMaxMultiSteps ? c.multi_K : kMaxMultiSteps;
  if (c.multi_K > 0) c.partials_cap = std::max(c.partials_cap, vecs * c.multi_tiles_x * ((c.nyl + 2 * c.ghost_rows + kMinMultiTY - 1) / kMinMultiTY) + 1);
}

// Five steps per launch (lbm_multi_kernel<5, TERMS, kGeomTall, kPartPlain>, lbm_geometry.h kMaxWholeGridSteps) is built for whole periodic
// grids on the tall geometry only: no ghost rows to advance, no ready words, no ghost columns.
bool five_steps_eligible(const ContextPlan& c, unsigned flags)
{
  return c.self_periodic && c.ghost == 0 && c.ghost_x == 0 && !c.tile_kernel && !(flags & LBM_FLAG_ONE_STEP) && c.multi_geom == kGeomTall;
}

// The one function that decides: lbm_create / lbm_create_global / lbm_create_rank / lbm_create_tile all end here.  The obstacle flags of
// the ghost rows that the K-step kernels need come either from the whole map (has_global_map, lbm_create_global) or from the rank's
// window (has_window, lbm_create_rank / lbm_create_tile); neither = no ghost rows possible.  forced_k < 0: K-step mode and K decided
// from this partition's own shape (lbm_create_global); >= 0: decided by the caller for the whole run (rank_layout, tile_layout_of).
int plan_context(const Knobs& knobs, const lbm_params* p, int free_cells, bool has_global_map, bool has_window, int forced_k, int forced_ghost,
                 int y0, int ny_local, unsigned flags, const TileSpec* tile, ContextPlan* out)
{
  if (!p || !out) { set_error("lbm_create: null argument"); return lbm_internal::kPlanRefused; }
  if (p->nx < 1) { set_error("lbm_create: nx must be positive"); return lbm_internal::kPlanRefused; }
  if (p->ny < 3) { set_error("lbm_create: ny must be >= 3 (accelerate_flow works on row ny-2, d2q9-bgk.c:449)"); return lbm_internal::kPlanRefused; }
  if (ny_local < 1 || y0 < 0 || y0 + ny_local > p->ny) { set_error("lbm_create: partition rows out of range"); return lbm_internal::kPlanRefused; }
  if (free_cells <= 0) { set_error("lbm_create: free_cells must be positive"); return lbm_internal::kPlanRefused; }
  if (flags & LBM_FLAG_FUSED_ARITH) {
    // one form of the sum|u| terms per kernel family for the fused arithmetic (that family's default): the flags that ask for another are refused
    if (flags & (LBM_FLAG_FAST_AVVELS | LBM_FLAG_EXACT_AVVELS)) {
      set_error("lbm_create: LBM_FLAG_FUSED_ARITH cannot be combined with LBM_FLAG_FAST_AVVELS or LBM_FLAG_EXACT_AVVELS (the fused kernels carry each family's default sum|u| terms only)");
      return lbm_internal::kPlanRefused;
    }
  }
  const bool self_periodic = (ny_local == p->ny) && !(flags & LBM_FLAG_FORCE_HALO);
  const int accel_global = p->ny - 2;
  int accel_row = -1;
  if (accel_global >= y0 && accel_global < y0 + ny_local) accel_row = accel_global - y0;
  if (!self_periodic && accel_row >= 0 && (accel_row == 0 || accel_row == ny_local - 1)) {
    set_error("lbm_create: the partition holding row ny-2 needs >= 3 rows (d2q9-bgk.c:848-849)");
    return lbm_internal::kPlanRefused;
  }
  if (static_cast<long long>(p->nx) * ny_local > (1LL << 31) - 4096) { set_error("lbm_create: partition too large for 32-bit cell indices"); return lbm_internal::kPlanRefused; }

  // ---- from here on lbm_create* has always had the device current: refusals are kPlanRefusedLate ----
  ContextPlan c;
  std::memset(&c, 0, sizeof c);
  c.flags = flags;
  c.nx = p->nx; c.y0 = y0; c.nyl = ny_local;
  c.free_cells_inv = 1.0f / free_cells;                                    // d2q9-bgk.c:950
  c.nxl = c.nx_global = p->nx;
  c.tiles_px = c.tiles_py = 1;
  if (tile) {
    c.ghost_x = tile->ghost_x; c.x0 = tile->x0; c.nxl = tile->nxl; c.nx_global = tile->nx_global;
    c.tiles_px = tile->px; c.tiles_py = tile->py; c.tile_rx = tile->rx; c.tile_ry = tile->ry;
  }
  c.self_periodic = self_periodic;
  c.fast_avvels = (flags & LBM_FLAG_FAST_AVVELS) != 0;
  c.fused = (flags & LBM_FLAG_FUSED_ARITH) != 0;
  c.multi_terms = c.fast_avvels ? kTermsFloat : (flags & LBM_FLAG_EXACT_AVVELS) ? kTermsDouble : kTermsCompensated;
  {
    const int t = knobs.terms;                                // 0 double, 1 float, 2 compensated (A/B runs of the DEFAULT form:
    if (t >= 0 && t <= 2 && !(flags & (LBM_FLAG_EXACT_AVVELS | LBM_FLAG_FAST_AVVELS))) c.multi_terms = t;   // a form asked for by flag stays)
  }
  c.accel_row = accel_row;
  c.accel_w1 = p->density * p->accel * 0.111111111111111111111111f;        // d2q9-bgk.c:445
  c.accel_w2 = p->density * p->accel * 0.0277777777777777777777778f;       // d2q9-bgk.c:446
  c.ncells = static_cast<long long>(p->nx) * ny_local;
  const size_t ncells = static_cast<size_t>(c.ncells);
  // K-step mode of a row-partitioned run: K ghost rows on each side of the owned rows, refreshed by the
  // neighbours every K steps, all steps done by lbm_multi_kernel (lbm_macro_* calls)
  c.group_max = 1;
  if (forced_k > 0) {
    if (self_periodic || !has_window || forced_k > kMaxMultiSteps || forced_ghost < forced_k || forced_ghost > kMaxGhost ||
        !macro_eligible(p, ny_local, flags)) {
      set_error("lbm_create_rank: partition cannot run the K-step mode its layout asks for");
      return lbm_internal::kPlanRefusedLate;
    }
    c.multi_K = forced_k; c.ghost = forced_ghost;
    c.ghost_rows = (tile && !tile->ghost_rows) ? 0 : forced_ghost;
    c.group_max = macro_group_for(knobs, forced_k, forced_ghost);
  } else if (forced_k < 0 && !self_periodic && has_global_map && macro_eligible(p, ny_local, flags)) {
    const int k = macro_k_for(knobs);
    if (k > 0) { c.multi_K = k; c.ghost = c.ghost_rows = macro_ghost_for(knobs, k, p->nx, ny_local, ny_local); c.group_max = macro_group_for(knobs, k, c.ghost); }
  }
  c.multi_tail4 = knobs.multi_tail4 != 0;
  c.ncells_storage = static_cast<long long>(p->nx) * (ny_local + 2 * c.ghost_rows);
  c.ps = static_cast<long long>(lbm_internal::plane_stride_floats(static_cast<size_t>(c.ncells_storage), knobs.skew));
  c.grid_floats = 9 * c.ps + 128;
  // non-temporal output stores once the two grids no longer fit the 256 MiB Infinity Cache
  const size_t state_bytes = 2 * 9 * ncells * sizeof(float);
  c.nt_stores = state_bytes > (192u << 20);
  if (flags & LBM_FLAG_NT_STORES) c.nt_stores = 1;
  if (flags & LBM_FLAG_NO_NT_STORES) c.nt_stores = 0;
  // narrow form for latency-bound grids (measured cross-over) and for nx % 4 != 0
  // (128x128: 3.5 vs 4.4 us/step, 256x256: 4.1 vs 4.6, 512x512: 7.3 vs 6.2 -> cross-over at 64 K cells)
  const size_t narrow_max = static_cast<size_t>(knobs.narrow_max);
  c.lane_cells = (p->nx % kCellsPerLane != 0 || ncells <= narrow_max) ? 1 : kCellsPerLane;
  if (flags & LBM_FLAG_KERNEL_LDS) {
    set_error("lbm_create: LBM_FLAG_KERNEL_LDS is retired (the LDS-staged one-step kernel was never faster and is no longer built)");
    return lbm_internal::kPlanRefusedLate;
  }
  // hipGraph replay of 64-step blocks is opt-in: measured on MI355X it changes nothing (128x128:
  // 4.47 vs 4.33 us/step) because even the smallest grids are bound by the device-side kernel
  // boundary + kernel latency, not by the host's launch rate
  c.use_graph = self_periodic && (flags & LBM_FLAG_GRAPH);
  // obstacle bitfield of the storage rows; halo buffers: 2 send + 2 recv, each [3][nxp]
  c.mask_words = static_cast<int>((static_cast<size_t>(c.ncells_storage) + 31) / 32 + 4);
  c.nxp = p->nx + 2 * kHaloGuard;
  // launch geometry + partial buffers
  const long long qrow = p->nx / c.lane_cells;
  const long long qfull = qrow * ny_local;
  c.iters_full = lbm_internal::pick_iters(qfull, knobs.maxblocks);
  c.n_part_full = lbm_internal::blocks_for(qfull, c.iters_full);
  const long long qint = ny_local > 2 ? qrow * (ny_local - 2) : 0;
  c.iters_interior = lbm_internal::pick_iters(qint > 0 ? qint : 1, knobs.maxblocks);
  c.n_part_interior = qint > 0 ? lbm_internal::blocks_for(qint, c.iters_interior) : 0;
  c.n_part_boundary = lbm_internal::blocks_for(ny_local > 1 ? 2 * qrow : qrow, 1);
  c.partials_cap = std::max(c.n_part_full, c.n_part_interior + c.n_part_boundary) + 1;
  // temporally blocked form: whole periodic grids whose edges are multiples of the tile edge and
  // that are small enough to be launch-latency-bound (measured cross-over)
  {
    // geometry by size, measured on MI355X (us/step for <8,4> / <8,8> / <16,4> / <16,8>; one-step kernels
    // 3.4 / 3.5 / 4.0):  128x128 1.7 / 1.4 / 1.8 / 1.6 | 128x256 2.2 / 1.8 / 1.9 / 1.7 | 256x256 3.4 / 3.0 / 2.2 / 1.9
    const int by_size = ncells <= 16384 ? 88 : 168;
    const int geom = knob_or(knobs.tile_geom, by_size);   // T*10 + H
    c.tile_T = geom / 10; c.tile_H = geom % 10;
    if (!((c.tile_T == 16 || c.tile_T == 8) && (c.tile_H == 8 || c.tile_H == 4))) { c.tile_T = 16; c.tile_H = 4; }
  }
  // measured whole-deck times (s) for 0 / 256 / 512: 128x128 0.0648 / 0.0576 / 0.0565, 128x256 0.0746 / 0.0747 / 0.0712,
  // 256x256 0.1598 / 0.1570 / 0.1532
  c.tile_single_max = knobs.tile_single_max;
  c.n_tiles = (p->nx % c.tile_T == 0 && ny_local % c.tile_T == 0) ? (p->nx / c.tile_T) * (ny_local / c.tile_T) : 0;
  c.tile_kernel = self_periodic && c.n_tiles > 0 &&
                  ncells <= static_cast<size_t>(knobs.tile_max);  // us/step here vs lbm_multi_kernel<3>: 256x256 1.9 / 3.1, 512x256 2.8 / 3.2, 384x384 3.6 / 3.2, 512x512 4.5 / 3.3
  c.multi_geom = kGeomStd; c.multi_tx = kMTX;
  if (c.ghost > 0) {
    // the packed messages of a K-step partition: one row message is 9 planes of its ghost rows (a column block — a tile rank that owns
    // every row, ghost_rows == 0 — has no row exchange: 0 floats, its buffers hold one row); a tile rank's column message 9 planes of
    // ghost_x columns of its owned rows.  Each buffer holds both directions.
    c.pack_floats = c.ghost_rows > 0 ? 9LL * c.ghost * p->nx : 0;
    c.pack_alloc_floats = 2LL * 9 * std::max(c.ghost_rows, 1) * p->nx;
    c.pack_floats_x = c.ghost_x > 0 ? 9LL * ny_local * c.ghost_x : 0;
    c.tile_kernel = 0;
    plan_multi(knobs, tile != nullptr, c);
  } else if (!c.tile_kernel && self_periodic && whole_grid_tiled(p->nx, ny_local)) {
    // K steps per pass over HBM (lbm_multi_kernel), measured us/step for K = 2 / 3 / 4 (one-step kernel):
    //   8192x8192 500 / 360 / 405 (853-917)   2048x2048 33.5 / 25.5 / 27.4 (59)
    //   1024x1024 11.2 / 8.3 / 8.5 (13.5)   512x512 3.7 / 3.4 / 3.3 (6.3; lbm_tile_kernel 5.2)
    // K = 2 is HBM-bound, K = 4 instruction-bound at 2 blocks per CU (60 KB frames); K = 3 sits at both limits
    // round 3, 4-step launch on 64 x 13 tiles: K = 3 / K = 4 8192x8192 346.6 / 324.0, 4096x4096 87.2 / 78.4, 2048x2048 24.0 / 21.6,
    // 1536x1536 14.2 / 13.8, 1024x1024 8.16 / 7.07, 768x768 5.39 / 4.63, 1024x512 4.51 / 4.72, 512x1024 4.39 / 4.62, 640x640 4.01 / 4.13,
    // 512x512 3.11 / 3.45 -> K = 4 from 768 x 768 cells up (profiles/r03/ab_k3_k4.txt, ab_k3_k4_threshold.txt)
    // K = 5 (five_steps_eligible: whole grids on the tall geometry; population 0 out of the LDS frame keeps two blocks per CU): the default from
    // LBM_TUNE_MULTI5_MIN cells up, the measurements behind that number in DESIGN.md section 4.2 (profiles/r15); LBM_TUNE_MULTI_K=5 asks for it at any
    // eligible size and falls back to 4 elsewhere.
    c.multi_geom = pick_geom(knobs, ncells);                  // (plan_multi's choice for a whole grid)
    const bool five_ok = five_steps_eligible(c, flags);
    const int by_size = (five_ok && knobs.multi5_min > 0 && ncells >= static_cast<size_t>(knobs.multi5_min)) ? kMaxWholeGridSteps : ncells >= size_t(768) * 768 ? 4 : 3;
    c.multi_K = std::min(std::max(knob_or(knobs.multi_k, by_size), 0), five_ok ? kMaxWholeGridSteps : kMaxMultiSteps);
    plan_multi(knobs, false, c);
  } else if (c.tile_kernel) {
    c.partials_cap = std::max(c.partials_cap, kMaxTileSteps * c.n_tiles + 1);
  }
  *out = c;
  return lbm_internal::kPlanOk;
}

}  // namespace

namespace lbm_internal {

int plan_whole(const Knobs& knobs, const lbm_params* p, int free_cells, int y0, int ny_local, unsigned flags, bool has_global_map, ContextPlan* out)
{
  return plan_context(knobs, p, free_cells, has_global_map, false, has_global_map ? -1 : 0, 0, y0, ny_local, flags, nullptr, out);
}

int plan_rank(const Knobs& knobs, const lbm_params* p, int free_cells, int nranks, int rank, unsigned flags, ContextPlan* out)
{
  lbm_layout lay;
  if (rank_layout(knobs, p, nranks, rank, flags, &lay)) return kPlanRefused;
  return plan_context(knobs, p, free_cells, false, true, lay.macro_k, lay.ghost, lay.y0, lay.ny_local, flags, nullptr, out);
}

int plan_tile(const Knobs& knobs, const lbm_params* p, int free_cells, int px, int py, int rank, unsigned flags, ContextPlan* out)
{
  lbm_tile_layout lay;
  if (tile_layout_of(knobs, p, px, py, rank, flags, &lay)) return kPlanRefused;
  lbm_params local = *p;
  local.nx = lay.nx_local + 2 * lay.ghost_x;                                           // the storage row: what every kernel works on
  const TileSpec tile{px, py, lay.rx, lay.ry, lay.x0, lay.nx_local, lay.ghost_x, p->nx, lay.ghost_y};
  return plan_context(knobs, &local, free_cells, false, true, lay.macro_k, lay.ghost, lay.y0, lay.ny_local, flags | LBM_FLAG_FORCE_HALO, &tile, out);
}

// Which kernel family advances a context: lbm_multi_kernel (whole grids it tiles and every K-step partition), lbm_tile_kernel (small whole
// grids), or the one-step kernels (everything else).  lbm_run launches by it and lbm_describe names it.
KernelFamily family_of(const ContextPlan& c)
{
  if (c.multi_K > 0 && (c.self_periodic || c.ghost > 0)) return kFamilyMulti;
  return (c.tile_kernel && c.self_periodic) ? kFamilyTile : kFamilyStep;
}

// The library's names for the families (a profiler prints the instantiations: lbm_multi_kernel<K, 6, GEOM, PART> with 6 = kTermsCompensated + kTermsFused,
// lbm_tile_kernel<T, H, FULL, TERMS>, lbm_step_kernel<CELLS, NT, FUSED>)
void plan_kernel_name(const ContextPlan& c, char* kernel_name, size_t len)
{
  const KernelFamily family = family_of(c);
  const char* nt = c.nt_stores ? "true" : "false";
  if (c.fused) {                 // LBM_FLAG_FUSED_ARITH
    if (family == kFamilyMulti) std::snprintf(kernel_name, len, "lbm_multi_kernel<%d, 6> (fused arithmetic)", c.multi_K);
    else if (family == kFamilyTile) std::snprintf(kernel_name, len, "lbm_tile_kernel_fused<%d, %d>", c.tile_T, c.tile_H);
    else std::snprintf(kernel_name, len, c.lane_cells == 1 ? "lbm_step_kernel_narrow_fused<%s>" : "lbm_step_kernel_fused<%s>", nt);
  }
  else if (family == kFamilyMulti) std::snprintf(kernel_name, len, c.multi_terms == kTermsFloat ? "lbm_multi_kernel<%d, fast av_vels>" : c.multi_terms == kTermsDouble ? "lbm_multi_kernel<%d, double-precision av_vels terms>" : "lbm_multi_kernel<%d>", c.multi_K);
  else if (family == kFamilyTile) std::snprintf(kernel_name, len, c.fast_avvels ? "lbm_tile_kernel<%d, %d, fast av_vels>" : "lbm_tile_kernel<%d, %d>", c.tile_T, c.tile_H);
  else std::snprintf(kernel_name, len, c.lane_cells == 1 ? "lbm_step_kernel_narrow<%s>" : "lbm_step_kernel<%s>", nt);
}

// ---- the double-precision mode --------------------------------------------------------------------------------------------------

// What lbm64_create decides.  The one-step launch (every context has it: set_cells, the fallbacks) by the float path's rules in
// elements; then, with LBM64_FLAG_TILE_STEPS, whether lbm_tile_kernel_f64 advances the grid and in which geometry.
void plan64_whole(const Knobs& knobs, const lbm64_params* p, unsigned flags, Plan64* out)
{
  Plan64 c{};
  c.flags = flags;
  const size_t ncells = static_cast<size_t>(p->nx) * p->ny;
  c.ps = static_cast<long long>(plane_stride_floats(ncells, knobs.skew));   // always even (the pair form's aligned 16-byte accesses)
  c.grid_doubles = 9 * c.ps + 128;
  // non-temporal output stores once the two grids no longer fit the 256 MiB Infinity Cache (the float path's rule and flags)
  const size_t state_bytes = 2 * 9 * ncells * sizeof(double);
  c.nt_stores = state_bytes > (192u << 20);
  if (flags & LBM_FLAG_NT_STORES) c.nt_stores = 1;
  if (flags & LBM_FLAG_NO_NT_STORES) c.nt_stores = 0;
  c.lane_cells = (p->nx % kPairCells == 0) ? kPairCells : 1;
  c.units = static_cast<unsigned>(ncells / c.lane_cells);
  c.iters = pick_iters(c.units, std::max(knobs.maxblocks, 1));
  c.blocks = static_cast<int>((static_cast<long long>(c.units) + static_cast<long long>(kBlock) * c.iters - 1) / (static_cast<long long>(kBlock) * c.iters));
  // geometry by size (T * 10 + H): the fastest measured per deck (profiles/r08/f64_tile.txt), s per whole deck for the one-step
  // kernel | <8,4> / <8,8> / <16,4> / <16,8>:  128x128 0.1429 | 0.0599 / 0.0621 / 0.0671 / 0.0660   128x256 0.1522 | 0.0837 / 0.0959 /
  // 0.0771 / 0.0714   256x256 0.3344 | 0.2403 / 0.3476 / 0.1970 / 0.1751   512x512 (10 000 steps) 0.0982 | 0.0628 / 0.1460 / 0.0678 /
  // 0.0666   1024x1024 0.4669 | 0.4129 / 1.1176 / 0.4572 / 0.4845.  Between two measured sizes the smaller one's geometry holds.
  const int by_size = ncells < 32768 ? 84 : ncells < 262144 ? 168 : 84;
  int geom = knob_or(knobs.tile64_geom, by_size);
  if (geom < 0 || !tile64_geom_ok(geom / 10, geom % 10)) geom = by_size;      // a malformed value: the default
  c.tile_T = geom / 10; c.tile_H = geom % 10;
  c.tile_block = tile64_block(c.tile_T, c.tile_H);
  c.tile_lds_bytes = tile64_lds_bytes(c.tile_T, c.tile_H);
  const bool tiles = p->nx % c.tile_T == 0 && p->ny % c.tile_T == 0;
  c.tiles_x = tiles ? p->nx / c.tile_T : 0;
  c.n_tiles = tiles ? c.tiles_x * (p->ny / c.tile_T) : 0;
  // the size cap (LBM_TUNE_TILE64_MAX): the largest measured grid at which the tiled launches beat the one-step ones by more than both
  // max - min spreads together: 1024 x 1024 (0.4129 against 0.4669 s, spreads 0.0022 s), the largest grid measured
  c.tile_kernel = (flags & LBM64_FLAG_TILE_STEPS) != 0u && tiles && static_cast<long long>(ncells) <= static_cast<long long>(knobs.tile64_max);
  c.partials_cap = std::max(c.blocks, c.tile_kernel ? c.tile_H * c.n_tiles : 0) + 1;   // a context that never launches the tiled kernel keeps no room for it
  *out = c;
}

void plan64_kernel_name(const Plan64& c, char* kernel_name, size_t len)
{
  if (c.tile_kernel) std::snprintf(kernel_name, len, "lbm_tile_kernel_f64<%d, %d>", c.tile_T, c.tile_H);
  else std::snprintf(kernel_name, len, c.nt_stores ? "lbm_step_kernel_f64<%d,nt>" : "lbm_step_kernel_f64<%d>", c.lane_cells);
}

// A run of n steps is launches of tile_H steps and one shorter tail: a function of what is left of THIS run only.
int plan64_next_steps(const Plan64& c, int left)
{
  return c.tile_kernel ? std::min(c.tile_H, left) : std::min(1, left);
}

// LBM64_FLAG_MULTI_STEPS: lbm_multi_kernel_f64 where the tiled kernel does not claim the context, the tiles cover the grid exactly and
// the grid has at least LBM_TUNE_MULTI64_MIN cells.  Both knobs' defaults are measured (profiles/r11/f64_multi.txt), us per step for the
// one-step kernel | K = 2 / 3 / 4:  8192x8192 1715.9 | 1039.8 / 706.3 / 624.3   4096x4096 448.4 | 253.0 / 178.3 / 157.7   2048x2048 106.9 |
// 67.5 / 46.4 / 41.3   1024x1024 23.46 | 18.40 / 13.70 / 11.99 (the tiled kernel there: 20.67).  K is the fastest at 8192 x 8192; the
// minimum is the smallest measured size that beats the one-step kernel by more than both max - min spreads together (11.46 us against
// 0.05 us), which is the smallest size measured.
constexpr int kMulti64DefaultK = 4, kMulti64DefaultMin = 1 << 20;         // cells of a whole grid (a row partition has a default of its own: plan64_rows_multi)
void plan64_multi(const Knobs& knobs, const lbm64_params* p, const Plan64& plan, PlanMulti64* out)
{
  PlanMulti64 m{};
  m.K = multi64_k_ok(knobs.multi64_k) ? knobs.multi64_k : kMulti64DefaultK;     // a malformed or unbuilt value: the default
  m.TX = kMulti64TX; m.TY = kMulti64TY;
  m.block = kMulti64Lanes;
  m.lds_bytes = multi64_lds_bytes(m.K);
  m.nt_stores = plan.nt_stores;
  const bool tiles = p->nx % m.TX == 0 && p->ny % m.TY == 0;
  m.tiles_x = tiles ? p->nx / m.TX : 0;
  m.n_tiles = tiles ? m.tiles_x * (p->ny / m.TY) : 0;
  m.multi_kernel = (plan.flags & (LBM64_FLAG_MULTI_STEPS | LBM64_FLAG_MULTI_ANY_SIZE)) != 0u && !plan.tile_kernel && tiles &&   // the latter means the former
                   static_cast<long long>(p->nx) * p->ny >= static_cast<long long>(knob_or(knobs.multi64_min, kMulti64DefaultMin));
  m.partials_cap = m.K * m.n_tiles + 1;
  *out = m;
}

void plan64_multi_kernel_name(const PlanMulti64& m, char* kernel_name, size_t len)
{
  if (!m.multi_kernel) { kernel_name[0] = '\0'; return; }
  std::snprintf(kernel_name, len, m.nt_stores ? "lbm_multi_kernel_f64<%d,nt>" : "lbm_multi_kernel_f64<%d>", m.K);
}

// A run of n steps is floor(n / K) launches of K steps and at most one shorter launch, the last: a function of what is left of THIS run only.
int plan64_multi_next_steps(const PlanMulti64& m, int left)
{
  return std::min(m.K, left);
}

// The multi-step launches of a context: plan64_multi's answer where the tiles cover the grid, and with LBM64_FLAG_MULTI_ANY_SIZE the
// edge-tile form on a grid they do not cover — nx even (aligned x-pairs) and >= TX, ny >= TY (a shifted tile lies inside the grid, and
// the wrap of sub-step 1 needs one correction per axis), at least LBM_TUNE_MULTI64_MIN cells (plan64_multi's knob and default), not
// claimed by the tiled kernel.  ceil(nx / TX) x ceil(ny / TY) tiles; the last column and row start at nx - TX and ny - TY.
// Measured (profiles/r20/f64_multi_any.txt), us per step for the one-step kernel | the edge form at K = 4:  8190x8190 1858.5 | 699.5
// 4098x4100 458.6 | 182.6   2050x2046 106.8 | 46.6   1022x1026 24.93 | 12.92.  The edge form beats the one-step kernel by more than both
// max - min spreads together at every size (at the smallest: 12.01 us against 0.42 us), so it has no minimum of its own.  8192x8192
// under this flag: 642.4, under LBM64_FLAG_MULTI_STEPS 641.4 (the same kernel); a tile-step of 8190x8190 costs 9 % more than one of it.
void plan64_multi_any(const Knobs& knobs, const lbm64_params* p, const Plan64& plan, PlanMultiAny64* out)
{
  PlanMulti64 m{};
  plan64_multi(knobs, p, plan, &m);
  PlanMultiAny64 a{};
  a.K = m.K; a.TX = m.TX; a.TY = m.TY;
  a.block = m.block; a.lds_bytes = m.lds_bytes;
  a.nt_stores = m.nt_stores;
  const bool exact = m.n_tiles > 0;
  const bool shape = exact || (p->nx % kPairCells == 0 && p->nx >= a.TX && p->ny >= a.TY);
  a.tiles_x = shape ? (p->nx + a.TX - 1) / a.TX : 0;
  a.tiles_y = shape ? (p->ny + a.TY - 1) / a.TY : 0;
  a.n_tiles = a.tiles_x * a.tiles_y;
  a.last_x0 = shape ? p->nx - a.TX : 0;
  a.last_y0 = shape ? p->ny - a.TY : 0;
  a.edge = (plan.flags & LBM64_FLAG_MULTI_ANY_SIZE) != 0u && !plan.tile_kernel && shape && !exact &&
           static_cast<long long>(p->nx) * p->ny >= static_cast<long long>(knob_or(knobs.multi64_min, kMulti64DefaultMin));
  a.multi_kernel = m.multi_kernel || a.edge;
  a.partials_cap = a.K * a.n_tiles + 1;
  *out = a;
}

void plan64_multi_any_kernel_name(const PlanMultiAny64& a, char* kernel_name, size_t len)
{
  if (!a.multi_kernel) { kernel_name[0] = '\0'; return; }
  const char* form = a.edge ? (a.nt_stores ? "lbm_multi_kernel_f64<%d,nt,edge>" : "lbm_multi_kernel_f64<%d,edge>")
                            : (a.nt_stores ? "lbm_multi_kernel_f64<%d,nt>" : "lbm_multi_kernel_f64<%d>");
  std::snprintf(kernel_name, len, form, a.K);
}

// plan64_multi_next_steps' rule: floor(n / K) launches of K steps and at most one shorter launch, the last.
int plan64_multi_any_next_steps(const PlanMultiAny64& a, int left)
{
  return std::min(a.K, left);
}

// One rank of a row-partitioned double-precision run (lbm_rows64_create).  Rows by the reference's rule; the launch over the rank's
// ny_local * nx owned cells by plan64_whole's rules (the same lane form, chunking and store rule, the latter on the RANK's two grids,
// ghost rows included); grids of ny_local + 2 storage rows.  Row ny-2, which accelerate_flow works on, lies in the last rank (the rule
// gives it at least 3 rows or the run is refused), and is neither that rank's first nor its last row: no edge row is ever accelerated
// after it was sent.
int plan64_rows(const Knobs& knobs, const lbm64_params* p, int nranks, int rank, unsigned flags, PlanRows64* out)
{
  if (!p || !out) { set_error("lbm_rows64: null argument"); return 1; }
  if (p->nx < 1) { set_error("lbm_rows64: nx must be positive"); return 1; }
  if (p->ny < 3) { set_error("lbm_rows64: ny must be >= 3 (accelerate_flow works on row ny-2, d2q9-bgk.c:449)"); return 1; }
  if (static_cast<long long>(p->nx) * p->ny > (1LL << 31) - 4096) { set_error("lbm_rows64: grid too large for 32-bit cell indices"); return 1; }
  if ((flags & (LBM64_FLAG_TILE_STEPS | LBM64_FLAG_MULTI_STEPS)) != 0u) {
    set_error("lbm_rows64: LBM64_FLAG_TILE_STEPS and LBM64_FLAG_MULTI_STEPS are refused: they are the whole grid's, for whose kernels several steps per exchange are not built (a row partition takes LBM_ROWS64_FLAG_MULTI_STEPS, alone or with a store form)");
    return 1;
  }
  if ((flags & ~kFlagsRows64) != 0u) { set_error("lbm_rows64: a row partition takes LBM_FLAG_NT_STORES or LBM_FLAG_NO_NT_STORES only"); return 1; }
  if (nranks < 1 || nranks > kMaxRows64Ranks) { set_error("lbm_rows64: nranks must be 1..64 (MPI_PROCS, d2q9-bgk.c:67)"); return 1; }
  if (rank < 0 || rank >= nranks) { set_error("lbm_rows64: rank outside 0..nranks-1"); return 1; }
  int nyl[kMaxRows64Ranks], dis[kMaxRows64Ranks];
  if (lbm_decompose(p->ny, nranks, nyl, dis)) return 1;                                  // d2q9-bgk.c:834-862
  for (int r = 0; r < nranks; ++r)
    if (nyl[r] < 1) { set_error("lbm_rows64: ny = " + std::to_string(p->ny) + " on " + std::to_string(nranks) + " ranks leaves rank " + std::to_string(r) + " without a row"); return 1; }
  if (nyl[nranks - 1] < 3) {                                                               // :848-849
    set_error("lbm_rows64: ny = " + std::to_string(p->ny) + " on " + std::to_string(nranks) + " ranks leaves the last rank fewer than 3 rows (d2q9-bgk.c:848-849)");
    return 1;
  }
  PlanRows64 c{};
  c.flags = flags;
  c.nranks = nranks; c.rank = rank;
  c.y0 = dis[rank]; c.ny_local = nyl[rank];
  const size_t owned = static_cast<size_t>(p->nx) * c.ny_local, storage = static_cast<size_t>(p->nx) * (c.ny_local + 2);
  c.ps = static_cast<long long>(plane_stride_floats(storage, knobs.skew));     // always even (the pair form's aligned 16-byte accesses)
  c.grid_doubles = 9 * c.ps + 128;
  c.nt_stores = 2 * 9 * storage * sizeof(double) > (192u << 20);                // plan64_whole's rule
  if (flags & LBM_FLAG_NT_STORES) c.nt_stores = 1;
  if (flags & LBM_FLAG_NO_NT_STORES) c.nt_stores = 0;
  c.lane_cells = (p->nx % kPairCells == 0) ? kPairCells : 1;
  c.units = static_cast<unsigned>(owned / c.lane_cells);
  c.iters = pick_iters(c.units, std::max(knobs.maxblocks, 1));
  c.blocks = blocks_for(c.units, c.iters);
  c.partials_cap = c.blocks + 1;
  c.mask_words = static_cast<int>((owned + 31) / 32 + 4);
  c.accel_rank = nranks - 1;
  c.accel_row = p->ny - 2 - dis[nranks - 1];
  *out = c;
  return 0;
}

void plan64_rows_kernel_name(const PlanRows64& c, char* kernel_name, size_t len)
{
  std::snprintf(kernel_name, len, c.nt_stores ? "lbm_rows_kernel_f64<%d,nt>" : "lbm_rows_kernel_f64<%d>", c.lane_cells);
}

// LBM_ROWS64_FLAG_MULTI_STEPS: lbm_rows_multi_kernel_f64 on every rank, or on none.  The shape rule is plan64_multi's on each rank's
// owned rows (nx % TX == 0, every ny_local % TY == 0: under lbm_decompose, ny % (TY * nranks) == 0, so uneven ranks fall back), K and
// the minimum size are plan64_multi's knobs, the minimum taken on the SMALLEST rank's owned cells.  Its default for ranks is measured
// (profiles/r18/f64_rows_multi.txt, all ranks on one MI355X), by plan64_multi's rule: the smallest measured rank size at which the
// flagged run beats the unflagged one by more than both max - min spreads together, us per step unflagged | flagged:
//   8192x8192 on 8 ranks (2^23 cells a rank) 1697.0 | 682.2   4096x4096 on 8 (2^21) 449.9 | 182.3   2048x2048 on 8 (2^19) 146.5 | 46.3
//   1024x1024 on 2 (2^19) 37.86 | 15.21   1024x1024 on 8 (2^17) 96.90 | 31.14, a gain of 65.76 us against spreads of 3.88 us
// which is the smallest rank size measured: 2^17 cells a rank.  (A rank's launch adds 2 K rows of ring work and a push of 72 nx
// doubles to a whole grid's, but it also saves K - 1 of every K exchanges, which weigh most on small ranks.)  Storage: K ghost rows on each side, K of a FULL launch, so that
// a launch of k <= K steps finds the k rows it consumes; the tile rows are ny_local / TY >= 1, so ny_local >= 16 > 2 K: the rows a rank
// pushes (its first and last K owned ones) and the ghost rows it receives are disjoint even where it is its own neighbour.
static_assert(LBM_ROWS64_FLAG_MULTI_STEPS == kFlagRows64MultiSteps, "lbm_internal.h restates the header's flag");
static_assert(kMulti64TY > 2 * kMulti64MaxK, "a rank's pushed rows and ghost rows are disjoint");
constexpr int kRowsMulti64DefaultMin = 1 << 17;                           // cells of the smallest rank
void plan64_rows_multi(const Knobs& knobs, const lbm64_params* p, const PlanRows64& rows, PlanRowsMulti64* out)
{
  PlanRowsMulti64 m{};
  constexpr int kDefaultK = 4, kDefaultMin = kRowsMulti64DefaultMin;
  m.K = multi64_k_ok(knobs.multi64_k) ? knobs.multi64_k : kDefaultK;     // a malformed or unbuilt value: the default
  m.ghost = m.K;
  m.block = kMulti64Lanes;
  m.lds_bytes = multi64_lds_bytes(m.K);
  int nyl[kMaxRows64Ranks], dis[kMaxRows64Ranks];
  (void)lbm_decompose(p->ny, rows.nranks, nyl, dis);                       // plan64_rows made `rows` of it
  bool tiles = p->nx % kMulti64TX == 0;
  int smallest = nyl[0];
  for (int r = 0; r < rows.nranks; ++r) {
    tiles = tiles && nyl[r] % kMulti64TY == 0;
    smallest = std::min(smallest, nyl[r]);
  }
  m.tiles_x = tiles ? p->nx / kMulti64TX : 0;
  m.n_tiles = tiles ? m.tiles_x * (rows.ny_local / kMulti64TY) : 0;
  m.multi_kernel = (rows.flags & (kFlagRows64MultiSteps | kFlagRows64MultiAnySize)) != 0u && tiles &&   // the latter means the former
                   static_cast<long long>(p->nx) * smallest >= static_cast<long long>(knob_or(knobs.multi64_min, kDefaultMin));
  const size_t storage = static_cast<size_t>(p->nx) * (rows.ny_local + 2 * m.ghost);
  m.ps = static_cast<long long>(plane_stride_floats(storage, knobs.skew));   // always even
  m.grid_doubles = 9 * m.ps + 128;
  m.nt_stores = 2 * 9 * storage * sizeof(double) > (192u << 20);             // plan64_whole's rule
  if (rows.flags & LBM_FLAG_NT_STORES) m.nt_stores = 1;
  if (rows.flags & LBM_FLAG_NO_NT_STORES) m.nt_stores = 0;
  m.mask_words = static_cast<int>((storage + 31) / 32 + 4);
  m.partials_cap = m.K * m.n_tiles + 1;
  *out = m;
}

void plan64_rows_multi_kernel_name(const PlanRowsMulti64& m, char* kernel_name, size_t len)
{
  if (!m.multi_kernel) { kernel_name[0] = '\0'; return; }
  std::snprintf(kernel_name, len, m.nt_stores ? "lbm_rows_multi_kernel_f64<%d,nt>" : "lbm_rows_multi_kernel_f64<%d>", m.K);
}

// As plan64_multi_next_steps: floor(n / K) launches of K steps and at most one shorter launch, the last.
int plan64_rows_multi_next_steps(const PlanRowsMulti64& m, int left)
{
  return std::min(m.K, left);
}

// The multi-step launches of a rank: plan64_rows_multi's answer where the tiles cover every rank, and with
// LBM_ROWS64_FLAG_MULTI_ANY_SIZE the edge-tile form on a run they do not cover — nx even (aligned x-pairs) and >= TX, EVERY rank of at
// least TY rows (a shifted tile lies inside the rank's owned rows; the pushed and the ghost rows stay disjoint: TY > 2 K), the smallest
// rank of at least LBM_TUNE_MULTI64_MIN cells (plan64_rows_multi's knob and default).  ceil(nx / TX) x ceil(ny_local / TY) tiles on
// this rank; its last tile column and row start at nx - TX and at the owned row ny_local - TY.  Storage, window bitfield, store rule
// and K are plan64_rows_multi's.
// Measured (profiles/r22/f64_rows_any.txt, all ranks on one MI355X), device us per step of the parent commit's run of the same shape
// (the one-step kernel there) | the edge form at K = 4, on 1 / 2 / 8 ranks:
//   8190x8190  2008.0 | 693.2   1716.9 | 720.2   1929.0 | 738.6      4098x4100  546.9 | 182.8   506.2 | 184.3   526.6 | 189.5
//   2050x2046  113.05 | 48.28   130.67 | 50.91   159.16 | 51.25      1022x1026  28.91 | 14.07   38.85 | 15.74   59.90 | 20.20
// The edge form wins by more than both max - min spreads together at every size and rank count; at the smallest rank measured,
// 1022x1026 on 8 ranks (130 816 cells a rank), by 39.70 us against spreads of 30.01 us (52.94 against 31.01 beside this tree's own
// unflagged run).  By plan64_rows_multi's rule the minimum is the smallest measured rank size that wins, which is the smallest size
// measured: the edge form gets no minimum of its own and shares the rows' default of 2^17 cells (which that one run, measured with
// the minimum lowered to 0, is 256 cells short of).  8192x8192, the control: under LBM_ROWS64_FLAG_MULTI_STEPS 642.2 / 678.8 / 685.1
// against the parent's 643.1 / 675.5 / 684.1 (the same kernel and instructions: within both spreads), under this flag 644.8 / 676.2 / 682.4.
static_assert(LBM_ROWS64_FLAG_MULTI_ANY_SIZE == kFlagRows64MultiAnySize, "lbm_internal.h restates the header's flag");
static_assert((kFlagRows64MultiAnySize & (LBM_FLAG_NT_STORES | LBM_FLAG_NO_NT_STORES | kFlagRows64MultiSteps | kFlags64)) == 0u, "a bit of its own");
void plan64_rows_multi_any(const Knobs& knobs, const lbm64_params* p, const PlanRows64& rows, PlanRowsMultiAny64* out)
{
  PlanRowsMulti64 m{};
  plan64_rows_multi(knobs, p, rows, &m);
  PlanRowsMultiAny64 a{};
  a.K = m.K; a.ghost = m.ghost;
  a.block = m.block; a.lds_bytes = m.lds_bytes;
  a.nt_stores = m.nt_stores;
  a.mask_words = m.mask_words;
  a.ps = m.ps; a.grid_doubles = m.grid_doubles;
  int nyl[kMaxRows64Ranks], dis[kMaxRows64Ranks];
  (void)lbm_decompose(p->ny, rows.nranks, nyl, dis);                       // plan64_rows made `rows` of it
  const int smallest = *std::min_element(nyl, nyl + rows.nranks);
  const bool exact = m.n_tiles > 0;
  const bool shape = exact || (p->nx % kPairCells == 0 && p->nx >= kMulti64TX && smallest >= kMulti64TY);
  a.tiles_x = shape ? (p->nx + kMulti64TX - 1) / kMulti64TX : 0;
  a.tiles_y = shape ? (rows.ny_local + kMulti64TY - 1) / kMulti64TY : 0;
  a.n_tiles = a.tiles_x * a.tiles_y;
  a.last_x0 = shape ? p->nx - kMulti64TX : 0;
  a.last_y0 = shape ? rows.ny_local - kMulti64TY : 0;
  a.edge = (rows.flags & kFlagRows64MultiAnySize) != 0u && shape && !exact &&
           static_cast<long long>(p->nx) * smallest >= static_cast<long long>(knob_or(knobs.multi64_min, kRowsMulti64DefaultMin));
  a.multi_kernel = m.multi_kernel || a.edge;
  a.partials_cap = a.K * a.n_tiles + 1;
  *out = a;
}

void plan64_rows_multi_any_kernel_name(const PlanRowsMultiAny64& a, char* kernel_name, size_t len)
{
  if (!a.multi_kernel) { kernel_name[0] = '\0'; return; }
  const char* form = a.edge ? (a.nt_stores ? "lbm_rows_multi_kernel_f64<%d,nt,edge>" : "lbm_rows_multi_kernel_f64<%d,edge>")
                            : (a.nt_stores ? "lbm_rows_multi_kernel_f64<%d,nt>" : "lbm_rows_multi_kernel_f64<%d>");
  std::snprintf(kernel_name, len, form, a.K);
}

// plan64_multi_next_steps' rule: floor(n / K) launches of K steps and at most one shorter launch, the last.
int plan64_rows_multi_any_next_steps(const PlanRowsMultiAny64& a, int left)
{
  return std::min(a.K, left);
}

// One rank of a column-partitioned double-precision run (lbm_cols64_create).  Columns by lbm_decompose_columns (whole x-pairs, the
// spare pairs to the first ranks); K is plan64_multi's knob and default; G = 2 ceil(K / 2) ghost columns on each side, so that a launch
// of k <= K steps finds the k columns it consumes and the pitch nxl + 2 G stays even.  A run is taken if and only if nx is even, every
// rank has at least TX columns and ny >= TY (a shifted tile lies inside the block; the wrap in y needs one correction): there is no
// one-step column kernel to fall back on and no size threshold, so everything else is refused, and the message names the row
// partition, which takes every shape.  nxl >= TX = 32 > 2 G: the columns a rank pushes (its first and last G owned ones) and the ghost
// columns it receives are disjoint even where it is its own neighbour.  The store rule is plan64_whole's on the RANK's two grids.
static_assert(kMulti64TX > 2 * 2 * ((kMulti64MaxK + 1) / 2), "a rank's pushed columns and ghost columns are disjoint");
static_assert(LBM_COLS64_MAX_RANKS == kMaxCols64Ranks, "lbm_internal.h restates the header's limit");
int plan64_cols(const Knobs& knobs, const lbm64_params* p, int nranks, int rank, unsigned flags, PlanCols64* out)
{
  static const char* const kRows = " (the row partition, lbm_rows64_create, takes every shape)";
  if (!p || !out) { set_error("lbm_cols64: null argument"); return 1; }
  if ((flags & ~kFlagsCols64) != 0u) { set_error("lbm_cols64: a column partition takes LBM_FLAG_NT_STORES or LBM_FLAG_NO_NT_STORES only"); return 1; }
  if (nranks < 1 || nranks > kMaxCols64Ranks) { set_error("lbm_cols64: nranks must be 1..64"); return 1; }
  if (rank < 0 || rank >= nranks) { set_error("lbm_cols64: rank outside 0..nranks-1"); return 1; }
  if (p->nx < 1 || p->nx % kPairCells != 0) { set_error(std::string("lbm_cols64: nx must be even: column blocks are made of whole x-pairs") + kRows); return 1; }
  if (p->ny < kMulti64TY) { set_error("lbm_cols64: ny = " + std::to_string(p->ny) + " is fewer than " + std::to_string(kMulti64TY) + " rows, the height of a tile" + kRows); return 1; }
  if (p->nx / kPairCells < nranks) { set_error("lbm_cols64: nx = " + std::to_string(p->nx) + " on " + std::to_string(nranks) + " ranks leaves a rank without an x-pair" + kRows); return 1; }
  int nxl[kMaxCols64Ranks], dis[kMaxCols64Ranks];
  if (lbm_decompose_columns(p->nx, nranks, nxl, dis)) return 1;
  for (int r = 0; r < nranks; ++r)
    if (nxl[r] < kMulti64TX) {
      set_error("lbm_cols64: nx = " + std::to_string(p->nx) + " on " + std::to_string(nranks) + " ranks leaves rank " + std::to_string(r) + " " + std::to_string(nxl[r]) +
                " columns, fewer than " + std::to_string(kMulti64TX) + ", the width of a tile" + kRows);
      return 1;
    }
  PlanCols64 c{};
  c.flags = flags;
  c.nranks = nranks; c.rank = rank;
  c.x0 = dis[rank]; c.nxl = nxl[rank];
  c.K = multi64_k_ok(knobs.multi64_k) ? knobs.multi64_k : kMulti64DefaultK;     // a malformed or unbuilt value: the default
  c.ghost = 2 * ((c.K + 1) / 2);
  c.pitch = c.nxl + 2 * c.ghost;
  for (int r = 0; r < nranks; ++r)
    if (static_cast<long long>(nxl[r] + 2 * c.ghost) * p->ny > (1LL << 31) - 4096) { set_error("lbm_cols64: a rank's storage is too large for 32-bit cell indices"); return 1; }
  c.tiles_x = (c.nxl + kMulti64TX - 1) / kMulti64TX;
  c.n_tiles = c.tiles_x * ((p->ny + kMulti64TY - 1) / kMulti64TY);
  c.edge = c.nxl % kMulti64TX != 0 || p->ny % kMulti64TY != 0;
  const size_t storage = static_cast<size_t>(c.pitch) * p->ny;
  c.nt_stores = 2 * 9 * storage * sizeof(double) > (192u << 20);                // plan64_whole's rule
  if (flags & LBM_FLAG_NT_STORES) c.nt_stores = 1;
  if (flags & LBM_FLAG_NO_NT_STORES) c.nt_stores = 0;
  c.block = kMulti64Lanes;
  c.lds_bytes = multi64_lds_bytes(c.K);
  c.mask_words = static_cast<int>((storage + 31) / 32 + 4);
  c.partials_cap = c.K * c.n_tiles + 1;
  c.ps = static_cast<long long>(plane_stride_floats(storage, knobs.skew));      // always even (the pair form's aligned 16-byte accesses)
  c.grid_doubles = 9 * c.ps + 128;
  *out = c;
  return 0;
}

void plan64_cols_kernel_name(const PlanCols64& c, char* kernel_name, size_t len)
{
  const char* form = c.edge ? (c.nt_stores ? "lbm_cols_multi_kernel_f64<%d,nt,edge>" : "lbm_cols_multi_kernel_f64<%d,edge>")
                            : (c.nt_stores ? "lbm_cols_multi_kernel_f64<%d,nt>" : "lbm_cols_multi_kernel_f64<%d>");
  std::snprintf(kernel_name, len, form, c.K);
}

// plan64_multi_next_steps' rule: floor(n / K) launches of K steps and at most one shorter launch, the last.
int plan64_cols_next_steps(const PlanCols64& c, int left)
{
  return std::min(c.K, left);
}

// ---- what a run launches ------------------------------------------------------------------------------------------------------

// Steps of the next launch of lbm_multi_kernel when `left` steps remain: multi_K, except that a count multi_K does not
// divide is split into 3s and 4s where that avoids a K = 2 / K = 1 launch at the end (8192 x 8192, us per launch: K = 1 870,
// K = 2 1000, K = 3 1050, K = 4 1290) — at K = 3: n = 3a + 4 or 3a + 8; at K = 4: n = 4a + 3, 4a + 6 or 4a + 9.  Whole periodic
// grids (the frame wraps) and row partitions that keep four ghost rows.  A function of (K, ghost, left) only, so every
// rank of a partitioned run makes the same sequence of macro-steps.
int next_multi_k(const ContextPlan& c, int left)
{
  return lbm_plan_next(c.multi_K, (c.self_periodic || c.ghost >= 4) ? 1 : 0, c.multi_tail4 ? 1 : 0, left);
}

static_assert(kGroupCap == kMaxGroup, "GroupPlan holds the longest group");
GroupPlan plan_group(const ContextPlan& c, int left)
{
  GroupPlan g;
  g.n = lbm_plan_group_for(c.multi_K, (c.self_periodic || c.ghost >= 4) ? 1 : 0, c.multi_tail4 ? 1 : 0, c.ghost,
                           std::min(c.group_max, static_cast<int>(kMaxGroup)), left, g.k, kMaxGroup);   // next_multi_k's launches
  for (int i = 0; i < g.n; ++i) g.total += g.k[i];
  return g;
}

// Tiles of a launch that makes `k` steps on the owned rows and `ext` more rows on each side (ext > 0: a launch of a partitioned
// run that is followed by `ext` more steps before the next halo exchange): the tile height depends on k (lbm_geometry.h multi_ty).
static int ext_rows(const ContextPlan& c, int ext) { return c.ghost_rows > 0 ? ext : 0; }   // ghost rows a launch advances (none where the rows wrap)
static int multi_tile_rows(const ContextPlan& c, int k, int ext) { return (c.nyl + 2 * ext_rows(c, ext) + multi_ty(k, c.multi_geom) - 1) / multi_ty(k, c.multi_geom); }
static int multi_tiles_for(const ContextPlan& c, int k, int ext) { return c.multi_tiles_x * multi_tile_rows(c, k, ext); }

// Tile rows of a launch of k steps that also advances `ext` ghost rows per side (tile row 0 starts at storage row ghost - ext): the
// first `bottom_edge_rows` and the last `top_edge_rows` tile rows read exchanged rows (edge launch, after the exchange); the
// `interior_rows` between them do not: the rows they need — their own, k below and k above — are owned rows.  (The last tile row
// may hold fewer rows than a launch makes steps: the ring of the row below then reaches the ghost rows, and the top edge is two rows.)
// (Tile ranks: the first `left_cols` and the last `right_cols` tile COLUMNS read exchanged columns as well — a tile's first sub-step reads
// multi_ex(k - 1) + 1 columns beyond its own on each side; the interior is then the rectangle inside all four.)
MacroRows macro_rows(const ContextPlan& c, int k, int ext)
{
  const int ty = multi_ty(k, c.multi_geom);
  const int ext_y = ext_rows(c, ext);
  const int first = c.ghost_rows - ext_y, rows = c.nyl + 2 * ext_y;
  const int nty = (rows + ty - 1) / ty;
  const int lo = c.ghost_rows, hi = c.ghost_rows + c.nyl;              // the owned rows [lo, hi)
  int b = 0, t = 0;
  if (c.ghost_rows > 0) {                                              // (a column block wraps in y: no tile row reads an exchanged row)
    while (b < nty && first + b * ty - k < lo) ++b;
    while (t < nty - b && std::min(first + (nty - t) * ty, first + rows) - 1 + k >= hi) ++t;
  }
  int l = 0, r = 0;
  if (c.ghost_x > 0) {
    const int tx = c.multi_tx, ntx = c.multi_tiles_x, reach = multi_ex(k - 1) + 1;
    const int xlo = c.ghost_x, xhi = c.ghost_x + c.nxl;                // the owned columns [xlo, xhi)
    while (l < ntx && l * tx - reach < xlo) ++l;
    while (r < ntx - l && (ntx - r) * tx - 1 + reach >= xhi) ++r;
    if (ntx - l - r <= 0) return {nty, 0, 0, 0, 0};               // no tile column inside the rim: everything waits for the exchange
  }
  return {b, nty - b - t, t, l, r};
}

// The tiles of a tile rank's launch of k steps + ext as rectangles: the interior (at most one), or the rim around it (at most four).
static int macro_rects(const ContextPlan& c, int k, int ext, bool interior, LaunchPlan::Rect* out)
{
  const MacroRows m = macro_rows(c, k, ext);
  const int ntx = c.multi_tiles_x, mid = m.interior_rows;
  int n = 0;
  auto add = [&](int ty0, int nrows, int tx0, int cols) { if (nrows > 0 && cols > 0) out[n++] = LaunchPlan::Rect{ty0, tx0, cols, nrows * cols}; };
  if (interior) {
    add(m.bottom_edge_rows, mid, m.left_cols, ntx - m.left_cols - m.right_cols);
  } else {
    add(0, m.bottom_edge_rows, 0, ntx);
    add(m.bottom_edge_rows + mid, m.top_edge_rows, 0, ntx);
    add(m.bottom_edge_rows, mid, 0, m.left_cols);
    add(m.bottom_edge_rows, mid, ntx - m.right_cols, m.right_cols);
  }
  return n;
}

// One launch of lbm_multi_kernel: `k` steps of the owned rows and `ext` ghost rows on each side (tile row 0 starts at storage row
// ghost - ext), over all its tiles (kLaunchWhole), over those that read no exchanged cell (kLaunchInterior) or over the rest (kLaunchEdge).
void plan_launch(const ContextPlan& c, const Knobs& knobs, int k, int ext, int which, bool says_ready, LaunchPlan* out)
{
  LaunchPlan a{};
  a.k = k; a.ext = ext;
  const int ext_y = ext_rows(c, ext);
  a.row_first = c.ghost_rows - ext_y; a.rows_compute = c.nyl + 2 * ext_y; a.rows_storage = c.nyl + 2 * c.ghost_rows;
  a.count_first = c.ghost_rows; a.count_end = c.ghost_rows + c.nyl;
  a.cx0 = c.ghost_x; a.cx1 = c.ghost_x + c.nxl;
  a.keep_x0 = std::max(0, (c.ghost_x - ext) & ~1); a.keep_x1 = std::min(c.nx, (c.ghost_x + c.nxl + ext + 1) & ~1);
  a.y_periodic = (c.self_periodic || (c.ghost > 0 && c.ghost_rows == 0)) ? 1 : 0;
  a.y0_global = c.y0 - ext_y;                                     // global row of storage row row_first
  a.tiles_x = c.multi_tiles_x;
  a.ntiles_total = multi_tiles_for(c, k, ext);
  if (which == kLaunchWhole) {
    a.tile_count = a.ntiles_total;
  } else if (c.ghost_x > 0) {                                     // tile rank: the rectangle inside the rim, or the rim (four rectangles at most)
    a.nrect = macro_rects(c, k, ext, which == kLaunchInterior, a.rect);
  } else {
    const MacroRows r = macro_rows(c, k, ext);
    if (which == kLaunchInterior) { a.tile_begin = r.bottom_edge_rows * a.tiles_x; a.tile_count = r.interior_rows * a.tiles_x; }
    else { a.tile_count = r.bottom_edge_rows * a.tiles_x; a.tile_begin2 = (r.bottom_edge_rows + r.interior_rows) * a.tiles_x; a.tile_count2 = r.top_edge_rows * a.tiles_x; }
  }
  int blocks = a.tile_count + a.tile_count2;
  for (int i = 0; i < a.nrect; ++i) blocks += a.rect[i].count;
  // measured on 8192x8192, K=2: 515 us/step with the XCD-contiguous tile order, 549 without
  a.xcd_remap = (knobs.multi_remap && blocks % 8 == 0 && blocks >= 64) ? 1 : 0;
  a.nblocks = blocks;
  if (c.ghost_x > 0 && knobs.multi_remap && blocks >= 64 && blocks % 8 != 0 && knobs.tile_pad_grid) {
    blocks = (blocks + 7) / 8 * 8;                                // tile ranks: pad the grid (the form drops the extra blocks) and keep the XCD-contiguous order
    a.xcd_remap = 1;
  }
  a.launched_blocks = blocks;
  // the instantiation that does exactly `k` steps: the tail of a run whose step count multi_K does not
  // divide is a launch of a smaller frame, not a run-time loop bound (which cost scratch and ~10 % speed)
  // the form (kernels/multi.h PART): ghost rows computed too -> the counted test; ready words to say -> the fold block carries them
  // (a rank of the tile decomposition: ghost columns in every launch)
  a.part = c.ghost_x > 0 ? kPartTile : ext > 0 ? kPartGhost : says_ready ? kPartReady : kPartPlain;
  const int steps = std::min(k, static_cast<int>(kMaxMultiSteps));       // k <= multi_K, or 4 in the tail of a K = 3 run (next_multi_k)
  a.row = multi_row(steps, c.multi_geom, c.fused ? kMultiTermsFused : c.multi_terms, a.part);
  a.lanes = multi_lanes(steps, c.multi_geom);
  if (k == kMaxWholeGridSteps && c.multi_K == kMaxWholeGridSteps) {      // the five-step launch of a whole grid (five_steps_eligible: tall, plain): its own rows
    a.row = multi_row5(c.fused ? kMultiTermsFused : c.multi_terms);
    a.lanes = multi_lanes(k, c.multi_geom);
  }
  *out = a;
}

// The next launch of lbm_tile_kernel when `left` steps remain: up to tile_H steps; FULL when it is exactly tile_H.
void plan_tile_launch(const ContextPlan& c, int left, LaunchPlan* out)
{
  LaunchPlan a{};
  a.k = std::min(c.tile_H, left);
  a.full = a.k == c.tile_H;
  a.tiles_x = c.nx / c.tile_T;
  a.ntiles_total = a.tile_count = a.nblocks = a.launched_blocks = c.n_tiles;
  a.row = tile_row(c.tile_T, c.tile_H, a.full != 0, c.fused ? kTileTermsFused : c.fast_avvels ? kTermsFloat : kTermsDouble);
  *out = a;
}

// The rows the next push sends are the last launch's: its edge rows when the group was one launch of a row partition and those tile
// rows hold all next_total rows of either side (then the push need not wait for the interior launch); else the compute stream's.
bool edge_rows_suffice(const ContextPlan& c, const GroupPlan& g, const MacroRows& rows, int next_total)
{
  const int first = c.ghost_rows - g.ext(0), ty = multi_ty(g.k[0], c.multi_geom);
  return g.n == 1 && c.ghost_x == 0 && first + rows.bottom_edge_rows * ty >= c.ghost_rows + next_total &&
         first + (rows.bottom_edge_rows + rows.interior_rows) * ty <= c.ghost_rows + c.nyl - next_total;
}

// The widest access every row segment of a column message is aligned for, in the grid and in the messages, and the blocks of its
// kernel: 1024 vectors per block.
ColumnMessagePlan plan_column_message(const ContextPlan& c, int cols, int max_blocks, const long long* peer, int npeer)
{
  auto all_mult = [&](int m) {
    for (int i = 0; i < npeer; ++i) if (peer[i] % m != 0) return false;
    return cols % m == 0 && c.ghost_x % m == 0 && c.nxl % m == 0 && c.nx % m == 0 && c.ps % m == 0;
  };
  const int per = all_mult(4) ? 4 : all_mult(2) ? 2 : 1;
  const long long work = 18LL * c.nyl * (cols / per);                  // vectors of the launch
  return {per, static_cast<int>(std::max(1LL, std::min(static_cast<long long>(max_blocks), (work + 1023) / 1024)))};
}

}  // namespace lbm_internal

extern "C" {

int lbm_plan_next(int K, int four_rows, int tail4, int left)
{
  int k = left < K ? left : K;
  if (!four_rows || !tail4) return k;
  if (K == 3 && ((left % 3 == 1 && left >= 4) || (left % 3 == 2 && left >= 8))) k = 4;
  if (K == 4 && ((left % 4 == 3) || (left % 4 == 2 && left >= 6) || (left % 4 == 1 && left >= 9))) k = 3;
  // K = 5 (whole grids): 5s for as long as what they leave is 0 or at least 3, then 4 + 3 or 3 + 3 — ceil(left / 5) launches, the fewest
  // that 5s, 4s and 3s can make, and none shorter than 3 (11 = 5 + 3 + 3, 12 = 5 + 4 + 3, 7 = 4 + 3, 6 = 3 + 3)
  if (K == 5 && left >= 3) k = (left == 5 || left >= 8) ? 5 : left == 7 ? 4 : left == 6 ? 3 : left;
  return k;
}

// The launches between two halo exchanges of a partitioned run ("a group"): the next launches by lbm_plan_next for as long as their
// steps add up to at most `ghost` (the first launch of a group advances the ghost rows the later ones read), `group_max` launches at most.
// The first launch is always taken.  One implementation for the loops (plan_group above, with the context's four_rows / tail4)
// and for the public lbm_plan_group that bench.py and the tests plan with, so that the two cannot disagree.
int lbm_plan_group_for(int K, int four_rows, int tail4, int ghost, int group_max, int left, int* steps, int cap)
{
  int n = 0, used = 0;
  while (left > 0 && n < group_max) {
    const int k = lbm_plan_next(K, four_rows, tail4, left);
    if (n > 0 && used + k > ghost) break;
    if (n < cap) steps[n] = k;
    ++n; used += k; left -= k;
  }
  return n;
}

int lbm_plan_group(int K, int ghost, int group_max, int left, int* steps, int cap)
{
  if (K < 1 || K > 4 || ghost < K || group_max < 1 || left < 0 || cap < 0 || (cap > 0 && !steps)) { lbm_internal::set_error("lbm_plan_group: bad argument"); return -1; }
  return lbm_plan_group_for(K, ghost >= 4 ? 1 : 0, 1, ghost, group_max, left, steps, cap);
}

int lbm_plan_steps(int K, int four_rows, int n_steps, int* steps, int cap)
{
  if (K < 1 || K > 4 || n_steps < 0 || cap < 0 || (cap > 0 && !steps)) { lbm_internal::set_error("lbm_plan_steps: bad argument"); return -1; }
  int n = 0;
  for (int left = n_steps; left > 0; ++n) {
    const int k = lbm_plan_next(K, four_rows, 1, left);
    if (n < cap) steps[n] = k;
    left -= k;
  }
  return n;
}

int lbm_rank_layout(const lbm_params* p, int nranks, int rank, unsigned flags, lbm_layout* out)
{
  return rank_layout(knobs_from_env(), p, nranks, rank, flags, out);
}

int lbm_tile_layout_of(const lbm_params* p, int px, int py, int rank, unsigned flags, lbm_tile_layout* out)
{
  return tile_layout_of(knobs_from_env(), p, px, py, rank, flags, out);
}

// Row blocks or tiles, and which tiles, for `nranks` ranks: the decomposition whose ranks recompute the smallest share of cells they do not own.
// A rank of R rows and C columns that keeps g ghost rows / columns advances, averaged over a group of launches, about 3/8 g ghost rows per
// side (the first launch of a group g - k of them, the last none) and — tiles — all 2 g ghost columns in every launch:
//     row blocks     0.75 g / R              + 0.1 below 128 rows (an exchange every 8 steps), + 0.2 below 64 (every 4), + 1 below 32 (one-step loop)
//     column blocks  2 g / C + 0.02          (px x 1 tilings: no ghost rows, one exchange kernel; the margin: 128-row blocks against 320 / 384 /
//                                            448 / 512-column blocks came out 4.58 / 5.06, 5.39 / 5.87, 5.80 / 5.61, 4.36 / 4.01 us/step)
//     other tiles    0.75 g / R + 2 g / C + 0.05 (the second exchange kernel), thin blocks charged as thin row blocks are
// The rule orders the 25 pairs measured on 1-rank rings as they came out (profiles/r04/{wide,tile,auto,column}_*.json), us/step
// rows / tiles of the same cells: 8192 x 1024 43.8 / 46.0 as 1024 x 8192 column blocks and 45.5 as 2048 x 4096; 1024 x 128 3.28 / 4.05 as 128 x 1024,
// 4.13 as 256 x 512; 1024 x 256 3.99 / 4.93; 2048 x 256 5.5 / 6.2; 1024 x 64 3.25 / 3.51 as 512 x 128 (rows: a second exchange kernel and ghost
// columns cost more than the ghost rows of blocks this tall, or than a small block's frequent exchanges) — and 2048 x 128 4.36 / 4.01 as 512 x 512
// column blocks, 4096 x 128 6.15 / 5.37, 2048 x 64 4.12 / 3.31, 4096 x 64 5.38 / 4.03, 8192 x 64 7.45 / 5.64, 16384 x 64 13.2 / 8.7, 32768 x 32 18.3 / 9.4,
// 65536 x 16 21.8 / 9.5 (tiles: wide column blocks beat row blocks of up to 128 rows).  Every BASELINE.json config comes out as row blocks.
// A function of p, nranks and flags only.  *px == 1 means ROW BLOCKS (lbm_create_rank: no ghost columns), anything else lbm_create_tile on *px x *py.
int lbm_choose_rank_grid(const lbm_params* p, int nranks, unsigned flags, int* px, int* py)
{
  if (!p || !px || !py || nranks < 1) { set_error("lbm_choose_rank_grid: bad argument"); return 1; }
  *px = 1; *py = nranks;
  const Knobs knobs = knobs_from_env();
  lbm_layout rows;
  if (rank_layout(knobs, p, nranks, nranks - 1, flags, &rows)) return 1;
  if (nranks == 1) return 0;
  std::vector<int> nyl(nranks), dis(nranks);
  if (lbm_decompose(p->ny, nranks, nyl.data(), dis.data())) return 1;
  const int rmin = *std::min_element(nyl.begin(), nyl.end());
  auto thin = [](int r) { return (r < 128 ? 0.1 : 0.0) + (r < 64 ? 0.2 : 0.0); };
  double best = rows.macro_k > 0 ? 0.75 * rows.ghost / rmin + thin(rmin) : 1.0 + thin(rmin);
  for (int qx = 2; qx <= nranks; ++qx) {
    if (nranks % qx != 0) continue;
    lbm_tile_layout t;
    if (tile_layout_of(knobs, p, qx, nranks / qx, nranks - 1, flags, &t)) continue;      // a rank would fall out of K-step mode: not a candidate
    // (the last rank holds the smallest column block and, by the reference's rule, not the largest row block)
    // (a column block's 32 ghost columns count as 16 here: the rule was measured at 16, and the deeper halo only made the column blocks faster)
    const double cost = t.ghost_y > 0 ? 0.75 * t.ghost_y / t.ny_local + 2.0 * t.ghost_x / t.nx_local + 0.05 + thin(t.ny_local)
                                      : 2.0 * std::min(t.ghost_x, 16) / t.nx_local + 0.02;
    if (cost < best) { best = cost; *px = qx; *py = nranks / qx; }
  }
  (void)lbm_last_error();
  return 0;
}

// ---- the plan, for tests (lbm_internal.h; not part of the ABI): the knobs are read per call, as the layout functions read them ----
int lbm_plan_sizeof(void) { return static_cast<int>(sizeof(ContextPlan)); }
int lbm_plan_whole(const lbm_params* p, int free_cells, int y0, int ny_local, unsigned flags, int has_global_map, ContextPlan* out)
{
  return lbm_internal::plan_whole(knobs_from_env(), p, free_cells, y0, ny_local, flags, has_global_map != 0, out) ? 1 : 0;
}
int lbm_plan_rank(const lbm_params* p, int free_cells, int nranks, int rank, unsigned flags, ContextPlan* out)
{
  return lbm_internal::plan_rank(knobs_from_env(), p, free_cells, nranks, rank, flags, out) ? 1 : 0;
}
int lbm_plan_tile(const lbm_params* p, int free_cells, int px, int py, int rank, unsigned flags, ContextPlan* out)
{
  return lbm_internal::plan_tile(knobs_from_env(), p, free_cells, px, py, rank, flags, out) ? 1 : 0;
}
int lbm_plan_kernel_name(const ContextPlan* plan, char* kernel_name, size_t len)
{
  if (!plan || !kernel_name || !len) { set_error("lbm_plan_kernel_name: null argument"); return 1; }
  lbm_internal::plan_kernel_name(*plan, kernel_name, len);
  return 0;
}

// A block's dynamic LDS in a launch of k steps on geometry `geom` (lbm_geometry.h multi_lds_bytes, which the kernels are sized by); -1: not built.
int lbm_plan_multi_lds_bytes(int k, int geom)
{
  if (geom < kGeomStd || geom > kGeomTall || k < 1 || k > (geom == kGeomTall ? kMaxWholeGridSteps : kMaxMultiSteps)) return -1;
  return multi_lds_bytes(k, geom_for(k, geom));
}

int lbm_plan_launch_sizeof(void) { return static_cast<int>(sizeof(lbm_internal::LaunchPlan)); }
int lbm_plan_launch(const ContextPlan* plan, int k, int ext, int which, int says_ready, lbm_internal::LaunchPlan* out)
{
  if (!plan || !out || plan->multi_tiles_x <= 0 || k < 1 || k > (plan->multi_K == kMaxWholeGridSteps ? kMaxWholeGridSteps : kMaxMultiSteps) || ext < 0 || ext > kMaxGhost || which < lbm_internal::kLaunchWhole || which > lbm_internal::kLaunchEdge) {
    set_error("lbm_plan_launch: bad argument");
    return 1;
  }
  lbm_internal::plan_launch(*plan, knobs_from_env(), k, ext, which, says_ready != 0, out);
  return 0;
}

int lbm_plan_run_launches(const ContextPlan* plan, int n_steps, int schedule, lbm_internal::LaunchPlan* out, int cap)
{
  using namespace lbm_internal;
  if (!plan || n_steps < 0 || cap < 0 || (cap > 0 && !out) || (schedule != kScheduleSerial && schedule != kScheduleEdge)) { set_error("lbm_plan_run_launches: bad argument"); return -1; }
  const Knobs knobs = knobs_from_env();
  const KernelFamily family = family_of(*plan);
  int n = 0;
  LaunchPlan l;
  auto put = [&](const LaunchPlan& a) { if (n < cap) out[n] = a; ++n; };
  if (family == kFamilyTile) {
    for (int left = n_steps; left > 0; left -= l.k) { plan_tile_launch(*plan, left, &l); put(l); }
  } else if (family == kFamilyMulti && plan->ghost == 0) {                  // lbm_run: whole periodic grids
    for (int left = n_steps; left > 0; left -= l.k) { plan_launch(*plan, knobs, next_multi_k(*plan, left), 0, kLaunchWhole, false, &l); put(l); }
  } else if (family == kFamilyMulti) {                                     // the split-phase calls and the peer-to-peer loop: group by group
    for (int left = n_steps; left > 0;) {
      const GroupPlan g = plan_group(*plan, left);
      const bool more = left > g.total;
      for (int i = 0; i < g.n; ++i) {
        if (i == 0 && schedule == kScheduleEdge) {
          plan_launch(*plan, knobs, g.k[0], g.ext(0), kLaunchInterior, false, &l);
          if (l.nblocks > 0) put(l);
          plan_launch(*plan, knobs, g.k[0], g.ext(0), kLaunchEdge, false, &l);
        } else {
          plan_launch(*plan, knobs, g.k[i], g.ext(i), kLaunchWhole, g.n > 1 && i == g.n - 1 && more, &l);   // the group's last launch says "ready" for the next push
        }
        put(l);
      }
      left -= g.total;
    }
  }
  return n;
}

// ---- the double-precision mode's plan, for tests ----
int lbm_plan64_sizeof(void) { return static_cast<int>(sizeof(lbm_internal::Plan64)); }
int lbm_plan64_whole(const lbm64_params* p, unsigned flags, lbm_internal::Plan64* out)
{
  if (!p || !out) { set_error("lbm_plan64_whole: null argument"); return 1; }
  if (p->nx < 1 || p->ny < 3) { set_error("lbm_plan64_whole: nx must be positive and ny >= 3"); return 1; }
  if ((flags & ~lbm_internal::kFlags64) != 0u) { set_error("lbm_plan64_whole: a flag lbm64_create refuses"); return 1; }
  if (static_cast<long long>(p->nx) * p->ny > (1LL << 31) - 4096) { set_error("lbm_plan64_whole: grid too large for 32-bit cell indices"); return 1; }
  lbm_internal::plan64_whole(knobs_from_env(), p, flags, out);
  return 0;
}
int lbm_plan64_multi_sizeof(void) { return static_cast<int>(sizeof(lbm_internal::PlanMulti64)); }
int lbm_plan64_multi(const lbm64_params* p, unsigned flags, lbm_internal::PlanMulti64* out)
{
  lbm_internal::Plan64 plan;
  if (!out) { set_error("lbm_plan64_multi: null argument"); return 1; }
  if (lbm_plan64_whole(p, flags, &plan)) return 1;
  lbm_internal::plan64_multi(knobs_from_env(), p, plan, out);
  return 0;
}
int lbm_plan64_multi_kernel_name(const lbm_internal::PlanMulti64* plan, char* kernel_name, size_t len)
{
  if (!plan || !kernel_name || !len) { set_error("lbm_plan64_multi_kernel_name: null argument"); return 1; }
  lbm_internal::plan64_multi_kernel_name(*plan, kernel_name, len);
  return 0;
}
int lbm_plan64_multi_run_launches(const lbm_internal::PlanMulti64* plan, int n_steps, int* steps, int* full, int cap)
{
  if (!plan || !multi64_k_ok(plan->K) || n_steps < 0 || cap < 0 || (cap > 0 && (!steps || !full))) { set_error("lbm_plan64_multi_run_launches: bad argument"); return -1; }
  int n = 0;
  for (int left = n_steps; left > 0; ++n) {
    const int k = lbm_internal::plan64_multi_next_steps(*plan, left);
    if (n < cap) { steps[n] = k; full[n] = k == plan->K; }
    left -= k;
  }
  return n;
}
int lbm_plan64_multi_any_sizeof(void) { return static_cast<int>(sizeof(lbm_internal::PlanMultiAny64)); }
int lbm_plan64_multi_any(const lbm64_params* p, unsigned flags, lbm_internal::PlanMultiAny64* out)
{
  lbm_internal::Plan64 plan;
  if (!out) { set_error("lbm_plan64_multi_any: null argument"); return 1; }
  if (lbm_plan64_whole(p, flags, &plan)) return 1;
  lbm_internal::plan64_multi_any(knobs_from_env(), p, plan, out);
  return 0;
}
int lbm_plan64_multi_any_kernel_name(const lbm_internal::PlanMultiAny64* plan, char* kernel_name, size_t len)
{
  if (!plan || !kernel_name || !len) { set_error("lbm_plan64_multi_any_kernel_name: null argument"); return 1; }
  lbm_internal::plan64_multi_any_kernel_name(*plan, kernel_name, len);
  return 0;
}
int lbm_plan64_multi_any_run_launches(const lbm_internal::PlanMultiAny64* plan, int n_steps, int* steps, int* full, int cap)
{
  if (!plan || !multi64_k_ok(plan->K) || n_steps < 0 || cap < 0 || (cap > 0 && (!steps || !full))) { set_error("lbm_plan64_multi_any_run_launches: bad argument"); return -1; }
  int count = 0;
  for (int left = n_steps; left > 0; ++count) {
    const int k = lbm_internal::plan64_multi_any_next_steps(*plan, left);
    if (count < cap) { steps[count] = k; full[count] = k == plan->K; }
    left -= k;
  }
  return count;
}
int lbm_plan64_kernel_name(const lbm_internal::Plan64* plan, char* kernel_name, size_t len)
{
  if (!plan || !kernel_name || !len) { set_error("lbm_plan64_kernel_name: null argument"); return 1; }
  lbm_internal::plan64_kernel_name(*plan, kernel_name, len);
  return 0;
}
int lbm_plan64_run_launches(const lbm_internal::Plan64* plan, int n_steps, int* steps, int* full, int cap)
{
  if (!plan || n_steps < 0 || cap < 0 || (cap > 0 && (!steps || !full))) { set_error("lbm_plan64_run_launches: bad argument"); return -1; }
  int n = 0;
  for (int left = n_steps; left > 0; ++n) {
    const int k = lbm_internal::plan64_next_steps(*plan, left);
    if (n < cap) { steps[n] = k; full[n] = plan->tile_kernel && k == plan->tile_H; }
    left -= k;
  }
  return n;
}

int lbm_plan64_rows_sizeof(void) { return static_cast<int>(sizeof(lbm_internal::PlanRows64)); }
int lbm_plan64_rows(const lbm64_params* p, int nranks, int rank, unsigned flags, lbm_internal::PlanRows64* out)
{
  return lbm_internal::plan64_rows(knobs_from_env(), p, nranks, rank, flags, out);
}
int lbm_plan64_rows_kernel_name(const lbm_internal::PlanRows64* plan, char* kernel_name, size_t len)
{
  if (!plan || !kernel_name || !len) { set_error("lbm_plan64_rows_kernel_name: null argument"); return 1; }
  lbm_internal::plan64_rows_kernel_name(*plan, kernel_name, len);
  return 0;
}
int lbm_plan64_rows_multi_sizeof(void) { return static_cast<int>(sizeof(lbm_internal::PlanRowsMulti64)); }
int lbm_plan64_rows_multi(const lbm64_params* p, int nranks, int rank, unsigned flags, lbm_internal::PlanRowsMulti64* out)
{
  lbm_internal::PlanRows64 rows;
  if (!out) { set_error("lbm_plan64_rows_multi: null argument"); return 1; }
  const Knobs knobs = knobs_from_env();
  if (lbm_internal::plan64_rows(knobs, p, nranks, rank, flags, &rows)) return 1;
  lbm_internal::plan64_rows_multi(knobs, p, rows, out);
  return 0;
}
int lbm_plan64_rows_multi_kernel_name(const lbm_internal::PlanRowsMulti64* plan, char* kernel_name, size_t len)
{
  if (!plan || !kernel_name || !len) { set_error("lbm_plan64_rows_multi_kernel_name: null argument"); return 1; }
  lbm_internal::plan64_rows_multi_kernel_name(*plan, kernel_name, len);
  return 0;
}
int lbm_plan64_rows_multi_run_launches(const lbm_internal::PlanRowsMulti64* plan, int n_steps, int* steps, int* full, int cap)
{
  if (!plan || !multi64_k_ok(plan->K) || n_steps < 0 || cap < 0 || (cap > 0 && (!steps || !full))) { set_error("lbm_plan64_rows_multi_run_launches: bad argument"); return -1; }
  int n = 0;
  for (int left = n_steps; left > 0; ++n) {
    const int k = lbm_internal::plan64_rows_multi_next_steps(*plan, left);
    if (n < cap) { steps[n] = k; full[n] = k == plan->K; }
    left -= k;
  }
  return n;
}

int lbm_plan64_rows_multi_any_sizeof(void) { return static_cast<int>(sizeof(lbm_internal::PlanRowsMultiAny64)); }
int lbm_plan64_rows_multi_any(const lbm64_params* p, int nranks, int rank, unsigned flags, lbm_internal::PlanRowsMultiAny64* out)
{
  lbm_internal::PlanRows64 rows;
  if (!out) { set_error("lbm_plan64_rows_multi_any: null argument"); return 1; }
  const Knobs knobs = knobs_from_env();
  if (lbm_internal::plan64_rows(knobs, p, nranks, rank, flags, &rows)) return 1;
  lbm_internal::plan64_rows_multi_any(knobs, p, rows, out);
  return 0;
}
int lbm_plan64_rows_multi_any_kernel_name(const lbm_internal::PlanRowsMultiAny64* plan, char* kernel_name, size_t len)
{
  if (!plan || !kernel_name || !len) { set_error("lbm_plan64_rows_multi_any_kernel_name: null argument"); return 1; }
  lbm_internal::plan64_rows_multi_any_kernel_name(*plan, kernel_name, len);
  return 0;
}
int lbm_plan64_rows_multi_any_run_launches(const lbm_internal::PlanRowsMultiAny64* plan, int n_steps, int* steps, int* full, int cap)
{
  if (!plan || !multi64_k_ok(plan->K) || n_steps < 0 || cap < 0 || (cap > 0 && (!steps || !full))) { set_error("lbm_plan64_rows_multi_any_run_launches: bad argument"); return -1; }
  int n = 0;
  for (int left = n_steps; left > 0; ++n) {
    const int k = lbm_internal::plan64_rows_multi_any_next_steps(*plan, left);
    if (n < cap) { steps[n] = k; full[n] = k == plan->K; }
    left -= k;
  }
  return n;
}

int lbm_plan64_cols_sizeof(void) { return static_cast<int>(sizeof(lbm_internal::PlanCols64)); }
int lbm_plan64_cols(const lbm64_params* p, int nranks, int rank, unsigned flags, lbm_internal::PlanCols64* out)
{
  return lbm_internal::plan64_cols(knobs_from_env(), p, nranks, rank, flags, out);
}
int lbm_plan64_cols_kernel_name(const lbm_internal::PlanCols64* plan, char* kernel_name, size_t len)
{
  if (!plan || !kernel_name || !len) { set_error("lbm_plan64_cols_kernel_name: null argument"); return 1; }
  lbm_internal::plan64_cols_kernel_name(*plan, kernel_name, len);
  return 0;
}
int lbm_plan64_cols_run_launches(const lbm_internal::PlanCols64* plan, int n_steps, int* steps, int* full, int cap)
{
  if (!plan || !multi64_k_ok(plan->K) || n_steps < 0 || cap < 0 || (cap > 0 && (!steps || !full))) { set_error("lbm_plan64_cols_run_launches: bad argument"); return -1; }
  int n = 0;
  for (int left = n_steps; left > 0; ++n) {
    const int k = lbm_internal::plan64_cols_next_steps(*plan, left);
    if (n < cap) { steps[n] = k; full[n] = k == plan->K; }
    left -= k;
  }
  return n;
}

int lbm_plan_edge_rows_suffice(const ContextPlan* plan, int left)
{
  using namespace lbm_internal;
  if (!plan || plan->ghost <= 0 || left <= 0) return 0;
  const GroupPlan g = plan_group(*plan, left);
  if (left <= g.total) return 0;
  return edge_rows_suffice(*plan, g, macro_rows(*plan, g.k[0], g.ext(0)), plan_group(*plan, left - g.total).total) ? 1 : 0;
}

}  // extern "C"
