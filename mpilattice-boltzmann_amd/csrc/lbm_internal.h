// lbm_internal.h — shared between the host-only (lbm_host.cpp, lbm_plan.cpp) and device (lbm_kernels.hip, lbm_f64.hip, lbm_rows64.hip, lbm_cols64.hip)
// units of liblbm_d2q9.so.  Not part of the ABI.
#pragma once
#include <cstddef>
#include <string>

#include "lbm_d2q9.h"
#include "lbm_d2q9_f64.h"
#include "lbm_knobs.h"

namespace lbm_internal {
// Sets the calling thread's lbm_last_error() message.
void set_error(const std::string& msg);

// ---- lbm_plan.cpp: what a context is, decided before anything is allocated ----------------------------------------------------
// Everything lbm_create* decides that does not depend on a device pointer, written once by plan_whole / plan_rank / plan_tile and
// only read afterwards (lbm_ctx::plan).  Plain data in this order — tests/test_plan.py mirrors it field for field and refuses a
// library whose lbm_plan_sizeof() differs; flags that were bool in the context are 0 / 1 here.
struct ContextPlan {
  // the domain: storage row width (a tile rank's: owned + ghost columns), first owned row, owned rows, the LBM_FLAG_* of the context
  int nx, y0, nyl;
  unsigned flags;
  int self_periodic, accel_row;      // a whole periodic grid; row ny-2 in owned-row coordinates (-1: another rank's)
  int use_graph;                     // LBM_FLAG_GRAPH on a whole grid: hipGraph replay of the one-step launches
  float accel_w1, accel_w2, free_cells_inv;
  // K-step mode
  int multi_K;                       // > 0: advanced K steps per launch by lbm_multi_kernel<K>
  int ghost;                         // steps between two halo exchanges of a K-step partition (0: not one)
  int ghost_rows;                    // storage rows kept below / above the owned rows: `ghost`, or 0 for a tile rank that owns ALL rows (a column
                                     // block, py = 1), whose launches wrap in y as a whole grid's do: only columns are exchanged
  int group_max;                     // most launches a partitioned run makes per halo exchange (a group: their steps add up to <= ghost)
  // Tile (2-D) decomposition: the rank owns the columns [x0, x0 + nxl) of its rows as well.  Its storage rows hold ghost_x ghost columns on
  // each side and nx is THEIR width (nxl + 2 * ghost_x): kernels, masks and row arithmetic all work on storage rows; nx_global is the
  // grid's.  Everywhere else ghost_x = 0, nxl = nx_global = nx.
  int ghost_x, x0, nxl, nx_global, tiles_px, tiles_py, tile_rx, tile_ry;
  // sizes, in cells / floats / words
  long long ncells, ncells_storage, ps, grid_floats;   // owned cells; cells incl. ghost rows; plane stride; one grid's allocation
  int mask_words, nxp;               // obstacle bitfield; halo-buffer row (nx + guards): a halo message is 3 of them
  // the one-step kernels
  int nt_stores, lane_cells;         // non-temporal stores; cells per lane: 4 (vector form) or 1 (narrow form: tiny grids, nx % 4 != 0)
  // arithmetic
  int fast_avvels;                   // LBM_FLAG_FAST_AVVELS: float sum|u| terms in lbm_multi_kernel / lbm_tile_kernel
  int fused;                         // LBM_FLAG_FUSED_ARITH: every launch takes the fused instantiation of its kernel
  int multi_terms;                   // lbm_multi_kernel's form of the terms (kTerms*): LBM_FLAG_FAST_AVVELS / LBM_FLAG_EXACT_AVVELS
  int multi_tail4;                   // lbm_run at K = 3: 4-step launches instead of a 1- or 2-step tail (LBM_TUNE_MULTI_TAIL4)
  // lbm_tile_kernel: owned tile edge, ghost ring = max steps per launch; sub-steps with regions of at most tile_single_max cells deal one
  // cell per lane; tile_kernel: lbm_run advances several steps per launch with it (small whole grids)
  int tile_T, tile_H, tile_single_max, n_tiles, tile_kernel;
  // lbm_multi_kernel's launches (kGeom*): standard, narrow (32-wide tiles), tall (K = 4 on 64 x 24); tile width; tiles per row
  // (multi_tiles_x > 0: the context may launch it, and its kernels' LDS limit is raised)
  int multi_geom, multi_tx, multi_tiles_x;
  // the one-step launches: chunks per block and blocks (= partial sums) of the whole-grid, interior and boundary launch; room for the
  // partial sums of the longest launch of any kernel
  int iters_full, iters_interior, n_part_full, n_part_interior, n_part_boundary, partials_cap;
  // packed messages of a K-step partition, in floats: one row message, one column message, one row-message buffer (both directions)
  long long pack_floats, pack_floats_x, pack_alloc_floats;
};
static_assert(sizeof(ContextPlan) == 44 * sizeof(int) + 7 * sizeof(long long), "no padding: the order above is the layout");

enum { kPlanOk = 0, kPlanRefused = 1, kPlanRefusedLate = 2 };   // Late: lbm_create* checked it after hipSetDevice, whose failure reports first
// One per way of creating a context: lbm_create / lbm_create_global, lbm_create_rank (by way of the row layout), lbm_create_tile (by
// way of the tile layout).  On a refusal lbm_last_error() holds the message.
int plan_whole(const Knobs& knobs, const lbm_params* p, int free_cells, int y0, int ny_local, unsigned flags, bool has_global_map, ContextPlan* out);
int plan_rank(const Knobs& knobs, const lbm_params* p, int free_cells, int nranks, int rank, unsigned flags, ContextPlan* out);
int plan_tile(const Knobs& knobs, const lbm_params* p, int free_cells, int px, int py, int rank, unsigned flags, ContextPlan* out);
enum KernelFamily { kFamilyMulti, kFamilyTile, kFamilyStep };
KernelFamily family_of(const ContextPlan& plan);
void plan_kernel_name(const ContextPlan& plan, char* kernel_name, size_t len);
// Sizing rules the double-precision unit shares, stated in elements.
size_t plane_stride_floats(size_t ncells, int skew);
int pick_iters(long long quads, int max_blocks);
int blocks_for(long long quads, int iters);

// ---- lbm_plan.cpp: a context of the double-precision mode (include/lbm_d2q9_f64.h; lbm_f64.hip allocates and launches by it) ------
// Plain data in this order — tests/test_plan64.py mirrors it field for field and refuses a library whose lbm_plan64_sizeof() differs.
struct Plan64 {
  unsigned flags;                    // as lbm64_create took them
  // the one-step kernel: non-temporal stores; cells per lane (2: x-pairs, nx even; 1); pairs or cells of the grid; 256-unit chunks per
  // block; work blocks of a launch
  int nt_stores, lane_cells;
  unsigned units;
  int iters, blocks;
  // lbm_tile_kernel_f64<tile_T, tile_H>: tile_kernel = the context advances up to tile_H steps per launch with it (LBM64_FLAG_TILE_STEPS
  // on an eligible grid); tiles (= work blocks of a launch) and tiles per row; lanes and dynamic LDS bytes of a block (lbm_geometry.h)
  int tile_kernel, tile_T, tile_H, n_tiles, tiles_x, tile_block, tile_lds_bytes;
  int partials_cap;                  // doubles of each partials buffer: max(blocks, tile_H * n_tiles where tile_kernel) + 1
  long long ps, grid_doubles;        // plane stride; one grid's allocation, in doubles
};
static_assert(sizeof(Plan64) == 14 * sizeof(int) + 2 * sizeof(long long), "no padding: the order above is the layout");
// Fills *out for a whole nx x ny grid (the caller has checked nx >= 1, ny >= 3 and the flags).
void plan64_whole(const Knobs& knobs, const lbm64_params* p, unsigned flags, Plan64* out);
void plan64_kernel_name(const Plan64& plan, char* kernel_name, size_t len);
// Steps of the next launch of a run with `left` steps remaining: 1 (one-step kernel), or up to tile_H.
int plan64_next_steps(const Plan64& plan, int left);

// lbm_multi_kernel_f64<K, NT, FULL> (kernels/multi64.h) for a context: LBM64_FLAG_MULTI_STEPS on a grid that TX x TY tiles cover exactly, of
// at least LBM_TUNE_MULTI64_MIN cells, which Plan64.tile_kernel does not claim.  Plain data in this order (tests/test_plan64_multi.py
// mirrors it); beside Plan64, whose layout does not change.
struct PlanMulti64 {
  int multi_kernel;                  // the context advances up to K steps per launch with it
  int K, TX, TY;                     // steps of a full launch (LBM_TUNE_MULTI64_K); the tile (lbm_geometry.h)
  int tiles_x, n_tiles;              // tiles per row; tiles (= work blocks of a launch); 0 where the tiles do not cover the grid
  int block, lds_bytes;              // lanes and dynamic LDS bytes of a block
  int nt_stores;                     // Plan64.nt_stores: the rule and flags of the one-step kernel
  int partials_cap;                  // doubles of each partials buffer this kernel needs: K * n_tiles + 1
};
static_assert(sizeof(PlanMulti64) == 10 * sizeof(int), "no padding: the order above is the layout");
// Fills *out for the context whose Plan64 is `plan` (the caller has checked the arguments as for plan64_whole).
void plan64_multi(const Knobs& knobs, const lbm64_params* p, const Plan64& plan, PlanMulti64* out);
void plan64_multi_kernel_name(const PlanMulti64& plan, char* kernel_name, size_t len);
// Steps of the next launch with `left` steps remaining: K, or what is left as the one shorter launch that ends the run.
int plan64_multi_next_steps(const PlanMulti64& plan, int left);
// The flags lbm64_create takes: a store form, LBM64_FLAG_TILE_STEPS, LBM64_FLAG_MULTI_STEPS, LBM64_FLAG_MULTI_ANY_SIZE.
constexpr unsigned kFlags64 = LBM_FLAG_NT_STORES | LBM_FLAG_NO_NT_STORES | LBM64_FLAG_TILE_STEPS | LBM64_FLAG_MULTI_STEPS | LBM64_FLAG_MULTI_ANY_SIZE;

// The multi-step launches of a context, whichever flag asks for them: what PlanMulti64 says where the tiles cover the grid exactly
// (LBM64_FLAG_MULTI_STEPS, or LBM64_FLAG_MULTI_ANY_SIZE, which means it), and under LBM64_FLAG_MULTI_ANY_SIZE the edge-tile form of
// lbm_multi_kernel_f64 (kernels/multi64.h EDGE) on a grid they do not cover: nx even and >= TX, ny >= TY, at least LBM_TUNE_MULTI64_MIN
// cells, not claimed by Plan64.tile_kernel.  lbm_f64.hip allocates and launches by this plan.  Plain data in this order
// (tests/test_plan64_any.py mirrors it); beside Plan64 and PlanMulti64, whose layouts and values do not change.
struct PlanMultiAny64 {
  int multi_kernel, edge;            // the context advances up to K steps per launch with lbm_multi_kernel_f64; in its edge-tile form
  int K, TX, TY;                     // as PlanMulti64
  int tiles_x, tiles_y, n_tiles;     // ceil(nx / TX), ceil(ny / TY), their product (= work blocks of a launch); 0 where no multi-step kernel can tile the grid
  int last_x0, last_y0;              // where the last tile column and row start: nx - TX, ny - TY (the others at TX * tx, TY * ty)
  int block, lds_bytes;              // as PlanMulti64
  int nt_stores;                     // Plan64.nt_stores
  int partials_cap;                  // K * n_tiles + 1
};
static_assert(sizeof(PlanMultiAny64) == 14 * sizeof(int), "no padding: the order above is the layout");
// Fills *out for the context whose Plan64 is `plan` (the caller has checked the arguments as for plan64_whole).
void plan64_multi_any(const Knobs& knobs, const lbm64_params* p, const Plan64& plan, PlanMultiAny64* out);
void plan64_multi_any_kernel_name(const PlanMultiAny64& plan, char* kernel_name, size_t len);
// Steps of the next launch with `left` steps remaining: plan64_multi_next_steps' rule.
int plan64_multi_any_next_steps(const PlanMultiAny64& plan, int left);

// One rank of a row-partitioned double-precision run (include/lbm_d2q9_f64_rows.h; lbm_rows64.hip allocates and launches by it): the
// rows lbm_decompose gives the rank, the one-step launch over them by plan64_whole's rules, and the sizes of its two grids of
// ny_local + 2 storage rows (one ghost row below, one above).  Plain data in this order — tests/test_f64_rows_host.py mirrors it field
// for field and refuses a library whose lbm_plan64_rows_sizeof() differs.  Beside Plan64 and PlanMulti64, whose layouts do not change.
struct PlanRows64 {
  unsigned flags;                    // as lbm_rows64_create took them
  int nranks, rank;
  int y0, ny_local;                  // first owned row of the grid, owned rows (d2q9-bgk.c:834-862)
  // lbm_rows_kernel_f64: non-temporal stores (the rule of plan64_whole on the RANK's two grids); cells per lane (2: x-pairs, nx even; 1);
  // pairs or cells of the owned rows; 256-unit chunks per block; work blocks of a launch
  int nt_stores, lane_cells;
  unsigned units;
  int iters, blocks;
  int partials_cap;                  // doubles of each partials buffer: blocks + 1
  int mask_words;                    // words of the obstacle bitfield of the owned rows
  int accel_rank, accel_row;         // of the whole run: the rank that owns row ny-2 of the grid, and that row's index among its owned rows
  long long ps, grid_doubles;        // plane stride of (ny_local + 2) * nx cells; one grid's allocation, in doubles
};
static_assert(sizeof(PlanRows64) == 14 * sizeof(int) + 2 * sizeof(long long), "no padding: the order above is the layout");
constexpr int kMaxRows64Ranks = 64;  // MPI_PROCS, d2q9-bgk.c:67
// The flags lbm_rows64_create takes: a store form, LBM_ROWS64_FLAG_MULTI_STEPS, LBM_ROWS64_FLAG_MULTI_ANY_SIZE (lbm_d2q9_f64_rows.h;
// lbm_plan.cpp holds each pair equal).
constexpr unsigned kFlagRows64MultiSteps = 2048u, kFlagRows64MultiAnySize = 8192u;
constexpr unsigned kFlagsRows64 = LBM_FLAG_NT_STORES | LBM_FLAG_NO_NT_STORES | kFlagRows64MultiSteps | kFlagRows64MultiAnySize;
// Fills *out for rank `rank` of `nranks`; checks every argument itself.  0, or 1 and the message in lbm_last_error(): nranks outside
// 1..64, a rank without a row, a last rank with fewer than 3 rows, the shapes lbm64_create refuses, any flag outside kFlagsRows64.
// LBM_ROWS64_FLAG_MULTI_STEPS and LBM_ROWS64_FLAG_MULTI_ANY_SIZE change nothing in *out but .flags: what they add is PlanRowsMulti64's
// and PlanRowsMultiAny64's.
int plan64_rows(const Knobs& knobs, const lbm64_params* p, int nranks, int rank, unsigned flags, PlanRows64* out);
void plan64_rows_kernel_name(const PlanRows64& plan, char* kernel_name, size_t len);

// lbm_rows_multi_kernel_f64<K, NT, FULL> (kernels/rows_multi64.h) for one rank of a row-partitioned run: LBM_ROWS64_FLAG_MULTI_STEPS on
// a run whose EVERY rank TX x TY tiles cover exactly (nx % 32 == 0, every ny_local % 16 == 0) and whose smallest rank owns at least
// LBM_TUNE_MULTI64_MIN cells (by default 2^17, measured for ranks: lbm_plan.cpp): one decision for all ranks.  The rank then keeps `ghost` = K ghost rows on each side, advances up to K
// steps per launch and exchanges once per launch.  Plain data in this order (tests/test_plan64_rows_multi.py mirrors it); beside
// PlanRows64, whose layout and values do not change.
struct PlanRowsMulti64 {
  int multi_kernel;                  // every rank of the run advances up to K steps per launch with it
  int K, ghost;                      // steps of a full launch (LBM_TUNE_MULTI64_K); ghost rows on each side of the owned rows: K
  int tiles_x, n_tiles;              // tiles per row; tiles of this rank (= work blocks of a launch); 0 where the tiles do not cover every rank
  int block, lds_bytes;              // lanes and dynamic LDS bytes of a block
  int nt_stores;                     // plan64_whole's rule on the RANK's two grids of ny_local + 2 * ghost rows, and the flags
  int mask_words;                    // words of the window bitfield over the ny_local + 2 * ghost storage rows
  int partials_cap;                  // doubles of each partials buffer this kernel needs: K * n_tiles + 1
  long long ps, grid_doubles;        // plane stride of (ny_local + 2 * ghost) * nx cells; one grid's allocation, in doubles
};
static_assert(sizeof(PlanRowsMulti64) == 10 * sizeof(int) + 2 * sizeof(long long), "no padding: the order above is the layout");
// Fills *out for the rank whose PlanRows64 is `rows` (plan64_rows has checked the arguments).
void plan64_rows_multi(const Knobs& knobs, const lbm64_params* p, const PlanRows64& rows, PlanRowsMulti64* out);
void plan64_rows_multi_kernel_name(const PlanRowsMulti64& plan, char* kernel_name, size_t len);
// Steps of the next launch with `left` steps remaining: plan64_multi_next_steps' rule.
int plan64_rows_multi_next_steps(const PlanRowsMulti64& plan, int left);

// The multi-step launches of one rank of a row-partitioned run, whichever flag asks for them: what PlanRowsMulti64 says where the tiles
// cover every rank exactly (LBM_ROWS64_FLAG_MULTI_STEPS, or LBM_ROWS64_FLAG_MULTI_ANY_SIZE, which means it), and under
// LBM_ROWS64_FLAG_MULTI_ANY_SIZE the edge-tile form of lbm_rows_multi_kernel_f64 (kernels/rows_multi64.h EDGE) on a run they do not
// cover: nx even and >= TX, EVERY rank of at least TY rows, the smallest rank of at least LBM_TUNE_MULTI64_MIN cells.  One decision for
// all ranks: ranks of an uneven run differ in tiles_y, n_tiles, last_y0, mask_words, partials_cap, ps and grid_doubles and agree on the
// rest.  lbm_rows64.hip allocates and launches by this plan.  Plain data in this order (tests/test_plan64_rows_any.py mirrors it);
// beside PlanRows64 and PlanRowsMulti64, whose layouts and values do not change.
struct PlanRowsMultiAny64 {
  int multi_kernel, edge;            // every rank advances up to K steps per launch with lbm_rows_multi_kernel_f64; in its edge-tile form
  int K, ghost;                      // as PlanRowsMulti64
  int tiles_x, tiles_y, n_tiles;     // ceil(nx / TX), ceil(ny_local / TY) of THIS rank, their product (= work blocks of a launch); 0 where no multi-step kernel can tile the run
  int last_x0, last_y0;              // where the last tile column and this rank's last tile row start: nx - TX, and the OWNED row ny_local - TY
  int block, lds_bytes;              // as PlanRowsMulti64
  int nt_stores;                     // as PlanRowsMulti64
  int mask_words;                    // as PlanRowsMulti64
  int partials_cap;                  // K * n_tiles + 1
  long long ps, grid_doubles;        // as PlanRowsMulti64
};
static_assert(sizeof(PlanRowsMultiAny64) == 14 * sizeof(int) + 2 * sizeof(long long), "no padding: the order above is the layout");
// Fills *out for the rank whose PlanRows64 is `rows` (plan64_rows has checked the arguments).
void plan64_rows_multi_any(const Knobs& knobs, const lbm64_params* p, const PlanRows64& rows, PlanRowsMultiAny64* out);
void plan64_rows_multi_any_kernel_name(const PlanRowsMultiAny64& plan, char* kernel_name, size_t len);
// Steps of the next launch with `left` steps remaining: plan64_multi_next_steps' rule.
int plan64_rows_multi_any_next_steps(const PlanRowsMultiAny64& plan, int left);

// One rank of a column-partitioned double-precision run (include/lbm_d2q9_f64_cols.h; lbm_cols64.hip allocates and launches by this
// plan alone): the columns lbm_decompose_columns gives the rank, its storage of ny rows of pitch nxl + 2 * ghost doubles, and its launch
// of lbm_cols_multi_kernel_f64 (kernels/cols64.h).  Ranks of one run agree on K, ghost, block and lds_bytes and may differ in the rest.
// Plain data in this order — tests/test_plan64_cols.py mirrors it field for field and refuses a library whose lbm_plan64_cols_sizeof()
// differs.  Beside the other plans, whose layouts and values do not change.
struct PlanCols64 {
  unsigned flags;                    // as lbm_cols64_create took them
  int nranks, rank;
  int x0, nxl, pitch;                // first owned column of the grid, owned columns (lbm_decompose_columns), doubles of a storage row: nxl + 2 * ghost
  int K, ghost;                      // steps of a full launch (LBM_TUNE_MULTI64_K); ghost columns on each side: 2 * ceil(K / 2)
  int n_tiles, tiles_x;              // ceil(nxl / TX) * ceil(ny / TY) (= work blocks of a launch); ceil(nxl / TX)
  int edge;                          // the tiles do not cover the block exactly: the kernel's edge-tile form
  int nt_stores;                     // plan64_whole's rule on the RANK's two grids of ny * pitch cells, and the flags
  int block, lds_bytes;              // lanes and dynamic LDS bytes of a block
  int mask_words;                    // words of the window bitfield over the ny * pitch storage cells
  int partials_cap;                  // doubles of each partials buffer: K * n_tiles + 1
  long long ps, grid_doubles;        // plane stride of ny * pitch cells; one grid's allocation, in doubles
};
static_assert(sizeof(PlanCols64) == 16 * sizeof(int) + 2 * sizeof(long long), "no padding: the order above is the layout");
constexpr int kMaxCols64Ranks = 64;
// The flags lbm_cols64_create takes: a store form.
constexpr unsigned kFlagsCols64 = LBM_FLAG_NT_STORES | LBM_FLAG_NO_NT_STORES;
// Fills *out for rank `rank` of `nranks`; checks every argument itself.  0, or 1 and the message in lbm_last_error(): nranks outside
// 1..64, odd nx, a rank of fewer than TX columns, ny < TY, any flag outside kFlagsCols64, a rank's storage too large for 32-bit cell
// indices.
int plan64_cols(const Knobs& knobs, const lbm64_params* p, int nranks, int rank, unsigned flags, PlanCols64* out);
void plan64_cols_kernel_name(const PlanCols64& plan, char* kernel_name, size_t len);
// Steps of the next launch with `left` steps remaining: plan64_multi_next_steps' rule.
int plan64_cols_next_steps(const PlanCols64& plan, int left);

// ---- lbm_plan.cpp: what a run launches ------------------------------------------------------------------------------------------
// The launches between two halo exchanges of a partitioned run (a group): next_multi_k's launches for as long as their steps add
// up to at most the ghost rows, group_max at most.  Launch i of a group advances, besides the owned rows, ext(i) = the steps of the
// launches AFTER it in the group ghost rows on each side: what those launches read in place of exchanged rows.
constexpr int kGroupCap = 8;         // kMaxGroup (lbm_geometry.h)
struct GroupPlan {
  int n = 0, total = 0;
  int k[kGroupCap] = {};
  int ext(int i) const { int e = 0; for (int j = i + 1; j < n; ++j) e += k[j]; return e; }
};
int next_multi_k(const ContextPlan& plan, int left);
GroupPlan plan_group(const ContextPlan& plan, int left);

// One launch of lbm_multi_kernel: every geometric argument (MultiArgs of the same names, kernels/multi.h), its grid and its row of the
// kernel table (lbm_kernels.hip kMultiKernels).  Plain data, no HIP type and no pointer; tests/test_launch_plan.py mirrors it field for
// field and refuses a library whose lbm_plan_launch_sizeof() differs.  The launch adds what only the context knows: grids, plane
// bases, mask, partials, sums, counter and ready words.
// A launch of lbm_tile_kernel (plan_tile_launch) uses k, full, tiles_x, ntiles_total = tile_count = nblocks = launched_blocks and row
// (of kTileKernels, whose block size and LDS bytes the launch takes); the rest is 0.
enum LaunchWhich { kLaunchWhole = 0, kLaunchInterior = 1, kLaunchEdge = 2 };
struct LaunchPlan {
  int k, ext;                        // steps; ghost rows (and kept ghost columns) advanced on each side besides the owned cells
  int row_first, rows_compute, rows_storage, count_first, count_end;
  int cx0, cx1, keep_x0, keep_x1;
  int y_periodic, y0_global, tiles_x, ntiles_total;
  int tile_begin, tile_count, tile_begin2, tile_count2;      // the launch's tiles as two ranges, or (nrect > 0, tile ranks) as rectangles
  int nrect;
  struct Rect { int ty0, tx0, ntx, count; } rect[4];
  int nblocks, launched_blocks, xcd_remap;                   // tiles; blocks of the grid (+ 1: the fold block) after padding; tile order
  int part, row, lanes;                                      // kPart*; index into the kernel table; block size
  int full;                                                  // lbm_tile_kernel only: the launch makes exactly tile_H steps
};
void plan_launch(const ContextPlan& plan, const Knobs& knobs, int k, int ext, int which, bool says_ready, LaunchPlan* out);
void plan_tile_launch(const ContextPlan& plan, int left, LaunchPlan* out);
// Tile rows of a launch of k steps + ext: the first / last read exchanged rows, the interior rows between them do not (tile ranks: nor do
// the tile columns between left_cols and right_cols).  The rule and its comment: lbm_plan.cpp.
struct MacroRows { int bottom_edge_rows, interior_rows, top_edge_rows, left_cols, right_cols; };
MacroRows macro_rows(const ContextPlan& plan, int k, int ext);
// May the push for the next group (next_total rows per side) start before the interior launch of group `g`, whose first launch splits as `rows`, has finished ?
bool edge_rows_suffice(const ContextPlan& plan, const GroupPlan& g, const MacroRows& rows, int next_total);
// Access width (4, 2 or 1 floats) and blocks of a tile rank's column messages of `cols` columns per side: packed (lbm_macro_pack_x: no peer)
// or pushed into the neighbours' grids (peer: their storage widths, plane strides, owned and ghost columns, which every access must divide too).
struct ColumnMessagePlan { int per, blocks; };
ColumnMessagePlan plan_column_message(const ContextPlan& plan, int cols, int max_blocks, const long long* peer, int npeer);
}  // namespace lbm_internal

// Steps of the next launch of the K-step kernels when `left` steps remain (lbm_plan.cpp; lbm_plan_steps is its public
// form): shared by lbm_run, the split-phase macro-steps and the peer-to-peer loop, so that they cannot disagree.
extern "C" int lbm_plan_next(int K, int four_rows, int tail4, int left);
// The launches of the next group (one halo exchange) of a partitioned run; public form in lbm_d2q9.h (four_rows = ghost >= 4, tail4 on).
extern "C" int lbm_plan_group_for(int K, int four_rows, int tail4, int ghost, int group_max, int left, int* steps, int cap);
extern "C" int lbm_plan_group(int K, int ghost, int group_max, int left, int* steps, int cap);
// The plan a context of these arguments would get, for tests (lbm_plan.cpp); the knobs are read from the environment per call.
extern "C" int lbm_plan_sizeof(void);
extern "C" int lbm_plan_whole(const lbm_params* p, int free_cells, int y0, int ny_local, unsigned flags, int has_global_map, lbm_internal::ContextPlan* out);
extern "C" int lbm_plan_rank(const lbm_params* p, int free_cells, int nranks, int rank, unsigned flags, lbm_internal::ContextPlan* out);
extern "C" int lbm_plan_tile(const lbm_params* p, int free_cells, int px, int py, int rank, unsigned flags, lbm_internal::ContextPlan* out);
extern "C" int lbm_plan_kernel_name(const lbm_internal::ContextPlan* plan, char* kernel_name, size_t len);
// One launch of a context of that plan, and every step-kernel launch of a run of n_steps in the order a serial-schedule run enqueues them
// (schedule kScheduleSerial: each launch over all its tiles; kScheduleEdge: the first launch of a group as interior + edge, adjacent) —
// lbm_run, the split-phase calls and the peer-to-peer loop alike.  Returns the number of launches (the first `cap` are written), -1 on a bad argument.
extern "C" int lbm_plan_multi_lds_bytes(int k, int geom);   // a block's dynamic LDS in a launch of k steps on that geometry (-1: not built)
extern "C" int lbm_plan_launch_sizeof(void);
extern "C" int lbm_plan_launch(const lbm_internal::ContextPlan* plan, int k, int ext, int which, int says_ready, lbm_internal::LaunchPlan* out);
extern "C" int lbm_plan_run_launches(const lbm_internal::ContextPlan* plan, int n_steps, int schedule, lbm_internal::LaunchPlan* out, int cap);
// edge_rows_suffice for the group a run makes with `left` steps remaining and the one after it (0 where no group follows).
extern "C" int lbm_plan_edge_rows_suffice(const lbm_internal::ContextPlan* plan, int left);
// The same for the double-precision mode: the plan a context of these arguments would get (0, or 1 where lbm64_create refuses them), its
// kernel's name, and the launches of a run of n_steps (steps[i], and full[i] = 1 where launch i makes exactly tile_H steps of the tiled
// kernel); returns the number of launches (the first `cap` are written), -1 on a bad argument.
extern "C" int lbm_plan64_sizeof(void);
extern "C" int lbm_plan64_whole(const lbm64_params* p, unsigned flags, lbm_internal::Plan64* out);
extern "C" int lbm_plan64_kernel_name(const lbm_internal::Plan64* plan, char* kernel_name, size_t len);
extern "C" int lbm_plan64_run_launches(const lbm_internal::Plan64* plan, int n_steps, int* steps, int* full, int cap);
// And for lbm_multi_kernel_f64: the PlanMulti64 a context of these arguments would get (0, or 1 where lbm64_create refuses them), its
// kernel's name ("" where multi_kernel is 0), and the launches of a run (full[i] = 1 where launch i makes exactly K steps).
extern "C" int lbm_plan64_multi_sizeof(void);
extern "C" int lbm_plan64_multi(const lbm64_params* p, unsigned flags, lbm_internal::PlanMulti64* out);
extern "C" int lbm_plan64_multi_kernel_name(const lbm_internal::PlanMulti64* plan, char* kernel_name, size_t len);
extern "C" int lbm_plan64_multi_run_launches(const lbm_internal::PlanMulti64* plan, int n_steps, int* steps, int* full, int cap);
// And for the multi-step launches under either flag, LBM64_FLAG_MULTI_ANY_SIZE's edge-tile form among them: the PlanMultiAny64 a context
// of these arguments would get, its kernel's name ("" where multi_kernel is 0), and the launches of a run, all as above.
extern "C" int lbm_plan64_multi_any_sizeof(void);
extern "C" int lbm_plan64_multi_any(const lbm64_params* p, unsigned flags, lbm_internal::PlanMultiAny64* out);
extern "C" int lbm_plan64_multi_any_kernel_name(const lbm_internal::PlanMultiAny64* plan, char* kernel_name, size_t len);
extern "C" int lbm_plan64_multi_any_run_launches(const lbm_internal::PlanMultiAny64* plan, int n_steps, int* steps, int* full, int cap);
// And for a row-partitioned run: the PlanRows64 rank `rank` of `nranks` would get (0, or 1 where lbm_rows64_create refuses the
// arguments, the message in lbm_last_error()), and its kernel's name.
extern "C" int lbm_plan64_rows_sizeof(void);
extern "C" int lbm_plan64_rows(const lbm64_params* p, int nranks, int rank, unsigned flags, lbm_internal::PlanRows64* out);
extern "C" int lbm_plan64_rows_kernel_name(const lbm_internal::PlanRows64* plan, char* kernel_name, size_t len);
// And for lbm_rows_multi_kernel_f64: the PlanRowsMulti64 that rank would get (0, or 1 where lbm_rows64_create refuses the arguments), its
// kernel's name ("" where multi_kernel is 0), and the launches of a run on one rank (full[i] = 1 where launch i makes exactly K steps).
extern "C" int lbm_plan64_rows_multi_sizeof(void);
extern "C" int lbm_plan64_rows_multi(const lbm64_params* p, int nranks, int rank, unsigned flags, lbm_internal::PlanRowsMulti64* out);
extern "C" int lbm_plan64_rows_multi_kernel_name(const lbm_internal::PlanRowsMulti64* plan, char* kernel_name, size_t len);
extern "C" int lbm_plan64_rows_multi_run_launches(const lbm_internal::PlanRowsMulti64* plan, int n_steps, int* steps, int* full, int cap);
// And for a rank's multi-step launches under either flag, LBM_ROWS64_FLAG_MULTI_ANY_SIZE's edge-tile form among them: the
// PlanRowsMultiAny64 that rank would get, its kernel's name ("" where multi_kernel is 0), and the launches of a run on one rank.
extern "C" int lbm_plan64_rows_multi_any_sizeof(void);
extern "C" int lbm_plan64_rows_multi_any(const lbm64_params* p, int nranks, int rank, unsigned flags, lbm_internal::PlanRowsMultiAny64* out);
extern "C" int lbm_plan64_rows_multi_any_kernel_name(const lbm_internal::PlanRowsMultiAny64* plan, char* kernel_name, size_t len);
extern "C" int lbm_plan64_rows_multi_any_run_launches(const lbm_internal::PlanRowsMultiAny64* plan, int n_steps, int* steps, int* full, int cap);
// And for a column-partitioned run: the PlanCols64 rank `rank` of `nranks` would get (0, or 1 where lbm_cols64_create refuses the
// arguments before its first HIP call, the message in lbm_last_error()), its kernel's name, and the launches of a run on one rank.
extern "C" int lbm_plan64_cols_sizeof(void);
extern "C" int lbm_plan64_cols(const lbm64_params* p, int nranks, int rank, unsigned flags, lbm_internal::PlanCols64* out);
extern "C" int lbm_plan64_cols_kernel_name(const lbm_internal::PlanCols64* plan, char* kernel_name, size_t len);
extern "C" int lbm_plan64_cols_run_launches(const lbm_internal::PlanCols64* plan, int n_steps, int* steps, int* full, int cap);
