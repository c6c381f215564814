// lbm_kernels.hip — the translation unit of liblbm_d2q9.so's device half: it includes the hand-written
// gfx950 (MI355X / CDNA4) kernels (kernels/*.h) and implements the device entry points of the C ABI
// (include/lbm_d2q9.h) for the D2Q9-BGK timestep path of ag14774/MPILattice-Boltzmann.
//
// What one lattice step does, whichever kernel performs it (reference lines, relative to its tree):
//   pull-stream            d2q9-bgk.c:526-538      9 populations from the 3x3 neighbourhood
//   moments + equilibrium  d2q9-bgk.c:546-646
//   BGK relaxation         d2q9-bgk.c:658-666      fluid cells
//   bounce-back            d2q9-bgk.c:687-695      obstacle cells
//   sum |u|                d2q9-bgk.c:667,684      -> per-block partial, double
//   accelerate_flow        d2q9-bgk.c:442-478      fused as an EPILOGUE on global row ny-2: the row is
//                                                  written already accelerated for the next step
//   av_vels[tt-1]          d2q9-bgk.c:367          block 0 of the next launch folds the partials
//
// Kernels (all produce the same bits): kernels/multi.h lbm_multi_kernel<K>, kernels/tile.h lbm_tile_kernel<T,H>,
// kernels/step.h lbm_step_kernel / _narrow, kernels/aux.h the rest.  WHICH of them a context runs, on what geometry and with what
// buffer sizes, is decided before anything here is allocated: lbm_plan.cpp fills a ContextPlan (lbm_internal.h), and this file
// allocates, uploads and launches by it.  Nothing here writes the plan after creation.  WHAT a run launches is decided there too:
// the steps of each launch and the groups between two exchanges (next_multi_k, plan_group), and every launch's rows, columns, tiles,
// grid and kernel-table row as a LaunchPlan (plan_launch, plan_tile_launch).  Nothing here decides a tile range: launch_multi and
// launch_tile add pointers and run state to a LaunchPlan, after_launch / end_run keep the run state.
//
// Layout in HBM: struct-of-arrays, 9 planes of rows*nx floats (plane stride padded, see
// lbm_plan.cpp plane_stride_floats()), two grids (source / destination, swapped per launch like :376-378), the
// obstacle map as a bitfield (1 bit per cell); K-step row partitions carry K ghost rows per side.
// No MFMA anywhere: nothing on this path is a contraction.
//
// Arithmetic is written in the reference's operation order and this file is compiled with
// -ffp-contract=off, so the post-step populations are BIT-IDENTICAL to the reference's
// (gcc -std=c99 never fuses either); 1.0f/x and sqrt are correctly rounded (hipcc default
// -fhip-fp32-correctly-rounded-divide-sqrt).  Only the summation order of sum|u| differs
// (tree in double instead of a serial float accumulator).
//
// gfx950 only: 64-wide wavefronts are assumed throughout (wave reductions step through 32..1).

#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <type_traits>
#include <utility>
#include <vector>

#include "lbm_d2q9.h"
#include "lbm_internal.h"
#include "lbm_hip_try.h"
#include "lbm_knobs.h"
#include "kernels/common.h"
#include "kernels/step.h"
#include "kernels/tile.h"
#include "kernels/multi.h"
#include "kernels/aux.h"
#include "kernels/p2p.h"

namespace {

// ------------------------------------------------------------------------------------------------
// host side of the device ABI
// ------------------------------------------------------------------------------------------------

size_t round_up(size_t v, size_t m) { return (v + m - 1) / m * m; }

// Profile modes (lbm_set_profile, lbm_p2p_set_profile): timing events around the launches of a run, from a pool grown on demand and
// reused from run to run (used = 0).  stamp: the next event, recorded on `s`; nullptr when the profile is off or on failure.
struct EventPool {
  bool on = false;
  std::vector<hipEvent_t> pool;
  size_t used = 0;
  hipEvent_t stamp(hipStream_t s)
  {
    if (!on) return nullptr;
    if (used == pool.size()) {
      hipEvent_t e = nullptr;
      if (hipEventCreate(&e) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
      pool.push_back(e);
    }
    hipEvent_t e = pool[used++];
    if (hipEventRecord(e, s) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return e;
  }
  void destroy() { for (hipEvent_t e : pool) (void)hipEventDestroy(e); }
};

}  // namespace

struct lbm_ctx {
  Knobs knobs;                       // the environment knobs as lbm_create* read them (lbm_knobs.h)
  lbm_internal::ContextPlan plan{};  // kernel, geometry and sizes: written once by lbm_plan.cpp before anything below is allocated
  lbm_params p{};                    // (p.nx: the storage row width, plan.nx)
  int free_cells = 0;
  int device = 0;
  unsigned long long* ready_ptr[4] = {nullptr, nullptr, nullptr, nullptr};   // peer-to-peer loop: the next launch_multi says "ready for epoch ready_epoch" to the
  unsigned long long ready_epoch = 0;                       // neighbours (MultiArgs::ready) and waits for theirs; cleared by that launch
  const unsigned long long* ready_wait = nullptr;
  long long ready_timeout_ticks = 0;
  int* ready_err = nullptr;
  float* grid_alloc[2] = {nullptr, nullptr};
  float* grid[2] = {nullptr, nullptr};       // plane 0 row 0 (after the front guard)
  int cur = 0;
  uint32_t* mask = nullptr;
  float* halo_alloc = nullptr;
  float* macro_pack[2] = {nullptr, nullptr};   // K-step mode: packed outgoing / incoming messages, [dir][plane][K*nx] each
  float* macro_pack_x[2] = {nullptr, nullptr}; // tile ranks: packed outgoing / incoming COLUMN messages, [dir][plane][nyl][ghost_x] each (lbm_macro_pack_x)
  float* send[2] = {nullptr, nullptr};
  bool release_sends = false;   // send[] point into peers' windows (one-step peer-to-peer loop)
  float* recv[2] = {nullptr, nullptr};
  double* partials[2] = {nullptr, nullptr};
  double* fold_scratch = nullptr;   // kFoldSlices x 8 slice sums of the end-of-run fold (long partial vectors)
  double* sums = nullptr;
  int sums_cap = 0;
  double* sums_host = nullptr;   // pinned, sums_cap doubles
  std::vector<std::pair<double*, double*>> sums_retired;   // (sums, sums_host) outgrown by a longer run: freed by lbm_destroy only (ensure_sums)
  int* counter = nullptr;
  bool counter_clean = false;   // the device counter is 0 (left so by the last fold of the previous run, enqueued on counter_clean_stream): a run that
  hipStream_t counter_clean_stream = nullptr;   // starts on THAT stream needs no memset; on another stream nothing would order its first fold behind the reset
  hipStream_t stream = nullptr;
  // launch-bound grids (plan.use_graph): kGraphSteps steps captured once into a hipGraph and replayed (one per
  // starting source grid); see lbm_run
  hipGraphExec_t graph_exec[2] = {nullptr, nullptr};
  hipEvent_t ev_begin = nullptr, ev_end = nullptr;   // around the step kernels of the last run
  int ev_launches = 0;
  int ev_tile_launches = 0;
  bool ev_valid = false;
  // run state (split-phase and lbm_run)
  int run_steps = 0, run_done = 0;
  int parity = 0;            // partials buffer written by the current step
  int n_prev = 0;            // partial count of the previous step (0 = nothing to fold)
  int n_prev_vecs = 1;       // ... and how many step vectors of that length the previous launch left (tile kernel: up to 8)
  EventPool prof;            // lbm_set_profile: timing events around every step-kernel launch of lbm_run
  struct ProfLaunch { int steps; hipEvent_t begin, end; };
  std::vector<ProfLaunch> prof_launches;
};

namespace {

using lbm_internal::KernelFamily;
using lbm_internal::kFamilyMulti;
using lbm_internal::kFamilyTile;
using lbm_internal::kFamilyStep;
KernelFamily family_of(const lbm_ctx* c) { return lbm_internal::family_of(c->plan); }

// Every entry point that launches or copies goes through here: the launch must happen with the context's
// device current (a caller driving several GPUs from one thread leaves another one current).
hipStream_t pick_stream(lbm_ctx* c, void* stream)
{
  (void)hipSetDevice(c->device);   // cheap when already current
  return stream ? static_cast<hipStream_t>(stream) : c->stream;
}

void drop_graphs(lbm_ctx* c)
{
  for (hipGraphExec_t& g : c->graph_exec) {
    if (g) (void)hipGraphExecDestroy(g);
    g = nullptr;
  }
}

// Room for n per-step sums.  Invariant: between the start of a partitioned run and its end nothing here calls hipFree, hipHostFree or
// anything else that waits for the whole DEVICE — the neighbours may already spin in their wait kernels for this rank's rows, and where
// several ranks of one process share a device such a wait dead-locks until the time-out (seen in the randomised tile cases: a second run
// one step longer than the first).  create_impl sizes the buffers for max(max_iters, 4096) steps; a longer run allocates larger ones and
// retires the old ones to sums_retired, which lbm_destroy frees.
int ensure_sums(lbm_ctx* c, int n)
{
  if (n <= c->sums_cap) return 0;
  n = std::max(n, std::max(c->p.max_iters, 4096));
  double* dev = nullptr;
  double* host = nullptr;
  HIP_TRY(hipMalloc(&dev, sizeof(double) * static_cast<size_t>(n)));
  // pinned landing zone of lbm_run's one device-to-host copy per run (a pageable destination is staged: ~2x the time)
  const hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&host), sizeof(double) * static_cast<size_t>(n), hipHostMallocDefault);
  if (e != hipSuccess) {
    c->sums_retired.emplace_back(dev, nullptr);
    lbm_internal::set_error(std::string("hipHostMalloc (per-step sums): ") + hipGetErrorString(e));
    return 1;
  }
  drop_graphs(c);   // captured kernel arguments hold the old pointer (whole grids only: partitions capture no graph)
  if (c->sums || c->sums_host) c->sums_retired.emplace_back(c->sums, c->sums_host);
  c->sums = dev;
  c->sums_host = host;
  c->sums_cap = n;
  return 0;
}

StepArgs base_args(lbm_ctx* c, bool accel_next)
{
  StepArgs a{};
  a.src = c->grid[c->cur];
  a.dst = c->grid[c->cur ^ 1];
  a.mask = c->mask;
  a.mask_words = c->plan.mask_words;
  a.ps = c->plan.ps;
  a.nx = c->p.nx;
  a.nyl = c->plan.nyl;
  a.nxp = c->plan.nxp;
  a.omega = c->p.omega;
  a.accel_w1 = c->plan.accel_w1;
  a.accel_w2 = c->plan.accel_w2;
  a.accel_row = accel_next ? c->plan.accel_row : -1;
  a.sums = c->sums;
  a.counter = c->counter;
  return a;
}

// Every instantiation of the one-step kernel, by [narrow form: one cell per lane][non-temporal stores][fused arithmetic].
using StepKernel = void (*)(StepArgs);
constexpr StepKernel kStepKernels[2][2][2] = {
  {{&lbm_step_kernel<kCellsPerLane, false, false>, &lbm_step_kernel<kCellsPerLane, false, true>},
   {&lbm_step_kernel<kCellsPerLane, true, false>, &lbm_step_kernel<kCellsPerLane, true, true>}},
  {{&lbm_step_kernel<1, false, false>, &lbm_step_kernel<1, false, true>},
   {&lbm_step_kernel<1, true, false>, &lbm_step_kernel<1, true, true>}},
};

void launch_step(lbm_ctx* c, const StepArgs& a, int blocks, hipStream_t s)
{
  kStepKernels[c->plan.lane_cells == 1][c->plan.nt_stores][c->plan.fused]<<<dim3(blocks + 1), dim3(kBlock), 0, s>>>(a);   // + the fold block
}

// Every instantiation of lbm_multi_kernel a context may launch, one row per (geometry, steps, terms, launch form; lbm_geometry.h multi_row)
// with what a launch of it needs besides its LaunchPlan.  Rows of the tall geometry with K < 4 name the standard kernels (geom_for): no
// instantiation of their own.  The terms index kMultiTermsFused: the instantiation <K, kTermsCompensated + kTermsFused, GEOM, PART>.
struct MultiKernel { void (*fn)(MultiArgs); size_t lds_bytes; };
static_assert(kTermsDouble == 0 && kTermsFloat == 1 && kTermsCompensated == 2 && kPartPlain == 0 && kPartTile == 3 && kGeomTall == 2, "the values index the table");
template <int ROW>
constexpr MultiKernel multi_kernel_row()
{
  constexpr int PART = ROW % kMultiParts, TERMS = ROW / kMultiParts % kMultiTerms, K = ROW / (kMultiParts * kMultiTerms) % kMaxMultiSteps + 1,
                GEOM = geom_for(K, ROW / kMultiRowsPerGeom);
  static_assert(multi_row(K, ROW / kMultiRowsPerGeom, TERMS, PART) == ROW, "multi_row and its inverse");
  static_assert(MultiGeom<K, GEOM>::LANES == multi_lanes(K, ROW / kMultiRowsPerGeom), "LaunchPlan::lanes is the row's block size");
  return {&lbm_multi_kernel<K, TERMS == kMultiTermsFused ? (kTermsCompensated | kTermsFused) : TERMS, GEOM, PART>, MultiGeom<K, GEOM>::lds_bytes};
}
// ... and behind them (multi_row5) the five-step launch of whole grids: tall geometry, plain form, one row per terms index.
template <int TERMS>
constexpr MultiKernel multi_kernel_row5()
{
  using G = MultiGeom<kMaxWholeGridSteps, kGeomTall>;
  static_assert(G::LANES == multi_lanes(kMaxWholeGridSteps, kGeomTall) && G::owned_lanes && G::compact0, "the tall tile, one owned pair per lane, population 0 out of the frame");
  return {&lbm_multi_kernel<kMaxWholeGridSteps, TERMS == kMultiTermsFused ? (kTermsCompensated | kTermsFused) : TERMS, kGeomTall, kPartPlain>, G::lds_bytes};
}
template <size_t... ROW>
constexpr std::array<MultiKernel, sizeof...(ROW) + kMultiTerms> multi_kernel_rows(std::index_sequence<ROW...>)
{
  static_assert(kMultiTerms == 4 && multi_row5(3) == sizeof...(ROW) + 3, "the four rows below");
  return {{multi_kernel_row<static_cast<int>(ROW)>()..., multi_kernel_row5<0>(), multi_kernel_row5<1>(), multi_kernel_row5<2>(), multi_kernel_row5<3>()}};
}
constexpr auto kMultiKernels = multi_kernel_rows(std::make_index_sequence<kMultiRows>{});
static_assert(kMultiKernels.size() == kMultiRowsTotal, "every row a LaunchPlan can name");

// Kernels whose dynamic LDS is above the default limit (lbm_multi_kernel's tall geometry: 79 KB; lbm_tile_kernel<16, 8>: 74 KB) need the limit
// raised — per DEVICE (a function attribute belongs to the device's copy of the code object): called from lbm_create on the context's
// device, not from the first launch of a process.  Rows [first, end) of a kernel table.
template <typename Table>
hipError_t raise_lds_limits(const Table& rows, int first, int end)
{
  for (int r = first; r < end; ++r) {
    if (rows[r].lds_bytes <= 65536) continue;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(rows[r].fn), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(rows[r].lds_bytes));
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}
hipError_t raise_multi_lds_limits_for(int geom)          // every instantiation a context of this geometry may launch (K = 3 tails of the tall one: standard)
{
  const hipError_t e = raise_lds_limits(kMultiKernels, geom * kMultiRowsPerGeom, (geom + 1) * kMultiRowsPerGeom);
  if (e != hipSuccess || geom != kGeomTall) return e;
  return raise_lds_limits(kMultiKernels, kMultiRows, kMultiRowsTotal);   // the five-step launch of whole grids
}

// Does the device hold two blocks of the five-step launch per CU ?  Its 76.6 KB of LDS are sized for exactly that (lbm_geometry.h); a
// device whose LDS allocation rounds them past half a CU's would run one block of twelve waves per CU, at which the four-step launch is
// the faster form.  Asked once per context that plans the form (lbm_create / lbm_create_global), with the context's device current.
bool five_step_launch_fits(int terms_row)
{
  const MultiKernel& k = kMultiKernels[multi_row5(terms_row)];
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(k.fn), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(k.lds_bytes)) != hipSuccess) { (void)hipGetLastError(); return false; }
  int blocks = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, reinterpret_cast<const void*>(k.fn), multi_lanes(kMaxWholeGridSteps, kGeomTall), k.lds_bytes) != hipSuccess) { (void)hipGetLastError(); return false; }
  return blocks >= 2;
}

// A whole-grid plan that names the five-step launch holds only if the device fits it twice per CU; otherwise the context is planned again
// as LBM_TUNE_MULTI_K=4 would plan it.
int plan_whole_on_device(const Knobs& knobs, const lbm_params* p, int free_cells, int y0, int ny_local, unsigned flags, bool has_global_map, int device,
                         lbm_internal::ContextPlan* plan)
{
  const int status = lbm_internal::plan_whole(knobs, p, free_cells, y0, ny_local, flags, has_global_map, plan);
  if (status != lbm_internal::kPlanOk || plan->multi_K != kMaxWholeGridSteps) return status;
  if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return status; }          // create_impl reports a bad device
  if (five_step_launch_fits(plan->fused ? kMultiTermsFused : plan->multi_terms)) return status;
  Knobs four = knobs;
  four.multi_k = kMaxMultiSteps;
  return lbm_internal::plan_whole(four, p, free_cells, y0, ny_local, flags, has_global_map, plan);
}

using lbm_internal::LaunchPlan;
using lbm_internal::GroupPlan;
using lbm_internal::kLaunchWhole;
using lbm_internal::kLaunchInterior;
using lbm_internal::kLaunchEdge;

// One launch of lbm_multi_kernel by its plan (lbm_plan.cpp plan_launch: rows, columns, tiles, grid and table row).  Added here, what
// only the context knows: grids, plane bases and mask, the partials by parity and what is left to fold, sums and counter, the ready words.
void launch_multi(lbm_ctx* c, const LaunchPlan& l, bool accel_last, bool fold, hipStream_t s)
{
  MultiArgs a{};
  a.src = c->grid[c->cur]; a.dst = c->grid[c->cur ^ 1];
  for (int k = 0; k < 9; ++k) { a.srck[k] = a.src + k * c->plan.ps; a.dstk[k] = a.dst + k * c->plan.ps; }
  a.mask = c->mask; a.ps = c->plan.ps; a.nx = c->p.nx;
  a.row_first = l.row_first; a.rows_compute = l.rows_compute; a.rows_storage = l.rows_storage;
  a.count_first = l.count_first; a.count_end = l.count_end;
  a.cx0 = l.cx0; a.cx1 = l.cx1; a.keep_x0 = l.keep_x0; a.keep_x1 = l.keep_x1;
  a.y_periodic = l.y_periodic; a.y0_global = l.y0_global; a.ny_global = c->p.ny;
  a.tiles_x = l.tiles_x;
  a.tile_begin = l.tile_begin; a.tile_count = l.tile_count; a.tile_begin2 = l.tile_begin2; a.tile_count2 = l.tile_count2;
  a.ntiles_total = l.ntiles_total;
  a.nrect = l.nrect;
  for (int i = 0; i < l.nrect; ++i) a.rect[i] = MultiArgs::Rect{l.rect[i].ty0, l.rect[i].tx0, l.rect[i].ntx, l.rect[i].count};
  a.xcd_remap = l.xcd_remap; a.nblocks = l.nblocks;
  a.omega = c->p.omega; a.accel_w1 = c->plan.accel_w1; a.accel_w2 = c->plan.accel_w2;
  a.accel_row = c->p.ny - 2; a.accel_last = accel_last ? 1 : 0;
  a.partials_out = c->partials[c->parity];
  a.prev_partials = c->partials[c->parity ^ 1];
  a.n_prev = fold ? c->n_prev : 0; a.n_prev_vecs = (fold && c->n_prev > 0) ? c->n_prev_vecs : 0;
  a.sums = c->sums; a.counter = c->counter;
  a.ready[0] = c->ready_ptr[0]; a.ready[1] = c->ready_ptr[1]; a.ready_x[0] = c->ready_ptr[2]; a.ready_x[1] = c->ready_ptr[3];
  a.ready_epoch = c->ready_epoch;
  a.wait_ready = c->ready_epoch ? c->ready_wait : nullptr; a.timeout_ticks = c->ready_timeout_ticks; a.err = c->ready_err;
  c->ready_epoch = 0;
  const MultiKernel& k = kMultiKernels[l.row];
  k.fn<<<dim3(l.launched_blocks + 1), dim3(l.lanes), k.lds_bytes, s>>>(a);                            // + the fold block
}

// Every instantiation of lbm_tile_kernel, one row per (geometry, FULL, terms; lbm_geometry.h tile_row) with what a launch of it needs.
struct TileKernel { void (*fn)(TileArgs); int block; size_t lds_bytes; };
static_assert(kTermsDouble == 0 && kTermsFloat == 1, "the values index the table");
template <int ROW>
constexpr TileKernel tile_kernel_row()
{
  constexpr int TERMS = ROW % kTileTerms, H = ROW / (2 * kTileTerms) % 2 ? 4 : 8, T = ROW / (4 * kTileTerms) ? 8 : 16;
  constexpr bool FULL = ROW / kTileTerms % 2 != 0;
  static_assert(tile_row(T, H, FULL, TERMS) == ROW, "tile_row and its inverse");
  return {&lbm_tile_kernel<T, H, FULL, TERMS == kTileTermsFused ? (kTermsDouble | kTermsFused) : TERMS>, TileGeom<T, H>::block, TileGeom<T, H>::lds_bytes};
}
template <size_t... ROW>
constexpr std::array<TileKernel, sizeof...(ROW)> tile_kernel_rows(std::index_sequence<ROW...>) { return {{tile_kernel_row<static_cast<int>(ROW)>()...}}; }
constexpr auto kTileKernels = tile_kernel_rows(std::make_index_sequence<kTileRows>{});

// One launch of lbm_tile_kernel by its plan (lbm_plan.cpp plan_tile_launch); every launch of such a run has this form.
void launch_tile(lbm_ctx* c, const LaunchPlan& l, bool accel_last, hipStream_t s)
{
  TileArgs a{};
  a.src = c->grid[c->cur]; a.dst = c->grid[c->cur ^ 1];
  a.mask = c->mask; a.ps = c->plan.ps; a.nx = c->p.nx; a.ny = c->plan.nyl; a.tiles_x = l.tiles_x;
  a.ksteps = l.k;
  a.single_max = c->plan.tile_single_max;
  a.omega = c->p.omega; a.accel_w1 = c->plan.accel_w1; a.accel_w2 = c->plan.accel_w2;
  a.accel_row = c->plan.accel_row; a.accel_last = accel_last ? 1 : 0;
  a.partials_out = c->partials[c->parity];
  a.prev_partials = c->partials[c->parity ^ 1];
  a.n_prev = c->n_prev; a.n_prev_vecs = c->n_prev > 0 ? c->n_prev_vecs : 0;
  a.sums = c->sums; a.counter = c->counter;
  const TileKernel& k = kTileKernels[l.row];
  k.fn<<<dim3(l.launched_blocks + 1), dim3(k.block), k.lds_bytes, s>>>(a);   // + the fold block
}

// The state flip after a launch (d2q9-bgk.c:376-378): it left `vecs` step vectors of n_partials per-block sums to fold and made `steps` steps.
void after_launch(lbm_ctx* c, int n_partials, int vecs, int steps)
{
  c->n_prev = n_partials;
  c->n_prev_vecs = vecs;
  c->parity ^= 1;
  c->cur ^= 1;
  c->run_done += steps;
}

int begin_run(lbm_ctx* c, int n_steps, hipStream_t s)
{
  if (ensure_sums(c, n_steps)) return 1;
  // the per-step sums of a run go to sums[counter++]: the counter starts at 0.  The last fold of a run leaves it there
  // (fold_last(final)); a memset launch — a kernel boundary on the critical path of a short run — only when it did not
  if (!c->counter_clean || c->counter_clean_stream != s) HIP_TRY(hipMemsetAsync(c->counter, 0, sizeof(int), s));
  c->counter_clean = false;
  c->run_steps = n_steps;
  c->run_done = 0;
  c->n_prev = 0;
  c->n_prev_vecs = 1;
  c->parity = 0;
  if (c->plan.accel_row >= 0 && n_steps > 0) {
    // accelerate_flow of step 0 (d2q9-bgk.c:345-348); later steps get it from the kernel epilogue
    const int nx = c->p.nx;
    hipLaunchKernelGGL(lbm_accelerate_kernel, dim3((c->plan.nxl + 255) / 256), dim3(256), 0, s, c->grid[c->cur], c->plan.ps,
                       c->mask, nx, c->plan.ghost_rows + c->plan.accel_row, c->plan.accel_w1, c->plan.accel_w2, c->plan.ghost_x, c->plan.nxl);
    HIP_TRY(hipGetLastError());
  }
  c->ev_valid = false;
  c->ev_launches = 0;
  c->ev_tile_launches = 0;
  HIP_TRY(hipEventRecord(c->ev_begin, s));
  return 0;
}

// d2q9-bgk.c:367 for the LAST launch of a (macro-)step sequence: its per-block sums have no following launch to fold them.
// final: the run ends here — the fold also resets the counter for the next run.
int fold_last(lbm_ctx* c, hipStream_t s, bool final = false)
{
  if (c->n_prev == 0) return 0;          // already folded (lbm_step_fold)
  const double* part = c->partials[c->parity ^ 1];
  // one block folds 23 K partials (4 vectors of an 8192 x 1024-row rank's 5760 tiles) in 31 us — at the end of EVERY run, on the critical
  // path of a 20-step region; sliced over 64 blocks per vector and folded again it is two launches of a few us (threshold was 8192)
  if (c->n_prev >= c->knobs.fold_sliced_min) {
    hipLaunchKernelGGL(lbm_fold_slices_kernel, dim3(kFoldSlices, c->n_prev_vecs), dim3(kBlock), 0, s, part, c->n_prev, c->fold_scratch);
    hipLaunchKernelGGL(lbm_fold_kernel, dim3(1), dim3(kBlock), 0, s, c->fold_scratch, kFoldSlices, c->n_prev_vecs, c->sums, c->counter, final ? 1 : 0);
  } else {
    hipLaunchKernelGGL(lbm_fold_kernel, dim3(1), dim3(kBlock), 0, s, part, c->n_prev, c->n_prev_vecs, c->sums, c->counter, final ? 1 : 0);
  }
  HIP_TRY(hipGetLastError());
  c->n_prev = 0;
  c->n_prev_vecs = 1;
  c->counter_clean = final;
  c->counter_clean_stream = s;
  return 0;
}

// The end of a run on stream `s`: the closing event, the launch count lbm_last_run_kernel_ms reports, the last fold (which resets the counter).
int end_run(lbm_ctx* c, int launches, hipStream_t s)
{
  HIP_TRY(hipEventRecord(c->ev_end, s));
  c->ev_launches = launches;
  c->ev_valid = true;
  return fold_last(c, s, /*final=*/true);
}

constexpr int kGraphSteps = 64;   // even: the source/destination roles and the partial-sum parity return to their start

// One whole-grid step of a self-contained domain: launch + state flip (d2q9-bgk.c:345-378).
void full_step(lbm_ctx* c, bool accel_next, hipStream_t s)
{
  const long long quads = static_cast<long long>(c->p.nx / c->plan.lane_cells) * c->plan.nyl;
  StepArgs a = base_args(c, accel_next);
  a.quad_begin = 0; a.quad_end = static_cast<int>(quads);
  a.quad_begin2 = a.quad_end2 = 0;
  a.iters = c->plan.iters_full;
  a.partials_out = c->partials[c->parity];
  a.prev_partials = c->partials[c->parity ^ 1];
  a.n_prev = c->n_prev;
  launch_step(c, a, c->plan.n_part_full, s);
  after_launch(c, c->plan.n_part_full, 1, 1);
}

// Captures kGraphSteps mid-run steps (previous partials to fold, accelerate epilogue on) starting
// from the current source grid.  Every per-step quantity that changes from step to step lives on
// the device (sums[counter++]), so the same graph replays anywhere inside a run.
int ensure_graph(lbm_ctx* c, hipStream_t s)
{
  if (c->graph_exec[c->cur]) return 0;
  const int cur = c->cur, parity = c->parity, n_prev = c->n_prev, run_done = c->run_done;
  hipGraph_t graph = nullptr;
  HIP_TRY(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
  for (int i = 0; i < kGraphSteps; ++i) full_step(c, true, s);
  hipError_t e = hipStreamEndCapture(s, &graph);
  c->cur = cur; c->parity = parity; c->n_prev = n_prev; c->run_done = run_done;   // nothing ran
  HIP_TRY(e);
  e = hipGraphInstantiate(&c->graph_exec[cur], graph, nullptr, nullptr, 0);
  (void)hipGraphDestroy(graph);
  HIP_TRY(e);
  return 0;
}

}  // namespace

// Obstacle bitfield of the storage rows: bit i of the linear storage cell index, row r of the storage taken
// from row_ptr(r).  Word ranges are packed by several host threads (67 M cells at 8192x8192).
template <typename RowPtr>
static void pack_obstacle_bits(std::vector<uint32_t>& bits, int rows, int nx, RowPtr row_ptr)
{
  const size_t ncells = static_cast<size_t>(rows) * nx, nwords = (ncells + 31) / 32;
  auto pack = [&](size_t w0, size_t w1) {
    size_t i = w0 * 32;
    int r = static_cast<int>(i / nx), x = static_cast<int>(i - static_cast<size_t>(r) * nx);
    const int* row = r < rows ? row_ptr(r) : nullptr;
    for (size_t w = w0; w < w1; ++w) {
      uint32_t v = 0;
      for (int b = 0; b < 32 && i < ncells; ++b, ++i) {
        if (row[x]) v |= 1u << b;
        if (++x == nx) { x = 0; ++r; row = r < rows ? row_ptr(r) : nullptr; }
      }
      bits[w] = v;
    }
  };
  unsigned workers = std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
  if (nwords < (1u << 16)) workers = 1;
  if (workers == 1) { pack(0, nwords); return; }
  std::vector<std::thread> pool;
  const size_t per = (nwords + workers - 1) / workers;
  for (unsigned t = 0; t < workers; ++t) {
    const size_t w0 = std::min(nwords, t * per), w1 = std::min(nwords, w0 + per);
    if (w0 < w1) pool.emplace_back(pack, w0, w1);
  }
  for (std::thread& t : pool) t.join();
}

// The shared allocator of lbm_create / lbm_create_global / lbm_create_rank / lbm_create_tile: the plan (lbm_plan.cpp) has decided; here
// the device is made current, the buffers are allocated and uploaded by the plan, the LDS limits of the kernels it names are raised and
// the state is initialised.  plan_status: what the entry point's plan_* call returned — a refusal that lbm_create* has always made with
// the device current (kPlanRefusedLate) is reported only after a bad device had its say.  The obstacle flags of the ghost rows come
// either from obstacles_global (ny*nx, lbm_create_global) or from obstacles_window ((ny_local + 2*ghost_rows) storage rows: the rows
// around the partition only, lbm_create_rank / lbm_create_tile).
static int create_impl(lbm_ctx** out, int plan_status, const lbm_internal::ContextPlan& plan, const Knobs& knobs, const lbm_params* p, int free_cells,
                       const int* obstacles_rows, const int* obstacles_global, const int* obstacles_window, int device)
{
  if (plan_status == lbm_internal::kPlanRefused) return 1;
  const std::string refused = plan_status == lbm_internal::kPlanRefusedLate ? lbm_last_error() : "";
  HIP_TRY(hipSetDevice(device));
  if (plan_status != lbm_internal::kPlanOk) { lbm_internal::set_error(refused); return 1; }
  lbm_ctx* c = new lbm_ctx();
  c->knobs = knobs;
  c->plan = plan;
  c->p = *p;
  c->p.nx = plan.nx;
  c->free_cells = free_cells;
  c->device = device;

  auto fail = [&](void) { lbm_destroy(c); return 1; };

  HIP_TRY_OR(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking), return fail());
  HIP_TRY_OR(hipEventCreate(&c->ev_begin), return fail());
  HIP_TRY_OR(hipEventCreate(&c->ev_end), return fail());
  const size_t grid_floats = static_cast<size_t>(plan.grid_floats);
  for (int g = 0; g < 2; ++g) {
    HIP_TRY_OR(hipMalloc(&c->grid_alloc[g], sizeof(float) * grid_floats), return fail());
    HIP_TRY_OR(hipMemsetAsync(c->grid_alloc[g], 0, sizeof(float) * grid_floats, c->stream), return fail());
    c->grid[g] = c->grid_alloc[g] + 64;
  }
  if (knobs.debug_addr)      // placement experiments (scripts/experiments/alloc_order.py)
    std::fprintf(stderr, "lbm_create: grids at %p %p (%zu bytes each, plane stride %zu floats)\n", static_cast<void*>(c->grid_alloc[0]),
                 static_cast<void*>(c->grid_alloc[1]), sizeof(float) * grid_floats, static_cast<size_t>(plan.ps));
  // obstacle bitfield
  const size_t mwords = static_cast<size_t>(plan.mask_words);
  std::vector<uint32_t> bits(mwords, 0u);
  {
    const int nx = plan.nx, ny = p->ny, ghost = plan.ghost_rows, y0 = plan.y0;
    const int rows = plan.nyl + 2 * ghost;
    if (ghost == 0) pack_obstacle_bits(bits, rows, nx, [&](int r) { return obstacles_rows + static_cast<size_t>(r) * nx; });
    else if (obstacles_window) pack_obstacle_bits(bits, rows, nx, [&](int r) { return obstacles_window + static_cast<size_t>(r) * nx; });
    else pack_obstacle_bits(bits, rows, nx, [&](int r) {          // storage row -> global row, periodic
      int g = (y0 + r - ghost) % ny;
      if (g < 0) g += ny;
      return obstacles_global + static_cast<size_t>(g) * nx;
    });
  }
  HIP_TRY_OR(hipMalloc(&c->mask, sizeof(uint32_t) * mwords), return fail());
  HIP_TRY_OR(hipMemcpy(c->mask, bits.data(), sizeof(uint32_t) * mwords, hipMemcpyHostToDevice), return fail());
  // halo buffers: 2 send + 2 recv, each [3][nxp]
  const size_t hb = static_cast<size_t>(3) * plan.nxp;
  HIP_TRY_OR(hipMalloc(&c->halo_alloc, sizeof(float) * hb * 4), return fail());
  HIP_TRY_OR(hipMemsetAsync(c->halo_alloc, 0, sizeof(float) * hb * 4, c->stream), return fail());
  c->send[0] = c->halo_alloc; c->send[1] = c->halo_alloc + hb;
  c->recv[0] = c->halo_alloc + 2 * hb; c->recv[1] = c->halo_alloc + 3 * hb;
  if (plan.ghost > 0) {
    for (int i = 0; i < 2; ++i) HIP_TRY_OR(hipMalloc(&c->macro_pack[i], sizeof(float) * plan.pack_alloc_floats), return fail());
    if (plan.ghost_x > 0)             // a tile rank's column messages: here, never during a run (ensure_sums)
      for (int i = 0; i < 2; ++i) HIP_TRY_OR(hipMalloc(&c->macro_pack_x[i], sizeof(float) * 2 * plan.pack_floats_x), return fail());
  }
  // the kernels the plan names: lbm_multi_kernel's of its geometry, or lbm_tile_kernel's (up to 74 KB of dynamic LDS per block — two
  // 9 x R x R float buffers — above the 64 KB default limit).  Here, while the device still clears the grids: after the allocations
  // below, which wait for it, these host calls made lbm_create of a 2048 x 2048 grid 1.45 ms instead of 0.97
  if (plan.multi_tiles_x > 0) HIP_TRY_OR(raise_multi_lds_limits_for(plan.multi_geom), return fail());
  else if (plan.tile_kernel) HIP_TRY_OR(raise_lds_limits(kTileKernels, 0, kTileRows), return fail());
  for (int i = 0; i < 2; ++i) HIP_TRY_OR(hipMalloc(&c->partials[i], sizeof(double) * plan.partials_cap), return fail());
  HIP_TRY_OR(hipMalloc(&c->fold_scratch, sizeof(double) * kFoldSlices * 8), return fail());
  HIP_TRY_OR(hipMalloc(&c->counter, sizeof(int)), return fail());
  HIP_TRY_OR(hipMemsetAsync(c->counter, 0, sizeof(int), c->stream), return fail());
  if (ensure_sums(c, 1)) return fail();                   // max(max_iters, 4096) steps before any run starts (ensure_sums)
  // initial state (d2q9-bgk.c:880-902)
  {
    const float w0 = p->density * 4.0f / 9.0f, w1 = p->density / 9.0f, w2 = p->density / 36.0f;
    const size_t cells = static_cast<size_t>(plan.ncells_storage);
    const int blocks = static_cast<int>((cells + 255) / 256);
    hipLaunchKernelGGL(lbm_init_kernel, dim3(blocks), dim3(256), 0, c->stream, c->grid[0], static_cast<size_t>(plan.ps), cells, w0, w1, w2);
    HIP_TRY_OR(hipGetLastError(), return fail());
  }
  HIP_TRY_OR(hipStreamSynchronize(c->stream), return fail());
  *out = c;
  return 0;
}

// The owned cells of a context as the I/O entry points see them: all columns of the owned rows, or — a rank of the tile
// decomposition — the columns [ghost_x, ghost_x + nxl) of its storage rows.
static ColWindow col_window(const lbm_ctx* c) { return ColWindow{static_cast<unsigned>(c->p.nx), static_cast<unsigned>(c->plan.ghost_x), static_cast<unsigned>(c->plan.nxl)}; }
static size_t owned_cells(const lbm_ctx* c) { return static_cast<size_t>(c->plan.nxl) * c->plan.nyl; }

extern "C" {

int lbm_create(lbm_ctx** out, const lbm_params* p, int free_cells, const int* obstacles_rows, int y0,
               int ny_local, int device, unsigned flags)
{
  if (!out || !p || !obstacles_rows) { lbm_internal::set_error("lbm_create: null argument"); return 1; }
  *out = nullptr;
  const Knobs knobs = knobs_from_env();
  lbm_internal::ContextPlan plan;
  const int status = plan_whole_on_device(knobs, p, free_cells, y0, ny_local, flags, false, device, &plan);
  return create_impl(out, status, plan, knobs, p, free_cells, obstacles_rows, nullptr, nullptr, device);
}

int lbm_create_global(lbm_ctx** out, const lbm_params* p, int free_cells, const int* obstacles_all, int y0,
                      int ny_local, int device, unsigned flags)
{
  if (!obstacles_all || !p || y0 < 0) { lbm_internal::set_error("lbm_create_global: bad argument"); return 1; }
  if (!out) { lbm_internal::set_error("lbm_create: null argument"); return 1; }
  *out = nullptr;
  const Knobs knobs = knobs_from_env();
  lbm_internal::ContextPlan plan;
  const int status = plan_whole_on_device(knobs, p, free_cells, y0, ny_local, flags, true, device, &plan);
  return create_impl(out, status, plan, knobs, p, free_cells, obstacles_all + static_cast<size_t>(y0) * p->nx, obstacles_all, nullptr, device);
}

int lbm_create_rank(lbm_ctx** out, const lbm_params* p, int free_cells, const int* obstacle_window, int nranks,
                    int rank, int device, unsigned flags)
{
  if (!obstacle_window) { lbm_internal::set_error("lbm_create_rank: null argument"); return 1; }
  if (!out) {      // refused after the layout's own refusals, as always
    lbm_layout lay;
    if (lbm_rank_layout(p, nranks, rank, flags, &lay) == 0) lbm_internal::set_error("lbm_create: null argument");
    return 1;
  }
  *out = nullptr;
  const Knobs knobs = knobs_from_env();
  lbm_internal::ContextPlan plan;
  const int status = lbm_internal::plan_rank(knobs, p, free_cells, nranks, rank, flags, &plan);
  const int* rows = status == lbm_internal::kPlanOk ? obstacle_window + static_cast<size_t>(plan.ghost_rows) * plan.nx : nullptr;   // the owned rows inside the window
  return create_impl(out, status, plan, knobs, p, free_cells, rows, nullptr, obstacle_window, device);
}

// ---- tile (2-D) decomposition: px x py ranks, rank = ry * px + rx (the layout: lbm_plan.cpp tile_layout_of) ----
int lbm_create_tile(lbm_ctx** out, const lbm_params* p, int free_cells, const int* obstacle_window, int px, int py, int rank, int device, unsigned flags)
{
  if (!obstacle_window) { lbm_internal::set_error("lbm_create_tile: null argument"); return 1; }
  if (!out) {      // refused after the layout's own refusals, as always
    lbm_tile_layout lay;
    if (lbm_tile_layout_of(p, px, py, rank, flags, &lay) == 0) lbm_internal::set_error("lbm_create: null argument");
    return 1;
  }
  *out = nullptr;
  const Knobs knobs = knobs_from_env();
  lbm_internal::ContextPlan plan;
  const int status = lbm_internal::plan_tile(knobs, p, free_cells, px, py, rank, flags, &plan);
  const int* rows = status == lbm_internal::kPlanOk ? obstacle_window + static_cast<size_t>(plan.ghost_rows) * plan.nx : nullptr;   // the owned rows inside the window
  return create_impl(out, status, plan, knobs, p, free_cells, rows, nullptr, obstacle_window, device);
}


int lbm_tile_info(const lbm_ctx* c, lbm_tile_layout* out)
{
  if (!c || !out) { lbm_internal::set_error("lbm_tile_info: null argument"); return 1; }
  std::memset(out, 0, sizeof *out);
  out->px = c->plan.tiles_px; out->py = c->plan.tiles_py; out->rx = c->plan.tile_rx; out->ry = c->plan.tile_ry;
  out->x0 = c->plan.x0; out->nx_local = c->plan.nxl; out->y0 = c->plan.y0; out->ny_local = c->plan.nyl;
  out->macro_k = c->plan.ghost > 0 ? c->plan.multi_K : 0; out->ghost = c->plan.ghost; out->ghost_x = c->plan.ghost_x; out->group = c->plan.group_max;
  out->ghost_y = c->plan.ghost_rows;
  return 0;
}

int lbm_destroy(lbm_ctx* c)
{
  if (!c) return 0;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  drop_graphs(c);
  for (int g = 0; g < 2; ++g) if (c->grid_alloc[g]) (void)hipFree(c->grid_alloc[g]);
  if (c->mask) (void)hipFree(c->mask);
  if (c->halo_alloc) (void)hipFree(c->halo_alloc);
  for (float* b : c->macro_pack) if (b) (void)hipFree(b);
  for (float* b : c->macro_pack_x) if (b) (void)hipFree(b);
  for (int i = 0; i < 2; ++i) if (c->partials[i]) (void)hipFree(c->partials[i]);
  if (c->sums) (void)hipFree(c->sums);
  if (c->sums_host) (void)hipHostFree(c->sums_host);
  for (const auto& r : c->sums_retired) {
    if (r.first) (void)hipFree(r.first);
    if (r.second) (void)hipHostFree(r.second);
  }
  if (c->fold_scratch) (void)hipFree(c->fold_scratch);
  if (c->counter) (void)hipFree(c->counter);
  if (c->ev_begin) (void)hipEventDestroy(c->ev_begin);
  if (c->ev_end) (void)hipEventDestroy(c->ev_end);
  c->prof.destroy();
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
  return 0;
}

int lbm_run(lbm_ctx* c, int n_steps, float* av_vels)
{
  if (!c) { lbm_internal::set_error("lbm_run: null context"); return 1; }
  if (!c->plan.self_periodic) { lbm_internal::set_error("lbm_run: partition is not a self-contained domain; use the lbm_step_* calls"); return 1; }
  if (n_steps < 0) { lbm_internal::set_error("lbm_run: negative step count"); return 1; }
  if (n_steps == 0) return 0;
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  c->prof.used = 0;
  c->prof_launches.clear();
  if (begin_run(c, n_steps, s)) return 1;
  const KernelFamily family = family_of(c);
  for (int t = 0; family != kFamilyStep && t < n_steps;) {
    // up to multi_K steps per pass over HBM (lbm_multi_kernel; a step count that K does not divide: next_multi_k), or up to tile_H
    // steps per launch (lbm_tile_kernel)
    LaunchPlan l;
    if (family == kFamilyMulti) lbm_internal::plan_launch(c->plan, c->knobs, lbm_internal::next_multi_k(c->plan, n_steps - t), 0, kLaunchWhole, c->ready_epoch != 0, &l);
    else lbm_internal::plan_tile_launch(c->plan, n_steps - t, &l);
    hipEvent_t pb = c->prof.stamp(s);
    if (family == kFamilyMulti) launch_multi(c, l, /*accel_last=*/t + l.k < n_steps, /*fold=*/true, s);
    else launch_tile(c, l, /*accel_last=*/t + l.k < n_steps, s);
    if (c->prof.on) c->prof_launches.push_back({l.k, pb, c->prof.stamp(s)});
    after_launch(c, l.ntiles_total, l.k, l.k);
    t += l.k;
    ++c->ev_tile_launches;
  }
  for (int t = 0; family == kFamilyStep && t < n_steps;) {
    // launch-bound grids: replay a captured block of kGraphSteps steps while at least one more
    // step follows it (the last step of a run is launched directly: it must not accelerate)
    if (c->plan.use_graph && c->n_prev > 0 && n_steps - t > kGraphSteps) {
      if (ensure_graph(c, s)) return 1;
      HIP_TRY(hipGraphLaunch(c->graph_exec[c->cur], s));
      c->run_done += kGraphSteps;
      t += kGraphSteps;
    } else {
      hipEvent_t pb = c->prof.stamp(s);
      full_step(c, /*accel_next=*/t + 1 < n_steps, s);
      if (c->prof.on) c->prof_launches.push_back({1, pb, c->prof.stamp(s)});
      t += 1;
    }
  }
  HIP_TRY(hipGetLastError());
  if (end_run(c, family != kFamilyStep ? c->ev_tile_launches : n_steps, s)) return 1;
  // blocking waits: polling hipStreamQuery first measured no faster on 20-step runs of a 1-rank ring of 8192 x 1024 rows
  // (52.70 us/step blocking, 52.63 polling; profiles/r03/ab_ring_spin_8192x1024_s20.txt)
  if (av_vels) {
    const double* host = c->sums_host;
    HIP_TRY(hipMemcpyAsync(c->sums_host, c->sums, sizeof(double) * n_steps, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const double inv = static_cast<double>(c->plan.free_cells_inv);
    for (int t = 0; t < n_steps; ++t) av_vels[t] = static_cast<float>(host[t] * inv);   // d2q9-bgk.c:367
  } else {
    HIP_TRY(hipStreamSynchronize(s));
  }
  return 0;
}

int lbm_get_cells(lbm_ctx* c, float* cells_aos)
{
  if (!c || !cells_aos) { lbm_internal::set_error("lbm_get_cells: null argument"); return 1; }
  HIP_TRY(hipSetDevice(c->device));
  float* tmp = nullptr;
  const size_t n = owned_cells(c) * 9;
  HIP_TRY(hipMalloc(&tmp, sizeof(float) * n));
  const int blocks = static_cast<int>((n + 255) / 256);
  hipLaunchKernelGGL(lbm_soa_to_aos_kernel, dim3(blocks), dim3(256), 0, c->stream,
                     c->grid[c->cur] + static_cast<size_t>(c->plan.ghost_rows) * c->p.nx, tmp, c->plan.ps, owned_cells(c), col_window(c));
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(cells_aos, tmp, sizeof(float) * n, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  (void)hipFree(tmp);
  HIP_TRY(e);
  return 0;
}

int lbm_set_cells(lbm_ctx* c, const float* cells_aos)
{
  if (!c || !cells_aos) { lbm_internal::set_error("lbm_set_cells: null argument"); return 1; }
  HIP_TRY(hipSetDevice(c->device));
  float* tmp = nullptr;
  const size_t n = owned_cells(c) * 9;
  HIP_TRY(hipMalloc(&tmp, sizeof(float) * n));
  hipError_t e = hipMemcpyAsync(tmp, cells_aos, sizeof(float) * n, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) {
    const int blocks = static_cast<int>((n + 255) / 256);
    hipLaunchKernelGGL(lbm_aos_to_soa_kernel, dim3(blocks), dim3(256), 0, c->stream, tmp,
                       c->grid[c->cur] + static_cast<size_t>(c->plan.ghost_rows) * c->p.nx, c->plan.ps, owned_cells(c), col_window(c));
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  (void)hipFree(tmp);
  HIP_TRY(e);
  return 0;
}

int lbm_get_observables(lbm_ctx* c, float* obs)
{
  if (!c || !obs) { lbm_internal::set_error("lbm_get_observables: null argument"); return 1; }
  HIP_TRY(hipSetDevice(c->device));
  // row blocks of at most 16 M cells through a 256 MB device buffer: no second copy of the state
  // (whole rows per block, so that a block of a tile rank's column window starts on a row)
  const size_t total = owned_cells(c);
  const size_t chunk = std::min<size_t>(total, std::max<size_t>(1, static_cast<size_t>(c->knobs.obs_chunk_cells) / c->plan.nxl) * c->plan.nxl);
  float* tmp = nullptr;
  HIP_TRY(hipMalloc(&tmp, sizeof(float) * 4 * chunk));
  hipError_t e = hipSuccess;
  const float* owned = c->grid[c->cur] + static_cast<size_t>(c->plan.ghost_rows) * c->p.nx;
  for (size_t c0 = 0; c0 < total && e == hipSuccess; c0 += chunk) {
    const size_t n = std::min(chunk, total - c0);
    hipLaunchKernelGGL(lbm_observables_kernel, dim3(static_cast<unsigned>((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, c->stream,
                       owned + c0 / c->plan.nxl * c->p.nx, c->plan.ps, n, tmp, col_window(c));
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(obs + 4 * c0, tmp, sizeof(float) * 4 * n, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  }
  (void)hipFree(tmp);
  HIP_TRY(e);
  return 0;
}

int lbm_state_checksum(lbm_ctx* c, int y_begin, int y_end, unsigned long long* digest)
{
  if (!c || !digest) { lbm_internal::set_error("lbm_state_checksum: null argument"); return 1; }
  if (y_begin < c->plan.y0 || y_end > c->plan.y0 + c->plan.nyl || y_begin > y_end) { lbm_internal::set_error("lbm_state_checksum: rows outside the partition"); return 1; }
  HIP_TRY(hipSetDevice(c->device));
  unsigned long long* dev = nullptr;
  HIP_TRY(hipMalloc(&dev, sizeof *dev));
  const size_t nx = static_cast<size_t>(c->p.nx);
  const size_t n = static_cast<size_t>(y_end - y_begin) * c->plan.nxl;
  const size_t c0 = (static_cast<size_t>(c->plan.ghost_rows) + static_cast<size_t>(y_begin - c->plan.y0)) * nx;
  hipError_t e = hipMemsetAsync(dev, 0, sizeof *dev, c->stream);
  if (e == hipSuccess && n > 0) {
    const int blocks = static_cast<int>(std::min<size_t>((n + kBlock - 1) / kBlock, 4096));
    hipLaunchKernelGGL(lbm_checksum_kernel, dim3(blocks), dim3(kBlock), 0, c->stream, c->grid[c->cur] + c0, c->plan.ps, n,
                       static_cast<unsigned long long>(y_begin) * c->plan.nx_global + c->plan.x0, dev, col_window(c), static_cast<unsigned>(c->plan.nx_global));
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(digest, dev, sizeof *dev, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  (void)hipFree(dev);
  HIP_TRY(e);
  return 0;
}

int lbm_av_velocity_sum(lbm_ctx* c, double* tot_u)
{
  if (!c || !tot_u) { lbm_internal::set_error("lbm_av_velocity_sum: null argument"); return 1; }
  HIP_TRY(hipSetDevice(c->device));
  const int blocks = static_cast<int>(std::min<size_t>((owned_cells(c) + kBlock - 1) / kBlock, 1024));
  double* part = nullptr;
  HIP_TRY(hipMalloc(&part, sizeof(double) * blocks));
  // owned rows only; in K-step mode they start ghost rows in: bit offset ghost*nx of the bitfield (any value:
  // nx = 130, K = 3 gives 390)
  hipLaunchKernelGGL(lbm_av_velocity_kernel, dim3(blocks), dim3(kBlock), 0, c->stream,
                     c->grid[c->cur] + static_cast<size_t>(c->plan.ghost_rows) * c->p.nx, c->plan.ps,
                     c->mask, static_cast<size_t>(c->plan.ghost_rows) * c->p.nx, owned_cells(c), part, col_window(c));
  std::vector<double> host(blocks);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(host.data(), part, sizeof(double) * blocks, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  (void)hipFree(part);
  HIP_TRY(e);
  double s = 0.0;
  for (double v : host) s += v;
  *tot_u = s;
  return 0;
}

size_t lbm_halo_floats(const lbm_ctx* c) { return c ? static_cast<size_t>(3) * c->plan.nxp : 0; }
void* lbm_halo_send_ptr(lbm_ctx* c, int dir) { return (c && (dir == 0 || dir == 1)) ? c->send[dir] : nullptr; }
void* lbm_halo_recv_ptr(lbm_ctx* c, int dir) { return (c && (dir == 0 || dir == 1)) ? c->recv[dir] : nullptr; }

int lbm_bind_halo_buffers(lbm_ctx* c, void* send_south, void* send_north, void* recv_south, void* recv_north)
{
  if (!c || !send_south || !send_north || !recv_south || !recv_north) { lbm_internal::set_error("lbm_bind_halo_buffers: null argument"); return 1; }
  void* ptrs[4] = {send_south, send_north, recv_south, recv_north};
  for (void* q : ptrs)
    if (reinterpret_cast<uintptr_t>(q) % 16 != 0) { lbm_internal::set_error("lbm_bind_halo_buffers: buffers must be 16-byte aligned"); return 1; }
  c->send[0] = static_cast<float*>(send_south); c->send[1] = static_cast<float*>(send_north);
  c->recv[0] = static_cast<float*>(recv_south); c->recv[1] = static_cast<float*>(recv_north);
  return 0;
}

int lbm_step_prepare(lbm_ctx* c, int n_steps, void* stream)
{
  if (!c || n_steps < 0) { lbm_internal::set_error("lbm_step_prepare: bad argument"); return 1; }
  if (c->plan.ghost > 0) { lbm_internal::set_error("lbm_step_prepare: the context runs in K-step mode; use the lbm_macro_* calls"); return 1; }
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = pick_stream(c, stream);
  if (begin_run(c, n_steps, s)) return 1;
  const int nx = c->p.nx;
  hipLaunchKernelGGL(lbm_pack_halo_kernel, dim3((nx + 255) / 256), dim3(256), 0, s, c->grid[c->cur], c->plan.ps, nx, c->plan.nyl, c->plan.nxp,
                     c->send[0], c->send[1], c->release_sends ? 1 : 0);
  HIP_TRY(hipGetLastError());
  return 0;
}

int lbm_step_interior(lbm_ctx* c, void* stream)
{
  if (!c) { lbm_internal::set_error("lbm_step_interior: null context"); return 1; }
  if (c->run_done >= c->run_steps) { lbm_internal::set_error("lbm_step_interior: no steps left; call lbm_step_prepare"); return 1; }
  hipStream_t s = pick_stream(c, stream);
  const int qrow = c->p.nx / c->plan.lane_cells;
  StepArgs a = base_args(c, c->run_done + 1 < c->run_steps);
  a.quad_begin = qrow; a.quad_end = qrow * (c->plan.nyl - 1);
  a.quad_begin2 = a.quad_end2 = 0;
  a.iters = c->plan.iters_interior;
  a.partials_out = c->partials[c->parity];
  a.prev_partials = c->partials[c->parity ^ 1];
  a.n_prev = c->n_prev;
  if (c->plan.n_part_interior > 0) {
    launch_step(c, a, c->plan.n_part_interior, s);
    HIP_TRY(hipGetLastError());
    c->n_prev = 0;   // folded (by block 0 of this launch)
  }
  return 0;
}

int lbm_step_boundary(lbm_ctx* c, void* stream)
{
  if (!c) { lbm_internal::set_error("lbm_step_boundary: null context"); return 1; }
  if (c->run_done >= c->run_steps) { lbm_internal::set_error("lbm_step_boundary: no steps left; call lbm_step_prepare"); return 1; }
  hipStream_t s = pick_stream(c, stream);
  const int qrow = c->p.nx / c->plan.lane_cells;
  StepArgs a = base_args(c, c->run_done + 1 < c->run_steps);
  a.quad_begin = 0; a.quad_end = qrow;
  if (c->plan.nyl > 1) { a.quad_begin2 = qrow * (c->plan.nyl - 1); a.quad_end2 = qrow * c->plan.nyl; }
  a.iters = 1;
  a.south_halo = c->recv[0];
  a.north_halo = c->recv[1];
  a.send_south = c->send[0];
  a.send_north = c->send[1];
  a.release_sends = c->release_sends ? 1 : 0;
  a.partials_out = c->partials[c->parity] + c->plan.n_part_interior;
  a.prev_partials = c->partials[c->parity ^ 1];
  a.n_prev = c->n_prev;   // non-zero only when there was no interior launch to fold it
  launch_step(c, a, c->plan.n_part_boundary, s);
  HIP_TRY(hipGetLastError());
  return 0;
}

int lbm_step_finish(lbm_ctx* c, void* stream)
{
  if (!c) { lbm_internal::set_error("lbm_step_finish: null context"); return 1; }
  hipStream_t s = pick_stream(c, stream);
  after_launch(c, c->plan.n_part_interior + c->plan.n_part_boundary, 1, 1);
  if (c->run_done == c->run_steps) return end_run(c, c->run_steps * ((c->plan.n_part_interior > 0 ? 1 : 0) + 1), s);
  return 0;
}

// ---- K-step ("macro-step") stepping of a row-partitioned run ------------------------------------

int lbm_macro_steps(const lbm_ctx* c) { return (c && c->plan.ghost > 0) ? c->plan.multi_K : 0; }

size_t lbm_macro_halo_floats(const lbm_ctx* c) { return (c && c->plan.ghost > 0) ? static_cast<size_t>(c->plan.ghost) * c->p.nx : 0; }

void* lbm_macro_send_ptr(lbm_ctx* c, int dir, int plane)
{
  if (!c || c->plan.ghost == 0 || plane < 0 || plane >= 9 || (dir != 0 && dir != 1)) return nullptr;
  // first K owned rows go south, last K owned rows go north
  const size_t row = dir == 0 ? static_cast<size_t>(c->plan.ghost) : static_cast<size_t>(c->plan.nyl);
  return c->grid[c->cur] + plane * c->plan.ps + row * c->p.nx;
}

void* lbm_macro_recv_ptr(lbm_ctx* c, int dir, int plane)
{
  if (!c || c->plan.ghost == 0 || plane < 0 || plane >= 9 || (dir != 0 && dir != 1)) return nullptr;
  // ghost rows below the first owned row come from the south, those above the last one from the north
  const size_t row = dir == 0 ? 0 : static_cast<size_t>(c->plan.ghost + c->plan.nyl);
  return c->grid[c->cur] + plane * c->plan.ps + row * c->p.nx;
}

// Packed form of the exchange: 2 messages per direction instead of 18.
// (A column block — a tile rank that owns every row, ghost_rows == 0 — has no row exchange: 0 floats, and pack / unpack refuse.)
size_t lbm_macro_pack_floats(const lbm_ctx* c) { return (c && c->plan.ghost > 0 && c->plan.ghost_rows > 0) ? static_cast<size_t>(9) * c->plan.ghost * c->p.nx : 0; }

void* lbm_macro_pack_ptr(lbm_ctx* c, int dir, int incoming)
{
  if (!c || c->plan.ghost == 0 || c->plan.ghost_rows == 0 || (dir != 0 && dir != 1)) return nullptr;
  return c->macro_pack[incoming ? 1 : 0] + static_cast<size_t>(dir) * lbm_macro_pack_floats(c);
}

static int macro_pack_launch(lbm_ctx* c, bool unpack, hipStream_t s)
{
  const int nfloats = c->plan.ghost * c->p.nx;
  const dim3 grid((nfloats / 2 + 255) / 256, 9, 2);
  // outgoing: first K owned rows (dir 0, south) and last K owned rows (dir 1, north);
  // incoming: ghost rows below (from the south, dir 0) and above (from the north, dir 1)
  const size_t row_a = unpack ? 0 : static_cast<size_t>(c->plan.ghost);
  const size_t row_b = unpack ? static_cast<size_t>(c->plan.ghost + c->plan.nyl) : static_cast<size_t>(c->plan.nyl);
  hipLaunchKernelGGL(lbm_macro_pack_kernel, grid, dim3(256), 0, s, c->grid[c->cur], c->macro_pack[unpack ? 1 : 0], c->plan.ps, nfloats,
                     row_a, row_b, c->p.nx, unpack ? 1 : 0);
  HIP_TRY(hipGetLastError());
  return 0;
}

int lbm_macro_pack(lbm_ctx* c, void* stream)
{
  if (!c || c->plan.ghost == 0) { lbm_internal::set_error("lbm_macro_pack: not a K-step context"); return 1; }
  if (c->plan.ghost_rows == 0) { lbm_internal::set_error("lbm_macro_pack: a column block keeps no ghost rows (its rows wrap inside the launch): the column exchange is its whole exchange"); return 1; }
  return macro_pack_launch(c, false, pick_stream(c, stream));
}

int lbm_macro_unpack(lbm_ctx* c, void* stream)
{
  if (!c || c->plan.ghost == 0) { lbm_internal::set_error("lbm_macro_unpack: not a K-step context"); return 1; }
  if (c->plan.ghost_rows == 0) { lbm_internal::set_error("lbm_macro_unpack: a column block keeps no ghost rows (its rows wrap inside the launch): the column exchange is its whole exchange"); return 1; }
  return macro_pack_launch(c, true, pick_stream(c, stream));
}

// ---- the column half of a tile rank's packed exchange ----
size_t lbm_macro_pack_floats_x(const lbm_ctx* c) { return (c && c->plan.ghost > 0 && c->plan.ghost_x > 0) ? static_cast<size_t>(9) * c->plan.nyl * c->plan.ghost_x : 0; }

void* lbm_macro_pack_ptr_x(lbm_ctx* c, int dir, int incoming)
{
  if (!c || c->plan.ghost == 0 || c->plan.ghost_x == 0 || (dir != 0 && dir != 1)) return nullptr;
  return c->macro_pack_x[incoming ? 1 : 0] + static_cast<size_t>(dir) * lbm_macro_pack_floats_x(c);
}

static int macro_pack_cols_launch(lbm_ctx* c, bool unpack, hipStream_t s)
{
  const int gx = c->plan.ghost_x;
  MacroPackColsArgs a{};
  a.grid = c->grid[c->cur]; a.buf = c->macro_pack_x[unpack ? 1 : 0]; a.ps = c->plan.ps; a.w = c->p.nx;
  a.row0 = c->plan.ghost_rows; a.nrows = c->plan.nyl; a.gx = gx; a.unpack = unpack ? 1 : 0;
  // outgoing: the first ghost_x owned columns (dir 0, west) and the last (dir 1, east);
  // incoming: the ghost columns before the owned ones (from the west, dir 0) and after them (from the east, dir 1)
  a.col[0] = unpack ? 0 : gx;
  a.col[1] = unpack ? gx + c->plan.nxl : c->plan.nxl;
  if (18LL * c->plan.nyl * gx >= (1LL << 30)) { lbm_internal::set_error("lbm_macro_pack_x: column messages too large for the kernel's 32-bit indices"); return 1; }
  const lbm_internal::ColumnMessagePlan m = lbm_internal::plan_column_message(c->plan, gx, 4096, nullptr, 0);
  const dim3 grid(m.blocks);
  const int per = m.per;
  if (per == 4) hipLaunchKernelGGL(lbm_macro_pack_cols_kernel<f4>, grid, dim3(256), 0, s, a);
  else if (per == 2) hipLaunchKernelGGL(lbm_macro_pack_cols_kernel<f2>, grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL(lbm_macro_pack_cols_kernel<float>, grid, dim3(256), 0, s, a);
  HIP_TRY(hipGetLastError());
  return 0;
}

int lbm_macro_pack_x(lbm_ctx* c, void* stream)
{
  if (!c || c->plan.ghost == 0 || c->plan.ghost_x == 0) { lbm_internal::set_error("lbm_macro_pack_x: not a rank of the tile decomposition (row partitions exchange rows only: lbm_macro_pack)"); return 1; }
  return macro_pack_cols_launch(c, false, pick_stream(c, stream));
}

int lbm_macro_unpack_x(lbm_ctx* c, void* stream)
{
  if (!c || c->plan.ghost == 0 || c->plan.ghost_x == 0) { lbm_internal::set_error("lbm_macro_unpack_x: not a rank of the tile decomposition (row partitions exchange rows only: lbm_macro_unpack)"); return 1; }
  return macro_pack_cols_launch(c, true, pick_stream(c, stream));
}

// lbm_macro_prepare for a rank of the tile decomposition.  A call of its own: a caller that knows the row protocol only would exchange
// rows and never columns, so lbm_macro_prepare keeps refusing these contexts.
int lbm_tile_prepare(lbm_ctx* c, int n_steps, void* stream)
{
  if (!c || n_steps < 0 || c->plan.ghost == 0 || c->plan.ghost_x == 0) { lbm_internal::set_error("lbm_tile_prepare: not a rank of the tile decomposition (row partitions: lbm_macro_prepare)"); return 1; }
  HIP_TRY(hipSetDevice(c->device));
  return begin_run(c, n_steps, pick_stream(c, stream));
}

int lbm_macro_prepare(lbm_ctx* c, int n_steps, void* stream)
{
  if (!c || n_steps < 0 || c->plan.ghost == 0) { lbm_internal::set_error("lbm_macro_prepare: not a K-step context"); return 1; }
  if (c->plan.ghost_x > 0) { lbm_internal::set_error("lbm_macro_prepare: ranks of the tile decomposition are stepped by the peer-to-peer loop (lbm_p2p_run) only"); return 1; }
  HIP_TRY(hipSetDevice(c->device));
  return begin_run(c, n_steps, pick_stream(c, stream));
}

static GroupPlan macro_group(const lbm_ctx* c) { return lbm_internal::plan_group(c->plan, c->run_steps - c->run_done); }

int lbm_macro_next_steps(const lbm_ctx* c) { return (c && c->plan.ghost > 0 && c->run_done < c->run_steps) ? macro_group(c).total : 0; }
int lbm_macro_next_launches(const lbm_ctx* c) { return (c && c->plan.ghost > 0 && c->run_done < c->run_steps) ? macro_group(c).n : 0; }

// Launch i of a group over `which` of its tiles (lbm_plan.cpp plan_launch: all of them, those that read no exchanged cell, or the rest),
// and the launch itself: called by both native loops and by the split-phase entry points below.
static LaunchPlan group_launch_plan(const lbm_ctx* c, const GroupPlan& g, int i, int which)
{
  LaunchPlan l;
  lbm_internal::plan_launch(c->plan, c->knobs, g.k[i], g.ext(i), which, /*says_ready=*/c->ready_epoch != 0, &l);
  return l;
}
static void launch_group(lbm_ctx* c, const GroupPlan& g, int i, const LaunchPlan& l, bool more_after_group, hipStream_t s)
{
  launch_multi(c, l, /*accel_last=*/i + 1 < g.n || more_after_group, /*fold=*/c->n_prev > 0, s);
}
// state flip after launch i of a group, made as `launches` launches
static void group_launch_done(lbm_ctx* c, const GroupPlan& g, int i, const LaunchPlan& l, int launches)
{
  after_launch(c, l.ntiles_total, g.k[i], g.k[i]);
  c->ev_tile_launches += launches;
}

// The split-phase calls of a group's first launch: `which` of its tiles, if it has any; whichever of the launches of a macro-step comes
// first folds the previous launch's sums.
static int macro_launch(lbm_ctx* c, int which, void* stream, const char* not_k_step, const char* no_steps)
{
  if (!c || c->plan.ghost == 0) { lbm_internal::set_error(not_k_step); return 1; }
  if (c->run_done >= c->run_steps) { lbm_internal::set_error(no_steps); return 1; }
  const GroupPlan g = macro_group(c);
  const LaunchPlan l = group_launch_plan(c, g, 0, which);
  if (which == kLaunchInterior && l.nblocks == 0) return 0;   // no tile whose rings stay inside the owned cells
  launch_group(c, g, 0, l, c->run_done + g.total < c->run_steps, pick_stream(c, stream));
  HIP_TRY(hipGetLastError());
  c->n_prev = 0;   // folded by this launch's block 0
  return 0;
}

int lbm_macro_interior(lbm_ctx* c, void* stream)
{
  return macro_launch(c, kLaunchInterior, stream, "lbm_macro_interior: not a K-step context", "lbm_macro_interior: no steps left; call lbm_macro_prepare");
}

int lbm_macro_edge(lbm_ctx* c, void* stream)
{
  return macro_launch(c, kLaunchEdge, stream, "lbm_macro_edge: not a K-step context", "lbm_macro_edge: no steps left; call lbm_macro_prepare");
}

int lbm_macro_all(lbm_ctx* c, void* stream)
{
  return macro_launch(c, kLaunchWhole, stream, "lbm_macro_all: not a K-step context", "lbm_macro_all: no steps left; call lbm_macro_prepare");
}

int lbm_macro_finish(lbm_ctx* c, void* stream)
{
  if (!c || c->plan.ghost == 0) { lbm_internal::set_error("lbm_macro_finish: not a K-step context"); return 1; }
  if (c->run_done >= c->run_steps) { lbm_internal::set_error("lbm_macro_finish: no steps left; call lbm_macro_prepare"); return 1; }
  hipStream_t s = pick_stream(c, stream);
  const GroupPlan g = macro_group(c);
  const bool more = c->run_done + g.total < c->run_steps;
  group_launch_done(c, g, 0, group_launch_plan(c, g, 0, kLaunchWhole), 2);
  // the rest of the group: launches over all tiles that read the ghost rows the first one advanced — no exchange in between
  for (int i = 1; i < g.n; ++i) {
    const LaunchPlan l = group_launch_plan(c, g, i, kLaunchWhole);
    launch_group(c, g, i, l, more, s);
    HIP_TRY(hipGetLastError());
    group_launch_done(c, g, i, l, 1);
  }
  if (c->run_done == c->run_steps) return end_run(c, c->ev_tile_launches, s);
  return 0;
}

int lbm_macro_exchange_local(lbm_ctx* dst, lbm_ctx* src, int dir, void* stream)
{
  if (!dst || !src || dst->plan.ghost == 0 || src->plan.ghost != dst->plan.ghost || src->p.nx != dst->p.nx || (dir != 0 && dir != 1)) {
    lbm_internal::set_error("lbm_macro_exchange_local: incompatible contexts");
    return 1;
  }
  // src's rows travelling in direction `dir` land in dst's ghost rows on the opposite side
  hipStream_t s = pick_stream(dst, stream);
  const size_t bytes = sizeof(float) * lbm_macro_halo_floats(src);
  for (int k = 0; k < 9; ++k)
    HIP_TRY(hipMemcpyAsync(lbm_macro_recv_ptr(dst, dir ^ 1, k), lbm_macro_send_ptr(src, dir, k), bytes, hipMemcpyDeviceToDevice, s));
  return 0;
}

// Tile ranks of one process: src's packed message of direction `dir` into dst's incoming buffer of the opposite side, one device copy
// (between lbm_macro_pack_x / lbm_macro_pack on src and lbm_macro_unpack_x / lbm_macro_unpack on dst; dst == src: a rank that is its own neighbour).
int lbm_macro_exchange_local_x(lbm_ctx* dst, lbm_ctx* src, int dir, void* stream)
{
  if (!dst || !src || dst->plan.ghost_x == 0 || src->plan.ghost_x != dst->plan.ghost_x || src->plan.nyl != dst->plan.nyl || src->plan.ghost != dst->plan.ghost || (dir != 0 && dir != 1)) {
    lbm_internal::set_error("lbm_macro_exchange_local_x: incompatible contexts (two tile ranks of one rank-grid row, dir 0 or 1)");
    return 1;
  }
  HIP_TRY(hipMemcpyAsync(lbm_macro_pack_ptr_x(dst, dir ^ 1, 1), lbm_macro_pack_ptr_x(src, dir, 0), sizeof(float) * lbm_macro_pack_floats_x(src),
                         hipMemcpyDeviceToDevice, pick_stream(dst, stream)));
  return 0;
}

int lbm_macro_exchange_local_y(lbm_ctx* dst, lbm_ctx* src, int dir, void* stream)
{
  if (!dst || !src || dst->plan.ghost_x == 0 || dst->plan.ghost_rows == 0 || src->plan.ghost_rows != dst->plan.ghost_rows || src->plan.ghost_x != dst->plan.ghost_x || src->p.nx != dst->p.nx ||
      (dir != 0 && dir != 1)) {
    lbm_internal::set_error("lbm_macro_exchange_local_y: incompatible contexts (two tile ranks with ghost rows of one rank-grid column, dir 0 or 1)");
    return 1;
  }
  HIP_TRY(hipMemcpyAsync(lbm_macro_pack_ptr(dst, dir ^ 1, 1), lbm_macro_pack_ptr(src, dir, 0), sizeof(float) * lbm_macro_pack_floats(src),
                         hipMemcpyDeviceToDevice, pick_stream(dst, stream)));
  return 0;
}

int lbm_step_fold(lbm_ctx* c, void* stream)
{
  if (!c) { lbm_internal::set_error("lbm_step_fold: null context"); return 1; }
  return fold_last(c, pick_stream(c, stream));
}

int lbm_step_collect(lbm_ctx* c, void* stream, double* tot_u_per_step, int n_steps)
{
  if (!c || !tot_u_per_step || n_steps > c->run_done) { lbm_internal::set_error("lbm_step_collect: bad argument"); return 1; }
  hipStream_t s = pick_stream(c, stream);
  HIP_TRY(hipMemcpyAsync(tot_u_per_step, c->sums, sizeof(double) * n_steps, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return 0;
}

void* lbm_step_sums_device_ptr(lbm_ctx* c) { return c ? c->sums : nullptr; }

int lbm_last_run_kernel_ms(lbm_ctx* c, double* ms, int* launches)
{
  if (!c || !ms) { lbm_internal::set_error("lbm_last_run_kernel_ms: null argument"); return 1; }
  if (!c->ev_valid) { lbm_internal::set_error("lbm_last_run_kernel_ms: no completed run"); return 1; }
  float t = 0.f;
  HIP_TRY(hipEventSynchronize(c->ev_end));
  HIP_TRY(hipEventElapsedTime(&t, c->ev_begin, c->ev_end));
  *ms = t;
  if (launches) *launches = c->ev_launches;
  return 0;
}

int lbm_set_profile(lbm_ctx* c, int on)
{
  if (!c) { lbm_internal::set_error("lbm_set_profile: null context"); return 1; }
  c->prof.on = on != 0;
  if (!c->prof.on) c->prof_launches.clear();
  return 0;
}

int lbm_launch_profile(lbm_ctx* c, int cap, int* steps, double* us, int* n_launches)
{
  if (!c || !n_launches || cap < 0 || (cap > 0 && (!steps || !us))) { lbm_internal::set_error("lbm_launch_profile: bad argument"); return 1; }
  HIP_TRY(hipSetDevice(c->device));
  *n_launches = static_cast<int>(c->prof_launches.size());
  const int n = std::min(cap, *n_launches);
  for (int i = 0; i < n; ++i) {
    const lbm_ctx::ProfLaunch& l = c->prof_launches[i];
    float ms = 0.f;
    if (!l.begin || !l.end) { lbm_internal::set_error("lbm_launch_profile: a timing event could not be recorded"); return 1; }
    HIP_TRY(hipEventSynchronize(l.end));
    HIP_TRY(hipEventElapsedTime(&ms, l.begin, l.end));
    steps[i] = l.steps;
    us[i] = static_cast<double>(ms) * 1e3;
  }
  return 0;
}

int lbm_device(const lbm_ctx* c) { return c ? c->device : -1; }
void* lbm_stream(lbm_ctx* c) { return c ? c->stream : nullptr; }

int lbm_describe(const lbm_ctx* c, char* kernel_name, size_t len, long long* cells_per_launch, long long* state_bytes)
{
  if (!c) { lbm_internal::set_error("lbm_describe: null context"); return 1; }
  if (kernel_name && len) lbm_internal::plan_kernel_name(c->plan, kernel_name, len);
  if (cells_per_launch) *cells_per_launch = static_cast<long long>(c->plan.ncells);
  if (state_bytes) *state_bytes = static_cast<long long>(2 * 9 * c->plan.ncells * sizeof(float) + c->plan.ncells / 8);
  return 0;
}

}  // extern "C"

#if LBM_TILE_STAMPS
extern "C" int lbm_debug_tile_stamps(unsigned long long* out16)   // diagnostic builds only
{
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_tile_stamps), sizeof(unsigned long long) * 16));
  return 0;
}
#endif

#include "lbm_p2p_impl.h"   // peer-to-peer halo transport: drives the K-step launches above (include/lbm_d2q9_p2p.h)
