// lbm_cols64.hip — column-partitioned runs of the double-precision mode: the entry points of include/lbm_d2q9_f64_cols.h and, through
// kernels/cols64.h, their gfx950 kernels.  A translation unit of its own: the code objects of lbm_kernels.hip, lbm_f64.hip and
// lbm_rows64.hip do not change with it.  What each rank gets is decided in lbm_plan.cpp (PlanCols64, lbm_internal.h); this unit
// allocates and launches by that plan alone.
//
// One lbm_cols64 holds every rank of a run and one host thread drives it.  Rank r owns the columns lbm_decompose_columns gives it, on
// its device, as two grids of ny storage rows of pitch nxl + 2 G doubles (kernels/cols64.h has the layout), with a stream of its own and
// two "pushed" events.  A launch of a rank is lbm_cols_multi_kernel_f64, k <= K steps from grid A (the current one) into grid B, then
// lbm64_push_ghost_cols_kernel, which stores all nine planes of B's first and last G owned columns into the neighbours' ghost columns of
// THEIR grid B, then the record of pushed[launch & 1].
//
// THE ORDER is lbm_rows64.hip's with west and east in place of below and above.  lbm_cols64_run enqueues, after the accelerate
// pre-pass of every rank on its owned cells of row ny-2, one push of the CURRENT grid's edge columns by every rank on the same stream
// ("push -1": every ghost column is then right whatever create, set_cells or an earlier run left), and then per launch t, rank after
// rank: a hipStreamWaitEvent on both neighbours' pushed events of launch t-1, kernel t, push t, the record of pushed[t & 1].  No
// kernel waits on the device, no flag, no spin.  With A the source and B the destination of launch t:
//   - kernel t of rank r reads A's ghost columns: the neighbours' pushes t-1 wrote them, and kernel t waited for exactly those.
//   - push t of rank r writes the ghost columns of a neighbour's B.  The last reader of those was the neighbour's kernel t-1 (B was its
//     source).  Rank r's kernel t waited for that neighbour's push t-1, which follows the neighbour's kernel t-1 on its stream, and
//     push t follows kernel t on r's stream: the neighbour's kernel t-1 has finished.  The neighbour's kernel t reads A; its kernel
//     t+1, the next reader of B, waits for this push.  So a push into a neighbour's grid cannot meet that neighbour's launch reading
//     the same grid.
//   - kernel t of rank r writes B's owned columns.  Their readers were r's own kernel t-1 and push t-2, earlier on the same stream; no
//     other rank ever reads them (the exchange is push only).  The neighbours' pushes t write B's ghost columns meanwhile: other cells.
//   - an event is recorded again two launches later; every wait on its earlier record was enqueued before that (the waits of launch
//     t+1 come before the records of launch t+2 in this one host thread), and a wait refers to the record that was current when it
//     was made.
//   - row ny-2 crosses EVERY cut.  The copies of it in a rank's ghost columns must be the accelerated cells exactly when the owned
//     ones are.  Before launch 0 each rank's pre-pass accelerates its owned cells of the row and its push -1 follows ON THE SAME
//     STREAM; the pre-pass touches owned columns only, the neighbours' pushes -1 ghost columns only.  A launch that another step
//     follows accelerates the row in its epilogue (accel_last), and push t follows kernel t on the same stream; the last launch of a
//     run does not, and neither does its push send accelerated cells: the next run's pre-pass and push -1 do.  Inside a launch the
//     kernel accelerates every copy of the row (owned, ghost column, ring: told by the row index) between its sub-steps.
// Every enqueued item depends only on items enqueued before it, so ranks that share a device (and its hardware queues) cannot block
// each other.  A run ends with every stream synchronised: the next call finds all ranks idle.
// Degenerate rings: with one rank the rank is its own neighbour, with two both neighbours are the other rank; the columns a push reads
// (owned) and writes (ghost) are disjoint in both, because nxl >= 32 > 2 G.
//
// av_vels[t]: per rank lbm_multi_kernel_f64's tree over the rank's tiles (the last launch's vectors folded by lbm64_fold_kernel), copied
// to the host and added there in rank order, times 1.0 / free_cells: nranks - 1 additions, the same bits in every run.  n_tiles is each
// rank's OWN count everywhere (the launch, n_prev of the next launch's fold block, the last fold): uneven ranks differ in it.
//
// A rank's device state is the Slab64 of lbm_f64_slab.h with every STORAGE cell as a cell of the slab (first = 0, ncells = ny * pitch):
// slab64_create then builds the window bitfield from the window's obstacle map and puts the rest state on ghost columns too.  The
// slab's chunked copies and read-outs assume a pitch equal to the width; their counterparts for a block are below.
//
// gfx950 only: 64-wide wavefronts (block_sum).

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "lbm_d2q9_f64_cols.h"
#include "lbm_internal.h"
#include "lbm_knobs.h"
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"      // step64.h's pre-pass and the slab's copies and read-outs want a pitch equal to the width: not used here
#include "kernels/cols64.h"
#include "lbm_f64_slab.h"
#pragma clang diagnostic pop

namespace {

struct ColsRank64 {
  lbm_internal::PlanCols64 plan{};   // written once (lbm_plan.cpp plan64_cols)
  Slab64 slab;                       // grid[g] is plane 0 storage cell 0; slab.mask is the WINDOW bitfield over the storage cells
  hipEvent_t pushed[2] = {nullptr, nullptr}; // this rank's push of launch t has finished: pushed[t & 1]
  std::vector<double> host_sums;

  size_t owned0() const { return static_cast<size_t>(plan.ghost); }   // doubles from a storage row's first cell to its first owned one
};

}  // namespace

struct lbm_cols64 {
  Knobs knobs;
  lbm64_params p{};
  int free_cells = 0;
  double free_cells_inv = 0.0;
  int nranks = 0;
  int cur = 0;                               // the current grid of EVERY rank
  double accel_w1 = 0.0, accel_w2 = 0.0;
  std::vector<ColsRank64> ranks;
  int current_device = -1;                   // of this call, once set
  int ev_launches = 0;
  bool ev_valid = false;
};

namespace {

using ColsMulti64Kernel = void (*)(ColsMulti64Args);
// every instantiation of the rank's kernel, by [EDGE][multi64_row(K, NT, FULL)] (lbm_geometry.h, as kMulti64Kernels of lbm_f64.hip)
#define LBM_COLS_MULTI64_ROWS(K, EDGE) &lbm_cols_multi_kernel_f64<K, false, false, EDGE>, &lbm_cols_multi_kernel_f64<K, false, true, EDGE>, &lbm_cols_multi_kernel_f64<K, true, false, EDGE>, &lbm_cols_multi_kernel_f64<K, true, true, EDGE>
constexpr ColsMulti64Kernel kColsMulti64Kernels[2][kMulti64Rows] = {
  {LBM_COLS_MULTI64_ROWS(2, false), LBM_COLS_MULTI64_ROWS(3, false), LBM_COLS_MULTI64_ROWS(4, false)},
  {LBM_COLS_MULTI64_ROWS(2, true), LBM_COLS_MULTI64_ROWS(3, true), LBM_COLS_MULTI64_ROWS(4, true)},
};
#undef LBM_COLS_MULTI64_ROWS
static_assert(kMulti64MinK == 2 && kMulti64MaxK == 4 && multi64_row(2, false, true) == 1 && multi64_row(4, true, true) == 11, "the order of kColsMulti64Kernels");
static_assert(multi64_lds_bytes(kMulti64MaxK) <= 65536, "no launch asks for more dynamic LDS than a kernel gets without hipFuncSetAttribute");

// hipSetDevice where the device changes: every launch, record and copy of a rank is made with its device current
int use_device(lbm_cols64* c, int device)
{
  if (c->current_device == device) return 0;
  HIP_TRY(hipSetDevice(device));
  c->current_device = device;
  return 0;
}

// Rank r's push of grid `g`: its first and last G owned columns into the ghost columns of the neighbours' grid `g`.
int enqueue_push(lbm_cols64* c, int r, int g)
{
  const ColsRank64& k = c->ranks[r];
  const ColsRank64& west = c->ranks[(r + c->nranks - 1) % c->nranks];
  const ColsRank64& east = c->ranks[(r + 1) % c->nranks];
  ColsPushGhost64Args a{};
  a.grid = k.slab.grid[g];
  a.ps = k.slab.ps;
  a.pitch = static_cast<uint32_t>(k.plan.pitch); a.nxl = static_cast<uint32_t>(k.plan.nxl);
  a.ny = static_cast<uint32_t>(c->p.ny); a.ghost = static_cast<uint32_t>(k.plan.ghost);
  a.west = west.slab.grid[g]; a.west_ps = west.slab.ps;
  a.west_pitch = static_cast<uint32_t>(west.plan.pitch); a.west_nxl = static_cast<uint32_t>(west.plan.nxl);
  a.east = east.slab.grid[g]; a.east_ps = east.slab.ps; a.east_pitch = static_cast<uint32_t>(east.plan.pitch);
  const unsigned accesses = a.ny * (a.ghost / kPairCells);               // of one plane and way
  lbm64_push_ghost_cols_kernel<<<dim3((accesses + kBlock - 1) / kBlock, 2 * 9), dim3(kBlock), 0, k.slab.stream>>>(a);
  HIP_TRY(hipGetLastError());
  return 0;
}

// Rows of a rank's block that the chunked copies (cells, observables) move at a time: LBM_TUNE_OBS_CHUNK cells' worth, one at least.
int chunk_rows(const lbm_cols64* c, const ColsRank64& k)
{
  const long long rows = static_cast<long long>(std::max(c->knobs.obs_chunk_cells, 1)) / k.plan.nxl;
  return static_cast<int>(std::min<long long>(c->p.ny, std::max<long long>(1, rows)));
}

// The whole grid's index of a rank's first owned cell of row y.
size_t whole_cell(const lbm_cols64* c, const ColsRank64& k, int y) { return static_cast<size_t>(y) * c->p.nx + k.plan.x0; }

// The chunked copies between the owned cells of a rank's grid `g` and the WHOLE grid's array: `rows` rows at a time through a device
// buffer of rows * nxl cells, which a strided host copy (the whole grid's row is nx cells, the block's nxl) joins to the caller's array.
// `per` = doubles per cell there (9: AoS cells, 4: observables).
enum CopyWhat { kCopyGet, kCopySet, kCopyObs };
int copy_block(const lbm_cols64* c, const ColsRank64& k, int g, CopyWhat what, double* whole)
{
  const Slab64& s = k.slab;
  const size_t per = what == kCopyObs ? 4 : 9, nxl = static_cast<size_t>(k.plan.nxl), pitch = static_cast<size_t>(k.plan.pitch);
  const int rows = chunk_rows(c, k);
  double* tmp = nullptr;
  HIP_TRY(hipMalloc(&tmp, sizeof(double) * per * nxl * rows));
  hipError_t e = hipSuccess;
  const size_t whole_pitch = sizeof(double) * per * c->p.nx, block_pitch = sizeof(double) * per * nxl;
  for (int y = 0; y < c->p.ny && e == hipSuccess; y += rows) {
    const int nr = std::min(rows, c->p.ny - y);
    const size_t n = nxl * nr;
    double* base = s.grid[g] + static_cast<size_t>(y) * pitch + k.owned0();       // row y's first owned cell
    double* host = whole + per * whole_cell(c, k, y);
    if (what == kCopySet) {
      e = hipMemcpy2DAsync(tmp, block_pitch, host, whole_pitch, block_pitch, nr, hipMemcpyHostToDevice, s.stream);
      if (e == hipSuccess) {
        hipLaunchKernelGGL(lbm64_cols_aos_to_soa_kernel, dim3(static_cast<unsigned>((n * 9 + 255) / 256)), dim3(256), 0, s.stream,
                           reinterpret_cast<const unsigned long long*>(tmp), reinterpret_cast<unsigned long long*>(base), s.ps, pitch, nxl, n);
        e = hipGetLastError();
      }
    } else {
      if (what == kCopyGet)
        hipLaunchKernelGGL(lbm64_cols_soa_to_aos_kernel, dim3(static_cast<unsigned>((n * 9 + 255) / 256)), dim3(256), 0, s.stream,
                           reinterpret_cast<const unsigned long long*>(base), reinterpret_cast<unsigned long long*>(tmp), s.ps, pitch, nxl, n);
      else
        hipLaunchKernelGGL(lbm64_cols_observables_kernel, dim3(static_cast<unsigned>((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s.stream,
                           base, s.ps, pitch, nxl, n, tmp);
      e = hipGetLastError();
      if (e == hipSuccess) e = hipMemcpy2DAsync(host, whole_pitch, tmp, block_pitch, block_pitch, nr, hipMemcpyDeviceToHost, s.stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s.stream);
  }
  (void)hipFree(tmp);
  HIP_TRY(e);
  return 0;
}

// The end of every run: all streams synchronised, then the ranks' per-step sums added on the host.
int finish_run(lbm_cols64* c, int n_steps, double* av_vels)
{
  const int nranks = c->nranks;
  for (int r = 0; r < nranks; ++r) {
    const Slab64& s = c->ranks[r].slab;
    if (use_device(c, s.device)) return 1;
    HIP_TRY(hipStreamSynchronize(s.stream));
  }
  if (av_vels) {
    for (int t = 0; t < n_steps; ++t) {
      double s = c->ranks[0].host_sums[t];
      for (int r = 1; r < nranks; ++r) s += c->ranks[r].host_sums[t];        // rank order: nranks - 1 additions
      av_vels[t] = s * c->free_cells_inv;                                    // d2q9-bgk.c:367
    }
  }
  return 0;
}

}  // namespace

extern "C" {

int lbm_cols64_abi_version(void) { return LBM_COLS64_ABI_VERSION; }

int lbm_cols64_destroy(lbm_cols64* c)
{
  if (!c) return 0;
  for (ColsRank64& k : c->ranks) {             // every stream first: a rank's last push stores into its neighbours' grids
    if (!k.slab.stream) continue;              // never reached its device
    (void)hipSetDevice(k.slab.device);
    (void)hipStreamSynchronize(k.slab.stream);
  }
  for (ColsRank64& k : c->ranks) {
    if (!k.slab.stream) continue;
    (void)hipSetDevice(k.slab.device);
    for (int i = 0; i < 2; ++i) if (k.pushed[i]) (void)hipEventDestroy(k.pushed[i]);
    slab64_destroy(k.slab);
  }
  delete c;
  return 0;
}

int lbm_cols64_create(lbm_cols64** out, const lbm64_params* p, int free_cells, const int* obstacles, int nranks, const int* devices, unsigned flags)
{
  if (!out || !p || !obstacles) { lbm_internal::set_error("lbm_cols64_create: null argument"); return 1; }
  *out = nullptr;
  const Knobs knobs = knobs_from_env();
  {
    lbm_internal::PlanCols64 first;
    if (lbm_internal::plan64_cols(knobs, p, nranks, 0, flags, &first)) return 1;      // every refusal that needs no device
  }
  if (free_cells <= 0) { lbm_internal::set_error("lbm_cols64_create: free_cells must be positive"); return 1; }
  lbm_cols64* c = new lbm_cols64();
  c->knobs = knobs;
  c->p = *p;
  c->free_cells = free_cells;
  c->free_cells_inv = 1.0 / free_cells;                                      // d2q9-bgk.c:950 in double
  c->nranks = nranks;
  c->accel_w1 = p->density * p->accel * 0.111111111111111111111111;         // d2q9-bgk.c:445
  c->accel_w2 = p->density * p->accel * 0.0277777777777777777777778;        // d2q9-bgk.c:446
  c->ranks.resize(static_cast<size_t>(nranks));
  auto fail = [&](void) { lbm_cols64_destroy(c); return 1; };
  for (int r = 0; r < nranks; ++r) {
    ColsRank64& k = c->ranks[r];
    if (lbm_internal::plan64_cols(knobs, p, nranks, r, flags, &k.plan)) return fail();
    k.slab.ncells = static_cast<size_t>(k.plan.pitch) * p->ny;               // every storage cell: the slab's bitfield is the window's
    k.slab.first = 0;
    k.slab.ps = static_cast<size_t>(k.plan.ps);
  }
  if (devices) {
    for (int r = 0; r < nranks; ++r) c->ranks[r].slab.device = devices[r];
  } else {
    int count = 0;
    HIP_TRY_OR(hipGetDeviceCount(&count), return fail());
    if (count < 1) { lbm_internal::set_error("lbm_cols64_create: no GPU"); return fail(); }
    for (int r = 0; r < nranks; ++r) c->ranks[r].slab.device = r % count;
  }
  for (int r = 0; r < nranks; ++r) {
    const int device = c->ranks[r].slab.device;
    HIP_TRY_OR(hipSetDevice(device), return fail());
  }
  // neighbours on distinct devices store into each other's grids: peer access, both ways
  for (int r = 0; r < nranks; ++r) {
    const int a = c->ranks[r].slab.device, b = c->ranks[(r + 1) % nranks].slab.device;
    if (a == b) continue;
    for (int way = 0; way < 2; ++way) {
      const int from = way ? b : a, to = way ? a : b;
      int can = 0;
      HIP_TRY_OR(hipDeviceCanAccessPeer(&can, from, to), return fail());
      if (!can) {
        lbm_internal::set_error("lbm_cols64_create: device " + std::to_string(from) + " cannot access device " + std::to_string(to) + " (hipDeviceCanAccessPeer): the ranks' edge columns travel as peer-to-peer stores");
        return fail();
      }
      HIP_TRY_OR(hipSetDevice(from), return fail());
      const hipError_t e = hipDeviceEnablePeerAccess(to, 0);
      if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) {
        lbm_internal::set_error(std::string("hipDeviceEnablePeerAccess: ") + hipGetErrorString(e));
        return fail();
      }
      (void)hipGetLastError();
    }
  }
  std::vector<int> window;
  for (int r = 0; r < nranks; ++r) {
    ColsRank64& k = c->ranks[r];
    const lbm_internal::PlanCols64& plan = k.plan;
    HIP_TRY_OR(hipSetDevice(k.slab.device), return fail());
    // the window's obstacle map: storage column i is column (x0 - G + i) mod nx of the whole grid
    const size_t nx = static_cast<size_t>(p->nx), pitch = static_cast<size_t>(plan.pitch);
    window.resize(pitch * p->ny);
    for (int y = 0; y < p->ny; ++y) {
      const int* row = obstacles + static_cast<size_t>(y) * nx;
      int* to = window.data() + static_cast<size_t>(y) * pitch;
      for (int i = 0; i < plan.pitch; ++i) to[i] = row[((plan.x0 - plan.ghost + i) % p->nx + p->nx) % p->nx];
    }
    if (slab64_create(k.slab, static_cast<size_t>(plan.grid_doubles), static_cast<size_t>(plan.mask_words), static_cast<size_t>(plan.partials_cap), window.data(),
                      p->density, p->max_iters))
      return fail();
    for (int i = 0; i < 2; ++i) HIP_TRY_OR(hipEventCreateWithFlags(&k.pushed[i], hipEventDisableTiming), return fail());
  }
  for (int r = 0; r < nranks; ++r) {
    HIP_TRY_OR(hipSetDevice(c->ranks[r].slab.device), return fail());
    HIP_TRY_OR(hipStreamSynchronize(c->ranks[r].slab.stream), return fail());
  }
  *out = c;
  return 0;
}

int lbm_cols64_run(lbm_cols64* c, int n_steps, double* av_vels)
{
  if (!c) { lbm_internal::set_error("lbm_cols64_run: null run"); return 1; }
  if (n_steps < 0) { lbm_internal::set_error("lbm_cols64_run: negative step count"); return 1; }
  if (n_steps == 0) return 0;
  c->current_device = -1;
  const int nranks = c->nranks;
  for (ColsRank64& k : c->ranks) {
    if (use_device(c, k.slab.device)) return 1;
    if (slab64_ensure_sums(k.slab, n_steps, c->p.max_iters)) return 1;
  }
  // accelerate_flow of the first step on every rank's owned cells of row ny-2, then on the same stream push -1, which sends some of them
  // (all ranks are idle: the last call synchronised them)
  for (int r = 0; r < nranks; ++r) {
    ColsRank64& k = c->ranks[r];
    const Slab64& s = k.slab;
    if (use_device(c, s.device)) return 1;
    const uint32_t nxl = static_cast<uint32_t>(k.plan.nxl);
    const uint32_t first = static_cast<uint32_t>(c->p.ny - 2) * static_cast<uint32_t>(k.plan.pitch) + static_cast<uint32_t>(k.plan.ghost);
    hipLaunchKernelGGL(lbm64_cols_accelerate_kernel, dim3((nxl + 255) / 256), dim3(256), 0, s.stream, s.grid[c->cur], s.ps, s.mask, first, nxl,
                       c->accel_w1, c->accel_w2);
    HIP_TRY(hipGetLastError());
    if (enqueue_push(c, r, c->cur)) return 1;
    HIP_TRY(hipEventRecord(k.pushed[1], s.stream));
  }
  int parity = 0, launches = 0, last_vecs = 0;
  for (int left = n_steps; left > 0; ++launches) {
    const int steps = lbm_internal::plan64_cols_next_steps(c->ranks[0].plan, left);     // K is the same on every rank
    left -= steps;
    const int before = (launches + 1) & 1, now = launches & 1;     // the pushed events of launch - 1 and of this launch
    for (int r = 0; r < nranks; ++r) {
      ColsRank64& k = c->ranks[r];
      const Slab64& s = k.slab;
      const lbm_internal::PlanCols64& m = k.plan;
      const int west = (r + nranks - 1) % nranks, east = (r + 1) % nranks;
      if (use_device(c, s.device)) return 1;
      if (west != r) HIP_TRY(hipStreamWaitEvent(s.stream, c->ranks[west].pushed[before], 0));
      if (east != r && east != west) HIP_TRY(hipStreamWaitEvent(s.stream, c->ranks[east].pushed[before], 0));
      if (launches == 0) HIP_TRY(hipEventRecord(s.ev_begin, s.stream));
      ColsMulti64Args a{};
      a.src = s.grid[c->cur];
      a.dst = s.grid[c->cur ^ 1];
      a.mask = s.mask;
      a.ps = s.ps;
      a.nxl = m.nxl; a.ny = c->p.ny;
      a.pitch = m.pitch;
      a.ghost = m.ghost;
      a.tiles_x = m.tiles_x;
      a.ksteps = steps;
      a.omega = c->p.omega;
      a.accel_w1 = c->accel_w1; a.accel_w2 = c->accel_w2;
      a.accel_row = c->p.ny - 2;
      a.accel_last = left > 0;
      a.partials_out = s.partials[parity];
      a.prev_partials = s.partials[parity ^ 1];
      a.n_prev = m.n_tiles; a.n_prev_vecs = last_vecs;                 // this rank's own tiles: the previous launch wrote that many per step
      a.sums = s.sums;
      a.counter = s.counter;
      const int row = multi64_row(m.K, m.nt_stores != 0, steps == m.K);
      kColsMulti64Kernels[m.edge != 0][row]<<<dim3(m.n_tiles + 1), dim3(m.block), static_cast<size_t>(m.lds_bytes), s.stream>>>(a);   // + the fold block
      HIP_TRY(hipGetLastError());
      if (enqueue_push(c, r, c->cur ^ 1)) return 1;
      HIP_TRY(hipEventRecord(k.pushed[now], s.stream));
    }
    last_vecs = steps;
    parity ^= 1;
    c->cur ^= 1;
  }
  for (int r = 0; r < nranks; ++r) {
    ColsRank64& k = c->ranks[r];
    const Slab64& s = k.slab;
    if (use_device(c, s.device)) return 1;
    HIP_TRY(hipEventRecord(s.ev_end, s.stream));
    hipLaunchKernelGGL(lbm64_fold_kernel, dim3(1), dim3(kBlock), 0, s.stream, s.partials[parity ^ 1], k.plan.n_tiles, last_vecs, s.sums, s.counter);
    HIP_TRY(hipGetLastError());
    if (av_vels) {
      k.host_sums.resize(static_cast<size_t>(n_steps));
      HIP_TRY(hipMemcpyAsync(k.host_sums.data(), s.sums, sizeof(double) * n_steps, hipMemcpyDeviceToHost, s.stream));
    }
  }
  c->ev_launches = launches * nranks;
  c->ev_valid = true;
  return finish_run(c, n_steps, av_vels);
}

int lbm_cols64_get_cells(lbm_cols64* c, double* cells_aos)
{
  if (!c || !cells_aos) { lbm_internal::set_error("lbm_cols64_get_cells: null argument"); return 1; }
  c->current_device = -1;
  for (const ColsRank64& k : c->ranks) {
    if (use_device(c, k.slab.device)) return 1;
    if (copy_block(c, k, c->cur, kCopyGet, cells_aos)) return 1;
  }
  return 0;
}

int lbm_cols64_set_cells(lbm_cols64* c, const double* cells_aos)
{
  if (!c || !cells_aos) { lbm_internal::set_error("lbm_cols64_set_cells: null argument"); return 1; }
  c->current_device = -1;
  for (const ColsRank64& k : c->ranks) {
    if (use_device(c, k.slab.device)) return 1;
    if (copy_block(c, k, c->cur, kCopySet, const_cast<double*>(cells_aos))) return 1;     // kCopySet reads the array only
  }
  return 0;
}

int lbm_cols64_get_observables(lbm_cols64* c, double* obs)
{
  if (!c || !obs) { lbm_internal::set_error("lbm_cols64_get_observables: null argument"); return 1; }
  c->current_device = -1;
  for (const ColsRank64& k : c->ranks) {
    if (use_device(c, k.slab.device)) return 1;
    if (copy_block(c, k, c->cur, kCopyObs, obs)) return 1;
  }
  return 0;
}

int lbm_cols64_av_velocity_sum(lbm_cols64* c, double* tot_u)
{
  if (!c || !tot_u) { lbm_internal::set_error("lbm_cols64_av_velocity_sum: null argument"); return 1; }
  c->current_device = -1;
  double total = 0.0;
  for (const ColsRank64& k : c->ranks) {
    const Slab64& s = k.slab;
    if (use_device(c, s.device)) return 1;
    const size_t ncells = static_cast<size_t>(k.plan.nxl) * c->p.ny;
    const int blocks = static_cast<int>(std::min<size_t>((ncells + kBlock - 1) / kBlock, 1024));
    double* part = nullptr;
    HIP_TRY(hipMalloc(&part, sizeof(double) * blocks));
    hipLaunchKernelGGL(lbm64_cols_av_velocity_kernel, dim3(blocks), dim3(kBlock), 0, s.stream, s.grid[c->cur], s.ps, s.mask, static_cast<size_t>(k.plan.pitch),
                       k.owned0(), static_cast<size_t>(k.plan.nxl), ncells, part);
    std::vector<double> host(blocks);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(host.data(), part, sizeof(double) * blocks, hipMemcpyDeviceToHost, s.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(s.stream);
    (void)hipFree(part);
    HIP_TRY(e);
    for (double v : host) total += v;          // the blocks' sums into the one accumulator, rank after rank
  }
  *tot_u = total;
  return 0;
}

int lbm_cols64_last_run_ms(lbm_cols64* c, double* ms, int* launches)
{
  if (!c || !ms) { lbm_internal::set_error("lbm_cols64_last_run_ms: null argument"); return 1; }
  if (!c->ev_valid) { lbm_internal::set_error("lbm_cols64_last_run_ms: no run yet"); return 1; }
  c->current_device = -1;
  double most = 0.0;
  for (const ColsRank64& k : c->ranks) {
    if (use_device(c, k.slab.device)) return 1;
    float t = 0.f;
    HIP_TRY(hipEventElapsedTime(&t, k.slab.ev_begin, k.slab.ev_end));
    most = std::max(most, static_cast<double>(t));
  }
  *ms = most;
  if (launches) *launches = c->ev_launches;
  return 0;
}

int lbm_cols64_describe(const lbm_cols64* c, char* kernel_name, size_t len, int* nranks, long long* blocks, long long* cells_per_block, long long* state_bytes)
{
  if (!c) { lbm_internal::set_error("lbm_cols64_describe: null run"); return 1; }
  const ColsRank64* most = &c->ranks[0];
  long long bytes = 0;
  for (const ColsRank64& k : c->ranks) {
    if (k.plan.n_tiles > most->plan.n_tiles) most = &k;
    bytes += static_cast<long long>(2 * 9 * sizeof(double)) * c->p.ny * k.plan.pitch;
  }
  if (kernel_name && len > 0) lbm_internal::plan64_cols_kernel_name(most->plan, kernel_name, len);
  if (nranks) *nranks = c->nranks;
  if (blocks) *blocks = most->plan.n_tiles;
  if (cells_per_block) *cells_per_block = static_cast<long long>(kMulti64TX) * kMulti64TY;
  if (state_bytes) *state_bytes = bytes;
  return 0;
}

// One digest per row of the current grids (include/lbm_d2q9_f64_digest.h).  Every rank digests its columns of the rows [y_begin, y_end)
// on its device and stream (all ranks are idle: the last call synchronised them), every rank enqueued before any is waited for; the
// host adds the ranks' parts of a row, wrap-around: the row's digest is by definition the wrap-around sum of its cells' terms, and the
// ranks' columns are a disjoint split of them.  Leaves the run as it was: cur, the partials, the counters and the events of the last run
// are not touched.
int lbm_cols64_digest(lbm_cols64* c, int y_begin, int y_end, unsigned long long* row_digests, unsigned long long* digest)
{
  if (!c) { lbm_internal::set_error("lbm_cols64_digest: null run"); return 1; }
  if (!row_digests && !digest) { lbm_internal::set_error("lbm_cols64_digest: both output pointers are null"); return 1; }
  if (y_begin < 0 || y_end > c->p.ny || y_begin > y_end) { lbm_internal::set_error("lbm_cols64_digest: rows outside the grid (0 <= y_begin <= y_end <= ny)"); return 1; }
  const int rows = y_end - y_begin;
  if (rows == 0) { if (digest) *digest = 0; return 0; }
  std::vector<unsigned long long> own;
  if (!row_digests) { own.resize(static_cast<size_t>(rows)); row_digests = own.data(); }
  c->current_device = -1;
  const size_t nranks = c->ranks.size();
  std::vector<unsigned long long*> dev(nranks, nullptr);
  int bad = 0;
  for (size_t r = 0; r < nranks && !bad; ++r) {
    const ColsRank64& k = c->ranks[r];
    const Slab64& s = k.slab;
    bad = use_device(c, s.device);
    if (bad) break;
    const hipError_t e = hipMalloc(&dev[r], sizeof(unsigned long long) * static_cast<size_t>(rows));
    if (e != hipSuccess) { lbm_internal::set_error(std::string("hipMalloc: ") + hipGetErrorString(e)); dev[r] = nullptr; bad = 1; break; }
    const double* base = s.grid[c->cur] + static_cast<size_t>(y_begin) * k.plan.pitch + k.owned0();
    hipLaunchKernelGGL(lbm64_cols_row_digest_kernel, dim3(static_cast<unsigned>(rows)), dim3(kBlock), 0, s.stream, reinterpret_cast<const unsigned long long*>(base), s.ps,
                       static_cast<size_t>(k.plan.pitch), static_cast<uint32_t>(k.plan.nxl), static_cast<uint32_t>(c->p.nx), static_cast<uint32_t>(k.plan.x0),
                       static_cast<unsigned long long>(y_begin), dev[r]);
    const hipError_t l = hipGetLastError();
    if (l != hipSuccess) { lbm_internal::set_error(std::string("lbm64_cols_row_digest_kernel: ") + hipGetErrorString(l)); bad = 1; }
  }
  std::string first_error;
  if (bad) first_error = lbm_last_error();
  std::vector<unsigned long long> part(static_cast<size_t>(rows));
  std::fill(row_digests, row_digests + rows, 0ull);
  for (size_t r = 0; r < nranks; ++r) {          // every rank that got a device array, after a failure too: the array is freed here
    if (!dev[r]) continue;
    const ColsRank64& k = c->ranks[r];
    const int no_device = use_device(c, k.slab.device);
    if ((slab64_collect_row_digests(k.slab, dev[r], rows, part.data()) || no_device) && !bad) {
      bad = 1;
      first_error = lbm_last_error();
    }
    if (!bad) for (int i = 0; i < rows; ++i) row_digests[i] += part[static_cast<size_t>(i)];      // wrap-around, rank after rank
  }
  if (bad) { lbm_internal::set_error(first_error); return 1; }
  if (digest) *digest = slab64_digest_sum(row_digests, rows);
  return 0;
}

}  // extern "C"
