// lbm_rows64.hip — row-partitioned runs of the double-precision mode: the entry points of include/lbm_d2q9_f64_rows.h and, through
// kernels/rows64.h, their gfx950 kernels.  A translation unit of its own: the code objects of lbm_kernels.hip and lbm_f64.hip do not
// change with it.  What each rank gets is decided in lbm_plan.cpp (PlanRows64, lbm_internal.h); this unit allocates and launches by
// the plans.  A rank's device state and its read-outs are lbm_f64.hip's for a whole grid: the Slab64 of lbm_f64_slab.h.
//
// One lbm_rows64 holds every rank of a run and one host thread drives it.  Rank r owns the rows lbm_decompose gives it, on its device,
// as two grids of ny_local + 2 storage rows (kernels/rows64.h has the layout), with a stream of its own and two "pushed" events.
// A step of a rank is lbm_rows_kernel_f64 from grid A (the current one) into grid B, then lbm64_push_rows_kernel, which stores B's edge
// rows into the neighbours' ghost rows of THEIR grid B, then the record of the rank's pushed event of that step.
//
// THE ORDER, and why nothing else is needed.  lbm_rows64_run enqueues, after the accelerate pre-pass on the rank that owns row ny-2,
// one push of the CURRENT grid's edge rows by every rank ("push -1": every ghost row is then right whatever set_cells or an earlier
// run left), and then per step t, rank after rank: a hipStreamWaitEvent on both neighbours' pushed events of step t-1, kernel t, push
// t, the record of pushed[t & 1].  No kernel waits on the device, no flag, no spin.  With A the source and B the destination of step t:
//   - kernel t of rank r reads A's ghost rows: the neighbours' pushes t-1 wrote them, and kernel t waited for exactly those.
//   - push t of rank r writes the ghost rows of a neighbour's B.  The last reader of those was the neighbour's kernel t-1 (B was its
//     source).  Rank r's kernel t waited for that neighbour's push t-1, which follows the neighbour's kernel t-1 on its stream, and
//     push t follows kernel t on r's stream: the neighbour's kernel t-1 has finished.
//   - kernel t of rank r writes B's owned rows.  Their readers were r's own kernel t-1 and push t-2, earlier on the same stream; no
//     other rank ever reads them (the exchange is push only).  The neighbours' pushes t write B's ghost rows meanwhile: other rows.
//   - an event is recorded again two steps later; every wait on its earlier record was enqueued before that (the waits of step t+1
//     come before the records of step t+2 in this one host thread), and a wait refers to the record that was current when it was made.
//   - row ny-2, which the pre-pass and the kernels' epilogue accelerate, is an interior row of the last rank (at least 3 rows): no push
//     reads it.
// Every enqueued item depends only on items enqueued before it, so ranks that share a device (and its hardware queues) cannot block
// each other.  A run ends with every stream synchronised: the next call finds all ranks idle.
//
// av_vels[t]: each rank's sums[t] (folded as lbm64_run folds them) copied to the host and added there in rank order, times
// 1.0 / free_cells: one more serial level of the summation tree, nranks - 1 additions, the same bits in every run.
//
// SEVERAL STEPS PER EXCHANGE (LBM_ROWS64_FLAG_MULTI_STEPS or LBM_ROWS64_FLAG_MULTI_ANY_SIZE where PlanRowsMultiAny64.multi_kernel, the
// same on every rank; .edge, the same on every rank too: the kernel's edge-tile form, on ranks that may differ in rows, tiles and strides).  Rank r then keeps
// two grids of ny_local + 2 K storage rows (kernels/rows_multi64.h has the layout) and, beside the slab's bitfield of its owned rows,
// a WINDOW bitfield over all its storage rows.  A launch of a rank is lbm_rows_multi_kernel_f64, k <= K steps from grid A into grid B,
// then lbm64_push_ghost_rows_kernel, which stores all nine planes of B's first and last K owned rows into the neighbours' ghost rows of
// THEIR grid B, then the record of pushed[launch & 1].  THE ORDER is the one above with "launch" for "step" and K rows for one, and
// every item of it holds as it is written, for the same reasons — but the last:
//   - row ny-2 IS among the pushed rows now (one of the last rank's last two rows, nyl >= 16): rank 0's lower ghost rows hold a copy of
//     it.  The copy must be the accelerated row exactly when the owned row is.  Before launch 0 the pre-pass accelerates the owned row
//     on its rank's stream and push -1 follows it ON THE SAME STREAM; a launch that another step follows accelerates the row in its
//     epilogue (accel_last), and push t follows kernel t on the same stream; the last launch of a run does not, and neither does its
//     push send an accelerated row: the next run's pre-pass and push -1 do.  Inside a launch the kernel accelerates every copy of the
//     row (owned, ghost, ring: told by the whole grid's row index) between its sub-steps, as lbm_multi_kernel_f64 does.
// A launch of k steps consumes k of the K ghost rows on each side; the K rows pushed after it are whole again.  Degenerate rings: with
// one rank the rank is its own neighbour, with two both neighbours are the other rank; the rows a push reads (owned) and writes (ghost)
// are disjoint in both, because ny_local >= 16 > 2 K.  av_vels[t]: per rank lbm_multi_kernel_f64's tree over the rank's tiles (the
// last launch's vectors folded by lbm64_fold_kernel(..., n_tiles, k, ...)), then the same nranks - 1 host additions.  n_tiles is each
// rank's OWN count everywhere (the launch, n_prev of the next launch's fold block, the last fold): uneven ranks differ in it.
// The one-step path's code and launches are what they were.
//
// gfx950 only: 64-wide wavefronts (block_sum).

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "lbm_d2q9_f64_rows.h"
#include "lbm_d2q9_f64_digest.h"
#include "lbm_internal.h"
#include "lbm_knobs.h"
#include "kernels/rows64.h"
#include "kernels/rows_multi64.h"
#include "lbm_f64_slab.h"

namespace {

struct Rank64 {
  lbm_internal::PlanRows64 plan{};   // written once (lbm_plan.cpp plan64_rows)
  lbm_internal::PlanRowsMultiAny64 multi{};   // lbm_rows_multi_kernel_f64's part of it (plan64_rows_multi_any): written once; multi_kernel, edge and K are the same on every rank
  uint32_t* window_mask = nullptr;   // multi_kernel: the obstacle bitfield over ALL storage rows of the rank, bit c of the storage cell c
  Slab64 slab;                       // the rank's row block on its device (lbm_f64_slab.h): grid[g] is plane 0 STORAGE row 0, the owned cells start one row on (multi_kernel: K rows)
  hipEvent_t pushed[2] = {nullptr, nullptr}; // this rank's push of step t has finished: pushed[t & 1]
  std::vector<double> host_sums;
};

}  // namespace

struct lbm_rows64 {
  Knobs knobs;
  lbm64_params p{};
  int free_cells = 0;
  double free_cells_inv = 0.0;
  int nranks = 0;
  int cur = 0;                               // the current grid of EVERY rank
  double accel_w1 = 0.0, accel_w2 = 0.0;
  std::vector<Rank64> ranks;
  int current_device = -1;                   // of this call, once set
  int ev_launches = 0;
  bool ev_valid = false;
};

namespace {

using Rows64Kernel = void (*)(RowsStep64Args);
// every instantiation of the rank kernel, by [one cell per lane][non-temporal stores]
constexpr Rows64Kernel kRows64Kernels[2][2] = {
  {&lbm_rows_kernel_f64<kPairCells, false>, &lbm_rows_kernel_f64<kPairCells, true>},
  {&lbm_rows_kernel_f64<1, false>, &lbm_rows_kernel_f64<1, true>},
};

using RowsMulti64Kernel = void (*)(RowsMulti64Args);
using RowsMulti64EdgeKernel = void (*)(RowsMulti64EdgeArgs);
// every instantiation of the rank's multi-step kernel, by multi64_row(K, NT, FULL) (lbm_geometry.h, as kMulti64Kernels of lbm_f64.hip);
// and of its edge-tile form, which takes one argument more
#define LBM_ROWS_MULTI64_ROWS(K, EDGE) &lbm_rows_multi_kernel_f64<K, false, false, EDGE>, &lbm_rows_multi_kernel_f64<K, false, true, EDGE>, &lbm_rows_multi_kernel_f64<K, true, false, EDGE>, &lbm_rows_multi_kernel_f64<K, true, true, EDGE>
constexpr RowsMulti64Kernel kRowsMulti64Kernels[kMulti64Rows] = {LBM_ROWS_MULTI64_ROWS(2, false), LBM_ROWS_MULTI64_ROWS(3, false), LBM_ROWS_MULTI64_ROWS(4, false)};
constexpr RowsMulti64EdgeKernel kRowsMulti64EdgeKernels[kMulti64Rows] = {LBM_ROWS_MULTI64_ROWS(2, true), LBM_ROWS_MULTI64_ROWS(3, true), LBM_ROWS_MULTI64_ROWS(4, true)};
#undef LBM_ROWS_MULTI64_ROWS
static_assert(kMulti64MinK == 2 && kMulti64MaxK == 4 && multi64_row(2, false, true) == 1 && multi64_row(4, true, true) == 11, "the order of kRowsMulti64Kernels");
static_assert(multi64_lds_bytes(kMulti64MaxK) <= 65536, "no launch asks for more dynamic LDS than a kernel gets without hipFuncSetAttribute");

// hipSetDevice where the device changes: every launch, record and copy of a rank is made with its device current
int use_device(lbm_rows64* c, int device)
{
  if (c->current_device == device) return 0;
  HIP_TRY(hipSetDevice(device));
  c->current_device = device;
  return 0;
}

// Rank r's push of grid `g`: its edge rows into the ghost rows of the neighbours' grid `g`.
int enqueue_push(lbm_rows64* c, int r, int g)
{
  const Rank64& k = c->ranks[r];
  const Rank64& down = c->ranks[(r + c->nranks - 1) % c->nranks];
  const Rank64& up = c->ranks[(r + 1) % c->nranks];
  RowsPush64Args a{};
  a.grid = k.slab.grid[g];
  a.ps = k.slab.ps;
  a.nx = static_cast<uint32_t>(c->p.nx); a.nyl = static_cast<uint32_t>(k.plan.ny_local);
  a.down = down.slab.grid[g]; a.down_ps = down.slab.ps; a.down_nyl = static_cast<uint32_t>(down.plan.ny_local);
  a.up = up.slab.grid[g]; a.up_ps = up.slab.ps;
  const bool wide = k.plan.lane_cells == kPairCells;
  const unsigned accesses = 6u * (a.nx / (wide ? kPairCells : 1));
  const dim3 blocks((accesses + kBlock - 1) / kBlock);
  if (wide) lbm64_push_rows_kernel<true><<<blocks, dim3(kBlock), 0, k.slab.stream>>>(a);
  else lbm64_push_rows_kernel<false><<<blocks, dim3(kBlock), 0, k.slab.stream>>>(a);
  HIP_TRY(hipGetLastError());
  return 0;
}

// Rank r's push of grid `g` in the multi-step mode: its first and last K owned rows into the neighbours' ghost rows of their grid `g`.
int enqueue_push_ghost(lbm_rows64* c, int r, int g)
{
  const Rank64& k = c->ranks[r];
  const Rank64& down = c->ranks[(r + c->nranks - 1) % c->nranks];
  const Rank64& up = c->ranks[(r + 1) % c->nranks];
  RowsPushGhost64Args a{};
  a.grid = k.slab.grid[g];
  a.ps = k.slab.ps;
  a.nx = static_cast<uint32_t>(c->p.nx); a.nyl = static_cast<uint32_t>(k.plan.ny_local); a.ghost = static_cast<uint32_t>(k.multi.ghost);
  a.down = down.slab.grid[g]; a.down_ps = down.slab.ps; a.down_nyl = static_cast<uint32_t>(down.plan.ny_local);
  a.up = up.slab.grid[g]; a.up_ps = up.slab.ps;
  const unsigned accesses = a.ghost * (a.nx / kPairCells);               // of one plane and way
  lbm64_push_ghost_rows_kernel<<<dim3((accesses + kBlock - 1) / kBlock, 2 * 9), dim3(kBlock), 0, k.slab.stream>>>(a);
  HIP_TRY(hipGetLastError());
  return 0;
}

// The end of every run: all streams synchronised, then the ranks' per-step sums added on the host.
int finish_run(lbm_rows64* c, int n_steps, double* av_vels)
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

// lbm_rows64_run where every rank advances with lbm_rows_multi_kernel_f64: the unit's header has the order.
int run_multi(lbm_rows64* c, int n_steps, double* av_vels)
{
  const int nranks = c->nranks;
  const uint32_t nx = static_cast<uint32_t>(c->p.nx);
  {
    // accelerate_flow of the first step on the rank that owns row ny-2, on its stream BEFORE its push -1, which sends that row
    const Rank64& k = c->ranks[c->ranks[0].plan.accel_rank];
    const Slab64& s = k.slab;
    if (use_device(c, s.device)) return 1;
    hipLaunchKernelGGL(lbm64_accelerate_kernel, dim3((nx + 255) / 256), dim3(256), 0, s.stream, s.owned(c->cur), s.ps, s.mask, nx,
                       static_cast<uint32_t>(k.plan.accel_row), c->accel_w1, c->accel_w2);
    HIP_TRY(hipGetLastError());
  }
  for (int r = 0; r < nranks; ++r) {             // push -1 (all ranks are idle: the last call synchronised them)
    Rank64& k = c->ranks[r];
    if (use_device(c, k.slab.device)) return 1;
    if (enqueue_push_ghost(c, r, c->cur)) return 1;
    HIP_TRY(hipEventRecord(k.pushed[1], k.slab.stream));
  }
  int parity = 0, launches = 0, last_vecs = 0;
  for (int left = n_steps; left > 0; ++launches) {
    const int steps = lbm_internal::plan64_rows_multi_any_next_steps(c->ranks[0].multi, left);     // K is the same on every rank
    left -= steps;
    const int before = (launches + 1) & 1, now = launches & 1;     // the pushed events of launch - 1 and of this launch
    for (int r = 0; r < nranks; ++r) {
      Rank64& k = c->ranks[r];
      const Slab64& s = k.slab;
      const lbm_internal::PlanRowsMultiAny64& m = k.multi;
      const int down = (r + nranks - 1) % nranks, up = (r + 1) % nranks;
      if (use_device(c, s.device)) return 1;
      if (down != r) HIP_TRY(hipStreamWaitEvent(s.stream, c->ranks[down].pushed[before], 0));
      if (up != r && up != down) HIP_TRY(hipStreamWaitEvent(s.stream, c->ranks[up].pushed[before], 0));
      if (launches == 0) HIP_TRY(hipEventRecord(s.ev_begin, s.stream));
      RowsMulti64Args a{};
      a.src = s.grid[c->cur];
      a.dst = s.grid[c->cur ^ 1];
      a.mask = k.window_mask;
      a.ps = s.ps;
      a.nx = c->p.nx; a.ny = c->p.ny;
      a.ghost = m.ghost;
      a.row0 = k.plan.y0 - m.ghost;
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
      const dim3 blocks(m.n_tiles + 1), lanes(m.block);                     // + the fold block
      if (m.edge) {
        RowsMulti64EdgeArgs e{};
        static_cast<RowsMulti64Args&>(e) = a;
        e.last_y0 = m.last_y0;
        kRowsMulti64EdgeKernels[row]<<<blocks, lanes, static_cast<size_t>(m.lds_bytes), s.stream>>>(e);
      } else {
        kRowsMulti64Kernels[row]<<<blocks, lanes, static_cast<size_t>(m.lds_bytes), s.stream>>>(a);
      }
      HIP_TRY(hipGetLastError());
      if (enqueue_push_ghost(c, r, c->cur ^ 1)) return 1;
      HIP_TRY(hipEventRecord(k.pushed[now], s.stream));
    }
    last_vecs = steps;
    parity ^= 1;
    c->cur ^= 1;
  }
  for (int r = 0; r < nranks; ++r) {
    Rank64& k = c->ranks[r];
    const Slab64& s = k.slab;
    if (use_device(c, s.device)) return 1;
    HIP_TRY(hipEventRecord(s.ev_end, s.stream));
    hipLaunchKernelGGL(lbm64_fold_kernel, dim3(1), dim3(kBlock), 0, s.stream, s.partials[parity ^ 1], k.multi.n_tiles, last_vecs, s.sums, s.counter);
    HIP_TRY(hipGetLastError());
    if (av_vels) {
      k.host_sums.resize(static_cast<size_t>(n_steps));
      HIP_TRY(hipMemcpyAsync(k.host_sums.data(), s.sums, sizeof(double) * n_steps, hipMemcpyDeviceToHost, s.stream));
    }
  }
  c->ev_launches = launches * nranks;
  c->ev_valid = true;
  return 0;
}

// The whole grid's index of a rank's first owned cell.
size_t first_cell(const lbm_rows64* c, const Rank64& k) { return static_cast<size_t>(k.plan.y0) * c->p.nx; }

}  // namespace

extern "C" {

int lbm_rows64_abi_version(void) { return LBM_ROWS64_ABI_VERSION; }

int lbm_rows64_destroy(lbm_rows64* c)
{
  if (!c) return 0;
  for (Rank64& k : c->ranks) {                 // every stream first: a rank's last push stores into its neighbours' grids
    if (!k.slab.stream) continue;              // never reached its device
    (void)hipSetDevice(k.slab.device);
    (void)hipStreamSynchronize(k.slab.stream);
  }
  for (Rank64& k : c->ranks) {
    if (!k.slab.stream) continue;
    (void)hipSetDevice(k.slab.device);
    for (int i = 0; i < 2; ++i) if (k.pushed[i]) (void)hipEventDestroy(k.pushed[i]);
    if (k.window_mask) (void)hipFree(k.window_mask);
    slab64_destroy(k.slab);
  }
  delete c;
  return 0;
}

int lbm_rows64_create(lbm_rows64** out, const lbm64_params* p, int free_cells, const int* obstacles, int nranks, const int* devices, unsigned flags)
{
  if (!out || !p || !obstacles) { lbm_internal::set_error("lbm_rows64_create: null argument"); return 1; }
  *out = nullptr;
  const Knobs knobs = knobs_from_env();
  {
    lbm_internal::PlanRows64 first;
    if (lbm_internal::plan64_rows(knobs, p, nranks, 0, flags, &first)) return 1;      // every refusal that needs no device
  }
  if (free_cells <= 0) { lbm_internal::set_error("lbm_rows64_create: free_cells must be positive"); return 1; }
  lbm_rows64* c = new lbm_rows64();
  c->knobs = knobs;
  c->p = *p;
  c->free_cells = free_cells;
  c->free_cells_inv = 1.0 / free_cells;                                      // d2q9-bgk.c:950 in double
  c->nranks = nranks;
  c->accel_w1 = p->density * p->accel * 0.111111111111111111111111;         // d2q9-bgk.c:445
  c->accel_w2 = p->density * p->accel * 0.0277777777777777777777778;        // d2q9-bgk.c:446
  c->ranks.resize(static_cast<size_t>(nranks));
  auto fail = [&](void) { lbm_rows64_destroy(c); return 1; };
  for (int r = 0; r < nranks; ++r) {
    Rank64& k = c->ranks[r];
    if (lbm_internal::plan64_rows(knobs, p, nranks, r, flags, &k.plan)) return fail();
    lbm_internal::plan64_rows_multi_any(knobs, p, k.plan, &k.multi);
    const bool multi = k.multi.multi_kernel != 0;
    k.slab.ncells = static_cast<size_t>(p->nx) * k.plan.ny_local;
    k.slab.first = static_cast<size_t>(p->nx) * (multi ? k.multi.ghost : 1);      // the first owned row: storage row 1, or K
    k.slab.ps = static_cast<size_t>(multi ? k.multi.ps : k.plan.ps);
  }
  if (devices) {
    for (int r = 0; r < nranks; ++r) c->ranks[r].slab.device = devices[r];
  } else {
    int count = 0;
    HIP_TRY_OR(hipGetDeviceCount(&count), return fail());
    if (count < 1) { lbm_internal::set_error("lbm_rows64_create: no GPU"); return fail(); }
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
        lbm_internal::set_error("lbm_rows64_create: device " + std::to_string(from) + " cannot access device " + std::to_string(to) + " (hipDeviceCanAccessPeer): the ranks' edge rows travel as peer-to-peer stores");
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
  for (int r = 0; r < nranks; ++r) {
    Rank64& k = c->ranks[r];
    const lbm_internal::PlanRows64& plan = k.plan;
    HIP_TRY_OR(hipSetDevice(k.slab.device), return fail());
    const lbm_internal::PlanRowsMultiAny64& multi = k.multi;
    if (slab64_create(k.slab, static_cast<size_t>(multi.multi_kernel ? multi.grid_doubles : plan.grid_doubles), static_cast<size_t>(plan.mask_words),
                      static_cast<size_t>(std::max(plan.partials_cap, multi.multi_kernel ? multi.partials_cap : 0)), obstacles + first_cell(c, k), p->density, p->max_iters))
      return fail();
    if (multi.multi_kernel) {
      // the window bitfield: storage row i is row (y0 - K + i) mod ny of the whole grid
      std::vector<uint32_t> bits(static_cast<size_t>(multi.mask_words), 0u);
      const size_t nx = static_cast<size_t>(p->nx);
      for (int i = 0; i < plan.ny_local + 2 * multi.ghost; ++i) {
        const int* row = obstacles + static_cast<size_t>(((plan.y0 - multi.ghost + i) % p->ny + p->ny) % p->ny) * nx;
        for (size_t x = 0; x < nx; ++x) {
          const size_t cell = static_cast<size_t>(i) * nx + x;
          if (row[x]) bits[cell >> 5] |= 1u << (cell & 31);
        }
      }
      HIP_TRY_OR(hipMalloc(&k.window_mask, sizeof(uint32_t) * bits.size()), return fail());
      HIP_TRY_OR(hipMemcpy(k.window_mask, bits.data(), sizeof(uint32_t) * bits.size(), hipMemcpyHostToDevice), return fail());
    }
    for (int i = 0; i < 2; ++i) HIP_TRY_OR(hipEventCreateWithFlags(&k.pushed[i], hipEventDisableTiming), return fail());
  }
  for (int r = 0; r < nranks; ++r) {
    HIP_TRY_OR(hipSetDevice(c->ranks[r].slab.device), return fail());
    HIP_TRY_OR(hipStreamSynchronize(c->ranks[r].slab.stream), return fail());
  }
  *out = c;
  return 0;
}

int lbm_rows64_run(lbm_rows64* c, int n_steps, double* av_vels)
{
  if (!c) { lbm_internal::set_error("lbm_rows64_run: null run"); return 1; }
  if (n_steps < 0) { lbm_internal::set_error("lbm_rows64_run: negative step count"); return 1; }
  if (n_steps == 0) return 0;
  c->current_device = -1;
  const int nranks = c->nranks;
  const uint32_t nx = static_cast<uint32_t>(c->p.nx);
  for (Rank64& k : c->ranks) {
    if (use_device(c, k.slab.device)) return 1;
    if (slab64_ensure_sums(k.slab, n_steps, c->p.max_iters)) return 1;
  }
  if (c->ranks[0].multi.multi_kernel) {
    if (run_multi(c, n_steps, av_vels)) return 1;
    return finish_run(c, n_steps, av_vels);
  }
  {
    // accelerate_flow of the first step (d2q9-bgk.c:345-348) on the rank that owns row ny-2: every later one is the epilogue of the step before it
    const Rank64& k = c->ranks[c->ranks[0].plan.accel_rank];
    const Slab64& s = k.slab;
    if (use_device(c, s.device)) return 1;
    hipLaunchKernelGGL(lbm64_accelerate_kernel, dim3((nx + 255) / 256), dim3(256), 0, s.stream, s.owned(c->cur), s.ps, s.mask, nx,
                       static_cast<uint32_t>(k.plan.accel_row), c->accel_w1, c->accel_w2);
    HIP_TRY(hipGetLastError());
  }
  // push -1: the current grid's edge rows into the neighbours' ghost rows (all ranks are idle: the last call synchronised them)
  for (int r = 0; r < nranks; ++r) {
    Rank64& k = c->ranks[r];
    if (use_device(c, k.slab.device)) return 1;
    if (enqueue_push(c, r, c->cur)) return 1;
    HIP_TRY(hipEventRecord(k.pushed[1], k.slab.stream));
  }
  int parity = 0;
  for (int t = 0; t < n_steps; ++t) {
    const int before = (t + 1) & 1, now = t & 1;            // the pushed events of step t-1 and of step t
    for (int r = 0; r < nranks; ++r) {
      Rank64& k = c->ranks[r];
      const Slab64& s = k.slab;
      const lbm_internal::PlanRows64& plan = k.plan;
      const int down = (r + nranks - 1) % nranks, up = (r + 1) % nranks;
      if (use_device(c, s.device)) return 1;
      if (down != r) HIP_TRY(hipStreamWaitEvent(s.stream, c->ranks[down].pushed[before], 0));
      if (up != r && up != down) HIP_TRY(hipStreamWaitEvent(s.stream, c->ranks[up].pushed[before], 0));
      if (t == 0) HIP_TRY(hipEventRecord(s.ev_begin, s.stream));
      RowsStep64Args a{};
      a.src = s.grid[c->cur];
      a.dst = s.grid[c->cur ^ 1];
      a.mask = s.mask;
      a.ps = s.ps;
      a.nx = nx;
      a.units = plan.units;
      a.iters = plan.iters;
      a.omega = c->p.omega;
      a.accel_w1 = c->accel_w1; a.accel_w2 = c->accel_w2;
      a.accel_row = (r == plan.accel_rank && t + 1 < n_steps) ? plan.accel_row : -1;
      a.partials_out = s.partials[parity];
      a.prev_partials = s.partials[parity ^ 1];
      a.n_prev = t > 0 ? plan.blocks : 0;
      a.sums = s.sums;
      a.counter = s.counter;
      kRows64Kernels[plan.lane_cells == 1][plan.nt_stores]<<<dim3(plan.blocks + 1), dim3(kBlock), 0, s.stream>>>(a);   // + the fold block
      HIP_TRY(hipGetLastError());
      if (enqueue_push(c, r, c->cur ^ 1)) return 1;
      HIP_TRY(hipEventRecord(k.pushed[now], s.stream));
    }
    parity ^= 1;
    c->cur ^= 1;
  }
  for (int r = 0; r < nranks; ++r) {
    Rank64& k = c->ranks[r];
    const Slab64& s = k.slab;
    if (use_device(c, s.device)) return 1;
    HIP_TRY(hipEventRecord(s.ev_end, s.stream));
    hipLaunchKernelGGL(lbm64_fold_kernel, dim3(1), dim3(kBlock), 0, s.stream, s.partials[parity ^ 1], k.plan.blocks, 1, s.sums, s.counter);
    HIP_TRY(hipGetLastError());
    if (av_vels) {
      k.host_sums.resize(static_cast<size_t>(n_steps));
      HIP_TRY(hipMemcpyAsync(k.host_sums.data(), s.sums, sizeof(double) * n_steps, hipMemcpyDeviceToHost, s.stream));
    }
  }
  c->ev_launches = n_steps * nranks;
  c->ev_valid = true;
  return finish_run(c, n_steps, av_vels);
}

int lbm_rows64_get_cells(lbm_rows64* c, double* cells_aos)
{
  if (!c || !cells_aos) { lbm_internal::set_error("lbm_rows64_get_cells: null argument"); return 1; }
  c->current_device = -1;
  for (const Rank64& k : c->ranks) {
    if (use_device(c, k.slab.device)) return 1;
    if (slab64_get_cells(k.slab, c->cur, slab64_chunk_cells(k.slab, c->p.nx, c->knobs), cells_aos + 9 * first_cell(c, k))) return 1;
  }
  return 0;
}

int lbm_rows64_set_cells(lbm_rows64* c, const double* cells_aos)
{
  if (!c || !cells_aos) { lbm_internal::set_error("lbm_rows64_set_cells: null argument"); return 1; }
  c->current_device = -1;
  for (const Rank64& k : c->ranks) {
    if (use_device(c, k.slab.device)) return 1;
    if (slab64_set_cells(k.slab, c->cur, slab64_chunk_cells(k.slab, c->p.nx, c->knobs), cells_aos + 9 * first_cell(c, k))) return 1;
  }
  return 0;
}

int lbm_rows64_get_observables(lbm_rows64* c, double* obs)
{
  if (!c || !obs) { lbm_internal::set_error("lbm_rows64_get_observables: null argument"); return 1; }
  c->current_device = -1;
  for (const Rank64& k : c->ranks) {
    if (use_device(c, k.slab.device)) return 1;
    if (slab64_get_observables(k.slab, c->cur, slab64_chunk_cells(k.slab, c->p.nx, c->knobs), obs + 4 * first_cell(c, k))) return 1;
  }
  return 0;
}

int lbm_rows64_av_velocity_sum(lbm_rows64* c, double* tot_u)
{
  if (!c || !tot_u) { lbm_internal::set_error("lbm_rows64_av_velocity_sum: null argument"); return 1; }
  c->current_device = -1;
  double s = 0.0;
  for (const Rank64& k : c->ranks) {
    if (use_device(c, k.slab.device)) return 1;
    if (slab64_add_velocity_sum(k.slab, c->cur, &s)) return 1;        // the blocks' sums into the one accumulator, rank after rank
  }
  *tot_u = s;
  return 0;
}

int lbm_rows64_last_run_ms(lbm_rows64* c, double* ms, int* launches)
{
  if (!c || !ms) { lbm_internal::set_error("lbm_rows64_last_run_ms: null argument"); return 1; }
  if (!c->ev_valid) { lbm_internal::set_error("lbm_rows64_last_run_ms: no run yet"); return 1; }
  c->current_device = -1;
  double most = 0.0;
  for (const Rank64& k : c->ranks) {
    if (use_device(c, k.slab.device)) return 1;
    float t = 0.f;
    HIP_TRY(hipEventElapsedTime(&t, k.slab.ev_begin, k.slab.ev_end));
    most = std::max(most, static_cast<double>(t));
  }
  *ms = most;
  if (launches) *launches = c->ev_launches;
  return 0;
}

int lbm_rows64_describe(const lbm_rows64* c, char* kernel_name, size_t len, int* nranks, long long* blocks, long long* cells_per_block, long long* state_bytes)
{
  if (!c) { lbm_internal::set_error("lbm_rows64_describe: null run"); return 1; }
  if (c->ranks[0].multi.multi_kernel) {
    const Rank64* most = &c->ranks[0];
    long long bytes = 0;
    for (const Rank64& k : c->ranks) {
      if (k.multi.n_tiles > most->multi.n_tiles) most = &k;
      bytes += static_cast<long long>(2 * 9 * sizeof(double)) * c->p.nx * (k.plan.ny_local + 2 * k.multi.ghost);
    }
    if (kernel_name && len > 0) lbm_internal::plan64_rows_multi_any_kernel_name(most->multi, kernel_name, len);
    if (nranks) *nranks = c->nranks;
    if (blocks) *blocks = most->multi.n_tiles;
    if (cells_per_block) *cells_per_block = static_cast<long long>(kMulti64TX) * kMulti64TY;
    if (state_bytes) *state_bytes = bytes;
    return 0;
  }
  const Rank64* most = &c->ranks[0];
  long long bytes = 0;
  for (const Rank64& k : c->ranks) {
    if (k.plan.blocks > most->plan.blocks) most = &k;
    bytes += static_cast<long long>(2 * 9 * sizeof(double)) * c->p.nx * (k.plan.ny_local + 2);
  }
  if (kernel_name && len > 0) lbm_internal::plan64_rows_kernel_name(most->plan, kernel_name, len);
  if (nranks) *nranks = c->nranks;
  if (blocks) *blocks = most->plan.blocks;
  if (cells_per_block) *cells_per_block = static_cast<long long>(kBlock) * most->plan.iters * most->plan.lane_cells;
  if (state_bytes) *state_bytes = bytes;
  return 0;
}

// include/lbm_d2q9_f64_digest.h: one digest per row of the current grids.  Every rank that owns rows of [y_begin, y_end) digests its
// share on its device and stream (all ranks are idle: the last call synchronised them), every rank enqueued before any is waited for;
// the share of rank k lands at row_digests + (its first row of the range - y_begin).  A rank's first owned row is row plan.y0 of the
// whole grid and lies slab.first doubles into its storage (one ghost row, or K): slab.owned() skips them.  Leaves the run as it was:
// cur, the partials, the counters and the events of the last run are not touched.
int lbm_digest64_rows(lbm_rows64* c, int y_begin, int y_end, unsigned long long* row_digests, unsigned long long* digest)
{
  if (!c) { lbm_internal::set_error("lbm_digest64_rows: null run"); return 1; }
  if (!row_digests && !digest) { lbm_internal::set_error("lbm_digest64_rows: both output pointers are null"); return 1; }
  if (y_begin < 0 || y_end > c->p.ny || y_begin > y_end) { lbm_internal::set_error("lbm_digest64_rows: rows outside the grid (0 <= y_begin <= y_end <= ny)"); return 1; }
  const int rows = y_end - y_begin;
  if (rows == 0) { if (digest) *digest = 0; return 0; }
  std::vector<unsigned long long> own;
  if (!row_digests) { own.resize(static_cast<size_t>(rows)); row_digests = own.data(); }
  c->current_device = -1;
  const size_t nranks = c->ranks.size();
  std::vector<unsigned long long*> dev(nranks, nullptr);
  // the rows of the range that rank r owns: [lo, hi) of the whole grid
  auto share = [&](size_t r, int* lo, int* hi) {
    const lbm_internal::PlanRows64& plan = c->ranks[r].plan;
    *lo = std::max(y_begin, plan.y0);
    *hi = std::min(y_end, plan.y0 + plan.ny_local);
    return *lo < *hi;
  };
  int bad = 0, lo = 0, hi = 0;
  for (size_t r = 0; r < nranks && !bad; ++r) {
    if (!share(r, &lo, &hi)) continue;
    const Rank64& k = c->ranks[r];
    bad = use_device(c, k.slab.device) || slab64_enqueue_row_digests(k.slab, c->cur, c->p.nx, lo - k.plan.y0, hi - lo, lo, &dev[r]);
  }
  std::string first_error;
  if (bad) first_error = lbm_last_error();
  for (size_t r = 0; r < nranks; ++r) {          // every rank that got a device array, after a failure too: the array is freed here
    if (!dev[r] || !share(r, &lo, &hi)) continue;
    const Rank64& k = c->ranks[r];
    const int no_device = use_device(c, k.slab.device);
    if ((slab64_collect_row_digests(k.slab, dev[r], hi - lo, row_digests + (lo - y_begin)) || no_device) && !bad) {
      bad = 1;
      first_error = lbm_last_error();
    }
  }
  if (bad) { lbm_internal::set_error(first_error); return 1; }
  if (digest) *digest = slab64_digest_sum(row_digests, rows);
  return 0;
}

}  // extern "C"
