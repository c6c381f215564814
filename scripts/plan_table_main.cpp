// plan_table_main.cpp — the planning unit under the host sanitizers: the three plan functions over the table of tests/plan_cases.py and
// over the refusals, printed one line per context, and under each context every launch of its runs of 11 and 20 steps, both schedules
// (lbm_plan_run_launches), one line per launch; then the row blocks of the double-precision mode (lbm_plan64_rows), one line per rank, and under LBM_ROWS64_FLAG_MULTI_STEPS their multi-step plans (lbm_plan64_rows_multi) with the launches of a run of 11 steps.  Host-only code, no GPU and no Python (of lbm_host.cpp the planner needs set_error and
// the two decompositions only):
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -I include -I mpilattice-boltzmann_amd/csrc
//       scripts/plan_table_main.cpp mpilattice-boltzmann_amd/csrc/lbm_plan.cpp mpilattice-boltzmann_amd/csrc/lbm_host.cpp -pthread -o plan_table && ./plan_table
#include <cstdio>

#include <cstdlib>

#include "lbm_d2q9.h"
#include "lbm_d2q9_f64_rows.h"
#include "lbm_internal.h"

static int shown = 0, launches = 0;
static void show(const char* what, int nx, int ny, int rc, const lbm_internal::ContextPlan& plan)
{
  char name[256] = "";
  if (rc == 0) lbm_plan_kernel_name(&plan, name, sizeof name);
  std::printf("%-5s %6d x %-6d %s\n", what, nx, ny, rc == 0 ? name : lbm_last_error());
  ++shown;
  if (rc != 0) return;
  static lbm_internal::LaunchPlan l[64];
  for (int steps : {11, 20})
    for (int schedule : {kScheduleSerial, kScheduleEdge}) {
      const int n = lbm_plan_run_launches(&plan, steps, schedule, l, 64);
      for (int i = 0; i < n && i < 64; ++i, ++launches)
        std::printf("  %2d steps %s  k %d ext %2d  rows %d+%d of %d  keep [%d, %d)  tiles %d+%d @%d,%d / %d rects of %d  blocks %d -> %d  remap %d  part %d row %d lanes %d\n",
                    steps, schedule == kScheduleEdge ? "edge  " : "serial", l[i].k, l[i].ext, l[i].row_first, l[i].rows_compute, l[i].rows_storage, l[i].keep_x0, l[i].keep_x1,
                    l[i].tile_count, l[i].tile_count2, l[i].tile_begin, l[i].tile_begin2, l[i].nrect, l[i].ntiles_total, l[i].nblocks, l[i].launched_blocks, l[i].xcd_remap,
                    l[i].part, l[i].row, l[i].lanes);
      if (schedule == kScheduleSerial && plan.ghost == 0) break;      // lbm_run has one schedule
    }
}

int main()
{
  const int whole[][2] = {{128, 128}, {128, 256}, {256, 256}, {512, 256}, {512, 512}, {768, 768}, {1024, 1024}, {2048, 2048}, {64, 16}, {130, 100},
                          {100, 100}, {127, 64}, {96, 2048}, {100, 40000}, {65536, 40000}, {1, 3}, {0, 0}};
  const unsigned flags[] = {0, LBM_FLAG_FAST_AVVELS, LBM_FLAG_EXACT_AVVELS, LBM_FLAG_FUSED_ARITH, LBM_FLAG_ONE_STEP, LBM_FLAG_NT_STORES, LBM_FLAG_KERNEL_LDS,
                            LBM_FLAG_FUSED_ARITH | LBM_FLAG_FAST_AVVELS, LBM_FLAG_GRAPH};
  lbm_internal::ContextPlan plan;
  for (const auto& g : whole)
    for (unsigned f : flags) {
      const lbm_params p{g[0], g[1], 11, 10, 0.1f, 0.005f, 1.85f};
      show("whole", g[0], g[1], lbm_plan_whole(&p, 1000, 0, g[1], f, 0, &plan), plan);
      if (g[1] > 40) show("part", g[0], g[1], lbm_plan_whole(&p, 1000, 3, g[1] - 7, f, 1, &plan), plan);     // lbm_create_global's rows [3, ny - 4)
    }
  const int rings[][2] = {{1024, 128}, {1024, 64}, {1024, 31}, {2048, 1024}, {64, 2}};
  for (const auto& g : rings)
    for (int nranks : {1, 2, 8}) {
      const lbm_params p{g[0], g[1], 11, 10, 0.1f, 0.005f, 1.85f};
      for (int r = 0; r < nranks; ++r) show("rank", g[0], g[1], lbm_plan_rank(&p, 1000, nranks, r, LBM_FLAG_FORCE_HALO, &plan), plan);
    }
  const int tiles[][4] = {{512, 512, 1, 1}, {512, 512, 2, 1}, {1024, 512, 2, 2}, {8192, 128, 8, 1}, {100, 100, 2, 2}};
  for (const auto& t : tiles) {
    const lbm_params p{t[0], t[1], 11, 10, 0.1f, 0.005f, 1.85f};
    for (int r = 0; r < t[2] * t[3]; ++r) show("tile", t[0], t[1], lbm_plan_tile(&p, 1000, t[2], t[3], r, 0, &plan), plan);
  }
  show("null", 0, 0, lbm_plan_whole(nullptr, 1, 0, 1, 0, 0, &plan), plan);
  // the row blocks of the double-precision mode (plan64_rows): every rank of the shapes tests/test_f64_rows.py runs, and the refusals
  const int rows[][3] = {{1, 3, 1}, {2, 6, 3}, {7, 5, 2}, {32, 16, 5}, {64, 48, 8}, {258, 33, 4}, {8192, 8192, 8}, {8, 5, 3}, {8, 3, 3}, {8, 16, 0}, {8, 16, 65}, {0, 16, 2}, {65536, 32768, 2}};
  for (const auto& g : rows)
    for (unsigned f : {0u, unsigned(LBM_FLAG_NT_STORES), unsigned(LBM64_FLAG_MULTI_STEPS), unsigned(LBM_FLAG_FUSED_ARITH)}) {
      const lbm64_params p{g[0], g[1], 11, 10, 0.1, 0.005, 1.85};
      for (int r = 0; r < (g[2] > 0 && g[2] <= 64 ? g[2] : 1); ++r, ++shown) {
        lbm_internal::PlanRows64 q;
        char name[64] = "";
        const int rc = lbm_plan64_rows(&p, g[2], r, f, &q);
        if (rc == 0) lbm_plan64_rows_kernel_name(&q, name, sizeof name);
        if (rc == 0) std::printf("rows  %6d x %-6d rank %d of %d: rows %d + %d, %s, %u units in %d blocks x %d, ps %lld\n", g[0], g[1], r, g[2], q.y0, q.ny_local, name, q.units, q.blocks, q.iters, q.ps);
        else std::printf("rows  %6d x %-6d rank %d of %d: %s\n", g[0], g[1], r, g[2], lbm_last_error());
      }
    }
  // ... and their multi-step plans (plan64_rows_multi): the shapes tests/test_plan64_rows_multi.py checks, eligible and not, at the
  // default minimum size and with it lowered to 0, every built K; under each eligible rank 0 the launches of a run of 11 steps
  const int multi[][3] = {{32, 16, 1}, {32, 32, 2}, {64, 48, 3}, {1024, 1024, 8}, {8192, 8192, 8}, {8, 16, 2}, {30, 32, 2}, {32, 48, 2}, {32, 33, 2}, {32, 32, 0}};
  for (const char* minimum : {"", "0"})
    for (const char* k : {"", "2", "3", "4"}) {
      if (*minimum) setenv("LBM_TUNE_MULTI64_MIN", minimum, 1); else unsetenv("LBM_TUNE_MULTI64_MIN");
      if (*k) setenv("LBM_TUNE_MULTI64_K", k, 1); else unsetenv("LBM_TUNE_MULTI64_K");
      for (const auto& g : multi)
        for (unsigned f : {unsigned(LBM_ROWS64_FLAG_MULTI_STEPS), unsigned(LBM_ROWS64_FLAG_MULTI_STEPS | LBM_FLAG_NT_STORES), unsigned(LBM_ROWS64_FLAG_MULTI_STEPS | LBM64_FLAG_MULTI_STEPS), 0u}) {
          const lbm64_params p{g[0], g[1], 11, 10, 0.1, 0.005, 1.85};
          for (int r = 0; r < (g[2] > 0 ? g[2] : 1); ++r, ++shown) {
            lbm_internal::PlanRowsMulti64 m;
            char name[64] = "";
            const int rc = lbm_plan64_rows_multi(&p, g[2], r, f, &m);
            if (rc != 0) { std::printf("rows* %6d x %-6d rank %d of %d flags %u: %s\n", g[0], g[1], r, g[2], f, lbm_last_error()); continue; }
            lbm_plan64_rows_multi_kernel_name(&m, name, sizeof name);
            std::printf("rows* %6d x %-6d rank %d of %d flags %u min '%s': %s K %d ghost %d, %d tiles (%d a row) x %d lanes, LDS %d, nt %d, mask %d words, partials %d, ps %lld, grid %lld\n",
                        g[0], g[1], r, g[2], f, minimum, m.multi_kernel ? name : "(falls back)", m.K, m.ghost, m.n_tiles, m.tiles_x, m.block, m.lds_bytes, m.nt_stores, m.mask_words, m.partials_cap, m.ps, m.grid_doubles);
            if (r == 0 && m.multi_kernel) {
              int steps[16], full[16];
              const int n = lbm_plan64_rows_multi_run_launches(&m, 11, steps, full, 16);
              for (int i = 0; i < n && i < 16; ++i, ++launches) std::printf("  11 steps  launch %d: k %d full %d\n", i, steps[i], full[i]);
            }
          }
        }
    }
  std::printf("%d plans, %d launches, clean\n", shown, launches);
  return 0;
}
