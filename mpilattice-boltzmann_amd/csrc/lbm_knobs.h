// lbm_knobs.h — every LBM_* environment knob of liblbm_d2q9.so and liblbm_d2q9_rccl.so, in one table.  Not part of the ABI.
//
// One row per knob: X(environment name, field of Knobs, default, parser).  knobs_from_env() reads every row: unset or empty means
// the default, any other value goes through the parser (std::atoi; schedule_of for "serial" / "edge").  kKnobUnset is the default
// of a knob whose fallback depends on the grid: the code that uses it computes that fallback (knob_or).
//
// knobs_from_env() is the only getenv of both libraries, and nothing reads it while it runs, launches or waits.  A context
// (lbm_create*) keeps the snapshot it was created with; a transport (lbm_p2p_create, lbm_comm_create) reads one when it is
// created; a free function (lbm_rank_layout, lbm_tile_layout_of, lbm_choose_rank_grid, the writers) reads one per call.
// scripts/README.md documents every row, and tests/test_host_logic.py checks that the two lists agree.
#pragma once

#include <climits>
#include <cstdlib>
#include <cstring>

constexpr int kKnobUnset = INT_MIN;
constexpr int kScheduleSerial = 0, kScheduleEdge = 1;

inline int schedule_of(const char* v) { return !std::strcmp(v, "serial") ? kScheduleSerial : !std::strcmp(v, "edge") ? kScheduleEdge : kKnobUnset; }
inline int knob_or(int v, int fallback) { return v == kKnobUnset ? fallback : v; }

#define LBM_KNOBS(X)                                                                        \
  /* contexts: read when lbm_create* makes one */                                          \
  X(LBM_TUNE_SKEW,              skew,              24,         std::atoi)                   \
  X(LBM_TUNE_MAXBLOCKS,         maxblocks,         16384,      std::atoi)                   \
  X(LBM_TUNE_NARROW_MAX,        narrow_max,        65536,      std::atoi)                   \
  X(LBM_TUNE_TILE_MAX,          tile_max,          131072,     std::atoi)                   \
  X(LBM_TUNE_TILE_GEOM,         tile_geom,         kKnobUnset, std::atoi)                   \
  X(LBM_TUNE_TILE_SINGLE_MAX,   tile_single_max,   512,        std::atoi)                   \
  X(LBM_TUNE_TILE64_MAX,        tile64_max,        1 << 20,    std::atoi)                   \
  X(LBM_TUNE_TILE64_GEOM,       tile64_geom,       kKnobUnset, std::atoi)                   \
  X(LBM_TUNE_MULTI64_K,         multi64_k,         kKnobUnset, std::atoi)                   \
  X(LBM_TUNE_MULTI64_MIN,       multi64_min,       kKnobUnset, std::atoi)                   \
  X(LBM_TUNE_MULTI_K,           multi_k,           kKnobUnset, std::atoi)                   \
  X(LBM_TUNE_MULTI5_MIN,        multi5_min,        1 << 26,    std::atoi)                   \
  X(LBM_TUNE_MULTI_TAIL4,       multi_tail4,       1,          std::atoi)                   \
  X(LBM_TUNE_MULTI_TILE,        multi_tile,        kKnobUnset, std::atoi)                   \
  X(LBM_TUNE_NARROW_TILE_MAX,   narrow_tile_max,   1 << 17,    std::atoi)                   \
  X(LBM_TUNE_TALL_TILE_MIN,     tall_tile_min,     1 << 20,    std::atoi)                   \
  X(LBM_TUNE_MULTI_GEOM,        multi_geom,        -1,         std::atoi)                   \
  X(LBM_TUNE_MULTI_REMAP,       multi_remap,       1,          std::atoi)                   \
  X(LBM_TUNE_TILE_PAD_GRID,     tile_pad_grid,     1,          std::atoi)                   \
  X(LBM_TUNE_TERMS,             terms,             -1,         std::atoi)                   \
  X(LBM_TUNE_FOLD_SLICED_MIN,   fold_sliced_min,   1024,       std::atoi)                   \
  X(LBM_TUNE_OBS_CHUNK_CELLS,   obs_chunk_cells,   16 << 20,   std::atoi)                   \
  X(LBM_DEBUG_ADDR,             debug_addr,        0,          std::atoi)                   \
  /* the layout rule: contexts, and every call of the layout functions */                  \
  X(LBM_TUNE_MACRO_K,           macro_k,           4,          std::atoi)                   \
  X(LBM_TUNE_MACRO_GHOST,       macro_ghost,       kKnobUnset, std::atoi)                   \
  X(LBM_TUNE_MACRO_GROUP,       macro_group,       kKnobUnset, std::atoi)                   \
  X(LBM_TUNE_TILE_GHOST_X,      tile_ghost_x,      kKnobUnset, std::atoi)                   \
  X(LBM_TUNE_TILE_GHOST_ROWS,   tile_ghost_rows,   0,          std::atoi)                   \
  /* transports: read when lbm_p2p_create / lbm_comm_create makes one */                   \
  X(LBM_P2P_TIMEOUT_MS,         p2p_timeout_ms,    30000,      std::atoi)                   \
  X(LBM_P2P_SCHEDULE,           p2p_schedule,      kKnobUnset, schedule_of)                 \
  X(LBM_P2P_PUSH_BLOCKS,        p2p_push_blocks,   32,         std::atoi)                   \
  X(LBM_P2P_WINDOW,             p2p_window,        0,          std::atoi)                   \
  X(LBM_RCCL_SCHEDULE,          rccl_schedule,     kKnobUnset, schedule_of)                 \
  /* writers (lbm_host.cpp): read per call */                                              \
  X(LBM_WRITE_THREADS,          write_threads,     kKnobUnset, std::atoi)

struct Knobs {
#define LBM_KNOB_FIELD(name, field, dflt, parse) int field = dflt;
  LBM_KNOBS(LBM_KNOB_FIELD)
#undef LBM_KNOB_FIELD
};

inline Knobs knobs_from_env()
{
  Knobs k;
#define LBM_KNOB_READ(name, field, dflt, parse) \
  if (const char* v = std::getenv(#name); v && *v) k.field = parse(v);
  LBM_KNOBS(LBM_KNOB_READ)
#undef LBM_KNOB_READ
  return k;
}
