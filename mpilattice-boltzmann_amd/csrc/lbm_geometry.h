// lbm_geometry.h — the numbers the kernels and the host agree on: block sizes, tile shapes, the steps a launch can make, the forms of
// the sum|u| terms.  constexpr values and functions only: no device code, no HIP header, so that the host-only planning unit
// (lbm_plan.cpp) and the device units (kernels/*.h) read one definition.  Not part of the ABI.
#pragma once

namespace {

// ---- every kernel (kernels/common.h) ----
constexpr int kBlock = 256;          // 4 wavefronts
constexpr int kCellsPerLane = 4;     // one 16-byte access per population per lane
constexpr int kHaloGuard = 4;        // floats of guard on each side of a halo-buffer row

// TERMS: how the sum|u| term of a cell, sqrt((double)msq) * (double)rinv (:667), is formed.  Populations never depend on it.
//   kTermsDouble (LBM_FLAG_EXACT_AVVELS; lbm_tile_kernel's default): in double precision, every term correctly
//     rounded before the product: v_rsq_f64 + 9 double-precision instructions per CELL.
//   kTermsCompensated (lbm_multi_kernel's default): without double-precision arithmetic.  The root as an unevaluated float
//     sum s + c (s = msq * rsq(msq); c = the Newton correction of s from the residual msq - s*s, which a fused multiply-add
//     delivers exactly), the product with rinv as p + lo (p = s * rinv, its rounding error by another fused multiply-add,
//     plus c * rinv): relative error at most 2^-43.6 + 2^-151 / msq per cell (float denormals kept, as this build keeps them)
//     where the double form has 2^-53, i.e. ~2^-44 for msq >= 2^-104 and growing to 2^-25 at msq = 2^-126, as the residual
//     underflows; below 2^-126 the guard on the rsq argument makes the term an under-estimate, between 0 and the double form's
//     (derivation, per-pair test through this function and measured maxima: tests/test_terms_cells.py, profiles/r13) —
//     av_vels, a float, comes out bit for
//     bit the same in every test here — in 7 packed float instructions and two v_rsq_f32 per PAIR.  Only p is widened per
//     pair; the lo parts are summed per lane in float (a lane adds at most a few per launch) and widened once.  Why it
//     matters: the launch runs AT the socket power limit (scripts/power_trace.py: 1380 of 1400 W, shader clock 2.2 of
//     2.4 GHz); double-precision instructions it does not execute come back as clock.  A cell at rest (msq = 0) gives 0:
//     the rsq argument is held at the smallest normal number.  msq = inf (a diverged run) gives NaN where the reference
//     gives inf.
//   kTermsFloat (LBM_FLAG_FAST_AVVELS): v_sqrt_f32 and one multiply; av_vels then agrees to ~1e-7 (an ulp of its float).
// kTermsFused added to one of them (LBM_FLAG_FUSED_ARITH): the same terms from the msq and rinv of the fused arithmetic (relax_core).
constexpr int kTermsDouble = 0, kTermsFloat = 1, kTermsCompensated = 2, kTermsFused = 4;

// ---- lbm_tile_kernel (kernels/tile.h): most steps of one launch, the ghost ring of its widest geometry ----
constexpr int kMaxTileSteps = 8;

// ---- the end-of-run fold (kernels/aux.h): blocks per step vector of lbm_fold_slices_kernel ----
constexpr int kFoldSlices = 64;

// ---- the double-precision one-step kernel (kernels/step64.h) ----
constexpr int kPairCells = 2;        // one 16-byte access per population per lane

// ---- lbm_tile_kernel_f64<T, H, FULL> (kernels/tile64.h): its geometries, and what a block of each takes ----
// T = owned tile edge, H = ghost ring = most steps of a launch; the region is R x R, R = T + 2H.  One cell per lane, dealt anew in every
// sub-step over a strided loop: 256 lanes hold the largest computed region of <8,4> (14 x 14), 512 that of <8,8> and <16,4> (22 x 22) in
// one pass; <16,8> (30 x 30 down to 16 x 16) takes two passes of 512 lanes while its region has more than 512 cells.
// LDS: two buffers of 9 R^2 doubles, H x waves doubles of reduction scratch, one flag byte per region cell.
constexpr bool tile64_geom_ok(int t, int h) { return (t == 8 || t == 16) && (h == 4 || h == 8); }
constexpr int tile64_region(int t, int h) { return t + 2 * h; }
constexpr int tile64_block(int t, int h) { return (t == 8 && h == 4) ? 256 : 512; }
constexpr int tile64_lds_bytes(int t, int h)
{
  return tile64_region(t, h) * tile64_region(t, h) * (2 * 9 * 8 + 1) + 8 * h * (tile64_block(t, h) / 64);
}
constexpr int kTile64Rows = 4 * 2;   // the host's table kTile64Kernels (lbm_f64.hip): one row per (geometry, FULL)
constexpr int tile64_row(int t, int h, bool full) { return ((t == 8 ? 2 : 0) + (h == 4 ? 1 : 0)) * 2 + (full ? 1 : 0); }
static_assert(tile64_lds_bytes(16, 8) <= 160 * 1024 && tile64_lds_bytes(8, 4) <= 64 * 1024, "a block's LDS: at most what a CU gives one workgroup");

// ---- lbm_multi_kernel (kernels/multi.h) ----
#ifndef LBM_MTY            // experiment builds: -DLBM_MTY=24 -DLBM_MLANES=768 (taller tiles, two blocks per CU)
#define LBM_MTY 16
#define LBM_MLANES 512
#endif
#ifndef LBM_MWAVES         // most waves per SIMD the kernels are compiled for (register budget 512 / LBM_MWAVES)
#define LBM_MWAVES 6
#endif
#ifndef LBM_MTY4           // tile height of the 4-step instantiation, standard and narrow geometry (512 lanes)
#define LBM_MTY4 13
#endif
#ifndef LBM_MTY4T          // tile height and block size of the 4-step instantiation, tall geometry
#define LBM_MTY4T 24
#define LBM_MLANES4T 768
#endif
constexpr int kMTX = 64, kMTXNarrow = 32, kMTY = LBM_MTY, kMTY4 = LBM_MTY4, kMTY4Tall = LBM_MTY4T, kMLanes = LBM_MLANES, kMLanes4Tall = LBM_MLANES4T,
              kMaxMultiSteps = 4,      // most steps of a launch of a partition, and of every geometry but the tall one
              kMaxWholeGridSteps = 5,  // ... of a whole periodic grid on the tall geometry: lbm_multi_kernel<5, TERMS, kGeomTall, kPartPlain> (multi_compact0 below)
              kMaxGhost = 32,      // most ghost rows / columns a K-step partition keeps per side: the steps of a group of launches between two halo exchanges (32: column blocks)
              kMaxGroup = 8;       // most launches of such a group
constexpr int kMinMultiTY = kMTY < kMTY4 ? (kMTY < kMTY4Tall ? kMTY : kMTY4Tall) : (kMTY4 < kMTY4Tall ? kMTY4 : kMTY4Tall);
// Geometry of a launch: tile width, and by steps per launch tile height and block size.
//   kGeomStd     64-wide tiles.  K <= 3: 64 x 16, 512 lanes (K = 3: 68 x 20 frame, 48.7 KB, three blocks per CU).  K = 4: 64 x 13 (72 x 19 frame,
//                49.0 KB, three blocks per CU).
//   kGeomTall    K = 4 on 64 x 24 tiles with 768-lane blocks: 72 x 30 frame = 77.4 KB, TWO blocks of twelve waves per CU (the same 24 waves);
//                the host picks it from 2^20 cells up.  K <= 3: as kGeomStd.  K = 5 (whole periodic grids only, kMaxWholeGridSteps): the same
//                64 x 24 tiles and 768 lanes on a 72 x 32 frame of EIGHT planes — population 0 never streams, so the owned pairs keep it in a
//                register and the ring pairs of sub-step 1 (384) in a compact array of their own: 76.6 KB, still two blocks per CU (nine
//                planes of 72 x 32 floats alone would be 82.9 KB).
//   kGeomNarrow  32-wide tiles, heights as kGeomStd: partitions so small that a launch is one round of blocks (twice the tiles, each
//                with half the dependent work — a 1024 x 128-row partition keeps 256 CUs busy instead of 128).
// The measurements behind each choice, round by round: DESIGN_APPENDIX.md R8.1.
constexpr int kGeomStd = 0, kGeomNarrow = 1, kGeomTall = 2;
constexpr int geom_tx(int g) { return g == kGeomNarrow ? kMTXNarrow : kMTX; }
constexpr int multi_ty(int k, int g) { return k >= 4 ? (g == kGeomTall ? kMTY4Tall : kMTY4) : kMTY; }
constexpr int multi_lanes(int k, int g) { return (k >= 4 && g == kGeomTall) ? kMLanes4Tall : kMLanes; }
constexpr int geom_for(int k, int g) { return (g == kGeomTall && k < 4) ? kGeomStd : g; }      // the instantiation a launch of k steps uses

// Sub-step j of k (1-based) works on the owned tile grown by (k-j) rows and multi_ex(k-j) = 2 ceil((k-j)/2)
// columns on each side: the column growth is rounded up to even so that every region starts on an even x
// and a lane can own an x-PAIR of cells (8-byte accesses; the two cells' arithmetic is packed by the
// compiler into v_pk_*_f32, which halves the instruction count - the one-cell form of this kernel was
// VALU-bound).  Where k-j is odd the region's outermost column lies outside every owned cell's dependency
// cone: it is computed from whatever the frame holds there (stale values of an earlier sub-step, always
// inside the frame) and never kept or counted.  (Rounds 1 - 4 grew the columns by 2(k-j): K = 4 regions
// 76 / 72 / 68 / 64 wide instead of 72 / 68 / 68 / 64, frames 12 columns wider than needed.)
constexpr int multi_ex(int ey) { return 2 * ((ey + 1) / 2); }

// A block's LDS, in bytes: the frame's planes, the reduction scratch (a double per step and wave) and a flag byte per x-pair of the frame.
// The kernel (MultiGeom::lds_bytes, kernels/multi.h) and the planner (lbm_plan.cpp) read this one definition.
// multi_compact0: the frame holds populations 1 - 8 only; population 0 of a ring pair lives in an array of one float pair per ring pair
// of sub-step 1 (the later rings are subsets of the first), between the planes and the reduction scratch.
constexpr bool multi_compact0(int k, int g) { return k == kMaxWholeGridSteps && g == kGeomTall; }
constexpr int multi_frame_w(int k, int g) { return geom_tx(g) + 2 * multi_ex(k - 1); }
constexpr int multi_frame_h(int k, int g) { return multi_ty(k, g) + 2 * (k - 1); }
// x-pairs of sub-step j's region outside the owned tile: k - j rows below and above it, multi_ex(k - j) / 2 pairs on each side of its rows
constexpr int multi_ring_pairs(int k, int g, int j) { return 2 * (k - j) * (geom_tx(g) / 2 + multi_ex(k - j)) + multi_ty(k, g) * multi_ex(k - j); }
constexpr int multi_lds_bytes(int k, int g)
{
  const int cells = multi_frame_w(k, g) * multi_frame_h(k, g);
  return 4 * (multi_compact0(k, g) ? 8 : 9) * cells + (multi_compact0(k, g) ? 8 * multi_ring_pairs(k, g, 1) : 0) + 8 * k * (multi_lanes(k, g) / 64) + (k >= 2 ? cells / 2 : 0);
}
static_assert(multi_lds_bytes(kMaxWholeGridSteps, kGeomTall) * 2 <= 160 * 1024, "two blocks of the five-step launch per CU");

// ---- lbm_multi_kernel_f64<K, NT, FULL> (kernels/multi64.h): lbm_multi_kernel's scheme with every object a double ----
// A block of kMulti64Lanes lanes owns a kMulti64TX x kMulti64TY tile, one owned cell per lane in the last sub-step.  The LDS frame is ONE
// buffer of (TX + 2 multi_ex(K-1)) x (TY + 2 (K-1)) cells of nine doubles, updated in place; behind it kMulti64Accs x waves doubles
// of reduction scratch and one flag byte per frame cell.  K = 2: 36 x 18, 47.6 KB; K = 3: 36 x 20, 52.8 KB (three blocks in a CU's
// 160 KiB); K = 4: 40 x 22, 64.5 KB (two).
constexpr int kMulti64TX = 32, kMulti64TY = 16, kMulti64Lanes = 512, kMulti64MinK = 2, kMulti64MaxK = 4;
constexpr int kMulti64Accs = 4;       // per-lane accumulators, one per sub-step: what wave_sum_vec4 joins
constexpr bool multi64_k_ok(int k) { return k >= kMulti64MinK && k <= kMulti64MaxK; }
constexpr int multi64_frame_x(int k) { return kMulti64TX + 2 * multi_ex(k - 1); }
constexpr int multi64_frame_y(int k) { return kMulti64TY + 2 * (k - 1); }
constexpr int multi64_lds_bytes(int k)
{
  return multi64_frame_x(k) * multi64_frame_y(k) * (9 * 8 + 1) + 8 * kMulti64Accs * (kMulti64Lanes / 64);
}
constexpr int kMulti64Rows = (kMulti64MaxK - kMulti64MinK + 1) * 2 * 2;   // the host's table kMulti64Kernels (lbm_f64.hip): one row per (K, NT, FULL)
constexpr int multi64_row(int k, bool nt, bool full) { return ((k - kMulti64MinK) * 2 + (nt ? 1 : 0)) * 2 + (full ? 1 : 0); }
static_assert(kMulti64TX * kMulti64TY == kMulti64Lanes, "the last sub-step deals one owned cell to every lane");
static_assert(kMulti64MaxK <= kMulti64Accs, "one accumulator per sub-step");
static_assert((kMulti64TX + 2 * (kMulti64MaxK - 2)) * (kMulti64TY + 2 * (kMulti64MaxK - 2)) <= 2 * kMulti64Lanes, "a frame sub-step deals a lane at most two cells");
static_assert(multi64_lds_bytes(kMulti64MaxK) <= 160 * 1024, "a block's LDS: at most what a CU gives one workgroup");

// PART of lbm_multi_kernel (the forms themselves: kernels/multi.h): kPartPlain (whole periodic grids, and the launches of a partition that
// compute its owned rows only), kPartGhost (a launch that also computes ghost rows: the counted test), kPartReady (owned rows only + the
// ready words in the fold block), kPartTile (every launch of a rank of the 2-D decomposition: ghost rows AND ghost columns — the counted
// and kept tests in x as well, in the tiles on the rim of the owned block only — and four ready words).
constexpr int kPartPlain = 0, kPartGhost = 1, kPartReady = 2, kPartTile = 3;

// ---- the host's tables of instantiations (lbm_kernels.hip kMultiKernels, kTileKernels): which row a launch takes ----
// lbm_multi_kernel: one row per (geometry, steps, terms, launch form).  The terms index of a row: the three forms of the sum|u| terms,
// then (index kMultiTermsFused) the fused arithmetic with lbm_multi_kernel's default form of them.
constexpr int kMultiTermsFused = 3;
constexpr int kMultiTerms = 4, kMultiParts = 4, kMultiGeoms = 3, kMultiRowsPerGeom = kMaxMultiSteps * kMultiTerms * kMultiParts;
constexpr int multi_row(int k, int geom, int terms, int part) { return ((geom * kMaxMultiSteps + k - 1) * kMultiTerms + terms) * kMultiParts + part; }
// ... and behind those rows the five-step launch of whole grids, tall geometry and plain form only: one row per terms index
constexpr int kMultiRows = kMultiGeoms * kMultiRowsPerGeom, kMultiRowsTotal = kMultiRows + kMultiTerms;
constexpr int multi_row5(int terms) { return kMultiRows + terms; }
// lbm_tile_kernel: one row per (geometry, FULL, terms).  The terms index of a row: double-precision sum|u| terms, float ones
// (LBM_FLAG_FAST_AVVELS), the fused arithmetic (LBM_FLAG_FUSED_ARITH; never with the float terms: plan_context).
constexpr int kTileTermsFused = 2, kTileTerms = 3, kTileRows = 4 * 2 * kTileTerms;
constexpr int tile_row(int t, int h, bool full, int terms) { return (((t == 8 ? 2 : 0) + (h == 4 ? 1 : 0)) * 2 + (full ? 1 : 0)) * kTileTerms + terms; }

}  // namespace
