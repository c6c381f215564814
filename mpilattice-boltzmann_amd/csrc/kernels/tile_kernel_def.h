// tile_kernel_def.h — the text of lbm_tile_kernel, included by kernels/tile.h once per arithmetic (no include guard on purpose).
// LBM_TILE_FUSED = 0: lbm_tile_kernel<T, H, FULL, FAST>; 1: lbm_tile_kernel_fused<T, H, FULL> (LBM_FLAG_FUSED_ARITH).
#if LBM_TILE_FUSED
template <int T, int H, bool FULL>              // the fused arithmetic of relax_core (kernels/common.h), double-precision sum|u| terms
__global__ void __launch_bounds__((TileGeom<T, H>::block)) lbm_tile_kernel_fused(const TileArgs a)
{
  constexpr bool FAST = false;
#else
template <int T, int H, bool FULL, bool FAST>   // FULL: this launch does exactly H steps (region sizes are compile-time constants); FAST: float sum|u| terms
__global__ void __launch_bounds__((TileGeom<T, H>::block)) lbm_tile_kernel(const TileArgs a)
{
#endif
  using G = TileGeom<T, H>;
  constexpr int R = G::R, RP = G::RP, kCells = G::cells, kWaves = G::waves, kBlock = G::block;
  extern __shared__ __attribute__((aligned(16))) float lds[];        // [2][9][R*R] floats, reduction scratch, flag bytes
  double* red = reinterpret_cast<double*>(lds + 2 * 9 * kCells);    // [H][kWaves]
  uint8_t* cell_flags = reinterpret_cast<uint8_t*>(red + H * kWaves);   // per region cell: bit 0 obstacle, 1 owned, 2 on row ny-2
  const int tid = threadIdx.x;

  if (blockIdx.x == 0) {
    // fold block: the previous launch's per-tile sums, one vector per step, into sums[counter..]
    for (int v = 0; v < a.n_prev_vecs; ++v) {
      double s = 0.0;
      for (int i = tid; i < a.n_prev; i += kBlock) s += a.prev_partials[static_cast<size_t>(v) * a.n_prev + i];
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
    return;
  }

  LBM_STAMP(0);
  const int tile = blockIdx.x - 1;
  const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
  // does the region of this tile meet row ny-2 at all ?  (block-uniform; the others skip accelerate_flow)
  bool tile_accel;
  {
    int d = (a.accel_row - (ty * T - H)) % a.ny;
    if (d < 0) d += a.ny;
    tile_accel = d < R || a.ny < R;
  }

  // ---- load: lane = one aligned x-pair of the region, periodic (d2q9-bgk.c:527-529 in x; :245-247 one-rank ring
  // in y); nx, T and H are even, so a pair never straddles the wrap and its first cell has an even index
  if (tid < RP * R) {
    const int ry = tid / RP, rx = 2 * (tid - ry * RP);
    int gx = (tx * T - H + rx) % a.nx; if (gx < 0) gx += a.nx;
    int gy = (ty * T - H + ry) % a.ny; if (gy < 0) gy += a.ny;
    const int cell = gy * a.nx + gx;
    const uint32_t mbits = (a.mask[cell >> 5] >> (cell & 31)) & 3u;
    const uint32_t common = ((rx >= H && rx < H + T && ry >= H && ry < H + T) ? 2u : 0u) | (gy == a.accel_row ? 4u : 0u);
    const int c = ry * R + rx;
#pragma unroll
    for (int k = 0; k < 9; ++k) *reinterpret_cast<f2*>(lds + k * kCells + c) = *reinterpret_cast<const f2*>(a.src + k * a.ps + cell);
    *reinterpret_cast<uint16_t*>(cell_flags + c) = static_cast<uint16_t>(((mbits & 1u) | common) | ((((mbits >> 1) & 1u) | common) << 8));
  }
  __syncthreads();
  LBM_STAMP(1);

  double acc[H];
#pragma unroll
  for (int i = 0; i < H; ++i) acc[i] = 0.0;

  const int k_total = FULL ? H : a.ksteps;
  // One sub-step; S is a compile-time constant (the sub-steps are unrolled: buffer roles and the accumulator slot fold).
  auto substep = [&](auto sc) __attribute__((always_inline)) {
    constexpr int S = decltype(sc)::value;
    const float* bufA = lds + ((S & 1) ? 0 : 9 * kCells);
    float* bufB = lds + ((S & 1) ? 9 * kCells : 0);
    // cells still needed after this sub-step: the owned tile expanded by e = k_total - S
    const int e = k_total - S;
    const int side = T + 2 * e;
    if (side * side <= a.single_max && side * side <= kBlock) {   // block-uniform
      // Late sub-steps: the region fits the block's SIMDs with one CELL per lane — a wave alone on its SIMD issues an
      // instruction every 4+ cycles whether it is packed or not, so what counts is the length of one lane's chain:
      // ~190 instructions for a cell against ~330 for an x-pair (division, double sqrt and the unaligned LDS
      // accesses are per cell either way).  Same relax_core, same order of operations: the same bits.
      if (tid < side * side) {
        const int ry = small_div(tid, side), rx = tid - ry * side;
        const int x = H - e + rx, y = H - e + ry;
        const int c = y * R + x;
        const uint32_t fl = cell_flags[c];
        float t[9], o[9], out[9];                                                  // d2q9-bgk.c:530-538
        t[0] = bufA[0 * kCells + c];         t[1] = bufA[1 * kCells + c - 1];     t[2] = bufA[2 * kCells + c - R];
        t[3] = bufA[3 * kCells + c + 1];     t[4] = bufA[4 * kCells + c + R];     t[5] = bufA[5 * kCells + c - R - 1];
        t[6] = bufA[6 * kCells + c - R + 1]; t[7] = bufA[7 * kCells + c + R + 1]; t[8] = bufA[8 * kCells + c + R - 1];
        float msq, rinv;
        relax_core<float, LBM_TILE_FUSED != 0>(t, a.omega, o, msq, rinv);
        const bool blocked = fl & 1u;
        bounce_or_relax(t, o, blocked, out);                                      // :687-695
        if (tile_accel && (fl & 4u) && !blocked && (S < k_total || a.accel_last)) accelerate_cell(out, a.accel_w1, a.accel_w2);   // :457-469
        double term = 0.0;
        if ((fl & 3u) == 2u)                                                          // owned fluid cell (:667)
          term = FAST ? static_cast<double>(__builtin_amdgcn_sqrtf(msq) * rinv) : sqrt_of_float(msq) * static_cast<double>(rinv);
        acc[S - 1] = term;
        if (S < k_total) {
#pragma unroll
          for (int k = 0; k < 9; ++k) bufB[k * kCells + c] = out[k];
        } else {
          const int cell = (ty * T + ry) * a.nx + tx * T + rx;
#pragma unroll
          for (int k = 0; k < 9; ++k) a.dst[k * a.ps + cell] = out[k];
        }
      }
    } else {
      const int w = T / 2 + e;                          // pairs per row of that region
      if (tid < w * (T + 2 * e)) {
        const int ry = small_div(tid, w), rp = tid - ry * w;
        const int x = H - e + 2 * rp, y = H - e + ry;   // region cells (x, y), (x+1, y)
        const int c = y * R + x;
        const uint32_t fl0 = cell_flags[c], fl1 = cell_flags[c + 1];
        const uint32_t mbits = (fl0 & 1u) | ((fl1 & 1u) << 1);
        // a pair that starts on an odd x may straddle the edge of the owned tile: per-cell skip bits
        const uint32_t skip = (((fl0 & 1u) | ((fl0 & 2u) ? 0u : 1u))) | (((fl1 & 1u) | ((fl1 & 2u) ? 0u : 1u)) << 1);
        f2 p[9], out[9];                                                           // d2q9-bgk.c:530-538
        p[0] = f2{bufA[0 * kCells + c], bufA[0 * kCells + c + 1]};
        p[2] = f2{bufA[2 * kCells + c - R], bufA[2 * kCells + c - R + 1]};
        p[4] = f2{bufA[4 * kCells + c + R], bufA[4 * kCells + c + R + 1]};
        p[1] = f2{bufA[1 * kCells + c - 1], bufA[1 * kCells + c]};
        p[5] = f2{bufA[5 * kCells + c - R - 1], bufA[5 * kCells + c - R]};
        p[8] = f2{bufA[8 * kCells + c + R - 1], bufA[8 * kCells + c + R]};
        p[3] = f2{bufA[3 * kCells + c + 1], bufA[3 * kCells + c + 2]};
        p[6] = f2{bufA[6 * kCells + c - R + 1], bufA[6 * kCells + c - R + 2]};
        p[7] = f2{bufA[7 * kCells + c + R + 1], bufA[7 * kCells + c + R + 2]};
        // relaxation, bounce-back (:687-695), accelerate_flow of the following step (:457-469), sum|u| terms
        acc[S - 1] = finish_pair<(FAST ? kTermsFloat : kTermsDouble) | (LBM_TILE_FUSED ? kTermsFused : 0)>(p, mbits, a.omega, tile_accel, (fl0 & 4u) && (S < k_total || a.accel_last), a.accel_w1, a.accel_w2,
                                 skip, out);
        if (S < k_total) {
#pragma unroll
          for (int k = 0; k < 9; ++k) { bufB[k * kCells + c] = out[k].x; bufB[k * kCells + c + 1] = out[k].y; }
        } else {
          // last sub-step: the region is the owned tile (x = H + 2 rp, y = H + ry), inside the grid
          const int cell = (ty * T + ry) * a.nx + tx * T + 2 * rp;
#pragma unroll
          for (int k = 0; k < 9; ++k) *reinterpret_cast<f2*>(a.dst + k * a.ps + cell) = out[k];
        }
      }
    }
    if (S < k_total) __syncthreads();
    LBM_STAMP(1 + S);
  };
  if (1 <= k_total) substep(std::integral_constant<int, 1>{});
  if (2 <= k_total) substep(std::integral_constant<int, 2>{});
  if (3 <= k_total) substep(std::integral_constant<int, 3>{});
  if (4 <= k_total) substep(std::integral_constant<int, 4>{});
  if constexpr (H >= 8) {
    if (5 <= k_total) substep(std::integral_constant<int, 5>{});
    if (6 <= k_total) substep(std::integral_constant<int, 6>{});
    if (7 <= k_total) substep(std::integral_constant<int, 7>{});
    if (8 <= k_total) substep(std::integral_constant<int, 8>{});
  }
  static_assert(H == 4 || H == 8, "sub-steps are unrolled for H = 4 and 8");

  // per-step sums over the owned cells of this tile: one halving butterfly per wave (common.h), then one lane per step
  // over the waves
  const int ntiles = gridDim.x - 1;
  if constexpr (H == 8) {
    const double w = wave_sum_vec8(acc);
    if ((tid & 7) == 0) red[wave_sum_slot<8>(tid & 63) * kWaves + (tid >> 6)] = w;
  } else {
    const double w = wave_sum_vec4(acc[0], acc[1], acc[2], acc[3]);
    if ((tid & 15) == 0) red[wave_sum_slot<4>(tid & 63) * kWaves + (tid >> 6)] = w;
  }
  lds_barrier();                 // LDS only: no wait for the tile's global stores
  if (tid < k_total) {
    double t = 0.0;
    for (int w = 0; w < kWaves; ++w) t += red[tid * kWaves + w];
    a.partials_out[static_cast<size_t>(tid) * ntiles + tile] = t;
  }
  LBM_STAMP(10);
}
