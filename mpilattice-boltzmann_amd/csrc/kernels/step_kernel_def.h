// step_kernel_def.h — the text of the two one-step kernels, included by kernels/step.h once per arithmetic (no include guard on purpose).
// LBM_STEP_FUSED = 0: lbm_step_kernel<NT>, lbm_step_kernel_narrow<NT>; 1: lbm_step_kernel_fused<NT>, lbm_step_kernel_narrow_fused<NT>
// (LBM_FLAG_FUSED_ARITH: relax_core's fused sequence through step_quad / step_cell).
#if LBM_STEP_FUSED
#define LBM_STEP_NAME(base) base##_fused
#define LBM_STEP_ARITH NT, true
#else
#define LBM_STEP_NAME(base) base
#define LBM_STEP_ARITH NT
#endif

// The fused streaming-pull step.  Grid: ceil(#quads / (256*iters)) work blocks of 256 lanes (block b
// owns `iters` consecutive 1024-cell chunks) after one fold block (block 0, dispatched first).
template <bool NT>
__global__ void __launch_bounds__(kBlock) LBM_STEP_NAME(lbm_step_kernel)(const StepArgs a)
{
  __shared__ double red[kBlock / 64];
  if (blockIdx.x == 0) { fold_previous(a, red); return; }
  const int wblock = blockIdx.x - 1;   // work block index
  double acc = 0.0;
  const int n1 = a.quad_end - a.quad_begin;
  const int n2 = a.quad_end2 > a.quad_begin2 ? a.quad_end2 - a.quad_begin2 : 0;
  const int base = wblock * a.iters * kBlock + threadIdx.x;
  for (int i = 0; i < a.iters; ++i) {
    const int r = base + i * kBlock;
    if (r < n1 + n2) acc += step_quad<LBM_STEP_ARITH>(a, r < n1 ? a.quad_begin + r : a.quad_begin2 + (r - n1));
  }
  acc = block_sum(acc, red);
  // boundary launch of a peer-to-peer run: the outgoing halo rows were stored straight into the neighbours' windows;
  // a full barrier drains every wave's stores (block_sum's barriers order LDS only), then one lane writes the XCD's L2
  // back towards the peers
  if (a.release_sends) __syncthreads();
  if (threadIdx.x == 0) {
    a.partials_out[wblock] = acc;
    if (a.release_sends) __atomic_thread_fence(__ATOMIC_RELEASE);
  }
}

// One cell per lane; the unit ranges of StepArgs are cell ranges here.
template <bool NT>
__global__ void __launch_bounds__(kBlock) LBM_STEP_NAME(lbm_step_kernel_narrow)(const StepArgs a)
{
  __shared__ double red[kBlock / 64];
  if (blockIdx.x == 0) { fold_previous(a, red); return; }
  const int wblock = blockIdx.x - 1;   // work block index
  double acc = 0.0;
  const int n1 = a.quad_end - a.quad_begin;
  const int n2 = a.quad_end2 > a.quad_begin2 ? a.quad_end2 - a.quad_begin2 : 0;
  const int base = wblock * a.iters * kBlock + threadIdx.x;
  for (int i = 0; i < a.iters; ++i) {
    const int r = base + i * kBlock;
    if (r < n1 + n2) acc += step_cell<LBM_STEP_ARITH>(a, r < n1 ? a.quad_begin + r : a.quad_begin2 + (r - n1));
  }
  acc = block_sum(acc, red);
  if (a.release_sends) __syncthreads();                                  // see lbm_step_kernel
  if (threadIdx.x == 0) {
    a.partials_out[wblock] = acc;
    if (a.release_sends) __atomic_thread_fence(__ATOMIC_RELEASE);
  }
}

#undef LBM_STEP_NAME
#undef LBM_STEP_ARITH
