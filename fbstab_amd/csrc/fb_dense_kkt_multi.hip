// The kernels of fbstab_hip_dense_kkt_solve_batch and fbstab_hip_dense_jacobian_batch (fb_dense_kkt_multi.h), one
// per dense adjoint kernel, and the factory fbstab_hip.hip's kernel table calls.  A translation unit of its own: the
// code of some kernels of fbstab_hip.hip depends on the order the compiler meets them (dense_resolve_kernels;
// tools/diff_device_code.py).
#include <hip/hip_runtime.h>

#include "fb_dense_kkt_multi.h"

namespace fbk {

// Next QP index for this workgroup (workgroup-uniform), as the dense adjoint kernels pull theirs.
template <int NT>
__device__ __forceinline__ int dense_kkt_next_qp(int* counter, lds_ptr slot) {
  if (NT <= 64) {
    int q = 0;
    if (threadIdx.x == 0) q = atomicAdd(counter, 1);
    return __shfl(q, 0, 64);
  } else {
    __syncthreads();
    if (threadIdx.x == 0) *((FB_LDS int*)slot) = atomicAdd(counter, 1);
    __syncthreads();
    return *((FB_LDS int*)slot);
  }
}

// One QP's slots of the seed and step blocks.
__device__ __forceinline__ DenseKktSlots dense_kkt_slots(const fbstab_multi_var_batch_t& seed,
                                                         const fbstab_multi_var_batch_t& step, int q) {
  DenseKktSlots s;
  for (int i = 0; i < 3; i++) {
    s.seed[i] = slot_or_null(seed.base[i], seed.stride[i], q);
    s.seed_rs[i] = seed.rhs_stride[i];
    s.step[i] = slot_or_null(step.base[i], step.stride[i], q);
    s.step_rs[i] = step.rhs_stride[i];
  }
  return s;
}

// One QP per workgroup, pulled from the queue like fbstab_dense_adjoint_kernel, whose instances, launch bounds and
// LDS layout these are: K is factored once per QP and the nrhs right-hand sides are solved one after the other on
// the stored factors.  `x`: the point (z, l, v); `seed`: nrhs vectors (gz, gl, gv) per QP, null l / v slots meaning
// zero - not read with wrt != kDenseKktSeeded, whose right-hand sides are the unit seeds of f, h or b; `step`: null
// slots, or nrhs vectors (dz, dl, dv) per QP.  kscratch: the handle's scratch (KGLOBAL: K, VGLOBAL: the iterate
// vectors behind it), not read otherwise.
template <int NT, bool KGLOBAL = false, bool VGLOBAL = false>
__global__ __launch_bounds__(NT, (NT > 64 ? 2 : 1)) void fbstab_dense_kkt_multi_kernel(
    DenseLayout lay, fbstab_dense_batch_t data, fbstab_var_batch_t x, fbstab_multi_var_batch_t seed,
    fbstab_multi_var_batch_t step, int* status, int nrhs, int wrt, double sigma, double alpha, int* counter, int batch,
    double* kscratch) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  lds_ptr lds = (lds_ptr)smem;
  typedef Ctx<NT> C;
  C ctx;
  ctx.tid = threadIdx.x;
  ctx.red = lds + lay.o_red;
  for (;;) {
    const int q = dense_kkt_next_qp<NT>(counter, lds + lay.o_slot);
    if (q >= batch) break;
    DenseProblem<C, KGLOBAL, VGLOBAL> p;
    double* ks = nullptr;
    if constexpr (KGLOBAL) ks = kscratch + (long)blockIdx.x * (lay.k_doubles + lay.v_doubles);
    p.bind(lay, dense_data_at(data, q), var_at(x, 0, q), var_at(x, 1, q), var_at(x, 2, q), nullptr, lds, ks);
    const bool ok = dense_kkt_multi(p, ctx, sigma, alpha, nrhs, wrt, dense_kkt_slots(seed, step, q));
    if (ctx.tid == 0) status[q] = ok ? 0 : 1;
    ctx.sync();
  }
}

// The one-wavefront policy: the launch bounds and the scratch of fbstab_dense_wave_adjoint_kernel (two wavefronts
// per SIMD; one region of lay.ws_doubles per workgroup).
constexpr int kDenseKktWaveMinWaves = 2;
__global__ __launch_bounds__(64, kDenseKktWaveMinWaves) void fbstab_dense_wave_kkt_multi_kernel(
    DenseWaveLayout lay, fbstab_dense_batch_t data, fbstab_var_batch_t x, fbstab_multi_var_batch_t seed,
    fbstab_multi_var_batch_t step, int* status, int nrhs, int wrt, double sigma, double alpha, int* counter, int batch,
    double* scratch) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  lds_ptr lds = (lds_ptr)smem;
  typedef DenseWave::C C;
  C ctx;
  ctx.tid = threadIdx.x;
  ctx.red = lds;  // (unused: one wavefront reduces in registers)
  double* ws = scratch + (long)blockIdx.x * lay.ws_doubles;
  for (;;) {
    const int q = dense_kkt_next_qp<64>(counter, lds);
    if (q >= batch) break;
    DenseWave p;
    p.bind(lay, dense_data_at(data, q), var_at(x, 0, q), var_at(x, 1, q), var_at(x, 2, q), nullptr, lds, ws, nullptr);
    const bool ok = dense_wave_kkt_multi(p, ctx, sigma, alpha, nrhs, wrt, dense_kkt_slots(seed, step, q));
    if (ctx.tid == 0) status[q] = ok ? 0 : 1;
    ctx.sync();
  }
}

}  // namespace fbk

// The kernel beside a handle's adjoint kernel, in the order of dense_resolve_kernels (fbstab_hip.hip): [0] the
// one-wavefront policy; the four-wavefront policy with [1] NT = 64, [2] K and the iterate vectors in global scratch,
// [3] K there, [4] everything in LDS.
__attribute__((visibility("hidden"))) const void* fbstab_dense_kkt_multi_kernel_for(int which) {
  constexpr int kThreads = 256;  // (kDenseThreads of fbstab_hip.hip)
  const void* const table[] = {reinterpret_cast<const void*>(fbk::fbstab_dense_wave_kkt_multi_kernel),
                               reinterpret_cast<const void*>(fbk::fbstab_dense_kkt_multi_kernel<64>),
                               reinterpret_cast<const void*>(fbk::fbstab_dense_kkt_multi_kernel<kThreads, true, true>),
                               reinterpret_cast<const void*>(fbk::fbstab_dense_kkt_multi_kernel<kThreads, true>),
                               reinterpret_cast<const void*>(fbk::fbstab_dense_kkt_multi_kernel<kThreads>)};
  return table[which];
}
