// The kernel of fbstab_hip_mpc_kkt_solve_batch and fbstab_hip_mpc_x0_sensitivity_batch (fb_kkt_multi.h), and the
// factory fbstab_hip.hip's kernel table calls.  A translation unit of its own: the code of some kernels of
// fbstab_hip.hip depends on the order the compiler meets them (mpc_resolve_kernels; tools/diff_device_code.py).
#include <hip/hip_runtime.h>

#include "fb_kkt_multi.h"

namespace fbk {

// One QP per workgroup (one wavefront), pulled from the queue like fbstab_mpc_adjoint_kernel: V is factored once per
// QP, and the nrhs right-hand sides are solved one after the other on the stored factors.  `x`: the point (z, l, v);
// `seed`: nrhs vectors (gz, gl, gv) per QP, null l / v slots meaning zero - not read with x0_mode, whose nrhs = nx
// right-hand sides are the unit directions of the initial state; `step`: null slots, or nrhs vectors (dz, dl, dv)
// per QP; gain: null, or nu x nx doubles per QP.  WG: the stage tile and the work matrices in global scratch
// (MpcLayout::wglobal).
template <int NT, bool WG>
__global__ __launch_bounds__(NT, 1) void fbstab_mpc_kkt_multi_kernel(
    MpcLayout lay, fbstab_mpc_batch_t data, fbstab_var_batch_t x, fbstab_multi_var_batch_t seed,
    fbstab_multi_var_batch_t step, double* gain, long long gain_stride, int* status, int nrhs, int x0_mode,
    double sigma, double alpha, double* scratch, int* counter, int batch) {
  static_assert(NT == 64, "one wavefront per QP: the queue word is broadcast by a shuffle");
  extern __shared__ __attribute__((aligned(16))) double smem[];
  lds_ptr lds = (lds_ptr)smem;
  typedef Ctx<NT> C;
  C ctx;
  ctx.tid = threadIdx.x;
  ctx.red = WG ? lds : lds + lay.w_red;
  double* ws = scratch + (long)blockIdx.x * lay.ws_doubles;
  for (;;) {
    int q = 0;
    if (threadIdx.x == 0) q = atomicAdd(counter, 1);
    q = __shfl(q, 0, 64);
    if (q >= batch) break;
    MpcProblem<C, WG> p;
    typename MpcProblem<C, WG>::mptr mb;
    if constexpr (WG) mb = ws + lay.v_carve;
    else mb = lds;
    p.bind(lay, mpc_data_at(data, q), var_at(x, 0, q), var_at(x, 1, q), var_at(x, 2, q), nullptr, mb, ws);
    KktMultiSlots s;
    for (int i = 0; i < 3; i++) {
      s.seed[i] = slot_or_null(seed.base[i], seed.stride[i], q);
      s.seed_rs[i] = seed.rhs_stride[i];
      s.step[i] = slot_or_null(step.base[i], step.stride[i], q);
      s.step_rs[i] = step.rhs_stride[i];
    }
    s.gain = slot_or_null(gain, gain_stride, q);
    const bool ok = mpc_kkt_multi(p, ctx, sigma, alpha, nrhs, x0_mode != 0, s);
    if (ctx.tid == 0) status[q] = ok ? 0 : 1;
    ctx.sync();
  }
}

}  // namespace fbk

// The kernel for a layout: [wglobal != 0] the stage tile and the work matrices in global scratch, or everything in
// LDS.
__attribute__((visibility("hidden"))) const void* fbstab_kkt_multi_kernel(int wglobal) {
  return wglobal ? reinterpret_cast<const void*>(fbk::fbstab_mpc_kkt_multi_kernel<64, true>)
                 : reinterpret_cast<const void*>(fbk::fbstab_mpc_kkt_multi_kernel<64, false>);
}
