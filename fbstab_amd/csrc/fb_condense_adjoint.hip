// The kernels of fbstab_hip_mpc_condensed_adjoint_batch (fb_condense_adjoint.h), and the getter fbstab_hip.hip reaches
// them through.  A translation unit of its own, as fb_condense.hip is: the code of some kernels of fbstab_hip.hip
// depends on the order the compiler meets them (tools/diff_device_code.py).
#include <hip/hip_runtime.h>

#include "fb_condense_adjoint.h"

namespace fbk {

constexpr int kCondenseAdjointThreads = 256;

// One workgroup per QP: the seeds of the dense adjoint, and its point U.
template <int NT>
__global__ __launch_bounds__(NT) void fbstab_mpc_condense_seed_kernel(int N, int nx, int nu, int nc, CondenseLds o,
                                                                      fbstab_mpc_batch_t data, fbstab_var_batch_t x,
                                                                      fbstab_var_batch_t seed,
                                                                      CondenseAdjointWork work) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  lds_ptr lds = (lds_ptr)smem;
  Ctx<NT> ctx;
  ctx.tid = threadIdx.x;
  ctx.red = lds;
  const long q = blockIdx.x;
  const long nzc = (long)(N + 1) * nu, nv = (long)(N + 1) * nc;
  condense_adjoint_seed(ctx, N, nx, nu, nc, mpc_data_at(data, q), var_at(x, 0, q), var_at(seed, 0, q),
                        var_or_null(seed, 1, q), var_or_null(seed, 2, q), o, lds, work.U + q * nzc, work.gU + q * nzc,
                        work.gv + q * nv);
}

// One workgroup per QP: (dz, dl) from the dense adjoint's (dU, dv), and the gradients.  status: the dense
// adjoint's, 1 where its factorisation failed.
template <int NT>
__global__ __launch_bounds__(NT) void fbstab_mpc_condensed_adjoint_finish_kernel(
    int N, int nx, int nu, int nc, CondenseLds o, fbstab_mpc_batch_t data, fbstab_var_batch_t x,
    fbstab_var_batch_t seed, CondenseAdjointWork work, fbstab_mpc_grad_batch_t grad, fbstab_var_batch_t adj,
    const int* status) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  lds_ptr lds = (lds_ptr)smem;
  Ctx<NT> ctx;
  ctx.tid = threadIdx.x;
  ctx.red = lds;
  const long q = blockIdx.x;
  const long nzc = (long)(N + 1) * nu, nv = (long)(N + 1) * nc;
  condense_adjoint_finish(ctx, N, nx, nu, nc, mpc_data_at(data, q), var_at(x, 0, q), var_at(x, 1, q), var_at(x, 2, q),
                          var_at(seed, 0, q), var_or_null(seed, 1, q), work.dU + q * nzc, work.dv + q * nv, o, lds,
                          mpc_grad_or_null(grad, q), status[q] == 0, var_or_null(adj, 0, q), var_or_null(adj, 1, q),
                          var_or_null(adj, 2, q));
}

// One workgroup per QP, no LDS: rU, the z rows' residual of the dense step in hand (dU, dv).  Hc, Ac: the images of
// the condensed QP, stride 0 for a shared model.  sigma: the value the dense adjoint ran with.
template <int NT>
__global__ __launch_bounds__(NT) void fbstab_mpc_condensed_adjoint_residual_kernel(int nzc, int nv, const double* Hc,
                                                                                   long long sH, const double* Ac,
                                                                                   long long sA, double sigma,
                                                                                   CondenseAdjointWork work) {
  Ctx<NT> ctx;
  ctx.tid = threadIdx.x;
  ctx.red = nullptr;
  const long q = blockIdx.x;
  condense_adjoint_residual(ctx, nzc, nv, Hc + q * sH, Ac + q * sA, sigma, work.gU + q * nzc, work.dU + q * nzc,
                            work.dv + q * nv, work.rU + q * nzc);
}

// One workgroup per QP, no LDS: (dU, dv) += (eU, ev), the correction the dense adjoint returned for (rU, 0).
template <int NT>
__global__ __launch_bounds__(NT) void fbstab_mpc_condensed_adjoint_correct_kernel(int nzc, int nv,
                                                                                  CondenseAdjointWork work) {
  Ctx<NT> ctx;
  ctx.tid = threadIdx.x;
  ctx.red = nullptr;
  const long q = blockIdx.x;
  condense_adjoint_correct(ctx, nzc, nv, work.eU + q * nzc, work.ev + q * nv, work.dU + q * nzc, work.dv + q * nv);
}

}  // namespace fbk

// *threads: the workgroup size of all four.
__attribute__((visibility("hidden"))) const void* fbstab_condense_kernel(fbk::CondenseAdjointKernel which, int* threads) {
  *threads = fbk::kCondenseAdjointThreads;
  if (which == fbk::kCondenseAdjSeed)
    return reinterpret_cast<const void*>(fbk::fbstab_mpc_condense_seed_kernel<fbk::kCondenseAdjointThreads>);
  if (which == fbk::kCondenseAdjResidual)
    return reinterpret_cast<const void*>(fbk::fbstab_mpc_condensed_adjoint_residual_kernel<fbk::kCondenseAdjointThreads>);
  if (which == fbk::kCondenseAdjCorrect)
    return reinterpret_cast<const void*>(fbk::fbstab_mpc_condensed_adjoint_correct_kernel<fbk::kCondenseAdjointThreads>);
  return reinterpret_cast<const void*>(fbk::fbstab_mpc_condensed_adjoint_finish_kernel<fbk::kCondenseAdjointThreads>);
}
