// The kernels of fbstab_hip_mpc_condensed_kkt_solve_batch / fbstab_hip_mpc_condensed_x0_sensitivity_batch
// (fb_condense_multi.h), and the getter fbstab_hip.hip reaches them through.  A translation unit of its own, as
// fb_condense_adjoint.hip is: the code of some kernels of fbstab_hip.hip depends on the order the compiler meets them
// (tools/diff_device_code.py).
//
// All four run on the grid batch x ceil(nrhs / R), workgroup q * groups + g: right-hand sides g R .. of QP q.
#include <hip/hip_runtime.h>

#include "fb_condense_multi.h"

namespace fbk {

constexpr int kCondenseMultiThreads = 256;

// Which QP and which right-hand sides a workgroup takes.
struct CondenseMultiGroup {
  long q;
  int k0, Rg;
};
__device__ __forceinline__ CondenseMultiGroup condense_multi_group(int nrhs, int R) {
  const int groups = (nrhs + R - 1) / R;
  const int g = (int)(blockIdx.x % (unsigned)groups);
  CondenseMultiGroup w;
  w.q = (long)(blockIdx.x / (unsigned)groups);
  w.k0 = g * R;
  w.Rg = nrhs - w.k0 < R ? nrhs - w.k0 : R;
  return w;
}

__device__ __forceinline__ CondenseMultiSeeds condense_multi_seeds(const fbstab_multi_var_batch_t& seed, int x0_mode,
                                                                   long q) {
  CondenseMultiSeeds sd;
  sd.gz = slot_or_null((const double*)seed.base[0], seed.stride[0], q);
  sd.gl = slot_or_null((const double*)seed.base[1], seed.stride[1], q);
  sd.gv = slot_or_null((const double*)seed.base[2], seed.stride[2], q);
  sd.rz = seed.rhs_stride[0]; sd.rl = seed.rhs_stride[1]; sd.rv = seed.rhs_stride[2];
  sd.x0_mode = x0_mode;
  return sd;
}

// The seeds (gU, gv_c) of the dense multi-solve for R right-hand sides of one QP; the workgroup that holds right-hand
// side 0 also writes U.  x0_mode != 0: `seed` is not read.
template <int NT>
__global__ __launch_bounds__(NT) void fbstab_mpc_condense_multi_seed_kernel(
    int N, int nx, int nu, int nc, CondenseLds o, int nrhs, int R, long long per, int x0_mode,
    fbstab_mpc_batch_t data, fbstab_var_batch_t x, fbstab_multi_var_batch_t seed, CondenseMultiWork work) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  lds_ptr lds = (lds_ptr)smem;
  Ctx<NT> ctx;
  ctx.tid = threadIdx.x;
  ctx.red = lds;
  const CondenseMultiGroup g = condense_multi_group(nrhs, R);
  const long nzc = (long)(N + 1) * nu, nv = (long)(N + 1) * nc;
  condense_multi_seed(ctx, N, nx, nu, nc, mpc_data_at(data, g.q), var_at(x, 0, g.q),
                      condense_multi_seeds(seed, x0_mode, g.q), g.k0, g.Rg, (long)per, o, lds,
                      g.k0 == 0 ? work.U + g.q * nzc : (double*)nullptr, work.gU + g.q * nrhs * nzc,
                      work.gv + g.q * nrhs * nv);
}

// No LDS: rU, the z rows' residual of the dense step in hand, for R right-hand sides of one QP.  Hc, Ac: the images of
// the condensed QP, stride 0 for a shared model.  sigma: the value the dense multi-solve ran with.
template <int NT>
__global__ __launch_bounds__(NT) void fbstab_mpc_condense_multi_residual_kernel(int nzc, int nv, int nrhs, int R,
                                                                                const double* Hc, long long sH,
                                                                                const double* Ac, long long sA,
                                                                                double sigma, CondenseMultiWork work) {
  Ctx<NT> ctx;
  ctx.tid = threadIdx.x;
  ctx.red = nullptr;
  const CondenseMultiGroup g = condense_multi_group(nrhs, R);
  const long u = (g.q * nrhs + g.k0) * nzc, v = (g.q * nrhs + g.k0) * nv;
  condense_multi_residual(ctx, nzc, nv, g.Rg, Hc + g.q * sH, Ac + g.q * sA, sigma, work.gU + u, work.dU + u,
                          work.dv + v, work.rU + u);
}

// No LDS: (dU, dv) += (eU, ev), the correction the dense multi-solve returned for (rU, 0); gain (x0 mode, may be
// null): the u_0 rows of the corrected dU, nu x nx column-major per QP.
template <int NT>
__global__ __launch_bounds__(NT) void fbstab_mpc_condense_multi_correct_kernel(int nzc, int nv, int nu, int nrhs,
                                                                               int R, CondenseMultiWork work,
                                                                               double* gain, long long gain_stride,
                                                                               const int* status) {
  Ctx<NT> ctx;
  ctx.tid = threadIdx.x;
  ctx.red = nullptr;
  const CondenseMultiGroup g = condense_multi_group(nrhs, R);
  const long u = (g.q * nrhs + g.k0) * nzc, v = (g.q * nrhs + g.k0) * nv;
  condense_multi_correct(ctx, nzc, nv, nu, g.k0, g.Rg, work.eU + u, work.ev + v, work.dU + u, work.dv + v,
                         slot_or_null(gain, gain_stride, g.q), status[g.q] == 0);
}

// (dz, dl, dv) of R right-hand sides of one QP into the caller's step slots.  status: the dense multi-solve's, 1
// where its factorisation failed.
template <int NT>
__global__ __launch_bounds__(NT) void fbstab_mpc_condense_multi_finish_kernel(
    int N, int nx, int nu, int nc, CondenseLds o, int nrhs, int R, long long per, int x0_mode,
    fbstab_mpc_batch_t data, fbstab_multi_var_batch_t seed, CondenseMultiWork work, fbstab_multi_var_batch_t step,
    const int* status) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  lds_ptr lds = (lds_ptr)smem;
  Ctx<NT> ctx;
  ctx.tid = threadIdx.x;
  ctx.red = lds;
  const CondenseMultiGroup g = condense_multi_group(nrhs, R);
  const long nzc = (long)(N + 1) * nu, nv = (long)(N + 1) * nc;
  condense_multi_finish(ctx, N, nx, nu, nc, mpc_data_at(data, g.q), condense_multi_seeds(seed, x0_mode, g.q), g.k0,
                        g.Rg, (long)per, work.dU + g.q * nrhs * nzc, work.dv + g.q * nrhs * nv, o, lds,
                        status[g.q] == 0, slot_or_null(step.base[0], step.stride[0], g.q), step.rhs_stride[0],
                        slot_or_null(step.base[1], step.stride[1], g.q), step.rhs_stride[1],
                        slot_or_null(step.base[2], step.stride[2], g.q), step.rhs_stride[2]);
}

}  // namespace fbk

// *threads: the workgroup size of all four.
__attribute__((visibility("hidden"))) const void* fbstab_condense_kernel(fbk::CondenseMultiKernel which, int* threads) {
  *threads = fbk::kCondenseMultiThreads;
  if (which == fbk::kCondenseMultiSeed)
    return reinterpret_cast<const void*>(fbk::fbstab_mpc_condense_multi_seed_kernel<fbk::kCondenseMultiThreads>);
  if (which == fbk::kCondenseMultiResidual)
    return reinterpret_cast<const void*>(fbk::fbstab_mpc_condense_multi_residual_kernel<fbk::kCondenseMultiThreads>);
  if (which == fbk::kCondenseMultiCorrect)
    return reinterpret_cast<const void*>(fbk::fbstab_mpc_condense_multi_correct_kernel<fbk::kCondenseMultiThreads>);
  return reinterpret_cast<const void*>(fbk::fbstab_mpc_condense_multi_finish_kernel<fbk::kCondenseMultiThreads>);
}
