// The kernels of fbstab_hip_mpc_condensed_receding_sweep_adjoint (fb_condense_sweep_adjoint.h), and the getter
// fbstab_hip.hip reaches them through.  A translation unit of its own, as fb_condense_sweep.hip is: the code of some
// kernels of fbstab_hip.hip depends on the order the compiler meets them (tools/diff_device_code.py).
#include <hip/hip_runtime.h>

#include "fb_condense_sweep_adjoint.h"

namespace fbk {

constexpr int kCondenseSweepAdjointThreads = 256;

// One workgroup per L.T trajectories: closes step k + 1 and opens step k.
template <int NT>
__global__ __launch_bounds__(NT) void fbstab_mpc_condensed_sweep_adjoint_step_kernel(CondenseSweepAdjStep a,
                                                                                     CondenseSweepLds L) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  lds_ptr lds = (lds_ptr)smem;
  Ctx<NT> ctx;
  ctx.tid = threadIdx.x;
  ctx.red = lds;
  const long t0 = (long)blockIdx.x * L.T;
  const int Tg = a.batch - t0 < L.T ? (int)(a.batch - t0) : L.T;
  condense_sweep_adjoint_step(ctx, a, L, t0, Tg, lds);
}

// One workgroup per trajectory, behind the refinement of a step: the gradients of the 11 sequences, added to the slots.
template <int NT>
__global__ __launch_bounds__(NT) void fbstab_mpc_condensed_sweep_adjoint_finish_kernel(
    int N, int nx, int nu, int nc, CondenseLds o, fbstab_mpc_batch_t data, CondenseSweepAdjFinish a,
    fbstab_mpc_grad_batch_t grad) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  lds_ptr lds = (lds_ptr)smem;
  Ctx<NT> ctx;
  ctx.tid = threadIdx.x;
  ctx.red = lds;
  const long q = blockIdx.x;
  const long nzc = (long)(N + 1) * nu, nv = (long)(N + 1) * nc, nz = (long)(N + 1) * (nx + nu), nl = (long)(N + 1) * nx;
  MpcData D = mpc_data_at(data, q);
  D.x0 = a.x + q * nx;
  MpcGrad G = mpc_grad_or_null(grad, q);
  G.x0 = a.dl0 ? a.dl0 + q * nx : nullptr;
  const bool ok = a.eflag[q] == FBSTAB_SUCCESS && a.st1[q] == 0 && a.st2[q] == 0;
  condense_sweep_adjoint_finish(ctx, N, nx, nu, nc, D, a.U + q * nzc, a.v + q * nv, a.dU + q * nzc, a.dv + q * nv,
                                a.gz + q * nz, o, lds, G, ok, a.z + q * nz, a.l + q * nl);
}

// One workgroup per trajectory, before the first step: zeros where the sums start.  gz, gf0, gb0: null, or packed.
template <int NT>
__global__ __launch_bounds__(NT) void fbstab_mpc_condensed_sweep_adjoint_begin_kernel(int N, int nx, int nu, int nc,
                                                                                      fbstab_mpc_grad_batch_t grad,
                                                                                      double* gz, double* gf0,
                                                                                      double* gb0, int* status) {
  Ctx<NT> ctx;
  ctx.tid = threadIdx.x;
  ctx.red = nullptr;
  const long q = blockIdx.x;
  const long nzc = (long)(N + 1) * nu, nv = (long)(N + 1) * nc, nz = (long)(N + 1) * (nx + nu);
  condense_sweep_adjoint_begin(ctx, N, nx, nu, nc, mpc_grad_or_null(grad, q), gz ? gz + q * nz : nullptr,
                               gf0 ? gf0 + q * nzc : nullptr, gb0 ? gb0 + q * nv : nullptr, status + q);
}

}  // namespace fbk

// *threads: the workgroup size of all three.
__attribute__((visibility("hidden"))) const void* fbstab_condense_kernel(fbk::CondenseSweepAdjKernel which, int* threads) {
  *threads = fbk::kCondenseSweepAdjointThreads;
  switch (which) {
    case fbk::kCondenseSweepAdjStep:
      return reinterpret_cast<const void*>(
          fbk::fbstab_mpc_condensed_sweep_adjoint_step_kernel<fbk::kCondenseSweepAdjointThreads>);
    case fbk::kCondenseSweepAdjFinish:
      return reinterpret_cast<const void*>(
          fbk::fbstab_mpc_condensed_sweep_adjoint_finish_kernel<fbk::kCondenseSweepAdjointThreads>);
    default:
      return reinterpret_cast<const void*>(
          fbk::fbstab_mpc_condensed_sweep_adjoint_begin_kernel<fbk::kCondenseSweepAdjointThreads>);
  }
}
