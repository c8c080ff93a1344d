// The kernel of fbstab_hip_mpc_condensed_receding_sweep_tangent (fb_condense_sweep_tangent.h), and the getter
// fbstab_hip.hip reaches it through.  A translation unit of its own, as fb_condense_sweep_adjoint.hip is: the code of
// some kernels of fbstab_hip.hip depends on the order the compiler meets them (tools/diff_device_code.py).
#include <hip/hip_runtime.h>

#include "fb_condense_sweep_tangent.h"

namespace fbk {

constexpr int kCondenseSweepTangentThreads = 256;

// One workgroup per L.T trajectories: closes step k and opens step k + 1.
template <int NT>
__global__ __launch_bounds__(NT) void fbstab_mpc_condensed_sweep_tangent_step_kernel(CondenseSweepTanStep a,
                                                                                     CondenseSweepLds L) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  lds_ptr lds = (lds_ptr)smem;
  Ctx<NT> ctx;
  ctx.tid = threadIdx.x;
  ctx.red = lds;
  const long t0 = (long)blockIdx.x * L.T;
  const int Tg = a.batch - t0 < L.T ? (int)(a.batch - t0) : L.T;
  condense_sweep_tangent_step(ctx, a, L, t0, Tg, lds);
}

}  // namespace fbk

// *threads: the workgroup size.
__attribute__((visibility("hidden"))) const void* fbstab_condense_kernel(fbk::CondenseSweepTanKernel, int* threads) {
  *threads = fbk::kCondenseSweepTangentThreads;
  return reinterpret_cast<const void*>(
      fbk::fbstab_mpc_condensed_sweep_tangent_step_kernel<fbk::kCondenseSweepTangentThreads>);
}
