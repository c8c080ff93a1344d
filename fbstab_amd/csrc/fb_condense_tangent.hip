// The direction kernel of fbstab_hip_mpc_condensed_tangent_batch (fb_tangent.h: mpc_tangent_stage on the blocks of the
// condensed route), and the getter fbstab_hip.hip reaches it through.  A translation unit of its own, as fb_condense.hip
// is: the code of some kernels of fbstab_hip.hip depends on the order the compiler meets them
// (tools/diff_device_code.py).
#include <hip/hip_runtime.h>

#include "fb_condense_plan.h"
#include "fb_tangent.h"

namespace fbk {

// Four wavefronts per (QP, stage).  Measured at (10, 40, 3, 6), 2048 QPs, all 12 sequences perturbed, both
// instantiations alternating in one process: the kernel takes 0.311 ms with 256 threads against 0.474 ms with 64, the
// whole call 1.88 ms against 2.07 ms (LABNOTES.md, "The condensed tangent") - a stage's 30 KB of images are some 30 load
// trips of one wavefront and 8 of four.  The 64-thread instantiation is retired.
constexpr int kCondenseTangentThreads = 256;

// One workgroup per (QP, stage): the seeds (gz, gl, gv) of the tangent system from the perturbations `dir` (a null
// base: zero; stride 0: one direction for the batch) and the point `x`.  No handle, no queue, no scratch, no atomics:
// a workgroup's QP and stage are its index, and every output entry is summed by one thread in ascending order, so the
// bits are those of fbstab_tangent_rhs_kernel (one wavefront per stage) whatever NT is.
template <int NT>
__global__ __launch_bounds__(NT) void fbstab_mpc_condensed_tangent_rhs_kernel(int N, int nx, int nu, int nc,
                                                                              MpcTangentLds o, fbstab_mpc_batch_t dir,
                                                                              fbstab_var_batch_t x,
                                                                              fbstab_var_batch_t seed) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  Ctx<NT> ctx;
  ctx.tid = threadIdx.x;
  ctx.red = (lds_ptr)smem;  // (unused)
  const long q = blockIdx.x / (N + 1);
  const int i = blockIdx.x % (N + 1);
  mpc_tangent_stage(ctx, N, nx, nu, nc, i, mpc_data_or_null(dir, q), var_at(x, 0, q), var_at(x, 1, q), var_at(x, 2, q),
                    o, (lds_ptr)smem, var_at(seed, 0, q), var_at(seed, 1, q), var_at(seed, 2, q));
}

}  // namespace fbk

// *threads: its workgroup size.
__attribute__((visibility("hidden"))) const void* fbstab_condense_kernel(fbk::CondenseTangentKernel, int* threads) {
  *threads = fbk::kCondenseTangentThreads;
  return reinterpret_cast<const void*>(fbk::fbstab_mpc_condensed_tangent_rhs_kernel<fbk::kCondenseTangentThreads>);
}
