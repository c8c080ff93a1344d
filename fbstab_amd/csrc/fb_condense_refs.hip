// The kernel of fbstab_hip_mpc_condensed_reference_images_batch (fb_condense_refs.h), and the getter fbstab_hip.hip
// reaches it through.  A translation unit of its own, as fb_condense_multi.hip is: the code of some kernels of
// fbstab_hip.hip depends on the order the compiler meets them (tools/diff_device_code.py).
#include <hip/hip_runtime.h>

#include "fb_condense_refs.h"

namespace fbk {

constexpr int kCondenseRefsThreads = 256;

// The grid is batch x ceil(steps / R), workgroup b * groups + g: steps g R .. of trajectory b, the last group partial.
// refs: no null slot (the host stage puts `data`'s sequence, step 0, where the caller gave none); data's q, r, c, d
// and x0 slots are not read.
template <int NT>
__global__ __launch_bounds__(NT) void fbstab_mpc_condense_reference_kernel(int N, int nx, int nu, int nc, CondenseLds o,
                                                                           int steps, int R, long long per,
                                                                           fbstab_mpc_batch_t data,
                                                                           fbstab_condensed_refs_t refs,
                                                                           fbstab_condensed_ref_images_t images) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  lds_ptr lds = (lds_ptr)smem;
  Ctx<NT> ctx;
  ctx.tid = threadIdx.x;
  ctx.red = lds;
  const int groups = (steps + R - 1) / R;
  const int g = (int)(blockIdx.x % (unsigned)groups);
  const long b = (long)(blockIdx.x / (unsigned)groups);
  const int k0 = g * R;
  const int Rg = steps - k0 < R ? steps - k0 : R;
  MpcData D;
  D.Q = slot_at(data.base[FBSTAB_MPC_Q], data.stride[FBSTAB_MPC_Q], b);
  D.R = slot_at(data.base[FBSTAB_MPC_R], data.stride[FBSTAB_MPC_R], b);
  D.S = slot_at(data.base[FBSTAB_MPC_S], data.stride[FBSTAB_MPC_S], b);
  D.A = slot_at(data.base[FBSTAB_MPC_A], data.stride[FBSTAB_MPC_A], b);
  D.B = slot_at(data.base[FBSTAB_MPC_B], data.stride[FBSTAB_MPC_B], b);
  D.E = slot_at(data.base[FBSTAB_MPC_E], data.stride[FBSTAB_MPC_E], b);
  D.L = slot_at(data.base[FBSTAB_MPC_L], data.stride[FBSTAB_MPC_L], b);
  D.q = D.r = D.c = D.d = D.x0 = nullptr;
  CondenseRefSeqs rs;
  rs.sq = refs.step[0]; rs.sr = refs.step[1]; rs.sc = refs.step[2]; rs.sd = refs.step[3];
  rs.q = refs.base[0] + b * refs.stride[0] + k0 * rs.sq;
  rs.r = refs.base[1] + b * refs.stride[1] + k0 * rs.sr;
  rs.c = refs.base[2] + b * refs.stride[2] + k0 * rs.sc;
  rs.d = refs.base[3] + b * refs.stride[3] + k0 * rs.sd;
  condense_reference_vectors(ctx, N, nx, nu, nc, D, rs, Rg, (long)per, o, lds,
                             images.f0 + b * images.stride_f0 + k0 * images.step_f0, images.step_f0,
                             images.b0 + b * images.stride_b0 + k0 * images.step_b0, images.step_b0);
}

}  // namespace fbk

// *threads: the workgroup size.
__attribute__((visibility("hidden"))) const void* fbstab_condense_kernel(fbk::CondenseRefsKernel which, int* threads) {
  (void)which;
  *threads = fbk::kCondenseRefsThreads;
  return reinterpret_cast<const void*>(fbk::fbstab_mpc_condense_reference_kernel<fbk::kCondenseRefsThreads>);
}
