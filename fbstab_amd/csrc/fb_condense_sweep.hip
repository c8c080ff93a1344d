// The kernels of fbstab_hip_mpc_condensed_x0_map_batch and fbstab_hip_mpc_condensed_receding_sweep
// (fb_condense_sweep.h), and the getter fbstab_hip.hip reaches them through.  A translation unit of its own, as
// fb_condense_multi.hip is: the code of some kernels of fbstab_hip.hip depends on the order the compiler meets them
// (tools/diff_device_code.py).
#include <hip/hip_runtime.h>

#include "fb_condense_sweep.h"

namespace fbk {

constexpr int kCondenseSweepThreads = 256;

// One workgroup per (QP, block of at most nu columns of x0): block q blocks + g, blocks = ceil(nx / nu).  map_stride 0:
// the one image of a batch that shares its model (the entry point launches QP 0 alone).
template <int NT>
__global__ __launch_bounds__(NT) void fbstab_mpc_condense_x0_map_kernel(int N, int nx, int nu, int nc, CondenseLds o,
                                                                        fbstab_mpc_batch_t data, double* map,
                                                                        long long map_stride) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  lds_ptr lds = (lds_ptr)smem;
  Ctx<NT> ctx;
  ctx.tid = threadIdx.x;
  ctx.red = lds;
  const unsigned blocks = (unsigned)((nx + nu - 1) / nu);
  const long q = blockIdx.x / blocks;
  const int c0 = (int)(blockIdx.x % blocks) * nu;
  const int ncol = nx - c0 < nu ? nx - c0 : nu;
  condense_x0_map(ctx, N, nx, nu, nc, c0, ncol, mpc_data_at(data, q), o, lds, map + q * map_stride);
}

// One workgroup per L.T trajectories, behind the dense solve of a step.
template <int NT>
__global__ __launch_bounds__(NT) void fbstab_mpc_condensed_sweep_step_kernel(CondenseSweepStep a, CondenseSweepLds L) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  lds_ptr lds = (lds_ptr)smem;
  Ctx<NT> ctx;
  ctx.tid = threadIdx.x;
  ctx.red = lds;
  const long t0 = (long)blockIdx.x * L.T;
  const int Tg = a.batch - t0 < L.T ? (int)(a.batch - t0) : L.T;
  condense_sweep_step(ctx, a, L, t0, Tg, lds);
}

// One workgroup per trajectory, before the first step: the guess (U, v) from the caller's (z, -, v, -).
template <int NT>
__global__ __launch_bounds__(NT) void fbstab_mpc_condensed_sweep_begin_kernel(int N, int nx, int nu, int nc,
                                                                              fbstab_var_batch_t x, double* U,
                                                                              double* v, int* gone) {
  Ctx<NT> ctx;
  ctx.tid = threadIdx.x;
  ctx.red = nullptr;
  const long q = blockIdx.x;
  condense_sweep_begin(ctx, N, nx, nu, nc, var_at(x, 0, q), var_at(x, 2, q), U + q * (long)(N + 1) * nu,
                       v + q * (long)(N + 1) * nc, gone + q);
}

}  // namespace fbk

// *threads: the workgroup size of all three.
__attribute__((visibility("hidden"))) const void* fbstab_condense_kernel(fbk::CondenseSweepKernel which, int* threads) {
  *threads = fbk::kCondenseSweepThreads;
  switch (which) {
    case fbk::kCondenseSweepX0Map: return reinterpret_cast<const void*>(fbk::fbstab_mpc_condense_x0_map_kernel<fbk::kCondenseSweepThreads>);
    case fbk::kCondenseSweepStep: return reinterpret_cast<const void*>(fbk::fbstab_mpc_condensed_sweep_step_kernel<fbk::kCondenseSweepThreads>);
    default: return reinterpret_cast<const void*>(fbk::fbstab_mpc_condensed_sweep_begin_kernel<fbk::kCondenseSweepThreads>);
  }
}
