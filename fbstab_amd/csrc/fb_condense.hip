// The kernels of fbstab_hip_mpc_condense_batch and fbstab_hip_mpc_expand_batch (fb_condense.h), and the getter
// fbstab_hip.hip reaches them through.  A translation unit of its own, as fb_kkt_multi.hip is: the code of some
// kernels of fbstab_hip.hip depends on the order the compiler meets them (tools/diff_device_code.py).
#include <hip/hip_runtime.h>

#include "fb_condense.h"

namespace fbk {

constexpr int kCondenseThreads = 256;

// One workgroup per (QP, column block k): block q (N + 1) + k.  An image with stride 0 is the one image of a batch
// that shares its model: QP 0 writes it (the entry point launches QP 0 alone where both are shared).
template <int NT>
__global__ __launch_bounds__(NT) void fbstab_mpc_condense_matrices_kernel(int N, int nx, int nu, int nc,
                                                                          CondenseLds o, fbstab_mpc_batch_t data,
                                                                          fbstab_dense_out_batch_t out) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  lds_ptr lds = (lds_ptr)smem;
  Ctx<NT> ctx;
  ctx.tid = threadIdx.x;
  ctx.red = lds;
  const long q = blockIdx.x / (unsigned)(N + 1);
  const int k = blockIdx.x % (unsigned)(N + 1);
  double* H = out.base[FBSTAB_DENSE_H];
  double* A = out.base[FBSTAB_DENSE_A];
  if (H) H = (q > 0 && out.stride[FBSTAB_DENSE_H] == 0) ? nullptr : H + q * out.stride[FBSTAB_DENSE_H];
  if (A) A = (q > 0 && out.stride[FBSTAB_DENSE_A] == 0) ? nullptr : A + q * out.stride[FBSTAB_DENSE_A];
  condense_matrices(ctx, N, nx, nu, nc, k, mpc_data_at(data, q), o, lds, H, A);
}

// One workgroup per QP.
template <int NT>
__global__ __launch_bounds__(NT) void fbstab_mpc_condense_vectors_kernel(int N, int nx, int nu, int nc,
                                                                         CondenseLds o, fbstab_mpc_batch_t data,
                                                                         fbstab_dense_out_batch_t out) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  lds_ptr lds = (lds_ptr)smem;
  Ctx<NT> ctx;
  ctx.tid = threadIdx.x;
  ctx.red = lds;
  const long q = blockIdx.x;
  condense_vectors(ctx, N, nx, nu, nc, mpc_data_at(data, q), o, lds,
                   slot_or_null(out.base[FBSTAB_DENSE_f], out.stride[FBSTAB_DENSE_f], q),
                   slot_or_null(out.base[FBSTAB_DENSE_b], out.stride[FBSTAB_DENSE_b], q));
}

// One workgroup per QP: xc holds (U, -, v_c, y_c), x receives (z, l, v, y).
template <int NT>
__global__ __launch_bounds__(NT) void fbstab_mpc_expand_kernel(int N, int nx, int nu, int nc, CondenseLds o,
                                                               fbstab_mpc_batch_t data, fbstab_var_batch_t xc,
                                                               fbstab_var_batch_t x) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  lds_ptr lds = (lds_ptr)smem;
  Ctx<NT> ctx;
  ctx.tid = threadIdx.x;
  ctx.red = lds;
  const long q = blockIdx.x;
  condense_expand(ctx, N, nx, nu, nc, mpc_data_at(data, q), var_at(xc, 0, q), var_at(xc, 2, q),
                  var_or_null(xc, 3, q), o, lds, var_or_null(x, 0, q), var_or_null(x, 1, q), var_or_null(x, 2, q),
                  var_or_null(x, 3, q));
}

}  // namespace fbk

// *threads: the workgroup size of all three.
__attribute__((visibility("hidden"))) const void* fbstab_condense_kernel(fbk::CondenseKernel which, int* threads) {
  *threads = fbk::kCondenseThreads;
  switch (which) {
    case fbk::kCondenseMatrices: return reinterpret_cast<const void*>(fbk::fbstab_mpc_condense_matrices_kernel<fbk::kCondenseThreads>);
    case fbk::kCondenseVectors: return reinterpret_cast<const void*>(fbk::fbstab_mpc_condense_vectors_kernel<fbk::kCondenseThreads>);
    default: return reinterpret_cast<const void*>(fbk::fbstab_mpc_expand_kernel<fbk::kCondenseThreads>);
  }
}
