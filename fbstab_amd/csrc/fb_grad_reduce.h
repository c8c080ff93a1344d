// Gradients summed over the batch (fbstab_hip_*_adjoint_batch_reduced): for data shared by every QP of a batch
// the gradient is sum_b of the per-QP gradients, and each of those is a function of the point (z, l, v) and the
// adjoint step (dz, dl, dv) alone (fb_adjoint.h).  With X = [Z L V] and P = [DZ DL DV], one QP per row,
//     M = -(P'Z + X'DZ)
// holds every matrix gradient and the column sums of P every vector gradient: matrix products whose inner
// dimension is the batch.  fb_grad_reduce_plan.h cuts M into 16 x 16 tiles and names what each entry is.
//
// fbstab_grad_reduce_kernel: one wavefront per (tile, chunk of kGradReduceChunk QPs), v_mfma_f64_16x16x4: lane
// 16 k + m supplies A(m, k) = P[b0 + k][row m] and B(k, n) = Z[b0 + k][col n] (n = m), then X and DZ into the same
// accumulator, four QPs per trip in ascending order; the sixteen lanes of a quarter-wave read one QP's
// contiguous rows.  The row sums ride along as a third product with a column of ones.  Outside the tile's edge,
// beyond the batch and for a QP that is left out (adjoint status 1, or a solve that did not end in SUCCESS) a
// lane supplies 0.0 by a SELECT on both operands: no address is formed, and nothing is multiplied by zero (a
// point that is left out may hold NaN or Inf).  The partial goes to the slot of its (tile, chunk) by plain stores.
// fbstab_grad_reduce_finish_kernel, the next launch on the stream: one workgroup per tile adds its slots in
// ascending chunk order, applies -1, -1/2 or +1 and writes the caller's array.  No atomics, no counters: the
// bits depend on the inputs and on the batch size only.
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/fbstab_types.h"
#include "fb_grad_reduce_plan.h"

namespace fbk {

constexpr int kGradReduceUnroll = 4;  // (kGradReduceChunk is a multiple of 4 x this)
static_assert(kGradReduceChunk % (4 * kGradReduceUnroll) == 0, "whole trips per chunk");

typedef double grad_reduce_d4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(64) void fbstab_grad_reduce_kernel(GradReduceArgs a) {
  const int chunks = (int)grad_reduce_chunks(a.batch);
  const int tile = blockIdx.x / chunks, chunk = blockIdx.x % chunks;
  const int lane = threadIdx.x, m = lane & 15, k = lane >> 4;
  int g, rt, ct;
  grad_reduce_tile(a.plan, tile, &g, &rt, &ct);
  const int r = rt * kGradReduceTile + m, c = ct * kGradReduceTile + m;
  const bool row_in = r < grad_reduce_group_rows(a.plan, g), col_in = c < grad_reduce_group_cols(a.plan, g);
  const double *pr = nullptr, *xr = nullptr, *zc = nullptr, *dzc = nullptr;
  long long prs = 0, xrs = 0;
  if (row_in) {
    int arr, off;
    grad_reduce_row(a.plan, g, r, &arr, &off);
    pr = a.p[arr] + off; prs = a.ps[arr];
    xr = a.x[arr] + off; xrs = a.xs[arr];
  }
  if (col_in) {
    const int off = grad_reduce_col(a.plan, g, c);
    zc = a.x[0] + off;
    dzc = a.p[0] + off;
  }
  const int b0 = chunk * kGradReduceChunk;
  const int b1 = b0 + kGradReduceChunk < a.batch ? b0 + kGradReduceChunk : a.batch;
  const bool sums = ct == 0;  // (wave-uniform)
  grad_reduce_d4 acc = {0.0, 0.0, 0.0, 0.0}, vec = {0.0, 0.0, 0.0, 0.0};
  // kGradReduceUnroll trips' worth of loads are issued before their products; the products stay in ascending order
  for (int bb = b0; bb < b1; bb += 4 * kGradReduceUnroll) {
    double pa[kGradReduceUnroll], xa[kGradReduceUnroll], zb[kGradReduceUnroll], db[kGradReduceUnroll];
    double one[kGradReduceUnroll];
    // (three rounds of loads - status, eflag, operands - each round's in flight together)
    int st[kGradReduceUnroll], ef[kGradReduceUnroll];
#pragma unroll
    for (int u = 0; u < kGradReduceUnroll; u++) {
      const long long b = bb + 4 * u + k;
      st[u] = 1;
      if (b < b1) st[u] = a.status[b];
    }
#pragma unroll
    for (int u = 0; u < kGradReduceUnroll; u++) {
      const long long b = bb + 4 * u + k;
      ef[u] = FBSTAB_SUCCESS;
      if (st[u] == 0 && a.out) ef[u] = a.out[b].eflag;
    }
#pragma unroll
    for (int u = 0; u < kGradReduceUnroll; u++) {
      const long long b = bb + 4 * u + k;
      const bool in = st[u] == 0 && ef[u] == FBSTAB_SUCCESS;
      pa[u] = xa[u] = zb[u] = db[u] = 0.0;
      if (in && row_in) { pa[u] = pr[b * prs]; xa[u] = xr[b * xrs]; }
      if (in && col_in) { zb[u] = zc[b * a.xs[0]]; db[u] = dzc[b * a.ps[0]]; }
      one[u] = in ? 1.0 : 0.0;
    }
#pragma unroll
    for (int u = 0; u < kGradReduceUnroll; u++) {
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[u], zb[u], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[u], db[u], acc, 0, 0, 0);
      if (sums) vec = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[u], one[u], vec, 0, 0, 0);
    }
  }
  // result q of a lane: row k + 4 q, column m
  double* slot = a.scratch + (long long)blockIdx.x * kGradReduceSlot;
#pragma unroll
  for (int q = 0; q < 4; q++) {
    slot[(k + 4 * q) * kGradReduceTile + m] = acc[q];
    if (sums && m == 0) slot[kGradReduceTile * kGradReduceTile + k + 4 * q] = vec[q];
  }
}

// One workgroup of 256 threads per tile: thread e adds entry e of the tile's slots, chunk 0 first; the first
// sixteen threads of a column-tile 0 add the row sums as well.
__global__ __launch_bounds__(256) void fbstab_grad_reduce_finish_kernel(GradReducePlan plan, const double* scratch,
                                                                        int chunks, GradReduceOut out) {
  const int tile = blockIdx.x, e = threadIdx.x;
  int g, rt, ct;
  grad_reduce_tile(plan, tile, &g, &rt, &ct);
  const double* slot = scratch + (long long)tile * chunks * kGradReduceSlot;
  int seq;
  long long idx;
  double scale;
  {
    const int r = rt * kGradReduceTile + e / kGradReduceTile, c = ct * kGradReduceTile + e % kGradReduceTile;
    if (grad_reduce_matrix_entry(plan, g, r, c, &seq, &idx, &scale) && out.base[seq]) {
      double s = 0.0;
      for (int k = 0; k < chunks; k++) s += slot[(long long)k * kGradReduceSlot + e];
      out.base[seq][idx] = scale * s;
    }
  }
  if (ct == 0 && e < kGradReduceTile) {
    const int r = rt * kGradReduceTile + e;
    if (grad_reduce_vector_entry(plan, g, r, &seq, &idx, &scale) && out.base[seq]) {
      double s = 0.0;
      for (int k = 0; k < chunks; k++) s += slot[(long long)k * kGradReduceSlot + kGradReduceTile * kGradReduceTile + e];
      out.base[seq][idx] = scale * s;
    }
  }
}

}  // namespace fbk
