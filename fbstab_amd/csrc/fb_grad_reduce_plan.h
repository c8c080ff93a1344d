// The tile table of the batch-summed gradients (fbstab_hip_*_adjoint_batch_reduced; kernels in fb_grad_reduce.h),
// as pure functions of the shape: no HIP types, so that tests/test_grad_reduce_plan.py compiles this header with
// the host compiler alone and walks the same table as the kernels.
//
// With X = [Z L V] the points and P = [DZ DL DV] the adjoint steps of a batch (one QP per row), every matrix
// gradient summed over the batch is a block of
//     M = -(P'Z + X'DZ),      M(r, c) = -sum_b (P[b][r] Z[b][c] + X[b][r] DZ[b][c])
// and every vector gradient is +-sum_b P[b][r] (fb_adjoint.h has the per-QP table).  The rows and columns that
// carry a gradient are cut into GROUPS, each a dense rectangle of M:
//   dense: one group, rows [z | l | v] (nz + nl + nv of them), columns z:
//          H = rows z (halved), G = rows l, A = rows v, each column-major; f = -sum dz, h = sum dl, b = sum dv.
//   MPC:   group i = stage i, 0 <= i <= N: rows [x_i u_i | l_(i+1) | v_i] (stage N has no l rows), columns [x_i u_i]:
//          Q_i = x rows, x columns (halved)   R_i = u rows, u columns (halved)   S_i = u rows, x columns
//          (x rows, u columns: S_i' once more - no entry)   [A_i B_i] = l rows   [E_i L_i] = v rows
//          q, r = -sum dz; c_i = -sum dl_(i+1); d_i = -sum dv_i;
//          group N + 1: rows l_0, no columns: x0 = -sum dl_0.
// A group is cut into 16 x 16 TILES, row tiles outer, column tiles inner (a group without columns has one column
// tile, all of it outside the edge); tiles are numbered group by group.  One wavefront accumulates one tile over
// one CHUNK of kGradReduceChunk consecutive QPs - a constant of this header: the reduced bits depend on the
// inputs and on the batch size only - into a slot of its own, kGradReduceSlot doubles: the tile row-major
// (m, n) -> 16 m + n, then the 16 row sums sum_b P[b][row m] (read from column-tile 0 only).  The finishing kernel
// adds the slots of a tile in ascending chunk order and applies the sign and the 1/2.
#pragma once

#include "../../include/fbstab_types.h"  // fbstab_solver_out_t (GradReduceArgs)

#if defined(__HIPCC__)
#define FB_PLAN_FN __host__ __device__ inline
#else
#define FB_PLAN_FN inline
#endif

namespace fbk {

constexpr int kGradReduceChunk = 128;          // QPs per partial sum
constexpr int kGradReduceTile = 16;            // v_mfma_f64_16x16x4: a 16 x 16 tile, four QPs per instruction
constexpr int kGradReduceSlot = 16 * 16 + 16;  // doubles per (tile, chunk): the tile and its row sums

struct GradReducePlan {
  int mpc;             // 0: dense, 1: MPC
  int N, nx, nu, nc;   // MPC (dense: 0)
  int nz, nl, nv;      // lengths of z, l, v
};

FB_PLAN_FN GradReducePlan grad_reduce_plan_dense(int nz, int nl, int nv) {
  GradReducePlan p;
  p.mpc = 0; p.N = p.nx = p.nu = p.nc = 0;
  p.nz = nz; p.nl = nl; p.nv = nv;
  return p;
}
FB_PLAN_FN GradReducePlan grad_reduce_plan_mpc(int N, int nx, int nu, int nc) {
  GradReducePlan p;
  p.mpc = 1; p.N = N; p.nx = nx; p.nu = nu; p.nc = nc;
  p.nz = (N + 1) * (nx + nu); p.nl = (N + 1) * nx; p.nv = (N + 1) * nc;
  return p;
}

FB_PLAN_FN int grad_reduce_groups(const GradReducePlan& p) { return p.mpc ? p.N + 2 : 1; }
FB_PLAN_FN int grad_reduce_group_rows(const GradReducePlan& p, int g) {
  if (!p.mpc) return p.nz + p.nl + p.nv;
  if (g < p.N) return p.nx + p.nu + p.nx + p.nc;
  return g == p.N ? p.nx + p.nu + p.nc : p.nx;
}
FB_PLAN_FN int grad_reduce_group_cols(const GradReducePlan& p, int g) {
  if (!p.mpc) return p.nz;
  return g <= p.N ? p.nx + p.nu : 0;
}
FB_PLAN_FN int grad_reduce_col_tiles(const GradReducePlan& p, int g) {
  const int c = grad_reduce_group_cols(p, g);
  return c > 0 ? (c + kGradReduceTile - 1) / kGradReduceTile : 1;
}
FB_PLAN_FN int grad_reduce_group_tiles(const GradReducePlan& p, int g) {
  return (grad_reduce_group_rows(p, g) + kGradReduceTile - 1) / kGradReduceTile * grad_reduce_col_tiles(p, g);
}
FB_PLAN_FN int grad_reduce_tiles(const GradReducePlan& p) {
  if (!p.mpc) return grad_reduce_group_tiles(p, 0);
  return p.N * grad_reduce_group_tiles(p, 0) + grad_reduce_group_tiles(p, p.N) + grad_reduce_group_tiles(p, p.N + 1);
}
// tile t -> its group, row tile and column tile
FB_PLAN_FN void grad_reduce_tile(const GradReducePlan& p, int t, int* g, int* rt, int* ct) {
  int grp = 0;
  if (p.mpc) {
    const int t0 = grad_reduce_group_tiles(p, 0);  // (N >= 1: group 0 is a stage with l rows)
    if (t < p.N * t0) {
      grp = t / t0; t -= grp * t0;
    } else {
      t -= p.N * t0; grp = p.N;
      const int tn = grad_reduce_group_tiles(p, p.N);
      if (t >= tn) { t -= tn; grp = p.N + 1; }
    }
  }
  const int nct = grad_reduce_col_tiles(p, grp);
  *g = grp; *rt = t / nct; *ct = t % nct;
}
FB_PLAN_FN long long grad_reduce_chunks(int batch) { return (batch + kGradReduceChunk - 1) / kGradReduceChunk; }
// doubles of the partial sums of a batch: one slot per (tile, chunk), slot (t, k) at (t * chunks + k) * kGradReduceSlot
FB_PLAN_FN long long grad_reduce_scratch_doubles(const GradReducePlan& p, int batch) {
  return (long long)grad_reduce_tiles(p) * grad_reduce_chunks(batch) * kGradReduceSlot;
}

// Row r of group g: which of (z, l, v) / (dz, dl, dv) it is an element of (*arr = 0, 1, 2), and which.
FB_PLAN_FN void grad_reduce_row(const GradReducePlan& p, int g, int r, int* arr, int* off) {
  if (!p.mpc) {
    if (r < p.nz) { *arr = 0; *off = r; }
    else if (r < p.nz + p.nl) { *arr = 1; *off = r - p.nz; }
    else { *arr = 2; *off = r - p.nz - p.nl; }
    return;
  }
  const int ns = p.nx + p.nu;
  if (g == p.N + 1) { *arr = 1; *off = r; return; }
  if (r < ns) { *arr = 0; *off = g * ns + r; return; }
  r -= ns;
  if (g < p.N) {
    if (r < p.nx) { *arr = 1; *off = (g + 1) * p.nx + r; return; }
    r -= p.nx;
  }
  *arr = 2; *off = g * p.nc + r;
}
// Column c of group g: the element of z / dz.
FB_PLAN_FN int grad_reduce_col(const GradReducePlan& p, int g, int c) { return p.mpc ? g * (p.nx + p.nu) + c : c; }

// Entry (r, c) of group g: false, or the sequence (the index of fbstab_mpc_batch_t / fbstab_dense_batch_t), the
// place in its image and the factor that M(r, c) takes (-1, or -1/2 for the symmetric parts).
FB_PLAN_FN bool grad_reduce_matrix_entry(const GradReducePlan& p, int g, int r, int c, int* seq, long long* idx,
                                         double* scale) {
  *scale = -1.0;
  if (r >= grad_reduce_group_rows(p, g) || c >= grad_reduce_group_cols(p, g)) return false;
  if (!p.mpc) {
    if (r < p.nz) { *seq = 0; *idx = r + (long long)c * p.nz; *scale = -0.5; }               // H
    else if (r < p.nz + p.nl) { *seq = 2; *idx = (r - p.nz) + (long long)c * p.nl; }          // G
    else { *seq = 4; *idx = (r - p.nz - p.nl) + (long long)c * p.nv; }                        // A
    return true;
  }
  const int nx = p.nx, nu = p.nu, nc = p.nc, ns = nx + nu;
  const long long i = g;
  if (r < nx) {
    if (c >= nx) return false;
    *seq = 0; *idx = i * nx * nx + r + c * nx; *scale = -0.5;                                 // Q
    return true;
  }
  if (r < ns) {
    if (c < nx) { *seq = 2; *idx = i * nu * nx + (r - nx) + c * nu; }                         // S
    else { *seq = 1; *idx = i * nu * nu + (r - nx) + (c - nx) * nu; *scale = -0.5; }          // R
    return true;
  }
  r -= ns;
  if (g < p.N) {
    if (r < nx) {
      if (c < nx) { *seq = 5; *idx = i * nx * nx + r + c * nx; }                              // A
      else { *seq = 6; *idx = i * nx * nu + r + (c - nx) * nx; }                              // B
      return true;
    }
    r -= nx;
  }
  if (c < nx) { *seq = 8; *idx = i * nc * nx + r + c * nc; }                                  // E
  else { *seq = 9; *idx = i * nc * nu + r + (c - nx) * nc; }                                  // L
  return true;
}
// Row r of group g: the vector gradient that sum_b P[b][r] belongs to, its place and its sign.
FB_PLAN_FN bool grad_reduce_vector_entry(const GradReducePlan& p, int g, int r, int* seq, long long* idx,
                                         double* scale) {
  *scale = -1.0;
  if (r >= grad_reduce_group_rows(p, g)) return false;
  if (!p.mpc) {
    if (r < p.nz) { *seq = 1; *idx = r; }                                                     // f
    else if (r < p.nz + p.nl) { *seq = 3; *idx = r - p.nz; *scale = 1.0; }                    // h
    else { *seq = 5; *idx = r - p.nz - p.nl; *scale = 1.0; }                                  // b
    return true;
  }
  const int nx = p.nx, nu = p.nu, nc = p.nc;
  const long long i = g;
  if (g == p.N + 1) { *seq = 11; *idx = r; return true; }                                     // x0
  if (r < nx) { *seq = 3; *idx = i * nx + r; return true; }                                   // q
  if (r < nx + nu) { *seq = 4; *idx = i * nu + (r - nx); return true; }                       // r
  r -= nx + nu;
  if (g < p.N) {
    if (r < nx) { *seq = 7; *idx = i * nx + r; return true; }                                 // c
    r -= nx;
  }
  *seq = 10; *idx = i * nc + r;                                                               // d
  return true;
}

// What the two kernels take, filled on the host (fb_host_stage.h: AdjointStage::reduce).
struct GradReduceArgs {
  GradReducePlan plan;
  const double* x[3];  // z, l, v
  long long xs[3];
  const double* p[3];  // dz, dl, dv
  long long ps[3];
  const int* status;               // the adjoint's, per QP
  const fbstab_solver_out_t* out;  // the solve's records, or null
  double* scratch;                 // grad_reduce_scratch_doubles(plan, batch)
  int batch;
};

constexpr int kGradReduceMaxSeq = 12;
struct GradReduceOut {
  double* base[kGradReduceMaxSeq];  // where the reduced array of each sequence goes (null: not reduced)
};

}  // namespace fbk
