// Condensing an MPC QP (fbstab_hip_mpc_condense_batch, fbstab_hip_mpc_expand_batch): the states are eliminated
// through the dynamics, which leaves a dense QP in the inputs U = (u_0 .. u_N) alone - nz_c = (N + 1) nu variables,
// no equalities, the nv = (N + 1) nc inequalities of the MPC QP in their order.  In the terms of mpc_data.cc
// (stage cost 1/2 [x; u]' [Q S'; S R] [x; u] + q'x + r'u, x_(i+1) = A_i x_i + B_i u_i + c_i, E_i x_i + L_i u_i + d_i <= 0):
//   xbar_0 = x0, xbar_(i+1) = A_i xbar_i + c_i           the free response (U = 0)
//   X_k^(i) = dx_i / du_k = A_(i-1) .. A_(k+1) B_k       for i > k, zero otherwise (causality)
//   A_c[i, k] = E_i X_k^(i) (i > k),  L_k (i = k),  0 (i < k)              b_c[i] = -d_i - E_i xbar_i
//   H_c[j, k] = B_j' P_(j+1) + S_j X_k^(j) (j > k) + R_k (j = k)   for j >= k, and H_c[k, j] = H_c[j, k]'
//       P_i = Q_i X_k^(i) + A_i' P_(i+1) for i > k, P_(N+1) = 0     (nx x nu, carried backwards)
//   f_c[k] = S_k xbar_k + r_k + B_k' p_(k+1),     p_i = Q_i xbar_i + q_i + A_i' p_(i+1), p_(N+1) = 0
// (terms of stage N + 1 and the [A B] of stage N do not exist).  The constant of the cost is dropped.
// Only the blocks on and below the diagonal of H_c are computed (and of the diagonal blocks the lower triangle,
// from the lower triangle of R_k); each is written twice, to (j, k) and mirrored to (k, j): H_c is symmetric bit
// for bit, and Q, R are taken as symmetric, as the solvers take them.
// The inverse map (condense_expand) rolls the dynamics out for the states and reads the costates off the x rows of
// the stationarity condition: l_i = Q_i x_i + S_i' u_i + q_i + E_i' v_i + A_i' l_(i+1).
//
// As fb_tangent.h: written against Ctx (c.tid, C::nt, c.sync()), every stage image reaches the work array w (LDS on
// the device) in contiguous runs of 16 B per lane, one thread owns each output entry and sums it in ascending index
// order.  No atomics and no sums across threads or workgroups: a QP's bits depend on its data and the shape alone.
// Images lie in w with an odd leading dimension, so that neither the walk along a column (M x) nor the one along a
// row (M' x) of 32 neighbouring threads meets one LDS bank twice.
#pragma once

#include "fb_batch.h"
#include "fb_condense_plan.h"  // (condense_ld, CondenseLds)

namespace fbk {

// dst (rows x cols, leading dimension ld) = the contiguous column-major image src: as tangent_stage, thread c.tid
// takes the 16-byte pairs c.tid, c.tid + C::nt, ... counted from the first 16-byte boundary of src.  The caller
// synchronises before dst is read.
template <class C, class P>
FB_DEV void condense_stage(const C& c, P dst, int ld, const double* src, int rows, int cols) {
  const int len = rows * cols;
  const int head = (len > 0 && (((uintptr_t)src >> 3) & 1)) ? 1 : 0;
  const int pairs = (len - head) / 2;
  for (int p = c.tid; p < pairs; p += C::nt) {
    double t[2];
    const int e = head + 2 * p;
    __builtin_memcpy(t, __builtin_assume_aligned(src + e, 16), 16);
    const int col = e / rows, row = e - col * rows;
    dst[row + col * ld] = t[0];
    if (row + 1 < rows) dst[row + 1 + col * ld] = t[1];
    else dst[(col + 1) * ld] = t[1];
  }
  if (c.tid == 0) {
    if (head) dst[0] = src[0];
    if (head + 2 * pairs < len) dst[(rows - 1) + (cols - 1) * ld] = src[len - 1];
  }
}

// sum_m M[r + m ld] x[m]  and  sum_m M[m + r ld] x[m], ascending m
template <class P, class PX>
FB_DEV double condense_dot_row(P M, int ld, int r, PX x, int n, double acc) {
  for (int m = 0; m < n; m++) acc = fma(M[r + m * ld], x[m], acc);
  return acc;
}
template <class P, class PX>
FB_DEV double condense_dot_col(P M, int ld, int r, PX x, int n, double acc) {
  for (int m = 0; m < n; m++) acc = fma(M[m + r * ld], x[m], acc);
  return acc;
}

// Column block k of H_c (nz_c x nz_c, column-major) and A_c (nv x nz_c, column-major) of one QP, with the mirror
// images of its blocks of H_c; a null H or Ac is not written.  Every entry of the two images is written by exactly
// one k.  The caller synchronises before w is used again.
template <class C, class P>
FB_DEV void condense_matrices(const C& c, int N, int nx, int nu, int nc, int k, const MpcData& D,
                              const CondenseLds& o, P w, double* H, double* Ac) {
  const int nzc = (N + 1) * nu, nv = (N + 1) * nc;
  const int ldx = o.ldx, ldc = o.ldc, ldu = o.ldu;
  const int xs = ldx * nu + ((ldx * nu) & 1);  // one X or P
  const P A = w + o.A, Q = w + o.Q, B = w + o.B, E = w + o.E, S = w + o.S, L = w + o.L, R = w + o.R;
  const P X = w + o.carry;  // X_k^(i) at X + (i - k - 1) xs, i = k + 1 .. N
  P Pa = X + (long)N * xs, Pb = Pa + xs;
  // ---- forward: X_k^(i), and column block k of A_c --------------------------------------------------------
  condense_stage(c, L, ldc, D.L + (long)k * nc * nu, nc, nu);
  if (k < N) condense_stage(c, X, ldx, D.B + (long)k * nx * nu, nx, nu);
  if (Ac)
    for (int e = c.tid; e < k * nc * nu; e += C::nt) {  // the blocks above the diagonal
      const int col = e / (k * nc), row = e - col * (k * nc);
      Ac[row + (long)(k * nu + col) * nv] = 0.0;
    }
  c.sync();
  if (Ac)
    for (int e = c.tid; e < nc * nu; e += C::nt) {
      const int col = e / nc, row = e - col * nc;
      Ac[(k * nc + row) + (long)(k * nu + col) * nv] = L[row + col * ldc];
    }
  for (int i = k + 1; i <= N; i++) {
    const P Xi = X + (long)(i - k - 1) * xs;
    condense_stage(c, E, ldc, D.E + (long)i * nc * nx, nc, nx);
    if (i < N) condense_stage(c, A, ldx, D.A + (long)i * nx * nx, nx, nx);
    c.sync();
    if (Ac)
      for (int e = c.tid; e < nc * nu; e += C::nt) {
        const int col = e / nc, row = e - col * nc;
        Ac[(i * nc + row) + (long)(k * nu + col) * nv] = condense_dot_row(E, ldc, row, Xi + col * ldx, nx, 0.0);
      }
    if (i < N)
      for (int e = c.tid; e < nx * nu; e += C::nt) {
        const int col = e / nx, row = e - col * nx;
        Xi[xs + row + col * ldx] = condense_dot_row(A, ldx, row, Xi + col * ldx, nx, 0.0);
      }
    c.sync();
  }
  if (!H) return;
  // ---- backward: P_(j+1), and the blocks (j, k), j = N .. k, of H_c ----------------------------------------
  for (int j = N; j >= k; j--) {
    const P Xj = X + (long)(j - k - 1) * xs;  // (read for j > k only)
    if (j < N) condense_stage(c, B, ldx, D.B + (long)j * nx * nu, nx, nu);
    if (j > k) {
      condense_stage(c, S, ldu, D.S + (long)j * nu * nx, nu, nx);
      condense_stage(c, Q, ldx, D.Q + (long)j * nx * nx, nx, nx);
      if (j < N) condense_stage(c, A, ldx, D.A + (long)j * nx * nx, nx, nx);
    } else {
      condense_stage(c, R, ldu, D.R + (long)k * nu * nu, nu, nu);
    }
    c.sync();
    for (int e = c.tid; e < nu * nu; e += C::nt) {
      const int col = e / nu, row = e - col * nu;
      if (j == k && row < col) continue;
      double acc = 0.0;
      if (j < N) acc = condense_dot_col(B, ldx, row, Pa + col * ldx, nx, acc);
      if (j > k) acc = condense_dot_row(S, ldu, row, Xj + col * ldx, nx, acc);
      else acc += R[row + col * ldu];
      const long r = j * nu + row, cc = k * nu + col;
      H[r + cc * nzc] = acc;
      if (r != cc) H[cc + r * nzc] = acc;
    }
    if (j > k)
      for (int e = c.tid; e < nx * nu; e += C::nt) {
        const int col = e / nx, row = e - col * nx;
        double acc = condense_dot_row(Q, ldx, row, Xj + col * ldx, nx, 0.0);
        if (j < N) acc = condense_dot_col(A, ldx, row, Pa + col * ldx, nx, acc);
        Pb[row + col * ldx] = acc;
      }
    c.sync();
    const P t = Pa; Pa = Pb; Pb = t;
  }
}

// f_c and b_c of one QP (null: not written), O(N nx^2).  The caller synchronises before w is used again.
template <class C, class P>
FB_DEV void condense_vectors(const C& c, int N, int nx, int nu, int nc, const MpcData& D, const CondenseLds& o, P w,
                             double* f, double* b) {
  const int ldx = o.ldx, ldc = o.ldc, ldu = o.ldu;
  const P A = w + o.A, Q = w + o.Q, B = w + o.B, E = w + o.E, S = w + o.S;
  const P xb = w + o.carry;  // xbar_i at xb + i nx
  P pa = xb + (long)(N + 1) * nx + (((N + 1) * nx) & 1), pb = pa + nx + (nx & 1);
  for (int r = c.tid; r < nx; r += C::nt) xb[r] = D.x0[r];
  // ---- forward: the free response, and b_c ----------------------------------------------------------------
  for (int i = 0; i <= N; i++) {
    const P xi = xb + (long)i * nx;
    if (b) condense_stage(c, E, ldc, D.E + (long)i * nc * nx, nc, nx);
    if (i < N) condense_stage(c, A, ldx, D.A + (long)i * nx * nx, nx, nx);
    c.sync();
    if (b)
      for (int r = c.tid; r < nc; r += C::nt)
        b[i * nc + r] = (0.0 - D.d[(long)i * nc + r]) - condense_dot_row(E, ldc, r, xi, nx, 0.0);
    if (i < N)
      for (int r = c.tid; r < nx; r += C::nt) xi[nx + r] = condense_dot_row(A, ldx, r, xi, nx, 0.0) + D.c[(long)i * nx + r];
    c.sync();
  }
  if (!f) return;
  // ---- backward: p_(j+1), and f_c -------------------------------------------------------------------------
  for (int j = N; j >= 0; j--) {
    const P xj = xb + (long)j * nx;
    condense_stage(c, S, ldu, D.S + (long)j * nu * nx, nu, nx);
    if (j > 0) condense_stage(c, Q, ldx, D.Q + (long)j * nx * nx, nx, nx);
    if (j < N) {
      condense_stage(c, B, ldx, D.B + (long)j * nx * nu, nx, nu);
      if (j > 0) condense_stage(c, A, ldx, D.A + (long)j * nx * nx, nx, nx);
    }
    c.sync();
    for (int r = c.tid; r < nu; r += C::nt) {
      double acc = condense_dot_row(S, ldu, r, xj, nx, 0.0);
      if (j < N) acc = condense_dot_col(B, ldx, r, pa, nx, acc);
      f[j * nu + r] = acc + D.r[(long)j * nu + r];
    }
    if (j > 0)
      for (int r = c.tid; r < nx; r += C::nt) {
        double acc = condense_dot_row(Q, ldx, r, xj, nx, 0.0);
        if (j < N) acc = condense_dot_col(A, ldx, r, pa, nx, acc);
        pb[r] = acc + D.q[(long)j * nx + r];
      }
    c.sync();
    const P t = pa; pa = pb; pb = t;
  }
}

// (z, l, v, y) of the MPC QP from (U, v_c, y_c) of the condensed one; null outputs are skipped, and yc may be null
// where y is.  The caller synchronises before w is used again.
template <class C, class P>
FB_DEV void condense_expand(const C& c, int N, int nx, int nu, int nc, const MpcData& D, const double* U,
                            const double* vc, const double* yc, const CondenseLds& o, P w, double* z, double* l,
                            double* v, double* y) {
  const int ldx = o.ldx, ldc = o.ldc, ldu = o.ldu, ns = nx + nu;
  const int nzc = (N + 1) * nu, nv = (N + 1) * nc;
  const P A = w + o.A, Q = w + o.Q, B = w + o.B, E = w + o.E, S = w + o.S;
  const P xs = w + o.carry;
  const P us = xs + (long)(N + 1) * nx + (((N + 1) * nx) & 1);
  const P vs = us + nzc + (nzc & 1);
  P la = vs + nv + (nv & 1), lb = la + nx + (nx & 1);
  condense_stage(c, us, nzc, U, nzc, 1);
  condense_stage(c, vs, nv, vc, nv, 1);
  for (int r = c.tid; r < nx; r += C::nt) xs[r] = D.x0[r];
  if (v)
    for (int e = c.tid; e < nv; e += C::nt) v[e] = vc[e];
  if (y)
    for (int e = c.tid; e < nv; e += C::nt) y[e] = yc[e];
  // ---- forward: the states ---------------------------------------------------------------------------------
  for (int i = 0; i < N; i++) {
    const P xi = xs + (long)i * nx;
    condense_stage(c, A, ldx, D.A + (long)i * nx * nx, nx, nx);
    condense_stage(c, B, ldx, D.B + (long)i * nx * nu, nx, nu);
    c.sync();
    for (int r = c.tid; r < nx; r += C::nt) {
      double acc = condense_dot_row(A, ldx, r, xi, nx, 0.0);
      acc = condense_dot_row(B, ldx, r, us + i * nu, nu, acc);
      xi[nx + r] = acc + D.c[(long)i * nx + r];
    }
    c.sync();
  }
  if (z)
    for (int e = c.tid; e < (N + 1) * ns; e += C::nt) {
      const int i = e / ns, r = e - i * ns;
      z[e] = r < nx ? xs[(long)i * nx + r] : us[i * nu + (r - nx)];
    }
  if (!l) return;
  // ---- backward: the costates ------------------------------------------------------------------------------
  for (int i = N; i >= 0; i--) {
    const P xi = xs + (long)i * nx;
    condense_stage(c, Q, ldx, D.Q + (long)i * nx * nx, nx, nx);
    condense_stage(c, S, ldu, D.S + (long)i * nu * nx, nu, nx);
    condense_stage(c, E, ldc, D.E + (long)i * nc * nx, nc, nx);
    if (i < N) condense_stage(c, A, ldx, D.A + (long)i * nx * nx, nx, nx);
    c.sync();
    for (int r = c.tid; r < nx; r += C::nt) {
      double acc = condense_dot_row(Q, ldx, r, xi, nx, 0.0);
      acc = condense_dot_col(S, ldu, r, us + i * nu, nu, acc);
      acc = condense_dot_col(E, ldc, r, vs + i * nc, nc, acc);
      if (i < N) acc = condense_dot_col(A, ldx, r, la, nx, acc);
      acc += D.q[(long)i * nx + r];
      lb[r] = acc;
      l[(long)i * nx + r] = acc;
    }
    c.sync();
    const P t = la; la = lb; lb = t;
  }
}

}  // namespace fbk
