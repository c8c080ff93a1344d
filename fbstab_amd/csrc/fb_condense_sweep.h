// Closed-loop sweeps on the condensed route (fbstab_hip_mpc_condensed_x0_map_batch,
// fbstab_hip_mpc_condensed_receding_sweep).  In a receding-horizon sweep the matrix sequences and q, r, c, d stay where
// they are and only x0 moves, so H_c and A_c stand and the two vectors of the condensed QP are affine in x0:
//   f_c(x) = f_c(0) + F x      b_c(x) = b_c(0) + G x       F: (N + 1) nu x nx,  G: (N + 1) nc x nx
// From fb_condense.h: xbar_i = Phi_i x0 + (terms of c), Phi_0 = I, Phi_(i+1) = A_i Phi_i, and
//   b_c[i] = -d_i - E_i xbar_i                            =>  G[i] = -E_i Phi_i
//   f_c[k] = S_k xbar_k + r_k + B_k' p_(k+1),
//   p_i = Q_i xbar_i + q_i + A_i' p_(i+1), p_(N+1) = 0    =>  F[k] = S_k Phi_k + B_k' P_(k+1),
//                                                             P_i = Q_i Phi_i + A_i' P_(i+1), P_(N+1) = 0
// which is condense_matrices for a virtual input u_(-1) = x0 with B_(-1) = I, a block of columns at a time:
// X^(0) = I[:, cols], X^(i+1) = A_i X^(i).  (The B' term of stage N and P_0 do not exist.)
//
// The image of one QP is M = [F; G], ne = (N + 1)(nu + nc) rows by nx columns, COLUMN-MAJOR with leading dimension
// ne: entry (e, j) at M[e + j ne], rows 0 .. (N + 1) nu of F in the order of U, then the rows of G in the order of v.
// The step kernel's thread (e, trajectory) walks a row with j ascending: the 64 lanes of a wavefront read 64
// neighbouring doubles of one column from memory, and from LDS - where a shared image lies with the odd leading
// dimension ne | 1 - 64 neighbouring words, no bank twice.
//
// As fb_condense.h: written against Ctx (c.tid, C::nt, c.sync()), stage images reach the work array w through
// condense_stage in the CondenseLds layout, one thread owns each output entry and sums it in ascending index order
// with plain FMAs.  No atomics, no sums across threads, no matrix cores.
//
// Not here: sharded sweeps, the C++ facade.  (Per-step references - q, r, c, d that move - need no code here: the
// host stage hands each launch of condense_sweep_step the f0, b0 of its step, fb_condense_refs.h.  The derivative through the
// sweep: fb_condense_sweep_adjoint.h.)
#pragma once

#include "fb_condense.h"
#include "fb_condense_plan.h"  // (CondenseSweepLds, CondenseSweepStep)

namespace fbk {

// Columns c0 .. c0 + ncol of M (ncol <= nu) of one QP.  Carry: X^(i) at X + (i - 1) xs for i = 1 .. N and two P, the
// (N + 2) e(ldx nu) doubles condense_matrices takes; X^(0) is read off the stage images (a column of I).  The caller
// synchronises before w is used again.
template <class C, class P>
FB_DEV void condense_x0_map(const C& c, int N, int nx, int nu, int nc, int c0, int ncol, const MpcData& D,
                            const CondenseLds& o, P w, double* M) {
  const int nzc = (N + 1) * nu, nv = (N + 1) * nc;
  const long ne = (long)nzc + nv;
  const int ldx = o.ldx, ldc = o.ldc, ldu = o.ldu;
  const int xs = ldx * nu + ((ldx * nu) & 1);
  const P A = w + o.A, Q = w + o.Q, B = w + o.B, E = w + o.E, S = w + o.S;
  const P X = w + o.carry;
  P Pa = X + (long)N * xs, Pb = Pa + xs;
  double* const F = M + (long)c0 * ne;
  double* const G = F + nzc;
  // ---- forward: X^(i), and G ----------------------------------------------------------------------------------
  condense_stage(c, E, ldc, D.E, nc, nx);
  condense_stage(c, A, ldx, D.A, nx, nx);
  c.sync();
  for (int e = c.tid; e < nc * ncol; e += C::nt) {
    const int col = e / nc, row = e - col * nc;
    G[row + col * ne] = 0.0 - E[row + (c0 + col) * ldc];
  }
  for (int e = c.tid; e < nx * ncol; e += C::nt) {
    const int col = e / nx, row = e - col * nx;
    X[row + col * ldx] = A[row + (c0 + col) * ldx];
  }
  c.sync();
  for (int i = 1; i <= N; i++) {
    const P Xi = X + (long)(i - 1) * xs;
    condense_stage(c, E, ldc, D.E + (long)i * nc * nx, nc, nx);
    if (i < N) condense_stage(c, A, ldx, D.A + (long)i * nx * nx, nx, nx);
    c.sync();
    for (int e = c.tid; e < nc * ncol; e += C::nt) {
      const int col = e / nc, row = e - col * nc;
      G[(i * nc + row) + col * ne] = 0.0 - condense_dot_row(E, ldc, row, Xi + col * ldx, nx, 0.0);
    }
    if (i < N)
      for (int e = c.tid; e < nx * ncol; e += C::nt) {
        const int col = e / nx, row = e - col * nx;
        Xi[xs + row + col * ldx] = condense_dot_row(A, ldx, row, Xi + col * ldx, nx, 0.0);
      }
    c.sync();
  }
  // ---- backward: P_(j+1), and F -------------------------------------------------------------------------------
  for (int j = N; j >= 0; j--) {
    const P Xj = X + (long)(j - 1) * xs;  // (read for j > 0 only)
    condense_stage(c, S, ldu, D.S + (long)j * nu * nx, nu, nx);
    if (j < N) condense_stage(c, B, ldx, D.B + (long)j * nx * nu, nx, nu);
    if (j > 0) {
      condense_stage(c, Q, ldx, D.Q + (long)j * nx * nx, nx, nx);
      if (j < N) condense_stage(c, A, ldx, D.A + (long)j * nx * nx, nx, nx);
    }
    c.sync();
    for (int e = c.tid; e < nu * ncol; e += C::nt) {
      const int col = e / nu, row = e - col * nu;
      double acc = j > 0 ? condense_dot_row(S, ldu, row, Xj + col * ldx, nx, 0.0) : S[row + (c0 + col) * ldu];
      if (j < N) acc = condense_dot_col(B, ldx, row, Pa + col * ldx, nx, acc);
      F[(j * nu + row) + col * ne] = acc;
    }
    if (j > 0)
      for (int e = c.tid; e < nx * ncol; e += C::nt) {
        const int col = e / nx, row = e - col * nx;
        double acc = condense_dot_row(Q, ldx, row, Xj + col * ldx, nx, 0.0);
        if (j < N) acc = condense_dot_col(A, ldx, row, Pa + col * ldx, nx, acc);
        Pb[row + col * ldx] = acc;
      }
    c.sync();
    const P t = Pa; Pa = Pb; Pb = t;
  }
}

// ---- the step between two solves -----------------------------------------------------------------------------
// Trajectories t0 .. t0 + Tg of the batch, Tg <= L.T.  No synchronisation is needed behind it.
template <class C, class P>
FB_DEV void condense_sweep_step(const C& c, const CondenseSweepStep& a, const CondenseSweepLds& L, long t0, int Tg,
                                P w) {
  const int N = a.N, nx = a.nx, nu = a.nu, nc = a.nc;
  const int nzc = (N + 1) * nu, nv = (N + 1) * nc, ne = nzc + nv;
  const int ex = (int)condense_sweep_even(nx), eU = (int)condense_sweep_even(nzc), ev = (int)condense_sweep_even(nv);
  const P Ml = w + L.M, xs = w + L.x, xn = w + L.xn, Us = w + L.U, vs = w + L.v, gs = w + L.gone;
  // ---- 1. the records of the solve: who is gone, and the two integer logs ---------------------------------------
  for (int t = c.tid; t < Tg; t += C::nt) {
    const long q = t0 + t;
    const int eflag = a.out[q].eflag;
    bool gone = a.gone[q] != 0;
    if (a.retire && !gone && eflag != FBSTAB_SUCCESS) {
      gone = true;
      a.gone[q] = 1;
    }
    gs[t] = gone ? 1.0 : 0.0;
    if (a.eflag_log) a.eflag_log[q] = gone ? -1 : eflag;
    if (a.newton_log) a.newton_log[q] = a.out[q].newton_iters;
  }
  if (a.affine && L.m_lds) condense_stage(c, Ml, L.ldm, a.M, ne, nx);
  c.sync();
  // ---- the state the step was solved for and the returned point, zero once gone ---------------------------------
  for (int i = c.tid; i < Tg * nx; i += C::nt) {
    const int t = i / nx, r = i - t * nx;
    xs[t * ex + r] = a.x0[(t0 + t) * a.sx0 + r];
  }
  for (int i = c.tid; i < Tg * nzc; i += C::nt) {
    const int t = i / nzc, e = i - t * nzc;
    Us[t * eU + e] = gs[t] != 0.0 ? 0.0 : a.U[(t0 + t) * nzc + e];
  }
  for (int i = c.tid; i < Tg * nv; i += C::nt) {
    const int t = i / nv, e = i - t * nv;
    vs[t * ev + e] = gs[t] != 0.0 ? 0.0 : a.v[(t0 + t) * nv + e];
  }
  c.sync();
  // ---- 2. the logs; 4. the guess of the next step: the point, zero once gone, moved one stage with `shift` ------
  for (int i = c.tid; i < Tg * nx; i += C::nt) {
    const int t = i / nx, r = i - t * nx;
    const long q = t0 + t;
    if (a.x_log) a.x_log[q * nx + r] = xs[t * ex + r];
    if (a.xkeep) a.xkeep[q * nx + r] = xs[t * ex + r];
  }
  if (a.u_log)
    for (int i = c.tid; i < Tg * nu; i += C::nt) {
      const int t = i / nu, j = i - t * nu;
      a.u_log[(t0 + t) * nu + j] = Us[t * eU + j];
    }
  for (int i = c.tid; i < Tg * nzc; i += C::nt) {
    const int t = i / nzc, e = i - t * nzc;
    const long q = t0 + t;
    if (a.U_log) a.U_log[q * nzc + e] = Us[t * eU + e];
    if (a.shift) a.U[q * nzc + e] = Us[t * eU + (e < N * nu ? e + nu : e)];
    else if (gs[t] != 0.0) a.U[q * nzc + e] = 0.0;
  }
  for (int i = c.tid; i < Tg * nv; i += C::nt) {
    const int t = i / nv, e = i - t * nv;
    const long q = t0 + t;
    if (a.v_log) a.v_log[q * nv + e] = vs[t * ev + e];
    if (a.shift) a.v[q * nv + e] = vs[t * ev + (e < N * nc ? e + nc : e)];
    else if (gs[t] != 0.0) a.v[q * nv + e] = 0.0;
  }
  // ---- 3. the plant: x+ = A_p x + B_p u0 (+ w), in the order of fbstab_receding_plant_kernel --------------------
  for (int i = c.tid; i < Tg * nx; i += C::nt) {
    const int t = i / nx, r = i - t * nx;
    const long q = t0 + t;
    const double* Aq = a.Ap + q * a.sAp;
    const double* Bq = a.Bp + q * a.sBp;
    double acc = 0.0;
    for (int m = 0; m < nx; m++) acc = fma(Aq[r + m * nx], xs[t * ex + m], acc);
    for (int j = 0; j < nu; j++) acc = fma(Bq[r + j * nx], Us[t * eU + j], acc);
    if (a.w) acc = acc + a.w[q * nx + r];
    if (gs[t] != 0.0) acc = 0.0;
    xn[t * ex + r] = acc;
    a.x0[q * a.sx0 + r] = acc;
  }
  if (!a.affine) return;
  c.sync();
  // ---- 5. f_c and b_c of the next step: base + M x+ --------------------------------------------------------------
  for (int i = c.tid; i < Tg * ne; i += C::nt) {
    const int t = i / ne, e = i - t * ne;
    const long q = t0 + t;
    double acc = 0.0;
    if (L.m_lds) {
      for (int j = 0; j < nx; j++) acc = fma(Ml[e + j * L.ldm], xn[t * ex + j], acc);
    } else {
      const double* Mq = a.M + q * a.sM;
      for (int j = 0; j < nx; j++) acc = fma(Mq[e + (long)j * ne], xn[t * ex + j], acc);
    }
    if (e < nzc) a.f[q * a.sf + e] = a.f0[q * a.sf0 + e] + acc;
    else a.b[q * a.sb + (e - nzc)] = a.b0[q * a.sb0 + (e - nzc)] + acc;
  }
}

// Before the first step: U = the u blocks of z, v = v, nobody gone.  z, v: the caller's guess of trajectory q.
template <class C>
FB_DEV void condense_sweep_begin(const C& c, int N, int nx, int nu, int nc, const double* z, const double* v,
                                 double* U, double* vc, int* gone) {
  const int nzc = (N + 1) * nu, nv = (N + 1) * nc;
  for (int e = c.tid; e < nzc; e += C::nt) {
    const int i = e / nu, j = e - i * nu;
    U[e] = z[(long)i * (nx + nu) + nx + j];
  }
  for (int e = c.tid; e < nv; e += C::nt) vc[e] = v[e];
  if (c.tid == 0) *gone = 0;
}

}  // namespace fbk
