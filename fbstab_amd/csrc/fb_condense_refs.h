// The images of per-step references on the condensed MPC route (fbstab_hip_mpc_condensed_reference_images_batch):
// H_c, A_c and the map M = [F; G] do not depend on q, r, c, d, so a closed loop whose references move solves, at step k,
//   f_c,k(x) = f0_k + F x        b_c,k(x) = b0_k + G x
// with (f0_k, b0_k) what condense_vectors gives for x0 = 0 and the step's q_k, r_k, c_k, d_k.  This is that map for R
// steps of one trajectory per workgroup: a stage's images are staged into the window of CondenseLds ONCE and used by
// all R references of the group, thread (row r, reference k) owns entry r of reference k, and the mat-vecs of the two
// sweeps become mat-mats that keep R nx threads busy instead of nx (the layout of fb_condense_multi.h).
//
// Per reference the operations and their order are those of condense_vectors with xbar_0 = 0 - ascending index order,
// plain FMAs, one thread per output entry, no atomics, no sums across threads - so the images are bit for bit those of
// fbstab_hip_mpc_condense_batch(VECTORS) on the step's data with x0 on a block of zeros.  R changes who computes an
// entry, never how: a step's bits depend on its sequences, the trajectory's model and the shape alone - not on R, the
// batch or the neighbouring steps.
//
// The carry region behind the window holds R copies of what condense_vectors carries, `per` doubles each
// (condense_refs_per): xbar_i of every stage, e((N + 1) nx), and two p, 2 e(nx)  (e(n): n rounded up to even).
//
// Not here: the gradients of the references (the sweep adjoint's finish kernel writes them), the map M
// (fb_condense_sweep.h).
#pragma once

#include "fb_condense.h"
#include "fb_condense_plan.h"  // (condense_refs_per, CondenseRefSeqs)

namespace fbk {

// References k0 .. k0 + Rg - 1 of one trajectory (rs: its four sequences at reference k0, reference kk at + kk step;
// D: its model - q, r, c, d and x0 of D are not read): f0 of reference kk at f0 + kk sf0, b0 at b0 + kk sb0.  The caller
// synchronises before w is used again.
template <class C, class P>
FB_DEV void condense_reference_vectors(const C& c, int N, int nx, int nu, int nc, const MpcData& D,
                                       const CondenseRefSeqs& rs, int Rg, long per, const CondenseLds& o, P w,
                                       double* f0, long long sf0, double* b0, long long sb0) {
  const int ldx = o.ldx, ldc = o.ldc, ldu = o.ldu;
  const P A = w + o.A, Q = w + o.Q, B = w + o.B, E = w + o.E, S = w + o.S;
  const P cb = w + o.carry;  // copy kk at cb + kk per: xbar_i at + i nx, then two p
  const long po = (long)(N + 1) * nx + (((N + 1) * nx) & 1), ps = nx + (nx & 1);
  long pa = po, pb = po + ps;
  for (int e = c.tid; e < nx * Rg; e += C::nt) {
    const int kk = e / nx, r = e - kk * nx;
    cb[kk * per + r] = 0.0;
  }
  // ---- forward: the free response, and b0 ------------------------------------------------------------------
  for (int i = 0; i <= N; i++) {
    condense_stage(c, E, ldc, D.E + (long)i * nc * nx, nc, nx);
    if (i < N) condense_stage(c, A, ldx, D.A + (long)i * nx * nx, nx, nx);
    c.sync();
    for (int e = c.tid; e < nc * Rg; e += C::nt) {
      const int kk = e / nc, r = e - kk * nc;
      const P xi = cb + kk * per + (long)i * nx;
      b0[kk * sb0 + i * nc + r] = (0.0 - rs.d[kk * rs.sd + (long)i * nc + r]) - condense_dot_row(E, ldc, r, xi, nx, 0.0);
    }
    if (i < N)
      for (int e = c.tid; e < nx * Rg; e += C::nt) {
        const int kk = e / nx, r = e - kk * nx;
        const P xi = cb + kk * per + (long)i * nx;
        xi[nx + r] = condense_dot_row(A, ldx, r, xi, nx, 0.0) + rs.c[kk * rs.sc + (long)i * nx + r];
      }
    c.sync();
  }
  // ---- backward: p_(j+1), and f0 ---------------------------------------------------------------------------
  for (int j = N; j >= 0; j--) {
    condense_stage(c, S, ldu, D.S + (long)j * nu * nx, nu, nx);
    if (j > 0) condense_stage(c, Q, ldx, D.Q + (long)j * nx * nx, nx, nx);
    if (j < N) {
      condense_stage(c, B, ldx, D.B + (long)j * nx * nu, nx, nu);
      if (j > 0) condense_stage(c, A, ldx, D.A + (long)j * nx * nx, nx, nx);
    }
    c.sync();
    for (int e = c.tid; e < nu * Rg; e += C::nt) {
      const int kk = e / nu, r = e - kk * nu;
      const P xj = cb + kk * per + (long)j * nx, p = cb + kk * per + pa;
      double acc = condense_dot_row(S, ldu, r, xj, nx, 0.0);
      if (j < N) acc = condense_dot_col(B, ldx, r, p, nx, acc);
      f0[kk * sf0 + j * nu + r] = acc + rs.r[kk * rs.sr + (long)j * nu + r];
    }
    if (j > 0)
      for (int e = c.tid; e < nx * Rg; e += C::nt) {
        const int kk = e / nx, r = e - kk * nx;
        const P xj = cb + kk * per + (long)j * nx, p = cb + kk * per + pa;
        double acc = condense_dot_row(Q, ldx, r, xj, nx, 0.0);
        if (j < N) acc = condense_dot_col(A, ldx, r, p, nx, acc);
        cb[kk * per + pb + r] = acc + rs.q[kk * rs.sq + (long)j * nx + r];
      }
    c.sync();
    const long t = pa; pa = pb; pb = t;
  }
}

}  // namespace fbk
