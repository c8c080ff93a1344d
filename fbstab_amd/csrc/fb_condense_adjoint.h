// The adjoint of the condensed MPC route (fbstab_hip_mpc_condensed_adjoint_batch): the two maps around the dense
// adjoint of the condensed QP.  At the point x = (z, l, v) the MPC adjoint solves V (dz, dl, dv) = (gz, -gl, -C gv)
// (include/fbstab_hip.h: fbstab_hip_mpc_adjoint_batch).  That system is the QP's own optimality system with the same
// matrices and the vectors
//   q_i := -gz_x_i    r_i := -gz_u_i    x0 := -gl_0    c_i := -gl_(i+1)    d_i := -gv_i,
// so it condenses as the QP does (fb_condense.h):
//   seed:    (f~, b~) = condense_vectors of those vectors;  gU = -f~  and  gv_c = b~  are the seeds of the dense adjoint
//   dense:   V_c (dU, dv) = (gU, -C gv_c) at (U, v)                     (fbstab_hip_dense_adjoint_batch)
//   refine:  one step of iterative refinement of (dU, dv) on the z rows' residual (condense_adjoint_residual below)
//   finish:  (dz, dl) = condense_expand of those vectors at (dU, dv), then the contraction of fb_adjoint.h.
// Both maps are linear in the five vectors; written out with the signs carried through (w_i = -xbar~_i, p_i = -p~_i):
//   w_0 = gl_0,  w_(i+1) = A_i w_i + gl_(i+1)                 gv_c[i] = gv_i + E_i w_i
//   p_j = Q_j w_j + A_j' p_(j+1) + gz_x_j  (p_(N+1) = 0)      gU[j]   = S_j w_j + B_j' p_(j+1) + gz_u_j
//   dx_0 = -gl_0,  dx_(i+1) = A_i dx_i + B_i du_i - gl_(i+1)
//   dl_i = Q_i dx_i + S_i' du_i + E_i' dv_i + A_i' dl_(i+1) - gz_x_i  (dl_(N+1) = 0)
// The step satisfies the u and v rows of the MPC system exactly; its x rows are off by sigma dx and its equality rows
// by sigma dl (the regularisation sits on U alone): the derivative of the solution map with V regularised in the
// condensed variables, a bias of O(sigma) like the MPC adjoint's own.
//
// As fb_condense.h: written against Ctx, stage images staged by condense_stage into the window of CondenseLds, one
// thread per output entry, sums in ascending index order, no atomics.  The vectors live in the carry region:
//   seed:    w_i of every stage and two p                        (N + 1) nx + 2 nx
//   finish:  dz (interleaved like z), dv and two dl              (N + 1)(nx + nu + nc) + 2 nx
// dl_i is held for one stage only: what reads it - the gradients of A_(i-1), B_(i-1), c_(i-1), of x0 at i = 0, and
// the dl slot of adj - is written in the sweep, the other gradients by mpc_adjoint_contract behind it.
#pragma once

#include "fb_adjoint.h"
#include "fb_condense.h"
#include "fb_condense_plan.h"  // (CondenseAdjointWork)

namespace fbk {

// One step of iterative refinement of the dense step, around a second launch of the dense adjoint.  The dense adjoint
// eliminates dv: it factors K = H_c + sigma I + A_c' Gamma A_c with Gamma = C / mus up to 1 / sigma on active rows, so
// the z rows of V_c (dU, dv) = (gU, -C gv_c) come back with a residual at eps / sigma, the v rows at eps.  The z rows'
// residual of the step in hand is cheap and exact to eps in the unreduced form,
//   rU = gU - (H_c dU + sigma dU + A_c' dv),
// the dense adjoint of the seeds (rU, 0) is the correction (eU, ev), and (dU, dv) += (eU, ev) leaves a residual at
// eps / sigma of the CORRECTION.  H_c (nzc x nzc) and A_c (nv x nzc) column-major as the dense QP holds them.
template <class C>
FB_DEV void condense_adjoint_residual(const C& c, int nzc, int nv, const double* H, const double* A, double sigma,
                                      const double* gU, const double* dU, const double* dv, double* rU) {
  for (int i = c.tid; i < nzc; i += C::nt) {
    double acc = sigma * dU[i];
    for (int j = 0; j < nzc; j++) acc += H[i + (long)j * nzc] * dU[j];
    const double* a = A + (long)i * nv;
    for (int k = 0; k < nv; k++) acc += a[k] * dv[k];
    rU[i] = gU[i] - acc;
  }
}

template <class C>
FB_DEV void condense_adjoint_correct(const C& c, int nzc, int nv, const double* eU, const double* ev, double* dU,
                                     double* dv) {
  for (int i = c.tid; i < nzc; i += C::nt) dU[i] += eU[i];
  for (int i = c.tid; i < nv; i += C::nt) dv[i] += ev[i];
}

// U (the u blocks of z, contiguous), gU and gv_c of one QP.  gl, gv: null is zero.  gz is interleaved like z.
// The caller synchronises before w is used again.
template <class C, class P>
FB_DEV void condense_adjoint_seed(const C& c, int N, int nx, int nu, int nc, const MpcData& D, const double* z,
                                  const double* gz, const double* gl, const double* gv, const CondenseLds& o, P w,
                                  double* U, double* gU, double* gvc) {
  const int ldx = o.ldx, ldc = o.ldc, ldu = o.ldu, ns = nx + nu;
  const P A = w + o.A, Q = w + o.Q, B = w + o.B, E = w + o.E, S = w + o.S;
  const P wb = w + o.carry;  // w_i at wb + i nx
  P pa = wb + (long)(N + 1) * nx + (((N + 1) * nx) & 1), pb = pa + nx + (nx & 1);
  for (int e = c.tid; e < (N + 1) * nu; e += C::nt) {
    const int i = e / nu, r = e - i * nu;
    U[e] = z[(long)i * ns + nx + r];
  }
  for (int r = c.tid; r < nx; r += C::nt) wb[r] = gl ? gl[r] : 0.0;
  // ---- forward: w_i, and gv_c ------------------------------------------------------------------------------
  for (int i = 0; i <= N; i++) {
    const P wi = wb + (long)i * nx;
    condense_stage(c, E, ldc, D.E + (long)i * nc * nx, nc, nx);
    if (i < N) condense_stage(c, A, ldx, D.A + (long)i * nx * nx, nx, nx);
    c.sync();
    for (int r = c.tid; r < nc; r += C::nt)
      gvc[i * nc + r] = (gv ? gv[(long)i * nc + r] : 0.0) + condense_dot_row(E, ldc, r, wi, nx, 0.0);
    if (i < N)
      for (int r = c.tid; r < nx; r += C::nt)
        wi[nx + r] = condense_dot_row(A, ldx, r, wi, nx, 0.0) + (gl ? gl[(long)(i + 1) * nx + r] : 0.0);
    c.sync();
  }
  // ---- backward: p_(j+1), and gU ---------------------------------------------------------------------------
  for (int j = N; j >= 0; j--) {
    const P wj = wb + (long)j * nx;
    condense_stage(c, S, ldu, D.S + (long)j * nu * nx, nu, nx);
    if (j > 0) condense_stage(c, Q, ldx, D.Q + (long)j * nx * nx, nx, nx);
    if (j < N) {
      condense_stage(c, B, ldx, D.B + (long)j * nx * nu, nx, nu);
      if (j > 0) condense_stage(c, A, ldx, D.A + (long)j * nx * nx, nx, nx);
    }
    c.sync();
    for (int r = c.tid; r < nu; r += C::nt) {
      double acc = condense_dot_row(S, ldu, r, wj, nx, 0.0);
      if (j < N) acc = condense_dot_col(B, ldx, r, pa, nx, acc);
      gU[j * nu + r] = acc + gz[(long)j * ns + nx + r];
    }
    if (j > 0)
      for (int r = c.tid; r < nx; r += C::nt) {
        double acc = condense_dot_row(Q, ldx, r, wj, nx, 0.0);
        if (j < N) acc = condense_dot_col(A, ldx, r, pa, nx, acc);
        pb[r] = acc + gz[(long)j * ns + r];
      }
    c.sync();
    const P t = pa; pa = pb; pb = t;
  }
}

// (dz, dl) from (dU, dv) of the dense adjoint, and the gradients of the 12 sequences: every slot of G that is not
// null is written, and (az, al, av) where they are not null receive (dz, dl, dv); ok = false writes zeros to all of
// them.  (z, l, v): the point.  gl: null is zero.  The caller synchronises before w is used again.
// ACC (fbstab_mpc_condensed_sweep_adjoint_finish_kernel): the slots of G are ADDED to, as mpc_adjoint_contract<true>
// adds - by the thread that wrote the entry before, so a caller that zeroes them with the same thread mapping needs
// no synchronisation between the steps it sums over.
#define FB_CONDENSE_ADJOINT_PUT(slot, val) \
  do {                                     \
    if constexpr (ACC) slot += val;        \
    else slot = val;                       \
  } while (0)

template <bool ACC = false, class C, class P>
FB_DEV void condense_adjoint_finish(const C& c, int N, int nx, int nu, int nc, const MpcData& D, const double* z,
                                    const double* l, const double* v, const double* gz, const double* gl,
                                    const double* dU, const double* dvc, const CondenseLds& o, P w, const MpcGrad& G,
                                    bool ok, double* az, double* al, double* av) {
  const int ldx = o.ldx, ldc = o.ldc, ldu = o.ldu, ns = nx + nu;
  const int nzc = (N + 1) * nu, nv = (N + 1) * nc, nz = (N + 1) * ns;
  const int sq = nx * nx, sb = nx * nu;
  const P A = w + o.A, Q = w + o.Q, B = w + o.B, E = w + o.E, S = w + o.S;
  const P dz = w + o.carry;  // (dx_i, du_i) at dz + i ns
  const P dv = dz + nz + (nz & 1);
  P la = dv + nv + (nv & 1), lb = la + nx + (nx & 1);
  for (int e = c.tid; e < nzc; e += C::nt) {
    const int i = e / nu, r = e - i * nu;
    dz[(long)i * ns + nx + r] = dU[e];
  }
  condense_stage(c, dv, nv, dvc, nv, 1);
  for (int r = c.tid; r < nx; r += C::nt) dz[r] = 0.0 - (gl ? gl[r] : 0.0);
  // ---- forward: dx_i ---------------------------------------------------------------------------------------
  for (int i = 0; i < N; i++) {
    const P xi = dz + (long)i * ns;
    condense_stage(c, A, ldx, D.A + (long)i * nx * nx, nx, nx);
    condense_stage(c, B, ldx, D.B + (long)i * nx * nu, nx, nu);
    c.sync();
    for (int r = c.tid; r < nx; r += C::nt) {
      double acc = condense_dot_row(A, ldx, r, xi, nx, 0.0);
      acc = condense_dot_row(B, ldx, r, xi + nx, nu, acc);
      xi[ns + r] = acc - (gl ? gl[(long)(i + 1) * nx + r] : 0.0);
    }
    c.sync();
  }
  // ---- backward: dl_i, and what reads it --------------------------------------------------------------------
  for (int i = N; i >= 0; i--) {
    const P xi = dz + (long)i * ns;
    condense_stage(c, Q, ldx, D.Q + (long)i * nx * nx, nx, nx);
    condense_stage(c, S, ldu, D.S + (long)i * nu * nx, nu, nx);
    condense_stage(c, E, ldc, D.E + (long)i * nc * nx, nc, nx);
    if (i < N) condense_stage(c, A, ldx, D.A + (long)i * nx * nx, nx, nx);
    c.sync();
    for (int r = c.tid; r < nx; r += C::nt) {
      double acc = condense_dot_row(Q, ldx, r, xi, nx, 0.0);
      acc = condense_dot_col(S, ldu, r, xi + nx, nu, acc);
      acc = condense_dot_col(E, ldc, r, dv + i * nc, nc, acc);
      if (i < N) acc = condense_dot_col(A, ldx, r, la, nx, acc);
      acc -= gz[(long)i * ns + r];
      lb[r] = acc;
      if (al) al[(long)i * nx + r] = ok ? acc : 0.0;
    }
    c.sync();
    // (as mpc_adjoint_contract writes them: dl_i is dl_(j+1) of stage j = i - 1)
    if (i > 0) {
      const int j = i - 1;
      const double *xj = z + (long)j * ns, *lp = l + (long)i * nx;
      const P dxj = dz + (long)j * ns;
      if (G.A)
        for (int e = c.tid; e < sq; e += C::nt) {
          const int r = e % nx, k = e / nx;
          FB_CONDENSE_ADJOINT_PUT(G.A[(long)j * sq + e], ok ? -(lb[r] * xj[k] + lp[r] * dxj[k]) : 0.0);
        }
      if (G.B)
        for (int e = c.tid; e < sb; e += C::nt) {
          const int r = e % nx, k = e / nx;
          FB_CONDENSE_ADJOINT_PUT(G.B[(long)j * sb + e], ok ? -(lb[r] * xj[nx + k] + lp[r] * dxj[nx + k]) : 0.0);
        }
      if (G.c)
        for (int e = c.tid; e < nx; e += C::nt) FB_CONDENSE_ADJOINT_PUT(G.c[(long)j * nx + e], ok ? -lb[e] : 0.0);
    } else if (G.x0) {
      for (int e = c.tid; e < nx; e += C::nt) FB_CONDENSE_ADJOINT_PUT(G.x0[e], ok ? -lb[e] : 0.0);
    }
    const P t = la; la = lb; lb = t;
  }
  // ---- the gradients that read (dz, dv) alone --------------------------------------------------------------
  MpcGrad H = G;
  H.A = H.B = H.c = H.x0 = nullptr;
  mpc_adjoint_contract<ACC>(c, N, nx, nu, nc, z, l, v, (const double*)dz, (const double*)nullptr, dvc, H, ok, az,
                            (double*)nullptr, av);
}

#undef FB_CONDENSE_ADJOINT_PUT

}  // namespace fbk
