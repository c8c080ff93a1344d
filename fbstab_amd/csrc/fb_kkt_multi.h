// Many right-hand sides on one factorisation of the Newton matrix (fbstab_hip_mpc_kkt_solve_batch,
// fbstab_hip_mpc_x0_sensitivity_batch): free functions over the flat-vector policy MpcProblem<C, WG> of fb_mpc.h,
// beside mpc_adjoint, so that nothing of fb_mpc.h changes.
//
// The adjoint and the tangent solve V (dz, dl, dv) = (gz, -gl, -C.gv) once per factorisation of V (fb_mpc.h:
// mpc_adjoint).  The factorisation of a stage is the O(nx^3) part of the Riccati solver - two Cholesky
// factorisations, a triangular inverse, two right-hand triangular solves and the P P' + AM AM' products
// (riccati_linear_solver.cc:127-183) - and the vector recursions of a Solve (:212-344) are O(nx^2).  Here
// right-hand side 0 goes through mpc_adjoint itself, which leaves every stage's factors in `fac`, and every
// further one re-runs the vector recursions alone on those factors, as MpcProblem::refine_step does for the
// residual of a step.
//
// Host-compilable against tests/hostsim/shim (tests/hostsim/kkt_multi.cc), like fb_mpc.h.
#pragma once

#include "fb_mpc.h"

namespace fbk {

// One QP's share of the seed and step blocks (fbstab_multi_var_batch_t): vector k of slot i is at
// base[i] + k * rhs_stride[i]; a null base is a zero seed (l, v) or a step slot that is not wanted.  gain: null, or
// the nu x nx column-major image that receives the u0 rows of dz, column k from right-hand side k.
struct KktMultiSlots {
  const double* seed[3];
  long long seed_rs[3];
  double* step[3];
  long long step_rs[3];
  double* gain;
};

// Right-hand side 0: V is factored at x = xbar = the point and solved for (gz, gl, gv) - mpc_adjoint, literally.
// Returns false iff a factorisation failed.
template <class C, bool WG>
FB_DEV bool mpc_kkt_factor(const MpcProblem<C, WG>& p, const C& c, double sigma, double alpha, const double* gz,
                           const double* gl, const double* gv) {
  return mpc_adjoint(p, c, sigma, alpha, gz, gl, gv);
}

// Every further right-hand side, behind a mpc_kkt_factor that returned true: the forward vector recursion of
// riccati_linear_solver.cc:212-262 on the M, Linv, SM, SG, AM, P that newton_step stored per stage, (tx, tu, theta)
// back into `fac`, then the backward sweep and the post sweep of the step.  The formulas are those of
// newton_step<true>, statement by statement, with the matrix work left out; no refinement, as in the adjoint.
//   * (C, mus) of a stage's constraints are RECOMPUTED from y, v, vb with pfb_gradient, not read back: the
//     constraint block's rvm = (-C.gv)/mus is then the expression of newton_step<true> on the same inputs (the stored
//     gam = C/mus would round the product differently).  gam itself is not rewritten: post_sweep's
//     dv = rvm + gam (A dz) reads what the factor pass left.
//   * backward_sweep takes stage N from LDS, not from `fac`: the loop below ends with stage N's factors and its
//     (tx, tu, theta) resident, as refine_step's does.
template <class C, bool WG>
FB_DEV void mpc_kkt_resolve(const MpcProblem<C, WG>& p, const C& c, double sigma, double alpha, const double* gz,
                            const double* gl, const double* gv) {
  typedef typename MpcProblem<C, WG>::mptr mptr;
  const MpcLayout& lay = p.lay;
  const int N = lay.N, nx = lay.nx, nu = lay.nu, nc = lay.nc, ns = lay.ns;
  mptr lds = p.lds;
  mptr tE = lds + lay.t_e; mptr tL = lds + lay.t_l;
  mptr Linv = lds + lay.w_linv; mptr M = lds + lay.w_m;
  mptr AM = lds + lay.w_am; mptr SM = lds + lay.w_sm; mptr SG = lds + lay.w_sg; mptr P = lds + lay.w_p;
  mptr Rvm = lds + lay.w_rvm;
  mptr r1 = lds + lay.w_r1;
  mptr th = lds + lay.w_th; mptr thp = lds + lay.w_thp; mptr hh = lds + lay.w_h;
  mptr tx = lds + lay.w_tx; mptr tu = lds + lay.w_tu;
  mptr t1 = lds + lay.w_t1;
  // the inner residual holds -R (mpc_adjoint): rz = -gz, rl = gl, and rvm carries gv into the stage loop
  for (int i = c.tid; i < p.nz; i += C::nt) p.rz[i] = -gz[i];
  for (int i = c.tid; i < p.nl; i += C::nt) p.rl[i] = gl ? gl[i] : 0.0;
  for (int i = c.tid; i < p.nv; i += C::nt) p.rvm[i] = gv ? gv[i] : 0.0;
  for (int r = c.tid; r < nx; r += C::nt) thp[r] = 0.0;
  c.sync();
  for (int i = 0; i <= N; i++) {
    double* F = p.fac + (long)i * lay.f_stride;
    p.load_tile(c, i);  // (E and L of the stage: r1 below)
    p.copy_in(c, M, F + lay.f_minv, nx * nx);
    p.copy_in(c, Linv, F + lay.f_linv, nx * nx);
    p.copy_in(c, SM, F + lay.f_sm, nu * nx);
    p.copy_in(c, SG, F + lay.f_sginv, nu * nu);
    if (i < N) {
      p.copy_in(c, AM, F + lay.f_am, nx * nx);
      p.copy_in(c, P, F + lay.f_p, nu * nx);
    }
    for (int k = c.tid; k < nc; k += C::nt) {
      const long g = (long)i * nc + k;
      const double vk = p.v[g];
      const double ys = p.y[g] + sigma * (vk - p.vb[g]);
      double g0, g1;
      pfb_gradient(ys, vk, alpha, &g0, &g1);
      const double mu = g1 + sigma * g0;
      const double rm = -(g0 * p.rvm[g]) / mu;  // (-C.gv)/mus
      Rvm[k] = rm;
      p.rvm[g] = rm;
    }
    c.sync();
    // r1 = gz_stage - [E L]' Rvm, theta(i) = theta(i) partial + gl_stage
    for (int r = c.tid; r < ns + nx; r += C::nt) {
      if (r < ns) {
        const long g = (long)i * ns + r;
        double s = -(p.rz[g] + sigma * (p.z[g] - p.zb[g]));
        mptr col = r < nx ? tE + r * nc : tL + (r - nx) * nc;
        for (int k = 0; k < nc; k++) s -= col[k] * Rvm[k];
        r1[r] = s;
      } else {
        const int rr = r - ns;
        const long g = (long)i * nx + rr;
        th[rr] = thp[rr] + (p.rl[g] + sigma * (p.l[g] - p.lb[g]));
      }
    }
    c.sync();
    for (int r = c.tid; r < nx; r += C::nt) {  // w = inv(L) theta
      double s = 0.0;
      for (int k = 0; k <= r; k++) s += Linv[r + k * nx] * th[k];
      t1[r] = s;
    }
    c.sync();
    for (int r = c.tid; r < nx; r += C::nt) {  // h = inv(L)' w - rx
      double s = -r1[r];
      for (int k = r; k < nx; k++) s += Linv[k + r * nx] * t1[k];
      hh[r] = s;
      tx[r] = s;
    }
    c.sync();
    p.solve_lower(c, M, nx, tx);  // tx = inv(M) h
    for (int r = c.tid; r < nu; r += C::nt) {  // t2 = SM tx + ru
      double s = r1[nx + r];
      for (int k = 0; k < nx; k++) s += SM[r + k * nu] * tx[k];
      tu[r] = s;
    }
    c.sync();
    p.solve_lower(c, SG, nu, tu);  // tu = inv(SG) t2
    for (int r = c.tid; r < nx; r += C::nt) {
      F[lay.f_tx + r] = tx[r];
      F[lay.f_th + r] = th[r];
      if (i < N) {  // theta(i+1) partial = P tu + AM tx
        double s = 0.0;
        for (int k = 0; k < nu; k++) s += P[r + k * nx] * tu[k];
        for (int k = 0; k < nx; k++) s += AM[r + k * nx] * tx[k];
        thp[r] = s;
      }
    }
    for (int r = c.tid; r < nu; r += C::nt) F[lay.f_tu + r] = tu[r];
    c.sync();
  }
  p.backward_sweep(c, p.dz, p.dl);
  p.post_sweep(c);
}

// The x0 mode's seed j, written into the workgroup's own scratch (wz, wl: free until a post sweep rewrites them, and
// the solve reads its seeds before that): the tangent's right-hand side for dx0 = e_j, gz = 0, gl = -e_j in the l_0
// block, gv = 0 (fb_tangent.h) - never read from the caller's memory.  Synchronised on return.
template <class C, bool WG>
FB_DEV void mpc_kkt_x0_seed(const MpcProblem<C, WG>& p, const C& c, int j) {
  for (int i = c.tid; i < p.nz; i += C::nt) p.wz[i] = 0.0;
  for (int i = c.tid; i < p.nl; i += C::nt) p.wl[i] = (i == j) ? -1.0 : 0.0;
  c.sync();
}

// The step of the right-hand side just solved (ok), or zeros, to the caller's slots that are not null, and its u0
// rows to column k of the gain.  Synchronised on return (the next right-hand side rewrites the step).
template <class C, bool WG>
FB_DEV void mpc_kkt_store(const MpcProblem<C, WG>& p, const C& c, bool ok, int k, const KktMultiSlots& s) {
  const MpcLayout& lay = p.lay;
  double* oz = s.step[0] ? s.step[0] + k * s.step_rs[0] : nullptr;
  double* ol = s.step[1] ? s.step[1] + k * s.step_rs[1] : nullptr;
  double* ov = s.step[2] ? s.step[2] + k * s.step_rs[2] : nullptr;
  if (oz)
    for (int i = c.tid; i < p.nz; i += C::nt) oz[i] = ok ? p.dz[i] : 0.0;
  if (ol)
    for (int i = c.tid; i < p.nl; i += C::nt) ol[i] = ok ? p.dl[i] : 0.0;
  if (ov)
    for (int i = c.tid; i < p.nv; i += C::nt) ov[i] = ok ? p.dv[i] : 0.0;
  if (s.gain)
    for (int r = c.tid; r < lay.nu; r += C::nt) s.gain[r + (long)k * lay.nu] = ok ? p.dz[lay.nx + r] : 0.0;
  c.sync();
}

// One QP, nrhs right-hand sides: the caller's seeds, or with x0_mode the nrhs = nx unit directions of the initial
// state.  A failed factorisation gives zeros in every output of the QP, for all right-hand sides.  Returns the QP's
// status: false iff the factorisation failed.
template <class C, bool WG>
FB_DEV bool mpc_kkt_multi(const MpcProblem<C, WG>& p, const C& c, double sigma, double alpha, int nrhs, bool x0_mode,
                          const KktMultiSlots& s) {
  bool ok = true;
  for (int k = 0; k < nrhs; k++) {
    const double *gz, *gl, *gv;
    if (x0_mode) {
      if (ok) mpc_kkt_x0_seed(p, c, k);
      gz = p.wz; gl = p.wl; gv = nullptr;
    } else {
      gz = s.seed[0] + k * s.seed_rs[0];
      gl = s.seed[1] ? s.seed[1] + k * s.seed_rs[1] : nullptr;
      gv = s.seed[2] ? s.seed[2] + k * s.seed_rs[2] : nullptr;
    }
    if (k == 0) ok = mpc_kkt_factor(p, c, sigma, alpha, gz, gl, gv);
    else if (ok) mpc_kkt_resolve(p, c, sigma, alpha, gz, gl, gv);
    mpc_kkt_store(p, c, ok, k, s);
  }
  return ok;
}

}  // namespace fbk
