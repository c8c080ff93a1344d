// Forward mode through the closed-loop sweep of the condensed route (fbstab_hip_mpc_condensed_receding_sweep_tangent).
// The logged sweep solved, at step k of a trajectory, the dense QP (H_c, f_c = f0_k + F x_k, A_c, b_c = b0_k + G x_k)
// and logged x_k, (U_k, v_k) and eflag_k; u_k = U_k[0:nu], x_(k+1) = A_p x_k + B_p u_k (+ w_k) (fb_condense_sweep.h).
// Directions dx0, dw_k, df0_k, db0_k.  Per trajectory dx = dx0 and for k = 0 .. steps-1
//   eflag_log[k] == -1 (retired):        du_k = 0, dx <- 0                (the parked state is the constant 0)
//   eflag_log[k] != FBSTAB_SUCCESS:      du_k = 0, dx <- A_p dx + dw_k    (u_k is a constant, as in the adjoint)
//   otherwise df_c = df0_k + F dx, db_c = db0_k + G dx and one dense adjoint at the logged (U_k, v_k) with the seeds
//   gU = -df_c, gv_c = db_c - the seeds fbstab_hip_dense_tangent_batch forms for (df, db) - refined once as
//   fbstab_hip_mpc_condensed_adjoint_batch refines it:
//     a factorisation failed:            status += 1, du_k = 0, dx <- A_p dx + dw_k
//     else                               du_k = dU[0:nu], dx <- A_p dx + B_p du_k + dw_k
//   du_out[k] = du_k, dx_out[k] = dx (= dx_(k+1)).
// This is the transpose of the recursion of fb_condense_sweep_adjoint.h, case for case:
//   sum_k <gu_k, du_k> + <gx_k, dx_(k+1)> = <lambda_0, dx0> + sum_k <mu_k, dw_k> [not retired] + <gf0, df0> + <gb0, db0>.
//
// condense_sweep_tangent_step is the forward mirror of condense_sweep_adjoint_step, T trajectories per workgroup in
// the CondenseSweepLds layout: one launch CLOSES step k (the case rule, du_k, dx+ in the summation order of the forward
// kernel's plant step) and OPENS step k + 1: f_c, b_c of that step from x_log[k + 1] exactly as condense_sweep_step
// forms them - the dense handle needs b_c at the point - and the seeds from dx+, which stays in LDS between the two
// parts.  Both products with M are formed in ONE pass over a row of M, two accumulators per thread (e, trajectory):
// M is read once, from LDS or from memory.
//
// As fb_condense.h: written against Ctx, one thread owns each output entry and sums it in ascending index order with
// plain FMAs.  No atomics, no sums across threads, no matrix cores.
//
// Not here: directions on matrix sequences, several directions per factorisation, RECONDENSE mode (a sweep that ran in
// that mode is differentiated through the map of fbstab_hip_mpc_condensed_x0_map_batch), the reduced form, sharded
// sweeps, the C++ facade, the record-kernel sweep.  (Directions of q, r, c, d - data or per-step references - need no
// code here: the images are linear in those four sequences, so fbstab_hip_mpc_condensed_reference_images_batch on the
// direction sequences gives df0_k, db0_k.)
#pragma once

#include "fb_condense.h"
#include "fb_condense_plan.h"  // (CondenseSweepLds, CondenseSweepTanStep)

namespace fbk {

// Trajectories t0 .. t0 + Tg of the batch, Tg <= L.T.  No synchronisation is needed behind it.
template <class C, class P>
FB_DEV void condense_sweep_tangent_step(const C& c, const CondenseSweepTanStep& a, const CondenseSweepLds& L, long t0,
                                        int Tg, P w) {
  const int N = a.N, nx = a.nx, nu = a.nu, nc = a.nc;
  const int nzc = (N + 1) * nu, nv = (N + 1) * nc, ne = nzc + nv;
  const int ex = (int)condense_sweep_even(nx), eU = (int)condense_sweep_even(nzc);
  // xs: dx, then x_log[k + 1]; xn: dx+; Us: du_k in its first nu entries; gs: the case of the closed step
  const P Ml = w + L.M, xs = w + L.x, xn = w + L.xn, Us = w + L.U, gs = w + L.gone;
  if (a.open && L.m_lds) condense_stage(c, Ml, L.ldm, a.M, ne, nx);
  if (a.close) {
    // ---- close step k: the case rule (0: retired, 1: the plant alone, 2: the step contributes) -------------------
    for (int t = c.tid; t < Tg; t += C::nt) {
      const long q = t0 + t;
      const int eflag = a.eflag_close[q];
      int cs = eflag == -1 ? 0 : eflag != FBSTAB_SUCCESS ? 1 : 2;
      if (cs == 2 && (a.st1[q] != 0 || a.st2[q] != 0)) {
        cs = 1;
        a.status[q] += 1;
      }
      gs[t] = (double)cs;
    }
    for (int i = c.tid; i < Tg * nx; i += C::nt) {
      const int t = i / nx, r = i - t * nx;
      xs[t * ex + r] = a.dx[(t0 + t) * nx + r];
    }
    c.sync();
    for (int i = c.tid; i < Tg * nu; i += C::nt) {
      const int t = i / nu, j = i - t * nu;
      const long q = t0 + t;
      const double d = gs[t] == 2.0 ? a.dU[q * nzc + j] : 0.0;
      Us[t * eU + j] = d;
      if (a.du_out) a.du_out[q * nu + j] = d;
    }
    c.sync();
    // dx+ = A_p dx + B_p du (+ dw), in the order of condense_sweep_step's plant
    for (int i = c.tid; i < Tg * nx; i += C::nt) {
      const int t = i / nx, r = i - t * nx;
      const long q = t0 + t;
      double acc = 0.0;
      if (gs[t] != 0.0) {
        const double* Aq = a.Ap + q * a.sAp;
        for (int m = 0; m < nx; m++) acc = fma(Aq[r + m * nx], xs[t * ex + m], acc);
        if (gs[t] == 2.0) {
          const double* Bq = a.Bp + q * a.sBp;
          for (int j = 0; j < nu; j++) acc = fma(Bq[r + j * nx], Us[t * eU + j], acc);
        }
        acc = acc + (a.dw ? a.dw[q * nx + r] : 0.0);
      }
      xn[t * ex + r] = acc;
      a.dx[q * nx + r] = acc;
      if (a.dx_out) a.dx_out[q * nx + r] = acc;
    }
  } else {
    // ---- before the first step: dx = dx0, nothing has counted yet -------------------------------------------------
    for (int t = c.tid; t < Tg; t += C::nt) a.status[t0 + t] = 0;
    for (int i = c.tid; i < Tg * nx; i += C::nt) {
      const int t = i / nx, r = i - t * nx;
      const long q = t0 + t;
      const double d = a.dx0 ? a.dx0[q * a.sdx0 + r] : 0.0;
      xn[t * ex + r] = d;
      a.dx[q * nx + r] = d;
    }
  }
  if (!a.open) return;
  c.sync();
  // ---- open step k + 1: f_c, b_c = base + M x_log[k + 1] as condense_sweep_step forms them, and the seeds
  // gU = -(df0 + F dx+), gv_c = db0 + G dx+, zero where the step does not contribute ---------------------------------
  for (int i = c.tid; i < Tg * nx; i += C::nt) {
    const int t = i / nx, r = i - t * nx;
    xs[t * ex + r] = a.x_log[(t0 + t) * nx + r];
  }
  c.sync();
  for (int i = c.tid; i < Tg * ne; i += C::nt) {
    const int t = i / ne, e = i - t * ne;
    const long q = t0 + t;
    double acc = 0.0, dac = 0.0;
    if (L.m_lds) {
      for (int j = 0; j < nx; j++) {
        const double m = Ml[e + j * L.ldm];
        acc = fma(m, xs[t * ex + j], acc);
        dac = fma(m, xn[t * ex + j], dac);
      }
    } else {
      const double* Mq = a.M + q * a.sM;
      for (int j = 0; j < nx; j++) {
        const double m = Mq[e + (long)j * ne];
        acc = fma(m, xs[t * ex + j], acc);
        dac = fma(m, xn[t * ex + j], dac);
      }
    }
    const bool good = a.eflag_open[q] == FBSTAB_SUCCESS;
    if (e < nzc) {
      a.f[q * a.sf + e] = a.f0[q * a.sf0 + e] + acc;
      const double d = (a.df0 ? a.df0[q * a.sdf0 + e] : 0.0) + dac;
      a.gU[q * nzc + e] = good ? 0.0 - d : 0.0;
    } else {
      const int r = e - nzc;
      a.b[q * a.sb + r] = a.b0[q * a.sb0 + r] + acc;
      const double d = (a.db0 ? a.db0[q * a.sdb0 + r] : 0.0) + dac;
      a.gv[q * nv + r] = good ? d : 0.0;
    }
  }
}

}  // namespace fbk
