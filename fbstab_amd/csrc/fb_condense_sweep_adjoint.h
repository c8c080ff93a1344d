// Reverse mode through the closed-loop sweep of the condensed route (fbstab_hip_mpc_condensed_receding_sweep_adjoint).
// Loss: a function of the closed-loop u_0 .. u_(T-1) and x_1 .. x_T; plant x_(k+1) = A_p x_k + B_p u_k (+ w_k) with
// u_k = U_k[0:nu]; step k solves the dense QP (H_c, f_c(x_k), A_c, b_c(x_k)), f_c(x) = f0 + F x, b_c(x) = b0 + G x
// (fb_condense_sweep.h).  Seeds gu[k] = dL/du_k, gx[k] = dL/dx_(k+1).  Per trajectory lambda = 0 and for k = T-1 .. 0
//   mu = gx[k] + lambda                                        (mu_log[k])
//   eflag_log[k] == -1 (retired):        lambda <- 0
//   eflag_log[k] != FBSTAB_SUCCESS:      lambda <- A_p' mu
//   otherwise the dense adjoint at the logged (U_k, v_k) with the seed gU = (gu[k] + B_p' mu, 0, .., 0), gv_c = 0 -
//   the condensing seed map (fb_condense_adjoint.h) is the identity on a seed that lives on u_0 alone - refined once
//   as fbstab_hip_mpc_condensed_adjoint_batch refines it:
//     a factorisation failed:            status += 1, lambda <- A_p' mu
//     else                               lambda <- A_p' mu + F'(-dU) + G' dv
// The dense adjoint's gradients are f_bar = -dU and b_bar = dv, and f_c, b_c reach x_k through M = [F; G] alone:
// F'(-dU) + G' dv is -dl[0:nx] of condense_adjoint_finish, without the finish.  The backward step is the transpose of
// the forward step's matrix-vector product: lambda[j] = sum_r A_p[r][j] mu[r] + sum_e M[e][j] g[e], g = [-dU; dv].
// Column j of M is contiguous in the column-major image, and in LDS the odd leading dimension ne | 1 keeps the
// threads of neighbouring j off one bank.  (RECONDENSE mode has no map: there the finish runs at every step and the
// close reads its -dl[0:nx].)
//
// condense_sweep_adjoint_step is the backward mirror of condense_sweep_step, T trajectories per workgroup in the
// CondenseSweepLds layout: one launch CLOSES step k + 1 (the case rule, lambda) and OPENS step k (mu, the seed, and
// f_c, b_c of step k from x_log[k] with the forward kernel's loop and summation order); lambda stays in LDS between
// the two parts.  The gradients of the other 11 sequences are condense_adjoint_finish<true> at the expanded logged
// point, summed over the contributing steps, last step first (condense_sweep_adjoint_finish).
//
// As fb_condense.h: written against Ctx, one thread owns each output entry and sums it in ascending index order with
// plain FMAs.  No atomics, no sums across threads, no matrix cores.
//
// Not here: the device-side reduced form for shared parameters, seeds on the rest of U_k and v_k, reuse of the forward
// call's images and map, sharded sweeps, the C++ facade.  (Forward mode: fb_condense_sweep_tangent.h.  Per-step
// references need no code here: the host stage hands the step kernel the f0, b0 of the step it opens and the finish
// kernel the step's sequences and, for a sequence that moves, the step's rows of its gradient - fb_condense_stage.h.)
#pragma once

#include "fb_condense_adjoint.h"
#include "fb_condense_plan.h"  // (CondenseSweepAdjStep, CondenseSweepAdjFinish)
#include "fb_condense_sweep.h"

namespace fbk {

// Trajectories t0 .. t0 + Tg of the batch, Tg <= L.T.  No synchronisation is needed behind it.
template <class C, class P>
FB_DEV void condense_sweep_adjoint_step(const C& c, const CondenseSweepAdjStep& a, const CondenseSweepLds& L, long t0,
                                        int Tg, P w) {
  const int N = a.N, nx = a.nx, nu = a.nu, nc = a.nc;
  const int nzc = (N + 1) * nu, nv = (N + 1) * nc, ne = nzc + nv;
  const int ex = (int)condense_sweep_even(nx), eU = (int)condense_sweep_even(nzc), ev = (int)condense_sweep_even(nv);
  // xs: lambda, then x_log[k]; xn: mu; Us, vs: g = [-dU; dv]; gs: the case of the closed step
  const P Ml = w + L.M, xs = w + L.x, xn = w + L.xn, Us = w + L.U, vs = w + L.v, gs = w + L.gone;
  if (a.affine && L.m_lds) condense_stage(c, Ml, L.ldm, a.M, ne, nx);
  // ---- close step k + 1: the case rule (0: retired, 1: the plant alone, 2: the adjoint contributes) ---------------
  if (a.close) {
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
      xn[t * ex + r] = a.mu[(t0 + t) * nx + r];
    }
    c.sync();
    for (int i = c.tid; i < Tg * nzc; i += C::nt) {
      const int t = i / nzc, e = i - t * nzc;
      const long q = t0 + t;
      const bool good = gs[t] == 2.0;
      const double g = good ? 0.0 - a.dU[q * nzc + e] : 0.0;
      Us[t * eU + e] = g;
      if (a.gf0 && good) a.gf0[q * nzc + e] += g;
    }
    for (int i = c.tid; i < Tg * nv; i += C::nt) {
      const int t = i / nv, e = i - t * nv;
      const long q = t0 + t;
      const bool good = gs[t] == 2.0;
      const double g = good ? a.dv[q * nv + e] : 0.0;
      vs[t * ev + e] = g;
      if (a.gb0 && good) a.gb0[q * nv + e] += g;
    }
    c.sync();
    // lambda[j] = sum_r A_p[r][j] mu[r] + sum_e M[e][j] g[e]
    for (int i = c.tid; i < Tg * nx; i += C::nt) {
      const int t = i / nx, j = i - t * nx;
      const long q = t0 + t;
      double acc = 0.0;
      if (gs[t] != 0.0) {
        const double* Aq = a.Ap + q * a.sAp + (long)j * nx;
        for (int r = 0; r < nx; r++) acc = fma(Aq[r], xn[t * ex + r], acc);
      }
      if (gs[t] == 2.0) {
        if (!a.affine) {
          acc = acc + a.dl0[q * nx + j];
        } else if (L.m_lds) {
          const P Mj = Ml + j * L.ldm;
          for (int e = 0; e < nzc; e++) acc = fma(Mj[e], Us[t * eU + e], acc);
          for (int e = 0; e < nv; e++) acc = fma(Mj[nzc + e], vs[t * ev + e], acc);
        } else {
          const double* Mj = a.M + q * a.sM + (long)j * ne;
          for (int e = 0; e < nzc; e++) acc = fma(Mj[e], Us[t * eU + e], acc);
          for (int e = 0; e < nv; e++) acc = fma(Mj[nzc + e], vs[t * ev + e], acc);
        }
      }
      xs[t * ex + j] = acc;
    }
  } else {
    for (int i = c.tid; i < Tg * nx; i += C::nt) {
      const int t = i / nx, j = i - t * nx;
      xs[t * ex + j] = 0.0;
    }
  }
  c.sync();
  if (!a.open) {
    if (a.gx0)
      for (int i = c.tid; i < Tg * nx; i += C::nt) {
        const int t = i / nx, j = i - t * nx;
        a.gx0[(t0 + t) * a.sgx0 + j] = xs[t * ex + j];
      }
    return;
  }
  // ---- open step k: mu = gx[k] + lambda ---------------------------------------------------------------------------
  for (int i = c.tid; i < Tg * nx; i += C::nt) {
    const int t = i / nx, r = i - t * nx;
    const long q = t0 + t;
    const double m = (a.gx ? a.gx[q * nx + r] : 0.0) + xs[t * ex + r];
    xn[t * ex + r] = m;
    a.mu[q * nx + r] = m;
    if (a.mu_log) a.mu_log[q * nx + r] = m;
    if (a.dl0) a.dl0[q * nx + r] = 0.0;
  }
  c.sync();
  // the seed: gU[0:nu] = gu[k] + B_p' mu, zeros behind it; zero where the step does not contribute
  for (int i = c.tid; i < Tg * nzc; i += C::nt) {
    const int t = i / nzc, e = i - t * nzc;
    const long q = t0 + t;
    double acc = 0.0;
    if (e < nu && a.eflag_open[q] == FBSTAB_SUCCESS) {
      const double* Bq = a.Bp + q * a.sBp + (long)e * nx;
      acc = a.gu ? a.gu[q * nu + e] : 0.0;
      for (int r = 0; r < nx; r++) acc = fma(Bq[r], xn[t * ex + r], acc);
    }
    a.gU[q * nzc + e] = acc;
  }
  if (!a.affine) return;
  // ---- f_c and b_c of step k: base + M x_log[k], as condense_sweep_step forms them -----------------------------------
  for (int i = c.tid; i < Tg * nx; i += C::nt) {
    const int t = i / nx, r = i - t * nx;
    xs[t * ex + r] = a.x_log[(t0 + t) * nx + r];
  }
  c.sync();
  for (int i = c.tid; i < Tg * ne; i += C::nt) {
    const int t = i / ne, e = i - t * ne;
    const long q = t0 + t;
    double acc = 0.0;
    if (L.m_lds) {
      for (int j = 0; j < nx; j++) acc = fma(Ml[e + j * L.ldm], xs[t * ex + j], acc);
    } else {
      const double* Mq = a.M + q * a.sM;
      for (int j = 0; j < nx; j++) acc = fma(Mq[e + (long)j * ne], xs[t * ex + j], acc);
    }
    if (e < nzc) a.f[q * a.sf + e] = a.f0[q * a.sf0 + e] + acc;
    else a.b[q * a.sb + (e - nzc)] = a.b0[q * a.sb0 + (e - nzc)] + acc;
  }
}

// One trajectory, one step: condense_expand of the logged point (U, v) at the state xk into (z, l), then the
// accumulating finish with the dense step (dU, dv), gl = 0 and gz = zeros (the finish reads its x entries alone).
// G: the caller's slots of this trajectory with the x0 slot replaced (null, or -dl[0:nx] for a close without a map:
// it is zero on entry).  D: the data with x0 := xk.  ok = false adds nothing.
template <class C, class P>
FB_DEV void condense_sweep_adjoint_finish(const C& c, int N, int nx, int nu, int nc, const MpcData& D, const double* U,
                                          const double* v, const double* dU, const double* dv, const double* gz,
                                          const CondenseLds& o, P w, const MpcGrad& G, bool ok, double* z, double* l) {
  if (!ok) return;
  condense_expand(c, N, nx, nu, nc, D, U, v, (const double*)nullptr, o, w, z, l, (double*)nullptr, (double*)nullptr);
  c.sync();
  condense_adjoint_finish<true>(c, N, nx, nu, nc, D, (const double*)z, (const double*)l, v, gz, (const double*)nullptr,
                                dU, dv, o, w, G, true, (double*)nullptr, (double*)nullptr, (double*)nullptr);
}

// Before the first step: zeros in every slot of G that is not null, by the threads that add to the entries later
// (the mapping of condense_adjoint_finish and mpc_adjoint_contract: entry e by thread e mod C::nt), in gz, and in the
// trajectory's gf0, gb0 and status.
template <class C>
FB_DEV void condense_sweep_adjoint_begin(const C& c, int N, int nx, int nu, int nc, const MpcGrad& G, double* gz,
                                         double* gf0, double* gb0, int* status) {
  const int sq = nx * nx, sr = nu * nu, su = nu * nx, sb = nx * nu, se = nc * nx, sl = nc * nu;
  const long len[12] = {(long)(N + 1) * sq, (long)(N + 1) * sr, (long)(N + 1) * su, (long)(N + 1) * nx,
                        (long)(N + 1) * nu, (long)N * sq, (long)N * sb, (long)N * nx, (long)(N + 1) * se,
                        (long)(N + 1) * sl, (long)(N + 1) * nc, nx};
  double* const slot[12] = {G.Q, G.R, G.S, G.q, G.r, G.A, G.B, G.c, G.E, G.L, G.d, G.x0};
  for (int s = 0; s < 12; s++)
    if (slot[s])
      for (long e = c.tid; e < len[s]; e += C::nt) slot[s][e] = 0.0;
  if (gz)
    for (long e = c.tid; e < (long)(N + 1) * (nx + nu); e += C::nt) gz[e] = 0.0;
  if (gf0)
    for (long e = c.tid; e < (long)(N + 1) * nu; e += C::nt) gf0[e] = 0.0;
  if (gb0)
    for (long e = c.tid; e < (long)(N + 1) * nc; e += C::nt) gb0[e] = 0.0;
  if (c.tid == 0) *status = 0;
}

}  // namespace fbk
