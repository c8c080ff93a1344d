// Many right-hand sides on one factorisation of the dense Newton matrix (fbstab_hip_dense_kkt_solve_batch,
// fbstab_hip_dense_jacobian_batch): free functions over the two dense policies - DenseProblem<C, KGLOBAL, VGLOBAL> of
// fb_dense.h and DenseWave of fb_dense_wave.h - beside dense_adjoint, so that nothing of those headers changes
// (what fb_kkt_multi.h is to fb_mpc.h).
//
// The adjoint and the tangent solve V (dz, dl, dv) = (gz, -gl, -C.gv) once per factorisation of V (fb_dense.h:
// dense_adjoint).  DenseCholeskySolver::Initialize is the O(nz^2 nv + n^3) part - A'Gamma A and the LDL' of the
// n = nz + nl matrix K (dense_cholesky_solver.cc:32-79) - and a Solve (:81-127) is O(n^2 + nz nv).  Here K is
// factored once per QP and every right-hand side runs the vector part of the step alone on the stored factors.
//
// The four-wavefront part is host-compilable against tests/hostsim/shim with FB_DENSE_NO_MFMA
// (tests/hostsim/dense_kkt_multi.cc), like fb_dense.h; the one-wavefront part needs a wavefront and is left out there.
#pragma once

#include "fb_batch.h"  // FBSTAB_DENSE_*
#include "fb_dense.h"
#if !defined(FB_DENSE_NO_MFMA)
#include "fb_dense_wave.h"
#endif

namespace fbk {

// One QP's share of the seed and step blocks (fbstab_multi_var_batch_t): vector k of slot i is at
// base[i] + k * rhs_stride[i]; a null base is a zero seed (l, v) or a step slot that is not wanted.
struct DenseKktSlots {
  const double* seed[3];
  long long seed_rs[3];
  double* step[3];
  long long step_rs[3];
};

// `wrt` of the kernels: the caller's seeds, or the Jacobian mode's array (FBSTAB_DENSE_f, _h, _b), whose seeds are
// generated in the kernel with the tangent's signs (fb_tangent.h: gz = -df, gl = dh, gv = db).
constexpr int kDenseKktSeeded = -1;

// The seeds of right-hand side k, entry by entry: read from the caller's vectors, or the Jacobian mode's unit seed
// - gz = -e_k (f), gl = e_k (h), gv = e_k (b) - never read from memory.
struct DenseKktSeed {
  const double *gz, *gl, *gv;
  int wrt, k;
  FB_DEV double z(int i) const {
    if (wrt == kDenseKktSeeded) return gz[i];
    return (wrt == FBSTAB_DENSE_f && i == k) ? -1.0 : 0.0;
  }
  FB_DEV double l(int i) const {
    if (wrt == kDenseKktSeeded) return gl ? gl[i] : 0.0;
    return (wrt == FBSTAB_DENSE_h && i == k) ? 1.0 : 0.0;
  }
  FB_DEV double v(int i) const {
    if (wrt == kDenseKktSeeded) return gv ? gv[i] : 0.0;
    return (wrt == FBSTAB_DENSE_b && i == k) ? 1.0 : 0.0;
  }
};

FB_DEV DenseKktSeed dense_kkt_seed(const DenseKktSlots& s, int wrt, int k) {
  DenseKktSeed sd;
  sd.wrt = wrt;
  sd.k = k;
  sd.gz = sd.gl = sd.gv = nullptr;
  if (wrt == kDenseKktSeeded) {
    sd.gz = s.seed[0] + k * s.seed_rs[0];
    sd.gl = s.seed[1] ? s.seed[1] + k * s.seed_rs[1] : nullptr;
    sd.gv = s.seed[2] ? s.seed[2] + k * s.seed_rs[2] : nullptr;
  }
  return sd;
}

// The step of the right-hand side just solved (ok), or zeros, to the caller's slots that are not null.
// Synchronised on return (the next right-hand side rewrites the step).  P: DenseProblem or DenseWave.
template <class P, class C>
FB_DEV void dense_kkt_store(const P& p, const C& c, bool ok, int k, const DenseKktSlots& s) {
  double* oz = s.step[0] ? s.step[0] + k * s.step_rs[0] : nullptr;
  double* ol = s.step[1] ? s.step[1] + k * s.step_rs[1] : nullptr;
  double* ov = s.step[2] ? s.step[2] + k * s.step_rs[2] : nullptr;
  if (oz)
    for (int i = c.tid; i < p.nz; i += C::nt) oz[i] = ok ? p.dz[i] : 0.0;
  if (ol)
    for (int i = c.tid; i < p.nl; i += C::nt) ol[i] = ok ? p.dl[i] : 0.0;
  if (ov)
    for (int i = c.tid; i < p.nv; i += C::nt) ov[i] = ok ? p.dv[i] : 0.0;
  c.sync();
}

// ---- the four-wavefront policy (DenseProblem<C, KGLOBAL, VGLOBAL>) ---------------------------------------------
// Right-hand side 0 goes through dense_adjoint itself (dense_kkt_multi below), which leaves the factored K (and, by
// layout, the multipliers, pivots and elimination order beside it), gam, and the point in z, l, v, zb, lb, vb.

// Every further right-hand side, behind a dense_adjoint that returned true: the vector part of newton_step<true>,
// statement by statement, with the assembly of K and its factorisation left out.
//   * (g0, mu) of a row are RECOMPUTED from y, v, vb with pfb_gradient, not read back: yb = -(g0 rvm) and
//     rvm = yb / mu are then the expressions of newton_step<true> on the same inputs (the stored gam = g0 / mu would
//     round the products differently) - the reason fb_kkt_multi.h gives for (C, mus).  gam is not rewritten.
//   * the three layouts' right-hand sides are one expression: A_col_dot is col_dot on the caller's A where A is not
//     in LDS.
//   * ldlt_solve works on `rhs` alone.
//   * W = (H dz + G'dl + A'dv, -G dz) is left out: nothing reads it here.
template <class P, class C>
FB_DEV void dense_kkt_resolve(const P& p, const C& c, double sigma, double alpha, const DenseKktSeed& sd) {
  const int n = p.lay.nk, nz = p.nz, nl = p.nl, nv = p.nv;
  // the inner residual holds -R (dense_adjoint): rz = -gz, rl = gl, and rvm carries gv into the gradient loop
  for (int i = c.tid; i < nz; i += C::nt) p.rz[i] = -sd.z(i);
  for (int i = c.tid; i < nl; i += C::nt) p.rl[i] = sd.l(i);
  for (int i = c.tid; i < nv; i += C::nt) p.rvm[i] = sd.v(i);
  c.sync();
  for (int i = c.tid; i < nv; i += C::nt) {
    const double ys = p.y[i] + sigma * (p.v[i] - p.vb[i]);
    double g0, g1;
    pfb_gradient(ys, p.v[i], alpha, &g0, &g1);
    const double mu = g1 + sigma * g0;
    p.yb[i] = -(g0 * p.rvm[i]);  // rv = -C.gv, kept for dv below
    p.rvm[i] = p.yb[i] / mu;
  }
  c.sync();
  // the eliminated right-hand side (dense_cholesky_solver.cc:98-104)
  for (int j = c.tid; j < n; j += C::nt) {
    if (j < nz) {
      p.rhs[j] = -(p.rz[j] + sigma * (p.z[j] - p.zb[j])) - p.A_col_dot(j, p.rvm);
    } else {
      const int q = j - nz;
      p.rhs[j] = p.rl[q] + sigma * (p.l[q] - p.lb[q]);
    }
  }
  c.sync();
  p.ldlt_solve(c);
  for (int i = c.tid; i < n; i += C::nt) {
    if (i < nz) p.dz[i] = p.rhs[i];
    else p.dl[i - nz] = p.rhs[i];
  }
  c.sync();
  for (int i = c.tid; i < nv; i += C::nt) {
    const double a = p.A_row_dot(i, p.dz);
    p.adz[i] = a;
    p.dv[i] = p.dv_as_the_reference(i, a, sigma, alpha);
  }
  c.sync();
}

// Right-hand side 0 of the Jacobian mode: dense_adjoint takes its seeds as vectors in memory, and the generated ones
// live nowhere, so its statements stand here with the seed read entry by entry.  Returns false iff the factorisation
// failed.
template <class P, class C>
FB_DEV bool dense_kkt_factor_generated(const P& p, const C& c, double sigma, double alpha, const DenseKktSeed& sd) {
  p.load_guess(c);  // (z, l, v) <- the point, y = b - A z
  for (int i = c.tid; i < p.nz; i += C::nt) { p.zb[i] = p.z[i]; p.rz[i] = -sd.z(i); }
  for (int i = c.tid; i < p.nl; i += C::nt) { p.lb[i] = p.l[i]; p.rl[i] = sd.l(i); }
  for (int i = c.tid; i < p.nv; i += C::nt) { p.vb[i] = p.v[i]; p.rvm[i] = sd.v(i); }
  c.sync();
  return p.template newton_step<true>(c, sigma, alpha);
}

// One QP, nrhs right-hand sides: the caller's seeds, or the unit seeds of `wrt`.  A failed factorisation gives
// zeros in every output of the QP, for all right-hand sides.  Returns the QP's status: false iff the factorisation
// failed.
template <class C, bool KG, bool VG>
FB_DEV bool dense_kkt_multi(const DenseProblem<C, KG, VG>& p, const C& c, double sigma, double alpha, int nrhs,
                            int wrt, const DenseKktSlots& s) {
  bool ok = true;
  for (int k = 0; k < nrhs; k++) {
    const DenseKktSeed sd = dense_kkt_seed(s, wrt, k);
    if (k == 0) {
      if (wrt == kDenseKktSeeded) ok = dense_adjoint(p, c, sigma, alpha, sd.gz, sd.gl, sd.gv);
      else ok = dense_kkt_factor_generated(p, c, sigma, alpha, sd);
    } else if (ok) {
      dense_kkt_resolve(p, c, sigma, alpha, sd);
    }
    dense_kkt_store(p, c, ok, k, s);
  }
  return ok;
}

#if !defined(FB_DENSE_NO_MFMA)
// ---- the one-wavefront policy (DenseWave, nz + nl <= 64) -------------------------------------------------------
// DenseWave::factor returns the elimination order and the pivots in registers and newton_step<true> drops them, so
// this path writes the step out itself.  Once per QP: the point, the PFB-gradient loop of newton_step<true> (gam
// alone: no seed exists yet, and rvm is zeroed for the sum `assemble` forms beside the matrix-core product, which is
// dropped), `assemble`, `factor` - always the pivoted rule, as the adjoint, and the nfallback counters left alone.
// Then per right-hand side, number 0 included, so that a seed's step depends neither on its slot nor on the other
// seeds: (yb, rvm) from the seed as in newton_step<true>, the eliminated right-hand side with A' rvm as a column dot,
// `substitute` on the multipliers in the workgroup's scratch (re-read per right-hand side; Kr is dead by then, and
// `substitute` holds lk[64] in its place), A dz and dv_of<true>.  These are not the bits of the adjoint kernel
// (column dot against the matrix-core operands' sum; A_row_dot against its two-row loop): the same accuracy.
// Returns false iff the factorisation failed.
FB_DEV bool dense_wave_kkt_multi(const DenseWave& p, const DenseWave::C& c, double sigma, double alpha, int nrhs,
                                 int wrt, const DenseKktSlots& s) {
  p.load_guess(c);  // (z, l, v) <- the point, y = b - A z
  for (int i = c.tid; i < p.nz; i += 64) p.zb[i] = p.z[i];
  for (int i = c.tid; i < p.nl; i += 64) p.lb[i] = p.l[i];
  for (int i = c.tid; i < p.nv; i += 64) p.vb[i] = p.v[i];
  c.sync();
  int t = c.tid;
  asm volatile("" : "+v"(t));  // (see DenseWave::assemble)
  const int nz = p.nz, nv = p.nv, n = p.lay.nk;
  DenseWave::d4 hd[10];
  p.load_hd(t, hd);  // (on its way while the gradients are formed)
  for (int i = t; i < nv; i += 64) {
    const double ys = p.y[i] + sigma * (p.v[i] - p.vb[i]);
    double g0, g1;
    pfb_gradient(ys, p.v[i], alpha, &g0, &g1);
    const double mu = g1 + sigma * g0;
    p.gam[i] = g0 / mu;
    p.rvm[i] = 0.0;
  }
  c.sync();
  int ord = 64, permv = 0;
  double dpiv = 0.0;
  bool ok;
  {
    double Kr[64], dg, atr;
    p.assemble(c, hd, sigma, Kr, &dg, &atr);
    ok = p.factor(c, Kr, dg, &ord, &dpiv, &permv);
  }
  for (int k = 0; k < nrhs; k++) {
    if (ok) {
      const DenseKktSeed sd = dense_kkt_seed(s, wrt, k);
      for (int i = t; i < nv; i += 64) {
        const double ys = p.y[i] + sigma * (p.v[i] - p.vb[i]);
        double g0, g1;
        pfb_gradient(ys, p.v[i], alpha, &g0, &g1);
        const double mu = g1 + sigma * g0;
        p.yb[i] = -(g0 * sd.v(i));  // rv = -C.gv, kept for dv below
        p.rvm[i] = p.yb[i] / mu;
      }
      c.sync();
      // eliminated right-hand side (dense_cholesky_solver.cc:98-104), entry t in lane t: rz = -gz, rl = gl
      double x = 0.0;
      if (t < nz) {
        const double rhs0 = -(-sd.z(t) + sigma * (p.z[t] - p.zb[t]));
        x = rhs0 - p.A_col_dot(t, p.rvm);
      } else if (t < n) {
        x = sd.l(t - nz) + sigma * (p.l[t - nz] - p.lb[t - nz]);
      }
      x = p.substitute(t, x, ord, dpiv, permv);
      if (t < nz) p.dz[t] = x;
      else if (t < n) p.dl[t - nz] = x;
      c.sync();
      for (int i = t; i < nv; i += 64) {
        const double a = p.A_row_dot(i, p.dz);
        p.adz[i] = a;
        p.dv[i] = p.dv_of<true>(i, a, sigma, alpha);
      }
      c.sync();
    }
    dense_kkt_store(p, c, ok, k, s);
  }
  return ok;
}
#endif  // !FB_DENSE_NO_MFMA

}  // namespace fbk
