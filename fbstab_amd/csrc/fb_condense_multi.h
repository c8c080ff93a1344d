// Many right-hand sides on the condensed MPC route (fbstab_hip_mpc_condensed_kkt_solve_batch,
// fbstab_hip_mpc_condensed_x0_sensitivity_batch): the two maps of fb_condense_adjoint.h around the dense multi-solve
// (fbstab_hip_dense_kkt_solve_batch), for R right-hand sides per workgroup.  The formulas, the signs and the order of
// every sum are those of condense_adjoint_seed / _residual / _correct / _finish, right-hand side by right-hand side;
// what changes is who computes them: a stage's images are staged into the window of CondenseLds ONCE and used by all
// R right-hand sides of the group, thread (row r, right-hand side k) owns entry r of right-hand side k, and the
// mat-vecs of the sweeps become mat-mats that keep R nx threads busy instead of nx.  No contraction: the step
// (dz, dl, dv) is the result.
//
// The carry region behind the window holds R copies of one right-hand side's vectors, `per` doubles each:
//   seed:    w_i of every stage and two p                        e((N + 1) nx) + 2 e(nx)
//   finish:  dz (interleaved like z), dv and two dl              e((N + 1)(nx + nu)) + e((N + 1) nc) + 2 e(nx)
// (e(n): n rounded up to even), per = the larger of the two.  R changes who computes an entry, never how: a right-hand
// side's bits depend on its seed, the QP's data and the shape alone - not on R, its slot or the other seeds.
//
// As fb_condense.h: written against Ctx, one thread per output entry, sums in ascending index order, no atomics.
#pragma once

#include "fb_condense_adjoint.h"
#include "fb_condense_plan.h"  // (condense_multi_per, condense_multi_rule, CondenseMultiWork)

namespace fbk {

// The seeds of one QP: right-hand side k of slot i at base + k * rhs_stride, a null gl or gv is zero; or, in x0 mode,
// right-hand side k is gz = 0, gl = -e_k in the l_0 block, gv = 0 (the tangent's seeds for dx0 = e_k), generated here.
// Both sources run the same arithmetic on the values they return: x0 mode is bitwise the explicit seeds.
struct CondenseMultiSeeds {
  const double *gz, *gl, *gv;
  long long rz, rl, rv;
  int x0_mode;
  FB_DEV double z(int k, long i) const { return x0_mode ? 0.0 : gz[k * rz + i]; }
  FB_DEV double l(int k, long i) const { return x0_mode ? (i == k ? -1.0 : 0.0) : (gl ? gl[k * rl + i] : 0.0); }
  FB_DEV double v(int k, long i) const { return x0_mode ? 0.0 : (gv ? gv[k * rv + i] : 0.0); }
};

// Right-hand sides k0 .. k0 + Rg - 1 of one QP: gU and gv_c (right-hand side k at gU + k nzc, gvc + k nv), and U
// where it is not null.  The caller synchronises before w is used again.
template <class C, class P>
FB_DEV void condense_multi_seed(const C& c, int N, int nx, int nu, int nc, const MpcData& D, const double* z,
                                const CondenseMultiSeeds& sd, int k0, int Rg, long per, const CondenseLds& o, P w,
                                double* U, double* gU, double* gvc) {
  const int ldx = o.ldx, ldc = o.ldc, ldu = o.ldu, ns = nx + nu;
  const int nzc = (N + 1) * nu, nv = (N + 1) * nc;
  const P A = w + o.A, Q = w + o.Q, B = w + o.B, E = w + o.E, S = w + o.S;
  const P cb = w + o.carry;  // copy kk at cb + kk per: w_i at + i nx, then two p
  const long po = (long)(N + 1) * nx + (((N + 1) * nx) & 1), ps = nx + (nx & 1);
  long pa = po, pb = po + ps;
  if (U)
    for (int e = c.tid; e < nzc; e += C::nt) {
      const int i = e / nu, r = e - i * nu;
      U[e] = z[(long)i * ns + nx + r];
    }
  for (int e = c.tid; e < nx * Rg; e += C::nt) {
    const int kk = e / nx, r = e - kk * nx;
    cb[kk * per + r] = sd.l(k0 + kk, r);
  }
  // ---- forward: w_i, and gv_c ------------------------------------------------------------------------------
  for (int i = 0; i <= N; i++) {
    condense_stage(c, E, ldc, D.E + (long)i * nc * nx, nc, nx);
    if (i < N) condense_stage(c, A, ldx, D.A + (long)i * nx * nx, nx, nx);
    c.sync();
    for (int e = c.tid; e < nc * Rg; e += C::nt) {
      const int kk = e / nc, r = e - kk * nc, k = k0 + kk;
      const P wi = cb + kk * per + (long)i * nx;
      gvc[(long)k * nv + i * nc + r] = sd.v(k, (long)i * nc + r) + condense_dot_row(E, ldc, r, wi, nx, 0.0);
    }
    if (i < N)
      for (int e = c.tid; e < nx * Rg; e += C::nt) {
        const int kk = e / nx, r = e - kk * nx;
        const P wi = cb + kk * per + (long)i * nx;
        wi[nx + r] = condense_dot_row(A, ldx, r, wi, nx, 0.0) + sd.l(k0 + kk, (long)(i + 1) * nx + r);
      }
    c.sync();
  }
  // ---- backward: p_(j+1), and gU ---------------------------------------------------------------------------
  for (int j = N; j >= 0; j--) {
    condense_stage(c, S, ldu, D.S + (long)j * nu * nx, nu, nx);
    if (j > 0) condense_stage(c, Q, ldx, D.Q + (long)j * nx * nx, nx, nx);
    if (j < N) {
      condense_stage(c, B, ldx, D.B + (long)j * nx * nu, nx, nu);
      if (j > 0) condense_stage(c, A, ldx, D.A + (long)j * nx * nx, nx, nx);
    }
    c.sync();
    for (int e = c.tid; e < nu * Rg; e += C::nt) {
      const int kk = e / nu, r = e - kk * nu, k = k0 + kk;
      const P wj = cb + kk * per + (long)j * nx, p = cb + kk * per + pa;
      double acc = condense_dot_row(S, ldu, r, wj, nx, 0.0);
      if (j < N) acc = condense_dot_col(B, ldx, r, p, nx, acc);
      gU[(long)k * nzc + j * nu + r] = acc + sd.z(k, (long)j * ns + nx + r);
    }
    if (j > 0)
      for (int e = c.tid; e < nx * Rg; e += C::nt) {
        const int kk = e / nx, r = e - kk * nx;
        const P wj = cb + kk * per + (long)j * nx, p = cb + kk * per + pa;
        double acc = condense_dot_row(Q, ldx, r, wj, nx, 0.0);
        if (j < N) acc = condense_dot_col(A, ldx, r, p, nx, acc);
        cb[kk * per + pb + r] = acc + sd.z(k0 + kk, (long)j * ns + r);
      }
    c.sync();
    const long t = pa; pa = pb; pb = t;
  }
}

// (hi, lo) += a b without the rounding of the product or of the sum (Ogita, Rump, Oishi 2005: Dot2); only lo rounds.
FB_DEV void condense_multi_dot2(double a, double b, double& hi, double& lo) {
#pragma clang fp contract(off)  // (the error terms below are those of a ROUNDED product and sum)
  const double p = a * b, e = fma(a, b, -p);
  const double s = hi + p, t = s - hi;
  lo += ((hi - (s - t)) + (p - t)) + e;
  hi = s;
}

// rU = gU - (H_c dU + sigma dU + A_c' dv) for the Rg right-hand sides at gU, dU, rU (+ kk nzc) and dv (+ kk nv): the
// terms of condense_adjoint_residual in its order, per right-hand side, summed in twice the working precision and
// rounded once.  On a QP without active rows the dense step is already at its rounding and a residual summed in
// double is that step's own noise: adding the correction of noise makes the step worse, not better (measured: the
// dense rule of the tests missed on exactly those QPs).  The threads of one row read the same entries of H_c and A_c.
template <class C>
FB_DEV void condense_multi_residual(const C& c, int nzc, int nv, int Rg, const double* H, const double* A,
                                    double sigma, const double* gU, const double* dU, const double* dv, double* rU) {
#pragma clang fp contract(off)
  for (int e = c.tid; e < nzc * Rg; e += C::nt) {
    const int kk = e / nzc, i = e - kk * nzc;
    const double *u = dU + (long)kk * nzc, *d = dv + (long)kk * nv;
    double hi = 0.0, lo = 0.0;
    condense_multi_dot2(sigma, u[i], hi, lo);
    for (int j = 0; j < nzc; j++) condense_multi_dot2(H[i + (long)j * nzc], u[j], hi, lo);
    const double* a = A + (long)i * nv;
    for (int k = 0; k < nv; k++) condense_multi_dot2(a[k], d[k], hi, lo);
    // g - (hi + lo): the difference g - hi with its rounding error, then lo
    const double g = gU[(long)kk * nzc + i];
    const double s = g - hi, t = s - g;
    rU[(long)kk * nzc + i] = s + (((g - (s - t)) + ((0.0 - hi) - t)) - lo);
  }
}

// (dU, dv) += (eU, ev) for Rg right-hand sides, and where gain is not null (x0 mode) column k0 + kk of the nu x nx
// column-major image: the u_0 rows of the corrected dU (zero where ok is false, as the step is).
template <class C>
FB_DEV void condense_multi_correct(const C& c, int nzc, int nv, int nu, int k0, int Rg, const double* eU,
                                   const double* ev, double* dU, double* dv, double* gain, bool ok) {
  for (int e = c.tid; e < nzc * Rg; e += C::nt) {
    const int kk = e / nzc, i = e - kk * nzc;
    const double s = dU[e] + eU[e];
    dU[e] = s;
    if (gain && i < nu) gain[(long)(k0 + kk) * nu + i] = ok ? s : 0.0;
  }
  for (int e = c.tid; e < nv * Rg; e += C::nt) dv[e] += ev[e];
}

// (dz, dl, dv) of right-hand sides k0 .. k0 + Rg - 1 from (dU, dv) of the dense step (right-hand side k at
// dU + k nzc, dvc + k nv): the sweeps of condense_adjoint_finish.  az, al, av: the QP's step slots (right-hand side k
// at + k rz / rl / rv), null slots are skipped; ok = false writes zeros.  The caller synchronises before w is used
// again.
template <class C, class P>
FB_DEV void condense_multi_finish(const C& c, int N, int nx, int nu, int nc, const MpcData& D,
                                  const CondenseMultiSeeds& sd, int k0, int Rg, long per, const double* dU,
                                  const double* dvc, const CondenseLds& o, P w, bool ok, double* az, long long rz,
                                  double* al, long long rl, double* av, long long rv) {
  const int ldx = o.ldx, ldc = o.ldc, ldu = o.ldu, ns = nx + nu;
  const int nzc = (N + 1) * nu, nv = (N + 1) * nc, nz = (N + 1) * ns;
  const P A = w + o.A, Q = w + o.Q, B = w + o.B, E = w + o.E, S = w + o.S;
  const P cb = w + o.carry;  // copy kk at cb + kk per: (dx_i, du_i) at + i ns, then dv and two dl
  const long vo = nz + (nz & 1);
  long la = vo + nv + (nv & 1), lb = la + nx + (nx & 1);
  for (int e = c.tid; e < nzc * Rg; e += C::nt) {
    const int kk = e / nzc, m = e - kk * nzc, i = m / nu, r = m - i * nu;
    cb[kk * per + (long)i * ns + nx + r] = dU[(long)(k0 + kk) * nzc + m];
  }
  for (int e = c.tid; e < nv * Rg; e += C::nt) {
    const int kk = e / nv, m = e - kk * nv;
    const double t = dvc[(long)(k0 + kk) * nv + m];
    cb[kk * per + vo + m] = t;
    if (av) av[(k0 + kk) * rv + m] = ok ? t : 0.0;
  }
  for (int e = c.tid; e < nx * Rg; e += C::nt) {
    const int kk = e / nx, r = e - kk * nx;
    cb[kk * per + r] = 0.0 - sd.l(k0 + kk, r);
  }
  // ---- forward: dx_i ---------------------------------------------------------------------------------------
  for (int i = 0; i < N; i++) {
    condense_stage(c, A, ldx, D.A + (long)i * nx * nx, nx, nx);
    condense_stage(c, B, ldx, D.B + (long)i * nx * nu, nx, nu);
    c.sync();
    for (int e = c.tid; e < nx * Rg; e += C::nt) {
      const int kk = e / nx, r = e - kk * nx;
      const P xi = cb + kk * per + (long)i * ns;
      double acc = condense_dot_row(A, ldx, r, xi, nx, 0.0);
      acc = condense_dot_row(B, ldx, r, xi + nx, nu, acc);
      xi[ns + r] = acc - sd.l(k0 + kk, (long)(i + 1) * nx + r);
    }
    c.sync();
  }
  if (az)
    for (int e = c.tid; e < nz * Rg; e += C::nt) {
      const int kk = e / nz, m = e - kk * nz;
      az[(k0 + kk) * rz + m] = ok ? cb[kk * per + m] : 0.0;
    }
  if (!al) return;
  // ---- backward: dl_i --------------------------------------------------------------------------------------
  for (int i = N; i >= 0; i--) {
    condense_stage(c, Q, ldx, D.Q + (long)i * nx * nx, nx, nx);
    condense_stage(c, S, ldu, D.S + (long)i * nu * nx, nu, nx);
    condense_stage(c, E, ldc, D.E + (long)i * nc * nx, nc, nx);
    if (i < N) condense_stage(c, A, ldx, D.A + (long)i * nx * nx, nx, nx);
    c.sync();
    for (int e = c.tid; e < nx * Rg; e += C::nt) {
      const int kk = e / nx, r = e - kk * nx, k = k0 + kk;
      const P xi = cb + kk * per + (long)i * ns, dv = cb + kk * per + vo;
      double acc = condense_dot_row(Q, ldx, r, xi, nx, 0.0);
      acc = condense_dot_col(S, ldu, r, xi + nx, nu, acc);
      acc = condense_dot_col(E, ldc, r, dv + i * nc, nc, acc);
      if (i < N) acc = condense_dot_col(A, ldx, r, cb + kk * per + la, nx, acc);
      acc -= sd.z(k, (long)i * ns + r);
      cb[kk * per + lb + r] = acc;
      al[k * rl + (long)i * nx + r] = ok ? acc : 0.0;
    }
    c.sync();
    const long t = la; la = lb; lb = t;
  }
}

}  // namespace fbk
