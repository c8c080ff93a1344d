// The contraction of the MPC adjoint (fbstab_hip_mpc_adjoint_batch), shared by the flat-vector kernel
// (fb_mpc.h: mpc_adjoint_gradients) and the one-row record instances (fb_record_kernel.h: the adjoint kernel):
// from the point x = (z, l, v) and the adjoint step (dz, dl, dv), theta_bar = -J_theta' w for the MPC data,
// stage by stage in the reference layout (column-major stage matrices, mpc_data.cc:17-289).  With x_i, u_i the
// parts of z and dx_i, du_i those of dz,
//   q_i, r_i: -dx_i, -du_i           x0: -dl_0      c_i: -dl_(i+1)      d_i: -dv_i
//   Q_i: -(dx x' + x dx')/2          R_i: -(du u' + u du')/2            S_i: -(du x' + u dx')
//   A_i: -(dl_(i+1) x_i' + l_(i+1) dx_i')       B_i: -(dl_(i+1) u_i' + l_(i+1) du_i')
//   E_i: -(dv_i x_i' + v_i dx_i')               L_i: -(dv_i u_i' + v_i du_i')
// (Q and R get the gradient of their symmetric part: the reference assumes symmetric blocks.)
#pragma once

#include "fb_batch.h"

namespace fbk {

// (MpcGrad, DenseGrad: fb_batch.h)
// Every slot of G that is not null is written; ok = false writes zeros there, and to (az, al, av) where they are
// not null (which otherwise receive dz, dl, dv).  Threads c.tid, c.tid + C::nt, ... of every sequence; the
// caller synchronises before and after.  ACC (fbstab_mpc_r16_sweep_adjoint_kernel): the slots of G are ADDED to
// - by the thread that wrote the entry before, so a caller that zeroes them with the same thread mapping needs no
// synchronisation between the steps it sums over.
// One entry of a gradient slot: stored, or (ACC: the sweep adjoint's sum over the steps) added to what is there.
// (A macro, so that the store of the instantiations without ACC is the statement it always was.)
#define FB_ADJOINT_PUT(slot, val) \
  do {                            \
    if constexpr (ACC) slot += val; \
    else slot = val;              \
  } while (0)

template <bool ACC = false, class C>
FB_DEV void mpc_adjoint_contract(const C& c, int N, int nx, int nu, int nc, const double* z, const double* l,
                                 const double* v, const double* dz, const double* dl, const double* dv,
                                 const MpcGrad& G, bool ok, double* az, double* al, double* av) {
  const int ns = nx + nu;
  const int sq = nx * nx, sr = nu * nu, su = nu * nx, sb = nx * nu, se = nc * nx, sl = nc * nu;
  if (G.Q)
    for (int e = c.tid; e < (N + 1) * sq; e += C::nt) {
      const int i = e / sq, r = (e % sq) % nx, k = (e % sq) / nx;
      const double *x = z + (long)i * ns, *dx = dz + (long)i * ns;
      FB_ADJOINT_PUT(G.Q[e], ok ? -0.5 * (dx[r] * x[k] + x[r] * dx[k]) : 0.0);
    }
  if (G.R)
    for (int e = c.tid; e < (N + 1) * sr; e += C::nt) {
      const int i = e / sr, r = (e % sr) % nu, k = (e % sr) / nu;
      const double *u = z + (long)i * ns + nx, *du = dz + (long)i * ns + nx;
      FB_ADJOINT_PUT(G.R[e], ok ? -0.5 * (du[r] * u[k] + u[r] * du[k]) : 0.0);
    }
  if (G.S)
    for (int e = c.tid; e < (N + 1) * su; e += C::nt) {
      const int i = e / su, r = (e % su) % nu, k = (e % su) / nu;
      const double *x = z + (long)i * ns, *dx = dz + (long)i * ns;
      FB_ADJOINT_PUT(G.S[e], ok ? -(dx[nx + r] * x[k] + x[nx + r] * dx[k]) : 0.0);
    }
  if (G.q)
    for (int e = c.tid; e < (N + 1) * nx; e += C::nt) FB_ADJOINT_PUT(G.q[e], ok ? -dz[(long)(e / nx) * ns + e % nx] : 0.0);
  if (G.r)
    for (int e = c.tid; e < (N + 1) * nu; e += C::nt) FB_ADJOINT_PUT(G.r[e], ok ? -dz[(long)(e / nu) * ns + nx + e % nu] : 0.0);
  if (G.A)
    for (int e = c.tid; e < N * sq; e += C::nt) {
      const int i = e / sq, r = (e % sq) % nx, k = (e % sq) / nx;
      const double *x = z + (long)i * ns, *dx = dz + (long)i * ns;
      const double *lp = l + (long)(i + 1) * nx, *dlp = dl + (long)(i + 1) * nx;
      FB_ADJOINT_PUT(G.A[e], ok ? -(dlp[r] * x[k] + lp[r] * dx[k]) : 0.0);
    }
  if (G.B)
    for (int e = c.tid; e < N * sb; e += C::nt) {
      const int i = e / sb, r = (e % sb) % nx, k = (e % sb) / nx;
      const double *u = z + (long)i * ns + nx, *du = dz + (long)i * ns + nx;
      const double *lp = l + (long)(i + 1) * nx, *dlp = dl + (long)(i + 1) * nx;
      FB_ADJOINT_PUT(G.B[e], ok ? -(dlp[r] * u[k] + lp[r] * du[k]) : 0.0);
    }
  if (G.c)
    for (int e = c.tid; e < N * nx; e += C::nt) FB_ADJOINT_PUT(G.c[e], ok ? -dl[nx + e] : 0.0);
  if (G.E)
    for (int e = c.tid; e < (N + 1) * se; e += C::nt) {
      const int i = e / se, r = (e % se) % nc, k = (e % se) / nc;
      const double *x = z + (long)i * ns, *dx = dz + (long)i * ns;
      const double *vi = v + (long)i * nc, *dvi = dv + (long)i * nc;
      FB_ADJOINT_PUT(G.E[e], ok ? -(dvi[r] * x[k] + vi[r] * dx[k]) : 0.0);
    }
  if (G.L)
    for (int e = c.tid; e < (N + 1) * sl; e += C::nt) {
      const int i = e / sl, r = (e % sl) % nc, k = (e % sl) / nc;
      const double *u = z + (long)i * ns + nx, *du = dz + (long)i * ns + nx;
      const double *vi = v + (long)i * nc, *dvi = dv + (long)i * nc;
      FB_ADJOINT_PUT(G.L[e], ok ? -(dvi[r] * u[k] + vi[r] * du[k]) : 0.0);
    }
  if (G.d)
    for (int e = c.tid; e < (N + 1) * nc; e += C::nt) FB_ADJOINT_PUT(G.d[e], ok ? -dv[e] : 0.0);
  if (G.x0)
    for (int e = c.tid; e < nx; e += C::nt) FB_ADJOINT_PUT(G.x0[e], ok ? -dl[e] : 0.0);
  const long nz = (long)(N + 1) * ns, nl = (long)(N + 1) * nx, nv = (long)(N + 1) * nc;
  if (az)
    for (long e = c.tid; e < nz; e += C::nt) az[e] = ok ? dz[e] : 0.0;
  if (al)
    for (long e = c.tid; e < nl; e += C::nt) al[e] = ok ? dl[e] : 0.0;
  if (av)
    for (long e = c.tid; e < nv; e += C::nt) av[e] = ok ? dv[e] : 0.0;
}

#undef FB_ADJOINT_PUT

// ---- dense (fbstab_hip_dense_adjoint_batch) -------------------------------------------------------------
// The same contraction for the dense data min 1/2 z'Hz + f'z s.t. Gz = h, Az <= b (h and b enter directly):
//   f: -dz      h: dl      b: dv
//   H: -(dz z' + z dz')/2 (the gradient of the symmetric part)      G: -(dl z' + l dz')      A: -(dv z' + v dz')
// column-major like the inputs (H_bar[r + c nz], G_bar[r + c nl], A_bar[r + c nv]).

// out[r + k m] = s (a[r] z[k] + w[r] dz[k]), r < m, k < nz: thread c.tid takes entries c.tid, c.tid + C::nt, ...
// of the column-major image, so that a wavefront's stores are one contiguous run; (r, k) follow the entry
// without a division.
template <class C, class VP>
FB_DEV void dense_adjoint_outer(const C& c, double* out, int m, int nz, double s, VP a, VP w, VP z, VP dz, bool ok) {
  if (m <= 0) return;
  int r = c.tid % m, k = c.tid / m;
  for (int e = c.tid; e < m * nz; e += C::nt) {
    out[e] = ok ? s * (a[r] * z[k] + w[r] * dz[k]) : 0.0;
    r += C::nt;
    while (r >= m) { r -= m; k++; }
  }
}

// Every slot of G that is not null is written; ok = false writes zeros there, and to (az, al, av) where they are
// not null (which otherwise receive dz, dl, dv).  VP: where the policy keeps its vectors (LDS, or global scratch
// for DenseLayout::v_global).  The caller synchronises before and after.
template <class C, class VP>
FB_DEV void dense_adjoint_contract(const C& c, int nz, int nl, int nv, VP z, VP l, VP v, VP dz, VP dl, VP dv,
                                   const DenseGrad& G, bool ok, double* az, double* al, double* av) {
  if (G.H) dense_adjoint_outer(c, G.H, nz, nz, -0.5, dz, z, z, dz, ok);
  if (G.G) dense_adjoint_outer(c, G.G, nl, nz, -1.0, dl, l, z, dz, ok);
  if (G.A) dense_adjoint_outer(c, G.A, nv, nz, -1.0, dv, v, z, dz, ok);
  if (G.f)
    for (int e = c.tid; e < nz; e += C::nt) G.f[e] = ok ? -dz[e] : 0.0;
  if (G.h)
    for (int e = c.tid; e < nl; e += C::nt) G.h[e] = ok ? dl[e] : 0.0;
  if (G.b)
    for (int e = c.tid; e < nv; e += C::nt) G.b[e] = ok ? dv[e] : 0.0;
  if (az)
    for (int e = c.tid; e < nz; e += C::nt) az[e] = ok ? dz[e] : 0.0;
  if (al)
    for (int e = c.tid; e < nl; e += C::nt) al[e] = ok ? dl[e] : 0.0;
  if (av)
    for (int e = c.tid; e < nv; e += C::nt) av[e] = ok ? dv[e] : 0.0;
}

}  // namespace fbk
