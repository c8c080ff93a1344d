// The right-hand side of the forward mode (fbstab_hip_mpc_tangent_batch, fbstab_hip_dense_tangent_batch): from a
// perturbation of the problem data and the point x = (z, l, v), the seeds (gz, gl, gv) for which the adjoint
// kernels' system V (dz, dl, dv) = (gz, -gl, -C gv) is the tangent system V dx = -dF/dtheta dtheta,
//   gz = -(dH z + df + dG' l + dA' v)      gl = dh - dG z      gv = db - dA z
// (dH: the symmetric part of the perturbation).  It is the mirror of the contraction of fb_adjoint.h: what that
// one writes per sequence, this one reads.  In MPC terms (mpc_data.cc: G = [-I; A B -I; ...], h = -(x0, c), b = -d;
// the constant -I blocks have no perturbation), stage by stage,
//   gz[x_i u_i] = -( sym[dQ_i dS_i'; dS_i dR_i] (x_i, u_i) + (dq_i, dr_i) + d[A_i B_i]' l_(i+1) + d[E_i L_i]' v_i )
//   gl[l_0] = -dx0      gl[l_(i+1)] = -dc_i - d[A_i B_i] (x_i, u_i)      gv[v_i] = -dd_i - d[E_i L_i] (x_i, u_i)
// (stage N has no [A B] term).
// Every image is loaded from memory once per QP, in contiguous runs of 16 B per lane (tangent_stage), into LDS; one
// thread then owns each output entry and sums it from LDS in ascending index order, so that both products an
// image enters (dA x and dA' l, ...) come from the one load.  No atomics, no reduction across threads: a QP's bits
// depend on its own inputs and the shape alone.  A null perturbation pointer is a zero perturbation and is
// neither loaded nor multiplied.
#pragma once

#include "fb_batch.h"

namespace fbk {

// (MpcDir, DenseDir - one QP's perturbations, nullptr: zero - are MpcData and DenseData: fb_batch.h)

// dst[0 .. len) = src[0 .. len): thread c.tid takes the 16-byte pairs c.tid, c.tid + C::nt, ... counted from the
// first 16-byte boundary of src, so that a wavefront's loads are one contiguous run of 16 B per lane; the at most
// two doubles outside the pairs go to thread 0.  The caller synchronises before dst is read.
template <class C, class P>
FB_DEV void tangent_stage(const C& c, P dst, const double* src, int len) {
  const int head = (len > 0 && (((uintptr_t)src >> 3) & 1)) ? 1 : 0;
  const int pairs = (len - head) / 2;
  for (int p = c.tid; p < pairs; p += C::nt) {
    double t[2];
    __builtin_memcpy(t, __builtin_assume_aligned(src + head + 2 * p, 16), 16);
    dst[head + 2 * p] = t[0];
    dst[head + 2 * p + 1] = t[1];
  }
  if (c.tid == 0) {
    if (head) dst[0] = src[0];
    if (head + 2 * pairs < len) dst[len - 1] = src[len - 1];
  }
}

// ---- MPC ------------------------------------------------------------------------------------------------
// Where one stage's images and vectors lie in the LDS of its wavefront (offsets in doubles).
struct MpcTangentLds {
  int Q, R, S, A, B, E, L, x, lp, v, total;
  void init(int nx, int nu, int nc) {
    int o = 0;
    auto take = [&o](int n) { const int at = o; o += n + (n & 1); return at; };  // (even offsets: 16-byte slots)
    Q = take(nx * nx); R = take(nu * nu); S = take(nu * nx); A = take(nx * nx); B = take(nx * nu);
    E = take(nc * nx); L = take(nc * nu); x = take(nx + nu); lp = take(nx); v = take(nc);
    total = o;
  }
};

// Stage i of one QP: loads the stage's images of D that are not null, and (x_i, u_i), l_(i+1), v_i, into w, then
// writes the stage's rows of (gz, gl, gv): gz[i ns .. (i + 1) ns), gl[(i + 1) nx ..) for i < N, gv[i nc ..), and
// gl[0 .. nx) with stage 0.  Threads c.tid, c.tid + C::nt, ... of the ns + nx + nc entries.  The caller
// synchronises before w is used again.
template <class C, class P>
FB_DEV void mpc_tangent_stage(const C& c, int N, int nx, int nu, int nc, int i, const MpcDir& D, const double* z,
                              const double* l, const double* v, const MpcTangentLds& o, P w, double* gz, double* gl,
                              double* gv) {
  const int ns = nx + nu;
  const bool last = i == N;
  const bool hA = D.A && !last, hB = D.B && !last;
  if (D.Q) tangent_stage(c, w + o.Q, D.Q + (long)i * nx * nx, nx * nx);
  if (D.R) tangent_stage(c, w + o.R, D.R + (long)i * nu * nu, nu * nu);
  if (D.S) tangent_stage(c, w + o.S, D.S + (long)i * nu * nx, nu * nx);
  if (hA) tangent_stage(c, w + o.A, D.A + (long)i * nx * nx, nx * nx);
  if (hB) tangent_stage(c, w + o.B, D.B + (long)i * nx * nu, nx * nu);
  if (D.E) tangent_stage(c, w + o.E, D.E + (long)i * nc * nx, nc * nx);
  if (D.L) tangent_stage(c, w + o.L, D.L + (long)i * nc * nu, nc * nu);
  tangent_stage(c, w + o.x, z + (long)i * ns, ns);
  if (!last) tangent_stage(c, w + o.lp, l + (long)(i + 1) * nx, nx);
  tangent_stage(c, w + o.v, v + (long)i * nc, nc);
  c.sync();
  const P Q = w + o.Q, R = w + o.R, S = w + o.S, A = w + o.A, B = w + o.B, E = w + o.E, L = w + o.L;
  const P x = w + o.x, u = w + o.x + nx, lp = w + o.lp, vi = w + o.v;
  for (int e = c.tid; e < ns + nx + nc; e += C::nt) {
    double acc = 0.0;
    if (e < nx) {  // gz, the x rows: sym(dQ) x + dS' u + dq + dA' l_(i+1) + dE' v_i
      const int r = e;
      if (D.Q)
        for (int k = 0; k < nx; k++) acc = fma(0.5 * (Q[r + k * nx] + Q[k + r * nx]), x[k], acc);
      if (D.S)
        for (int j = 0; j < nu; j++) acc = fma(S[j + r * nu], u[j], acc);
      if (D.q) acc += D.q[(long)i * nx + r];
      if (hA)
        for (int m = 0; m < nx; m++) acc = fma(A[m + r * nx], lp[m], acc);
      if (D.E)
        for (int m = 0; m < nc; m++) acc = fma(E[m + r * nc], vi[m], acc);
      gz[(long)i * ns + r] = 0.0 - acc;
    } else if (e < ns) {  // gz, the u rows: sym(dR) u + dS x + dr + dB' l_(i+1) + dL' v_i
      const int r = e - nx;
      if (D.R)
        for (int k = 0; k < nu; k++) acc = fma(0.5 * (R[r + k * nu] + R[k + r * nu]), u[k], acc);
      if (D.S)
        for (int k = 0; k < nx; k++) acc = fma(S[r + k * nu], x[k], acc);
      if (D.r) acc += D.r[(long)i * nu + r];
      if (hB)
        for (int m = 0; m < nx; m++) acc = fma(B[m + r * nx], lp[m], acc);
      if (D.L)
        for (int m = 0; m < nc; m++) acc = fma(L[m + r * nc], vi[m], acc);
      gz[(long)i * ns + nx + r] = 0.0 - acc;
    } else if (e < ns + nx) {  // gl, the rows of l_(i+1): dc_i + dA x + dB u
      const int r = e - ns;
      if (last) continue;
      if (hA)
        for (int k = 0; k < nx; k++) acc = fma(A[r + k * nx], x[k], acc);
      if (hB)
        for (int j = 0; j < nu; j++) acc = fma(B[r + j * nx], u[j], acc);
      if (D.c) acc += D.c[(long)i * nx + r];
      gl[(long)(i + 1) * nx + r] = 0.0 - acc;
    } else {  // gv, the rows of v_i: dd_i + dE x + dL u
      const int r = e - ns - nx;
      if (D.E)
        for (int k = 0; k < nx; k++) acc = fma(E[r + k * nc], x[k], acc);
      if (D.L)
        for (int j = 0; j < nu; j++) acc = fma(L[r + j * nc], u[j], acc);
      if (D.d) acc += D.d[(long)i * nc + r];
      gv[(long)i * nc + r] = 0.0 - acc;
    }
  }
  if (i == 0)
    for (int r = c.tid; r < nx; r += C::nt) gl[r] = D.x0 ? 0.0 - D.x0[r] : 0.0;
}

// ---- dense ----------------------------------------------------------------------------------------------
// Where one QP's vectors, sums and the current block of columns lie in the LDS of its workgroup (doubles).
struct DenseTangentLds {
  int z, l, v, row, col, H, G, A, cb, total;
  // cb: columns per block.  Returns false where not even one column fits into `budget` doubles.
  bool init(int nz, int nl, int nv, int budget) {
    int o = 0;
    auto take = [&o](int n) { const int at = o; o += n + (n & 1); return at; };
    z = take(nz); l = take(nl); v = take(nv); row = take(nz + nl + nv); col = take(nz);
    const int per_col = (nz + 1) + (nl + 1) + (nv + 1);
    cb = (budget - o) / per_col;
    if (cb > nz) cb = nz;
    if (cb < 1) return false;
    H = take(nz * cb); G = take(nl * cb); A = take(nv * cb);
    total = o;
    return true;
  }
};

// One QP.  The column-major images dH (nz x nz), dG (nl x nz), dA (nv x nz) are walked in blocks of o.cb columns
// (a block of columns is one contiguous run of each image); of every block, thread-owned entries take
//   the nz + nl + nv ROW sums    row[r] += M[r, k] z[k]   over the block's columns k, ascending, and
//   the block's COLUMN sums      col[k] = sum_r dH[r, k] z[r] / 2 + sum_m dG[m, k] l[m] + sum_m dA[m, k] v[m]
// (row[r] carried in LDS by the thread that owns it: the same chain of additions for every cb).  Then
//   gz = -((row_H / 2 + col) + df)      gl = dh - row_G      gv = db - row_A
// where row_H / 2 + col is sym(dH) z + dG' l + dA' v.  The caller synchronises before w is used again.
template <class C, class P>
FB_DEV void dense_tangent(const C& c, int nz, int nl, int nv, const DenseDir& D, const double* z, const double* l,
                          const double* v, const DenseTangentLds& o, P w, double* gz, double* gl, double* gv) {
  const int rows = nz + nl + nv;
  const bool hG = D.G && nl > 0;
  tangent_stage(c, w + o.z, z, nz);
  if (nl > 0) tangent_stage(c, w + o.l, l, nl);
  tangent_stage(c, w + o.v, v, nv);
  const P zs = w + o.z, ls = w + o.l, vs = w + o.v, row = w + o.row, col = w + o.col;
  const P Hb = w + o.H, Gb = w + o.G, Ab = w + o.A;
  for (int k0 = 0; k0 < nz; k0 += o.cb) {
    const int wd = nz - k0 < o.cb ? nz - k0 : o.cb;
    c.sync();  // (the block before has been read)
    if (D.H) tangent_stage(c, Hb, D.H + (long)k0 * nz, nz * wd);
    if (hG) tangent_stage(c, Gb, D.G + (long)k0 * nl, nl * wd);
    if (D.A) tangent_stage(c, Ab, D.A + (long)k0 * nv, nv * wd);
    c.sync();
    for (int e = c.tid; e < rows + wd; e += C::nt) {
      if (e < rows) {
        double acc = k0 == 0 ? 0.0 : row[e];
        if (e < nz) {
          if (D.H)
            for (int k = 0; k < wd; k++) acc = fma(0.5 * Hb[e + k * nz], zs[k0 + k], acc);
        } else if (e < nz + nl) {
          if (hG)
            for (int k = 0; k < wd; k++) acc = fma(Gb[(e - nz) + k * nl], zs[k0 + k], acc);
        } else {
          if (D.A)
            for (int k = 0; k < wd; k++) acc = fma(Ab[(e - nz - nl) + k * nv], zs[k0 + k], acc);
        }
        row[e] = acc;
      } else {
        const int k = e - rows;
        double acc = 0.0;
        if (D.H)
          for (int r = 0; r < nz; r++) acc = fma(0.5 * Hb[r + k * nz], zs[r], acc);
        if (hG)
          for (int m = 0; m < nl; m++) acc = fma(Gb[m + k * nl], ls[m], acc);
        if (D.A)
          for (int m = 0; m < nv; m++) acc = fma(Ab[m + k * nv], vs[m], acc);
        col[k0 + k] = acc;
      }
    }
  }
  c.sync();
  for (int e = c.tid; e < nz; e += C::nt) gz[e] = 0.0 - ((row[e] + col[e]) + (D.f ? D.f[e] : 0.0));
  for (int e = c.tid; e < nl; e += C::nt) gl[e] = (D.h ? D.h[e] : 0.0) - row[nz + e];
  for (int e = c.tid; e < nv; e += C::nt) gv[e] = (D.b ? D.b[e] : 0.0) - row[nz + nl + e];
}

}  // namespace fbk
