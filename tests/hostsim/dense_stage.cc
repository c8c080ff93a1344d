// TEST INFRASTRUCTURE ONLY - the stages of fbstab_amd/csrc/fb_dense.h on one host thread, for
// tests/test_dense_rules_cpu.py: DenseLayout::init as the compiled header decides it (the path map), and
// DenseProblem<Ctx<1>>'s ldlt (ldlt_impl on a workgroup narrower than a wavefront), ldlt_solve (ldlt_solve_impl),
// newton_step and dense_adjoint, with the same outputs as the device probe (tests/kernels/dense_probe.hip), so that
// the rules of tests/dense_rules.py are shown to pass the actual code before anything reaches a GPU.  Compiled
// against tests/hostsim/shim like the other entries; not part of libfbstab_hip.so.  With -DDENSE_STAGE_MAIN it is
// a stand-alone program over a few fixed shapes (the sanitizer build of tests/test_dense_rules_cpu.py).
#define FB_DENSE_NO_MFMA 1  // (the K assembly on the matrix cores needs four wavefronts; the scalar loop is the same sum)
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../fbstab_amd/csrc/fb_dense.h"

using namespace fbk;
typedef Ctx<1> C1;

// DenseLayout::init(nz, nl, nv, nthreads): out = {wave, k_global, v_global, a_lds, lds_doubles, lda, nk}; returns
// k_doubles + v_doubles.
extern "C" long hostsim_dense_path(int nz, int nl, int nv, int nthreads, int* out) {
  DenseLayout lay;
  lay.init(nz, nl, nv, nthreads);
  out[0] = lay.wave; out[1] = lay.k_global; out[2] = lay.v_global; out[3] = lay.a_lds; out[4] = lay.lds_doubles;
  out[5] = lay.lda; out[6] = lay.nk;
  return lay.k_doubles + lay.v_doubles;
}

namespace {

struct Host {
  std::vector<double> lds, ks;
  C1 ctx;
  explicit Host(const DenseLayout& lay) : lds(lay.lds_doubles + 2, 0.0), ks(lay.k_doubles + lay.v_doubles + 2, 0.0) {
    ctx.tid = 0;
    ctx.red = lds.data() + lay.o_red;
  }
};

template <class P>
void put_factors(const P& p, int* perm, double* Kout) {
  const int n = p.lay.nk;
  for (int i = 0; i < n; i++) perm[i] = p.perm[i];
  std::memcpy(Kout, p.K, sizeof(double) * n * n);
}

template <bool KG, bool VG>
int factor(const DenseLayout& lay, const double* img, const double* rhs, int* perm, double* Kout, double* x) {
  Host h(lay);
  DenseData D = {};
  DenseProblem<C1, KG, VG> p;
  p.bind(lay, D, nullptr, nullptr, nullptr, nullptr, h.lds.data(), h.ks.data());
  const int n = lay.nk;
  std::memcpy(p.K, img, sizeof(double) * n * n);
  for (int i = 0; i < n; i++) p.rhs[i] = rhs[i];
  if (!p.ldlt(h.ctx)) return 0;
  put_factors(p, perm, Kout);
  p.ldlt_solve(h.ctx);
  for (int i = 0; i < n; i++) x[i] = p.rhs[i];
  return 1;
}

// outs: y, rz, rl, dz, dl, dv, adz, wz, wl, gam, rvm, yb (the order of tests/dense_probe.py)
template <bool KG, bool VG>
int step(const DenseLayout& lay, const DenseData& D, const double* z, const double* l, const double* v,
         const double* Hstep, const double* zb, const double* lb, const double* vb, double sigma, double alpha,
         int adjoint, int* perm, double* Kout, double* const* outs) {
  Host h(lay);
  const int nz = lay.nz, nl = lay.nl, nv = lay.nv;
  std::vector<double> uz(z, z + nz), ul(l, l + nl), uv(v, v + nv);
  DenseProblem<C1, KG, VG> p;
  p.bind(lay, D, uz.data(), ul.data(), uv.data(), nullptr, h.lds.data(), h.ks.data());
  // (as the device probe: the K region starts as a sentinel NaN, and the step reads its H from Hstep)
  const long long sentinel = 0x7ff80000dead0000LL;
  for (long e = 0; e < (long)lay.nk * lay.nk; e++) std::memcpy(&p.K[e], &sentinel, sizeof(double));
  bool ok;
  if (adjoint) {
    p.D.H = Hstep;
    ok = dense_adjoint(p, h.ctx, sigma, alpha, zb, lb, vb);
  } else {
    p.load_guess(h.ctx);
    p.residual(h.ctx);
    for (int i = 0; i < nz; i++) p.zb[i] = zb[i];
    for (int i = 0; i < nl; i++) p.lb[i] = lb[i];
    for (int i = 0; i < nv; i++) p.vb[i] = vb[i];
    p.D.H = Hstep;
    ok = p.template newton_step<false>(h.ctx, sigma, alpha);
  }
  const double* src[12] = {p.y, p.rz, p.rl, p.dz, p.dl, p.dv, p.adz, p.wz, p.wl, p.gam, p.rvm, p.yb};
  const int len[12] = {nv, nz, nl, nz, nl, nv, nv, nz, nl, nv, nv, nv};
  for (int k = 0; k < 12; k++) {
    const bool always = k < 3 || k >= 9;  // (the others exist only behind a true verdict)
    if ((ok || always) && (k != 11 || adjoint)) std::memcpy(outs[k], src[k], sizeof(double) * len[k]);
  }
  if (ok) put_factors(p, perm, Kout);
  return ok ? 1 : 0;
}

}  // namespace

// ldlt and ldlt_solve on an image (n x n by columns) behind the layout of (n, 0, nv); returns the verdict.
extern "C" int hostsim_dense_stage_factor(int n, int nv, const double* img, const double* rhs, int* perm,
                                          double* Kout, double* x) {
  DenseLayout lay;
  lay.init(n, 0, nv, 1);
  if (lay.v_global) return factor<true, true>(lay, img, rhs, perm, Kout, x);
  if (lay.k_global) return factor<true, false>(lay, img, rhs, perm, Kout, x);
  return factor<false, false>(lay, img, rhs, perm, Kout, x);
}

extern "C" int hostsim_dense_stage_step(int nz, int nl, int nv, const double* const* data, const double* z,
                                        const double* l, const double* v, const double* Hstep, const double* zb,
                                        const double* lb, const double* vb, double sigma, double alpha, int adjoint, int* perm,
                                        double* Kout, double* const* outs) {
  DenseLayout lay;
  lay.init(nz, nl, nv, 1);
  DenseData D = {data[0], data[1], data[2], data[3], data[4], data[5]};
  if (lay.v_global) return step<true, true>(lay, D, z, l, v, Hstep, zb, lb, vb, sigma, alpha, adjoint, perm, Kout, outs);
  if (lay.k_global) return step<true, false>(lay, D, z, l, v, Hstep, zb, lb, vb, sigma, alpha, adjoint, perm, Kout, outs);
  return step<false, false>(lay, D, z, l, v, Hstep, zb, lb, vb, sigma, alpha, adjoint, perm, Kout, outs);
}

#ifdef DENSE_STAGE_MAIN
// A fixed pseudo-random problem per shape through both entries and both forms of the step; every output must come
// back finite.  The placements: everything in LDS, A in global memory, K in scratch, K and the vectors in scratch.
static double lcg(unsigned long long& s) {
  s = s * 6364136223846793005ULL + 1442695040888963407ULL;
  return ((double)(s >> 11) / 9007199254740992.0) * 2.0 - 1.0;
}

int main() {
  const int shapes[][3] = {{1, 0, 1}, {7, 2, 5}, {20, 5, 40}, {20, 5, 330}, {66, 3, 4}, {140, 0, 4}, {20, 5, 2534}};
  unsigned long long s = 12345;
  for (const auto& sh : shapes) {
    const int nz = sh[0], nl = sh[1], nv = sh[2], n = nz + nl;
    std::vector<double> H(nz * nz), f(nz), G(nl * nz + 1), hh(nl + 1), A((size_t)nv * nz), b(nv), z(nz), l(nl + 1),
        v(nv), zb(nz), lb(nl + 1), vb(nv);
    for (int i = 0; i < nz; i++)
      for (int j = 0; j <= i; j++) H[i + j * nz] = H[j + i * nz] = (i == j ? 2.0 + nz : 0.0) + lcg(s);
    for (auto* a : {&f, &G, &hh, &A, &b, &z, &l, &zb, &lb})
      for (auto& e : *a) e = lcg(s);
    for (int i = 0; i < nv; i++) { v[i] = std::fabs(lcg(s)); vb[i] = std::fabs(lcg(s)); }
    const double* data[6] = {H.data(), f.data(), G.data(), hh.data(), A.data(), b.data()};
    std::vector<int> perm(n);
    std::vector<double> Kout((size_t)n * n), buf((size_t)12 * (nz + nl + nv + 1), 0.0);
    double* outs[12];
    for (int k = 0; k < 12; k++) outs[k] = buf.data() + (size_t)k * (nz + nl + nv + 1);
    for (int adjoint = 0; adjoint < 2; adjoint++) {
      const int ok = hostsim_dense_stage_step(nz, nl, nv, data, z.data(), l.data(), v.data(), H.data(), zb.data(), lb.data(),
                                              vb.data(), 1e-4, 0.95, adjoint, perm.data(), Kout.data(), outs);
      if (!ok) { std::printf("step (%d, %d, %d) adjoint %d: false verdict\n", nz, nl, nv, adjoint); return 1; }
      for (double e : buf)
        if (!std::isfinite(e)) { std::printf("step (%d, %d, %d): not finite\n", nz, nl, nv); return 1; }
    }
    // the factors of the step as an image of their own: symmetric indefinite n x n
    std::vector<double> img((size_t)n * n, 0.0), rhs(n), x(n);
    for (int i = 0; i < n; i++)
      for (int j = 0; j <= i; j++) img[i + j * n] = img[j + i * n] = (i == j ? (i < nz ? n : -1.0) : 0.0) + lcg(s);
    for (auto& e : rhs) e = lcg(s);
    if (!hostsim_dense_stage_factor(n, nv, img.data(), rhs.data(), perm.data(), Kout.data(), x.data())) {
      std::printf("factor %d: false verdict\n", n);
      return 1;
    }
    for (double e : x)
      if (!std::isfinite(e)) { std::printf("factor %d: not finite\n", n); return 1; }
    std::printf("(%d, %d, %d) ok\n", nz, nl, nv);
  }
  return 0;
}
#endif
