// TEST INFRASTRUCTURE ONLY - the dense many-right-hand-side solve of fbstab_amd/csrc/fb_dense_kkt_multi.h
// (dense_kkt_multi over DenseProblem: what fbstab_dense_kkt_multi_kernel runs per QP) compiled single-threaded for the
// host against tests/hostsim/shim, the same way dense_adjoint.cc compiles the adjoint.  Built by
// tests/dense_kkt_multi_helpers.py only; not part of libfbstab_hip.so.  With -DDENSE_KKT_MULTI_MAIN the file is a
// stand-alone program (one small QP per layout), which the CPU suite builds with the address and undefined-behaviour
// sanitizers and runs once.
#define FB_DENSE_NO_MFMA 1  // (the K assembly on the matrix cores needs four wavefronts; the scalar loop is the same sum)
#include <cstdio>
#include <vector>

#include "../../fbstab_amd/csrc/fb_dense_kkt_multi.h"

using namespace fbk;
typedef Ctx<1> C1;

template <bool KG, bool VG>
static int run(const DenseLayout& lay, const DenseData& D, const double* z, const double* l, const double* v, int nrhs,
               int wrt, const DenseKktSlots& s, double sigma, double alpha) {
  std::vector<double> lds(lay.lds_doubles + 2, 0.0), ks(lay.k_doubles + lay.v_doubles + 2, 0.0);
  std::vector<double> uz(z, z + lay.nz), ul(l, l + lay.nl), uv(v, v + lay.nv);
  C1 ctx;
  ctx.tid = 0;
  ctx.red = lds.data() + lay.o_red;
  DenseProblem<C1, KG, VG> p;
  p.bind(lay, D, uz.data(), ul.data(), uv.data(), nullptr, lds.data(), ks.data());
  return dense_kkt_multi(p, ctx, sigma, alpha, nrhs, wrt, s) ? 0 : 1;
}

// One QP at the point (z, l, v).  wrt < 0: nrhs seeds gz, gl, gv, packed vectors each (gl, gv may be null: zero);
// otherwise the Jacobian mode of array `wrt` (FBSTAB_DENSE_f, _h, _b), nrhs its length, the seeds not read.  dz, dl,
// dv (each may be null: skipped) receive nrhs packed vectors.  Returns the per-QP status of the kernel: 0, or 1 when
// the factorisation failed.
extern "C" int hostsim_dense_kkt_multi(int nz, int nl, int nv, const double* const* data, const double* z,
                                       const double* l, const double* v, int nrhs, int wrt, const double* gz,
                                       const double* gl, const double* gv, double sigma, double alpha, double* dz,
                                       double* dl, double* dv) {
  DenseLayout lay;
  lay.init(nz, nl, nv, 1);
  DenseData D = {data[0], data[1], data[2], data[3], data[4], data[5]};
  DenseKktSlots s;
  s.seed[0] = gz; s.seed[1] = gl; s.seed[2] = gv;
  s.step[0] = dz; s.step[1] = dl; s.step[2] = dv;
  const long long len[3] = {nz, nl, nv};
  for (int i = 0; i < 3; i++) s.seed_rs[i] = s.step_rs[i] = len[i];
  if (wrt < 0) wrt = kDenseKktSeeded;
  if (lay.v_global) return run<true, true>(lay, D, z, l, v, nrhs, wrt, s, sigma, alpha);
  if (lay.k_global) return run<true, false>(lay, D, z, l, v, nrhs, wrt, s, sigma, alpha);
  return run<false, false>(lay, D, z, l, v, nrhs, wrt, s, sigma, alpha);
}

#if defined(DENSE_KKT_MULTI_MAIN)
// One small QP per layout of DenseLayout::init - K in LDS, K in global scratch, the iterate vectors there too - with
// H = 2 I, a few equalities and bounds z_i <= 1, at the origin: three seeded right-hand sides and the three Jacobian
// modes, every output buffer exactly as long as the call may write.
static int one(int nz, int nl, int nv, int kg, int vg) {
  DenseLayout lay;
  lay.init(nz, nl, nv, 1);
  if (lay.k_global != kg || lay.v_global != vg) {
    std::printf("layout of (%d, %d, %d): k_global %d v_global %d\n", nz, nl, nv, lay.k_global, lay.v_global);
    return 1;
  }
  std::vector<double> H((size_t)nz * nz, 0.0), f(nz, 1.0), G((size_t)nl * nz + 1, 0.0), h(nl + 1, 0.5),
      A((size_t)nv * nz, 0.0), b(nv, 1.0);
  for (int i = 0; i < nz; i++) H[i + (size_t)i * nz] = 2.0;
  for (int i = 0; i < nl; i++) G[i + (size_t)i * nl] = 1.0;
  for (int i = 0; i < nv; i++) A[i + (size_t)(i % nz) * nv] = 1.0;
  const double* data[6] = {H.data(), f.data(), G.data(), h.data(), A.data(), b.data()};
  std::vector<double> z(nz, 0.0), l(nl + 1, 0.0), v(nv, 0.0);
  int bad = 0;
  const int nrhs = 3;
  std::vector<double> gz((size_t)nrhs * nz, 1.0), gl((size_t)nrhs * nl + 1, -1.0), gv((size_t)nrhs * nv, 0.5);
  std::vector<double> dz((size_t)nrhs * nz), dl((size_t)nrhs * nl), dv((size_t)nrhs * nv);
  bad += hostsim_dense_kkt_multi(nz, nl, nv, data, z.data(), l.data(), v.data(), nrhs, -1, gz.data(), gl.data(),
                                 gv.data(), 1e-8, 0.95, dz.data(), dl.data(), dv.data());
  bad += hostsim_dense_kkt_multi(nz, nl, nv, data, z.data(), l.data(), v.data(), 1, -1, gz.data(), nullptr, nullptr,
                                 1e-8, 0.95, dz.data(), nullptr, nullptr);
  const int wrts[3] = {FBSTAB_DENSE_f, FBSTAB_DENSE_h, FBSTAB_DENSE_b}, lens[3] = {nz, nl, nv};
  for (int m = 0; m < 3; m++) {
    const int k = lens[m];
    if (k == 0) continue;
    std::vector<double> jz((size_t)k * nz), jl((size_t)k * nl), jv((size_t)k * nv);
    bad += hostsim_dense_kkt_multi(nz, nl, nv, data, z.data(), l.data(), v.data(), k, wrts[m], nullptr, nullptr,
                                   nullptr, 1e-8, 0.95, jz.data(), jl.data(), jv.data());
    if (!(jz[0] == jz[0])) bad++;
  }
  return bad;
}

int main() {
  int bad = one(6, 2, 9, 0, 0);
  bad += one(5, 0, 7, 0, 0);
  bad += one(150, 3, 20, 1, 0);
  bad += one(4, 1, 2560, 1, 1);
  std::printf("dense_kkt_multi: %s\n", bad ? "FAILED" : "ok");
  return bad ? 1 : 0;
}
#endif
