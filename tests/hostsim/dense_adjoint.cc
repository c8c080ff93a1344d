// TEST INFRASTRUCTURE ONLY - the dense adjoint of fbstab_amd/csrc/fb_dense.h (dense_adjoint,
// dense_adjoint_gradients; the contraction of fb_adjoint.h) compiled single-threaded for the host against
// tests/hostsim/shim, the same way adjoint.cc compiles the MPC one: the CPU suite checks the kernel's arithmetic
// against the oracle where no GPU exists.  Built by tests/test_dense_adjoint_hostsim.py only; not part of
// libfbstab_hip.so.
#define FB_DENSE_NO_MFMA 1  // (the K assembly on the matrix cores needs four wavefronts; the scalar loop is the same sum)
#include <cstring>
#include <vector>

#include "../../fbstab_amd/csrc/fb_dense.h"

using namespace fbk;
typedef Ctx<1> C1;

template <bool KG, bool VG>
static int run(const DenseLayout& lay, const DenseData& D, const double* z, const double* l, const double* v,
               const double* gz, const double* gl, const double* gv, double sigma, double alpha, double* adj,
               const DenseGrad& G) {
  std::vector<double> lds(lay.lds_doubles + 2, 0.0), ks(lay.k_doubles + lay.v_doubles + 2, 0.0);
  std::vector<double> uz(z, z + lay.nz), ul(l, l + lay.nl), uv(v, v + lay.nv);
  C1 ctx;
  ctx.tid = 0;
  ctx.red = lds.data() + lay.o_red;
  DenseProblem<C1, KG, VG> p;
  p.bind(lay, D, uz.data(), ul.data(), uv.data(), nullptr, lds.data(), ks.data());
  const bool ok = dense_adjoint(p, ctx, sigma, alpha, gz, gl, gv);
  dense_adjoint_gradients(p, ctx, G, ok, adj, adj + lay.nz, adj + lay.nz + lay.nl);
  return ok ? 0 : 1;
}

// One QP: the adjoint at the point (z, l, v) with seeds (gz, gl, gv) (gl, gv may be null: zero).
// adj receives (dz, dl, dv); grad[k] (k in the FBSTAB_DENSE_* order, may be null) the gradient of array k.
// Returns the per-QP status of the kernel: 0, or 1 when the factorisation failed.
extern "C" int hostsim_dense_adjoint(int nz, int nl, int nv, const double* const* data, const double* z,
                                     const double* l, const double* v, const double* gz, const double* gl,
                                     const double* gv, double sigma, double alpha, double* adj,
                                     double* const* grad) {
  DenseLayout lay;
  lay.init(nz, nl, nv, 1);
  DenseData D = {data[0], data[1], data[2], data[3], data[4], data[5]};
  DenseGrad G = {grad[0], grad[1], grad[2], grad[3], grad[4], grad[5]};
  if (lay.v_global) return run<true, true>(lay, D, z, l, v, gz, gl, gv, sigma, alpha, adj, G);
  if (lay.k_global) return run<true, false>(lay, D, z, l, v, gz, gl, gv, sigma, alpha, adj, G);
  return run<false, false>(lay, D, z, l, v, gz, gl, gv, sigma, alpha, adj, G);
}

// DenseLayout::init on the host (the GPU tests pick their shapes by the kernel they reach): out = {wave,
// k_global, v_global, a_lds, lds_doubles}.
extern "C" void hostsim_dense_layout(int nz, int nl, int nv, int nthreads, int* out) {
  DenseLayout lay;
  lay.init(nz, nl, nv, nthreads);
  out[0] = lay.wave; out[1] = lay.k_global; out[2] = lay.v_global; out[3] = lay.a_lds; out[4] = lay.lds_doubles;
}
