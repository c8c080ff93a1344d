// TEST INFRASTRUCTURE ONLY - the flat-vector adjoint of fbstab_amd/csrc/fb_mpc.h (mpc_adjoint,
// mpc_adjoint_gradients) compiled single-threaded for the host against tests/hostsim/shim, the same way
// hostsim.cc compiles the solver: the CPU suite checks the kernel's arithmetic against the oracle where no GPU
// exists.  Built by tests/test_adjoint_hostsim.py only; not part of libfbstab_hip.so.
#include <cstring>
#include <vector>

#include "../../fbstab_amd/csrc/fb_mpc.h"

using namespace fbk;
typedef Ctx<1> C1;

// One QP: the adjoint at the point (z, l, v) with seeds (gz, gl, gv) (gl, gv may be null: zero).
// adj receives (dz, dl, dv); grad[k] (k in the FBSTAB_MPC_* order, may be null) the gradient of sequence k.
// Returns the per-QP status of the kernel: 0, or 1 when a factorisation failed.
extern "C" int hostsim_mpc_adjoint(int N, int nx, int nu, int nc, const double* const* data, const double* z,
                                   const double* l, const double* v, const double* gz, const double* gl,
                                   const double* gv, double sigma, double alpha, double* adj, double* const* grad) {
  MpcLayout lay;
  lay.init(N, nx, nu, nc, 1);
  std::vector<double> lds(lay.lds_doubles, 0.0), ws(lay.ws_doubles, 0.0);
  std::vector<double> uz(z, z + lay.nz), ul(l, l + lay.nl), uv(v, v + lay.nv);
  MpcData D = {data[0], data[1], data[2], data[3], data[4], data[5],
               data[6], data[7], data[8], data[9], data[10], data[11]};
  MpcGrad G = {grad[0], grad[1], grad[2], grad[3], grad[4], grad[5],
               grad[6], grad[7], grad[8], grad[9], grad[10], grad[11]};
  C1 ctx;
  ctx.tid = 0;
  ctx.red = nullptr;
  MpcProblem<C1> p;
  p.bind(lay, D, uz.data(), ul.data(), uv.data(), nullptr, lds.data(), ws.data());
  const bool ok = mpc_adjoint(p, ctx, sigma, alpha, gz, gl, gv);
  mpc_adjoint_gradients(p, ctx, G, ok, adj, adj + lay.nz, adj + lay.nz + lay.nl);
  return ok ? 0 : 1;
}
