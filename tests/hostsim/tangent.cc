// TEST INFRASTRUCTURE ONLY - the direction arithmetic of fbstab_amd/csrc/fb_tangent.h (mpc_tangent_stage,
// dense_tangent: the right-hand side of fbstab_hip_*_tangent_batch) compiled single-threaded for the host against
// tests/hostsim/shim, the same way adjoint.cc compiles the adjoint: the CPU suite checks the kernel's arithmetic
// where no GPU exists.  Built by tests/tangent_helpers.py only; not part of libfbstab_hip.so.
#include <vector>

#include "../../fbstab_amd/csrc/fb_tangent.h"

using namespace fbk;
typedef Ctx<1> C1;

// One QP: (gz, gl, gv) from the perturbations dir[k] (k in the FBSTAB_MPC_* order; null: zero) and the point.
extern "C" int hostsim_mpc_tangent_rhs(int N, int nx, int nu, int nc, const double* const* dir, const double* z,
                                       const double* l, const double* v, double* gz, double* gl, double* gv) {
  MpcTangentLds o;
  o.init(nx, nu, nc);
  std::vector<double> w(o.total + 2, 0.0);
  MpcDir D = {dir[0], dir[1], dir[2], dir[3], dir[4], dir[5], dir[6], dir[7], dir[8], dir[9], dir[10], dir[11]};
  C1 ctx;
  ctx.tid = 0;
  ctx.red = nullptr;
  for (int i = 0; i <= N; i++) mpc_tangent_stage(ctx, N, nx, nu, nc, i, D, z, l, v, o, w.data(), gz, gl, gv);
  return 0;
}

// The same for the dense QP (dir in the FBSTAB_DENSE_* order), with `budget` doubles of "LDS": it decides how many
// columns a block holds (DenseTangentLds::cb, returned; 0: not one column fits).
extern "C" int hostsim_dense_tangent_rhs(int nz, int nl, int nv, int budget, const double* const* dir, const double* z,
                                         const double* l, const double* v, double* gz, double* gl, double* gv) {
  DenseTangentLds o;
  if (!o.init(nz, nl, nv, budget)) return 0;
  std::vector<double> w(o.total + 2, 0.0);
  DenseDir D = {dir[0], dir[1], dir[2], dir[3], dir[4], dir[5]};
  C1 ctx;
  ctx.tid = 0;
  ctx.red = nullptr;
  dense_tangent(ctx, nz, nl, nv, D, z, l, v, o, w.data(), gz, gl, gv);
  return o.cb;
}
