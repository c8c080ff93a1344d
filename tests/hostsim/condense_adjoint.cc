// TEST INFRASTRUCTURE ONLY - the two maps of fbstab_amd/csrc/fb_condense_adjoint.h (condense_adjoint_seed,
// condense_adjoint_finish: the kernels of fbstab_hip_mpc_condensed_adjoint_batch) compiled single-threaded for the host
// against tests/hostsim/shim, the same way condense.cc compiles the condensing maps.  Built by
// tests/condense_adjoint_helpers.py only; not part of libfbstab_hip.so.
#include <vector>

#include "../../fbstab_amd/csrc/fb_condense_adjoint.h"

using namespace fbk;
typedef Ctx<1> C1;

static MpcData data_of(const double* const* d) {
  return MpcData{d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7], d[8], d[9], d[10], d[11]};
}

// One QP: data[k] in the FBSTAB_MPC_* order; gl, gv may be null.  Returns the doubles of "LDS" the layout takes.
extern "C" int hostsim_condense_adjoint_seed(int N, int nx, int nu, int nc, const double* const* data, const double* z,
                                             const double* gz, const double* gl, const double* gv, double* U,
                                             double* gU, double* gvc) {
  CondenseLds o;
  o.init(N, nx, nu, nc);
  std::vector<double> w(o.total + 2, 0.0);
  C1 ctx;
  ctx.tid = 0;
  ctx.red = nullptr;
  condense_adjoint_seed(ctx, N, nx, nu, nc, data_of(data), z, gz, gl, gv, o, w.data(), U, gU, gvc);
  return o.total;
}

// One QP: the gradients grad[k] (FBSTAB_MPC_* order, null: not wanted) and adj = (dz, dl, dv) (null slots skipped)
// from the dense adjoint's (dU, dv); ok = 0: a failed factorisation.
extern "C" int hostsim_condense_adjoint_finish(int N, int nx, int nu, int nc, const double* const* data,
                                               const double* z, const double* l, const double* v, const double* gz,
                                               const double* gl, const double* dU, const double* dv,
                                               double* const* grad, int ok, double* az, double* al, double* av) {
  CondenseLds o;
  o.init(N, nx, nu, nc);
  std::vector<double> w(o.total + 2, 0.0);
  C1 ctx;
  ctx.tid = 0;
  ctx.red = nullptr;
  const MpcGrad G{grad[0], grad[1], grad[2], grad[3], grad[4], grad[5], grad[6], grad[7], grad[8], grad[9], grad[10],
                  grad[11]};
  condense_adjoint_finish(ctx, N, nx, nu, nc, data_of(data), z, l, v, gz, gl, dU, dv, o, w.data(), G, ok != 0, az, al,
                          av);
  return o.total;
}

// One QP: rU = gU - (H_c dU + sigma dU + A_c' dv), H_c (nzc x nzc) and A_c (nv x nzc) column-major.
extern "C" void hostsim_condense_adjoint_residual(int nzc, int nv, const double* H, const double* A, double sigma,
                                                  const double* gU, const double* dU, const double* dv, double* rU) {
  C1 ctx;
  ctx.tid = 0;
  ctx.red = nullptr;
  condense_adjoint_residual(ctx, nzc, nv, H, A, sigma, gU, dU, dv, rU);
}

// One QP: (dU, dv) += (eU, ev).
extern "C" void hostsim_condense_adjoint_correct(int nzc, int nv, const double* eU, const double* ev, double* dU,
                                                 double* dv) {
  C1 ctx;
  ctx.tid = 0;
  ctx.red = nullptr;
  condense_adjoint_correct(ctx, nzc, nv, eU, ev, dU, dv);
}
