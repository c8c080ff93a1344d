// TEST INFRASTRUCTURE ONLY - the maps of fbstab_amd/csrc/fb_condense_sweep_adjoint.h (condense_sweep_adjoint_step,
// condense_sweep_adjoint_finish, condense_sweep_adjoint_begin: the kernels of
// fbstab_hip_mpc_condensed_receding_sweep_adjoint) and both instantiations of condense_adjoint_finish, compiled
// single-threaded for the host against tests/hostsim/shim, the same way condense_sweep.cc compiles the forward maps.
// The loops of the kernels' grids run here, one "workgroup" after the other, each in a work array of its own filled
// with NaN.  Built by tests/condense_sweep_adjoint_helpers.py only; not part of libfbstab_hip.so.
#include <cmath>
#include <vector>

#include "../../fbstab_amd/csrc/fb_condense_sweep_adjoint.h"

using namespace fbk;
typedef Ctx<1> C1;

static MpcData data_of(const double* const* d) {
  return MpcData{d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7], d[8], d[9], d[10], d[11]};
}
static MpcGrad grad_of(double* const* g) {
  return MpcGrad{g[0], g[1], g[2], g[3], g[4], g[5], g[6], g[7], g[8], g[9], g[10], g[11]};
}

// One launch of the step kernel on a batch in workgroups of T trajectories.
//   ip: N, nx, nu, nc, batch, close, open, affine, T, stage_m
//   sp: sAp, sBp, sM, sf0, sb0, sf, sb, sgx0
//   dp: dU, dv, dl0, mu, Ap, Bp, gu, gx, mu_log, gU, x_log, M, f0, b0, f, b, gf0, gb0, gx0   (null: as the kernel takes it)
//   np: eflag_close, eflag_open, st1, st2, status
extern "C" void hostsim_sweep_adjoint_step(const int* ip, const long long* sp, double* const* dp, int* const* np) {
  CondenseSweepAdjStep a = {};
  a.N = ip[0]; a.nx = ip[1]; a.nu = ip[2]; a.nc = ip[3]; a.batch = ip[4];
  a.close = ip[5]; a.open = ip[6]; a.affine = ip[7];
  a.sAp = sp[0]; a.sBp = sp[1]; a.sM = sp[2]; a.sf0 = sp[3]; a.sb0 = sp[4]; a.sf = sp[5]; a.sb = sp[6]; a.sgx0 = sp[7];
  a.dU = dp[0]; a.dv = dp[1]; a.dl0 = dp[2]; a.mu = dp[3]; a.Ap = dp[4]; a.Bp = dp[5]; a.gu = dp[6]; a.gx = dp[7];
  a.mu_log = dp[8]; a.gU = dp[9]; a.x_log = dp[10]; a.M = dp[11]; a.f0 = dp[12]; a.b0 = dp[13]; a.f = dp[14];
  a.b = dp[15]; a.gf0 = dp[16]; a.gb0 = dp[17]; a.gx0 = dp[18];
  a.eflag_close = np[0]; a.eflag_open = np[1]; a.st1 = np[2]; a.st2 = np[3]; a.status = np[4];
  CondenseSweepLds L;
  L.init(a.N, a.nx, a.nu, a.nc, ip[8], ip[9] != 0);
  for (long t0 = 0; t0 < a.batch; t0 += L.T) {
    std::vector<double> w(L.total + 2, NAN);
    C1 ctx;
    ctx.tid = 0;
    ctx.red = nullptr;
    condense_sweep_adjoint_step(ctx, a, L, t0, a.batch - t0 < L.T ? (int)(a.batch - t0) : L.T, w.data());
  }
}

// condense_adjoint_finish of one QP, storing (acc = 0) or accumulating (acc != 0); the arguments of
// hostsim_condense_adjoint_finish (condense_adjoint.cc).
extern "C" int hostsim_sweep_adjoint_plain_finish(int acc, int N, int nx, int nu, int nc, const double* const* data,
                                                  const double* z, const double* l, const double* v, const double* gz,
                                                  const double* gl, const double* dU, const double* dv,
                                                  double* const* grad, int ok, double* az, double* al, double* av) {
  CondenseLds o;
  o.init(N, nx, nu, nc);
  std::vector<double> w(o.total + 2, NAN);
  C1 ctx;
  ctx.tid = 0;
  ctx.red = nullptr;
  const MpcGrad G = grad_of(grad);
  if (acc)
    condense_adjoint_finish<true>(ctx, N, nx, nu, nc, data_of(data), z, l, v, gz, gl, dU, dv, o, w.data(), G, ok != 0, az,
                                  al, av);
  else
    condense_adjoint_finish(ctx, N, nx, nu, nc, data_of(data), z, l, v, gz, gl, dU, dv, o, w.data(), G, ok != 0, az, al,
                            av);
  return o.total;
}

// The finish kernel's work on one trajectory: data with x0 := the step's state; z, l: scratch of nz, nl doubles;
// gz: nz zeros.  grad: the slots that are added to (the x0 slot: null, or the zeroed -dl0).
extern "C" void hostsim_sweep_adjoint_finish(int N, int nx, int nu, int nc, const double* const* data, const double* U,
                                             const double* v, const double* dU, const double* dv, const double* gz,
                                             double* const* grad, int ok, double* z, double* l) {
  CondenseLds o;
  o.init(N, nx, nu, nc);
  std::vector<double> w(o.total + 2, NAN);
  C1 ctx;
  ctx.tid = 0;
  ctx.red = nullptr;
  condense_sweep_adjoint_finish(ctx, N, nx, nu, nc, data_of(data), U, v, dU, dv, gz, o, w.data(), grad_of(grad), ok != 0,
                                z, l);
}

// One trajectory: the zeros before the first step.
extern "C" void hostsim_sweep_adjoint_begin(int N, int nx, int nu, int nc, double* const* grad, double* gz, double* gf0,
                                            double* gb0, int* status) {
  C1 ctx;
  ctx.tid = 0;
  ctx.red = nullptr;
  condense_sweep_adjoint_begin(ctx, N, nx, nu, nc, grad_of(grad), gz, gf0, gb0, status);
}
