// TEST INFRASTRUCTURE ONLY - the map of fbstab_amd/csrc/fb_condense_sweep_tangent.h (condense_sweep_tangent_step: the
// kernel of fbstab_hip_mpc_condensed_receding_sweep_tangent), compiled single-threaded for the host against
// tests/hostsim/shim, the same way condense_sweep_adjoint.cc compiles the backward map.  The loop of the kernel's grid
// runs here, one "workgroup" after the other, each in a work array of its own filled with NaN.  Built by
// tests/condense_sweep_tangent_helpers.py only; not part of libfbstab_hip.so.
#include <cmath>
#include <vector>

#include "../../fbstab_amd/csrc/fb_condense_sweep_tangent.h"

using namespace fbk;
typedef Ctx<1> C1;

// One launch of the step kernel on a batch in workgroups of T trajectories.
//   ip: N, nx, nu, nc, batch, close, open, T, stage_m
//   sp: sdx0, sAp, sBp, sM, sf0, sb0, sf, sb, sdf0, sdb0
//   dp: dU, dx, dx0, Ap, Bp, dw, du_out, dx_out, x_log, M, f0, b0, f, b, df0, db0, gU, gv   (null: as the kernel takes it)
//   np: eflag_close, eflag_open, st1, st2, status
extern "C" void hostsim_sweep_tangent_step(const int* ip, const long long* sp, double* const* dp, int* const* np) {
  CondenseSweepTanStep a = {};
  a.N = ip[0]; a.nx = ip[1]; a.nu = ip[2]; a.nc = ip[3]; a.batch = ip[4];
  a.close = ip[5]; a.open = ip[6];
  a.sdx0 = sp[0]; a.sAp = sp[1]; a.sBp = sp[2]; a.sM = sp[3]; a.sf0 = sp[4]; a.sb0 = sp[5]; a.sf = sp[6]; a.sb = sp[7];
  a.sdf0 = sp[8]; a.sdb0 = sp[9];
  a.dU = dp[0]; a.dx = dp[1]; a.dx0 = dp[2]; a.Ap = dp[3]; a.Bp = dp[4]; a.dw = dp[5]; a.du_out = dp[6];
  a.dx_out = dp[7]; a.x_log = dp[8]; a.M = dp[9]; a.f0 = dp[10]; a.b0 = dp[11]; a.f = dp[12]; a.b = dp[13];
  a.df0 = dp[14]; a.db0 = dp[15]; a.gU = dp[16]; a.gv = dp[17];
  a.eflag_close = np[0]; a.eflag_open = np[1]; a.st1 = np[2]; a.st2 = np[3]; a.status = np[4];
  CondenseSweepLds L;
  L.init(a.N, a.nx, a.nu, a.nc, ip[7], ip[8] != 0);
  for (long t0 = 0; t0 < a.batch; t0 += L.T) {
    std::vector<double> w(L.total + 2, NAN);
    C1 ctx;
    ctx.tid = 0;
    ctx.red = nullptr;
    condense_sweep_tangent_step(ctx, a, L, t0, a.batch - t0 < L.T ? (int)(a.batch - t0) : L.T, w.data());
  }
}
