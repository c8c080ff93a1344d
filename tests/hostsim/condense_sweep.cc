// TEST INFRASTRUCTURE ONLY - the maps of fbstab_amd/csrc/fb_condense_sweep.h (condense_x0_map, condense_sweep_step,
// condense_sweep_begin: the kernels of fbstab_hip_mpc_condensed_x0_map_batch / fbstab_hip_mpc_condensed_receding_sweep)
// compiled single-threaded for the host against tests/hostsim/shim, the same way condense_multi.cc compiles the
// many-right-hand-side maps.  The loops of the kernels' grids run here, one "workgroup" after the other, each in a
// work array of its own filled with NaN.  Built by tests/condense_sweep_helpers.py only; not part of
// libfbstab_hip.so.
#include <cmath>
#include <vector>

#include "../../fbstab_amd/csrc/fb_condense_sweep.h"

using namespace fbk;
typedef Ctx<1> C1;

static MpcData data_of(const double* const* d) {
  return MpcData{d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7], d[8], d[9], d[10], d[11]};
}

// One QP: M = [F; G], ne x nx column-major, a block of at most nu columns per "workgroup".
extern "C" int hostsim_x0_map(int N, int nx, int nu, int nc, const double* const* data, double* M) {
  CondenseLds o;
  o.init(N, nx, nu, nc);
  for (int c0 = 0; c0 < nx; c0 += nu) {
    std::vector<double> w(o.total + 2, NAN);
    C1 ctx;
    ctx.tid = 0;
    ctx.red = nullptr;
    condense_x0_map(ctx, N, nx, nu, nc, c0, nx - c0 < nu ? nx - c0 : nu, data_of(data), o, w.data(), M);
  }
  return o.total;
}

// The rule and the layout: out = {T, total doubles, m_lds, ldm}.
extern "C" void hostsim_sweep_sizes(int N, int nx, int nu, int nc, int T, int stage_m, long long* out) {
  CondenseSweepLds L;
  L.init(N, nx, nu, nc, T, stage_m != 0);
  out[0] = L.T; out[1] = L.total; out[2] = L.m_lds; out[3] = L.ldm;
}

// One step of a batch in workgroups of T trajectories.
//   ip: N, nx, nu, nc, batch, retire, shift, affine, T, stage_m (a shared M goes through the staged copy)
//   sp: sx0, sAp, sBp, sM, sf0, sb0, sf, sb
//   dp: U, v, x0, xkeep, Ap, Bp, w, u_log, x_log, U_log, v_log, M, f0, b0, f, b    (null: as the kernel takes null)
//   eflag, newton: the dense records' fields, [batch]
extern "C" void hostsim_sweep_step(const int* ip, const long long* sp, double* const* dp, const int* eflag,
                                   const int* newton, int* gone, int* eflag_log, int* newton_log) {
  CondenseSweepStep a = {};
  a.N = ip[0]; a.nx = ip[1]; a.nu = ip[2]; a.nc = ip[3]; a.batch = ip[4];
  a.retire = ip[5]; a.shift = ip[6]; a.affine = ip[7];
  std::vector<fbstab_solver_out_t> out(a.batch);
  for (int q = 0; q < a.batch; q++) {
    out[q] = fbstab_solver_out_t{};
    out[q].eflag = eflag[q];
    out[q].newton_iters = newton[q];
  }
  a.out = out.data();
  a.gone = gone;
  a.U = dp[0]; a.v = dp[1]; a.x0 = dp[2]; a.xkeep = dp[3];
  a.Ap = dp[4]; a.Bp = dp[5]; a.w = dp[6];
  a.u_log = dp[7]; a.x_log = dp[8]; a.U_log = dp[9]; a.v_log = dp[10];
  a.M = dp[11]; a.f0 = dp[12]; a.b0 = dp[13]; a.f = dp[14]; a.b = dp[15];
  a.sx0 = sp[0]; a.sAp = sp[1]; a.sBp = sp[2]; a.sM = sp[3]; a.sf0 = sp[4]; a.sb0 = sp[5]; a.sf = sp[6]; a.sb = sp[7];
  a.eflag_log = eflag_log;
  a.newton_log = newton_log;
  CondenseSweepLds L;
  L.init(a.N, a.nx, a.nu, a.nc, ip[8], ip[9] != 0);
  for (long t0 = 0; t0 < a.batch; t0 += L.T) {
    std::vector<double> w(L.total + 2, NAN);
    C1 ctx;
    ctx.tid = 0;
    ctx.red = nullptr;
    condense_sweep_step(ctx, a, L, t0, a.batch - t0 < L.T ? (int)(a.batch - t0) : L.T, w.data());
  }
}

// One trajectory: the guess (U, v) from (z, v), and the gone flag.
extern "C" void hostsim_sweep_begin(int N, int nx, int nu, int nc, const double* z, const double* v, double* U,
                                    double* vc, int* gone) {
  C1 ctx;
  ctx.tid = 0;
  ctx.red = nullptr;
  condense_sweep_begin(ctx, N, nx, nu, nc, z, v, U, vc, gone);
}
