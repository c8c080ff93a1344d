// TEST INFRASTRUCTURE ONLY - the maps of fbstab_amd/csrc/fb_condense_multi.h (condense_multi_seed,
// condense_multi_residual, condense_multi_correct, condense_multi_finish: the kernels of
// fbstab_hip_mpc_condensed_kkt_solve_batch / _x0_sensitivity_batch) compiled single-threaded for the host against
// tests/hostsim/shim, the same way condense_adjoint.cc compiles the adjoint's maps.  The group loop of the kernels'
// grid runs here, one "workgroup" after the other, each in a work array of its own filled with NaN.  Built by
// tests/condense_multi_helpers.py only; not part of libfbstab_hip.so.
#include <cmath>
#include <vector>

#include "../../fbstab_amd/csrc/fb_condense_multi.h"

using namespace fbk;
typedef Ctx<1> C1;

static MpcData data_of(const double* const* d) {
  return MpcData{d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7], d[8], d[9], d[10], d[11]};
}

// per, the window and the rule of the library (out: per, window doubles, R of the rule).
extern "C" void hostsim_condense_multi_sizes(int N, int nx, int nu, int nc, int nrhs, long long* out) {
  CondenseLds o;
  o.init(N, nx, nu, nc);
  out[0] = condense_multi_per(N, nx, nu, nc);
  out[1] = o.carry;
  out[2] = condense_multi_rule(nx, nrhs, o.carry, out[0]);
}

// One QP, nrhs right-hand sides in groups of R: seeds[i] (gz, gl, gv; gl, gv may be null) with right-hand side k at
// + k rs[i], or generated (x0_mode).  groups < 0: all of them; otherwise only the first `groups` run (the seeded
// defect "the partial last group is not written").  gU, gvc: [nrhs][n] packed.
extern "C" int hostsim_condense_multi_seed(int N, int nx, int nu, int nc, const double* const* data, const double* z,
                                           int x0_mode, const double* const* seeds, const long long* rs, int nrhs,
                                           int R, int groups, double* U, double* gU, double* gvc) {
  CondenseLds o;
  o.init(N, nx, nu, nc);
  const long per = (long)condense_multi_per(N, nx, nu, nc);
  const CondenseMultiSeeds sd{seeds[0], seeds[1], seeds[2], rs[0], rs[1], rs[2], x0_mode};
  const int all = (nrhs + R - 1) / R;
  for (int g = 0; g < (groups < 0 ? all : groups); g++) {
    std::vector<double> w(o.carry + (size_t)R * per + 2, NAN);
    C1 ctx;
    ctx.tid = 0;
    ctx.red = nullptr;
    const int k0 = g * R, Rg = nrhs - k0 < R ? nrhs - k0 : R;
    condense_multi_seed(ctx, N, nx, nu, nc, data_of(data), z, sd, k0, Rg, per, o, w.data(), k0 == 0 ? U : nullptr, gU,
                        gvc);
  }
  return (int)(o.carry + R * per);
}

// One QP: (dz, dl, dv) of nrhs right-hand sides (step[i] at + k srs[i], null slots skipped) from dU, dvc ([nrhs][n]
// packed); the seeds as above (only gz and gl are read).
extern "C" int hostsim_condense_multi_finish(int N, int nx, int nu, int nc, const double* const* data, int x0_mode,
                                             const double* const* seeds, const long long* rs, int nrhs, int R,
                                             int groups, const double* dU, const double* dvc, int ok,
                                             double* const* step, const long long* srs) {
  CondenseLds o;
  o.init(N, nx, nu, nc);
  const long per = (long)condense_multi_per(N, nx, nu, nc);
  const CondenseMultiSeeds sd{seeds[0], seeds[1], seeds[2], rs[0], rs[1], rs[2], x0_mode};
  const int all = (nrhs + R - 1) / R;
  for (int g = 0; g < (groups < 0 ? all : groups); g++) {
    std::vector<double> w(o.carry + (size_t)R * per + 2, NAN);
    C1 ctx;
    ctx.tid = 0;
    ctx.red = nullptr;
    const int k0 = g * R, Rg = nrhs - k0 < R ? nrhs - k0 : R;
    condense_multi_finish(ctx, N, nx, nu, nc, data_of(data), sd, k0, Rg, per, dU, dvc, o, w.data(), ok != 0, step[0],
                          srs[0], step[1], srs[1], step[2], srs[2]);
  }
  return (int)(o.carry + R * per);
}

// One QP, nrhs right-hand sides in groups of R: rU = gU - (H_c dU + sigma dU + A_c' dv), all [nrhs][n] packed.
extern "C" void hostsim_condense_multi_residual(int nzc, int nv, int nrhs, int R, const double* H, const double* A,
                                                double sigma, const double* gU, const double* dU, const double* dv,
                                                double* rU) {
  C1 ctx;
  ctx.tid = 0;
  ctx.red = nullptr;
  for (int k0 = 0; k0 < nrhs; k0 += R) {
    const int Rg = nrhs - k0 < R ? nrhs - k0 : R;
    const long u = (long)k0 * nzc, v = (long)k0 * nv;
    condense_multi_residual(ctx, nzc, nv, Rg, H, A, sigma, gU + u, dU + u, dv + v, rU + u);
  }
}

// One QP: (dU, dv) += (eU, ev), and gain (null, or nu x nrhs column-major) = the first nu rows of the corrected dU.
extern "C" void hostsim_condense_multi_correct(int nzc, int nv, int nu, int nrhs, int R, const double* eU,
                                               const double* ev, double* dU, double* dv, double* gain, int ok) {
  C1 ctx;
  ctx.tid = 0;
  ctx.red = nullptr;
  for (int k0 = 0; k0 < nrhs; k0 += R) {
    const int Rg = nrhs - k0 < R ? nrhs - k0 : R;
    const long u = (long)k0 * nzc, v = (long)k0 * nv;
    condense_multi_correct(ctx, nzc, nv, nu, k0, Rg, eU + u, ev + v, dU + u, dv + v, gain, ok != 0);
  }
}
