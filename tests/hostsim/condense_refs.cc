// TEST INFRASTRUCTURE ONLY - condense_reference_vectors of fbstab_amd/csrc/fb_condense_refs.h (the kernel of
// fbstab_hip_mpc_condensed_reference_images_batch) compiled single-threaded for the host against tests/hostsim/shim,
// the way condense.cc compiles condense_vectors: the CPU suite compares the two bit for bit.  The groups of R steps are
// walked as the kernel's grid walks them.  Built by tests/condense_tracking_helpers.py only; not part of
// libfbstab_hip.so.
#include <cmath>
#include <vector>

#include "../../fbstab_amd/csrc/fb_condense_refs.h"

using namespace fbk;
typedef Ctx<1> C1;

// One trajectory: data[k] in the FBSTAB_MPC_* order (q, r, c, d and x0 are not read: they may be null); ref[i], step[i]
// (i = 0 .. 3: q, r, c, d): the sequence of step 0 and the doubles between steps.  f0 of step k at f0 + k sf0, b0
// likewise.  Returns the doubles of "LDS" a workgroup takes, or -1 where the words behind them were written.
extern "C" long long hostsim_condense_refs(int N, int nx, int nu, int nc, const double* const* data,
                                           const double* const* ref, const long long* step, int steps, int R,
                                           double* f0, long long sf0, double* b0, long long sb0) {
  CondenseLds o;
  o.init(N, nx, nu, nc);
  const long long per = condense_refs_per(N, nx);
  const long long total = (long long)o.carry + R * per;
  std::vector<double> w(total + 2, 0.0);
  w[total] = w[total + 1] = -7.25;
  MpcData D = MpcData{data[0], data[1], data[2], nullptr, nullptr, data[5], data[6], nullptr, data[8], data[9],
                      nullptr, nullptr};
  C1 ctx;
  ctx.tid = 0;
  ctx.red = nullptr;
  const int groups = (steps + R - 1) / R;
  for (int g = 0; g < groups; g++) {
    const int k0 = g * R;
    const int Rg = steps - k0 < R ? steps - k0 : R;
    CondenseRefSeqs rs;
    rs.sq = step[0]; rs.sr = step[1]; rs.sc = step[2]; rs.sd = step[3];
    rs.q = ref[0] + k0 * rs.sq; rs.r = ref[1] + k0 * rs.sr; rs.c = ref[2] + k0 * rs.sc; rs.d = ref[3] + k0 * rs.sd;
    for (double& e : w) e = std::nan("");  // (a group starts from LDS it never wrote)
    w[total] = w[total + 1] = -7.25;
    condense_reference_vectors(ctx, N, nx, nu, nc, D, rs, Rg, (long)per, o, w.data(), f0 + k0 * sf0, sf0,
                               b0 + k0 * sb0, sb0);
    if (w[total] != -7.25 || w[total + 1] != -7.25) return -1;
  }
  return total;
}
