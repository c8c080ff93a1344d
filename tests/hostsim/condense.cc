// TEST INFRASTRUCTURE ONLY - the condensing arithmetic of fbstab_amd/csrc/fb_condense.h (condense_matrices,
// condense_vectors, condense_expand: the kernels of fbstab_hip_mpc_condense_batch and fbstab_hip_mpc_expand_batch)
// compiled single-threaded for the host against tests/hostsim/shim, the same way tangent.cc compiles the tangent
// right-hand side: the CPU suite checks the kernels' arithmetic where no GPU exists.  Built by
// tests/condense_helpers.py only; not part of libfbstab_hip.so.
#include <vector>

#include "../../fbstab_amd/csrc/fb_condense.h"

using namespace fbk;
typedef Ctx<1> C1;

static MpcData data_of(const double* const* d) {
  return MpcData{d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7], d[8], d[9], d[10], d[11]};
}

// One QP: data[k] in the FBSTAB_MPC_* order; what: bit 0 - H and A, bit 1 - f and b (the others are not touched).
// Returns the doubles of "LDS" the layout takes.
extern "C" int hostsim_condense(int N, int nx, int nu, int nc, const double* const* data, int what, double* H,
                                double* f, double* A, double* b) {
  CondenseLds o;
  o.init(N, nx, nu, nc);
  std::vector<double> w(o.total + 2, 0.0);
  const MpcData D = data_of(data);
  C1 ctx;
  ctx.tid = 0;
  ctx.red = nullptr;
  if (what & 1)
    for (int k = 0; k <= N; k++) condense_matrices(ctx, N, nx, nu, nc, k, D, o, w.data(), H, A);
  if (what & 2) condense_vectors(ctx, N, nx, nu, nc, D, o, w.data(), f, b);
  return o.total;
}

// One QP: (z, l, v, y) from (U, vc, yc); null outputs are skipped.
extern "C" int hostsim_expand(int N, int nx, int nu, int nc, const double* const* data, const double* U,
                              const double* vc, const double* yc, double* z, double* l, double* v, double* y) {
  CondenseLds o;
  o.init(N, nx, nu, nc);
  std::vector<double> w(o.total + 2, 0.0);
  C1 ctx;
  ctx.tid = 0;
  ctx.red = nullptr;
  condense_expand(ctx, N, nx, nu, nc, data_of(data), U, vc, yc, o, w.data(), z, l, v, y);
  return o.total;
}
