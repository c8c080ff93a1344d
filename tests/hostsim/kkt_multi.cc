// TEST INFRASTRUCTURE ONLY - the many-right-hand-side solve of fbstab_amd/csrc/fb_kkt_multi.h (mpc_kkt_multi: what
// fbstab_mpc_kkt_multi_kernel runs per QP) compiled single-threaded for the host against tests/hostsim/shim, the
// same way adjoint.cc compiles the adjoint.  Built by tests/kkt_multi_helpers.py only; not part of
// libfbstab_hip.so.
#include <vector>

#include "../../fbstab_amd/csrc/fb_kkt_multi.h"

using namespace fbk;
typedef Ctx<1> C1;

// One QP at the point (z, l, v), nrhs right-hand sides.  x0_mode == 0: seeds gz, gl, gv, nrhs packed vectors each
// (gl, gv may be null: zero); otherwise the nrhs = nx unit directions of the initial state, the seeds not read.
// dz, dl, dv (each may be null: skipped) receive nrhs packed vectors, gain (may be null) nu x nx column-major.
// Returns the per-QP status of the kernel: 0, or 1 when a factorisation failed.
extern "C" int hostsim_mpc_kkt_multi(int N, int nx, int nu, int nc, const double* const* data, const double* z,
                                     const double* l, const double* v, int nrhs, int x0_mode, const double* gz,
                                     const double* gl, const double* gv, double sigma, double alpha, double* dz,
                                     double* dl, double* dv, double* gain) {
  MpcLayout lay;
  lay.init(N, nx, nu, nc, 1);
  std::vector<double> lds(lay.lds_doubles, 0.0), ws(lay.ws_doubles, 0.0);
  std::vector<double> uz(z, z + lay.nz), ul(l, l + lay.nl), uv(v, v + lay.nv);
  MpcData D = {data[0], data[1], data[2], data[3], data[4], data[5],
               data[6], data[7], data[8], data[9], data[10], data[11]};
  C1 ctx;
  ctx.tid = 0;
  ctx.red = nullptr;
  MpcProblem<C1> p;
  p.bind(lay, D, uz.data(), ul.data(), uv.data(), nullptr, lds.data(), ws.data());
  KktMultiSlots s;
  s.seed[0] = gz; s.seed[1] = gl; s.seed[2] = gv;
  s.step[0] = dz; s.step[1] = dl; s.step[2] = dv;
  const long long len[3] = {lay.nz, lay.nl, lay.nv};
  for (int i = 0; i < 3; i++) s.seed_rs[i] = s.step_rs[i] = len[i];
  s.gain = gain;
  return mpc_kkt_multi(p, ctx, sigma, alpha, nrhs, x0_mode != 0, s) ? 0 : 1;
}
