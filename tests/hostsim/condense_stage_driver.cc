// TEST INFRASTRUCTURE ONLY - the driver of tests/test_condense_stage.py: fbstab_amd/csrc/fb_condense_stage.h over the
// heap-backed runtime of runtime_shim/, a bare SolverBase with the lengths fbstab_hip_dense_create sets, and host
// lambdas in the place of the kernels and of the dense handle's entry points.  Every buffer of a caller is allocated
// exactly as long as include/fbstab_hip.h and the *_sizes functions say; a lambda decodes its arguments by kernel id
// and reads every input double and writes every output double it is entitled to, through the bases and strides it was
// given - so that under the address sanitizer a stride, a carve or a log share that is off by one double ends the
// driver.  The expected blocks, sequences and refusal texts are restated here from include/fbstab_hip.h and from the
// entry points as they stood before the stage was moved out of fbstab_hip.hip, not taken from the header under test.
// Not shown: asynchrony and copy direction (runtime_shim), and "no HIP device" (the shim always has one).
//
// usage: condense_stage_driver <group>; prints one line per failed check and exits 1, prints nothing and exits 0
// otherwise.
#include "fb_condense_stage.h"

#include <cstdint>
#include <cstdio>
#include <functional>
#include <memory>

namespace {

int g_failures = 0;
#define CHECK(cond, ...)                                            \
  do {                                                              \
    if (!(cond)) {                                                  \
      if (g_failures++ < 40) {                                      \
        std::printf("FAIL %s:%d: %s: ", __func__, __LINE__, #cond); \
        std::printf(__VA_ARGS__);                                   \
        std::printf("\n");                                          \
      }                                                             \
    }                                                               \
  } while (0)

// ---- memory: exact allocations, and lambdas that touch all of what they are given ----------------------------------
std::vector<std::unique_ptr<double[]>> g_doubles;
std::vector<std::unique_ptr<int[]>> g_ints;
double* D(long long n) {
  g_doubles.emplace_back(new double[(size_t)n]);
  for (long long i = 0; i < n; i++) g_doubles.back()[i] = 1.0;
  return g_doubles.back().get();
}
int* I(long long n) {
  g_ints.emplace_back(new int[(size_t)n]());
  return g_ints.back().get();
}
volatile double g_sink = 0.0;
void rd(const double* p, long long n) { for (long long i = 0; i < n; i++) g_sink = g_sink + p[i]; }
void wr(double* p, long long n) { for (long long i = 0; i < n; i++) p[i] = 2.0; }
void rdi(const int* p, long long n) { for (long long i = 0; i < n; i++) g_sink = g_sink + p[i]; }
void wri(int* p, long long n) { for (long long i = 0; i < n; i++) p[i] = 0; }
// rows of a block: QP q at base + q * stride; stride 0: one row for all
void rd_rows(const double* b, long long stride, long long len, int batch) {
  if (b) for (int q = 0; q < (stride == 0 ? 1 : batch); q++) rd(b + q * stride, len);
}
void wr_rows(double* b, long long stride, long long len, int batch) {
  if (b) for (int q = 0; q < (stride == 0 ? 1 : batch); q++) wr(b + q * stride, len);
}

constexpr long long kGarbage = 0x7777777;  // a caller's stride where the header says it is not read
constexpr int kGap = 3;

// ---- what a run queued --------------------------------------------------------------------------------------------
enum Family { COND, ADJ, MULTI, SWEEP, SADJ, DENSE };
enum DenseCall { D_SOLVE, D_ADJOINT, D_MULTI };
struct Ev {
  int fam, id, grid;
  long long lds;
  bool operator==(const Ev& o) const { return fam == o.fam && id == o.id && grid == o.grid && lds == o.lds; }
};

template <class T>
T& arg(void** args, int i) { return *static_cast<T*>(args[i]); }

// The kernels' and the dense handle's stand-ins for one call, and what they saw.
struct Sim {
  int N = 0, nx = 0, nu = 0, nc = 0, batch = 0, nrhs = 1;
  long long nz = 0, nv = 0, nzf = 0, nlf = 0, len[FBSTAB_MPC_NSEQ] = {};
  std::vector<Ev> ev;
  std::vector<std::pair<const char*, long long>> pieces;  // of the work array: (address, bytes)
  // the blocks as the kernels received them (the last launch that took one)
  fbstab_mpc_batch_t a = {};
  fbstab_var_batch_t xv = {}, sd = {}, ad = {}, in = {}, outv = {};
  fbstab_dense_out_batch_t out = {};
  fbstab_dense_batch_t dc = {};
  fbstab_mpc_grad_batch_t g = {};
  fbstab_multi_var_batch_t msd = {}, mst = {};
  long long ms = -1, gs = -1;
  CondenseSweepStep st = {};
  CondenseSweepAdjStep ast = {};
  std::vector<CondenseSweepStep> steps_seen;

  void shape(int N_, int nx_, int nu_, int nc_, int batch_, int nrhs_) {
    N = N_; nx = nx_; nu = nu_; nc = nc_; batch = batch_; nrhs = nrhs_;
    const long long M = N + 1;
    nz = M * nu; nv = M * nc; nzf = M * (nx + nu); nlf = M * nx;
    const long long l[FBSTAB_MPC_NSEQ] = {M * nx * nx, M * nu * nu, M * nu * nx, M * nx, M * nu, (long long)N * nx * nx,
                                          (long long)N * nx * nu, (long long)N * nx, M * nc * nx, M * nc * nu, M * nc, nx};
    for (int i = 0; i < FBSTAB_MPC_NSEQ; i++) len[i] = l[i];
  }
  void piece(const void* p, long long bytes) {
    if (p) pieces.emplace_back(static_cast<const char*>(p), bytes);
  }
  void pd(const double* p, long long n) { piece(p, 8 * n); }
  void rd_data(const fbstab_mpc_batch_t& d, bool x0 = true) {
    for (int i = 0; i < FBSTAB_MPC_NSEQ; i++)
      if (x0 || i != FBSTAB_MPC_x0) rd_rows(d.base[i], d.stride[i], len[i], batch);
  }
  void rd_dense(const fbstab_dense_batch_t& d) {
    const long long dl[FBSTAB_DENSE_NARR] = {nz * nz, nz, 0, 0, nv * nz, nv};
    for (int i = 0; i < FBSTAB_DENSE_NARR; i++) rd_rows(d.base[i], d.stride[i], dl[i], batch);
  }
  void adjoint_work(const CondenseAdjointWork& w) {
    pd(w.U, nz * batch); pd(w.gU, nz * batch); pd(w.dU, nz * batch); pd(w.rU, nz * batch); pd(w.eU, nz * batch);
    pd(w.gv, nv * batch); pd(w.dv, nv * batch); pd(w.ev, nv * batch);
  }
  void multi_work(const CondenseMultiWork& w) {
    const long long r = nrhs;
    pd(w.U, nz * batch); pd(w.gU, nz * r * batch); pd(w.dU, nz * r * batch); pd(w.rU, nz * r * batch);
    pd(w.eU, nz * r * batch); pd(w.gv, nv * r * batch); pd(w.dv, nv * r * batch); pd(w.ev, nv * r * batch);
  }
  void multi_rows(const fbstab_multi_var_batch_t& b, const long long* xl, bool write) {
    for (int i = 0; i < 3; i++)
      if (b.base[i])
        for (int q = 0; q < (b.stride[i] == 0 ? 1 : batch); q++)
          for (int k = 0; k < nrhs; k++) {
            double* p = b.base[i] + q * b.stride[i] + k * b.rhs_stride[i];
            if (write) wr(p, xl[i]); else rd(p, xl[i]);
          }
  }

  // fb_condense.hip
  int launch(CondenseKernel id, int grid, long long lds, void** args, hipStream_t) {
    ev.push_back({COND, id, grid, lds});
    a = arg<fbstab_mpc_batch_t>(args, 5);
    rd_data(a);
    if (id == kCondenseExpand) {
      in = arg<fbstab_var_batch_t>(args, 6); outv = arg<fbstab_var_batch_t>(args, 7);
      const long long cl[4] = {nz, 0, nv, nv}, xl[4] = {nzf, nlf, nv, nv};
      for (int i = 0; i < 4; i++) {
        rd_rows(in.base[i], in.stride[i], cl[i], batch);
        wr_rows(outv.base[i], outv.stride[i], xl[i], batch);
      }
      return FBSTAB_HIP_OK;
    }
    out = arg<fbstab_dense_out_batch_t>(args, 6);
    if (id == kCondenseMatrices) {
      wr_rows(out.base[FBSTAB_DENSE_H], out.stride[FBSTAB_DENSE_H], nz * nz, batch);
      wr_rows(out.base[FBSTAB_DENSE_A], out.stride[FBSTAB_DENSE_A], nv * nz, batch);
    } else {
      wr_rows(out.base[FBSTAB_DENSE_f], out.stride[FBSTAB_DENSE_f], nz, batch);
      wr_rows(out.base[FBSTAB_DENSE_b], out.stride[FBSTAB_DENSE_b], nv, batch);
    }
    return FBSTAB_HIP_OK;
  }
  // fb_condense_adjoint.hip
  int launch(CondenseAdjointKernel id, int grid, long long lds, void** args, hipStream_t) {
    ev.push_back({ADJ, id, grid, lds});
    const long long xl[3] = {nzf, nlf, nv};
    if (id == kCondenseAdjSeed || id == kCondenseAdjFinish) {
      a = arg<fbstab_mpc_batch_t>(args, 5);
      xv = arg<fbstab_var_batch_t>(args, 6); sd = arg<fbstab_var_batch_t>(args, 7);
      const CondenseAdjointWork w = arg<CondenseAdjointWork>(args, 8);
      adjoint_work(w);
      rd_data(a);
      for (int i = 0; i < 3; i++) { rd_rows(xv.base[i], xv.stride[i], xl[i], batch); rd_rows(sd.base[i], sd.stride[i], xl[i], batch); }
      if (id == kCondenseAdjSeed) {
        wr(w.U, nz * batch); wr(w.gU, nz * batch); wr(w.gv, nv * batch);
      } else {
        rd(w.dU, nz * batch); rd(w.dv, nv * batch);
        g = arg<fbstab_mpc_grad_batch_t>(args, 9); ad = arg<fbstab_var_batch_t>(args, 10);
        rdi(arg<const int*>(args, 11), batch);
        for (int i = 0; i < FBSTAB_MPC_NSEQ; i++) wr_rows(g.base[i], g.stride[i], len[i], batch);
        for (int i = 0; i < 3; i++) wr_rows(ad.base[i], ad.stride[i], xl[i], batch);
      }
    } else if (id == kCondenseAdjResidual) {
      CHECK(arg<int>(args, 0) == nz && arg<int>(args, 1) == nv, "residual sizes");
      rd_rows(arg<const double*>(args, 2), arg<long long>(args, 3), nz * nz, batch);
      rd_rows(arg<const double*>(args, 4), arg<long long>(args, 5), nv * nz, batch);
      const CondenseAdjointWork w = arg<CondenseAdjointWork>(args, 7);
      adjoint_work(w);
      rd(w.gU, nz * batch); rd(w.dU, nz * batch); rd(w.dv, nv * batch); wr(w.rU, nz * batch);
    } else {
      const CondenseAdjointWork w = arg<CondenseAdjointWork>(args, 2);
      adjoint_work(w);
      rd(w.eU, nz * batch); rd(w.ev, nv * batch); wr(w.dU, nz * batch); wr(w.dv, nv * batch);
    }
    return FBSTAB_HIP_OK;
  }
  // fb_condense_multi.hip
  int launch(CondenseMultiKernel id, int grid, long long lds, void** args, hipStream_t) {
    ev.push_back({MULTI, id, grid, lds});
    const long long xl[3] = {nzf, nlf, nv}, r = nrhs;
    if (id == kCondenseMultiSeed) {
      CHECK(arg<int>(args, 5) == nrhs, "nrhs %d", arg<int>(args, 5));
      a = arg<fbstab_mpc_batch_t>(args, 9); xv = arg<fbstab_var_batch_t>(args, 10);
      msd = arg<fbstab_multi_var_batch_t>(args, 11);
      const CondenseMultiWork w = arg<CondenseMultiWork>(args, 12);
      multi_work(w);
      rd_data(a);
      for (int i = 0; i < 3; i++) rd_rows(xv.base[i], xv.stride[i], xl[i], batch);
      multi_rows(msd, xl, false);
      wr(w.U, nz * batch); wr(w.gU, nz * r * batch); wr(w.gv, nv * r * batch);
    } else if (id == kCondenseMultiResidual) {
      rd_rows(arg<const double*>(args, 4), arg<long long>(args, 5), nz * nz, batch);
      rd_rows(arg<const double*>(args, 6), arg<long long>(args, 7), nv * nz, batch);
      const CondenseMultiWork w = arg<CondenseMultiWork>(args, 9);
      multi_work(w);
      rd(w.gU, nz * r * batch); rd(w.dU, nz * r * batch); rd(w.dv, nv * r * batch); wr(w.rU, nz * r * batch);
    } else if (id == kCondenseMultiCorrect) {
      const CondenseMultiWork w = arg<CondenseMultiWork>(args, 5);
      multi_work(w);
      rd(w.eU, nz * r * batch); rd(w.ev, nv * r * batch); wr(w.dU, nz * r * batch); wr(w.dv, nv * r * batch);
      gs = arg<long long>(args, 7);
      wr_rows(arg<double*>(args, 6), gs, (long long)nu * nx, batch);
      rdi(arg<const int*>(args, 8), batch);
    } else {
      a = arg<fbstab_mpc_batch_t>(args, 9); msd = arg<fbstab_multi_var_batch_t>(args, 10);
      const CondenseMultiWork w = arg<CondenseMultiWork>(args, 11);
      mst = arg<fbstab_multi_var_batch_t>(args, 12);
      multi_work(w);
      rd_data(a);
      multi_rows(msd, xl, false);
      rd(w.dU, nz * r * batch); rd(w.dv, nv * r * batch);
      multi_rows(mst, xl, true);
      rdi(arg<const int*>(args, 13), batch);
    }
    return FBSTAB_HIP_OK;
  }
  // fb_condense_sweep.hip
  int launch(CondenseSweepKernel id, int grid, long long lds, void** args, hipStream_t) {
    ev.push_back({SWEEP, id, grid, lds});
    if (id == kCondenseSweepX0Map) {
      a = arg<fbstab_mpc_batch_t>(args, 5);
      rd_data(a);
      ms = arg<long long>(args, 7);
      wr_rows(arg<double*>(args, 6), ms, (nz + nv) * nx, batch);
    } else if (id == kCondenseSweepBegin) {
      xv = arg<fbstab_var_batch_t>(args, 4);
      rd_rows(xv.base[0], xv.stride[0], nzf, batch); rd_rows(xv.base[2], xv.stride[2], nv, batch);
      pd(arg<double*>(args, 5), nz * batch); pd(arg<double*>(args, 6), nv * batch); piece(arg<int*>(args, 7), 4LL * batch);
      wr(arg<double*>(args, 5), nz * batch); wr(arg<double*>(args, 6), nv * batch); wri(arg<int*>(args, 7), batch);
    } else {
      st = arg<CondenseSweepStep>(args, 0);
      steps_seen.push_back(st);
      pd(st.U, nz * batch); pd(st.v, nv * batch); piece(st.gone, 4LL * batch); pd(st.xkeep, (long long)nx * batch);
      for (int q = 0; q < batch; q++) g_sink = g_sink + st.out[q].solve_time;
      rdi(st.gone, batch); wri(st.gone, batch);
      rd(st.U, nz * batch); wr(st.U, nz * batch); rd(st.v, nv * batch); wr(st.v, nv * batch);
      rd_rows(st.x0, st.sx0, nx, batch); wr_rows(st.x0, st.sx0, nx, batch);
      if (st.xkeep) wr(st.xkeep, (long long)nx * batch);
      rd_rows(st.Ap, st.sAp, (long long)nx * nx, batch); rd_rows(st.Bp, st.sBp, (long long)nx * nu, batch);
      if (st.w) rd(st.w, (long long)nx * batch);
      if (st.u_log) wr(st.u_log, (long long)nu * batch);
      if (st.x_log) wr(st.x_log, (long long)nx * batch);
      if (st.U_log) wr(st.U_log, nz * batch);
      if (st.v_log) wr(st.v_log, nv * batch);
      if (st.eflag_log) wri(st.eflag_log, batch);
      if (st.newton_log) wri(st.newton_log, batch);
      if (st.affine) {
        rd_rows(st.M, st.sM, (nz + nv) * nx, batch); rd_rows(st.f0, st.sf0, nz, batch); rd_rows(st.b0, st.sb0, nv, batch);
        wr_rows(st.f, st.sf, nz, batch); wr_rows(st.b, st.sb, nv, batch);
      }
    }
    return FBSTAB_HIP_OK;
  }
  // fb_condense_sweep_adjoint.hip
  int launch(CondenseSweepAdjKernel id, int grid, long long lds, void** args, hipStream_t) {
    ev.push_back({SADJ, id, grid, lds});
    if (id == kCondenseSweepAdjBegin) {
      g = arg<fbstab_mpc_grad_batch_t>(args, 4);
      for (int i = 0; i < FBSTAB_MPC_NSEQ; i++) wr_rows(g.base[i], g.stride[i], len[i], batch);
      double* gz = arg<double*>(args, 5);
      pd(gz, nzf * batch);
      if (gz) wr(gz, nzf * batch);
      if (arg<double*>(args, 6)) wr(arg<double*>(args, 6), nz * batch);
      if (arg<double*>(args, 7)) wr(arg<double*>(args, 7), nv * batch);
      wri(arg<int*>(args, 8), batch);
    } else if (id == kCondenseSweepAdjStep) {
      const CondenseSweepAdjStep s = ast = arg<CondenseSweepAdjStep>(args, 0);
      piece(s.st1, 4LL * batch); piece(s.st2, 4LL * batch);
      pd(s.dU, nz * batch); pd(s.dv, nv * batch); pd(s.dl0, (long long)nx * batch); pd(s.mu, (long long)nx * batch);
      pd(s.gU, nz * batch);
      if (s.close) {
        rdi(s.eflag_close, batch); rdi(s.st1, batch); rdi(s.st2, batch);
        rd(s.dU, nz * batch); rd(s.dv, nv * batch); rd(s.mu, (long long)nx * batch);
        if (s.dl0) rd(s.dl0, (long long)nx * batch);
        if (s.gf0) wr(s.gf0, nz * batch);
        if (s.gb0) wr(s.gb0, nv * batch);
      }
      rdi(s.status, batch); wri(s.status, batch);
      rd_rows(s.Ap, s.sAp, (long long)nx * nx, batch); rd_rows(s.Bp, s.sBp, (long long)nx * nu, batch);
      if (s.affine) { rd_rows(s.M, s.sM, (nz + nv) * nx, batch); rd_rows(s.f0, s.sf0, nz, batch); rd_rows(s.b0, s.sb0, nv, batch); }
      if (s.open) {
        rdi(s.eflag_open, batch); rd(s.x_log, (long long)nx * batch);
        if (s.gu) rd(s.gu, (long long)nu * batch);
        if (s.gx) rd(s.gx, (long long)nx * batch);
        if (s.mu_log) wr(s.mu_log, (long long)nx * batch);
        wr(s.mu, (long long)nx * batch); wr(s.gU, nz * batch);
        if (s.dl0) wr(s.dl0, (long long)nx * batch);
        if (s.affine) { wr_rows(s.f, s.sf, nz, batch); wr_rows(s.b, s.sb, nv, batch); }
      } else {
        wr_rows(s.gx0, s.sgx0, nx, batch);
      }
    } else {
      a = arg<fbstab_mpc_batch_t>(args, 5);
      rd_data(a, false);
      const CondenseSweepAdjFinish f = arg<CondenseSweepAdjFinish>(args, 6);
      const fbstab_mpc_grad_batch_t gf = arg<fbstab_mpc_grad_batch_t>(args, 7);
      CHECK(gf.base[FBSTAB_MPC_x0] == nullptr, "the finish kernel takes no x0 slot");
      pd(f.z, nzf * batch); pd(f.gz, nzf * batch); pd(f.l, nlf * batch);
      rd(f.x, (long long)nx * batch); rd(f.U, nz * batch); rd(f.v, nv * batch); rd(f.dU, nz * batch); rd(f.dv, nv * batch);
      rdi(f.eflag, batch); rdi(f.st1, batch); rdi(f.st2, batch);
      wr(f.z, nzf * batch); wr(f.l, nlf * batch); rd(f.gz, nzf * batch);
      if (f.dl0) wr(f.dl0, (long long)nx * batch);
      for (int i = 0; i < FBSTAB_MPC_NSEQ; i++) wr_rows(gf.base[i], gf.stride[i], len[i], batch);
    }
    return FBSTAB_HIP_OK;
  }

  // the dense handle's entry points
  int solve(int b, const fbstab_dense_batch_t* d, const fbstab_var_batch_t* xc, fbstab_solver_out_t* o, hipStream_t) {
    ev.push_back({DENSE, D_SOLVE, b, 0});
    dc = *d;
    rd_dense(dc);
    pd(xc->base[0], nz * batch); pd(xc->base[2], nv * batch); pd(xc->base[3], nv * batch);
    CHECK(xc->stride[0] == nz && xc->stride[2] == nv && xc->stride[3] == nv && !xc->base[1], "the condensed point is packed");
    rd(xc->base[0], nz * batch); wr(xc->base[0], nz * batch); rd(xc->base[2], nv * batch); wr(xc->base[2], nv * batch);
    wr(xc->base[3], nv * batch);
    for (int q = 0; q < batch; q++) o[q].solve_time = 0.0;
    return FBSTAB_HIP_OK;
  }
  int adjoint(int b, const fbstab_dense_batch_t* d, const fbstab_var_batch_t* xc, const fbstab_var_batch_t* s, double,
              const fbstab_var_batch_t* ac, int* status, hipStream_t) {
    ev.push_back({DENSE, D_ADJOINT, b, 0});
    dc = *d;
    rd_dense(dc);
    rd_rows(xc->base[0], xc->stride[0], nz, batch); rd_rows(xc->base[2], xc->stride[2], nv, batch);
    CHECK(s->stride[0] == nz && s->stride[2] == nv && ac->stride[0] == nz && ac->stride[2] == nv, "packed seeds and steps");
    rd(s->base[0], nz * batch);
    if (s->base[2]) rd(s->base[2], nv * batch);
    wr(ac->base[0], nz * batch); wr(ac->base[2], nv * batch);
    wri(status, batch);
    return FBSTAB_HIP_OK;
  }
  int multi(int b, const fbstab_dense_batch_t* d, const fbstab_var_batch_t* xc, int r, const fbstab_multi_var_batch_t* s,
            double, const fbstab_multi_var_batch_t* ac, int* status, hipStream_t) {
    ev.push_back({DENSE, D_MULTI, b, 0});
    dc = *d;
    rd_dense(dc);
    CHECK(r == nrhs, "nrhs %d", r);
    rd_rows(xc->base[0], xc->stride[0], nz, batch); rd_rows(xc->base[2], xc->stride[2], nv, batch);
    CHECK(s->stride[0] == nz * r && s->rhs_stride[0] == nz && ac->stride[2] == nv * r && ac->rhs_stride[2] == nv, "packed");
    rd(s->base[0], nz * r * batch);
    if (s->base[2]) rd(s->base[2], nv * r * batch);
    wr(ac->base[0], nz * r * batch); wr(ac->base[2], nv * r * batch);
    wri(status, batch);
    return FBSTAB_HIP_OK;
  }
};

// ---- a caller: every argument of every entry point, valid, in buffers of exactly the documented length ----------------
struct Case {
  int N, nx, nu, nc, batch, nrhs, steps, mode, what = FBSTAB_CONDENSE_ALL, retire = 0, device = 0;
  int traj_per_group = 0, rhs_per_group = 0;
  bool shared, x0_mode = false, data_grads = true;
  double sigma = 0.0;
  Sim sim;
  SolverBase h;
  SolverBase* hp = &h;
  fbstab_mpc_batch_t data = {};
  const fbstab_mpc_batch_t* data_p = &data;
  fbstab_dense_batch_t dense = {};
  fbstab_dense_out_batch_t dout = {};
  const fbstab_dense_out_batch_t* dout_p = &dout;
  fbstab_var_batch_t x = {}, xc = {}, seed = {}, adj = {};
  const fbstab_var_batch_t* x_p = &x;
  fbstab_mpc_grad_batch_t grad = {};
  fbstab_multi_var_batch_t mseed = {}, mstep = {};
  const fbstab_multi_var_batch_t* mstep_p = &mstep;
  double *gain = nullptr, *mapout = nullptr, *work = nullptr;
  long long gain_stride = 0, map_stride = 0;
  fbstab_condensed_map_t map = {};
  const fbstab_condensed_map_t* map_p = &map;
  fbstab_receding_plant_t plant = {};
  fbstab_sweep_scenario_t scen = {};
  fbstab_condensed_sweep_log_t log = {};
  fbstab_solver_out_t* out = nullptr;
  double *gu = nullptr, *gx = nullptr, *gf0 = nullptr, *gb0 = nullptr, *mu_log = nullptr;
  int* status = nullptr;

  // one block of `batch` rows of n doubles: records with a gap, one shared row, or one QP with a garbage stride
  double* blk(long long n, long long* stride, bool share = false) {
    if (batch <= 1) { *stride = kGarbage; return D(n); }
    if (share) { *stride = 0; return D(n); }
    *stride = n + kGap;
    return D((batch - 1) * *stride + n);
  }
  void mblk(fbstab_multi_var_batch_t* b, int i, long long n) {
    const long long rs = nrhs > 1 ? n + 1 : n;
    const long long st = (nrhs - 1) * rs + n + 2;
    b->base[i] = D((batch > 1 ? (batch - 1) * st : 0) + (nrhs - 1) * rs + n);
    b->rhs_stride[i] = nrhs > 1 ? rs : kGarbage;
    b->stride[i] = batch > 1 ? st : kGarbage;
  }
  Case(int N_, int nx_, int nu_, int nc_, int batch_, int nrhs_, int steps_, int mode_, bool shared_)
      : N(N_), nx(nx_), nu(nu_), nc(nc_), batch(batch_), nrhs(nrhs_), steps(steps_), mode(mode_), shared(shared_) {
    sim.shape(N, nx, nu, nc, batch, nrhs);
    const long long nz = sim.nz, nv = sim.nv, B = batch, S = steps;
    h.max_batch = 3; h.device = 0;
    h.var_len[0] = nz; h.var_len[1] = 0; h.var_len[2] = h.var_len[3] = nv;
    for (int i = 0; i < FBSTAB_MPC_NSEQ; i++) {
      const bool matrix = i == FBSTAB_MPC_Q || i == FBSTAB_MPC_R || i == FBSTAB_MPC_S || i == FBSTAB_MPC_A ||
                          i == FBSTAB_MPC_B || i == FBSTAB_MPC_E || i == FBSTAB_MPC_L;
      data.base[i] = blk(sim.len[i], &data.stride[i], shared && matrix);
      grad.base[i] = blk(sim.len[i], &grad.stride[i]);
    }
    const long long dl[FBSTAB_DENSE_NARR] = {nz * nz, nz, 0, 0, nv * nz, nv};
    for (int i : {FBSTAB_DENSE_H, FBSTAB_DENSE_f, FBSTAB_DENSE_A, FBSTAB_DENSE_b}) {
      const bool matrix = i == FBSTAB_DENSE_H || i == FBSTAB_DENSE_A;
      dout.base[i] = blk(dl[i], &dout.stride[i], shared && matrix);
      dense.base[i] = dout.base[i]; dense.stride[i] = dout.stride[i];
    }
    const long long xl[4] = {sim.nzf, sim.nlf, nv, nv}, cl[4] = {nz, 0, nv, nv};
    for (int i = 0; i < 4; i++) {
      x.base[i] = blk(xl[i], &x.stride[i]);
      if (i != 1) xc.base[i] = blk(cl[i], &xc.stride[i]);
      if (i < 3) { seed.base[i] = blk(xl[i], &seed.stride[i]); adj.base[i] = blk(xl[i], &adj.stride[i]); }
      if (i < 3) { mblk(&mseed, i, xl[i]); mblk(&mstep, i, xl[i]); }
    }
    gain = blk((long long)nu * nx, &gain_stride);
    mapout = blk((nz + nv) * nx, &map_stride, shared);
    map.M = blk((nz + nv) * nx, &map.stride_M, shared);
    map.f0 = blk(nz, &map.stride_f0, shared);
    map.b0 = blk(nv, &map.stride_b0, shared);
    plant.A = blk((long long)nx * nx, &plant.stride_A, shared);
    plant.B = blk((long long)nx * nu, &plant.stride_B, shared);
    scen.w = D(S * B * nx); scen.shift = 1;
    log.u = D(S * B * nu); log.x = D(S * B * nx); log.U = D(S * B * nz); log.v = D(S * B * nv);
    log.eflag = I(S * B); log.newton = I(S * B);
    gu = D(S * B * nu); gx = D(S * B * nx); mu_log = D(S * B * nx); gf0 = D(B * nz); gb0 = D(B * nv);
    status = I(B);
    g_out.emplace_back(new fbstab_solver_out_t[(size_t)B]());
    out = g_out.back().get();
  }
  static std::vector<std::unique_ptr<fbstab_solver_out_t[]>> g_out;

  auto launcher() {
    return [this](auto id, int grid, long long lds, void** args, hipStream_t s) { return sim.launch(id, grid, lds, args, s); };
  }
  auto dense_solve() {
    return [this](int b, const fbstab_dense_batch_t* d, const fbstab_var_batch_t* c, fbstab_solver_out_t* o, hipStream_t s) {
      return sim.solve(b, d, c, o, s);
    };
  }
  auto dense_adjoint() {
    return [this](int b, const fbstab_dense_batch_t* d, const fbstab_var_batch_t* c, const fbstab_var_batch_t* sd, double sg,
                  const fbstab_var_batch_t* ac, int* st, hipStream_t s) { return sim.adjoint(b, d, c, sd, sg, ac, st, s); };
  }
  auto dense_multi() {
    return [this](int b, const fbstab_dense_batch_t* d, const fbstab_var_batch_t* c, int r, const fbstab_multi_var_batch_t* sd,
                  double sg, const fbstab_multi_var_batch_t* ac, int* st, hipStream_t s) {
      return sim.multi(b, d, c, r, sd, sg, ac, st, s);
    };
  }

  // the entry points; each allocates its work array from its *_sizes function (the adjoint: from the header's formula)
  int condense() { return condense_run(N, nx, nu, nc, batch, data_p, what, dout_p, device, nullptr, launcher()); }
  int expand() { return expand_run(N, nx, nu, nc, batch, data_p, &xc, x_p, device, nullptr, launcher()); }
  long long work_per = 0;
  int adjoint() {
    work_per = 5 * sim.nz + 3 * sim.nv;
    if (!work) work = D(work_per * batch);
    return condensed_adjoint_run(hp, N, nx, nu, nc, batch, data_p, &dense, &x, &seed, sigma, &grad, &adj, work, status,
                                 nullptr, launcher(), dense_adjoint());
  }
  int kkt() {
    condensed_multi_sizes(N, nx, nu, nc, nrhs, rhs_per_group, nullptr, nullptr, &work_per);
    if (!work) work = D(work_per * batch);
    return condensed_multi_run(hp, N, nx, nu, nc, batch, data_p, &dense, &x, false, nrhs, &mseed, sigma, mstep_p, nullptr, 0,
                               rhs_per_group, work, status, nullptr, launcher(), dense_multi());
  }
  int x0_sensitivity() {  // (nrhs == nx: the Case is built so)
    condensed_multi_sizes(N, nx, nu, nc, nx, rhs_per_group, nullptr, nullptr, &work_per);
    if (!work) work = D(work_per * batch);
    return condensed_multi_run(hp, N, nx, nu, nc, batch, data_p, &dense, &x, true, nx, nullptr, sigma, mstep_p, gain,
                               gain_stride, rhs_per_group, work, status, nullptr, launcher(), dense_multi());
  }
  int x0_map() { return condensed_x0_map_run(N, nx, nu, nc, batch, data_p, mapout, map_stride, device, nullptr, launcher()); }
  int sweep() {
    condensed_sweep_sizes("condensed sweep", N, nx, nu, nc, 0, 0, nullptr, nullptr, &work_per, nullptr, false);
    if (!work) work = D(work_per * batch);
    return condensed_sweep_run(hp, N, nx, nu, nc, batch, data_p, &dense, map_p, &x, out, &plant, steps, retire, &scen, mode,
                               &log, traj_per_group, work, nullptr, launcher(), dense_solve());
  }
  int sweep_adjoint() {
    long long per = 0, per_grad = 0;
    condensed_sweep_sizes("condensed sweep adjoint", N, nx, nu, nc, 0, 0, nullptr, nullptr, &per, &per_grad, true);
    if (!data_grads)
      for (int i = 0; i < FBSTAB_MPC_NSEQ; i++)
        if (i != FBSTAB_MPC_x0) grad.base[i] = nullptr;
    work_per = data_grads || mode == FBSTAB_CONDENSED_SWEEP_RECONDENSE ? per_grad : per;
    if (!work) work = D(work_per * batch);
    return condensed_sweep_adjoint_run(hp, N, nx, nu, nc, batch, data_p, &dense, map_p, &plant, steps, &log, gu, gx, sigma,
                                       &grad, gf0, gb0, mu_log, status, mode, traj_per_group, work, nullptr, launcher(),
                                       dense_adjoint());
  }
};
std::vector<std::unique_ptr<fbstab_solver_out_t[]>> Case::g_out;

const int kShapes[2][4] = {{2, 2, 1, 1}, {2, 3, 2, 1}};
#define OK(call) do { const int rc_ = (call); CHECK(rc_ == FBSTAB_HIP_OK, "%s", g_error.c_str()); } while (0)

// ---- placement --------------------------------------------------------------------------------------------------
// kernel side against caller: equal with batch > 1, the packed length with batch == 1
void same(const char* what, const void* kb, long long ks, const void* cb, long long cs, long long len, int batch) {
  CHECK(kb == cb, "%s: base", what);
  CHECK(ks == (batch > 1 ? cs : len), "%s: stride %lld (caller %lld, length %lld, batch %d)", what, ks, cs, len, batch);
}
void placement_of(const int* s, int batch, bool shared) {
  const int nx = s[1];
  {
    Case c(s[0], s[1], s[2], s[3], batch, 1, 0, 0, shared);
    OK(c.condense());
    const Sim& m = c.sim;
    const long long dl[FBSTAB_DENSE_NARR] = {m.nz * m.nz, m.nz, 0, 0, m.nv * m.nz, m.nv};
    for (int i = 0; i < FBSTAB_MPC_NSEQ; i++) {
      CHECK(m.a.base[i] == c.data.base[i] && m.a.stride[i] == c.data.stride[i], "the data block passes as it is (slot %d)", i);
      if (shared && batch > 1 && i < FBSTAB_MPC_q) CHECK(m.a.stride[i] == 0, "stride 0 is kept");
    }
    for (int i : {FBSTAB_DENSE_H, FBSTAB_DENSE_f, FBSTAB_DENSE_A, FBSTAB_DENSE_b})
      same("condense out", m.out.base[i], m.out.stride[i], c.dout.base[i], c.dout.stride[i], dl[i], batch);
    if (shared && batch > 1) CHECK(m.out.stride[FBSTAB_DENSE_H] == 0 && m.out.stride[FBSTAB_DENSE_A] == 0, "stride 0 is kept");
  }
  {
    Case c(s[0], s[1], s[2], s[3], batch, 1, 0, 0, shared);
    OK(c.expand());
    const Sim& m = c.sim;
    const long long xl[4] = {m.nzf, m.nlf, m.nv, m.nv}, cl[4] = {m.nz, 0, m.nv, m.nv};
    for (int i = 0; i < 4; i++) {
      same("expand x", m.outv.base[i], m.outv.stride[i], c.x.base[i], c.x.stride[i], xl[i], batch);
      if (i != 1) same("expand xc", m.in.base[i], m.in.stride[i], c.xc.base[i], c.xc.stride[i], cl[i], batch);
    }
  }
  {
    Case c(s[0], s[1], s[2], s[3], batch, 1, 0, 0, shared);
    OK(c.adjoint());
    const Sim& m = c.sim;
    const long long xl[3] = {m.nzf, m.nlf, m.nv}, dl[FBSTAB_DENSE_NARR] = {m.nz * m.nz, m.nz, 0, 0, m.nv * m.nz, m.nv};
    for (int i = 0; i < 3; i++) {
      same("adjoint x", m.xv.base[i], m.xv.stride[i], c.x.base[i], c.x.stride[i], xl[i], batch);
      same("adjoint seed", m.sd.base[i], m.sd.stride[i], c.seed.base[i], c.seed.stride[i], xl[i], batch);
      same("adjoint adj", m.ad.base[i], m.ad.stride[i], c.adj.base[i], c.adj.stride[i], xl[i], batch);
    }
    for (int i : {FBSTAB_DENSE_H, FBSTAB_DENSE_f, FBSTAB_DENSE_A, FBSTAB_DENSE_b})
      same("adjoint images", m.dc.base[i], m.dc.stride[i], c.dense.base[i], c.dense.stride[i], dl[i], batch);
    for (int i = 0; i < FBSTAB_MPC_NSEQ; i++)  // (the gradient block passes as it is: the kernel reads QP 0 at the base)
      CHECK(m.g.base[i] == c.grad.base[i] && m.g.stride[i] == c.grad.stride[i], "gradient slot %d", i);
  }
  for (int nrhs : {1, 3}) {
    Case c(s[0], s[1], s[2], s[3], batch, nrhs, 0, 0, shared);
    OK(c.kkt());
    const Sim& m = c.sim;
    const long long xl[3] = {m.nzf, m.nlf, m.nv};
    for (int i = 0; i < 3; i++) {
      same("multi x", m.xv.base[i], m.xv.stride[i], c.x.base[i], c.x.stride[i], xl[i], batch);
      for (int w = 0; w < 2; w++) {
        const fbstab_multi_var_batch_t &k = w ? m.mst : m.msd, &u = w ? c.mstep : c.mseed;
        const long long rs = nrhs > 1 ? u.rhs_stride[i] : xl[i];
        CHECK(k.base[i] == u.base[i] && k.rhs_stride[i] == rs, "multi block %d slot %d: rhs_stride %lld", w, i, k.rhs_stride[i]);
        CHECK(k.stride[i] == (batch > 1 ? u.stride[i] : (nrhs - 1) * rs + xl[i]), "multi block %d slot %d: stride", w, i);
      }
    }
  }
  {
    Case c(s[0], s[1], s[2], s[3], batch, nx, 0, 0, shared);
    OK(c.x0_sensitivity());
    CHECK(c.sim.gs == (batch > 1 ? c.gain_stride : (long long)c.nu * nx), "gain stride %lld", c.sim.gs);
    CHECK(!c.sim.msd.base[0] && !c.sim.msd.base[1] && !c.sim.msd.base[2], "x0 mode has no seed block");
  }
  {
    Case c(s[0], s[1], s[2], s[3], batch, 1, 0, 0, shared);
    OK(c.x0_map());
    CHECK(c.sim.ms == (batch > 1 ? c.map_stride : (c.sim.nz + c.sim.nv) * nx), "map stride %lld", c.sim.ms);
  }
  for (int mode : {FBSTAB_CONDENSED_SWEEP_AFFINE, FBSTAB_CONDENSED_SWEEP_RECONDENSE}) {
    {
      Case c(s[0], s[1], s[2], s[3], batch, 1, 2, mode, shared);
      OK(c.sweep());
      const Sim& m = c.sim;
      const CondenseSweepStep& t = m.st;
      const long long xl[4] = {m.nzf, m.nlf, m.nv, m.nv};
      for (int i = 0; i < 4; i++) same("sweep x", m.xv.base[i], m.xv.stride[i], c.x.base[i], c.x.stride[i], xl[i], batch);
      same("sweep x0", t.x0, t.sx0, c.data.base[FBSTAB_MPC_x0], c.data.stride[FBSTAB_MPC_x0], nx, batch);
      same("sweep A_p", t.Ap, t.sAp, c.plant.A, c.plant.stride_A, 0, batch);
      same("sweep B_p", t.Bp, t.sBp, c.plant.B, c.plant.stride_B, 0, batch);
      same("sweep f", t.f, t.sf, c.dense.base[FBSTAB_DENSE_f], c.dense.stride[FBSTAB_DENSE_f], m.nz, batch);
      same("sweep b", t.b, t.sb, c.dense.base[FBSTAB_DENSE_b], c.dense.stride[FBSTAB_DENSE_b], m.nv, batch);
      if (mode == FBSTAB_CONDENSED_SWEEP_AFFINE) {
        const CondenseSweepStep& f = m.steps_seen[0];  // (behind the last step the map is not read)
        same("sweep M", f.M, f.sM, c.map.M, c.map.stride_M, 0, batch);
        same("sweep f0", f.f0, f.sf0, c.map.f0, c.map.stride_f0, 0, batch);
        same("sweep b0", f.b0, f.sb0, c.map.b0, c.map.stride_b0, 0, batch);
        CHECK(f.affine && f.shift && !t.affine && !t.shift && !f.xkeep && t.xkeep, "the last step neither shifts nor maps");
      }
    }
    Case c(s[0], s[1], s[2], s[3], batch, 1, 2, mode, shared);
    OK(c.sweep_adjoint());
    const Sim& m = c.sim;
    const CondenseSweepAdjStep& t = m.ast;
    same("sweep adjoint A_p", t.Ap, t.sAp, c.plant.A, c.plant.stride_A, 0, batch);
    same("sweep adjoint B_p", t.Bp, t.sBp, c.plant.B, c.plant.stride_B, 0, batch);
    same("sweep adjoint f", t.f, t.sf, c.dense.base[FBSTAB_DENSE_f], c.dense.stride[FBSTAB_DENSE_f], m.nz, batch);
    same("sweep adjoint gx0", t.gx0, t.sgx0, c.grad.base[FBSTAB_MPC_x0], c.grad.stride[FBSTAB_MPC_x0], nx, batch);
    if (mode == FBSTAB_CONDENSED_SWEEP_AFFINE) same("sweep adjoint M", t.M, t.sM, c.map.M, c.map.stride_M, 0, batch);
    for (int i = 0; i < FBSTAB_MPC_NSEQ; i++)
      same("sweep adjoint grad", m.g.base[i], m.g.stride[i], c.grad.base[i], c.grad.stride[i], m.len[i], batch);
  }
}
void placement() {
  for (const int* s : {kShapes[0], kShapes[1]})
    for (int batch : {1, 2, 3})
      for (bool shared : {false, true}) placement_of(s, batch, shared);
}

// ---- carve --------------------------------------------------------------------------------------------------------
void carve_check(const char* what, Case& c, long long header_per) {
  CHECK(c.work_per == header_per, "%s: the sizes function reports %lld doubles, the header %lld", what, c.work_per, header_per);
  const char* lo = reinterpret_cast<const char*>(c.work);
  const char* hi = lo + 8 * c.work_per * c.batch;
  auto& p = c.sim.pieces;
  CHECK(!p.empty(), "%s: no piece of the work array was seen", what);
  for (size_t i = 0; i < p.size(); i++) {
    CHECK(p[i].first >= lo && p[i].first + p[i].second <= hi, "%s: piece %zu leaves the work array", what, i);
    for (size_t j = 0; j < i; j++) {
      const bool same_piece = p[i] == p[j];
      const bool apart = p[i].first + p[i].second <= p[j].first || p[j].first + p[j].second <= p[i].first;
      CHECK(same_piece || apart, "%s: pieces %zu and %zu overlap", what, j, i);
    }
  }
}
void carve() {
  for (const int* s : {kShapes[0], kShapes[1]})
    for (int batch : {1, 2, 3}) {
      const long long M = s[0] + 1, nx = s[1], nz = M * s[2], nv = M * s[3];
      {
        Case c(s[0], s[1], s[2], s[3], batch, 1, 0, 0, false);
        OK(c.adjoint());
        carve_check("condensed adjoint", c, 5 * nz + 3 * nv);
      }
      for (int nrhs : {1, 3}) {
        Case c(s[0], s[1], s[2], s[3], batch, nrhs, 0, 0, false);
        OK(c.kkt());
        carve_check("condensed multi", c, nz + nrhs * (4 * nz + 3 * nv));
      }
      for (int mode : {FBSTAB_CONDENSED_SWEEP_AFFINE, FBSTAB_CONDENSED_SWEEP_RECONDENSE})
        for (int steps : {1, 2}) {
          {
            Case c(s[0], s[1], s[2], s[3], batch, 1, steps, mode, false);
            OK(c.sweep());
            carve_check("condensed sweep", c, nz + 2 * nv + nx + 1);
            // the logs' shares: step k at log + k * batch * n, inside [steps][batch][n]
            CHECK((int)c.sim.steps_seen.size() == steps, "%zu step launches", c.sim.steps_seen.size());
            for (int k = 0; k < (int)c.sim.steps_seen.size(); k++) {
              const CondenseSweepStep& t = c.sim.steps_seen[k];
              const long long kb = (long long)k * batch;
              CHECK(t.u_log == c.log.u + kb * s[2] && t.x_log == c.log.x + kb * nx && t.U_log == c.log.U + kb * nz &&
                        t.v_log == c.log.v + kb * nv && t.eflag_log == c.log.eflag + kb && t.newton_log == c.log.newton + kb &&
                        t.w == c.scen.w + kb * nx, "the log shares of step %d", k);
            }
          }
          for (bool grads : {false, true}) {
            Case c(s[0], s[1], s[2], s[3], batch, 1, steps, mode, false);
            c.data_grads = grads;
            OK(c.sweep_adjoint());
            const bool finish = grads || mode == FBSTAB_CONDENSED_SWEEP_RECONDENSE;
            carve_check("condensed sweep adjoint", c, 4 * nz + 2 * nv + 2 * nx + 1 + (finish ? 2 * M * (nx + s[2]) + M * nx : 0));
          }
        }
    }
}

// ---- sequence -------------------------------------------------------------------------------------------------------
// the LDS bytes of the launches, restated from include/fbstab_hip.h (fbstab_hip_mpc_condensed_sizes, _multi_sizes,
// _sweep_sizes)
long long even(long long n) { return n + (n & 1); }
long long window_doubles(int nx, int nu, int nc) {
  const long long ldx = nx | 1, ldc = nc | 1, ldu = nu | 1;
  return 2 * even(ldx * nx) + even(ldx * nu) + even(ldc * nx) + even(ldu * nx) + even(ldc * nu) + even(ldu * nu);
}
long long condense_lds(int N, int nx, int nu, int nc) {
  const long long m = (N + 2) * even((long long)(nx | 1) * nu), v = (long long)(N + 1) * (nx + nu + nc) + 2 * nx + 8;
  return 8 * (window_doubles(nx, nu, nc) + even(m > v ? m : v));
}
long long multi_lds(int N, int nx, int nu, int nc, int R) {
  const long long M = N + 1, seed = even(M * nx) + 2 * even(nx), fin = even(M * (nx + nu)) + even(M * nc) + 2 * even(nx);
  return 8 * (window_doubles(nx, nu, nc) + R * (seed > fin ? seed : fin));
}
long long sweep_lds(int N, int nx, int nu, int nc, int T, bool shared_m) {
  const long long nz = (long long)(N + 1) * nu, nv = (long long)(N + 1) * nc;
  const long long m = shared_m ? even(((nz + nv) | 1) * nx) : 0;  // (these shapes leave room for it)
  return 8 * (m + T * (2 * even(nx) + even(nz) + even(nv) + 2));
}
void expect_sequence(const char* what, const std::vector<Ev>& got, const std::vector<Ev>& want) {
  CHECK(got.size() == want.size(), "%s: %zu launches, expected %zu", what, got.size(), want.size());
  for (size_t i = 0; i < got.size() && i < want.size(); i++)
    CHECK(got[i] == want[i], "%s: launch %zu is (%d, %d, grid %d, lds %lld), expected (%d, %d, grid %d, lds %lld)", what, i,
          got[i].fam, got[i].id, got[i].grid, got[i].lds, want[i].fam, want[i].id, want[i].grid, want[i].lds);
}
void sequence() {
  for (const int* s : {kShapes[0], kShapes[1]}) {
    const int N = s[0], nx = s[1], nu = s[2], nc = s[3], B = 3;
    const long long lds = condense_lds(N, nx, nu, nc);
    const Ev dsolve = {DENSE, D_SOLVE, B, 0}, dadj = {DENSE, D_ADJOINT, B, 0}, dmulti = {DENSE, D_MULTI, B, 0};
    const Ev vectors = {COND, kCondenseVectors, B, lds}, expand = {COND, kCondenseExpand, B, lds};
    const Ev residual = {ADJ, kCondenseAdjResidual, B, 0}, correct = {ADJ, kCondenseAdjCorrect, B, 0};
    {  // condense: the matrices on batch x (N + 1) workgroups - N + 1 for a shared model - then the vectors
      Case c(N, nx, nu, nc, B, 1, 0, 0, false);
      OK(c.condense());
      expect_sequence("condense", c.sim.ev, {{COND, kCondenseMatrices, B * (N + 1), lds}, vectors});
      Case sh(N, nx, nu, nc, B, 1, 0, 0, true);
      OK(sh.condense());
      expect_sequence("condense, shared model", sh.sim.ev, {{COND, kCondenseMatrices, N + 1, lds}, vectors});
      Case m(N, nx, nu, nc, B, 1, 0, 0, false);
      m.what = FBSTAB_CONDENSE_MATRICES;
      OK(m.condense());
      expect_sequence("condense MATRICES", m.sim.ev, {{COND, kCondenseMatrices, B * (N + 1), lds}});
      Case v(N, nx, nu, nc, B, 1, 0, 0, false);
      v.what = FBSTAB_CONDENSE_VECTORS;
      OK(v.condense());
      expect_sequence("condense VECTORS", v.sim.ev, {vectors});
      Case e(N, nx, nu, nc, B, 1, 0, 0, false);
      OK(e.expand());
      expect_sequence("expand", e.sim.ev, {expand});
      Case z(N, nx, nu, nc, 0, 1, 0, 0, false);
      OK(z.condense()); OK(z.expand());
      expect_sequence("batch 0", z.sim.ev, {});
    }
    {
      Case c(N, nx, nu, nc, B, 1, 0, 0, false);
      OK(c.adjoint());
      expect_sequence("condensed adjoint", c.sim.ev,
                      {{ADJ, kCondenseAdjSeed, B, lds}, dadj, residual, dadj, correct, {ADJ, kCondenseAdjFinish, B, lds}});
    }
    {  // 3 right-hand sides: the rule takes all in one group; rhs_per_group = 1 makes three
      for (int per_group : {0, 1}) {
        Case c(N, nx, nu, nc, B, 3, 0, 0, false);
        c.rhs_per_group = per_group;
        OK(c.kkt());
        const int R = per_group ? 1 : 3, grid = B * (3 / R);
        const long long ml = multi_lds(N, nx, nu, nc, R);
        expect_sequence("condensed kkt solve", c.sim.ev,
                        {{MULTI, kCondenseMultiSeed, grid, ml}, dmulti, {MULTI, kCondenseMultiResidual, grid, 0}, dmulti,
                         {MULTI, kCondenseMultiCorrect, grid, 0}, {MULTI, kCondenseMultiFinish, grid, ml}});
      }
      for (bool gain_only : {false, true}) {
        Case c(N, nx, nu, nc, B, nx, 0, 0, false);
        if (gain_only) c.mstep_p = nullptr;
        OK(c.x0_sensitivity());
        const long long ml = multi_lds(N, nx, nu, nc, nx);
        std::vector<Ev> want = {{MULTI, kCondenseMultiSeed, B, ml}, dmulti, {MULTI, kCondenseMultiResidual, B, 0}, dmulti,
                                {MULTI, kCondenseMultiCorrect, B, 0}};
        if (!gain_only) want.push_back({MULTI, kCondenseMultiFinish, B, ml});
        expect_sequence("condensed x0 sensitivity", c.sim.ev, want);
      }
    }
    {
      const int blocks = (nx + nu - 1) / nu;
      Case c(N, nx, nu, nc, B, 1, 0, 0, false);
      OK(c.x0_map());
      expect_sequence("x0 map", c.sim.ev, {{SWEEP, kCondenseSweepX0Map, B * blocks, lds}});
      Case sh(N, nx, nu, nc, B, 1, 0, 0, true);
      OK(sh.x0_map());
      expect_sequence("x0 map, shared model", sh.sim.ev, {{SWEEP, kCondenseSweepX0Map, blocks, lds}});
    }
    // traj_per_group: 0 - the rule gives 64 for these sizes, clamped to the batch, one group; 2 - two groups of 2;
    // 8 - clamped as well
    for (int T : {0, 2, 8})
      for (bool shared : {false, true}) {
        const int Tu = T == 2 ? 2 : B, groups = T == 2 ? 2 : 1;
        const Ev begin = {SWEEP, kCondenseSweepBegin, B, 0};
        for (int steps : {0, 1, 2}) {
          Case c(N, nx, nu, nc, B, 1, steps, FBSTAB_CONDENSED_SWEEP_AFFINE, shared);
          c.traj_per_group = T;
          OK(c.sweep());
          const Ev step = {SWEEP, kCondenseSweepStep, groups, sweep_lds(N, nx, nu, nc, Tu, shared)};
          std::vector<Ev> want;
          if (steps > 0) want.push_back(begin);
          for (int k = 0; k < steps; k++) { want.push_back(dsolve); want.push_back(step); }
          if (steps > 0) want.push_back(expand);
          expect_sequence("sweep AFFINE", c.sim.ev, want);

          Case r(N, nx, nu, nc, B, 1, steps, FBSTAB_CONDENSED_SWEEP_RECONDENSE, shared);
          r.traj_per_group = T;
          OK(r.sweep());
          const Ev rstep = {SWEEP, kCondenseSweepStep, groups, sweep_lds(N, nx, nu, nc, Tu, false)};
          want.clear();
          if (steps > 0) want.push_back(begin);
          for (int k = 0; k < steps; k++) {
            want.push_back(dsolve); want.push_back(rstep);
            if (k + 1 < steps) want.push_back(vectors);  // (not behind the last step)
          }
          if (steps > 0) want.push_back(expand);
          expect_sequence("sweep RECONDENSE", r.sim.ev, want);

          for (int mode : {FBSTAB_CONDENSED_SWEEP_AFFINE, FBSTAB_CONDENSED_SWEEP_RECONDENSE})
            for (bool grads : {false, true}) {
              Case a(N, nx, nu, nc, B, 1, steps, mode, shared);
              a.traj_per_group = T;
              a.data_grads = grads;
              OK(a.sweep_adjoint());
              const bool affine = mode == FBSTAB_CONDENSED_SWEEP_AFFINE, finish = grads || !affine;
              const Ev astep = {SADJ, kCondenseSweepAdjStep, groups, sweep_lds(N, nx, nu, nc, Tu, affine && shared)};
              want = {{SADJ, kCondenseSweepAdjBegin, B, 0}};
              for (int k = steps - 1; k >= 0; k--) {
                want.push_back(astep);
                if (!affine) want.push_back(vectors);
                want.insert(want.end(), {dadj, residual, dadj, correct});
                if (finish) want.push_back({SADJ, kCondenseSweepAdjFinish, B, lds});
              }
              if (steps > 0) want.push_back(astep);  // (the launch that only closes)
              expect_sequence("sweep adjoint", a.sim.ev, want);
            }
        }
      }
  }
  // the launch helper: a launch of more than 64 KiB of dynamic LDS sets the kernel's attribute first
  for (long long lds : {0LL, 64LL * 1024, 64LL * 1024 + 8}) {
    const long calls = fb_shim::state().calls;
    int asked = -1;
    OK(condense_launch([&](CondenseKernel k, int* threads) { asked = k; *threads = 256; return (const void*)&asked; },
                       kCondenseVectors, 1, lds, nullptr, nullptr));
    CHECK(asked == kCondenseVectors, "the getter is asked for the id");
    CHECK(fb_shim::state().calls - calls == (lds > 64 * 1024 ? 2 : 1), "%lld bytes: %ld runtime calls", lds,
          fb_shim::state().calls - calls);
  }
}

// ---- refusals -------------------------------------------------------------------------------------------------------
typedef int (Case::*Entry)();
// `early`: refused before any device call
void refuse(const char* what, Entry entry, int code, const char* text, const std::function<void(Case&)>& spoil,
            bool early = true, int nrhs = 1) {
  Case c(2, 2, 1, 1, 2, nrhs, 2, FBSTAB_CONDENSED_SWEEP_AFFINE, false);
  c.work = D(4096);  // (no refused call reaches it)
  spoil(c);
  const long calls = fb_shim::state().calls;
  g_error.clear();
  const int rc = (c.*entry)();
  CHECK(rc == code && g_error == text, "%s: %d \"%s\", expected %d \"%s\"", what, rc, g_error.c_str(), code, text);
  if (early) CHECK(fb_shim::state().calls == calls, "%s: %ld device calls before the refusal", what, fb_shim::state().calls - calls);
  CHECK(c.sim.ev.empty(), "%s: %zu launches queued", what, c.sim.ev.size());
}
const int A = FBSTAB_HIP_ERR_ARGUMENT, U = FBSTAB_HIP_ERR_UNSUPPORTED, DV = FBSTAB_HIP_ERR_DEVICE;

// what every entry point refuses through condense_check, and (with_device) the device and the LDS rule behind it
void refuse_common(const char* what, Entry e, bool with_device, int nrhs = 1) {
  refuse(what, e, A, "condense: problem sizes must be positive", [](Case& c) { c.N = 0; c.batch = -1; }, true, nrhs);
  refuse(what, e, A, "condense: problem sizes must be positive", [](Case& c) { c.nc = 0; }, true, nrhs);
  refuse(what, e, A, "condense: negative batch", [](Case& c) { c.batch = -1; c.data.base[3] = nullptr; }, true, nrhs);
  refuse(what, e, A, "condense: null problem data block", [](Case& c) { c.data_p = nullptr; }, true, nrhs);
  refuse(what, e, A, "condense: null problem data pointer", [](Case& c) { c.data.base[FBSTAB_MPC_x0] = nullptr; }, true, nrhs);
  refuse(what, e, A, "condense: problem data stride smaller than the array length",
         [](Case& c) { c.data.stride[FBSTAB_MPC_q] = 1; }, true, nrhs);
  if (!with_device) return;
  refuse(what, e, DV, "condense: no such device", [](Case& c) { c.device = 5; c.h.device = 5; }, false, nrhs);
  refuse(what, e, DV, "condense: no such device", [](Case& c) { c.device = -1; c.h.device = -1; }, false, nrhs);
}
void refuse_images(const std::string& who, Entry e, int nrhs = 1) {
  refuse(who.c_str(), e, A, (who + ": null pointer in the condensed images").c_str(),
         [](Case& c) { c.dense.base[FBSTAB_DENSE_H] = nullptr; c.dense.stride[FBSTAB_DENSE_b] = 1; }, true, nrhs);
  refuse(who.c_str(), e, A, (who + ": stride of a condensed image smaller than the array length").c_str(),
         [](Case& c) { c.dense.stride[FBSTAB_DENSE_H] = 1; }, true, nrhs);
  refuse(who.c_str(), e, A, (who + ": stride of a condensed image smaller than the array length").c_str(),
         [](Case& c) { c.dense.stride[FBSTAB_DENSE_f] = 0; }, true, nrhs);
}
void refuse_handle(const std::string& who, Entry e, int nrhs = 1) {
  refuse(who.c_str(), e, A, (who + ": null dense solver handle").c_str(), [](Case& c) { c.hp = nullptr; }, true, nrhs);
  refuse(who.c_str(), e, A, (who + ": the dense handle is not one of ((N + 1) nu, 0, (N + 1) nc)").c_str(),
         [](Case& c) { c.h.var_len[1] = 1; c.h.max_batch = 1; }, true, nrhs);
  refuse(who.c_str(), e, A, (who + ": the dense handle is not one of ((N + 1) nu, 0, (N + 1) nc)").c_str(),
         [](Case& c) { c.h.var_len[2]++; }, true, nrhs);
  refuse(who.c_str(), e, A, (who + ": batch exceeds the max_batch the handle was created with").c_str(),
         [](Case& c) { c.h.max_batch = 1; }, true, nrhs);
}
void refuse_plant_and_map(const std::string& who, Entry e) {
  refuse(who.c_str(), e, A, (who + ": null plant matrix").c_str(), [](Case& c) { c.plant.B = nullptr; c.steps = -1; });
  refuse(who.c_str(), e, A, (who + ": negative step count").c_str(), [](Case& c) { c.steps = -1; c.mode = 7; });
  refuse(who.c_str(), e, A, (who + ": `mode` must be AFFINE (0) or RECONDENSE (1)").c_str(),
         [](Case& c) { c.mode = 2; c.traj_per_group = -1; });
  refuse(who.c_str(), e, A, (who + ": negative traj_per_group").c_str(),
         [](Case& c) { c.traj_per_group = -1; c.dense.base[0] = nullptr; });
  refuse(who.c_str(), e, A, (who + ": plant stride smaller than the matrix").c_str(), [](Case& c) { c.plant.stride_A = 3; });
  refuse(who.c_str(), e, A, (who + ": plant stride smaller than the matrix").c_str(),
         [](Case& c) { c.plant.stride_B = 1; c.map_p = nullptr; });
  refuse(who.c_str(), e, A, (who + ": AFFINE mode needs the map").c_str(), [](Case& c) { c.map_p = nullptr; c.hp = nullptr; });
  refuse(who.c_str(), e, A, (who + ": null pointer in the map").c_str(), [](Case& c) { c.map.f0 = nullptr; });
  refuse(who.c_str(), e, A, (who + ": stride of the map smaller than the array length").c_str(),
         [](Case& c) { c.map.stride_M = 5; });
  refuse(who.c_str(), e, A, (who + ": stride of the map smaller than the array length").c_str(),
         [](Case& c) { c.map.stride_b0 = 1; });
  refuse(who.c_str(), e, U, "condensed sweep: traj_per_group copies of a trajectory's vectors do not fit the 160 KiB LDS budget",
         [](Case& c) { c.traj_per_group = 100000; }, false);
}
const char* kLdsText = "condense: the stage images and dx/du of a horizon do not fit the 160 KiB LDS budget";
const char* kIntText = "condense: the condensed sizes do not fit an int";
void refuse_sizes() {
  auto none = [] { return fb_shim::state().calls; };
  const long calls = none();
  int a = 7, b = 7;
  long long l = 7, w = 7, wg = 7;
#define SIZES(call, code, text)                                                                              \
  do {                                                                                                       \
    g_error.clear(); a = b = 7; l = w = wg = 7;                                                              \
    const int rc_ = (call);                                                                                  \
    CHECK(rc_ == (code) && g_error == (text), "%d \"%s\", expected \"%s\"", rc_, g_error.c_str(), text);     \
    CHECK((a == 0 || (code) == U) && l == 0 && (w == 0 || w == 7) && (wg == 0 || wg == 7), "a refusal leaves zeros: %d %lld %lld", a, l, w); \
  } while (0)
  SIZES(condensed_sizes(0, 2, 1, 1, &a, &b, &l), A, "condense: problem sizes must be positive");
  SIZES(condensed_sizes(0x7ffffffe, 2, 2, 1, &a, &b, &l), U, kIntText);
  SIZES(condensed_sizes(2, 200, 1, 1, &a, &b, &l), U, kLdsText);
  SIZES(condensed_multi_sizes(2, 2, 0, 1, 0, -1, &a, &l, &w), A, "condensed multi: problem sizes must be positive");
  SIZES(condensed_multi_sizes(0x7ffffffe, 2, 2, 1, 0, -1, &a, &l, &w), A, "condensed multi: fewer than one right-hand side");
  SIZES(condensed_multi_sizes(0x7ffffffe, 2, 2, 1, 1, -1, &a, &l, &w), A, "condensed multi: negative rhs_per_group");
  SIZES(condensed_multi_sizes(0x7ffffffe, 2, 1, 2, 1, 0, &a, &l, &w), U, kIntText);
  SIZES(condensed_multi_sizes(2, 200, 1, 1, 1, 0, &a, &l, &w), U,
        "condensed multi: the stage images do not fit the 160 KiB LDS budget");
  SIZES(condensed_multi_sizes(50, 20, 1, 1, 20, 20, &a, &l, &w), U,
        "condensed multi: the stage images and rhs_per_group copies of a right-hand side's vectors do not fit the 160 KiB LDS budget");
  for (bool adj : {false, true}) {
    const std::string who = adj ? "condensed sweep adjoint" : "condensed sweep";
    long long* g = adj ? &wg : nullptr;
    SIZES(condensed_sweep_sizes(who.c_str(), 2, 0, 1, 1, -1, 0, &a, &l, &w, g, adj), A, (who + ": problem sizes must be positive").c_str());
    SIZES(condensed_sweep_sizes(who.c_str(), 0x7ffffffe, 2, 2, 1, -1, 0, &a, &l, &w, g, adj), A, (who + ": negative traj_per_group").c_str());
    SIZES(condensed_sweep_sizes(who.c_str(), 0x7ffffffe, 2, 2, 1, 0, 0, &a, &l, &w, g, adj), U, kIntText);
    SIZES(condensed_sweep_sizes(who.c_str(), 2, 2, 1, 1, 100000, 1, &a, &l, &w, g, adj), U,
          "condensed sweep: traj_per_group copies of a trajectory's vectors do not fit the 160 KiB LDS budget");
  }
#undef SIZES
  // and what they report where they do not refuse (include/fbstab_hip.h)
  OK(condensed_sizes(2, 3, 2, 1, &a, &b, &l));
  CHECK(a == 6 && b == 3 && l == condense_lds(2, 3, 2, 1), "condensed sizes %d %d %lld", a, b, l);
  OK(condensed_multi_sizes(2, 3, 2, 1, 3, 0, &a, &l, &w));
  CHECK(a == 3 && l == multi_lds(2, 3, 2, 1, 3) && w == 6 + 3 * (24 + 9), "condensed multi sizes %d %lld %lld", a, l, w);
  OK(condensed_sweep_sizes("condensed sweep", 2, 3, 2, 1, 2, 1, &a, &l, &w, nullptr, false));
  CHECK(a == 2 && l == sweep_lds(2, 3, 2, 1, 2, true) && w == 6 + 6 + 3 + 1, "condensed sweep sizes %d %lld %lld", a, l, w);
  OK(condensed_sweep_sizes("condensed sweep adjoint", 2, 3, 2, 1, 0, 0, &a, &l, &w, &wg, true));
  CHECK(a == 64 && l == sweep_lds(2, 3, 2, 1, 64, false) && w == 24 + 6 + 6 + 1 && wg == w + 30 + 9,
        "condensed sweep adjoint sizes %d %lld %lld %lld", a, l, w, wg);
  CHECK(none() == calls, "the sizes functions make no device call");
}

void refusals() {
  refuse_sizes();
  // condense
  refuse_common("condense", &Case::condense, true);
  refuse("condense", &Case::condense, A, "condense: `what` must be MATRICES (1), VECTORS (2) or ALL (3)",
         [](Case& c) { c.what = 0; c.dout.base[0] = nullptr; });
  refuse("condense", &Case::condense, A, "condense: `what` must be MATRICES (1), VECTORS (2) or ALL (3)", [](Case& c) { c.what = 4; });
  refuse("condense", &Case::condense, A, "condense: null output block", [](Case& c) { c.dout_p = nullptr; });
  refuse("condense", &Case::condense, A, "condense: null pointer in a selected output slot",
         [](Case& c) { c.dout.base[FBSTAB_DENSE_f] = nullptr; c.dout.stride[FBSTAB_DENSE_A] = 1; });
  refuse("condense", &Case::condense, A, "condense: output stride smaller than the array length", [](Case& c) { c.dout.stride[FBSTAB_DENSE_A] = 1; });
  refuse("condense", &Case::condense, A, "condense: output stride smaller than the array length", [](Case& c) { c.dout.stride[FBSTAB_DENSE_b] = 0; });
  refuse("condense", &Case::condense, A, "condense: output stride 0 needs stride 0 on every one of Q, R, S, A, B, E, L",
         [](Case& c) { c.dout.stride[FBSTAB_DENSE_H] = 0; });
  refuse("condense", &Case::condense, U, kLdsText, [](Case& c) { c.nx = 200; for (long long& s : c.data.stride) s = 0; for (long long& s : c.dout.stride) s = 1 << 30; }, false);
  // expand
  refuse_common("expand", &Case::expand, true);
  refuse("expand", &Case::expand, A, "expand: null variable block", [](Case& c) { c.x_p = nullptr; c.xc.base[0] = nullptr; });
  refuse("expand", &Case::expand, A, "expand: null U or v pointer", [](Case& c) { c.xc.base[2] = nullptr; c.xc.base[3] = nullptr; });
  refuse("expand", &Case::expand, A, "expand: y is wanted and the condensed y is null", [](Case& c) { c.xc.base[3] = nullptr; c.x.stride[0] = 1; });
  refuse("expand", &Case::expand, A, "expand: stride of the condensed point smaller than the vector length", [](Case& c) { c.xc.stride[0] = 1; });
  refuse("expand", &Case::expand, A, "expand: variable stride smaller than the vector length", [](Case& c) { c.x.stride[1] = 1; });
  // the condensed adjoint
  refuse_common("condensed adjoint", &Case::adjoint, true);
  refuse("condensed adjoint", &Case::adjoint, A, "condensed adjoint: null argument", [](Case& c) { c.status = nullptr; c.dense.base[0] = nullptr; });
  refuse_images("condensed adjoint", &Case::adjoint);
  refuse("condensed adjoint", &Case::adjoint, A, "condensed adjoint: null seed pointer (z)", [](Case& c) { c.seed.base[0] = nullptr; c.x.base[0] = nullptr; });
  refuse("condensed adjoint", &Case::adjoint, A, "condensed adjoint: null variable pointer", [](Case& c) { c.x.base[2] = nullptr; });
  refuse("condensed adjoint", &Case::adjoint, A, "condensed adjoint: variable stride smaller than the vector length", [](Case& c) { c.x.stride[0] = 1; c.seed.stride[0] = 1; });
  refuse("condensed adjoint", &Case::adjoint, A, "condensed adjoint: seed stride smaller than the vector length", [](Case& c) { c.seed.stride[1] = 0; });
  refuse("condensed adjoint", &Case::adjoint, A, "condensed adjoint: adjoint stride smaller than the vector length", [](Case& c) { c.adj.stride[2] = 1; c.grad.stride[0] = 0; });
  refuse("condensed adjoint", &Case::adjoint, A, "condensed adjoint: gradient stride smaller than the array length", [](Case& c) { c.grad.stride[0] = 0; c.hp = nullptr; });
  refuse_handle("condensed adjoint", &Case::adjoint);
  // many right-hand sides
  refuse_common("condensed kkt solve", &Case::kkt, false, 3);
  refuse("condensed kkt solve", &Case::kkt, A, "condensed kkt solve: fewer than one right-hand side", [](Case& c) { c.nrhs = 0; c.mseed.base[0] = nullptr; }, true, 3);
  refuse("condensed kkt solve", &Case::kkt, A, "condensed kkt solve: null seed or step block", [](Case& c) { c.mstep_p = nullptr; c.mseed.base[0] = nullptr; }, true, 3);
  refuse("condensed kkt solve", &Case::kkt, A, "condensed kkt solve: null seed pointer (z)", [](Case& c) { c.mseed.base[0] = nullptr; c.status = nullptr; }, true, 3);
  refuse("condensed kkt solve", &Case::kkt, A, "condensed multi: null argument", [](Case& c) { c.status = nullptr; c.dense.base[0] = nullptr; }, true, 3);
  refuse_images("condensed multi", &Case::kkt, 3);
  refuse("condensed kkt solve", &Case::kkt, A, "condensed multi: null variable pointer", [](Case& c) { c.x.base[1] = nullptr; }, true, 3);
  refuse("condensed kkt solve", &Case::kkt, A, "condensed multi: variable stride smaller than the vector length", [](Case& c) { c.x.stride[2] = 1; c.mseed.rhs_stride[0] = 1; }, true, 3);
  refuse("condensed kkt solve", &Case::kkt, A, "seed rhs_stride smaller than the vector length", [](Case& c) { c.mseed.rhs_stride[0] = 1; }, true, 3);
  refuse("condensed kkt solve", &Case::kkt, A, "seed stride smaller than the right-hand sides of one QP", [](Case& c) { c.mseed.stride[1] -= 3; }, true, 3);
  refuse("condensed kkt solve", &Case::kkt, A, "step rhs_stride smaller than the vector length", [](Case& c) { c.mstep.rhs_stride[2] = 1; }, true, 3);
  refuse("condensed kkt solve", &Case::kkt, A, "step stride smaller than the right-hand sides of one QP", [](Case& c) { c.mstep.stride[0] = 0; c.rhs_per_group = -1; }, true, 3);
  refuse("condensed kkt solve", &Case::kkt, A, "condensed multi: negative rhs_per_group", [](Case& c) { c.rhs_per_group = -1; c.hp = nullptr; }, true, 3);
  refuse_handle("condensed multi", &Case::kkt, 3);
  refuse("condensed kkt solve", &Case::kkt, DV, "condensed multi: no such device", [](Case& c) { c.h.device = 1; }, false, 3);
  refuse("condensed kkt solve", &Case::kkt, U, "condensed multi: the stage images do not fit the 160 KiB LDS budget",
         [](Case& c) { c.nx = 200; for (long long& s : c.data.stride) s = 0; for (int i = 0; i < 3; i++) { c.x.stride[i] = c.mseed.stride[i] = c.mstep.stride[i] = 1LL << 40; c.mseed.rhs_stride[i] = c.mstep.rhs_stride[i] = 1 << 20; } }, false, 3);
  refuse("condensed kkt solve", &Case::kkt, A, "condensed multi: batch x groups of right-hand sides exceeds the grid limit",
         [](Case& c) { c.batch = c.nrhs = c.h.max_batch = 70000; c.rhs_per_group = 1; for (int i = 0; i < 3; i++) c.mseed.stride[i] = c.mstep.stride[i] = 1LL << 40; }, false, 3);
  refuse_common("condensed x0 sensitivity", &Case::x0_sensitivity, false, 2);
  refuse("condensed x0 sensitivity", &Case::x0_sensitivity, A, "condensed x0 sensitivity: both step and gain are null",
         [](Case& c) { c.mstep_p = nullptr; c.gain = nullptr; c.status = nullptr; }, true, 2);
  refuse("condensed x0 sensitivity", &Case::x0_sensitivity, A, "condensed multi: gain stride smaller than nu x nx",
         [](Case& c) { c.gain_stride = 1; c.rhs_per_group = -1; }, true, 2);
  refuse_images("condensed multi", &Case::x0_sensitivity, 2);
  refuse_handle("condensed multi", &Case::x0_sensitivity, 2);
  // the x0 map
  refuse_common("condensed x0 map", &Case::x0_map, true);
  refuse("condensed x0 map", &Case::x0_map, A, "condensed x0 map: null output pointer", [](Case& c) { c.mapout = nullptr; c.map_stride = 1; });
  refuse("condensed x0 map", &Case::x0_map, A, "condensed x0 map: output stride smaller than the image", [](Case& c) { c.map_stride = 1; });
  refuse("condensed x0 map", &Case::x0_map, A, "condensed x0 map: output stride 0 needs stride 0 on every one of Q, R, S, A, B, E, L", [](Case& c) { c.map_stride = 0; });
  refuse("condensed x0 map", &Case::x0_map, A, "condensed x0 map: batch x column blocks exceeds the grid limit",
         [](Case& c) { c.batch = 1 << 30; c.nx = 3; for (long long& s : c.data.stride) s = 0; c.map_stride = 1 << 20; }, false);
  // the sweep
  refuse_common("condensed sweep", &Case::sweep, true);
  refuse("condensed sweep", &Case::sweep, A, "condensed sweep: null argument", [](Case& c) { c.out = nullptr; c.plant.A = nullptr; });
  refuse_plant_and_map("condensed sweep", &Case::sweep);
  refuse("condensed sweep", &Case::sweep, A, "condensed sweep: shift is 0 or 1", [](Case& c) { c.scen.shift = 2; c.mode = 5; });
  refuse("condensed sweep", &Case::sweep, A, "condensed sweep: every trajectory needs its own x0 (stride >= nx)",
         [](Case& c) { c.data.stride[FBSTAB_MPC_x0] = 0; c.dense.base[0] = nullptr; });
  refuse_images("condensed sweep", &Case::sweep);
  refuse("condensed sweep", &Case::sweep, A, "condensed sweep: null variable pointer", [](Case& c) { c.x.base[3] = nullptr; });
  refuse("condensed sweep", &Case::sweep, A, "condensed sweep: variable stride smaller than the vector length", [](Case& c) { c.x.stride[3] = 1; c.plant.stride_A = 1; });
  refuse_handle("condensed sweep", &Case::sweep);
  // its adjoint
  refuse_common("condensed sweep adjoint", &Case::sweep_adjoint, true);
  refuse("condensed sweep adjoint", &Case::sweep_adjoint, A, "condensed sweep adjoint: null argument", [](Case& c) { c.status = nullptr; c.plant.A = nullptr; });
  refuse_plant_and_map("condensed sweep adjoint", &Case::sweep_adjoint);
  refuse_images("condensed sweep adjoint", &Case::sweep_adjoint);
  refuse("condensed sweep adjoint", &Case::sweep_adjoint, A, "condensed sweep adjoint: the x, U, v and eflag logs are required",
         [](Case& c) { c.log.eflag = nullptr; c.grad.stride[0] = 0; });
  refuse("condensed sweep adjoint", &Case::sweep_adjoint, A,
         "condensed sweep adjoint: gradient stride smaller than the array length (sums over the batch are the caller's)",
         [](Case& c) { c.grad.stride[FBSTAB_MPC_x0] = 0; c.map_p = nullptr; });
  refuse_handle("condensed sweep adjoint", &Case::sweep_adjoint);
}

}  // namespace

int main(int argc, char** argv) {
  const std::string group = argc > 1 ? argv[1] : "";
  if (group == "placement") placement();
  else if (group == "carve") carve();
  else if (group == "sequence") sequence();
  else if (group == "refusals") refusals();
  else return 2;
  return g_failures ? 1 : 0;
}
