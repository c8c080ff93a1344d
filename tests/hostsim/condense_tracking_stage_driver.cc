// TEST INFRASTRUCTURE ONLY - the driver of tests/test_condense_tracking_cpu.py: the per-step references of
// fbstab_amd/csrc/fb_condense_stage.h (condensed_reference_images_run, condensed_tracking_sweep_run,
// condensed_tracking_sweep_adjoint_run) over the heap-backed runtime of runtime_shim/, a bare SolverBase, and host
// lambdas in the place of the kernels and of the dense handle's entry points, as condense_stage_driver.cc runs the
// calls without references.  Every buffer of the caller is allocated exactly as long as include/fbstab_hip.h says; a
// lambda records the pointers it was handed, reads every input double and writes every output double it is entitled
// to - so that under the address sanitizer a step offset or a stride that is off by one double ends the driver.  What
// is expected is restated here from include/fbstab_hip.h, not taken from the header under test.
//
// usage: condense_tracking_stage_driver <group>; prints one line per failed check and exits 1, prints nothing and
// exits 0 otherwise.
#include "fb_condense_stage.h"

#include <cstdio>
#include <cstring>
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

std::vector<std::unique_ptr<double[]>> g_doubles;
std::vector<std::unique_ptr<int[]>> g_ints;
std::vector<std::unique_ptr<fbstab_solver_out_t[]>> g_out;
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
void wri(int* p, long long n) { for (long long i = 0; i < n; i++) p[i] = 0; }
void rd_rows(const double* b, long long stride, long long len, int batch) {
  if (b) for (int q = 0; q < (stride == 0 ? 1 : batch); q++) rd(b + q * stride, len);
}
void wr_rows(double* b, long long stride, long long len, int batch) {
  if (b) for (int q = 0; q < (stride == 0 ? 1 : batch); q++) wr(b + q * stride, len);
}

constexpr long long kGarbage = 0x7777777;  // a caller's stride or step where the header says it is not read
constexpr int kGap = 3;
constexpr int kRefSeq[4] = {FBSTAB_MPC_q, FBSTAB_MPC_r, FBSTAB_MPC_c, FBSTAB_MPC_d};

template <class T>
T& arg(void** args, int i) { return *static_cast<T*>(args[i]); }

// What one launch was handed.
enum Kind { K_MATRICES, K_VECTORS, K_EXPAND, K_REFS, K_SWEEP_BEGIN, K_SWEEP_STEP, K_ADJ_BEGIN, K_ADJ_STEP, K_ADJ_FINISH,
            K_RESIDUAL, K_CORRECT, K_DENSE_SOLVE, K_DENSE_ADJOINT };
struct Ev {
  int kind, grid;
  long long lds;
  fbstab_mpc_batch_t a;               // the data block (VECTORS, EXPAND, REFS, ADJ_FINISH)
  fbstab_mpc_grad_batch_t g;          // the gradient block (ADJ_BEGIN, ADJ_FINISH)
  const double *f0, *b0;              // SWEEP_STEP, ADJ_STEP
  long long sf0, sb0;
  int affine, open;
  fbstab_condensed_refs_t rr;         // REFS
  fbstab_condensed_ref_images_t im;
  int steps, R;
  long long per;
};
bool same_launch(const Ev& x, const Ev& y) { return x.kind == y.kind && x.grid == y.grid && x.lds == y.lds; }

struct Sim {
  int N, nx, nu, nc, batch;
  long long nz, nv, nzf, nlf, len[FBSTAB_MPC_NSEQ];
  std::vector<Ev> ev;
  Sim(int N_, int nx_, int nu_, int nc_, int batch_) : N(N_), nx(nx_), nu(nu_), nc(nc_), batch(batch_) {
    const long long M = N + 1;
    nz = M * nu; nv = M * nc; nzf = M * (nx + nu); nlf = M * nx;
    const long long l[FBSTAB_MPC_NSEQ] = {M * nx * nx, M * nu * nu, M * nu * nx, M * nx, M * nu, (long long)N * nx * nx,
                                          (long long)N * nx * nu, (long long)N * nx, M * nc * nx, M * nc * nu, M * nc, nx};
    for (int i = 0; i < FBSTAB_MPC_NSEQ; i++) len[i] = l[i];
  }
  Ev& push(int kind, int grid, long long lds) {
    Ev e;
    std::memset(&e, 0, sizeof e);
    e.kind = kind; e.grid = grid; e.lds = lds;
    ev.push_back(e);
    return ev.back();
  }
  void rd_data(const fbstab_mpc_batch_t& d, bool x0) {
    for (int i = 0; i < FBSTAB_MPC_NSEQ; i++)
      if (x0 || i != FBSTAB_MPC_x0) rd_rows(d.base[i], d.stride[i], len[i], batch);
  }
  int launch(CondenseKernel id, int grid, long long lds, void** args, hipStream_t) {
    Ev& e = push(id == kCondenseMatrices ? K_MATRICES : id == kCondenseVectors ? K_VECTORS : K_EXPAND, grid, lds);
    e.a = arg<fbstab_mpc_batch_t>(args, 5);
    rd_data(e.a, true);
    if (id == kCondenseExpand) {
      const fbstab_var_batch_t in = arg<fbstab_var_batch_t>(args, 6), outv = arg<fbstab_var_batch_t>(args, 7);
      const long long cl[4] = {nz, 0, nv, nv}, xl[4] = {nzf, nlf, nv, nv};
      for (int i = 0; i < 4; i++) {
        rd_rows(in.base[i], in.stride[i], cl[i], batch);
        wr_rows(outv.base[i], outv.stride[i], xl[i], batch);
      }
    } else if (id == kCondenseVectors) {
      const fbstab_dense_out_batch_t out = arg<fbstab_dense_out_batch_t>(args, 6);
      wr_rows(out.base[FBSTAB_DENSE_f], out.stride[FBSTAB_DENSE_f], nz, batch);
      wr_rows(out.base[FBSTAB_DENSE_b], out.stride[FBSTAB_DENSE_b], nv, batch);
    }
    return FBSTAB_HIP_OK;
  }
  int launch(CondenseRefsKernel, int grid, long long lds, void** args, hipStream_t) {
    Ev& e = push(K_REFS, grid, lds);
    e.steps = arg<int>(args, 5); e.R = arg<int>(args, 6); e.per = arg<long long>(args, 7);
    e.a = arg<fbstab_mpc_batch_t>(args, 8);
    e.rr = arg<fbstab_condensed_refs_t>(args, 9);
    e.im = arg<fbstab_condensed_ref_images_t>(args, 10);
    for (int i : {FBSTAB_MPC_Q, FBSTAB_MPC_R, FBSTAB_MPC_S, FBSTAB_MPC_A, FBSTAB_MPC_B, FBSTAB_MPC_E, FBSTAB_MPC_L})
      rd_rows(e.a.base[i], e.a.stride[i], len[i], batch);
    for (int k = 0; k < e.steps; k++)
      for (int q = 0; q < batch; q++) {
        for (int i = 0; i < 4; i++) rd(e.rr.base[i] + k * e.rr.step[i] + q * e.rr.stride[i], len[kRefSeq[i]]);
        wr(e.im.f0 + k * e.im.step_f0 + q * e.im.stride_f0, nz);
        wr(e.im.b0 + k * e.im.step_b0 + q * e.im.stride_b0, nv);
      }
    return FBSTAB_HIP_OK;
  }
  int launch(CondenseSweepKernel id, int grid, long long lds, void** args, hipStream_t) {
    if (id == kCondenseSweepBegin) { push(K_SWEEP_BEGIN, grid, lds); return FBSTAB_HIP_OK; }
    Ev& e = push(K_SWEEP_STEP, grid, lds);
    const CondenseSweepStep st = arg<CondenseSweepStep>(args, 0);
    e.f0 = st.f0; e.b0 = st.b0; e.sf0 = st.sf0; e.sb0 = st.sb0; e.affine = st.affine;
    if (st.affine) {
      rd_rows(st.M, st.sM, (nz + nv) * nx, batch); rd_rows(st.f0, st.sf0, nz, batch); rd_rows(st.b0, st.sb0, nv, batch);
      wr_rows(st.f, st.sf, nz, batch); wr_rows(st.b, st.sb, nv, batch);
    }
    return FBSTAB_HIP_OK;
  }
  int launch(CondenseSweepAdjKernel id, int grid, long long lds, void** args, hipStream_t) {
    if (id == kCondenseSweepAdjBegin) {
      Ev& e = push(K_ADJ_BEGIN, grid, lds);
      e.g = arg<fbstab_mpc_grad_batch_t>(args, 4);
      for (int i = 0; i < FBSTAB_MPC_NSEQ; i++) wr_rows(e.g.base[i], e.g.stride[i], len[i], batch);
      wri(arg<int*>(args, 8), batch);
    } else if (id == kCondenseSweepAdjStep) {
      Ev& e = push(K_ADJ_STEP, grid, lds);
      const CondenseSweepAdjStep s = arg<CondenseSweepAdjStep>(args, 0);
      e.f0 = s.f0; e.b0 = s.b0; e.sf0 = s.sf0; e.sb0 = s.sb0; e.affine = s.affine; e.open = s.open;
      CHECK(!s.gf0 && !s.gb0, "the tracked adjoint has no gf0 / gb0");
      if (s.affine && s.open) {
        rd_rows(s.f0, s.sf0, nz, batch); rd_rows(s.b0, s.sb0, nv, batch);
        wr_rows(s.f, s.sf, nz, batch); wr_rows(s.b, s.sb, nv, batch);
      }
    } else {
      Ev& e = push(K_ADJ_FINISH, grid, lds);
      e.a = arg<fbstab_mpc_batch_t>(args, 5);
      rd_data(e.a, false);
      e.g = arg<fbstab_mpc_grad_batch_t>(args, 7);
      for (int i = 0; i < FBSTAB_MPC_NSEQ; i++) wr_rows(e.g.base[i], e.g.stride[i], len[i], batch);
    }
    return FBSTAB_HIP_OK;
  }
  int launch(CondenseAdjointKernel id, int grid, long long lds, void**, hipStream_t) {
    push(id == kCondenseAdjResidual ? K_RESIDUAL : K_CORRECT, grid, lds);
    return FBSTAB_HIP_OK;
  }
  int launch(CondenseMultiKernel, int, long long, void**, hipStream_t) { return FBSTAB_HIP_ERR_ARGUMENT; }
  int launch(CondenseTangentKernel, int, long long, void**, hipStream_t) { return FBSTAB_HIP_ERR_ARGUMENT; }
  int solve(int b, const fbstab_dense_batch_t* d, const fbstab_var_batch_t*, fbstab_solver_out_t*, hipStream_t) {
    push(K_DENSE_SOLVE, b, 0);
    rd_rows(d->base[FBSTAB_DENSE_f], d->stride[FBSTAB_DENSE_f], nz, batch);
    rd_rows(d->base[FBSTAB_DENSE_b], d->stride[FBSTAB_DENSE_b], nv, batch);
    return FBSTAB_HIP_OK;
  }
  int adjoint(int b, const fbstab_dense_batch_t* d, const fbstab_var_batch_t*, const fbstab_var_batch_t*, double,
              const fbstab_var_batch_t*, int*, hipStream_t) {
    push(K_DENSE_ADJOINT, b, 0);
    rd_rows(d->base[FBSTAB_DENSE_f], d->stride[FBSTAB_DENSE_f], nz, batch);
    rd_rows(d->base[FBSTAB_DENSE_b], d->stride[FBSTAB_DENSE_b], nv, batch);
    return FBSTAB_HIP_OK;
  }
};

// A caller: valid arguments of all three calls in buffers of exactly the documented length.  The references: q moves in
// rows of its own ([steps][batch] with gaps), r has no slot (NULL: `data`'s at every step), c is one row per step for
// the whole batch (stride 0), and d is a window that slides by nc over one array shared by the batch.
struct Case {
  int N = 3, nx = 4, nu = 2, nc = 3, batch, steps, mode;
  Sim sim;
  SolverBase h;
  fbstab_mpc_batch_t data = {};
  fbstab_dense_batch_t dense = {};
  fbstab_var_batch_t x = {};
  fbstab_mpc_grad_batch_t grad = {};
  fbstab_condensed_map_t map = {};
  fbstab_receding_plant_t plant = {};
  fbstab_sweep_scenario_t scen = {};
  fbstab_condensed_sweep_log_t log = {};
  fbstab_condensed_refs_t refs = {};
  fbstab_condensed_ref_images_t im = {};
  fbstab_condensed_ref_grad_t rg = {};
  fbstab_solver_out_t* out;
  double *gu, *gx, *mu_log, *work = nullptr;
  int* status;
  const fbstab_condensed_refs_t* refs_p = &refs;
  const fbstab_condensed_ref_images_t* im_p = &im;
  const fbstab_condensed_ref_grad_t* rg_p = &rg;
  int refs_per_group = 0;

  double* blk(long long n, long long* stride, bool share = false) {
    if (batch <= 1) { *stride = kGarbage; return D(n); }
    if (share) { *stride = 0; return D(n); }
    *stride = n + kGap;
    return D((batch - 1) * *stride + n);
  }
  // [steps][batch] rows of n doubles with gaps: *step doubles between steps, *stride between trajectories
  double* rows(long long n, long long* step, long long* stride) {
    const long long st = n + kGap, sp = batch * st + 1;
    *stride = batch > 1 ? st : kGarbage;
    *step = steps > 1 ? sp : kGarbage;
    return D((steps - 1) * (steps > 1 ? sp : 0) + (batch - 1) * (batch > 1 ? st : 0) + n);
  }
  Case(int batch_, int steps_, int mode_) : batch(batch_), steps(steps_), mode(mode_), sim(3, 4, 2, 3, batch_) {
    const long long nz = sim.nz, nv = sim.nv, B = batch, S = steps;
    h.max_batch = 3; h.device = 0;
    h.var_len[0] = nz; h.var_len[1] = 0; h.var_len[2] = h.var_len[3] = nv;
    for (int i = 0; i < FBSTAB_MPC_NSEQ; i++) {
      data.base[i] = blk(sim.len[i], &data.stride[i]);
      grad.base[i] = blk(sim.len[i], &grad.stride[i]);
    }
    const long long dl[FBSTAB_DENSE_NARR] = {nz * nz, nz, 0, 0, nv * nz, nv};
    for (int i : {FBSTAB_DENSE_H, FBSTAB_DENSE_f, FBSTAB_DENSE_A, FBSTAB_DENSE_b}) dense.base[i] = blk(dl[i], &dense.stride[i]);
    const long long xl[4] = {sim.nzf, sim.nlf, nv, nv};
    for (int i = 0; i < 4; i++) x.base[i] = blk(xl[i], &x.stride[i]);
    map.M = blk((nz + nv) * nx, &map.stride_M);
    map.f0 = blk(nz, &map.stride_f0);
    map.b0 = blk(nv, &map.stride_b0);
    plant.A = blk((long long)nx * nx, &plant.stride_A);
    plant.B = blk((long long)nx * nu, &plant.stride_B);
    scen.w = D(S * B * nx); scen.shift = 1;
    log.u = D(S * B * nu); log.x = D(S * B * nx); log.U = D(S * B * nz); log.v = D(S * B * nv);
    log.eflag = I(S * B); log.newton = I(S * B);
    gu = D(S * B * nu); gx = D(S * B * nx); mu_log = D(S * B * nx);
    status = I(B);
    g_out.emplace_back(new fbstab_solver_out_t[(size_t)B]());
    out = g_out.back().get();
    // the references
    refs.base[0] = rows(sim.len[FBSTAB_MPC_q], &refs.step[0], &refs.stride[0]);
    refs.base[1] = nullptr; refs.step[1] = -5; refs.stride[1] = -5;       // (a NULL slot's numbers are not looked at)
    refs.base[2] = D((S - 1) * (sim.len[FBSTAB_MPC_c] + 1) + sim.len[FBSTAB_MPC_c]);
    refs.step[2] = steps > 1 ? sim.len[FBSTAB_MPC_c] + 1 : kGarbage; refs.stride[2] = batch > 1 ? 0 : kGarbage;
    refs.base[3] = D((S - 1) * nc + sim.len[FBSTAB_MPC_d]);
    refs.step[3] = steps > 1 ? nc : kGarbage; refs.stride[3] = batch > 1 ? 0 : kGarbage;
    im.f0 = rows(nz, &im.step_f0, &im.stride_f0);
    im.b0 = rows(nv, &im.step_b0, &im.stride_b0);
    rg.base[0] = rows(sim.len[FBSTAB_MPC_q], &rg.step[0], &rg.stride[0]);
    rg.base[3] = rows(sim.len[FBSTAB_MPC_d], &rg.step[3], &rg.stride[3]);
    grad.base[FBSTAB_MPC_q] = grad.base[FBSTAB_MPC_c] = grad.base[FBSTAB_MPC_d] = nullptr;   // (they move)
  }
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
  int images() {
    return condensed_reference_images_run(N, nx, nu, nc, batch, steps, &data, refs_p, im_p, refs_per_group, 0, nullptr,
                                          launcher());
  }
  int sweep() {
    long long per = 0;
    condensed_sweep_sizes("condensed sweep", N, nx, nu, nc, 0, 0, nullptr, nullptr, &per, nullptr, false);
    if (!work) work = D(per * batch);
    return condensed_tracking_sweep_run(&h, N, nx, nu, nc, batch, &data, &dense, &map, &x, out, &plant, steps, 1, &scen,
                                        mode, &log, refs_p, im_p, 0, work, nullptr, launcher(), dense_solve());
  }
  int sweep_plain() {
    long long per = 0;
    condensed_sweep_sizes("condensed sweep", N, nx, nu, nc, 0, 0, nullptr, nullptr, &per, nullptr, false);
    if (!work) work = D(per * batch);
    return condensed_sweep_run(&h, N, nx, nu, nc, batch, &data, &dense, &map, &x, out, &plant, steps, 1, &scen, mode, &log,
                               0, work, nullptr, launcher(), dense_solve());
  }
  int adjoint() {
    long long per = 0, per_grad = 0;
    condensed_sweep_sizes("condensed sweep adjoint", N, nx, nu, nc, 0, 0, nullptr, nullptr, &per, &per_grad, true);
    if (!work) work = D(per_grad * batch);
    return condensed_tracking_sweep_adjoint_run(&h, N, nx, nu, nc, batch, &data, &dense, &map, &plant, steps, &log, gu, gx,
                                                0.0, &grad, nullptr, nullptr, mu_log, status, mode, refs_p, im_p, rg_p, 0,
                                                work, nullptr, launcher(), dense_adjoint());
  }
  int adjoint_plain() {
    long long per = 0, per_grad = 0;
    condensed_sweep_sizes("condensed sweep adjoint", N, nx, nu, nc, 0, 0, nullptr, nullptr, &per, &per_grad, true);
    if (!work) work = D(per_grad * batch);
    return condensed_sweep_adjoint_run(&h, N, nx, nu, nc, batch, &data, &dense, &map, &plant, steps, &log, gu, gx, 0.0,
                                       &grad, nullptr, nullptr, mu_log, status, mode, 0, work, nullptr, launcher(),
                                       dense_adjoint());
  }

  // what the header says step k's sequences are: slot i of the data block a launch received
  void check_step_data(const fbstab_mpc_batch_t& a, int k, const char* what) {
    const bool one = batch == 1;
    CHECK(a.base[FBSTAB_MPC_q] == refs.base[0] + (steps > 1 ? k * refs.step[0] : 0), "%s of step %d: q", what, k);
    CHECK(one || a.stride[FBSTAB_MPC_q] == refs.stride[0], "%s of step %d: q stride", what, k);
    CHECK(a.base[FBSTAB_MPC_r] == data.base[FBSTAB_MPC_r], "%s of step %d: r is the data's", what, k);
    CHECK(one || a.stride[FBSTAB_MPC_r] == data.stride[FBSTAB_MPC_r], "%s of step %d: r stride", what, k);
    CHECK(a.base[FBSTAB_MPC_c] == refs.base[2] + (steps > 1 ? k * refs.step[2] : 0), "%s of step %d: c", what, k);
    CHECK(a.stride[FBSTAB_MPC_c] == 0, "%s of step %d: c is shared", what, k);
    CHECK(a.base[FBSTAB_MPC_d] == refs.base[3] + (steps > 1 ? (long long)k * nc : 0), "%s of step %d: d slides by nc", what, k);
    CHECK(a.stride[FBSTAB_MPC_d] == 0, "%s of step %d: d is shared", what, k);
    for (int i : {FBSTAB_MPC_Q, FBSTAB_MPC_R, FBSTAB_MPC_S, FBSTAB_MPC_A, FBSTAB_MPC_B, FBSTAB_MPC_E, FBSTAB_MPC_L})
      CHECK(a.base[i] == data.base[i], "%s of step %d: matrix sequence %d", what, k, i);
  }
  std::vector<Ev> of(int kind) {
    std::vector<Ev> r;
    for (const Ev& e : sim.ev)
      if (e.kind == kind) r.push_back(e);
    return r;
  }
};

// ---- the images call ------------------------------------------------------------------------------------------------------
void group_images() {
  for (int batch : {3, 1})
    for (int steps : {5, 1})
      for (int rpg : {0, 2}) {
        Case c(batch, steps, 0);
        c.refs_per_group = rpg;
        CHECK(c.images() == FBSTAB_HIP_OK, "%s", g_error.c_str());
        CHECK(c.sim.ev.size() == 1 && c.sim.ev[0].kind == K_REFS, "one launch");
        if (c.sim.ev.size() != 1) continue;
        const Ev& e = c.sim.ev[0];
        // the rule: clamp(256 / nx, 1, steps) (80 KB is far away at this shape)
        const int R = rpg ? (rpg < steps ? rpg : steps) : (steps < 64 ? steps : 64);
        auto even = [](long long n) { return n + (n & 1); };
        const long long per = even(4LL * c.nx) + 2 * even(c.nx);
        CondenseLds o;
        o.init(c.N, c.nx, c.nu, c.nc);
        CHECK(e.R == R && e.steps == steps && e.per == per, "R %d steps %d per %lld", e.R, e.steps, e.per);
        CHECK(e.grid == batch * ((steps + R - 1) / R), "grid %d", e.grid);
        CHECK(e.lds == 8 * (o.carry + R * per), "lds %lld", e.lds);
        fbstab_mpc_batch_t a0 = e.a;   // the block of step 0 from the references as the kernel received them
        for (int i = 0; i < 4; i++) { a0.base[kRefSeq[i]] = e.rr.base[i]; a0.stride[kRefSeq[i]] = e.rr.stride[i]; }
        c.check_step_data(a0, 0, "the launch");
        CHECK(e.rr.step[1] == 0, "a NULL slot does not move");
        if (steps > 1) {
          CHECK(e.rr.step[0] == c.refs.step[0] && e.rr.step[2] == c.refs.step[2] && e.rr.step[3] == c.nc, "steps");
          CHECK(e.im.step_f0 == c.im.step_f0 && e.im.step_b0 == c.im.step_b0, "image steps");
        }
        if (batch > 1) CHECK(e.im.stride_f0 == c.im.stride_f0 && e.im.stride_b0 == c.im.stride_b0, "image strides");
        CHECK(e.im.f0 == c.im.f0 && e.im.b0 == c.im.b0, "image bases");
      }
  // nothing to do queues nothing
  Case z(3, 4, 0);
  z.steps = 0;
  CHECK(z.images() == FBSTAB_HIP_OK && z.sim.ev.empty(), "steps == 0");
}

// ---- the tracked sweep ------------------------------------------------------------------------------------------------------
void group_sweep() {
  for (int batch : {3, 1})
    for (int mode : {FBSTAB_CONDENSED_SWEEP_AFFINE, FBSTAB_CONDENSED_SWEEP_RECONDENSE}) {
      const int steps = 4;
      Case c(batch, steps, mode), plain(batch, steps, mode);
      CHECK(c.sweep() == FBSTAB_HIP_OK, "%s", g_error.c_str());
      CHECK(plain.sweep_plain() == FBSTAB_HIP_OK, "%s", g_error.c_str());
      // the launches and their order are those of the call without references
      CHECK(c.sim.ev.size() == plain.sim.ev.size(), "%zu launches, %zu without references", c.sim.ev.size(), plain.sim.ev.size());
      for (size_t i = 0; i < c.sim.ev.size() && i < plain.sim.ev.size(); i++)
        CHECK(same_launch(c.sim.ev[i], plain.sim.ev[i]), "launch %zu", i);
      const std::vector<Ev> st = c.of(K_SWEEP_STEP), vec = c.of(K_VECTORS), ex = c.of(K_EXPAND);
      CHECK((int)st.size() == steps && ex.size() == 1, "steps and the expand");
      if (mode == FBSTAB_CONDENSED_SWEEP_AFFINE) {
        CHECK(vec.empty(), "no VECTORS launch in AFFINE mode");
        for (int k = 0; k < (int)st.size(); k++) {
          CHECK(st[k].affine == (k + 1 < steps), "step %d: affine", k);
          if (k + 1 == steps) continue;
          CHECK(st[k].f0 == c.im.f0 + (k + 1) * c.im.step_f0 && st[k].b0 == c.im.b0 + (k + 1) * c.im.step_b0,
                "step %d forms the vectors of step %d from its images", k, k + 1);
          CHECK(batch == 1 || (st[k].sf0 == c.im.stride_f0 && st[k].sb0 == c.im.stride_b0), "step %d: image strides", k);
          CHECK(st[k].f0 != c.map.f0 && st[k].b0 != c.map.b0, "the map's f0, b0 are not looked at");
        }
      } else {
        CHECK((int)vec.size() == steps - 1, "%zu VECTORS launches", vec.size());
        for (int k = 0; k < (int)vec.size(); k++) {
          c.check_step_data(vec[k].a, k + 1, "the VECTORS launch");
          CHECK(vec[k].a.base[FBSTAB_MPC_x0] == c.data.base[FBSTAB_MPC_x0], "VECTORS launch %d: x0 in place", k);
        }
      }
      if (ex.size() == 1) {
        c.check_step_data(ex[0].a, steps - 1, "the expand");
        CHECK(ex[0].a.base[FBSTAB_MPC_x0] != c.data.base[FBSTAB_MPC_x0] && ex[0].a.stride[FBSTAB_MPC_x0] == c.nx,
              "the expand reads the kept state");
      }
    }
}

// ---- the tracked adjoint ------------------------------------------------------------------------------------------------------
void group_adjoint() {
  for (int batch : {3, 1})
    for (int mode : {FBSTAB_CONDENSED_SWEEP_AFFINE, FBSTAB_CONDENSED_SWEEP_RECONDENSE}) {
      const int steps = 4;
      Case c(batch, steps, mode);
      CHECK(c.adjoint() == FBSTAB_HIP_OK, "%s", g_error.c_str());
      const bool one = batch == 1;
      const std::vector<Ev> bg = c.of(K_ADJ_BEGIN), st = c.of(K_ADJ_STEP), vec = c.of(K_VECTORS), fin = c.of(K_ADJ_FINISH);
      // one begin launch for the sums, then one per step for the rows of the per-step gradients - all in front
      CHECK((int)bg.size() == 1 + steps, "%zu begin launches", bg.size());
      for (size_t i = 0; i < bg.size() && i < c.sim.ev.size(); i++) CHECK(c.sim.ev[i].kind == K_ADJ_BEGIN, "begin launches come first");
      if ((int)bg.size() == 1 + steps) {
        for (int i : {FBSTAB_MPC_q, FBSTAB_MPC_c, FBSTAB_MPC_d}) CHECK(!bg[0].g.base[i], "no summed slot of a sequence that moves");
        CHECK(bg[0].g.base[FBSTAB_MPC_r] == c.grad.base[FBSTAB_MPC_r] && bg[0].g.base[FBSTAB_MPC_Q] == c.grad.base[FBSTAB_MPC_Q], "the sums");
        for (int k = 0; k < steps; k++) {
          const fbstab_mpc_grad_batch_t& g = bg[1 + k].g;
          CHECK(g.base[FBSTAB_MPC_q] == c.rg.base[0] + k * c.rg.step[0] && g.base[FBSTAB_MPC_d] == c.rg.base[3] + k * c.rg.step[3],
                "begin launch of step %d zeroes its rows", k);
          CHECK(one || (g.stride[FBSTAB_MPC_q] == c.rg.stride[0] && g.stride[FBSTAB_MPC_d] == c.rg.stride[3]), "rows of step %d: strides", k);
          for (int i = 0; i < FBSTAB_MPC_NSEQ; i++)
            if (i != FBSTAB_MPC_q && i != FBSTAB_MPC_d) CHECK(!g.base[i], "begin launch of step %d: slot %d", k, i);
        }
      }
      // steps + 1 step launches, last step first; the launch that opens step k reads the images of step k
      CHECK((int)st.size() == steps + 1, "%zu step launches", st.size());
      if (mode == FBSTAB_CONDENSED_SWEEP_AFFINE)
        for (int j = 0; j < (int)st.size() && j < steps; j++) {
          const int k = steps - 1 - j;
          CHECK(st[j].open && st[j].f0 == c.im.f0 + k * c.im.step_f0 && st[j].b0 == c.im.b0 + k * c.im.step_b0,
                "opening step %d uses its images", k);
          CHECK(one || (st[j].sf0 == c.im.stride_f0 && st[j].sb0 == c.im.stride_b0), "opening step %d: image strides", k);
        }
      CHECK((int)vec.size() == (mode == FBSTAB_CONDENSED_SWEEP_AFFINE ? 0 : steps), "%zu VECTORS launches", vec.size());
      for (int j = 0; j < (int)vec.size(); j++) {
        const int k = steps - 1 - j;
        c.check_step_data(vec[j].a, k, "the VECTORS launch");
        CHECK(vec[j].a.base[FBSTAB_MPC_x0] == c.log.x + (long long)k * batch * c.nx, "VECTORS launch of step %d: x0 is x_log[k]", k);
      }
      CHECK((int)fin.size() == steps, "%zu finish launches", fin.size());
      for (int j = 0; j < (int)fin.size(); j++) {
        const int k = steps - 1 - j;
        c.check_step_data(fin[j].a, k, "the finish kernel");
        const fbstab_mpc_grad_batch_t& g = fin[j].g;
        CHECK(g.base[FBSTAB_MPC_q] == c.rg.base[0] + k * c.rg.step[0] && g.base[FBSTAB_MPC_d] == c.rg.base[3] + k * c.rg.step[3],
              "the finish kernel of step %d writes its rows", k);
        CHECK(!g.base[FBSTAB_MPC_c] && !g.base[FBSTAB_MPC_x0], "step %d: c is not wanted, x0 is the step kernel's", k);
        CHECK(g.base[FBSTAB_MPC_r] == c.grad.base[FBSTAB_MPC_r] && g.base[FBSTAB_MPC_E] == c.grad.base[FBSTAB_MPC_E], "step %d: the sums", k);
      }
    }
}

// ---- refusals: FBSTAB_HIP_ERR_ARGUMENT, nothing queued ----------------------------------------------------------------------
template <class F>
void refuse(const char* what, int mode, F breaker, int which) {
  Case c(3, 4, mode);
  breaker(c);
  const int rc = which == 0 ? c.images() : which == 1 ? c.sweep() : c.adjoint();
  CHECK(rc == FBSTAB_HIP_ERR_ARGUMENT && c.sim.ev.empty(), "%s: rc %d, %zu launches", what, rc, c.sim.ev.size());
}
void group_refusals() {
  const int AFF = FBSTAB_CONDENSED_SWEEP_AFFINE, REC = FBSTAB_CONDENSED_SWEEP_RECONDENSE;
  for (int which : {0, 1, 2}) {
    refuse("negative step", REC, [](Case& c) { c.refs.step[0] = -1; }, which);
    refuse("negative stride", REC, [](Case& c) { c.refs.stride[2] = -1; }, which);
    refuse("stride below the length", REC, [](Case& c) { c.refs.stride[0] = c.sim.len[FBSTAB_MPC_q] - 1; }, which);
  }
  for (int which : {1, 2}) {
    refuse("NULL images in AFFINE mode", AFF, [](Case& c) { c.im_p = nullptr; }, which);
    refuse("NULL f0", AFF, [](Case& c) { c.im.f0 = nullptr; }, which);
    refuse("negative image step", AFF, [](Case& c) { c.im.step_b0 = -1; }, which);
    refuse("image stride below the length", AFF, [](Case& c) { c.im.stride_f0 = c.sim.nz - 1; }, which);
    refuse("NULL map", AFF, [](Case& c) { c.map.M = nullptr; }, which);
    // the references are checked in front of the handle
    Case c(3, 4, REC);
    c.refs.step[3] = -2;
    c.h.var_len[0] = 1;
    const int rc = which == 1 ? c.sweep() : c.adjoint();
    CHECK(rc == FBSTAB_HIP_ERR_ARGUMENT && g_error.find("references") != std::string::npos, "%s", g_error.c_str());
    // ... and RECONDENSE mode does not look at the images
    Case r(3, 4, REC);
    r.im_p = nullptr;
    CHECK((which == 1 ? r.sweep() : r.adjoint()) == FBSTAB_HIP_OK, "%s", g_error.c_str());
  }
  refuse("output step below the length", AFF, [](Case& c) { c.im.step_f0 = c.sim.nz - 1; }, 0);
  refuse("output stride 0", AFF, [](Case& c) { c.im.stride_b0 = 0; }, 0);
  refuse("NULL output", AFF, [](Case& c) { c.im.b0 = nullptr; }, 0);
  refuse("negative refs_per_group", AFF, [](Case& c) { c.refs_per_group = -1; }, 0);
  refuse("summed slot of a sequence that moves", AFF, [](Case& c) { c.grad.base[FBSTAB_MPC_q] = D(c.sim.len[FBSTAB_MPC_q] * 4); c.grad.stride[FBSTAB_MPC_q] = c.sim.len[FBSTAB_MPC_q]; }, 2);
  refuse("per-step gradient of a sequence that does not move", AFF, [](Case& c) { c.rg.base[1] = c.rg.base[0]; c.rg.step[1] = c.rg.step[0]; c.rg.stride[1] = c.rg.stride[0]; }, 2);
  refuse("per-step gradient step 0", AFF, [](Case& c) { c.rg.step[0] = 0; }, 2);
  refuse("per-step gradient stride 0", AFF, [](Case& c) { c.rg.stride[3] = 0; }, 2);
}

// ---- refs == NULL: exactly the existing calls ---------------------------------------------------------------------------------
void group_no_refs() {
  for (int mode : {FBSTAB_CONDENSED_SWEEP_AFFINE, FBSTAB_CONDENSED_SWEEP_RECONDENSE})
    for (int which : {1, 2}) {
      Case c(3, 4, mode), plain(3, 4, mode);
      for (Case* p : {&c, &plain})   // (what the existing adjoint takes: every summed slot)
        for (int i : {FBSTAB_MPC_q, FBSTAB_MPC_c, FBSTAB_MPC_d}) p->grad.base[i] = D((p->batch - 1) * p->grad.stride[i] + p->sim.len[i]);
      c.refs_p = nullptr; c.im_p = nullptr; c.rg_p = nullptr;
      CHECK((which == 1 ? c.sweep() : c.adjoint()) == FBSTAB_HIP_OK, "%s", g_error.c_str());
      CHECK((which == 1 ? plain.sweep_plain() : plain.adjoint_plain()) == FBSTAB_HIP_OK, "%s", g_error.c_str());
      CHECK(c.sim.ev.size() == plain.sim.ev.size(), "%zu launches, %zu from the existing call", c.sim.ev.size(), plain.sim.ev.size());
      for (size_t i = 0; i < c.sim.ev.size() && i < plain.sim.ev.size(); i++) {
        const Ev &e = c.sim.ev[i], &w = plain.sim.ev[i];
        CHECK(same_launch(e, w), "launch %zu", i);
        // the same pointers, relative to each caller's own buffers
        if (e.kind == K_SWEEP_STEP || e.kind == K_ADJ_STEP)
          CHECK((e.f0 == nullptr) == (w.f0 == nullptr) && (!e.f0 || (e.f0 == c.map.f0 && w.f0 == plain.map.f0 && e.b0 == c.map.b0)),
                "launch %zu: the map's f0, b0", i);
        if (e.kind == K_VECTORS || e.kind == K_EXPAND || e.kind == K_ADJ_FINISH)
          for (int s : {FBSTAB_MPC_q, FBSTAB_MPC_r, FBSTAB_MPC_c, FBSTAB_MPC_d})
            CHECK(e.a.base[s] == c.data.base[s] && e.a.stride[s] == c.data.stride[s], "launch %zu: the data's sequence %d", i, s);
        if (e.kind == K_ADJ_BEGIN || e.kind == K_ADJ_FINISH)
          for (int s = 0; s < FBSTAB_MPC_NSEQ; s++)
            CHECK((e.g.base[s] == nullptr) == (w.g.base[s] == nullptr) && (!e.g.base[s] || e.g.base[s] == c.grad.base[s]), "launch %zu: gradient slot %d", i, s);
      }
    }
}

}  // namespace

int main(int argc, char** argv) {
  const std::string group = argc > 1 ? argv[1] : "";
  if (group == "images") group_images();
  else if (group == "sweep") group_sweep();
  else if (group == "adjoint") group_adjoint();
  else if (group == "refusals") group_refusals();
  else if (group == "no_refs") group_no_refs();
  else return 2;
  return g_failures ? 1 : 0;
}
