// TEST INFRASTRUCTURE ONLY - the driver of tests/test_condense_tangent_cpu.py: condensed_tangent_run of
// fbstab_amd/csrc/fb_condense_stage.h over the heap-backed runtime of runtime_shim/, a bare SolverBase with the lengths
// fbstab_hip_dense_create sets, and host lambdas in the place of the direction kernel, of the adjoint's kernels and of
// the dense handle's adjoint.  As condense_stage_driver.cc: every buffer of the caller is allocated exactly as long as
// include/fbstab_hip.h says, a lambda reads every input double and writes every output double it is entitled to through
// the bases and strides it was given, so that under the address sanitizer a stride that should not have been read, a
// seed tail that starts one double early or a work array that is addressed where the caller gave rhs ends the driver.
// The expected blocks, the sequence and the refusal texts are restated here from include/fbstab_hip.h.
//
// usage: condense_tangent_stage_driver <group>; prints one line per failed check and exits 1, prints nothing and
// exits 0 otherwise.
#include "fb_condense_stage.h"

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
#define OK(call) do { const int rc_ = (call); CHECK(rc_ == FBSTAB_HIP_OK, "%s", g_error.c_str()); } while (0)

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
// rows of a block: QP q at base + q * stride; stride 0: one row for all
void rd_rows(const double* b, long long stride, long long len, int batch) {
  if (b) for (int q = 0; q < (stride == 0 ? 1 : batch); q++) rd(b + q * stride, len);
}
void wr_rows(double* b, long long stride, long long len, int batch) {
  if (b) for (int q = 0; q < (stride == 0 ? 1 : batch); q++) wr(b + q * stride, len);
}

constexpr long long kGarbage = 0x7777777;  // a caller's stride where the header says it is not read
constexpr int kGap = 3;

enum Family { DIR, ADJ, DENSE };
struct Ev {
  int fam, id, grid;
  long long lds;
  bool operator==(const Ev& o) const { return fam == o.fam && id == o.id && grid == o.grid && lds == o.lds; }
};
template <class T>
T& arg(void** args, int i) { return *static_cast<T*>(args[i]); }

// One call: the caller's arguments, valid, and the stand-ins with what they saw.
struct Case {
  int N, nx, nu, nc, batch;
  bool with_rhs, shared_dir;
  long long nz, nv, nzf, nlf, len[FBSTAB_MPC_NSEQ], xl[3];
  double sigma = 0.0;
  SolverBase h;
  SolverBase* hp = &h;
  fbstab_mpc_batch_t data = {}, ddata = {};
  const fbstab_mpc_batch_t *data_p = &data, *ddata_p = &ddata;
  fbstab_dense_batch_t dense = {};
  const fbstab_dense_batch_t* dense_p = &dense;
  fbstab_var_batch_t x = {}, dx = {}, rhs = {};
  const fbstab_var_batch_t *x_p = &x, *dx_p = &dx, *rhs_p = nullptr;
  double* work = nullptr;
  long long work_doubles = 0;
  int* status = nullptr;
  int dir_rc = FBSTAB_HIP_OK;
  // what the stand-ins saw
  std::vector<Ev> ev;
  int dN = 0, dnx = 0, dnu = 0, dnc = 0, dbatch = 0;
  fbstab_mpc_batch_t dir = {}, a = {};
  fbstab_var_batch_t dir_x = {}, dir_sd = {}, xv = {}, sd = {}, ad = {};
  fbstab_mpc_grad_batch_t g = {};
  fbstab_dense_batch_t dc = {};
  CondenseAdjointWork wk = {};
  const int* finish_status = nullptr;

  double* blk(long long n, long long* stride, bool share = false) {
    if (batch <= 1) { *stride = kGarbage; return D(n); }
    if (share) { *stride = 0; return D(n); }
    *stride = n + kGap;
    return D((batch - 1) * *stride + n);
  }
  Case(int N_, int nx_, int nu_, int nc_, int batch_, bool with_rhs_, bool shared_dir_ = false)
      : N(N_), nx(nx_), nu(nu_), nc(nc_), batch(batch_), with_rhs(with_rhs_), shared_dir(shared_dir_) {
    const long long M = N + 1;
    nz = M * nu; nv = M * nc; nzf = M * (nx + nu); nlf = M * nx;
    const long long l[FBSTAB_MPC_NSEQ] = {M * nx * nx, M * nu * nu, M * nu * nx, M * nx, M * nu, (long long)N * nx * nx,
                                          (long long)N * nx * nu, (long long)N * nx, M * nc * nx, M * nc * nu, M * nc, nx};
    xl[0] = nzf; xl[1] = nlf; xl[2] = nv;
    h.max_batch = 3; h.device = 0;
    h.var_len[0] = nz; h.var_len[1] = 0; h.var_len[2] = h.var_len[3] = nv;
    for (int i = 0; i < FBSTAB_MPC_NSEQ; i++) {
      len[i] = l[i];
      data.base[i] = blk(len[i], &data.stride[i]);
      // every other perturbation slot is NULL, with a stride that must not matter
      if (i % 2 == 0) ddata.base[i] = blk(len[i], &ddata.stride[i], shared_dir);
      else ddata.stride[i] = 1;
    }
    const long long dl[FBSTAB_DENSE_NARR] = {nz * nz, nz, 0, 0, nv * nz, nv};
    for (int i : {FBSTAB_DENSE_H, FBSTAB_DENSE_f, FBSTAB_DENSE_A, FBSTAB_DENSE_b})
      dense.base[i] = blk(dl[i], &dense.stride[i]);
    for (int i = 0; i < 3; i++) {
      x.base[i] = blk(xl[i], &x.stride[i]);
      dx.base[i] = blk(xl[i], &dx.stride[i]);
      rhs.base[i] = blk(xl[i], &rhs.stride[i]);
    }
    if (with_rhs) rhs_p = &rhs;
    status = I(batch > 0 ? batch : 1);
    // with rhs the tail is not the call's: the work array ends behind the adjoint's part
    work_doubles = (5 * nz + 3 * nv + (with_rhs ? 0 : nzf + nlf + nv)) * batch;
    work = D(work_doubles > 0 ? work_doubles : 1);
  }

  void adjoint_work(const CondenseAdjointWork& w) {
    for (double* p : {w.U, w.gU, w.dU, w.rU, w.eU}) { CHECK(inside(p, nz * batch), "a U piece leaves the work array"); }
    for (double* p : {w.gv, w.dv, w.ev}) { CHECK(inside(p, nv * batch), "a v piece leaves the work array"); }
  }
  bool inside(const double* p, long long n) const { return p >= work && p + n <= work + 5 * nz * batch + 3 * nv * batch; }

  int run() {
    auto launch = [this](CondenseAdjointKernel id, int grid, long long lds, void** args, hipStream_t) {
      ev.push_back({ADJ, id, grid, lds});
      if (id == kCondenseAdjSeed || id == kCondenseAdjFinish) {
        CHECK(arg<int>(args, 0) == N && arg<int>(args, 1) == nx && arg<int>(args, 2) == nu && arg<int>(args, 3) == nc, "sizes");
        a = arg<fbstab_mpc_batch_t>(args, 5);
        xv = arg<fbstab_var_batch_t>(args, 6); sd = arg<fbstab_var_batch_t>(args, 7);
        wk = arg<CondenseAdjointWork>(args, 8);
        adjoint_work(wk);
        for (int i = 0; i < FBSTAB_MPC_NSEQ; i++) rd_rows(a.base[i], a.stride[i], len[i], batch);
        for (int i = 0; i < 3; i++) { rd_rows(xv.base[i], xv.stride[i], xl[i], batch); rd_rows(sd.base[i], sd.stride[i], xl[i], batch); }
        if (id == kCondenseAdjSeed) {
          wr(wk.U, nz * batch); wr(wk.gU, nz * batch); wr(wk.gv, nv * batch);
        } else {
          rd(wk.dU, nz * batch); rd(wk.dv, nv * batch);
          g = arg<fbstab_mpc_grad_batch_t>(args, 9); ad = arg<fbstab_var_batch_t>(args, 10);
          finish_status = arg<const int*>(args, 11);
          for (int q = 0; q < batch; q++) g_sink = g_sink + finish_status[q];
          for (int i = 0; i < 3; i++) wr_rows(ad.base[i], ad.stride[i], xl[i], batch);
        }
      } else if (id == kCondenseAdjResidual) {
        const CondenseAdjointWork w = arg<CondenseAdjointWork>(args, 7);
        adjoint_work(w);
        rd(w.gU, nz * batch); rd(w.dU, nz * batch); rd(w.dv, nv * batch); wr(w.rU, nz * batch);
      } else {
        const CondenseAdjointWork w = arg<CondenseAdjointWork>(args, 2);
        adjoint_work(w);
        rd(w.eU, nz * batch); rd(w.ev, nv * batch); wr(w.dU, nz * batch); wr(w.dv, nv * batch);
      }
      return FBSTAB_HIP_OK;
    };
    auto dense_adjoint = [this](int b, const fbstab_dense_batch_t* d, const fbstab_var_batch_t* xc, const fbstab_var_batch_t* s,
                                double, const fbstab_var_batch_t* ac, int* st, hipStream_t) {
      ev.push_back({DENSE, 0, b, 0});
      dc = *d;
      const long long dl[FBSTAB_DENSE_NARR] = {nz * nz, nz, 0, 0, nv * nz, nv};
      for (int i = 0; i < FBSTAB_DENSE_NARR; i++) rd_rows(dc.base[i], dc.stride[i], dl[i], batch);
      rd_rows(xc->base[0], xc->stride[0], nz, batch); rd_rows(xc->base[2], xc->stride[2], nv, batch);
      rd(s->base[0], nz * batch);
      if (s->base[2]) rd(s->base[2], nv * batch);
      wr(ac->base[0], nz * batch); wr(ac->base[2], nv * batch);
      CHECK(st == status, "the dense adjoint reports into the caller's status");
      for (int q = 0; q < batch; q++) st[q] = 0;
      return FBSTAB_HIP_OK;
    };
    auto direction = [this](int N_, int nx_, int nu_, int nc_, int b, const fbstab_mpc_batch_t& d, const fbstab_var_batch_t& xp,
                            const fbstab_var_batch_t& seeds, hipStream_t) -> int {
      if (dir_rc != FBSTAB_HIP_OK) return fail(dir_rc, "the direction refuses");
      ev.push_back({DIR, 0, b * (N_ + 1), 0});
      dN = N_; dnx = nx_; dnu = nu_; dnc = nc_; dbatch = b;
      dir = d; dir_x = xp; dir_sd = seeds;
      for (int i = 0; i < FBSTAB_MPC_NSEQ; i++) rd_rows(d.base[i], d.stride[i], len[i], batch);
      for (int i = 0; i < 3; i++) { rd_rows(xp.base[i], xp.stride[i], xl[i], batch); wr_rows(seeds.base[i], seeds.stride[i], xl[i], batch); }
      return FBSTAB_HIP_OK;
    };
    return condensed_tangent_run(hp, N, nx, nu, nc, batch, data_p, dense_p, x_p, ddata_p, sigma, dx_p, rhs_p, work, status,
                                 nullptr, launch, dense_adjoint, direction);
  }
};

const int kShapes[2][4] = {{2, 2, 1, 1}, {2, 3, 2, 1}};

long long even(long long n) { return n + (n & 1); }
// the LDS bytes of the seed and finish launches, restated from include/fbstab_hip.h (fbstab_hip_mpc_condensed_sizes)
long long condense_lds(int N, int nx, int nu, int nc) {
  const long long ldx = nx | 1, ldc = nc | 1, ldu = nu | 1;
  const long long window = 2 * even(ldx * nx) + even(ldx * nu) + even(ldc * nx) + even(ldu * nx) + even(ldc * nu) + even(ldu * nu);
  const long long m = (N + 2) * even(ldx * nu), v = (long long)(N + 1) * (nx + nu + nc) + 2 * nx + 8;
  return 8 * (window + even(m > v ? m : v));
}

// ---- carve: the seed tail begins where the adjoint's work ends, nothing lies beyond the documented size; with rhs the
// tail is never addressed (the work array of such a Case ends before it) -------------------------------------------
void carve() {
  for (const int* s : {kShapes[0], kShapes[1]})
    for (int batch : {1, 2, 3}) {
      {
        Case c(s[0], s[1], s[2], s[3], batch, false);
        OK(c.run());
        const long long adj = (5 * c.nz + 3 * c.nv) * batch;
        CHECK(c.dir_sd.base[0] == c.work + adj, "gz begins where the adjoint's work ends");
        CHECK(c.dir_sd.base[1] == c.dir_sd.base[0] + c.nzf * batch, "gl follows gz, packed");
        CHECK(c.dir_sd.base[2] == c.dir_sd.base[1] + c.nlf * batch, "gv follows gl, packed");
        CHECK(c.dir_sd.base[2] + c.nv * batch == c.work + c.work_doubles, "the tail ends with the documented size");
        for (int i = 0; i < 3; i++) CHECK(c.dir_sd.stride[i] == c.xl[i], "the tail is packed (slot %d)", i);
        // the adjoint's eight pieces, in the order of the header, each packed
        const CondenseAdjointWork& w = c.wk;
        double* want = c.work;
        for (double* p : {w.U, w.gU, w.dU}) { CHECK(p == want, "U, gU, dU in order"); want += c.nz * batch; }
        for (double* p : {w.gv, w.dv}) { CHECK(p == want, "gv_c, dv in order"); want += c.nv * batch; }
        for (double* p : {w.rU, w.eU}) { CHECK(p == want, "rU, eU in order"); want += c.nz * batch; }
        CHECK(w.ev == want && want + c.nv * batch == c.work + adj, "ev closes the adjoint's part");
      }
      {
        Case c(s[0], s[1], s[2], s[3], batch, true);
        OK(c.run());
        for (int i = 0; i < 3; i++) {
          CHECK(c.dir_sd.base[i] == c.rhs.base[i] && c.sd.base[i] == c.rhs.base[i], "the seeds live in the caller's rhs (slot %d)", i);
          CHECK(c.dir_sd.stride[i] == (batch > 1 ? c.rhs.stride[i] : c.xl[i]), "rhs stride (slot %d)", i);
        }
      }
    }
}

// ---- sequence and the argument blocks of every launch ---------------------------------------------------------------
void sequence() {
  for (const int* s : {kShapes[0], kShapes[1]})
    for (int batch : {1, 2, 3})
      for (bool with_rhs : {false, true})
        for (bool shared_dir : {false, true}) {
          Case c(s[0], s[1], s[2], s[3], batch, with_rhs, shared_dir);
          OK(c.run());
          const int N = s[0];
          const long long lds = condense_lds(s[0], s[1], s[2], s[3]);
          const Ev dadj = {DENSE, 0, batch, 0};
          const std::vector<Ev> want = {{DIR, 0, batch * (N + 1), 0}, {ADJ, kCondenseAdjSeed, batch, lds}, dadj,
                                        {ADJ, kCondenseAdjResidual, batch, 0}, dadj, {ADJ, kCondenseAdjCorrect, batch, 0},
                                        {ADJ, kCondenseAdjFinish, batch, lds}};
          CHECK(c.ev.size() == want.size(), "%zu launches, expected %zu", c.ev.size(), want.size());
          for (size_t i = 0; i < c.ev.size() && i < want.size(); i++)
            CHECK(c.ev[i] == want[i], "launch %zu is (%d, %d, grid %d, lds %lld)", i, c.ev[i].fam, c.ev[i].id, c.ev[i].grid, c.ev[i].lds);
          CHECK(c.dN == s[0] && c.dnx == s[1] && c.dnu == s[2] && c.dnc == s[3] && c.dbatch == batch, "the direction's sizes");
          for (int i = 0; i < FBSTAB_MPC_NSEQ; i++) {
            CHECK(c.a.base[i] == c.data.base[i] && c.a.stride[i] == c.data.stride[i], "the data block passes as it is (slot %d)", i);
            CHECK(c.dir.base[i] == c.ddata.base[i], "direction slot %d: base", i);
            if (!c.ddata.base[i]) continue;   // (a NULL slot: its stride is nobody's)
            CHECK(c.dir.stride[i] == (batch > 1 ? c.ddata.stride[i] : c.len[i]), "direction slot %d: stride %lld", i, c.dir.stride[i]);
            if (shared_dir && batch > 1) CHECK(c.dir.stride[i] == 0, "stride 0 is kept (slot %d)", i);
          }
          for (int i = 0; i < 3; i++) {
            const long long xs = batch > 1 ? c.x.stride[i] : c.xl[i], ds = batch > 1 ? c.dx.stride[i] : c.xl[i];
            CHECK(c.dir_x.base[i] == c.x.base[i] && c.dir_x.stride[i] == xs, "the direction's point (slot %d)", i);
            CHECK(c.xv.base[i] == c.x.base[i] && c.xv.stride[i] == xs, "the adjoint's point (slot %d)", i);
            CHECK(c.sd.base[i] == c.dir_sd.base[i] && c.sd.stride[i] == c.dir_sd.stride[i], "the chain reads the seeds where the direction wrote them (slot %d)", i);
            CHECK(c.ad.base[i] == c.dx.base[i] && c.ad.stride[i] == ds, "adj = dx (slot %d)", i);
          }
          for (int i = 0; i < FBSTAB_MPC_NSEQ; i++) CHECK(!c.g.base[i], "gradient slot %d is NULL", i);
          CHECK(c.finish_status == c.status, "the finish kernel reads the caller's status");
        }
  {  // batch 0: OK, nothing queued, no device call
    Case c(2, 2, 1, 1, 0, false);
    const long calls = fb_shim::state().calls;
    OK(c.run());
    CHECK(c.ev.empty() && fb_shim::state().calls == calls, "batch 0 queues nothing");
  }
  {  // a direction that refuses: its code comes back and nothing of the adjoint is queued
    Case c(2, 2, 1, 1, 2, false);
    c.dir_rc = FBSTAB_HIP_ERR_UNSUPPORTED;
    const int rc = c.run();
    CHECK(rc == FBSTAB_HIP_ERR_UNSUPPORTED && c.ev.empty(), "rc %d, %zu launches", rc, c.ev.size());
  }
}

// ---- refusals, in the documented order: each case spoils the argument of one check AND of a later one -----------------
void refuse(int code, const char* text, const std::function<void(Case&)>& spoil, bool early = true) {
  Case c(2, 2, 1, 1, 2, true);
  spoil(c);
  const long calls = fb_shim::state().calls;
  g_error.clear();
  const int rc = c.run();
  CHECK(rc == code && g_error == text, "%d \"%s\", expected %d \"%s\"", rc, g_error.c_str(), code, text);
  if (early) CHECK(fb_shim::state().calls == calls, "\"%s\": %ld device calls before the refusal", text, fb_shim::state().calls - calls);
  CHECK(c.ev.empty(), "\"%s\": %zu launches queued", text, c.ev.size());
}
void refusals() {
  const int A = FBSTAB_HIP_ERR_ARGUMENT, U = FBSTAB_HIP_ERR_UNSUPPORTED, DV = FBSTAB_HIP_ERR_DEVICE;
  refuse(A, "condense: problem sizes must be positive", [](Case& c) { c.nu = 0; c.batch = -1; });
  refuse(A, "condense: negative batch", [](Case& c) { c.batch = -1; c.data_p = nullptr; });
  refuse(A, "condense: null problem data block", [](Case& c) { c.data_p = nullptr; c.dense_p = nullptr; });
  refuse(A, "condense: null problem data pointer", [](Case& c) { c.data.base[FBSTAB_MPC_d] = nullptr; c.x_p = nullptr; });
  refuse(A, "condense: problem data stride smaller than the array length", [](Case& c) { c.data.stride[FBSTAB_MPC_q] = 1; c.x_p = nullptr; });
  for (int k = 0; k < 6; k++)
    refuse(A, "condensed tangent: null argument", [k](Case& c) {
      if (k == 0) c.dense_p = nullptr;
      if (k == 1) c.x_p = nullptr;
      if (k == 2) c.ddata_p = nullptr;
      if (k == 3) c.dx_p = nullptr;
      if (k == 4) c.work = nullptr;
      if (k == 5) c.status = nullptr;
      c.dense.base[FBSTAB_DENSE_H] = nullptr;
    });
  refuse(A, "condensed tangent: null pointer in the condensed images", [](Case& c) { c.dense.base[FBSTAB_DENSE_A] = nullptr; c.x.base[0] = nullptr; });
  refuse(A, "condensed tangent: stride of a condensed image smaller than the array length", [](Case& c) { c.dense.stride[FBSTAB_DENSE_f] = 0; c.x.base[0] = nullptr; });
  refuse(A, "condensed tangent: null variable pointer", [](Case& c) { c.x.base[1] = nullptr; c.dx.base[1] = nullptr; c.ddata.stride[0] = 1; });
  refuse(A, "condensed tangent: variable stride smaller than the vector length", [](Case& c) { c.x.stride[0] = 1; c.dx.base[0] = nullptr; });
  refuse(A, "condensed tangent: null tangent pointer (dx)", [](Case& c) { c.dx.base[2] = nullptr; c.ddata.stride[0] = 1; });
  refuse(A, "condensed tangent: tangent stride smaller than the vector length", [](Case& c) { c.dx.stride[1] = 0; c.rhs.base[1] = nullptr; });
  refuse(A, "condensed tangent: null right-hand side pointer (rhs)", [](Case& c) { c.rhs.base[1] = nullptr; c.ddata.stride[0] = 1; });
  refuse(A, "condensed tangent: right-hand side stride smaller than the vector length", [](Case& c) { c.rhs.stride[2] = 0; c.ddata.stride[0] = 1; });
  refuse(A, "condensed tangent: perturbation stride is neither 0 nor at least the array length", [](Case& c) { c.ddata.stride[0] = 1; c.hp = nullptr; });
  refuse(A, "condensed tangent: perturbation stride is neither 0 nor at least the array length", [](Case& c) { c.ddata.stride[FBSTAB_MPC_x0 - 1] = -2; });
  refuse(A, "condensed tangent: null dense solver handle", [](Case& c) { c.hp = nullptr; c.h.device = 5; });
  refuse(A, "condensed tangent: the dense handle is not one of ((N + 1) nu, 0, (N + 1) nc)", [](Case& c) { c.h.var_len[1] = 1; c.h.max_batch = 1; });
  refuse(A, "condensed tangent: batch exceeds the max_batch the handle was created with", [](Case& c) { c.h.max_batch = 1; c.h.device = 5; });
  refuse(DV, "condense: no such device", [](Case& c) { c.h.device = 5; c.dir_rc = FBSTAB_HIP_ERR_ARGUMENT; }, false);
  refuse(U, "condense: the stage images and dx/du of a horizon do not fit the 160 KiB LDS budget",
         [](Case& c) {
           c.nx = 200;
           c.dir_rc = FBSTAB_HIP_ERR_ARGUMENT;
           for (int i = 0; i < FBSTAB_MPC_NSEQ; i++) c.data.stride[i] = c.ddata.stride[i] = 0;
           for (int i = 0; i < 3; i++) c.x.stride[i] = c.dx.stride[i] = c.rhs.stride[i] = 1 << 20;
           c.dense.stride[FBSTAB_DENSE_f] = c.dense.stride[FBSTAB_DENSE_b] = 1 << 20;
         }, false);
  // ... and behind all of that the direction's own refusals (the callable's: here the stand-in's)
  refuse(A, "the direction refuses", [](Case& c) { c.dir_rc = FBSTAB_HIP_ERR_ARGUMENT; }, false);
  // what is allowed: a NULL rhs, a NULL perturbation slot with any stride, stride 0 on a perturbation
  {
    Case c(2, 2, 1, 1, 2, false, true);
    for (int i = 0; i < FBSTAB_MPC_NSEQ; i++)
      if (!c.ddata.base[i]) c.ddata.stride[i] = -7;
    OK(c.run());
    CHECK(c.ev.size() == 7, "%zu launches", c.ev.size());
  }
}

}  // namespace

int main(int argc, char** argv) {
  const std::string group = argc > 1 ? argv[1] : "";
  if (group == "carve") carve();
  else if (group == "sequence") sequence();
  else if (group == "refusals") refusals();
  else return 2;
  return g_failures ? 1 : 0;
}
