// TEST INFRASTRUCTURE ONLY - the driver of tests/test_host_stage.py: fbstab_amd/csrc/fb_host_stage.h and
// fb_sweep_stage.h over the heap-backed runtime of runtime_shim/, bare SolverBase objects with the lengths the create functions set, and host
// lambdas in the kernels' place.  A lambda reads every input double through the kernel-side base / stride and
// writes every output double with a value that names its kind, QP, slot and index (val below); the driver then looks
// for those values where include/fbstab_hip.h says QP q of a slot lives: base + q * stride, one row for stride 0,
// at the base for batch 1 - restated here, not taken from the header under test.
//
// usage: stage_driver <group>; prints one line per failed check and exits 1, prints nothing and exits 0 otherwise.
#include "fb_sweep_stage.h"

#include <cstdint>
#include <cstdio>
#include <functional>
#include <memory>
#include <utility>

namespace {

int g_failures = 0;
#define CHECK(cond, ...)                                   \
  do {                                                     \
    if (!(cond)) {                                         \
      if (g_failures++ < 40) {                             \
        std::printf("FAIL %s:%d: %s: ", __func__, __LINE__, #cond); \
        std::printf(__VA_ARGS__);                          \
        std::printf("\n");                                 \
      }                                                    \
    }                                                      \
  } while (0)

constexpr uint64_t kCanary = 0x7FF8C0DEFACE5EEDull;  // (tests/placement_helpers.py: a quiet NaN with a payload)
constexpr int kGap = 3;
double canary() {
  double d;
  memcpy(&d, &kCanary, 8);
  return d;
}
bool is_canary(double d) {
  uint64_t u;
  memcpy(&u, &d, 8);
  return u == kCanary;
}

enum Tag { DATA = 1, POINT, SEED, DIR, SOL, GRAD, ADJ, RHS, STEP, NORM, RES, SUM, IO_IN, IO_OUT, GAIN };
double val(int tag, long q, int slot, long j) { return tag * 1e6 + q * 1e4 + slot * 1e2 + (double)j; }

struct Shape {
  std::vector<long long> arr;
  long long var[4];
};
Shape mpc_shape(int N, int nx, int nu, int nc) {  // (include/fbstab_hip.h: the sequences of fbstab_mpc_batch_t)
  const long long M = N + 1;
  return {{M * nx * nx, M * nu * nu, M * nu * nx, M * nx, M * nu, (long long)N * nx * nx, (long long)N * nx * nu,
           (long long)N * nx, M * nc * nx, M * nc * nu, M * nc, nx},
          {M * (nx + nu), M * nx, M * nc, M * nc}};
}
Shape dense_shape(int nz, int nl, int nv) {
  return {{(long long)nz * nz, nz, (long long)nl * nz, nl, (long long)nv * nz, nv}, {nz, nl, nv, nv}};
}
const Shape kShapes[3] = {mpc_shape(2, 2, 1, 1), dense_shape(2, 1, 3), dense_shape(2, 0, 3)};
constexpr int kMaxBatch = 3;

void init_handle(SolverBase& h, const Shape& sh) {
  int rc = h.common_init(0, kMaxBatch);
  CHECK(rc == FBSTAB_HIP_OK, "%s", g_error.c_str());
  h.arr_len = sh.arr;
  for (int i = 0; i < 4; i++) h.var_len[i] = sh.var[i];
}

// ---- placements (tests/placement_helpers.py): every buffer is exactly as long as its slots and gaps ----------------
enum Layout { PACKED, RECORDS, SHARED };  // SHARED: every slot of `share` one row (stride 0), the others in records
struct Placed {
  int B = 0;
  std::vector<long long> len, stride;
  std::vector<double*> base;
  std::vector<bool> shared;
  std::vector<std::unique_ptr<std::vector<double>>> bufs;
  std::vector<std::vector<char>> used;

  double* add(long long n) {
    bufs.emplace_back(new std::vector<double>((size_t)n, canary()));
    used.emplace_back((size_t)n, 0);
    return bufs.back()->data();
  }
  long rows(int i) const { return shared[i] ? 1 : B; }
  void mark() {
    for (size_t i = 0; i < len.size(); i++) {
      if (!base[i]) continue;
      for (size_t b = 0; b < bufs.size(); b++) {
        double* lo = bufs[b]->data();
        if (base[i] < lo || base[i] >= lo + bufs[b]->size()) continue;
        for (long r = 0; r < rows((int)i); r++)
          for (long long j = 0; j < len[i]; j++) used[b][(size_t)(base[i] - lo + r * stride[i] + j)] = 1;
      }
    }
  }
  double& at(int i, long q, long long j) { return base[i][(shared[i] ? 0 : q) * stride[i] + j]; }
  void fill(int tag, unsigned only = ~0u) {
    for (size_t i = 0; i < len.size(); i++)
      if (base[i] && (only >> i & 1))
        for (long r = 0; r < rows((int)i); r++)
          for (long long j = 0; j < len[i]; j++) at((int)i, r, j) = val(tag, r, (int)i, j);
  }
  void expect(int tag, unsigned only, const char* what) {
    for (size_t i = 0; i < len.size(); i++)
      if (base[i] && (only >> i & 1))
        for (long r = 0; r < rows((int)i); r++)
          for (long long j = 0; j < len[i]; j++)
            CHECK(at((int)i, r, j) == val(tag, r, (int)i, j), "%s slot %zu QP %ld index %lld holds %.17g", what, i, r, j,
                  at((int)i, r, j));
  }
  void expect_untouched(unsigned only, const char* what) {
    for (size_t i = 0; i < len.size(); i++)
      if (base[i] && (only >> i & 1))
        for (long r = 0; r < rows((int)i); r++)
          for (long long j = 0; j < len[i]; j++) CHECK(is_canary(at((int)i, r, j)), "%s slot %zu was written", what, i);
  }
  void gaps_intact(const char* what) {
    for (size_t b = 0; b < bufs.size(); b++)
      for (size_t k = 0; k < bufs[b]->size(); k++)
        CHECK(used[b][k] || is_canary((*bufs[b])[k]), "%s: canary %zu of buffer %zu overwritten", what, k, b);
  }
};

// `share`: the slots given as one row; `null`: the slots left out (a slot of length 0 is always NULL).
Placed place(const long long* len, int n, int B, Layout lay, unsigned share = 0, unsigned null = 0) {
  Placed p;
  p.B = B;
  p.len.assign(len, len + n);
  p.stride.assign(n, 0);
  p.base.assign(n, nullptr);
  p.shared.assign(n, false);
  const long rows = B > 0 ? B : 1;  // (batch 0: pointers that are not NULL, and nothing behind them is touched)
  long long rec = 0;
  for (int i = 0; i < n; i++) {
    p.shared[i] = lay == SHARED && (share >> i & 1);
    if (len[i] > 0 && !(null >> i & 1) && !p.shared[i]) rec += len[i] + kGap;
  }
  double* record = lay != PACKED && rec > 0 ? p.add(rows * rec) : nullptr;
  long long off = 0;
  for (int i = 0; i < n; i++) {
    if (len[i] == 0 || (null >> i & 1)) continue;
    if (p.shared[i]) {
      p.base[i] = p.add(len[i] + kGap);
    } else if (lay == PACKED) {
      p.base[i] = p.add(rows * len[i]);
      p.stride[i] = len[i];
    } else {
      p.base[i] = record + off;
      p.stride[i] = rec;
      off += len[i] + kGap;
    }
  }
  p.mark();
  return p;
}

template <class Block>
Block block_of(const Placed& p) {
  Block b{};
  for (size_t i = 0; i < p.len.size(); i++) {
    b.base[i] = p.base[i];
    b.stride[i] = p.stride[i];
  }
  return b;
}

// What a kernel does with an input block: every double of every QP, through the kernel-side base and stride.
template <class Block>
void kernel_reads(const Block& k, const Placed& from, int tag, int nslots, const char* what) {
  for (int i = 0; i < nslots; i++) {
    if (!from.base[i]) {
      CHECK(!k.base[i] || from.len[i] == 0, "%s slot %d: NULL became a pointer", what, i);
      continue;
    }
    for (long q = 0; q < from.B; q++)
      for (long long j = 0; j < from.len[i]; j++) {
        const double got = k.base[i][q * k.stride[i] + j];
        CHECK(got == val(tag, from.shared[i] ? 0 : q, i, j), "%s slot %d QP %ld index %lld reads %.17g", what, i, q, j,
              got);
      }
  }
}
template <class Block>
void kernel_writes(const Block& k, const long long* len, int B, int tag, int nslots) {
  for (int i = 0; i < nslots; i++)
    if (k.base[i])
      for (long q = 0; q < B; q++)
        for (long long j = 0; j < len[i]; j++) k.base[i][q * k.stride[i] + j] = val(tag, q, i, j);
}
// host-pointer calls: the kernel-side block is packed (stride = length; 0 for a row the batch shares)
template <class Block>
void expect_packed(const Block& k, const Placed& from, int nslots, const char* what) {
  for (int i = 0; i < nslots; i++)
    if (from.base[i])
      CHECK(k.stride[i] == (from.shared[i] && from.B > 1 ? 0 : from.len[i]), "%s slot %d: kernel-side stride %lld",
            what, i, k.stride[i]);
}
template <class Block>
void expect_same(const Block& k, const Placed& from, int nslots, const char* what) {
  for (int i = 0; i < nslots; i++)
    CHECK(k.base[i] == from.base[i] && k.stride[i] == from.stride[i], "%s slot %d is not the caller's", what, i);
}

const Layout kLayouts[3] = {PACKED, RECORDS, SHARED};
const int kBatches[3] = {0, 1, 3};

// ---- solve_run -----------------------------------------------------------------------------------------------------
void solves(bool dev_ptrs) {
  for (const Shape& sh : kShapes)
    for (Layout lay : kLayouts)
      for (int B : kBatches)
        for (int out_on_host = 0; out_on_host < (dev_ptrs ? 2 : 1); out_on_host++)
          for (int with_norms = 0; with_norms < 2; with_norms++) {
            SolverBase h;
            init_handle(h, sh);
            const int n = (int)sh.arr.size();
            Placed data = place(sh.arr.data(), n, B, lay, ~0u), x = place(sh.var, 4, B, lay == SHARED ? RECORDS : lay);
            data.fill(DATA);
            x.fill(POINT, 7);
            fbstab_mpc_batch_t d = block_of<fbstab_mpc_batch_t>(data);
            fbstab_var_batch_t xv = block_of<fbstab_var_batch_t>(x);
            std::vector<fbstab_solver_out_t> out((size_t)(B > 0 ? B : 1));
            std::vector<double> norms((size_t)(B > 0 ? 4 * B : 1), canary());
            const int flags = dev_ptrs ? FBSTAB_HIP_DEVICE_POINTERS | (out_on_host ? FBSTAB_HIP_OUT_ON_HOST : 0) : 0;
            int launches = 0;
            const long mallocs0 = fb_shim::state().mallocs, calls0 = fb_shim::state().calls;
            auto launch = [&](hipStream_t, const fbstab_mpc_batch_t& a, const fbstab_var_batch_t& v,
                              fbstab_solver_out_t* d_out) {
              launches++;
              if (dev_ptrs) {
                expect_same(a, data, n, "data");
                expect_same(v, x, 4, "x");
                CHECK((d_out == out.data()) == !out_on_host, "records: %p", (void*)d_out);
              } else {
                expect_packed(a, data, n, "data");
                expect_packed(v, x, 4, "x");
              }
              kernel_reads(a, data, DATA, n, "data");
              kernel_reads(v, x, POINT, 3, "x");
              kernel_writes(v, sh.var, B, SOL, 4);
              for (int q = 0; q < B; q++) {
                d_out[q] = fbstab_solver_out_t{};
                d_out[q].eflag = 7 + q;
                d_out[q].newton_iters = 20 + q;
                d_out[q].residual = val(RES, q, 0, 0);
              }
              return (int)FBSTAB_HIP_OK;
            };
            auto launch_norms = [&](hipStream_t, const fbstab_mpc_batch_t&, const fbstab_var_batch_t&, double* dn) {
              CHECK((dn == norms.data()) == (dev_ptrs && !out_on_host), "norms: %p", (void*)dn);
              for (int k = 0; k < 4 * B; k++) dn[k] = val(NORM, k / 4, 0, k % 4);
            };
            int rc = solve_run(&h, B, &d, &xv, out.data(), flags, nullptr, with_norms ? norms.data() : nullptr, launch,
                               launch_norms);
            CHECK(rc == FBSTAB_HIP_OK, "%s", g_error.c_str());
            CHECK(launches == (B > 0), "%d launches for batch %d", launches, B);
            if (B == 0) CHECK(fb_shim::state().calls == calls0, "batch 0 made a device call");
            if (dev_ptrs)  // pass-through; OUT_ON_HOST: exactly the record buffer and the norm buffer
              CHECK(fb_shim::state().mallocs - mallocs0 == (B > 0 && out_on_host ? 1 + with_norms : 0),
                    "%ld allocations", fb_shim::state().mallocs - mallocs0);
            if (B > 0) {
              x.expect(SOL, 15, "solution");
              for (int q = 0; q < B; q++)
                CHECK(out[q].eflag == 7 + q && out[q].newton_iters == 20 + q && out[q].residual == val(RES, q, 0, 0),
                      "record %d", q);
              for (int k = 0; k < 4 * B; k++)
                CHECK(with_norms ? norms[k] == val(NORM, k / 4, 0, k % 4) : is_canary(norms[k]), "norm %d", k);
            }
            data.expect(DATA, ~0u, "data after the call");
            data.gaps_intact("data");
            x.gaps_intact("x");
          }
  CHECK(fb_shim::state().live == 0, "%ld allocations live", fb_shim::state().live);
}

// ---- adjoint_run and tangent_run: the launches are function pointers, their context is here -----------------------
struct Ctx {
  const Shape* sh = nullptr;
  int B = 0, n = 0, launches = 0, reduces = 0;
  bool dev_ptrs = false;
  Placed *data = nullptr, *x = nullptr, *seed = nullptr, *grad = nullptr, *adj = nullptr, *dir = nullptr;
  unsigned reduced = 0;  // gradient slots summed over the batch
  bool seeds_from_dir = false;
  const fbstab_solver_out_t* out = nullptr;
} g;

int adjoint_launch(SolverBase*, int batch, AdjointLaunchArgs& st, double sigma) {
  g.launches++;
  CHECK(batch == g.B && sigma == 0.5, "batch %d sigma %g", batch, sigma);
  if (g.dev_ptrs) {
    expect_same(st.a, *g.data, g.n, "data");
    expect_same(st.v, *g.x, 3, "x");
  } else {
    expect_packed(st.a, *g.data, g.n, "data");
    expect_packed(st.v, *g.x, 3, "x");
  }
  kernel_reads(st.a, *g.data, DATA, g.n, "data");
  kernel_reads(st.v, *g.x, POINT, 3, "x");
  if (g.seeds_from_dir) {  // the tangent: the seeds are where the direction kernel left them
    for (int i = 0; i < 3; i++)
      for (long q = 0; q < g.B; q++)
        for (long long j = 0; j < g.sh->var[i]; j++)
          CHECK(st.sd.base[i][q * st.sd.stride[i] + j] == val(RHS, q, i, j), "seed slot %d QP %ld", i, q);
  } else {
    kernel_reads(st.sd, *g.seed, SEED, 3, "seed");
  }
  for (int i = 0; i < g.n; i++) {
    const bool per_qp = g.grad && g.grad->base[i] && !(g.reduced >> i & 1);
    CHECK((st.g.base[i] != nullptr) == per_qp, "gradient slot %d: %p", i, (void*)st.g.base[i]);
  }
  kernel_writes(st.g, g.sh->arr.data(), g.B, GRAD, g.n);
  for (int i = 0; i < 3; i++)  // a reduced call takes every adjoint step, the caller's or the handle's own
    CHECK((st.ad.base[i] != nullptr) == (g.sh->var[i] > 0 && ((g.adj && g.adj->base[i]) || g.reduced)),
          "adjoint slot %d: %p", i, (void*)st.ad.base[i]);
  kernel_writes(st.ad, g.sh->var, g.B, ADJ, 3);
  for (int q = 0; q < g.B; q++) st.d_st[q] = 40 + q;
  return FBSTAB_HIP_OK;
}

int reduce_launch(const GradReduceArgs& ra, const GradReduceOut& ro, hipStream_t) {
  g.reduces++;
  CHECK(ra.batch == g.B && ra.scratch != nullptr, "batch %d", ra.batch);
  CHECK(ra.plan.nz == g.sh->var[0] && ra.plan.nl == g.sh->var[1] && ra.plan.nv == g.sh->var[2], "plan");
  for (int i = 0; i < 3; i++)
    for (long q = 0; q < g.B; q++)
      for (long long j = 0; j < g.sh->var[i]; j++) {
        CHECK(ra.x[i][q * ra.xs[i] + j] == val(POINT, q, i, j), "point slot %d QP %ld", i, q);
        CHECK(ra.p[i][q * ra.ps[i] + j] == val(ADJ, q, i, j), "adjoint step slot %d QP %ld", i, q);
      }
  for (int q = 0; q < g.B; q++) {
    CHECK(ra.status[q] == 40 + q, "status %d", q);
    if (g.out) CHECK(ra.out && ra.out[q].eflag == g.out[q].eflag, "record %d", q);
  }
  if (!g.out) CHECK(!ra.out, "records out of nowhere");
  for (int i = 0; i < kGradReduceMaxSeq; i++) {
    CHECK((ro.base[i] != nullptr) == (i < g.n && (g.reduced >> i & 1) && g.sh->arr[i] > 0), "reduced slot %d", i);
    if (ro.base[i])
      for (long long j = 0; j < g.sh->arr[i]; j++) ro.base[i][j] = val(SUM, 0, i, j);
  }
  return FBSTAB_HIP_OK;
}

struct AdjointCase {
  bool adj, dev_ptrs;
  unsigned seed_null, grad_null, reduced;
  bool with_out;
};
const AdjointCase kAdjointCases[] = {
    {true, false, 0, 0, 0, false},        // everything, host pointers
    {false, false, 6, 0, 0, false},       // no adj; gl and gv NULL
    {true, false, 0, ~0u ^ 0x12, 0, false},  // a subset of gradient slots (1 and 4)
    {true, true, 0, 0, 0, false},         // device pointers: the caller's blocks
    {false, false, 0, 0, 0x9, true},      // reduced: slots 0 and 3 summed, no adj, the solve's records
    {true, true, 2, 0, 0x3f, false},      // reduced, device pointers, every dense slot summed
};

void adjoints() {
  for (const Shape& sh : kShapes)
    for (Layout lay : {PACKED, RECORDS})
      for (int B : kBatches)
        for (const AdjointCase& c : kAdjointCases) {
          SolverBase h;
          init_handle(h, sh);
          const int n = (int)sh.arr.size();
          // (a reduced slot is ONE array of the slot's length: stride 0)
          Placed data = place(sh.arr.data(), n, B, lay), x = place(sh.var, 3, B, lay),
                 seed = place(sh.var, 3, B, lay, 0, c.seed_null), adj = place(sh.var, 3, B, lay),
                 grad = place(sh.arr.data(), n, B, c.reduced ? SHARED : lay, c.reduced, c.grad_null);
          data.fill(DATA); x.fill(POINT); seed.fill(SEED);
          fbstab_mpc_batch_t d = block_of<fbstab_mpc_batch_t>(data);
          fbstab_mpc_grad_batch_t gr = block_of<fbstab_mpc_grad_batch_t>(grad);
          fbstab_var_batch_t xv = block_of<fbstab_var_batch_t>(x), sv = block_of<fbstab_var_batch_t>(seed),
                             av = block_of<fbstab_var_batch_t>(adj);
          std::vector<int> status((size_t)(B > 0 ? B : 1), -1);
          std::vector<fbstab_solver_out_t> out((size_t)(B > 0 ? B : 1));
          for (int q = 0; q < B; q++) out[q].eflag = 3 + q;
          g = Ctx{};
          g.sh = &sh; g.B = B; g.n = n; g.dev_ptrs = c.dev_ptrs;
          g.data = &data; g.x = &x; g.seed = &seed; g.grad = &grad; g.adj = c.adj ? &adj : nullptr;
          // (B == 1: a slot of stride 0 is the one QP's own - nothing to sum - unless it is what `reduced` means)
          g.reduced = c.reduced & ~c.grad_null;
          for (int i = 0; i < n; i++)
            if (sh.arr[i] == 0) g.reduced &= ~(1u << i);
          g.out = c.with_out ? out.data() : nullptr;
          GradReducePlan plan = grad_reduce_plan_dense((int)sh.var[0], (int)sh.var[1], (int)sh.var[2]);
          const long calls0 = fb_shim::state().calls;
          int rc = adjoint_run(&h, B, &d, &xv, &sv, 0.5, &gr, c.adj ? &av : nullptr, status.data(), g.out,
                               c.dev_ptrs ? (int)FBSTAB_HIP_DEVICE_POINTERS : 0, nullptr, c.reduced != 0, plan,
                               adjoint_launch, reduce_launch);
          CHECK(rc == FBSTAB_HIP_OK, "%s", g_error.c_str());
          CHECK(g.launches == (B > 0) && g.reduces == (B > 0 && g.reduced), "%d launches, %d reductions", g.launches,
                g.reduces);
          if (B == 0) CHECK(fb_shim::state().calls == calls0, "batch 0 made a device call");
          if (B > 0) {
            grad.expect(GRAD, ~g.reduced, "gradient");
            grad.expect(SUM, g.reduced, "summed gradient");
            if (c.adj) adj.expect(ADJ, 7, "adjoint");
            else adj.expect_untouched(7, "adjoint");
            for (int q = 0; q < B; q++) CHECK(status[q] == 40 + q, "status %d: %d", q, status[q]);
          }
          for (Placed* p : {&data, &x, &seed, &adj, &grad}) p->gaps_intact("adjoint");
          data.expect(DATA, ~0u, "data after the call");
        }
  CHECK(fb_shim::state().live == 0, "%ld allocations live", fb_shim::state().live);
}

void tangents() {
  for (const Shape& sh : kShapes)
    for (Layout lay : kLayouts)
      for (int B : kBatches)
        for (int with_rhs = 0; with_rhs < 2; with_rhs++)
          for (int dev_ptrs = 0; dev_ptrs < 2; dev_ptrs++) {
            SolverBase h;
            init_handle(h, sh);
            const int n = (int)sh.arr.size();
            // perturbations: slot 2 left out (zero); SHARED: slots 0 and 1 one direction for every QP
            Placed data = place(sh.arr.data(), n, B, lay, ~0u), x = place(sh.var, 3, B, lay == SHARED ? RECORDS : lay),
                   dir = place(sh.arr.data(), n, B, lay, 3, 4), dx = place(sh.var, 3, B, lay == SHARED ? RECORDS : lay),
                   rhs = place(sh.var, 3, B, lay == SHARED ? RECORDS : lay);
            data.fill(DATA); x.fill(POINT); dir.fill(DIR);
            fbstab_mpc_batch_t d = block_of<fbstab_mpc_batch_t>(data), dd = block_of<fbstab_mpc_batch_t>(dir);
            fbstab_var_batch_t xv = block_of<fbstab_var_batch_t>(x), dxv = block_of<fbstab_var_batch_t>(dx),
                               rv = block_of<fbstab_var_batch_t>(rhs);
            std::vector<int> status((size_t)(B > 0 ? B : 1), -1);
            g = Ctx{};
            g.sh = &sh; g.B = B; g.n = n; g.dev_ptrs = dev_ptrs != 0;
            g.data = &data; g.x = &x; g.adj = &dx; g.seeds_from_dir = true;
            int dirs = 0;
            auto launch_dir = [&](const fbstab_mpc_batch_t& p, const AdjointLaunchArgs& st) {
              dirs++;
              if (dev_ptrs && B > 1) expect_same(p, dir, n, "perturbation");
              if (!dev_ptrs) expect_packed(p, dir, n, "perturbation");
              kernel_reads(p, dir, DIR, n, "perturbation");
              kernel_reads(st.v, x, POINT, 3, "x");
              // device pointers and a caller's rhs: the seeds are written there
              for (int i = 0; i < 3; i++)
                if (sh.var[i] > 0)
                  CHECK((st.sd.base[i] == rhs.base[i]) == (dev_ptrs && with_rhs), "seed slot %d", i);
              kernel_writes(st.sd, sh.var, B, RHS, 3);
            };
            int rc = TangentStage::check(&h, B, dd.base, dd.stride, &dxv, with_rhs ? &rv : nullptr);
            CHECK(rc == FBSTAB_HIP_OK, "%s", g_error.c_str());
            const long calls0 = fb_shim::state().calls;
            rc = tangent_run(&h, B, &d, &xv, &dd, 0.5, &dxv, with_rhs ? &rv : nullptr, status.data(),
                             dev_ptrs ? (int)FBSTAB_HIP_DEVICE_POINTERS : 0, nullptr, (const void*)&g, launch_dir,
                             adjoint_launch);
            CHECK(rc == FBSTAB_HIP_OK, "%s", g_error.c_str());
            CHECK(dirs == (B > 0) && g.launches == (B > 0), "%d and %d launches", dirs, g.launches);
            if (B == 0) CHECK(fb_shim::state().calls == calls0, "batch 0 made a device call");
            if (B > 0) {
              dx.expect(ADJ, 7, "tangent");
              if (with_rhs) rhs.expect(RHS, 7, "right-hand side");
              else rhs.expect_untouched(7, "right-hand side");
              for (int q = 0; q < B; q++) CHECK(status[q] == 40 + q, "status %d: %d", q, status[q]);
            }
            for (Placed* p : {&data, &x, &dir, &dx, &rhs}) p->gaps_intact("tangent");
            dir.expect(DIR, ~0u, "perturbations after the call");
          }
  CHECK(fb_shim::state().live == 0, "%ld allocations live", fb_shim::state().live);
}

// ---- MultiStage: vector k of QP q of slot i at base[i] + q stride[i] + k rhs_stride[i] ---------------------------
struct MultiBlock {
  fbstab_multi_var_batch_t b{};
  std::vector<std::vector<double>> buf;
  const long long* len;
  int B, nrhs;
  // pad: how much larger than needed rhs_stride and stride are; shared: one block for the batch (stride 0)
  MultiBlock(const long long* len_, int B_, int nrhs_, int pad, bool shared, unsigned null) : len(len_), B(B_), nrhs(nrhs_) {
    buf.resize(3);
    for (int i = 0; i < 3; i++) {
      if (len[i] == 0 || (null >> i & 1)) continue;
      const long long rs = len[i] + pad, st = nrhs * rs + 2 * pad;
      buf[i].assign((size_t)((shared ? 1 : B) * st), canary());
      b.base[i] = buf[i].data();
      b.rhs_stride[i] = rs;
      b.stride[i] = shared ? 0 : st;
    }
  }
  template <class F>
  void each(F f) {  // f(slot, QP, vector, index, the caller's double)
    for (int i = 0; i < 3; i++)
      if (b.base[i])
        for (long q = 0; q < (b.stride[i] == 0 && B > 1 ? 1 : B); q++)
          for (int k = 0; k < nrhs; k++)
            for (long long j = 0; j < len[i]; j++) f(i, q, k, j, b.base[i][q * b.stride[i] + k * b.rhs_stride[i] + j]);
  }
  long canaries() {
    long c = 0;
    for (auto& v : buf)
      for (double d : v) c += is_canary(d);
    return c;
  }
};

void multi() {
  const Shape& sh = kShapes[0];
  const long long* len = sh.var;
  for (int B : {1, 3})
    for (int nrhs : {1, 3})
      for (int pad : {0, 1})
        for (int dev_ptrs = 0; dev_ptrs < 2; dev_ptrs++)
          for (int shared = 0; shared < 2; shared++) {
            MultiBlock seed(len, B, nrhs, pad, shared != 0, 4), step(len, B, nrhs, pad, false, 2);
            seed.each([](int i, long q, int k, long long j, double& d) { d = val(SEED, q, i, 10 * k + j); });
            CHECK(check_multi_strides(&seed.b, len, B, nrhs, true) == FBSTAB_HIP_OK, "%s", g_error.c_str());
            CHECK(check_multi_strides(&step.b, len, B, nrhs, false) == FBSTAB_HIP_OK, "%s", g_error.c_str());
            const long gaps = step.canaries();
            {
              MultiStage sd, st;
              const long mallocs0 = fb_shim::state().mallocs;
              CHECK(sd.open(&seed.b, len, B, nrhs, dev_ptrs != 0, true, nullptr) == FBSTAB_HIP_OK, "%s", g_error.c_str());
              CHECK(st.open(&step.b, len, B, nrhs, dev_ptrs != 0, false, nullptr) == FBSTAB_HIP_OK, "%s", g_error.c_str());
              if (dev_ptrs) CHECK(fb_shim::state().mallocs == mallocs0, "device pointers were staged");
              for (int i = 0; i < 3; i++) {
                CHECK((sd.k.base[i] != nullptr) == (seed.b.base[i] != nullptr), "seed slot %d", i);
                CHECK((st.k.base[i] != nullptr) == (step.b.base[i] != nullptr), "step slot %d", i);
                if (dev_ptrs && seed.b.base[i]) CHECK(sd.k.base[i] == seed.b.base[i], "seed slot %d is not the caller's", i);
                if (sd.k.base[i] && (shared || B == 1)) CHECK(sd.k.stride[i] == 0, "one block, stride %lld", sd.k.stride[i]);
              }
              // the kernel: reads every seed vector, writes every step vector
              seed.each([&](int i, long q, int k, long long j, double&) {
                for (long qq = q; qq < (shared ? B : q + 1); qq++) {
                  const double got = sd.k.base[i][qq * sd.k.stride[i] + k * (nrhs > 1 ? sd.k.rhs_stride[i] : 0) + j];
                  CHECK(got == val(SEED, q, i, 10 * k + j), "seed slot %d QP %ld vector %d reads %.17g", i, qq, k, got);
                }
              });
              step.each([&](int i, long q, int k, long long j, double&) {
                st.k.base[i][q * st.k.stride[i] + k * (nrhs > 1 ? st.k.rhs_stride[i] : 0) + j] = val(STEP, q, i, 10 * k + j);
              });
              if (!dev_ptrs) CHECK(st.download(&step.b, len, B, nrhs, nullptr) == FBSTAB_HIP_OK, "%s", g_error.c_str());
            }
            step.each([](int i, long q, int k, long long j, double& d) {
              CHECK(d == val(STEP, q, i, 10 * k + j), "step slot %d QP %ld vector %d index %lld holds %.17g", i, q, k, j, d);
            });
            // the doubles between a QP's vectors, and between QPs, stay as they were
            long written = 0;
            step.each([&](int, long, int, long long, double&) { written++; });
            CHECK(step.canaries() == gaps - written, "%ld canaries of %ld left", step.canaries(), gaps - written);
          }
  // one QP is at the base: strides that batch 2 refuses serve batch 1
  for (int nrhs : {1, 3}) {
    MultiBlock step(len, 1, nrhs, 0, false, 0);
    for (int i = 0; i < 3; i++) step.b.stride[i] = 1;
    CHECK(check_multi_strides(&step.b, len, 1, nrhs, false) == FBSTAB_HIP_OK, "%s", g_error.c_str());
    CHECK(check_multi_strides(&step.b, len, 2, nrhs, false) == FBSTAB_HIP_ERR_ARGUMENT, "accepted for batch 2");
    MultiStage st;
    CHECK(st.open(&step.b, len, 1, nrhs, false, false, nullptr) == FBSTAB_HIP_OK, "%s", g_error.c_str());
    step.each([&](int i, long, int k, long long j, double&) { st.k.base[i][k * len[i] + j] = val(STEP, 0, i, 10 * k + j); });
    CHECK(st.download(&step.b, len, 1, nrhs, nullptr) == FBSTAB_HIP_OK, "%s", g_error.c_str());
    step.each([](int i, long, int k, long long j, double& d) { CHECK(d == val(STEP, 0, i, 10 * k + j), "slot %d", i); });
  }
  CHECK(fb_shim::state().live == 0, "%ld allocations live", fb_shim::state().live);
}

// ---- probe_run: ONE packed QP whatever strides the caller wrote ------------------------------------------------------
void probes() {
  for (const Shape& sh : kShapes) {
    SolverBase h;
    init_handle(h, sh);
    const int n = (int)sh.arr.size();
    Placed data = place(sh.arr.data(), n, 1, PACKED), x = place(sh.var, 4, 1, PACKED);
    data.fill(DATA); x.fill(POINT, 7);
    fbstab_mpc_batch_t d = block_of<fbstab_mpc_batch_t>(data);
    fbstab_var_batch_t xv = block_of<fbstab_var_batch_t>(x);
    for (int i = 0; i < n; i++) d.stride[i] = -5;
    for (int i = 0; i < 4; i++) xv.stride[i] = 1;
    const long long nz = sh.var[0], nl = sh.var[1], nv = sh.var[2], n_in = nz + nl + nv, n_io = 3 * nz + 3 * nl + 2 * nv + 1;
    std::vector<double> io((size_t)n_io, canary());
    for (long long j = 0; j < n_in; j++) io[(size_t)j] = val(IO_IN, 0, 0, j);
    int launches = 0;
    int rc = probe_run(&h, &d, &xv, io.data(), [&](const fbstab_mpc_batch_t& a, const fbstab_var_batch_t& v, double* d_io) {
      launches++;
      expect_packed(a, data, n, "data");
      kernel_reads(a, data, DATA, n, "data");
      kernel_reads(v, x, POINT, 3, "x");
      for (long long j = 0; j < n_in; j++) CHECK(d_io[j] == val(IO_IN, 0, 0, j), "io %lld in", j);
      for (long long j = 0; j < n_io; j++) d_io[j] = val(IO_OUT, 0, 0, j);
      return (int)FBSTAB_HIP_OK;
    });
    CHECK(rc == FBSTAB_HIP_OK && launches == 1, "%s", g_error.c_str());
    for (long long j = 0; j < n_io; j++) CHECK(io[(size_t)j] == val(IO_OUT, 0, 0, j), "io %lld out", j);
    x.expect(POINT, 7, "the probe's point");
  }
  CHECK(fb_shim::state().live == 0, "%ld allocations live", fb_shim::state().live);
}

// ---- multi_run: the four many-right-hand-side entry points around their launch ------------------------------------
// mode 0: a seed block per QP; 1: one seed block for the batch (stride 0); 2: the seeds are generated in the kernel
// (seed == nullptr, nrhs from `sizes`).  with_gain: MPC's x0 mode, a gain block and no step block at all.
void multi_run_case(const Shape& sh, bool with_gain, int B, int nrhs, int pad, bool dev_ptrs, bool out_on_host, int mode) {
  const long long* len = sh.var;
  const int n = (int)sh.arr.size(), rows = B > 0 ? B : 1;
  const long long glen = 2;  // (nu x nx of kShapes[0])
  SolverBase h;
  init_handle(h, sh);
  Placed data = place(sh.arr.data(), n, B, pad ? RECORDS : PACKED), x = place(sh.var, 3, B, pad ? RECORDS : PACKED);
  data.fill(DATA);
  x.fill(POINT);
  fbstab_mpc_batch_t d = block_of<fbstab_mpc_batch_t>(data);
  fbstab_var_batch_t xv = block_of<fbstab_var_batch_t>(x);
  // gv is left out; of the steps dl is left out where there is one right-hand side
  MultiBlock seed(len, rows, nrhs, pad, mode == 1, 4), step(len, rows, nrhs, pad, false, nrhs == 1 ? 2 : 0);
  seed.each([](int i, long q, int k, long long j, double& v) { v = val(SEED, q, i, 10 * k + j); });
  // nl == 0: whatever the caller left in the l slots is dropped
  std::unique_ptr<double> junk(new double(canary()));
  if (len[1] == 0) {
    seed.b.base[1] = step.b.base[1] = junk.get();
    seed.b.stride[1] = step.b.stride[1] = seed.b.rhs_stride[1] = step.b.rhs_stride[1] = -7;
  }
  const fbstab_multi_var_batch_t* seed_arg = mode == 2 ? nullptr : &seed.b;
  const fbstab_multi_var_batch_t* step_arg = with_gain ? nullptr : &step.b;
  std::vector<double> gain((size_t)(rows * (glen + pad)), canary());
  std::vector<int> status((size_t)rows, -1);
  const long gaps = step.canaries();
  const int flags = dev_ptrs ? FBSTAB_HIP_DEVICE_POINTERS | (out_on_host ? FBSTAB_HIP_OUT_ON_HOST : 0) : 0;
  int launches = 0;
  auto sizes = [&](int* nr, long long* gain_len) {
    if (mode == 2) *nr = nrhs;
    if (with_gain) *gain_len = glen;
    return (int)FBSTAB_HIP_OK;
  };
  auto launch = [&](MultiLaunchArgs<fbstab_mpc_batch_t>& k) {
    launches++;
    CHECK(k.nrhs == nrhs && k.s == h.stream, "nrhs %d", k.nrhs);
    if (dev_ptrs) {
      expect_same(k.a, data, n, "data");
      expect_same(k.v, x, 3, "x");
      CHECK((k.d_st == status.data()) == !out_on_host, "status: %p", (void*)k.d_st);
    } else {
      expect_packed(k.a, data, n, "data");
      expect_packed(k.v, x, 3, "x");
    }
    kernel_reads(k.a, data, DATA, n, "data");
    kernel_reads(k.v, x, POINT, 3, "x");
    for (int i = 0; i < 3; i++) {
      const bool given = seed_arg && seed.b.base[i] && len[i] > 0, asked = step_arg && step.b.base[i] && len[i] > 0;
      CHECK((k.sd.base[i] != nullptr) == given, "seed slot %d: %p", i, (void*)k.sd.base[i]);
      CHECK((k.st.base[i] != nullptr) == asked, "step slot %d: %p", i, (void*)k.st.base[i]);
      if (dev_ptrs && given) CHECK(k.sd.base[i] == seed.b.base[i], "seed slot %d is not the caller's", i);
      if (dev_ptrs && asked) CHECK(k.st.base[i] == step.b.base[i], "step slot %d is not the caller's", i);
      for (long q = 0; q < B; q++)
        for (int r = 0; r < nrhs; r++)
          for (long long j = 0; j < len[i]; j++) {
            if (given) {
              const double got = k.sd.base[i][q * k.sd.stride[i] + r * (nrhs > 1 ? k.sd.rhs_stride[i] : 0) + j];
              CHECK(got == val(SEED, mode == 1 ? 0 : q, i, 10 * r + j), "seed slot %d QP %ld vector %d reads %.17g", i, q,
                    r, got);
            }
            if (asked)
              k.st.base[i][q * k.st.stride[i] + r * (nrhs > 1 ? k.st.rhs_stride[i] : 0) + j] = val(STEP, q, i, 10 * r + j);
          }
    }
    CHECK((k.gain != nullptr) == with_gain, "gain: %p", (void*)k.gain);
    if (with_gain) {
      if (dev_ptrs) CHECK(k.gain == gain.data() && k.gain_stride == (B > 1 ? glen + pad : 0), "gain is not the caller's");
      else CHECK(k.gain_stride == glen, "gain stride %lld", k.gain_stride);
      for (long q = 0; q < B; q++)
        for (long long j = 0; j < glen; j++) k.gain[q * k.gain_stride + j] = val(GAIN, q, 0, j);
    }
    for (int q = 0; q < B; q++) k.d_st[q] = 40 + q;
    return (int)FBSTAB_HIP_OK;
  };
  const long mallocs0 = fb_shim::state().mallocs, calls0 = fb_shim::state().calls;
  const int rc = multi_run(&h, B, &d, &xv, mode == 2 ? 0 : nrhs, seed_arg, step_arg, with_gain ? gain.data() : nullptr,
                           glen + pad, status.data(), flags, nullptr, sizes, launch);
  CHECK(rc == FBSTAB_HIP_OK, "%s", g_error.c_str());
  CHECK(launches == (B > 0), "%d launches for batch %d", launches, B);
  if (B == 0) CHECK(fb_shim::state().calls == calls0, "batch 0 made a device call");
  if (dev_ptrs)  // pass-through; OUT_ON_HOST: exactly the status buffer
    CHECK(fb_shim::state().mallocs - mallocs0 == (B > 0 && out_on_host ? 1 : 0), "%ld allocations",
          fb_shim::state().mallocs - mallocs0);
  long written = 0;
  if (B > 0 && step_arg) {
    step.each([&](int i, long q, int k, long long j, double& v) {
      written++;
      CHECK(v == val(STEP, q, i, 10 * k + j), "step slot %d QP %ld vector %d index %lld holds %.17g", i, q, k, j, v);
    });
  }
  // the doubles between a QP's vectors, between QPs, and of a call that asks for nothing stay as they were
  CHECK(step.canaries() == gaps - written, "%ld canaries of %ld left", step.canaries(), gaps - written);
  for (long q = 0; q < rows; q++)
    for (long long j = 0; j < glen + pad; j++) {
      const double got = gain[(size_t)(q * (glen + pad) + j)];
      if (with_gain && B > 0 && j < glen) CHECK(got == val(GAIN, q, 0, j), "gain QP %ld index %lld holds %.17g", q, j, got);
      else CHECK(is_canary(got), "gain QP %ld index %lld was written", q, j);
    }
  for (int q = 0; q < rows; q++) CHECK(status[q] == (B > 0 ? 40 + q : -1), "status %d: %d", q, status[q]);
  seed.each([](int i, long q, int k, long long j, double& v) {
    CHECK(v == val(SEED, q, i, 10 * k + j), "seed slot %d was written", i);
  });
  CHECK(is_canary(*junk), "the l slot of a handle with nl == 0 was written");
  data.expect(DATA, ~0u, "data after the call");
  data.gaps_intact("data");
  x.gaps_intact("x");
}

void multi_runs() {
  for (int si = 0; si < 3; si++)
    for (int with_gain = 0; with_gain < (si == 0 ? 2 : 1); with_gain++)
      for (int B : kBatches)
        for (int nrhs : {1, 3})
          for (int pad : {0, 1})
            for (int dev_ptrs = 0; dev_ptrs < 2; dev_ptrs++)
              for (int out_on_host = 0; out_on_host < (dev_ptrs ? 2 : 1); out_on_host++)
                for (int mode = with_gain ? 2 : 0; mode < 3; mode++)
                  multi_run_case(kShapes[si], with_gain != 0, B, nrhs, pad, dev_ptrs != 0, out_on_host != 0, mode);
  CHECK(fb_shim::state().live == 0, "%ld allocations live", fb_shim::state().live);
}

// ---- sweep_run and sweep_adjoint_run ------------------------------------------------------------------------------
// One call of either run with every argument in place (the logs [steps][batch][n], restated from
// include/fbstab_hip.h), for the groups below to take slots out of or to break.
struct SweepArgsStandIn {  // (what the driver copies to the device in SweepArgs' place)
  unsigned long long* stats;
  int* cnt;
  double tag;
};
constexpr int kWorkgroups = 4;
struct SweepCall {
  int N, nx, nu, nc, B, steps;
  Shape sh;
  long long nz, nl, nv;
  SolverBase h;
  SweepShape sp;
  SweepScratch scratch;
  Placed data, x, grad;
  fbstab_mpc_batch_t d;
  fbstab_var_batch_t xv;
  fbstab_mpc_grad_batch_t gr;
  std::vector<fbstab_solver_out_t> out;
  std::vector<double> A, Bm, log_z, log_l, log_v, log_x0, u_log, w, gu, gx, mu_log;
  std::vector<int> log_e, status;
  std::vector<unsigned long long> stats;
  std::vector<float> kernel_ms;
  fbstab_receding_plant_t plant;
  fbstab_sweep_log_t log;
  fbstab_sweep_scenario_t sc;
  int launches = 0;

  static size_t some(long long n) { return (size_t)(n > 0 ? n : 1); }  // (steps == 0: a pointer all the same)
  SweepCall(int N_, int nx_, int nu_, int nc_, int B_, int steps_, unsigned want = 0xfff)
      : N(N_), nx(nx_), nu(nu_), nc(nc_), B(B_), steps(steps_), sh(mpc_shape(N_, nx_, nu_, nc_)), nz(sh.var[0]),
        nl(sh.var[1]), nv(sh.var[2]), data(place(sh.arr.data(), 12, B_, RECORDS)), x(place(sh.var, 4, B_, RECORDS)),
        grad(place(sh.arr.data(), 12, B_, PACKED, 0, ~want & 0xfffu)), out(some(B_)), A(some((long long)nx_ * nx_)),
        Bm(some((long long)nx_ * nu_)) {
    init_handle(h, sh);
    h.workgroups = kWorkgroups;
    sp.N = N; sp.nx = nx; sp.nu = nu; sp.nc = nc;
    const long long sb = (long long)steps * B;
    log_z.assign(some(sb * nz), canary()); log_l.assign(some(sb * nl), canary()); log_v.assign(some(sb * nv), canary());
    log_x0.assign(some(sb * nx), canary()); log_e.assign(some(sb), 0);
    u_log.assign(some(sb * nu), canary()); w.assign(some(sb * nx), 0.25);
    gu.assign(some(sb * nu), 0.5); gx.assign(some(sb * nx), 0.75); mu_log.assign(some(sb * nx), canary());
    stats.assign(some(4LL * steps), ~0ull); kernel_ms.assign(some(steps), -1.f);
    status.assign(some(B), -1);
    d = block_of<fbstab_mpc_batch_t>(data);
    xv = block_of<fbstab_var_batch_t>(x);
    gr = block_of<fbstab_mpc_grad_batch_t>(grad);
    plant = fbstab_receding_plant_t{};
    plant.A = A.data(); plant.B = Bm.data();
    log = fbstab_sweep_log_t{};
    log.z = log_z.data(); log.l = log_l.data(); log.v = log_v.data(); log.x0 = log_x0.data(); log.eflag = log_e.data();
    sc = fbstab_sweep_scenario_t{};
    sc.w = w.data();
  }
  // (the handle's teardown frees what the sweep adjoint left with it)
  ~SweepCall() {
    if (scratch.seed) (void)hipFree(scratch.seed);
    if (scratch.tmp) (void)hipFree(scratch.tmp);
  }
  // the runs on callables that only count: what refusals and failed allocations need
  int sweep(SolverBase* handle, const fbstab_sweep_log_t* lg, const fbstab_sweep_scenario_t* scn) {
    return sweep_run<SweepArgsStandIn>(
        handle, sp, B, &d, &xv, out.data(), &plant, steps, u_log.data(), stats.data(), kernel_ms.data(), nullptr, lg, scn,
        [](SweepArgsStandIn*, unsigned long long*, int*) {},
        [&](hipStream_t, double*) { launches++; return (int)FBSTAB_HIP_OK; },
        [&](hipStream_t, int) { launches++; return (int)FBSTAB_HIP_OK; },
        [&](hipStream_t, const SweepStep&, int*, double*) { launches++; });
  }
  int adjoint(SolverBase* handle) {
    return sweep_adjoint_run(
        handle, sp, scratch, B, &d, &plant, steps, &log, gu.data(), gx.data(), 0.5, &gr, mu_log.data(), status.data(),
        nullptr, [&](hipStream_t, const fbstab_mpc_batch_t&, double*) { launches++; return (int)FBSTAB_HIP_OK; },
        [&](hipStream_t, const SweepCostateStep&, int, int) { launches++; },
        [&](AdjointLaunchArgs&, double) { launches++; return (int)FBSTAB_HIP_OK; });
  }
};

// path 0: one launch; 1: per step, the handle has no record instance; 2: per step by the environment's switch
void choose_path(SweepCall& c, int path) {
  c.sp.record = c.sp.adjoint_kernel = path != 1;
  if (path == 2) {
    setenv("FBSTAB_HIP_SWEEP_PER_STEP", "1", 1);
    setenv("FBSTAB_HIP_SWEEP_ADJOINT_PER_STEP", "1", 1);
  } else {
    unsetenv("FBSTAB_HIP_SWEEP_PER_STEP");
    unsetenv("FBSTAB_HIP_SWEEP_ADJOINT_PER_STEP");
  }
}

enum { W_LOG = 1, W_ULOG = 2, W_W = 4, W_STATS = 8, W_MS = 16 };
void sweep_case(int N, int nx, int nu, int nc, int path, int B, int steps, int with, int shift) {
  SweepCall c(N, nx, nu, nc, B, steps);
  choose_path(c, path);
  c.sc.shift = shift;
  if (!(with & W_W)) c.sc.w = nullptr;
  if ((with & W_LOG) && shift) c.log.l = c.log.x0 = nullptr;  // (a log of some of the arrays)
  const fbstab_sweep_log_t* lg = with & W_LOG ? &c.log : nullptr;
  const fbstab_sweep_scenario_t* scn = (with & W_W) || shift ? &c.sc : nullptr;
  double* const u_log = with & W_ULOG ? c.u_log.data() : nullptr;
  int fills = 0, ones = 0, solves = 0, plants = 0;
  const long long nz = c.nz, nl = c.nl, nv = c.nv;
  auto fill_args = [&](SweepArgsStandIn* a, unsigned long long* d_stats, int* d_ret) {
    fills++;
    for (int q = 0; q < B; q++) CHECK(d_ret[q] == 0, "retirement flag %d starts at %d", q, d_ret[q]);
    for (int i = 0; i < 4 * steps; i++) CHECK(d_stats[i] == 0, "counter %d starts at %llu", i, d_stats[i]);
    *a = SweepArgsStandIn{d_stats, d_ret, 4711.0};
  };
  auto one_launch = [&](hipStream_t s, double* d_args) {
    ones++;
    SweepArgsStandIn a;
    memcpy(&a, d_args, sizeof(a));
    CHECK(s == c.h.stream && fills == 1 && a.tag == 4711.0, "the device copy of the arguments");
    for (int i = 0; i < 4 * steps; i++) a.stats[i] = 1000 + i;
    return (int)FBSTAB_HIP_OK;
  };
  auto solve = [&](hipStream_t s, int k) {
    CHECK(s == c.h.stream && k == solves && plants == solves, "solve %d behind %d solves and %d plant steps", k, solves, plants);
    solves++;
    return (int)FBSTAB_HIP_OK;
  };
  // (a step writes every double it is given: the buffers are exactly [steps][batch][n] long)
  auto step_of = [&](const char* what, double* got, double* base, long long len, int k, bool given) {
    CHECK(got == (given ? base + (long long)k * B * len : nullptr), "%s of step %d", what, k);
    if (got)
      for (long long j = 0; j < B * len; j++) got[j] = val(SOL, k, 0, j);
  };
  auto plant_step = [&](hipStream_t s, const SweepStep& st, int* d_ret, double* d_xtmp) {
    const int k = st.k;
    CHECK(s == c.h.stream && k == plants && solves == plants + 1, "plant step %d behind %d solves", k, solves);
    plants++;
    step_of("log z", st.z, c.log_z.data(), nz, k, lg && lg->z);
    step_of("log l", st.l, c.log_l.data(), nl, k, lg && lg->l);
    step_of("log v", st.v, c.log_v.data(), nv, k, lg && lg->v);
    step_of("log x0", st.x0, c.log_x0.data(), nx, k, lg && lg->x0);
    step_of("u_log", st.u_log, c.u_log.data(), nu, k, u_log != nullptr);
    CHECK(st.eflag == (lg ? c.log_e.data() + (long long)k * B : nullptr), "log eflag of step %d", k);
    if (st.eflag)
      for (int q = 0; q < B; q++) st.eflag[q] = k;
    CHECK(st.w == (with & W_W ? c.w.data() + (long long)k * B * nx : nullptr), "disturbances of step %d", k);
    if (st.w)
      for (long long j = 0; j < (long long)B * nx; j++) CHECK(st.w[j] == 0.25, "disturbance %lld of step %d", j, k);
    CHECK(st.shift_stages == (shift && k + 1 < steps ? N : 0), "step %d shifts %d stages", k, st.shift_stages);
    for (int i = 0; i < 4; i++) {
      CHECK(st.stats[i] == 0, "counter %d of step %d starts at %llu", i, k, st.stats[i]);
      st.stats[i] = 1000 + 4 * k + i;
    }
    for (int q = 0; q < B; q++) CHECK(d_ret[q] == 0, "retirement flag %d", q);
    CHECK((d_xtmp != nullptr) == (nx > 64), "the plant step's state buffer: %p", (void*)d_xtmp);
    if (d_xtmp)
      for (long long j = 0; j < (long long)B * nx; j++) d_xtmp[j] = 0.0;
  };
  const long calls0 = fb_shim::state().calls;
  const int rc = sweep_run<SweepArgsStandIn>(&c.h, c.sp, B, &c.d, &c.xv, c.out.data(), &c.plant, steps, u_log,
                                             with & W_STATS ? c.stats.data() : nullptr,
                                             with & W_MS ? c.kernel_ms.data() : nullptr, nullptr, lg, scn, fill_args,
                                             one_launch, solve, plant_step);
  CHECK(rc == FBSTAB_HIP_OK, "%s", g_error.c_str());
  if (steps == 0) CHECK(fb_shim::state().calls == calls0, "a sweep of no steps made a device call");
  const bool one = path == 0 && steps > 0;
  CHECK(fills == one && ones == one && solves == (one ? 0 : steps) && plants == solves,
        "path %d: %d argument blocks, %d sweep launches, %d solves, %d plant steps", path, fills, ones, solves, plants);
  // written for `steps` entries (the vectors are exactly that long) where asked for, not at all otherwise
  for (int i = 0; i < 4 * steps; i++)
    CHECK(c.stats[(size_t)i] == (with & W_STATS ? 1000ull + i : ~0ull), "counter %d holds %llu", i, c.stats[(size_t)i]);
  for (int k = 0; k < steps; k++)
    CHECK(c.kernel_ms[(size_t)k] == (with & W_MS ? 0.f : -1.f), "time of step %d: %g", k, c.kernel_ms[(size_t)k]);
  c.data.gaps_intact("data");
  c.x.gaps_intact("x");
}

void sweeps() {
  for (int path = 0; path < 3; path++)
    for (int B : {1, 3})
      for (int steps : {0, 1, 3})
        for (int with = 0; with < 32; with++)
          for (int shift = 0; shift < 2; shift++) sweep_case(2, 2, 1, 1, path, B, steps, with, shift);
  sweep_case(1, 65, 1, 1, 1, 3, 2, 31, 1);  // more than 64 states: the plant step gets a buffer for the new ones
  // a record handle without a slot per trajectory, and with more steps than a row counts, runs per step
  for (int which = 0; which < 2; which++) {
    SweepCall c(2, 2, 1, 1, 3, which ? 0xffff : 2);
    choose_path(c, 0);
    if (!which) c.h.workgroups = 2;
    CHECK(c.sweep(&c.h, nullptr, nullptr) == FBSTAB_HIP_OK && c.launches == 2 * c.steps, "%d launches", c.launches);
  }
  choose_path(*std::unique_ptr<SweepCall>(new SweepCall(2, 2, 1, 1, 1, 0)), 0);  // (the environment as it was)
  CHECK(fb_shim::state().live == 0, "%ld allocations live", fb_shim::state().live);
}

enum { W_GU = 1, W_GX = 2, W_MU = 4 };
void sweep_adjoint_case(int path, int B, int steps, int with, unsigned want) {
  const int N = 2, nx = 2, nu = 1, nc = 1, qps = 2;
  SweepCall c(N, nx, nu, nc, B, steps, want);
  choose_path(c, path);
  c.sp.qps_per_wg = qps;
  c.d.base[FBSTAB_MPC_x0] = nullptr;  // (not read: the kernels get the logged states)
  const long long nz = c.nz, nl = c.nl, nv = c.nv, mb = kMaxBatch;
  const double* gu = with & W_GU ? c.gu.data() : nullptr;
  const double* gx = with & W_GX ? c.gx.data() : nullptr;
  double* mu_log = with & W_MU ? c.mu_log.data() : nullptr;
  auto data_of = [&](const fbstab_mpc_batch_t& a) {
    for (int i = 0; i < 12; i++) {
      if (i == FBSTAB_MPC_x0) CHECK(a.base[i] == c.log_z.data() && a.stride[i] == nz, "the x0 slot is not the logged z");
      else CHECK(a.base[i] == c.data.base[i] && a.stride[i] == (B == 1 ? 0 : c.data.stride[i]), "data slot %d", i);
    }
  };
  int ones = 0;
  std::vector<int> order;  // phase 0: 0; step k: 10 k + 1 (costate before), + 3 (adjoint), + 2 (costate behind)
  auto one_launch = [&](hipStream_t s, const fbstab_mpc_batch_t& a, double* seed) {
    ones++;
    data_of(a);
    CHECK(s == c.h.stream && seed == c.scratch.seed, "the seed vectors are not the handle's");
    // nz doubles per QP slot of the grid, zeroed (the allocation is exactly that long)
    CHECK(fb_shim::state().last_bytes == sizeof(double) * (size_t)(nz * kWorkgroups * qps), "%zu seed bytes",
          fb_shim::state().last_bytes);
    for (long long j = 0; j < nz * kWorkgroups * qps; j++) {
      CHECK(seed[j] == 0.0, "seed %lld", j);
      seed[j] = 1.0;
    }
    return (int)FBSTAB_HIP_OK;
  };
  // the carve-up of the per-step scratch, restated: per QP of max_batch the image of every sequence, nz, nx, nx
  // doubles and the status word in a double's place
  long long per_qp = nz + 2 * nx + 1;
  for (long long n : c.sh.arr) per_qp += n;
  const int* step_eflag = nullptr;
  auto costate = [&](hipStream_t s, const SweepCostateStep& k, int phase, int last) {
    CHECK(s == c.h.stream, "stream");
    double* w = c.scratch.tmp;
    if (phase == 0)
      CHECK(fb_shim::state().last_bytes == sizeof(double) * (size_t)(per_qp * mb), "%zu scratch bytes", fb_shim::state().last_bytes);
    for (int i = 0; i < 12; i++) {
      const bool wanted = (want >> i & 1) || i == FBSTAB_MPC_x0;
      CHECK(k.len[i] == c.sh.arr[(size_t)i] && k.tmp[i] == (wanted ? w : nullptr), "image slot %d", i);
      w += c.sh.arr[(size_t)i] * mb;
    }
    CHECK(k.seed == w && k.lam == w + nz * mb && k.atm == w + (nz + nx) * mb, "seed, lambda and A'mu");
    CHECK((double*)k.tmp_status == w + (nz + 2 * nx) * mb, "the status word sits behind the last double range");
    if (phase == 0) {  // every range written to its end, the status words of max_batch QPs included
      for (double* p = c.scratch.tmp; p < w + (nz + 2 * nx) * mb; p++) *p = 0.0;
      for (long long q = 0; q < mb; q++) k.tmp_status[q] = 0;
      CHECK(!k.eflag && !k.gu && !k.gx && !k.mu_log, "phase 0 has no step");
      order.push_back(0);
      return;
    }
    const int step = (int)((k.eflag - c.log_e.data()) / B);
    CHECK(k.eflag == c.log_e.data() + (long long)step * B, "eflag of step %d", step);
    CHECK(k.gu == (gu ? gu + (long long)step * B * nu : nullptr), "gu of step %d", step);
    CHECK(k.gx == (gx ? gx + (long long)step * B * nx : nullptr), "gx of step %d", step);
    CHECK(k.mu_log == (mu_log ? mu_log + (long long)step * B * nx : nullptr), "mu_log of step %d", step);
    if (k.mu_log && phase == 1)
      for (long long j = 0; j < (long long)B * nx; j++) k.mu_log[j] = val(ADJ, step, 0, j);
    CHECK(last == (phase == 2 && step == 0), "step %d phase %d: last = %d", step, phase, last);
    step_eflag = k.eflag;
    order.push_back(10 * step + phase);
  };
  auto adjoint = [&](AdjointLaunchArgs& st, double sigma) {
    const int step = (int)((st.v.base[0] - c.log_z.data()) / (B * nz));
    CHECK(sigma == 0.5 && st.s == c.h.stream, "sigma %g", sigma);
    data_of(st.a);
    CHECK(st.v.base[0] == c.log_z.data() + step * B * nz && st.v.stride[0] == nz, "z of step %d", step);
    CHECK(st.v.base[1] == c.log_l.data() + step * B * nl && st.v.stride[1] == nl, "l of step %d", step);
    CHECK(st.v.base[2] == c.log_v.data() + step * B * nv && st.v.stride[2] == nv, "v of step %d", step);
    CHECK(step_eflag == c.log_e.data() + (long long)step * B, "the adjoint of step %d is not behind its costate launch", step);
    double* w = c.scratch.tmp;
    for (int i = 0; i < 12; i++) {
      const bool wanted = (want >> i & 1) || i == FBSTAB_MPC_x0;
      CHECK(st.g.base[i] == (wanted ? w : nullptr) && st.g.stride[i] == c.sh.arr[(size_t)i], "gradient image slot %d", i);
      w += c.sh.arr[(size_t)i] * mb;
    }
    CHECK(st.sd.base[0] == w && st.sd.stride[0] == nz && !st.sd.base[1] && !st.sd.base[2], "the seed");
    CHECK(!st.ad.base[0] && !st.ad.base[1] && !st.ad.base[2], "no adjoint steps are taken");
    CHECK((double*)st.d_st == w + (nz + 2 * nx) * mb, "the step's status");
    order.push_back(10 * step + 3);
    return (int)FBSTAB_HIP_OK;
  };
  const int rc = sweep_adjoint_run(&c.h, c.sp, c.scratch, B, &c.d, &c.plant, steps, &c.log, gu, gx, 0.5, &c.gr, mu_log,
                                   c.status.data(), nullptr, one_launch, costate, adjoint);
  CHECK(rc == FBSTAB_HIP_OK, "%s", g_error.c_str());
  std::vector<int> expected;
  if (path != 0) {
    expected.push_back(0);
    for (int k = steps - 1; k >= 0; k--)
      for (int what : {1, 3, 2}) expected.push_back(10 * k + what);
  }
  CHECK(ones == (path == 0) && order == expected, "path %d: %d sweep launches, %zu per-step launches", path, ones, order.size());
  CHECK((c.scratch.seed != nullptr) == (path == 0) && (c.scratch.tmp != nullptr) == (path != 0), "the handle's scratch");
  for (long long j = 0; j < (long long)steps * B * nx; j++)
    CHECK(mu_log && path != 0 ? !is_canary(c.mu_log[(size_t)j]) : is_canary(c.mu_log[(size_t)j]), "mu_log %lld", j);
  // the caller's gradient slots and data are the kernels' business: the stage touches neither
  c.grad.expect_untouched(want, "gradient");
  c.data.gaps_intact("data");
}

void sweep_adjoints() {
  for (int path = 0; path < 3; path++)
    for (int B : {1, 3})
      for (int steps : {0, 1, 3})
        for (int with = 0; with < 8; with++)
          for (unsigned want : {0xfffu, 0u, 0x8a5u}) sweep_adjoint_case(path, B, steps, with, want);
  {  // a second call takes the scratch the first one left with the handle
    SweepCall c(2, 2, 1, 1, 3, 2);
    for (int path : {1, 0, 1, 0}) {
      choose_path(c, path);
      const long mallocs0 = fb_shim::state().mallocs;
      CHECK(c.adjoint(&c.h) == FBSTAB_HIP_OK, "%s", g_error.c_str());
      CHECK(fb_shim::state().mallocs - mallocs0 == (c.launches <= 8), "%ld allocations", fb_shim::state().mallocs - mallocs0);
    }
    CHECK(c.launches == 7 + 1 + 7 + 1, "%d launches", c.launches);
    choose_path(c, 0);
  }
  CHECK(fb_shim::state().live == 0, "%ld allocations live", fb_shim::state().live);
}

// ---- the refusals of the runs above: text, order, and not one device call ------------------------------------------
// `breakers` in the order of the checks: each alone gives its text, and of two at once the earlier one's.
template <class Call>
struct Breaker {
  const char* text;
  std::function<void(Call&)> brk;
};
template <class Call, class Make, class Run>
void ordered_refusals(const char* who, const std::vector<Breaker<Call>>& breakers, Make make, Run run) {
  for (size_t i = 0; i < breakers.size(); i++)
    for (size_t j = i; j < breakers.size(); j++) {
      std::unique_ptr<Call> c(make());
      breakers[j].brk(*c);
      breakers[i].brk(*c);
      g_error.clear();
      const long calls0 = fb_shim::state().calls;
      const int rc = run(*c);
      CHECK(rc == FBSTAB_HIP_ERR_ARGUMENT && g_error == breakers[i].text, "%s: %s (with %s): got %d \"%s\"", who,
            breakers[i].text, breakers[j].text, rc, g_error.c_str());
      CHECK(fb_shim::state().calls == calls0 && c->launches == 0, "%s: %s: %ld device calls, %d launches", who,
            breakers[i].text, fb_shim::state().calls - calls0, c->launches);
    }
}

struct MultiCall {
  const Shape& sh;
  SolverBase h;
  SolverBase* handle = &h;
  int B = kMaxBatch, nrhs = 3, launches = 0;
  bool sizes_refuse = false;
  Placed data, x;
  fbstab_mpc_batch_t d;
  const fbstab_mpc_batch_t* dp = &d;
  fbstab_var_batch_t xv;
  MultiBlock seed, step;
  std::vector<double> gain;
  long long gain_stride = 2;
  std::vector<int> status;
  explicit MultiCall(const Shape& s)
      : sh(s), data(place(s.arr.data(), (int)s.arr.size(), B, RECORDS)), x(place(s.var, 3, B, RECORDS)),
        seed(s.var, B, nrhs, 1, false, 0), step(s.var, B, nrhs, 1, false, 0), gain(2 * kMaxBatch), status(kMaxBatch) {
    init_handle(h, s);
    d = block_of<fbstab_mpc_batch_t>(data);
    xv = block_of<fbstab_var_batch_t>(x);
  }
  int run() {
    return multi_run(
        handle, B, dp, &xv, nrhs, &seed.b, &step.b, gain.data(), gain_stride, status.data(), 0, nullptr,
        [&](int*, long long* gain_len) {
          *gain_len = 2;
          // (the text of fbstab_hip_dense_jacobian_batch's refusal, which the wrapper makes here)
          return sizes_refuse ? fail(FBSTAB_HIP_ERR_ARGUMENT, "dense jacobian: wrt = h on a handle without equality constraints")
                              : (int)FBSTAB_HIP_OK;
        },
        [&](MultiLaunchArgs<fbstab_mpc_batch_t>&) { launches++; return (int)FBSTAB_HIP_OK; });
  }
};

// The order all four entry points have always had behind their own checks (fbstab_hip_mpc_kkt_solve_batch,
// _x0_sensitivity_batch, fbstab_hip_dense_kkt_solve_batch, _jacobian_batch; the gain is MPC's, the refusal of `sizes`
// the dense Jacobian's): handle, null arguments, batch, what takes nrhs from the handle, null data, null point, the
// point's strides, the seeds' and the steps' (slot by slot: rhs_stride, then stride), the gain's, the data's.
void multi_run_refusals() {
  for (const Shape& sh : kShapes) {
    std::vector<Breaker<MultiCall>> b = {
        {"null solver handle", [](MultiCall& c) { c.handle = nullptr; }},
        {"null argument", [](MultiCall& c) { c.dp = nullptr; }},
        {"batch exceeds the max_batch the handle was created with", [](MultiCall& c) { c.B = kMaxBatch + 1; }},
        {"dense jacobian: wrt = h on a handle without equality constraints", [](MultiCall& c) { c.sizes_refuse = true; }},
        {"null problem data pointer", [](MultiCall& c) { c.d.base[4] = nullptr; }},
        {"null variable pointer", [](MultiCall& c) { c.xv.base[2] = nullptr; }},
        {"variable stride smaller than the vector length", [](MultiCall& c) { c.xv.stride[0] = 1; }},
        {"seed rhs_stride smaller than the vector length", [](MultiCall& c) { c.seed.b.rhs_stride[0] = 0; }},
        {"seed stride smaller than the right-hand sides of one QP", [](MultiCall& c) { c.seed.b.stride[0] = 1; }},
        {"step rhs_stride smaller than the vector length", [](MultiCall& c) { c.step.b.rhs_stride[0] = 0; }},
        {"step stride smaller than the right-hand sides of one QP", [](MultiCall& c) { c.step.b.stride[0] = 0; }},
        {"gain stride smaller than nu x nx", [](MultiCall& c) { c.gain_stride = 1; }},
        {"problem data stride smaller than the array length", [](MultiCall& c) { c.d.stride[0] = 1; }},
    };
    ordered_refusals<MultiCall>("multi_run", b, [&] { return new MultiCall(sh); }, [](MultiCall& c) { return c.run(); });
    // batch 1: the strides are not read, and a gain stride below nu x nx serves
    MultiCall one(sh);
    one.B = 1;
    one.gain_stride = 0;
    one.xv.stride[0] = one.d.stride[0] = 0;
    for (int i = 0; i < 3; i++) one.seed.b.stride[i] = one.step.b.stride[i] = 0;
    CHECK(one.run() == FBSTAB_HIP_OK && one.launches == 1, "%s", g_error.c_str());
  }
}

void sweep_refusals() {
  auto make = [] { return new SweepCall(2, 2, 1, 1, kMaxBatch, 2); };
  const char* kBatch = "batch exceeds the max_batch the handle was created with";
  const char* kData = "problem data stride smaller than the array length";
  // fbstab_hip_mpc_receding_sweep, _logged and _scenario (the last one alone can be refused for its shift)
  for (int entry = 0; entry < 3; entry++) {
    std::vector<Breaker<SweepCall>> b;
    b.push_back({kBatch, [](SweepCall& c) { c.B = kMaxBatch + 1; }});
    b.push_back({"plant matrices and a non-negative step count are required", [](SweepCall& c) { c.plant.B = nullptr; }});
    if (entry == 2) b.push_back({"receding sweep scenario: shift is 0 or 1", [](SweepCall& c) { c.sc.shift = 2; }});
    b.push_back({"null problem data pointer", [](SweepCall& c) { c.d.base[7] = nullptr; }});
    b.push_back({"null variable pointer", [](SweepCall& c) { c.xv.base[3] = nullptr; }});
    b.push_back({"receding sweep: every trajectory needs its own x0 (stride >= nx)",
                 [](SweepCall& c) { c.d.stride[FBSTAB_MPC_x0] = 0; }});
    b.push_back({kData, [](SweepCall& c) { c.d.stride[2] = 1; }});
    b.push_back({"variable stride smaller than the vector length", [](SweepCall& c) { c.xv.stride[1] = 0; }});
    ordered_refusals<SweepCall>("sweep_run", b, make, [=](SweepCall& c) {
      return c.sweep(&c.h, entry > 0 ? &c.log : nullptr, entry > 1 ? &c.sc : nullptr);
    });
    // the handle and the null arguments come first
    SweepCall c(2, 2, 1, 1, kMaxBatch + 1, 2);
    g_error.clear();
    CHECK(c.sweep(nullptr, nullptr, nullptr) == FBSTAB_HIP_ERR_ARGUMENT && g_error == "null solver handle", "%s", g_error.c_str());
    CHECK(sweep_run<SweepArgsStandIn>(&c.h, c.sp, c.B, &c.d, nullptr, c.out.data(), &c.plant, 2, nullptr, nullptr, nullptr,
                                      nullptr, nullptr, nullptr, [](SweepArgsStandIn*, unsigned long long*, int*) {},
                                      [](hipStream_t, double*) { return 0; }, [](hipStream_t, int) { return 0; },
                                      [](hipStream_t, const SweepStep&, int*, double*) {}) == FBSTAB_HIP_ERR_ARGUMENT &&
              g_error == "null argument", "%s", g_error.c_str());
    c.steps = -1;
    c.B = kMaxBatch;
    CHECK(c.sweep(&c.h, nullptr, nullptr) == FBSTAB_HIP_ERR_ARGUMENT &&
              g_error == "plant matrices and a non-negative step count are required", "%s", g_error.c_str());
    CHECK(c.launches == 0, "a refused sweep was launched");
  }
  // fbstab_hip_mpc_receding_sweep_adjoint: what needs no handle, then the handle, then slot by slot the data
  // pointer, the data stride and the gradient stride
  std::vector<Breaker<SweepCall>> b = {
      {"sweep adjoint: the log's z, l, v and eflag are required", [](SweepCall& c) { c.log.v = nullptr; }},
      {"sweep adjoint: negative step count", [](SweepCall& c) { c.steps = -1; }},
      {"sweep adjoint: plant matrices are required", [](SweepCall& c) { c.plant.A = nullptr; }},
      {"sweep adjoint: a gradient slot of stride 0 (summed over the batch) is not served",
       [](SweepCall& c) { c.gr.stride[11] = 0; }},
      {kBatch, [](SweepCall& c) { c.B = kMaxBatch + 1; }},
      {"gradient stride smaller than the array length", [](SweepCall& c) { c.gr.stride[0] = 1; }},
      {"null problem data pointer", [](SweepCall& c) { c.d.base[1] = nullptr; }},
      {kData, [](SweepCall& c) { c.d.stride[1] = 1; }},
      {"gradient stride smaller than the array length", [](SweepCall& c) { c.gr.stride[1] = 1; }},
      {kData, [](SweepCall& c) { c.d.stride[10] = -1; }},
  };
  ordered_refusals<SweepCall>("sweep_adjoint_run", b, make, [](SweepCall& c) { return c.adjoint(&c.h); });
  SweepCall c(2, 2, 1, 1, kMaxBatch + 1, 2);
  g_error.clear();
  CHECK(c.adjoint(nullptr) == FBSTAB_HIP_ERR_ARGUMENT && g_error == "null solver handle", "%s", g_error.c_str());
  c.gr.stride[3] = 0;
  CHECK(c.adjoint(nullptr) == FBSTAB_HIP_ERR_ARGUMENT &&
            g_error == "sweep adjoint: a gradient slot of stride 0 (summed over the batch) is not served", "%s", g_error.c_str());
  CHECK(sweep_adjoint_run(nullptr, c.sp, c.scratch, c.B, &c.d, &c.plant, -1, nullptr, nullptr, nullptr, 0.0, &c.gr, nullptr,
                          c.status.data(), nullptr, [](hipStream_t, const fbstab_mpc_batch_t&, double*) { return 0; },
                          [](hipStream_t, const SweepCostateStep&, int, int) {},
                          [](AdjointLaunchArgs&, double) { return 0; }) == FBSTAB_HIP_ERR_ARGUMENT &&
            g_error == "sweep adjoint: null log", "%s", g_error.c_str());
  CHECK(sweep_adjoint_run(&c.h, c.sp, c.scratch, c.B, &c.d, &c.plant, 2, &c.log, nullptr, nullptr, 0.0, &c.gr, nullptr,
                          nullptr, nullptr, [](hipStream_t, const fbstab_mpc_batch_t&, double*) { return 0; },
                          [](hipStream_t, const SweepCostateStep&, int, int) {},
                          [](AdjointLaunchArgs&, double) { return 0; }) == FBSTAB_HIP_ERR_ARGUMENT &&
            g_error == "null argument", "%s", g_error.c_str());
  // one trajectory: its strides are not read, a shared x0 and a gradient slot of stride 0 included
  for (int adjoint = 0; adjoint < 2; adjoint++) {
    SweepCall one(2, 2, 1, 1, 1, 2);
    for (int i = 0; i < 12; i++) one.d.stride[i] = one.gr.stride[i] = 0;
    for (int i = 0; i < 4; i++) one.xv.stride[i] = 0;
    CHECK((adjoint ? one.adjoint(&one.h) : one.sweep(&one.h, &one.log, &one.sc)) == FBSTAB_HIP_OK && one.launches > 0,
          "%s", g_error.c_str());
  }
}

// ... and their allocations: the n-th one fails, the call says so, and nothing stays behind but the sweep
// adjoint's scratch, which is the handle's (SweepCall's teardown frees it as the handle's does)
void new_run_leaks() {
  for (int what = 0; what < 5; what++) {
    bool done = false;
    for (int nth = 1; !done && nth < 64; nth++) {
      {
        std::unique_ptr<MultiCall> m;
        std::unique_ptr<SweepCall> c;
        if (what == 0) m.reset(new MultiCall(kShapes[0]));
        else c.reset(new SweepCall(1, 65, 1, 1, kMaxBatch, 2));
        if (c) choose_path(*c, what == 1 || what == 3 ? 0 : 1);
        fb_shim::state().fail_malloc_at = fb_shim::state().mallocs + nth;
        const int rc = what == 0 ? m->run() : what < 3 ? c->sweep(&c->h, &c->log, &c->sc) : c->adjoint(&c->h);
        done = fb_shim::state().fail_malloc_at != 0;  // the call made fewer allocations than nth: it went through
        fb_shim::state().fail_malloc_at = 0;
        CHECK(rc == (done ? FBSTAB_HIP_OK : FBSTAB_HIP_ERR_DEVICE), "run %d, allocation %d: %d %s", what, nth, rc,
              g_error.c_str());
        if (!done) CHECK(g_error.find("out of memory") != std::string::npos, "%s", g_error.c_str());
      }
      CHECK(fb_shim::state().live == 0, "run %d, allocation %d failed: %ld allocations live", what, nth,
            fb_shim::state().live);
    }
    CHECK(done, "run %d never went through", what);
  }
}

// ---- refusals that take the handle's lengths: code, text, and not one device call ----------------------------------
struct Refusal {
  SolverBase h;
  const Shape& sh;
  int n, B = kMaxBatch;
  Placed data, x, seed, adj, grad, dir, rhs;
  fbstab_mpc_batch_t d, dd;
  fbstab_mpc_grad_batch_t gr;
  fbstab_var_batch_t xv, sv, av, rv;
  std::vector<fbstab_solver_out_t> out;
  std::vector<int> status;
  explicit Refusal(const Shape& s)
      : sh(s), n((int)s.arr.size()), data(place(s.arr.data(), n, B, RECORDS)), x(place(s.var, 4, B, RECORDS)),
        seed(place(s.var, 3, B, RECORDS)), adj(place(s.var, 3, B, RECORDS)), grad(place(s.arr.data(), n, B, RECORDS)),
        dir(place(s.arr.data(), n, B, RECORDS)), rhs(place(s.var, 3, B, RECORDS)), out(8), status(8) {
    init_handle(h, s);
    d = block_of<fbstab_mpc_batch_t>(data); dd = block_of<fbstab_mpc_batch_t>(dir);
    gr = block_of<fbstab_mpc_grad_batch_t>(grad);
    xv = block_of<fbstab_var_batch_t>(x); sv = block_of<fbstab_var_batch_t>(seed);
    av = block_of<fbstab_var_batch_t>(adj); rv = block_of<fbstab_var_batch_t>(rhs);
  }
  int solve() {
    return solve_run(&h, B, &d, &xv, out.data(), 0, nullptr, nullptr,
                     [](hipStream_t, const fbstab_mpc_batch_t&, const fbstab_var_batch_t&, fbstab_solver_out_t*) {
                       CHECK(false, "a refused solve was launched");
                       return (int)FBSTAB_HIP_OK;
                     },
                     [](hipStream_t, const fbstab_mpc_batch_t&, const fbstab_var_batch_t&, double*) {});
  }
  int adjoint(bool reduced = false) {
    return adjoint_run(&h, B, &d, &xv, &sv, 0.5, &gr, &av, status.data(), nullptr, 0, nullptr, reduced,
                       grad_reduce_plan_dense((int)sh.var[0], (int)sh.var[1], (int)sh.var[2]), adjoint_launch,
                       reduce_launch);
  }
  int tangent_check() { return TangentStage::check(&h, B, dd.base, dd.stride, &av, &rv); }
};

template <class Break, class Call>
void refused(const Shape& sh, const char* text, Break brk, Call call) {
  Refusal r(sh);
  brk(r);
  g = Ctx{};
  g_error.clear();
  const long calls0 = fb_shim::state().calls;
  const int rc = call(r);
  CHECK(rc == FBSTAB_HIP_ERR_ARGUMENT && g_error == text, "%s: got %d \"%s\"", text, rc, g_error.c_str());
  CHECK(fb_shim::state().calls == calls0, "%s: %ld device calls", text, fb_shim::state().calls - calls0);
  CHECK(g.launches == 0, "%s: launched", text);
}

void refusals() {
  auto solve = [](Refusal& r) { return r.solve(); };
  auto adjoint = [](Refusal& r) { return r.adjoint(); };
  auto tangent = [](Refusal& r) { return r.tangent_check(); };
  const char* kData = "problem data stride smaller than the array length";
  const char* kVar = "variable stride smaller than the vector length";
  const char* kGrad = "gradient stride smaller than the array length";
  for (const Shape& sh : kShapes) {
    const int n = (int)sh.arr.size();
    for (int i = 0; i < n; i++) {
      if (sh.arr[i] == 0) continue;
      for (long long bad : {1LL, sh.arr[i] - 1, -1LL, -sh.arr[i]}) {
        if (bad >= sh.arr[i] || bad == 0) continue;
        refused(sh, kData, [&](Refusal& r) { r.d.stride[i] = bad; }, solve);
        refused(sh, kData, [&](Refusal& r) { r.d.stride[i] = bad; }, adjoint);
        refused(sh, kGrad, [&](Refusal& r) { r.gr.stride[i] = bad; }, adjoint);
        if (bad > 0)
          refused(sh, "perturbation stride is neither 0 nor at least the array length",
                  [&](Refusal& r) { r.dd.stride[i] = bad; }, tangent);
      }
      refused(sh, kGrad, [&](Refusal& r) { r.gr.stride[i] = 0; }, adjoint);  // stride 0 without `reduced`
      refused(sh, "null problem data pointer", [&](Refusal& r) { r.d.base[i] = nullptr; }, solve);
      refused(sh, "null problem data pointer", [&](Refusal& r) { r.d.base[i] = nullptr; }, adjoint);
    }
    for (int i = 0; i < 4; i++) {
      if (sh.var[i] == 0) continue;
      for (long long bad : {0LL, sh.var[i] - 1, -1LL}) {
        refused(sh, kVar, [&](Refusal& r) { r.xv.stride[i] = bad; }, solve);
        if (i == 3) continue;
        refused(sh, kVar, [&](Refusal& r) { r.xv.stride[i] = bad; }, adjoint);
        refused(sh, "seed stride smaller than the vector length", [&](Refusal& r) { r.sv.stride[i] = bad; }, adjoint);
        refused(sh, "adjoint stride smaller than the vector length", [&](Refusal& r) { r.av.stride[i] = bad; }, adjoint);
        refused(sh, "right-hand side stride smaller than the vector length",
                [&](Refusal& r) { r.rv.stride[i] = bad; }, tangent);
      }
      refused(sh, "null variable pointer", [&](Refusal& r) { r.xv.base[i] = nullptr; }, solve);
      if (i == 3) continue;
      refused(sh, "null variable pointer", [&](Refusal& r) { r.xv.base[i] = nullptr; }, adjoint);
      refused(sh, "null tangent pointer (dx)", [&](Refusal& r) { r.av.base[i] = nullptr; }, tangent);
      refused(sh, "null right-hand side pointer (rhs)", [&](Refusal& r) { r.rv.base[i] = nullptr; }, tangent);
    }
    refused(sh, "null seed pointer (z)", [&](Refusal& r) { r.sv.base[0] = nullptr; }, adjoint);
    const char* kBatch = "batch exceeds the max_batch the handle was created with";
    refused(sh, kBatch, [](Refusal& r) { r.B = kMaxBatch + 1; }, solve);
    refused(sh, kBatch, [](Refusal& r) { r.B = -1; }, solve);
    // the many-right-hand-side blocks: rhs_stride below the length, a QP stride below the span of its vectors
    for (int seed = 0; seed < 2; seed++)
      for (int i = 0; i < 3; i++) {
        if (sh.var[i] == 0) continue;
        auto multi_refused = [&](const char* text, int B, int nrhs, long long rs, long long st) {
          MultiBlock b(sh.var, B, nrhs, 0, false, 0);
          b.b.rhs_stride[i] = rs;
          b.b.stride[i] = st;
          g_error.clear();
          const long calls0 = fb_shim::state().calls;
          const int rc = check_multi_strides(&b.b, sh.var, B, nrhs, seed != 0);
          CHECK(rc == FBSTAB_HIP_ERR_ARGUMENT && g_error == text, "%s: got %d \"%s\"", text, rc, g_error.c_str());
          CHECK(fb_shim::state().calls == calls0, "%s: device calls", text);
        };
        const long long len = sh.var[i];
        multi_refused(seed ? "seed rhs_stride smaller than the vector length" : "step rhs_stride smaller than the vector length",
                      1, 3, len - 1, 3 * len);
        const char* span = seed ? "seed stride smaller than the right-hand sides of one QP"
                                : "step stride smaller than the right-hand sides of one QP";
        multi_refused(span, 3, 3, len, 3 * len - 1);
        multi_refused(span, 3, 1, len, len - 1 > 0 || !seed ? len - 1 : -1);
        if (!seed) multi_refused(span, 3, 3, len, 0);  // (a step block is never shared)
      }
  }
  multi_run_refusals();
  sweep_refusals();
  CHECK(fb_shim::state().live == 0, "%ld allocations live", fb_shim::state().live);
}

// ---- a handle whose calls fail half-way holds nothing once it is gone ---------------------------------------------
void leaks() {
  for (const Shape& sh : kShapes)
    for (int what = 0; what < 3; what++) {
      bool done = false;
      for (int nth = 1; !done && nth < 64; nth++) {
        {
          Refusal r(sh);
          g = Ctx{};
          g.sh = &sh; g.B = r.B; g.n = r.n; g.data = &r.data; g.x = &r.x; g.seed = &r.seed; g.grad = &r.grad;
          g.adj = &r.adj;
          r.data.fill(DATA); r.x.fill(POINT, 7); r.seed.fill(SEED);
          fb_shim::state().fail_malloc_at = fb_shim::state().mallocs + nth;
          int rc;
          if (what == 0) {
            std::vector<double> norms(4 * kMaxBatch);
            rc = solve_run(&r.h, r.B, &r.d, &r.xv, r.out.data(), 0, nullptr, norms.data(),
                           [](hipStream_t, const fbstab_mpc_batch_t&, const fbstab_var_batch_t&, fbstab_solver_out_t*) {
                             return (int)FBSTAB_HIP_OK;
                           },
                           [](hipStream_t, const fbstab_mpc_batch_t&, const fbstab_var_batch_t&, double*) {});
          } else if (what == 1) {
            for (int i = 0; i < r.n; i += 2) r.gr.stride[i] = 0;
            for (int i = 0; i < r.n; i += 2) g.reduced |= sh.arr[i] > 0 ? 1u << i : 0;
            g.adj = nullptr;
            r.av = fbstab_var_batch_t{};
            // (the lambdas' placement checks are the other groups' business: only the allocations matter here)
            rc = adjoint_run(&r.h, r.B, &r.d, &r.xv, &r.sv, 0.5, &r.gr, nullptr, r.status.data(), r.out.data(), 0,
                             nullptr, true, grad_reduce_plan_dense((int)sh.var[0], (int)sh.var[1], (int)sh.var[2]),
                             +[](SolverBase*, int, AdjointLaunchArgs&, double) { return (int)FBSTAB_HIP_OK; },
                             +[](const GradReduceArgs&, const GradReduceOut&, hipStream_t) { return (int)FBSTAB_HIP_OK; });
          } else {
            rc = tangent_run(&r.h, r.B, &r.d, &r.xv, &r.dd, 0.5, &r.av, &r.rv, r.status.data(), 0, nullptr,
                             (const void*)&g, [](const fbstab_mpc_batch_t&, const AdjointLaunchArgs&) {},
                             +[](SolverBase*, int, AdjointLaunchArgs&, double) { return (int)FBSTAB_HIP_OK; });
          }
          done = fb_shim::state().fail_malloc_at != 0;  // the call made fewer allocations than nth: it went through
          fb_shim::state().fail_malloc_at = 0;
          CHECK(rc == (done ? FBSTAB_HIP_OK : FBSTAB_HIP_ERR_DEVICE), "call %d, allocation %d: %d %s", what, nth, rc,
                g_error.c_str());
          if (!done) CHECK(g_error.find("out of memory") != std::string::npos, "%s", g_error.c_str());
        }
        CHECK(fb_shim::state().live == 0, "call %d, allocation %d failed: %ld allocations live", what, nth,
              fb_shim::state().live);
      }
      CHECK(done, "call %d never went through", what);
    }
  new_run_leaks();
}

}  // namespace

int main(int argc, char** argv) {
  const std::string group = argc > 1 ? argv[1] : "";
  if (group == "solve") solves(false);
  else if (group == "solve_device_pointers") solves(true);
  else if (group == "adjoint") adjoints();
  else if (group == "tangent") tangents();
  else if (group == "multi") multi();
  else if (group == "multi_run") multi_runs();
  else if (group == "sweep") sweeps();
  else if (group == "sweep_adjoint") sweep_adjoints();
  else if (group == "probe") probes();
  else if (group == "refusals") refusals();
  else if (group == "leaks") leaks();
  else return 2;
  if (g_failures) std::printf("%d checks failed\n", g_failures);
  return g_failures ? 1 : 0;
}
