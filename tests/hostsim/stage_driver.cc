// TEST INFRASTRUCTURE ONLY - the driver of tests/test_host_stage.py: fbstab_amd/csrc/fb_host_stage.h over the
// heap-backed runtime of runtime_shim/, bare SolverBase objects with the lengths the create functions set, and host
// lambdas in the kernels' place.  A lambda reads every input double through the kernel-side base / stride and
// writes every output double with a value that names its kind, QP, slot and index (val below); the driver then looks
// for those values where include/fbstab_hip.h says QP q of a slot lives: base + q * stride, one row for stride 0,
// at the base for batch 1 - restated here, not taken from the header under test.
//
// usage: stage_driver <group>; prints one line per failed check and exits 1, prints nothing and exits 0 otherwise.
#include "fb_host_stage.h"

#include <cstdint>
#include <cstdio>
#include <memory>

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

enum Tag { DATA = 1, POINT, SEED, DIR, SOL, GRAD, ADJ, RHS, STEP, NORM, RES, SUM, IO_IN, IO_OUT };
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
}

}  // namespace

int main(int argc, char** argv) {
  const std::string group = argc > 1 ? argv[1] : "";
  if (group == "solve") solves(false);
  else if (group == "solve_device_pointers") solves(true);
  else if (group == "adjoint") adjoints();
  else if (group == "tangent") tangents();
  else if (group == "multi") multi();
  else if (group == "probe") probes();
  else if (group == "refusals") refusals();
  else if (group == "leaks") leaks();
  else return 2;
  if (g_failures) std::printf("%d checks failed\n", g_failures);
  return g_failures ? 1 : 0;
}
