// Test-only probe library over fb_dense.h: one small kernel per STAGE of the four-wavefront dense policy
// (DenseProblem<C, KGLOBAL, VGLOBAL>), so that tests/test_gpu_dense_stages.py can hold each stage to an
// extended-precision reference and to the rounding bounds of tests/dense_rules.py instead of through a whole
// solve.  Never linked into libfbstab_hip.so; built by `make -C fbstab_amd/csrc denseprobe` into
// tests/_build/libdense_probe.so with the product's flags.
//
// Every kernel runs ONE workgroup per QP (workgroup q = QP q).  The layout comes from DenseLayout::init(nz, nl,
// nv, nt) and the instance - <Ctx<256>>, <Ctx<256>, true>, <Ctx<256>, true, true>, <Ctx<64>> - from its k_global
// and v_global exactly as fbstab_hip_dense_create and fbstab_dense_kernel choose it, the fall-back from 64 to 256
// threads (K in global scratch, or A not in LDS) included.  Dynamic LDS is lay.lds_doubles doubles, global scratch
// k_doubles + v_doubles per QP.  Each stage of DenseProblem is called UNCHANGED; no function of fb_dense.h is
// restated here.  Inputs are per-QP blocks (QP q at base + q * length, the lengths those of the shape); every load
// of the probe itself is at an index below the length of its block (i < nz / nl / nv / nk, e < nk * nk), every store
// to row q < count of an output of `count` rows of that length.
//
// Each entry point takes device pointers, the shape, the requested workgroup width (256 or 64) and the QP count,
// launches on the null stream, synchronises and returns the hipError_t (hipErrorInvalidValue for a shape or a
// width the policy does not take).
#include "fb_dense.h"

using namespace fbk;

namespace {

constexpr int kLdsLimit = 160 * 1024;

// One call's problem data and point, QP q at base + q * (length of the shape)
struct Blocks {
  const double *H, *f, *G, *h, *A, *b, *z, *l, *v;
};

template <class P>
__device__ __forceinline__ void bind_qp(P& p, const DenseLayout& lay, const Blocks& B, long q, lds_ptr lds,
                                        double* scratch) {
  const long nz = lay.nz, nl = lay.nl, nv = lay.nv;
  DenseData D;
  D.H = B.H + q * nz * nz; D.f = B.f + q * nz;
  D.G = B.G + q * nl * nz; D.h = B.h + q * nl;
  D.A = B.A + q * nv * nz; D.b = B.b + q * nv;
  // (the stages probed here only read the caller's point; uy is never touched)
  p.bind(lay, D, const_cast<double*>(B.z + q * nz), const_cast<double*>(B.l + q * nl),
         const_cast<double*>(B.v + q * nv), nullptr, lds, scratch + q * (lay.k_doubles + lay.v_doubles));
}

// what a factorisation leaves: the K region (L and D, or the multipliers of ldlt_rows), perm, and - where the
// layout has them (lay.wave, K in LDS) - the pivots and the elimination steps of ldlt_rows
struct FactorOut {
  int* verdict;   // [count]
  int* perm;      // [count, nk]
  double* Kout;   // [count, nk * nk]
  double* dpiv;   // [count, 64]
  int* ord;       // [count, 64]
};

template <class P, class C>
__device__ __forceinline__ void write_factors(const P& p, const C& c, const FactorOut& o, long q, bool rows) {
  const int n = p.lay.nk;
  for (int i = c.tid; i < n; i += C::nt) o.perm[q * n + i] = p.perm[i];
  for (long e = c.tid; e < (long)n * n; e += C::nt) o.Kout[q * n * n + e] = p.K[e];
  if (rows) {
    for (int t = c.tid; t < 64; t += C::nt) {
      o.dpiv[q * 64 + t] = (p.lds + p.lay.o_dpiv)[t];
      o.ord[q * 64 + t] = ((FB_LDS int*)(p.lds + p.lay.o_ord))[t];
    }
  }
}

// ---- the stages: Args (plain pointers and numbers) and run(p, ctx, args, q) --------------------------------------
// load_guess, residual, forcing_norm; and, where A sits in LDS, that copy read back through A_row_dot and
// A_col_dot on unit vectors (dz and dv hold them)
struct Products {
  struct Args {
    double *y, *rz, *rl, *nrm, *a_rows, *a_cols;  // a_rows, a_cols: [count, nv * nz] by columns, like A
  };
  template <class P, class C>
  static __device__ __forceinline__ void run(P& p, const C& c, const Args& a, long q) {
    const int nz = p.nz, nl = p.nl, nv = p.nv;
    p.load_guess(c);
    p.residual(c);
    const double nrm = p.forcing_norm(c);
    for (int i = c.tid; i < nv; i += C::nt) a.y[q * nv + i] = p.y[i];
    for (int i = c.tid; i < nz; i += C::nt) a.rz[q * nz + i] = p.rz[i];
    for (int i = c.tid; i < nl; i += C::nt) a.rl[q * nl + i] = p.rl[i];
    if (c.tid == 0) a.nrm[q] = nrm;
    if (!p.lay.a_lds) return;  // (uniform)
    for (int k = 0; k < nz; k++) {
      for (int i = c.tid; i < nz; i += C::nt) p.dz[i] = i == k ? 1.0 : 0.0;
      c.sync();
      for (int i = c.tid; i < nv; i += C::nt) a.a_rows[q * nv * nz + i + (long)k * nv] = p.A_row_dot(i, p.dz);
      c.sync();
    }
    for (int k = 0; k < nv; k++) {
      for (int i = c.tid; i < nv; i += C::nt) p.dv[i] = i == k ? 1.0 : 0.0;
      c.sync();
      for (int j = c.tid; j < nz; j += C::nt) a.a_cols[q * nv * nz + k + (long)j * nv] = p.A_col_dot(j, p.dv);
      c.sync();
    }
  }
};

// feasibility(tol) on given directions (behind load_guess: the LDS copy of A)
struct FeasibilityStage {
  struct Args {
    const double *dz, *dl, *dv;
    double tol;
    int* cls;
  };
  template <class P, class C>
  static __device__ __forceinline__ void run(P& p, const C& c, const Args& a, long q) {
    const int nz = p.nz, nl = p.nl, nv = p.nv;
    p.load_guess(c);
    for (int i = c.tid; i < nz; i += C::nt) p.dz[i] = a.dz[q * nz + i];
    for (int i = c.tid; i < nl; i += C::nt) p.dl[i] = a.dl[q * nl + i];
    for (int i = c.tid; i < nv; i += C::nt) p.dv[i] = a.dv[q * nv + i];
    c.sync();
    const int r = p.feasibility(c, a.tol);
    if (c.tid == 0) a.cls[q] = r;
  }
};

// the caller's image into K, wherever K lives, its right-hand side into rhs; ldlt and, on a true verdict,
// ldlt_solve.  (The shape is (n, 0, nv): the problem blocks are not read.)
struct Factor {
  struct Args {
    const double *img, *rhs;  // [count, n * n] by columns, [count, n]
    FactorOut out;
    double* x;  // [count, n]
  };
  template <class P, class C>
  static __device__ __forceinline__ void run(P& p, const C& c, const Args& a, long q) {
    const int n = p.lay.nk;
    for (long e = c.tid; e < (long)n * n; e += C::nt) p.K[e] = a.img[q * n * n + e];
    for (int i = c.tid; i < n; i += C::nt) p.rhs[i] = a.rhs[q * n + i];
    c.sync();
    const bool ok = p.ldlt(c);
    if (c.tid == 0) a.out.verdict[q] = ok ? 1 : 0;
    if (!ok) return;  // (uniform: every thread read the same verdict)
    c.sync();
    write_factors(p, c, a.out, q, P::kRows && p.lay.wave);
    c.sync();
    p.ldlt_solve(c);
    c.sync();
    for (int i = c.tid; i < n; i += C::nt) a.x[q * n + i] = p.rhs[i];
  }
};

// load_guess, residual, the caller's xbar, newton_step<false>; or, ADJ, dense_adjoint with the caller's seeds.
// Two things are the probe's own.  The K region starts filled with kSentinel, so that what the assembly and the
// factorisation leave untouched (ldlt_impl: everything above the diagonal) can be told from what they wrote.  And
// the step itself reads H from `Hstep`, the residual before it from the blocks' H: the caller can hand the step an
// H whose strict upper triangle is NaN (residual and the step's wz = H dz + .. read the full symmetric H by design).
constexpr long long kSentinel = 0x7ff80000dead0000LL;  // a quiet NaN with a payload
template <bool ADJ>
struct Step {
  struct Args {
    const double* Hstep;         // [count, nz * nz]
    const double *zb, *lb, *vb;  // ADJ: the seeds gz, gl, gv
    double sigma, alpha;
    FactorOut out;
    double *y, *rz, *rl, *dz, *dl, *dv, *adz, *wz, *wl, *gam, *rvm, *yb;
  };
  template <class P, class C>
  static __device__ __forceinline__ void run(P& p, const C& c, const Args& a, long q) {
    const int nz = p.nz, nl = p.nl, nv = p.nv;
    const long kk = (long)p.lay.nk * p.lay.nk;
    for (long e = c.tid; e < kk; e += C::nt) p.K[e] = __longlong_as_double(kSentinel);
    c.sync();
    bool ok;
    if constexpr (ADJ) {
      p.D.H = a.Hstep + q * nz * nz;
      ok = dense_adjoint(p, c, a.sigma, a.alpha, a.zb + q * nz, a.lb + q * nl, a.vb + q * nv);
    } else {
      p.load_guess(c);
      p.residual(c);
      for (int i = c.tid; i < nz; i += C::nt) p.zb[i] = a.zb[q * nz + i];
      for (int i = c.tid; i < nl; i += C::nt) p.lb[i] = a.lb[q * nl + i];
      for (int i = c.tid; i < nv; i += C::nt) p.vb[i] = a.vb[q * nv + i];
      p.D.H = a.Hstep + q * nz * nz;
      c.sync();
      ok = p.template newton_step<false>(c, a.sigma, a.alpha);
    }
    c.sync();
    if (c.tid == 0) a.out.verdict[q] = ok ? 1 : 0;
    for (int i = c.tid; i < nv; i += C::nt) {
      a.y[q * nv + i] = p.y[i];
      a.gam[q * nv + i] = p.gam[i];
      a.rvm[q * nv + i] = p.rvm[i];
      if (ADJ) a.yb[q * nv + i] = p.yb[i];
    }
    for (int i = c.tid; i < nz; i += C::nt) a.rz[q * nz + i] = p.rz[i];
    for (int i = c.tid; i < nl; i += C::nt) a.rl[q * nl + i] = p.rl[i];
    if (!ok) return;  // (uniform)
    write_factors(p, c, a.out, q, P::kRows && p.lay.wave);
    for (int i = c.tid; i < nz; i += C::nt) {
      a.dz[q * nz + i] = p.dz[i];
      a.wz[q * nz + i] = p.wz[i];
    }
    for (int i = c.tid; i < nl; i += C::nt) {
      a.dl[q * nl + i] = p.dl[i];
      a.wl[q * nl + i] = p.wl[i];
    }
    for (int i = c.tid; i < nv; i += C::nt) {
      a.dv[q * nv + i] = p.dv[i];
      a.adz[q * nv + i] = p.adz[i];
    }
  }
};

// DenseProblem and whether its ldlt can take ldlt_rows (the condition of `ldlt` itself: K in LDS, a whole wavefront)
template <class C, bool KG, bool VG>
struct Probed : DenseProblem<C, KG, VG> {
  static constexpr bool kRows = !KG && C::nt >= 64;
};

template <int NT, bool KG, bool VG, class Stage>
__global__ __launch_bounds__(NT, (NT > 64 ? 2 : 1)) void k_stage(DenseLayout lay, Blocks B, typename Stage::Args a,
                                                                  double* scratch) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  lds_ptr lds = (lds_ptr)smem;
  typedef Ctx<NT> C;
  C ctx;
  ctx.tid = threadIdx.x;
  ctx.red = lds + lay.o_red;
  Probed<C, KG, VG> p;
  bind_qp(p, lay, B, blockIdx.x, lds, scratch);
  Stage::run(p, ctx, a, blockIdx.x);
}

// the layout and the workgroup width the product would run (nz, nl, nv) at when `want` threads are asked for
inline bool layout_of(int nz, int nl, int nv, int want, int count, DenseLayout& lay, int& nt) {
  if (nz < 1 || nl < 0 || nv < 1 || count < 1 || count > (1 << 16) || (want != 256 && want != 64)) return false;
  if ((long)nz + nl > 4096 || nv > (1 << 20)) return false;
  nt = want;
  lay.init(nz, nl, nv, nt);
  if (nt == 64 && (lay.k_global || !lay.a_lds)) {  // does not fit that way (fbstab_hip_dense_create)
    nt = 256;
    lay.init(nz, nl, nv, nt);
  }
  return (long)lay.lds_doubles * 8 <= kLdsLimit;
}

template <int NT, bool KG, bool VG, class Stage>
int launch(const DenseLayout& lay, int count, const Blocks& B, const typename Stage::Args& a, double* scratch) {
  const size_t lds = (size_t)lay.lds_doubles * sizeof(double);
  auto kern = k_stage<NT, KG, VG, Stage>;
  if (lds > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsLimit);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(kern, dim3(count), dim3(NT), lds, 0, lay, B, a, scratch);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  return (int)hipDeviceSynchronize();
}

template <class Stage>
int run(int nz, int nl, int nv, int want, int count, const Blocks& B, const typename Stage::Args& a,
        double* scratch) {
  DenseLayout lay;
  int nt;
  if (!layout_of(nz, nl, nv, want, count, lay, nt)) return (int)hipErrorInvalidValue;
  if (nt == 64) return launch<64, false, false, Stage>(lay, count, B, a, scratch);
  if (lay.v_global) return launch<256, true, true, Stage>(lay, count, B, a, scratch);
  if (lay.k_global) return launch<256, true, false, Stage>(lay, count, B, a, scratch);
  return launch<256, false, false, Stage>(lay, count, B, a, scratch);
}

}  // namespace

#define DP_BLOCKS const double *H, const double *f, const double *G, const double *h, const double *A, \
                  const double *b, const double *z, const double *l, const double *v
#define DP_BLOCKS_INIT {H, f, G, h, A, b, z, l, v}

// out = {threads, wave, k_global, v_global, a_lds, lds_doubles, nk}; returns the scratch doubles per QP (>= 0),
// -1 for a shape or width the policy does not take
extern "C" long dp_layout(int nz, int nl, int nv, int want, int* out) {
  DenseLayout lay;
  int nt;
  if (!layout_of(nz, nl, nv, want, 1, lay, nt)) return -1;
  out[0] = nt; out[1] = lay.wave; out[2] = lay.k_global; out[3] = lay.v_global; out[4] = lay.a_lds;
  out[5] = lay.lds_doubles; out[6] = lay.nk;
  return lay.k_global ? lay.k_doubles + lay.v_doubles : 0;
}

extern "C" int dp_products(DP_BLOCKS, double* y, double* rz, double* rl, double* nrm, double* a_rows,
                           double* a_cols, double* scratch, int nz, int nl, int nv, int want, int count) {
  const Blocks B = DP_BLOCKS_INIT;
  const Products::Args a = {y, rz, rl, nrm, a_rows, a_cols};
  return run<Products>(nz, nl, nv, want, count, B, a, scratch);
}

extern "C" int dp_feasibility(DP_BLOCKS, const double* dz, const double* dl, const double* dv, double tol, int* cls,
                              double* scratch, int nz, int nl, int nv, int want, int count) {
  const Blocks B = DP_BLOCKS_INIT;
  const FeasibilityStage::Args a = {dz, dl, dv, tol, cls};
  return run<FeasibilityStage>(nz, nl, nv, want, count, B, a, scratch);
}

// (images: the shape is (n, 0, nv) - nv selects the placement; the problem blocks are not read)
extern "C" int dp_factor(DP_BLOCKS, const double* img, const double* rhs, int* verdict, int* perm, double* Kout,
                         double* dpiv, int* ord, double* x, double* scratch, int n, int nv, int want, int count) {
  const Blocks B = DP_BLOCKS_INIT;
  const Factor::Args a = {img, rhs, {verdict, perm, Kout, dpiv, ord}, x};
  return run<Factor>(n, 0, nv, want, count, B, a, scratch);
}

#define DP_STEP_OUT int *verdict, int *perm, double *Kout, double *dpiv, int *ord, double *y, double *rz, \
                    double *rl, double *dz, double *dl, double *dv, double *adz, double *wz, double *wl,  \
                    double *gam, double *rvm, double *yb
#define DP_STEP_ARGS {Hstep, zb, lb, vb, sigma, alpha, {verdict, perm, Kout, dpiv, ord}, y, rz, rl, dz, dl, dv, adz, \
                      wz, wl, gam, rvm, yb}

extern "C" int dp_step(DP_BLOCKS, const double* Hstep, const double* zb, const double* lb, const double* vb, double sigma, double alpha,
                       DP_STEP_OUT, double* scratch, int nz, int nl, int nv, int want, int count) {
  const Blocks B = DP_BLOCKS_INIT;
  const Step<false>::Args a = DP_STEP_ARGS;
  return run<Step<false>>(nz, nl, nv, want, count, B, a, scratch);
}

// (zb, lb, vb: the seeds gz, gl, gv of dense_adjoint)
extern "C" int dp_step_adjoint(DP_BLOCKS, const double* Hstep, const double* zb, const double* lb, const double* vb, double sigma,
                               double alpha, DP_STEP_OUT, double* scratch, int nz, int nl, int nv, int want,
                               int count) {
  const Blocks B = DP_BLOCKS_INIT;
  const Step<true>::Args a = DP_STEP_ARGS;
  return run<Step<true>>(nz, nl, nv, want, count, B, a, scratch);
}
