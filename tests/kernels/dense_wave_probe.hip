// Test-only probe library over fb_dense_wave.h: one small kernel per STAGE of the one-wavefront dense policy, so
// that tests/test_gpu_dense_wave_stages.py can hold each stage to an extended-precision reference and to the
// rounding bounds of tests/dense_wave_rules.py instead of through a whole solve.  Never linked into
// libfbstab_hip.so; built by `make -C fbstab_amd/csrc denseprobe` into tests/_build/libdense_wave_probe.so with
// the product's flags.
//
// Every kernel runs ONE wavefront per QP (workgroup q = QP q, 64 threads): it binds a DenseWave on a
// DenseWaveLayout exactly as fbstab_dense_wave_kernel does, fills the LDS vectors the stage reads from its
// inputs, calls the stage UNCHANGED and writes out what the stage leaves.  No function of fb_dense_wave.h is
// restated here.  Inputs are per-QP blocks (QP q at base + q * length, the lengths those of the shape); all loads
// of the probe itself are in bounds by construction (i < nz / nl / nv, t < 64), every store is to row q < count
// of an output of `count` rows.  The scratch `ws` holds DenseWaveLayout::ws_doubles doubles per QP
// (dwp_ws_doubles) and arrives ZEROED: rows n .. 63 of the multipliers are never written and read as zero, as
// in the product, whose scratch is zero from its allocation on.
//
// Each entry point takes device pointers, the shape and the QP count, launches on the null stream,
// synchronises and returns the hipError_t (hipErrorInvalidValue for a shape the policy does not take).
#include "fb_dense_wave.h"

using namespace fbk;

namespace {

typedef DenseWave::C C;

// One call's problem data and point, QP q at base + q * (length of the shape)
struct Blocks {
  const double *H, *f, *G, *h, *A, *b, *z, *l, *v;
};

__device__ __forceinline__ C make_ctx(lds_ptr lds) {
  C c;
  c.tid = threadIdx.x;
  c.red = lds;  // (unused: one wavefront reduces in registers)
  return c;
}

__device__ __forceinline__ void bind_qp(DenseWave& p, const DenseWaveLayout& lay, const Blocks& B, long q, lds_ptr lds,
                                        double* ws) {
  const long nz = lay.nz, nl = lay.nl, nv = lay.nv;
  DenseData D;
  D.H = B.H + q * nz * nz; D.f = B.f + q * nz;
  D.G = B.G + q * nl * nz; D.h = B.h + q * nl;
  D.A = B.A + q * nv * nz; D.b = B.b + q * nv;
  // (the stages probed here only read the caller's point)
  p.bind(lay, D, const_cast<double*>(B.z + q * nz), const_cast<double*>(B.l + q * nl),
         const_cast<double*>(B.v + q * nv), nullptr, lds, ws + q * lay.ws_doubles, nullptr);
}

// the matrix image of QP q: lane t holds row t, dg its diagonal entry
__device__ __forceinline__ void load_image(const double* img, long q, int t, double (&Kr)[64], double& dg) {
  const double* row = img + (q * 64 + t) * 64;
#pragma unroll
  for (int c = 0; c < 64; c++) Kr[c] = row[c];
  dg = row[t];
}

// assemble(), behind load_guess (Hd, Gt) and the caller's Gamma and rv / mu
__global__ __launch_bounds__(64) void k_assemble(DenseWaveLayout lay, Blocks B, const double* gam, const double* rvm,
                                                 double sigma, double* Kout, double* dg, double* atr, double* ws) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  lds_ptr lds = (lds_ptr)smem;
  const C ctx = make_ctx(lds);
  const long q = blockIdx.x;
  const int t = ctx.tid;
  DenseWave p;
  bind_qp(p, lay, B, q, lds, ws);
  p.load_guess(ctx);
  for (int i = t; i < lay.nv; i += 64) {
    p.gam[i] = gam[q * lay.nv + i];
    p.rvm[i] = rvm[q * lay.nv + i];
  }
  ctx.sync();
  DenseWave::d4 hd[10];
  p.load_hd(t, hd);
  double Kr[64], d, a;
  p.assemble(ctx, hd, sigma, Kr, &d, &a);
  double* row = Kout + (q * 64 + t) * 64;
#pragma unroll
  for (int c = 0; c < 64; c++) row[c] = Kr[c];
  dg[q * 64 + t] = d;
  atr[q * 64 + t] = a;
}

// factor() on an image, then substitute() on its factors; the multipliers stay in ws (o_lg = 0)
__global__ __launch_bounds__(64) void k_factor(DenseWaveLayout lay, Blocks B, const double* img, const double* rhs,
                                               int* verdict, int* ord, double* dpiv, int* permv, double* x,
                                               double* ws) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  lds_ptr lds = (lds_ptr)smem;
  const C ctx = make_ctx(lds);
  const long q = blockIdx.x;
  const int t = ctx.tid;
  DenseWave p;
  bind_qp(p, lay, B, q, lds, ws);
  double Kr[64], d;
  load_image(img, q, t, Kr, d);
  int o = -1, pv = -1;
  double dp = 0.0;
  const bool ok = p.factor(ctx, Kr, d, &o, &dp, &pv);
  if (t == 0) verdict[q] = ok ? 1 : 0;
  if (!ok) return;  // (wavefront-uniform)
  ord[q * 64 + t] = o;
  dpiv[q * 64 + t] = dp;
  permv[q * 64 + t] = pv;
  x[q * 64 + t] = p.substitute(t, rhs[q * 64 + t], o, dp, pv);
}

// factor_solve_static() on an image and a right-hand side (lay.order, lay.spread_bits from the caller)
__global__ __launch_bounds__(64) void k_static(DenseWaveLayout lay, Blocks B, const double* img, const double* rhs,
                                               int* verdict, double* x, double* ws) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  lds_ptr lds = (lds_ptr)smem;
  const C ctx = make_ctx(lds);
  const long q = blockIdx.x;
  const int t = ctx.tid;
  DenseWave p;
  bind_qp(p, lay, B, q, lds, ws);
  double Kr[64], d;
  load_image(img, q, t, Kr, d);
  double xv = rhs[q * 64 + t];
  const bool ok = p.factor_solve_static(ctx, Kr, xv);
  if (t == 0) verdict[q] = ok ? 1 : 0;
  if (ok) x[q * 64 + t] = xv;  // (a false verdict leaves x destroyed)
}

// y = b - A z of load_guess; rz, rl of residual
__global__ __launch_bounds__(64) void k_products(DenseWaveLayout lay, Blocks B, double* y, double* rz, double* rl,
                                                 double* ws) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  lds_ptr lds = (lds_ptr)smem;
  const C ctx = make_ctx(lds);
  const long q = blockIdx.x;
  const int t = ctx.tid;
  DenseWave p;
  bind_qp(p, lay, B, q, lds, ws);
  p.load_guess(ctx);
  p.residual(ctx);
  for (int i = t; i < lay.nv; i += 64) y[q * lay.nv + i] = p.y[i];
  for (int i = t; i < lay.nz; i += 64) rz[q * lay.nz + i] = p.rz[i];
  for (int i = t; i < lay.nl; i += 64) rl[q * lay.nl + i] = p.rl[i];
}

// feasibility(tol) on a given direction
__global__ __launch_bounds__(64) void k_feasibility(DenseWaveLayout lay, Blocks B, const double* dz, const double* dl,
                                                    const double* dv, double tol, int* cls, double* ws) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  lds_ptr lds = (lds_ptr)smem;
  const C ctx = make_ctx(lds);
  const long q = blockIdx.x;
  const int t = ctx.tid;
  DenseWave p;
  bind_qp(p, lay, B, q, lds, ws);
  for (int i = t; i < lay.nz; i += 64) p.dz[i] = dz[q * lay.nz + i];
  for (int i = t; i < lay.nl; i += 64) p.dl[i] = dl[q * lay.nl + i];
  for (int i = t; i < lay.nv; i += 64) p.dv[i] = dv[q * lay.nv + i];
  ctx.sync();
  const int r = p.feasibility(ctx, tol);
  if (t == 0) cls[q] = r;
}

inline bool layout_of(int nz, int nl, int nv, int count, DenseWaveLayout& lay) {
  if (nz < 1 || nl < 0 || nv < 1 || count < 1 || count > (1 << 20)) return false;
  lay.init(nz, nl, nv);
  return lay.fits();
}

template <class K, class... Args>
int launch(K kern, const DenseWaveLayout& lay, int count, Args... args) {
  hipLaunchKernelGGL(kern, dim3(count), dim3(64), (size_t)lay.lds_doubles * sizeof(double), 0, lay, args...);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  return (int)hipDeviceSynchronize();
}

}  // namespace

#define DWP_BLOCKS const double *H, const double *f, const double *G, const double *h, const double *A, \
                   const double *b, const double *z, const double *l, const double *v
#define DWP_BLOCKS_INIT {H, f, G, h, A, b, z, l, v}

extern "C" long dwp_ws_doubles(int nz, int nl, int nv) {
  DenseWaveLayout lay;
  return layout_of(nz, nl, nv, 1, lay) ? lay.ws_doubles : -1;
}

extern "C" int dwp_assemble(DWP_BLOCKS, const double* gam, const double* rvm, double sigma, double* Kout,
                            double* dg, double* atr, double* ws, int nz, int nl, int nv, int count) {
  DenseWaveLayout lay;
  if (!layout_of(nz, nl, nv, count, lay)) return (int)hipErrorInvalidValue;
  const Blocks B = DWP_BLOCKS_INIT;
  return launch(k_assemble, lay, count, B, gam, rvm, sigma, Kout, dg, atr, ws);
}

// (images: the shape is (n, 0, 1); the problem blocks are not read by these stages)
extern "C" int dwp_factor(DWP_BLOCKS, const double* img, const double* rhs, int* verdict, int* ord, double* dpiv,
                          int* permv, double* x, double* ws, int n, int count) {
  DenseWaveLayout lay;
  if (!layout_of(n, 0, 1, count, lay)) return (int)hipErrorInvalidValue;
  const Blocks B = DWP_BLOCKS_INIT;
  return launch(k_factor, lay, count, B, img, rhs, verdict, ord, dpiv, permv, x, ws);
}

extern "C" int dwp_static(DWP_BLOCKS, const double* img, const double* rhs, int* verdict, double* x, double* ws,
                          int n, int order, int spread_bits, int count) {
  DenseWaveLayout lay;
  if (!layout_of(n, 0, 1, count, lay) || order < 0 || order > 2) return (int)hipErrorInvalidValue;
  lay.order = order;
  lay.spread_bits = spread_bits;
  const Blocks B = DWP_BLOCKS_INIT;
  return launch(k_static, lay, count, B, img, rhs, verdict, x, ws);
}

extern "C" int dwp_products(DWP_BLOCKS, double* y, double* rz, double* rl, double* ws, int nz, int nl, int nv,
                            int count) {
  DenseWaveLayout lay;
  if (!layout_of(nz, nl, nv, count, lay)) return (int)hipErrorInvalidValue;
  const Blocks B = DWP_BLOCKS_INIT;
  return launch(k_products, lay, count, B, y, rz, rl, ws);
}

extern "C" int dwp_feasibility(DWP_BLOCKS, const double* dz, const double* dl, const double* dv, double tol,
                               int* cls, double* ws, int nz, int nl, int nv, int count) {
  DenseWaveLayout lay;
  if (!layout_of(nz, nl, nv, count, lay)) return (int)hipErrorInvalidValue;
  const Blocks B = DWP_BLOCKS_INIT;
  return launch(k_feasibility, lay, count, B, dz, dl, dv, tol, cls, ws);
}
