// Test-only probe library over fb_row16.h (and the scalar chains of fb_common.h): one small kernel per
// primitive, so that tests/test_gpu_row_primitives.py can compare each of them with an extended-precision
// reference instead of through a whole solve.  Never linked into libfbstab_hip.so; built by
// `make -C fbstab_amd/csrc rowprobe` into tests/_build/ in three variants (default, FB_FMAC_GUARD_NOP=1,
// FB_FMAC_DPP=0 - the last without the fused forms, which do not compile there).
//
// Lane discipline.  A QP occupies LPQ = 16 R lanes, a wavefront holds 4 / R QPs, thread t of the grid is
// lane t % LPQ of QP t / LPQ.  EVERY lane of every launched wavefront executes every DPP instruction: no
// kernel returns early or predicates a primitive.  Inputs are "lane images": [alloc][LPQ][K] doubles, lane
// r of QP q reads row (q, r) - rows r < N are the matrix, rows r >= N whatever the test put there - and a
// QP index beyond the allocation is clamped to the last allocated one, so every load is in bounds whatever
// the grid.  Only stores are predicated (qp < count, and r < N where the output is N rows per QP); every
// output index is bounded by count.
//
// Each entry point takes device pointers, the QP count, the allocated QP count of the inputs and the
// workgroup size (64 or 256), launches on the null stream, synchronises and returns the hipError_t.
#include "fb_common.h"
#include "fb_row16.h"

using namespace fbk;

namespace {

template <int R>
struct Lane {
  int qp, r, ld;  // QP, lane within it, QP index clamped for loads
  __device__ __forceinline__ explicit Lane(int alloc) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    qp = t / (16 * R);
    r = t % (16 * R);
    ld = qp < alloc ? qp : alloc - 1;
  }
  __device__ __forceinline__ long row() const { return (long)ld * (16 * R) + r; }
};

template <int K>
__device__ __forceinline__ void load_row(const double* src, long row, double (&a)[K]) {
#pragma unroll
  for (int c = 0; c < K; c++) a[c] = src[row * K + c];
}
// rows r < NR of QP qp < count: out[count][NR][K]
template <int NR, int K>
__device__ __forceinline__ void store_row(double* out, int qp, int r, int count, const double (&a)[K]) {
  if (qp < count && r < NR) {
#pragma unroll
    for (int c = 0; c < K; c++) out[((long)qp * NR + r) * K + c] = a[c];
  }
}

// ---- factorisation and triangular work ------------------------------------------------------------
template <int N, int R>
__global__ void k_chol(const double* A, const double* dadd, double* L, int* flag, int count, int alloc) {
  const Lane<R> ln(alloc);
  double a[N];
  load_row<N>(A, ln.row(), a);
  const bool ok = chol_rows<N, R>(a, ln.r, dadd[ln.ld]);
  store_row<N, N>(L, ln.qp, ln.r, count, a);
  if (ln.qp < count) flag[(long)ln.qp * (16 * R) + ln.r] = ok ? 1 : 0;
}
template <int N, int R>
__global__ void k_triinv(const double* L, double* X, int count, int alloc) {
  const Lane<R> ln(alloc);
  double a[N], x[N];
  load_row<N>(L, ln.row(), a);
  tri_inv_cols<N, R>(a, x, ln.r);
  store_row<N, N>(X, ln.qp, ln.r, count, x);
}
template <int N, int R>
__global__ void k_triinvsolve(const double* L, const double* B, double* X, double* W, int count, int alloc) {
  const Lane<R> ln(alloc);
  double a[N], x[N], w[N];
  load_row<N>(L, ln.row(), a);
  load_row<N>(B, ln.row(), w);
  tri_inv_cols_solve<N, R>(a, x, w, ln.r);
  store_row<N, N>(X, ln.qp, ln.r, count, x);
  store_row<N, N>(W, ln.qp, ln.r, count, w);
}
template <int N, int R>
__global__ void k_trisolve(const double* L, const double* B, double* W, int count, int alloc) {
  const Lane<R> ln(alloc);
  double a[N], w[N];
  load_row<N>(L, ln.row(), a);
  load_row<N>(B, ln.row(), w);
  tri_solve_right<N, R>(a, w, ln.r);
  store_row<N, N>(W, ln.qp, ln.r, count, w);
}
// COLS: the factor image holds columns (lane r: a[j] = L[j][r]) and the chain is subst_cols_t
template <int N, int R, bool COLS>
__global__ void k_subst(const double* L, const double* b, double* x, int count, int alloc) {
  const Lane<R> ln(alloc);
  double a[N];
  load_row<N>(L, ln.row(), a);
  const double bv = b[ln.row()];
  double xv[1];
  if constexpr (COLS) xv[0] = subst_cols_t<N, R>(a, bv, ln.r);
  else xv[0] = subst_rows<N, R>(a, bv, ln.r);
  store_row<N, 1>(x, ln.qp, ln.r, count, xv);
}
#if FB_FMAC_DPP
// MODE 0: chol_inv_cols_solve, 1: chol_inv_cols, 2: chol_solve_right (the PARK form)
template <int N, int R, int MODE>
__global__ void k_fused(const double* A, const double* dadd, const double* B, double* L, double* X, double* W,
                        int* flag, int count, int alloc) {
  const Lane<R> ln(alloc);
  double a[N], x[N], w[N];
  load_row<N>(A, ln.row(), a);
  load_row<N>(B, ln.row(), w);
#pragma unroll
  for (int c = 0; c < N; c++) x[c] = 0.0;
  bool ok;
  if constexpr (MODE == 0) ok = chol_inv_cols_solve<N, R>(a, x, w, ln.r, dadd[ln.ld]);
  else if constexpr (MODE == 1) ok = chol_inv_cols<N, R>(a, x, ln.r, dadd[ln.ld]);
  else ok = chol_solve_right<N, R>(a, w, ln.r, dadd[ln.ld]);
  store_row<N, N>(L, ln.qp, ln.r, count, a);
  store_row<N, N>(X, ln.qp, ln.r, count, x);
  store_row<N, N>(W, ln.qp, ln.r, count, w);
  if (ln.qp < count) flag[(long)ln.qp * (16 * R) + ln.r] = ok ? 1 : 0;
}
#endif

// ---- dot products: one result per LANE (all 16 R of a QP), out[count][LPQ][..] ------------------------
template <int B, int E, int R>
__global__ void k_bcdot(const double* M, const double* v, const double* init, double* out, int count, int alloc) {
  const Lane<R> ln(alloc);
  double m[E];
  load_row<E>(M, ln.row(), m);
  double o[1] = {bc_dot<B, E, R>(m, v[ln.row()], init[ln.row()])};
  store_row<16 * R, 1>(out, ln.qp, ln.r, count, o);
}
template <int NC, int R, bool NEG>
__global__ void k_bccols(const double* C, const double* src, const double* p0, double* out, int count, int alloc) {
  const Lane<R> ln(alloc);
  constexpr int NSRC = (NC + 16 * R - 1) / (16 * R);
  double c[NC], s[NSRC], p[4];
  load_row<NC>(C, ln.row(), c);
  load_row<NSRC>(src, ln.row(), s);
  load_row<4>(p0, ln.row(), p);
  bc_cols_dot<NC, R, NEG>(c, s, p);
  store_row<16 * R, 4>(out, ln.qp, ln.r, count, p);
}
template <int N>
__global__ void k_dot4(const double* M, const double* Bv, const double* init, double* out, int count, int alloc) {
  const Lane<1> ln(alloc);
  double m[N], b[N];
  load_row<N>(M, ln.row(), m);
  load_row<N>(Bv, ln.row(), b);
  double o[1] = {dot4<N>(m, b, init[ln.row()])};
  store_row<16, 1>(out, ln.qp, ln.r, count, o);
}

// ---- lane maps and reductions ---------------------------------------------------------------------------
template <int N, int R>
__global__ void k_bcall(const double* v, double* out, int count, int alloc) {
  const Lane<R> ln(alloc);
  double o[N];
  bc_all<N, R>(v[ln.row()], o);
  store_row<16 * R, N>(out, ln.qp, ln.r, count, o);
}
// out_d[count][LPQ][3][LPQ]: bc<J & 15>, bcs<R, J>, bcr<R, J>; out_i[count][LPQ][2][LPQ]: bci<J & 15>, bcri<R, J>
template <int R>
__global__ void k_lanemap(const double* v, const int* vi, double* out_d, int* out_i, int count, int alloc) {
  const Lane<R> ln(alloc);
  constexpr int LPQ = 16 * R;
  const double x = v[ln.row()];
  const int xi = vi[ln.row()];
  double d0[LPQ], d1[LPQ], d2[LPQ];
  int i0[LPQ], i1[LPQ];
  const Spread<R> s = spread<R>(x);
  sfor<0, LPQ>([&](auto J) {
    constexpr int j = decltype(J)::value;
    d0[j] = bc<(j & 15)>(x);
    d1[j] = bcs<R, j>(s);
    d2[j] = bcr<R, j>(x);
    i0[j] = bci<(j & 15)>(xi);
    i1[j] = bcri<R, j>(xi);
  });
  if (ln.qp < count) {
    const long o = ((long)ln.qp * LPQ + ln.r);
#pragma unroll
    for (int j = 0; j < LPQ; j++) {
      out_d[(o * 3 + 0) * LPQ + j] = d0[j];
      out_d[(o * 3 + 1) * LPQ + j] = d1[j];
      out_d[(o * 3 + 2) * LPQ + j] = d2[j];
      out_i[(o * 2 + 0) * LPQ + j] = i0[j];
      out_i[(o * 2 + 1) * LPQ + j] = i1[j];
    }
  }
}
// out[count][LPQ][4]: row_reduce sum, row_reduce max, qp_reduce sum, qp_reduce max
template <int R>
__global__ void k_reduce(const double* v, double* out, int count, int alloc) {
  const Lane<R> ln(alloc);
  const double x = v[ln.row()];
  double o[4];
  o[0] = row_reduce<OpSum16>(x);
  o[1] = row_reduce<OpMax16>(x);
  o[2] = qp_reduce<R, OpSum16>(x);
  o[3] = qp_reduce<R, OpMax16>(x);
  store_row<16 * R, 4>(out, ln.qp, ln.r, count, o);
}

// ---- scalar chains on the chip's seeds (one value per thread) ----------------------------------------
// out[n][3]: rsqrt_full, fsqrt, rcp_fast of x[i]
__global__ void k_scalar(const double* x, double* out, int n) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const double v = x[t < n ? t : n - 1];
  const double a = rsqrt_full(v), b = fsqrt(v), c = rcp_fast(v);
  if (t < n) {
    out[3L * t + 0] = a;
    out[3L * t + 1] = b;
    out[3L * t + 2] = c;
  }
}
// out[n][6]: pfb_all's phi, g0, g1, then pfb's phi and pfb_gradient's g0, g1
__global__ void k_pfb(const double* a, const double* b, const double* alpha, double* out, int n) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int i = t < n ? t : n - 1;
  double o[6];
  pfb_all(a[i], b[i], alpha[i], &o[0], &o[1], &o[2]);
  o[3] = pfb(a[i], b[i], alpha[i]);
  pfb_gradient(a[i], b[i], alpha[i], &o[4], &o[5]);
  if (t < n) {
#pragma unroll
    for (int k = 0; k < 6; k++) out[6L * t + k] = o[k];
  }
}

template <class K, class... A>
int launch(K kern, long threads, int wg, A... args) {
  if ((wg != 64 && wg != 256) || threads <= 0 || threads > (1L << 24)) return (int)hipErrorInvalidValue;
  const int grid = (int)((threads + wg - 1) / wg);
  hipLaunchKernelGGL(kern, dim3(grid), dim3(wg), 0, 0, args...);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  return (int)hipDeviceSynchronize();
}
// (count QPs of lpq lanes each; the inputs hold alloc >= 1 QPs)
inline bool bad(int count, int alloc) { return count <= 0 || alloc <= 0; }

}  // namespace

#define RP_CHECK if (bad(count, alloc)) return (int)hipErrorInvalidValue

#define RP_PAIR(N, R)                                                                                              \
  extern "C" int rp_chol_##N##_##R(const double* A, const double* dadd, double* L, int* flag, int count, int alloc, \
                                   int wg) {                                                                       \
    RP_CHECK;                                                                                                      \
    return launch(k_chol<N, R>, 16L * R * count, wg, A, dadd, L, flag, count, alloc);                              \
  }                                                                                                                \
  extern "C" int rp_triinv_##N##_##R(const double* L, double* X, int count, int alloc, int wg) {                   \
    RP_CHECK;                                                                                                      \
    return launch(k_triinv<N, R>, 16L * R * count, wg, L, X, count, alloc);                                        \
  }                                                                                                                \
  extern "C" int rp_triinvsolve_##N##_##R(const double* L, const double* B, double* X, double* W, int count,       \
                                          int alloc, int wg) {                                                     \
    RP_CHECK;                                                                                                      \
    return launch(k_triinvsolve<N, R>, 16L * R * count, wg, L, B, X, W, count, alloc);                             \
  }                                                                                                                \
  extern "C" int rp_trisolve_##N##_##R(const double* L, const double* B, double* W, int count, int alloc, int wg) { \
    RP_CHECK;                                                                                                      \
    return launch(k_trisolve<N, R>, 16L * R * count, wg, L, B, W, count, alloc);                                   \
  }                                                                                                                \
  extern "C" int rp_substrows_##N##_##R(const double* L, const double* b, double* x, int count, int alloc,         \
                                        int wg) {                                                                  \
    RP_CHECK;                                                                                                      \
    return launch(k_subst<N, R, false>, 16L * R * count, wg, L, b, x, count, alloc);                               \
  }                                                                                                                \
  extern "C" int rp_substcolst_##N##_##R(const double* L, const double* b, double* x, int count, int alloc,        \
                                         int wg) {                                                                 \
    RP_CHECK;                                                                                                      \
    return launch(k_subst<N, R, true>, 16L * R * count, wg, L, b, x, count, alloc);                                \
  }
RP_PAIR(16, 1)
RP_PAIR(12, 1)
RP_PAIR(23, 2)
RP_PAIR(32, 2)
RP_PAIR(18, 2)
RP_PAIR(24, 2)
RP_PAIR(1, 1)
RP_PAIR(2, 1)
RP_PAIR(17, 2)

#if FB_FMAC_DPP
#define RP_FUSED(NAME, N, R, MODE)                                                                            \
  extern "C" int rp_##NAME##_##N##_##R(const double* A, const double* dadd, const double* B, double* L,       \
                                       double* X, double* W, int* flag, int count, int alloc, int wg) {       \
    RP_CHECK;                                                                                                 \
    return launch(k_fused<N, R, MODE>, 16L * R * count, wg, A, dadd, B, L, X, W, flag, count, alloc);         \
  }
RP_FUSED(cholinvsolve, 16, 1, 0)
RP_FUSED(cholinv, 12, 1, 1)
RP_FUSED(cholinv, 18, 2, 1)
RP_FUSED(cholinv, 24, 2, 1)
RP_FUSED(cholsolveright, 23, 2, 2)
RP_FUSED(cholsolveright, 32, 2, 2)
#endif

#define RP_BCDOT(B, E, R)                                                                                    \
  extern "C" int rp_bcdot_##B##_##E##_##R(const double* M, const double* v, const double* init, double* out, \
                                          int count, int alloc, int wg) {                                    \
    RP_CHECK;                                                                                                \
    return launch(k_bcdot<B, E, R>, 16L * R * count, wg, M, v, init, out, count, alloc);                     \
  }
RP_BCDOT(0, 16, 1)
RP_BCDOT(0, 12, 1)
RP_BCDOT(0, 23, 2)
RP_BCDOT(0, 32, 2)
RP_BCDOT(0, 18, 2)
RP_BCDOT(0, 24, 2)
RP_BCDOT(3, 11, 1)
RP_BCDOT(14, 19, 2)

#define RP_BCCOLS(NC, R)                                                                                        \
  extern "C" int rp_bccols_##NC##_##R##_0(const double* C, const double* src, const double* p0, double* out,    \
                                          int count, int alloc, int wg) {                                       \
    RP_CHECK;                                                                                                   \
    return launch(k_bccols<NC, R, false>, 16L * R * count, wg, C, src, p0, out, count, alloc);                  \
  }                                                                                                             \
  extern "C" int rp_bccols_##NC##_##R##_1(const double* C, const double* src, const double* p0, double* out,    \
                                          int count, int alloc, int wg) {                                       \
    RP_CHECK;                                                                                                   \
    return launch(k_bccols<NC, R, true>, 16L * R * count, wg, C, src, p0, out, count, alloc);                   \
  }
RP_BCCOLS(20, 1)
RP_BCCOLS(32, 1)
RP_BCCOLS(10, 2)
RP_BCCOLS(16, 2)
RP_BCCOLS(32, 2)

#define RP_DOT4(N)                                                                                              \
  extern "C" int rp_dot4_##N(const double* M, const double* Bv, const double* init, double* out, int count,     \
                             int alloc, int wg) {                                                               \
    RP_CHECK;                                                                                                   \
    return launch(k_dot4<N>, 16L * count, wg, M, Bv, init, out, count, alloc);                                  \
  }
RP_DOT4(16)
RP_DOT4(12)
RP_DOT4(23)
RP_DOT4(32)
RP_DOT4(18)
RP_DOT4(24)

#define RP_LANES(R)                                                                                             \
  extern "C" int rp_bcall_##R(const double* v, double* out, int count, int alloc, int wg) {                     \
    RP_CHECK;                                                                                                   \
    return launch(k_bcall<16 * R, R>, 16L * R * count, wg, v, out, count, alloc);                               \
  }                                                                                                             \
  extern "C" int rp_lanemap_##R(const double* v, const int* vi, double* out_d, int* out_i, int count, int alloc, \
                                int wg) {                                                                       \
    RP_CHECK;                                                                                                   \
    return launch(k_lanemap<R>, 16L * R * count, wg, v, vi, out_d, out_i, count, alloc);                        \
  }                                                                                                             \
  extern "C" int rp_reduce_##R(const double* v, double* out, int count, int alloc, int wg) {                    \
    RP_CHECK;                                                                                                   \
    return launch(k_reduce<R>, 16L * R * count, wg, v, out, count, alloc);                                      \
  }
RP_LANES(1)
RP_LANES(2)

extern "C" int rp_scalar(const double* x, double* out, int n, int wg) {
  if (n <= 0) return (int)hipErrorInvalidValue;
  return launch(k_scalar, n, wg, x, out, n);
}
extern "C" int rp_pfb(const double* a, const double* b, const double* alpha, double* out, int n, int wg) {
  if (n <= 0) return (int)hipErrorInvalidValue;
  return launch(k_pfb, n, wg, a, b, alpha, out, n);
}
// which build this is: bit 0 FB_FMAC_DPP, bit 1 FB_FMAC_GUARD_NOP
extern "C" int rp_variant() { return (FB_FMAC_DPP ? 1 : 0) | (FB_FMAC_GUARD_NOP ? 2 : 0); }
