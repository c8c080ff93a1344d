// libfbstab_hip.so: gfx950 kernels and the C-ABI of include/fbstab_hip.h.
//
// Execution model: a persistent grid of workgroups, one QP per workgroup at a
// time.  Workgroups pull QP indices from a device-side counter (iteration
// counts differ per QP by 5-10x, so a static assignment would leave CUs idle at
// the tail).  The whole FBstab solve of a QP (proximal loop, Newton loop,
// factorisation, line search) runs inside the kernel; the host only launches.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdio>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "../../include/fbstab_hip.h"
#include "fb_algorithm.h"
#include "fb_dense.h"
#include "fb_dense_kkt_multi.h"  // (kDenseKktSeeded; its kernels are fb_dense_kkt_multi.hip's)
#include "fb_condense_plan.h"  // (the condensed route: its kernels are fb_condense*.hip's, its host side fb_condense_stage.h)
#include "fb_dense_wave.h"
#include "fb_final_norms.h"
#include "fb_grad_reduce.h"
#include "fb_in_flight.h"
#include "fb_launch_plan.h"
#include "fb_mpc.h"
#include "fb_mpc_r16.h"
#include "fb_record_kernel.h"
#include "fb_tangent.h"
#include "fb_queue_order.h"

#if defined(FB_ANY_STAMP)
namespace fbk { __device__ unsigned long long g_stamps[32]; }
#endif

namespace {

using namespace fbk;

constexpr int kMpcThreads = 64;     // one wavefront per MPC QP
constexpr int kDenseThreads = 256;  // four wavefronts per dense QP

// Next QP index for this workgroup (workgroup-uniform).
template <int NT>
__device__ __forceinline__ int next_qp(int* counter, lds_ptr slot) {
  if (NT <= 64) {
    int q = 0;
    if (threadIdx.x == 0) q = atomicAdd(counter, 1);
    return __shfl(q, 0, 64);
  } else {
    __syncthreads();
    if (threadIdx.x == 0) *((FB_LDS int*)slot) = atomicAdd(counter, 1);
    __syncthreads();
    return *((FB_LDS int*)slot);
  }
}

constexpr int kMpcMinWaves = 1;  // wavefronts per SIMD the flat-vector MPC kernels are compiled for
// DBG: the Newton-step probe; TRACE: `dbg` is the trace buffer of
// fbstab_hip_mpc_solve_traced (see Solver in fb_algorithm.h); WG: the stage tile and the
// work matrices in global scratch (MpcLayout::wglobal: shapes beyond the LDS).
template <int NT, bool DBG, bool TRACE = false, bool WG = false>
__global__ __launch_bounds__(NT, kMpcMinWaves) void fbstab_mpc_kernel(MpcLayout lay, fbstab_mpc_batch_t data,
                                                        fbstab_var_batch_t x,
                                                        fbstab_solver_out_t* out,
                                                        fbstab_options_t opts, double* scratch,
                                                        int* counter, int batch, double* dbg) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  lds_ptr lds = (lds_ptr)smem;
  typedef Ctx<NT> C;
  C ctx;
  ctx.tid = threadIdx.x;
  ctx.red = WG ? lds : lds + lay.w_red;
  double* ws = scratch + (long)blockIdx.x * lay.ws_doubles;
  for (;;) {
    const int q = next_qp<NT>(counter, WG ? lds + kMaxReduce * ((NT + 63) / 64) : lds + lay.w_out);
    if (q >= batch) break;
    MpcProblem<C, WG> p;
    typename MpcProblem<C, WG>::mptr mb;
    if constexpr (WG) mb = ws + lay.v_carve;
    else mb = lds;
    p.bind(lay, mpc_data_at(data, q), var_at(x, 0, q), var_at(x, 1, q), var_at(x, 2, q), var_at(x, 3, q), mb, ws);
    if constexpr (DBG) {
      newton_probe(p, ctx, opts, dbg);
    } else {
      Solver<MpcProblem<C, WG>, C, TRACE> solver(p, ctx, opts, dbg);
      solver.solve(out + q);
      if (solver.refined_ > 0 && ctx.tid == 0) atomicAdd(counter + 1, solver.refined_);  // fbstab_hip_mpc_refined_steps
    }
    ctx.sync();
  }
}


// The adjoint of fbstab_hip_mpc_adjoint_batch on the flat-vector policy (fb_mpc.h: mpc_adjoint,
// mpc_adjoint_gradients), one QP per workgroup pulled from the queue like the solve: the shapes of the flat-vector
// kernel, and the record handles that FBSTAB_HIP_FLAT_ADJOINT or the row-pair instances' default keeps on it (they
// give it a scratch of its own; the others run fbstab_mpc_r16_adjoint_kernel, fb_record_kernel.h).  `x`: the point
// (z, l, v); `seed`: (gz, gl, gv), null l / v slots meaning zero; `adj`: null slots, or (dz, dl, dv).
template <int NT, bool WG>
__global__ __launch_bounds__(NT, kMpcMinWaves) void fbstab_mpc_adjoint_kernel(
    MpcLayout lay, fbstab_mpc_batch_t data, fbstab_var_batch_t x, fbstab_var_batch_t seed, fbstab_mpc_grad_batch_t grad, fbstab_var_batch_t adj,
    int* status, double sigma, double alpha, double* scratch, int* counter, int batch) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  lds_ptr lds = (lds_ptr)smem;
  typedef Ctx<NT> C;
  C ctx;
  ctx.tid = threadIdx.x;
  ctx.red = WG ? lds : lds + lay.w_red;
  double* ws = scratch + (long)blockIdx.x * lay.ws_doubles;
  for (;;) {
    const int q = next_qp<NT>(counter, WG ? lds + kMaxReduce * ((NT + 63) / 64) : lds + lay.w_out);
    if (q >= batch) break;
    MpcProblem<C, WG> p;
    typename MpcProblem<C, WG>::mptr mb;
    if constexpr (WG) mb = ws + lay.v_carve;
    else mb = lds;
    p.bind(lay, mpc_data_at(data, q), var_at(x, 0, q), var_at(x, 1, q), var_at(x, 2, q), nullptr, mb, ws);
    // (the seed and adjoint slots one by one, the gradients named before the call: var_at / var_or_null on these
    // two blocks, or the gradients formed among the call's arguments, re-schedule this kernel - LABNOTES)
    const bool ok = mpc_adjoint(p, ctx, sigma, alpha, slot_at(seed.base[0], seed.stride[0], q),
                                slot_or_null(seed.base[1], seed.stride[1], q), slot_or_null(seed.base[2], seed.stride[2], q));
    const MpcGrad G = mpc_grad_or_null(grad, q);
    mpc_adjoint_gradients(p, ctx, G, ok, slot_or_null(adj.base[0], adj.stride[0], q),
                          slot_or_null(adj.base[1], adj.stride[1], q), slot_or_null(adj.base[2], adj.stride[2], q));
    if (ctx.tid == 0) status[q] = ok ? 0 : 1;
    ctx.sync();
  }
}

// Closed-loop step of the receding-horizon sweep (fbstab_hip_mpc_receding_sweep):
// one thread per trajectory.  u0 = first input of the solution just computed,
// x0 <- A x0 + B u0 (the SimulationInputs of the reference's generator,
// fbstab/test/ocp_generator.h:31-38); (z, l, v) stay where they are and are the
// next step's initial guess, unshifted (the reference has no shift logic;
// fbstab_algorithm-impl.h:140 starts from whatever the caller's Variable holds) unless
// fbstab_hip_mpc_receding_sweep_scenario asks for the shift (shift_stages below).
// With `retire`, a trajectory whose solve did not end in SUCCESS is parked at the
// origin for the rest of the sweep (x0 = 0, guess 0), as a controller's fallback
// would: its QP is then solved by the zero vector in one proximal iteration.
// stats[step] = {sum of Newton iterations, solves that ended in SUCCESS,
// trajectories retired so far, largest Newton count}.
// lg: this step's share of the sweep log (fbstab_hip_mpc_receding_sweep_logged; null slots are not logged).
// w: null, or this step's disturbances [batch][nx], added behind the fma chain (fbstab_hip_mpc_receding_sweep_scenario;
// a parked trajectory stays at the origin).  shift_stages: 0, or N: (z, l, v) are then moved one stage towards the
// present, block i <- block i + 1 for i < N in ascending order, stage N keeping its values (receding_plant_step).
struct SweepLogStep {
  double *z, *l, *v, *x0;
  int* eflag;
};
__global__ void fbstab_receding_plant_kernel(int batch, int nx, int nu, int nz, int nl, int nv, const double* A,
                                             long long sA, const double* B, long long sB, double* x0, long long sx0,
                                             fbstab_var_batch_t x, const fbstab_solver_out_t* out, int* retired,
                                             int retire, double* u_log, unsigned long long* stats, double* xtmp,
                                             SweepLogStep lg, const double* w, int shift_stages, int nc) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = q < batch;
  fbstab_solver_out_t o;
  o.eflag = FBSTAB_SUCCESS;
  o.newton_iters = 0;
  if (live) o = out[q];
  double* z = var_at(x, 0, live ? q : 0);
  double* xs = x0 + (live ? q : 0) * sx0;
  bool gone = live && retired[q] != 0;
  if (live && retire && !gone && o.eflag != FBSTAB_SUCCESS) {
    gone = true;
    retired[q] = 1;
    for (int i = 0; i < nz; i++) z[i] = 0.0;
    double* l = var_at(x, 1, q);
    double* v = var_at(x, 2, q);
    for (int i = 0; i < nl; i++) l[i] = 0.0;
    for (int i = 0; i < nv; i++) v[i] = 0.0;
  }
  {
    // statistics: one set of atomics per wavefront (thousands of same-address atomics
    // a step would cost more than the solve)
    int ns = live ? o.newton_iters : 0, ok = (live && o.eflag == FBSTAB_SUCCESS) ? 1 : 0, gn = gone ? 1 : 0, mx = ns;
    for (int m = 32; m >= 1; m >>= 1) {
      ns += __shfl_xor(ns, m, 64);
      ok += __shfl_xor(ok, m, 64);
      gn += __shfl_xor(gn, m, 64);
      const int om = __shfl_xor(mx, m, 64);
      mx = om > mx ? om : mx;
    }
    if ((threadIdx.x & 63) == 0) {
      atomicAdd(&stats[0], (unsigned long long)ns);
      atomicAdd(&stats[1], (unsigned long long)ok);
      atomicAdd(&stats[2], (unsigned long long)gn);
      atomicMax(&stats[3], (unsigned long long)mx);
    }
  }
  if (!live) return;
  // (u0 = z[nx .. nx + nu) is read where it is used; the new state is collected in
  // registers up to 64 states, in the caller's per-trajectory buffer beyond)
  if (u_log)
    for (int j = 0; j < nu; j++) u_log[(long long)q * nu + j] = gone ? 0.0 : z[nx + j];
  // the log of the backward pass: the point this step returned (zeros once retired), the state it was solved
  // for and its eflag (what receding_plant_step logs in the one-launch sweep)
  if (lg.z)
    for (int i = 0; i < nz; i++) lg.z[(long long)q * nz + i] = gone ? 0.0 : z[i];
  if (lg.l) {
    const double* l = var_at(x, 1, q);
    for (int i = 0; i < nl; i++) lg.l[(long long)q * nl + i] = gone ? 0.0 : l[i];
  }
  if (lg.v) {
    const double* v = var_at(x, 2, q);
    for (int i = 0; i < nv; i++) lg.v[(long long)q * nv + i] = gone ? 0.0 : v[i];
  }
  if (lg.x0)
    for (int r = 0; r < nx; r++) lg.x0[(long long)q * nx + r] = xs[r];
  if (lg.eflag) lg.eflag[q] = gone ? -1 : o.eflag;
  const double* Aq = A + q * sA;
  const double* Bq = B + q * sB;
  double xloc[64];
  double* xn = nx <= 64 ? xloc : xtmp + (long long)q * nx;
  for (int r = 0; r < nx; r++) {
    double acc = 0.0;
    for (int c = 0; c < nx; c++) acc = fma(Aq[r + c * nx], xs[c], acc);
    for (int j = 0; j < nu; j++) acc = fma(Bq[r + j * nx], gone ? 0.0 : z[nx + j], acc);
    if (w) acc = acc + w[(long long)q * nx + r];
    xn[r] = gone ? 0.0 : acc;
  }
  for (int r = 0; r < nx; r++) xs[r] = xn[r];
  if (shift_stages > 0) {
    double* l = var_at(x, 1, q);
    double* v = var_at(x, 2, q);
    const int bz = nx + nu;
    for (int i = 0; i < shift_stages * bz; i++) z[i] = z[i + bz];
    for (int i = 0; i < shift_stages * nx; i++) l[i] = l[i + nx];
    for (int i = 0; i < shift_stages * nc; i++) v[i] = v[i + nc];
  }
}

// The per-step form of fbstab_hip_mpc_receding_sweep_adjoint (include/fbstab_hip.h has the recursion): between
// the adjoint launches of the steps, one workgroup per trajectory.
//   phase 0: zeros in the caller's gradient slots, lambda = 0, status = 0, a zero seed vector;
//   phase 1 (before step k's adjoint launch): mu = gx[k] + lambda (kept where lambda was, and in mu_log), A'mu,
//            and the seed gu[k] + B'mu on the u0 entries;
//   phase 2 (after it): the step's gradients, which the launch left in the handle's per-QP image, are added to the
//            slots and lambda <- A'mu - dl[0:nx] (the image's x0 slot is -dl[0:nx]) - or the step does not count:
//            retired (lambda <- 0), no solution or a failed factorisation (lambda <- A'mu).  `last`: lambda goes
//            to the x0 slot.
// Every sum is formed in a fixed order by one thread: the same inputs give the same bits.
struct SweepCostateArgs {
  const double *A, *B;
  long long sA, sB;
  const int* eflag;       // step k's [batch]
  const double *gu, *gx;  // step k's [batch][nu | nx], or null
  double* mu_log;         // step k's [batch][nx], or null
  fbstab_mpc_grad_batch_t grad;
  const double* tmp[FBSTAB_MPC_NSEQ];  // the image of one step (null where the slot is; x0 always)
  long long len[FBSTAB_MPC_NSEQ];
  double *seed, *lam, *atm;  // [batch][nz], [batch][nx], [batch][nx]
  const int* tmp_status;
  int* status;
  int nx, nu, nz;
};
__global__ __launch_bounds__(64) void fbstab_sweep_costate_kernel(SweepCostateArgs a, int phase, int last) {
  const long long q = blockIdx.x;
  const int t = threadIdx.x, nt = 64;
  const int nx = a.nx, nu = a.nu;
  double* lam = a.lam + q * nx;
  double* atm = a.atm + q * nx;
  if (phase == 0) {
    for (int s = 0; s < FBSTAB_MPC_NSEQ; s++)
      if (a.grad.base[s])
        for (long long e = t; e < a.len[s]; e += nt) a.grad.base[s][q * a.grad.stride[s] + e] = 0.0;
    for (int i = t; i < nx; i += nt) lam[i] = 0.0;
    for (long long i = t; i < a.nz; i += nt) a.seed[q * a.nz + i] = 0.0;
    if (t == 0) a.status[q] = 0;
    return;
  }
  if (phase == 1) {
    for (int i = t; i < nx; i += nt) {
      const double mu = (a.gx ? a.gx[q * nx + i] : 0.0) + lam[i];
      lam[i] = mu;
      if (a.mu_log) a.mu_log[q * nx + i] = mu;
    }
    __syncthreads();
    const double* Aq = a.A + q * a.sA;
    const double* Bq = a.B + q * a.sB;
    for (int i = t; i < nx; i += nt) {
      double acc = 0.0;
      for (int r = 0; r < nx; r++) acc = fma(Aq[r + (long long)i * nx], lam[r], acc);
      atm[i] = acc;
    }
    for (int j = t; j < nu; j += nt) {
      double acc = 0.0;
      for (int r = 0; r < nx; r++) acc = fma(Bq[r + (long long)j * nx], lam[r], acc);
      a.seed[q * a.nz + nx + j] = (a.gu ? a.gu[q * nu + j] : 0.0) + acc;
    }
    return;
  }
  const int e = a.eflag[q];
  const bool solved = e == FBSTAB_SUCCESS, ok = solved && a.tmp_status[q] == 0;
  if (ok)
    for (int s = 0; s < FBSTAB_MPC_NSEQ; s++)
      if (a.grad.base[s] && s != FBSTAB_MPC_x0)
        for (long long i = t; i < a.len[s]; i += nt)
          a.grad.base[s][q * a.grad.stride[s] + i] += a.tmp[s][q * a.len[s] + i];
  for (int i = t; i < nx; i += nt) {
    const double l = e == -1 ? 0.0 : (ok ? atm[i] + a.tmp[FBSTAB_MPC_x0][q * nx + i] : atm[i]);
    lam[i] = l;
    if (last && a.grad.base[FBSTAB_MPC_x0]) a.grad.base[FBSTAB_MPC_x0][q * a.grad.stride[FBSTAB_MPC_x0] + i] = l;
  }
  if (solved && !ok && t == 0) a.status[q] += 1;
}

// KGLOBAL: K in a per-workgroup global scratch (fb_dense.h); the argument is
// empty for the LDS instance, like the trace buffer for the untraced ones.
template <bool KGLOBAL>
struct KScratchArg {
  __device__ double* get() const { return nullptr; }
};
template <>
struct KScratchArg<true> {
  double* p;
  __device__ double* get() const { return p; }
};

// VGLOBAL (with KGLOBAL): the iterate vectors too live in the workgroup's global scratch
// (DenseLayout::v_global: nv beyond what the LDS holds).
template <int NT, bool TRACE = false, bool KGLOBAL = false, bool VGLOBAL = false>
__global__ __launch_bounds__(NT, (NT > 64 ? 2 : 1)) void fbstab_dense_kernel(DenseLayout lay, fbstab_dense_batch_t data,
                                                          fbstab_var_batch_t x,
                                                          fbstab_solver_out_t* out,
                                                          fbstab_options_t opts, int* counter,
                                                          int batch, TraceArg<TRACE> trace,
                                                          KScratchArg<KGLOBAL> kscratch) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  FB_WAVE_TIMER(28);  // total wave cycles (diagnostic builds)
  lds_ptr lds = (lds_ptr)smem;
  typedef Ctx<NT> C;
  C ctx;
  ctx.tid = threadIdx.x;
  ctx.red = lds + lay.o_red;
  for (;;) {
    const int q = next_qp<NT>(counter, lds + lay.o_slot);
    if (q >= batch) break;
    DenseProblem<C, KGLOBAL, VGLOBAL> p;
    double* ks = nullptr;
    if constexpr (KGLOBAL) ks = kscratch.get() + (long)blockIdx.x * (lay.k_doubles + lay.v_doubles);
    p.bind(lay, dense_data_at(data, q), var_at(x, 0, q), var_at(x, 1, q), var_at(x, 2, q), var_at(x, 3, q), lds, ks);
    Solver<DenseProblem<C, KGLOBAL, VGLOBAL>, C, TRACE> solver(p, ctx, opts, trace.get());
    solver.solve(out + q);
    ctx.sync();
  }
}

// Diagnostic probe for the dense path (tests only): one Newton step at (x, xbar,
// sigma0) for QP 0 of the batch arrays, see newton_probe.
template <int NT>
__global__ __launch_bounds__(NT, (NT > 64 ? 2 : 1)) void fbstab_dense_probe_kernel(DenseLayout lay, fbstab_dense_batch_t data,
                                                                                fbstab_var_batch_t x,
                                                                                fbstab_options_t opts, double* dbg) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  lds_ptr lds = (lds_ptr)smem;
  typedef Ctx<NT> C;
  C ctx;
  ctx.tid = threadIdx.x;
  ctx.red = lds + lay.o_red;
  DenseProblem<C, false> p;
  p.bind(lay, dense_data_at(data, 0), x.base[0], x.base[1], x.base[2], x.base[3], lds, nullptr);
  newton_probe(p, ctx, opts, dbg);
}

// One wavefront per dense QP for every phase (fb_dense_wave.h; nz + nl <= 64): the KKT
// matrix in registers, two wavefronts per SIMD.  scratch: one region of
// lay.ws_doubles per workgroup (A' and the multipliers).  DBG: the Newton-step probe.
constexpr int kDwMinWaves = 2;
template <bool DBG>
__global__ __launch_bounds__(64, kDwMinWaves) void fbstab_dense_wave_kernel(DenseWaveLayout lay, fbstab_dense_batch_t data,
                                                                   fbstab_var_batch_t x, fbstab_solver_out_t* out,
                                                                   fbstab_options_t opts, int* counter, int batch,
                                                                   double* scratch, double* dbg) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  FB_WAVE_TIMER(28);  // total wave cycles (diagnostic builds)
  lds_ptr lds = (lds_ptr)smem;
  typedef DenseWave::C C;
  C ctx;
  ctx.tid = threadIdx.x;
  ctx.red = lds;  // (unused: one wavefront reduces in registers)
  double* ws = scratch + (long)blockIdx.x * lay.ws_doubles;
  for (;;) {
    const int q = DBG ? (int)blockIdx.x : next_qp<64>(counter, lds);
    if (q >= batch) break;
    DenseWave p;
    p.bind(lay, dense_data_at(data, q), var_at(x, 0, q), var_at(x, 1, q), var_at(x, 2, q), var_at(x, 3, q), lds, ws,
           counter + kDenseFallbackSlot);
    if constexpr (DBG) {
      newton_probe(p, ctx, opts, dbg);
      break;
    } else {
      Solver<DenseWave, C> solver(p, ctx, opts);
      solver.solve(out + q);
      ctx.sync();
    }
  }
}

// The adjoint of fbstab_hip_dense_adjoint_batch (fb_dense.h: dense_adjoint, dense_adjoint_gradients; the
// contraction of fb_adjoint.h), one QP per workgroup pulled from the queue like the solve.  `x`: the point
// (z, l, v); `seed`: (gz, gl, gv), null l / v slots meaning zero; `adj`: null slots, or (dz, dl, dv).

// The four-wavefront policy (fb_dense.h), the instances of fbstab_dense_kernel: K in LDS, K in global scratch
// (KGLOBAL), the iterate vectors there too (VGLOBAL), and NT = 64.  Its factorisation always pivots.
template <int NT, bool KGLOBAL = false, bool VGLOBAL = false>
__global__ __launch_bounds__(NT, (NT > 64 ? 2 : 1)) void fbstab_dense_adjoint_kernel(
    DenseLayout lay, fbstab_dense_batch_t data, fbstab_var_batch_t x, fbstab_var_batch_t seed, fbstab_dense_grad_batch_t grad, fbstab_var_batch_t adj,
    int* status, double sigma, double alpha, int* counter, int batch, KScratchArg<KGLOBAL> kscratch) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  lds_ptr lds = (lds_ptr)smem;
  typedef Ctx<NT> C;
  C ctx;
  ctx.tid = threadIdx.x;
  ctx.red = lds + lay.o_red;
  for (;;) {
    const int q = next_qp<NT>(counter, lds + lay.o_slot);
    if (q >= batch) break;
    DenseProblem<C, KGLOBAL, VGLOBAL> p;
    double* ks = nullptr;
    if constexpr (KGLOBAL) ks = kscratch.get() + (long)blockIdx.x * (lay.k_doubles + lay.v_doubles);
    p.bind(lay, dense_data_at(data, q), var_at(x, 0, q), var_at(x, 1, q), var_at(x, 2, q), nullptr, lds, ks);
    // (the seed and adjoint slots stay written out: slot_or_null in their place re-schedules the
    // <kDenseThreads, true, true> instance - LABNOTES)
    auto at = [q](double* b, long long s) { return b ? b + q * s : nullptr; };
    const bool ok = dense_adjoint(p, ctx, sigma, alpha, seed.base[0] + q * seed.stride[0],
                                  at(seed.base[1], seed.stride[1]), at(seed.base[2], seed.stride[2]));
    ctx.sync();
    dense_adjoint_gradients(p, ctx, dense_grad_or_null(grad, q), ok, at(adj.base[0], adj.stride[0]),
                            at(adj.base[1], adj.stride[1]), at(adj.base[2], adj.stride[2]));
    if (ctx.tid == 0) status[q] = ok ? 0 : 1;
    ctx.sync();
  }
}

// The one-wavefront policy (fb_dense_wave.h; nz + nl <= 64): K in registers, A'Gamma A on the matrix cores, the
// handle's own scratch region per workgroup.  newton_step<true> factors by the pivoted rule whatever the handle's
// order, and the fallback counters of the last solve are neither passed nor reset.
__global__ __launch_bounds__(64, kDwMinWaves) void fbstab_dense_wave_adjoint_kernel(
    DenseWaveLayout lay, fbstab_dense_batch_t data, fbstab_var_batch_t x, fbstab_var_batch_t seed, fbstab_dense_grad_batch_t grad, fbstab_var_batch_t adj,
    int* status, double sigma, double alpha, int* counter, int batch, double* scratch) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  lds_ptr lds = (lds_ptr)smem;
  typedef DenseWave::C C;
  C ctx;
  ctx.tid = threadIdx.x;
  ctx.red = lds;  // (unused: one wavefront reduces in registers)
  double* ws = scratch + (long)blockIdx.x * lay.ws_doubles;
  for (;;) {
    const int q = next_qp<64>(counter, lds);
    if (q >= batch) break;
    DenseWave p;
    p.bind(lay, dense_data_at(data, q), var_at(x, 0, q), var_at(x, 1, q), var_at(x, 2, q), nullptr, lds, ws, nullptr);
    const bool ok = dense_adjoint(p, ctx, sigma, alpha, var_at(seed, 0, q), var_or_null(seed, 1, q), var_or_null(seed, 2, q));
    ctx.sync();
    dense_adjoint_gradients(p, ctx, dense_grad_or_null(grad, q), ok, var_or_null(adj, 0, q), var_or_null(adj, 1, q),
                            var_or_null(adj, 2, q));
    if (ctx.tid == 0) status[q] = ok ? 0 : 1;
    ctx.sync();
  }
}

// The direction kernels of fbstab_hip_*_tangent_batch (fb_tangent.h): the seeds (gz, gl, gv) of the tangent system
// from the perturbations `dir` (base / stride per array as in the data blocks: a null base is a zero perturbation,
// stride 0 one direction for the whole batch) and the points `x`.  No queue and no scratch: a workgroup's QP (and
// stage) is its index, so the bits of a QP's seeds depend on its own inputs only.
// MPC: one wavefront per (QP, stage), the stage's images in its LDS (MpcTangentLds).
constexpr int kDenseTangentThreads = 256;
__global__ __launch_bounds__(64) void fbstab_tangent_rhs_kernel(int N, int nx, int nu, int nc, MpcTangentLds o,
                                                                fbstab_mpc_batch_t dir, fbstab_var_batch_t x, fbstab_var_batch_t seed) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  typedef Ctx<64> C;
  C ctx;
  ctx.tid = threadIdx.x;
  ctx.red = (lds_ptr)smem;  // (unused)
  const long q = blockIdx.x / (N + 1);
  const int i = blockIdx.x % (N + 1);
  mpc_tangent_stage(ctx, N, nx, nu, nc, i, mpc_data_or_null(dir, q), var_at(x, 0, q), var_at(x, 1, q), var_at(x, 2, q),
                    o, (lds_ptr)smem, var_at(seed, 0, q), var_at(seed, 1, q), var_at(seed, 2, q));
}

// Dense: one workgroup per QP, walking the images in blocks of columns (DenseTangentLds).
__global__ __launch_bounds__(kDenseTangentThreads) void fbstab_dense_tangent_rhs_kernel(
    int nz, int nl, int nv, DenseTangentLds o, fbstab_dense_batch_t dir, fbstab_var_batch_t x, fbstab_var_batch_t seed) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  typedef Ctx<kDenseTangentThreads> C;
  C ctx;
  ctx.tid = threadIdx.x;
  ctx.red = (lds_ptr)smem;  // (unused)
  const long q = blockIdx.x;
  // (nl == 0: the l slots are null)
  dense_tangent(ctx, nz, nl, nv, dense_data_or_null(dir, q), var_at(x, 0, q), var_or_null(x, 1, q), var_at(x, 2, q), o,
                (lds_ptr)smem, var_at(seed, 0, q), var_or_null(seed, 1, q), var_at(seed, 2, q));
}

}  // namespace

// The host staging of every entry point below (fb_host_stage.h, and the sweeps' beside it): no device code, and tested
// on the CPU (tests/test_host_stage.py).
#include "fb_sweep_stage.h"

// An entry of an MPC handle's table.  The kernels of a record instance share one argument list and run in the
// handle's scratch; the flat-vector kernels share another (the adjoint a third) and run in `ws`.
struct MpcKernel : KernelEntry {
  bool record = false;
  enum Ws { kHandle, kTrace, kAdjoint } ws = kHandle;  // (flat_workspace)
};

struct fbstab_mpc_solver : SolverBase {
  fbk::MpcLayout lay;
  const RecordInstance* rec = nullptr;  // record kernel (fb_mpc_r16.h) serving this shape, or the flat-vector kernel
  bool exact = false;     // the problem has exactly the instance's shape
  int kept_batch = -1;    // batch size of the last FBSTAB_HIP_KEEP_MATRICES call whose copies are still in the slots
  int qps_per_wg = 1;
  // fbstab_hip_mpc_adjoint_batch: a record handle on the flat-vector adjoint (FBSTAB_HIP_FLAT_ADJOINT at creation;
  // the row-pair instances' default) - then with a scratch of the flat kernel's own (the handle's is laid out for
  // the record kernel), allocated by the first call
  bool flat_adjoint = false;
  double* adj_scratch = nullptr;
  // fbstab_hip_mpc_receding_sweep_adjoint, allocated by the first call that needs them (sweep_adjoint_run): the seed
  // vectors of the one-launch kernel (nz doubles per row slot of the grid) and the per-step form's image of one step
  SweepScratch sweep;
  // The longest-first queue (fb_queue_order_plan.h): whether this handle keeps an order at all (record handles,
  // FBSTAB_HIP_QUEUE_ORDER at creation), the QP indices by descending Newton count of the last packed batch solve
  // (max_batch ints, written by fbstab_mpc_queue_order_kernel behind that solve; the kernel's counters behind them:
  // queue_order_ints), and the batch size they are valid for, or -1
  bool queue_order = false;
  int* order = nullptr;
  int order_batch = -1;
  // What this handle launches (mpc_resolve_kernels).  solve_keep: record handles only; adjoint: on the record or
  // the flat-vector kernel (`record`); sweep_adjoint: null where the sweep adjoint runs per step; kkt_multi: the
  // flat-vector kernel of fb_kkt_multi.hip on every handle.
  struct {
    MpcKernel solve, solve_keep, traced, probe, adjoint, sweep_adjoint, kkt_multi;
  } kern;

  ~fbstab_mpc_solver() {
    (void)hipSetDevice(device);
    if (adj_scratch) (void)hipFree(adj_scratch);
    if (sweep.seed) (void)hipFree(sweep.seed);
    if (sweep.tmp) (void)hipFree(sweep.tmp);
    if (order) (void)hipFree(order);
  }
  // Grid of a batch launch of entry `e` (fbk::batch_grid: a record kernel's small batches are spread)
  int batch_grid(const MpcKernel& e, int batch) const {
    return fbk::batch_grid(batch, workgroups, e.record ? qps_per_wg : 1);
  }
};

// The record-kernel instances compiled into the library (one translation unit each),
// smallest first: a shape runs on the first one it fits (zero-padded unless it is that
// instance's own).
FB_RECORD_INSTANCE_DECL(12, 4, 20, 1)
// the same stage width with up to two constraint rows per stage variable (two-sided
// bounds on all of x and u written as 32 rows); a third of its registers' worth of
// constraint slots more than the instance above, so that one stays the first choice
FB_RECORD_INSTANCE_DECL(12, 4, 32, 1)
// two 16-lane rows per QP: 16 < nx + nu <= 23 (the reference's copolymerization
// reactor, nx = 18, nu = 5, nc = 10: fbstab/test/ocp_generator.cc:73-174)
FB_RECORD_INSTANCE_DECL(18, 5, 10, 2)
// any stage width up to 32 (nx <= 24, nu <= 8) with up to 16 or 32 constraint rows: a row
// of a 32-wide stage matrix per lane is more than the register file holds (660-850
// spilled registers), three to four times the flat-vector kernel all the same
FB_RECORD_INSTANCE_DECL(24, 8, 16, 2)
FB_RECORD_INSTANCE_DECL(24, 8, 32, 2)
// fbstab_mpc_kkt_multi_kernel (fb_kkt_multi.hip, a translation unit of its own): [wglobal != 0] the stage tile and the
// work matrices in global scratch, or everything in LDS
__attribute__((visibility("hidden"))) const void* fbstab_kkt_multi_kernel(int wglobal);
// fbstab_dense_kkt_multi_kernel / fbstab_dense_wave_kkt_multi_kernel (fb_dense_kkt_multi.hip, a translation unit of its
// own): the kernel beside adjoint kernel `which` of dense_resolve_kernels
__attribute__((visibility("hidden"))) const void* fbstab_dense_kkt_multi_kernel_for(int which);
// The kernels of the condensed route (fb_condense.hip, fb_condense_adjoint.hip, fb_condense_multi.hip,
// fb_condense_sweep.hip, fb_condense_sweep_adjoint.hip, fb_condense_sweep_tangent.hip, fb_condense_tangent.hip,
// fb_condense_refs.hip, a translation unit each): the kernel
// that the unit's enum of fb_condense_plan.h names; *threads: its workgroup size
__attribute__((visibility("hidden"))) const void* fbstab_condense_kernel(fbk::CondenseKernel which, int* threads);
__attribute__((visibility("hidden"))) const void* fbstab_condense_kernel(fbk::CondenseAdjointKernel which, int* threads);
__attribute__((visibility("hidden"))) const void* fbstab_condense_kernel(fbk::CondenseMultiKernel which, int* threads);
__attribute__((visibility("hidden"))) const void* fbstab_condense_kernel(fbk::CondenseSweepKernel which, int* threads);
__attribute__((visibility("hidden"))) const void* fbstab_condense_kernel(fbk::CondenseSweepAdjKernel which, int* threads);
__attribute__((visibility("hidden"))) const void* fbstab_condense_kernel(fbk::CondenseSweepTanKernel which, int* threads);
__attribute__((visibility("hidden"))) const void* fbstab_condense_kernel(fbk::CondenseTangentKernel which, int* threads);
__attribute__((visibility("hidden"))) const void* fbstab_condense_kernel(fbk::CondenseRefsKernel which, int* threads);
#if defined(FB_SINGLE_TU)
// (diagnostic builds with device-side counters: one translation unit, one g_stamps)
#include "rec_12_4_20.hip"
#include "rec_12_4_32.hip"
#include "rec_18_5_10.hip"
#include "rec_24_8_16.hip"
#include "rec_24_8_32.hip"
#include "fb_kkt_multi.hip"
#include "fb_dense_kkt_multi.hip"
#include "fb_condense.hip"
#include "fb_condense_adjoint.hip"
#include "fb_condense_multi.hip"
#include "fb_condense_sweep.hip"
#include "fb_condense_sweep_adjoint.hip"
#include "fb_condense_sweep_tangent.hip"
#include "fb_condense_tangent.hip"
#include "fb_condense_refs.hip"
#endif

// The condensed route (include/fbstab_hip.h): its host side is fb_condense_stage.h, tested on the CPU
// (tests/test_condense_stage.py); here, what that header is handed: the kernels of the route's units, and the dense
// handle's own entry points on device pointers, asynchronous.
#include "fb_condense_stage.h"

namespace {
const auto condense_gpu = [](auto id, int grid, long long lds, void** args, hipStream_t s) {
  return condense_launch([](auto k, int* threads) { return fbstab_condense_kernel(k, threads); }, id, grid, lds, args, s);
};
constexpr int kCondenseDenseFlags = FBSTAB_HIP_DEVICE_POINTERS | FBSTAB_HIP_ASYNC;
auto condense_dense_adjoint(fbstab_dense_handle_t h) {
  return [h](int batch, const fbstab_dense_batch_t* dc, const fbstab_var_batch_t* xc, const fbstab_var_batch_t* seeds,
             double sigma, const fbstab_var_batch_t* adj, int* status, hipStream_t s) {
    const fbstab_dense_grad_batch_t none = {};  // (no gradients of the condensed data)
    return fbstab_hip_dense_adjoint_batch(h, batch, dc, xc, seeds, sigma, &none, adj, status, kCondenseDenseFlags, (void*)s);
  };
}
// The direction kernel of the forward mode on the grid batch x (N + 1), behind the limits of its own LDS layout
// (fb_tangent.h: MpcTangentLds) and of the grid.
const auto condense_tangent_direction = [](int N, int nx, int nu, int nc, int batch, fbstab_mpc_batch_t dir,
                                           fbstab_var_batch_t x, fbstab_var_batch_t seed, hipStream_t s) {
  MpcTangentLds o;
  o.init(nx, nu, nc);
  if ((long long)o.total * 8 > kLdsLimitBytes)
    return fail(FBSTAB_HIP_ERR_UNSUPPORTED,
                "condensed tangent: the perturbation images of one stage do not fit the 160 KiB LDS budget");
  if ((long long)batch * (N + 1) > 0x7fffffffLL)
    return condense_bad("condensed tangent", "batch x stages exceeds the grid limit");
  void* args[] = {&N, &nx, &nu, &nc, &o, &dir, &x, &seed};
  return condense_gpu(kCondenseTangentRhs, batch * (N + 1), (long long)o.total * 8, args, s);
};
auto condense_dense_multi(fbstab_dense_handle_t h) {
  return [h](int batch, const fbstab_dense_batch_t* dc, const fbstab_var_batch_t* xc, int nrhs,
             const fbstab_multi_var_batch_t* seeds, double sigma, const fbstab_multi_var_batch_t* step, int* status,
             hipStream_t s) {
    return fbstab_hip_dense_kkt_solve_batch(h, batch, dc, xc, nrhs, seeds, sigma, step, status, kCondenseDenseFlags, (void*)s);
  };
}
}  // namespace

namespace {
const RecordInstance* record_instances(int* count) {
  static const RecordInstance table[] = {
      fbstab_record_instance_12_4_20_1(),
      fbstab_record_instance_12_4_32_1(),
      fbstab_record_instance_18_5_10_2(),
      fbstab_record_instance_24_8_16_2(),
      fbstab_record_instance_24_8_32_2(),
  };
  *count = (int)(sizeof(table) / sizeof(table[0]));
  return table;
}
const RecordInstance* record_instance_for(int nx, int nu, int nc) {
  int n = 0;
  const RecordInstance* t = record_instances(&n);
  for (int i = 0; i < n; i++)
    if (nx <= t[i].nx && nu <= t[i].nu && nc <= t[i].nc) return &t[i];
  return nullptr;
}

// The problem data of a record kernel: the block and the problem's own sizes.
MpcBatchPtrs record_data(const fbstab_mpc_solver* h, const fbstab_mpc_batch_t& a) {
  return MpcBatchPtrs{a, h->lay.nx, h->lay.nu, h->lay.nc};
}

// The workspace of a flat-vector kernel: the handle's own, the traced solve's (one QP's, kept from call to call), or
// that of the flat-vector adjoint on a record handle (lay.ws_doubles x workgroups doubles; fbstab_hip_mpc_query does
// not count it) - the last two allocated by the first launch that needs them.
int flat_workspace(fbstab_mpc_solver* h, const MpcKernel& e, double** ws) {
  double** own = e.ws == MpcKernel::kTrace ? &h->trace_ws : e.ws == MpcKernel::kAdjoint ? &h->adj_scratch : &h->scratch;
  const size_t slots = e.ws == MpcKernel::kAdjoint ? (size_t)h->workgroups : 1;
  if (!*own) HIP_TRY(hipMalloc(own, sizeof(double) * (size_t)h->lay.ws_doubles * slots));
  *ws = *own;
  return FBSTAB_HIP_OK;
}

// Launches a solve, traced solve or probe entry: one argument list for the kernels of a record instance, one for
// the flat-vector kernels.
int launch_mpc(fbstab_mpc_solver* h, MpcKernel& e, int grid, hipStream_t s, const fbstab_mpc_batch_t& a,
               fbstab_var_batch_t x, fbstab_solver_out_t* out, int batch, double* dbg, bool reuse) {
  if (e.record) {
    MpcBatchPtrs d = record_data(h, a);
    int N = h->lay.N, ru = reuse ? 1 : 0;
    void* args[] = {&d, &x, &out, &h->opts, &h->scratch, &h->counter, &batch, &N, &ru, &dbg};
    return launch_entry(e, grid, args, s);
  }
  double* ws;
  RC_TRY(flat_workspace(h, e, &ws));
  void* args[] = {&h->lay, const_cast<fbstab_mpc_batch_t*>(&a), &x, &out, &h->opts, &ws, &h->counter, &batch, &dbg};
  return launch_entry(e, grid, args, s);
}

// The one place that knows which compiled kernel serves which operation of an MPC handle, with what block, LDS
// size and workspace: read once, when the handle is created, behind the layout and the knobs that choose
// (FBSTAB_HIP_GENERIC, FBSTAB_HIP_FLAT_ADJOINT, FBSTAB_HIP_LDS_PAD_BYTES).
void mpc_resolve_kernels(fbstab_mpc_solver* h) {
  // the flat-vector kernels, [0] with the stage tile and the work matrices in global scratch (MpcLayout::wglobal),
  // [1] with everything in LDS.  (Named in the order the compiler has always met them: the code of some kernels
  // of this file depends on it - tools/diff_device_code.py.)
  const void* const solve_probe[2][2] = {{kernel_ptr(fbstab_mpc_kernel<kMpcThreads, false, false, true>),
                                          kernel_ptr(fbstab_mpc_kernel<kMpcThreads, true, false, true>)},
                                         {kernel_ptr(fbstab_mpc_kernel<kMpcThreads, false>),
                                          kernel_ptr(fbstab_mpc_kernel<kMpcThreads, true>)}};
  const void* const traced[2] = {kernel_ptr(fbstab_mpc_kernel<kMpcThreads, false, true, true>),
                                 kernel_ptr(fbstab_mpc_kernel<kMpcThreads, false, true, false>)};
  const void* const adjoint[2] = {kernel_ptr(fbstab_mpc_adjoint_kernel<kMpcThreads, true>),
                                  kernel_ptr(fbstab_mpc_adjoint_kernel<kMpcThreads, false>)};
  const int f = h->lay.wglobal ? 0 : 1;
  const char* const flat_name = "fbstab_mpc_kernel<64>";
  // what the flat-vector kernels ask for, whatever the handle's lds_bytes (a record instance's, or padded) says
  const int flat_lds = h->lay.launch_lds_doubles * (int)sizeof(double);
  const int lds = h->lds_bytes;
  auto& k = h->kern;
  if (h->rec) {
    const RecordInstance& r = *h->rec;
    const RecordKernels& rk = h->exact ? r.exact : r.padded;
    k.solve = {{rk.solve, r.name, kMpcThreads, lds}, true, MpcKernel::kHandle};
    k.solve_keep = {{rk.solve_keep, r.name, kMpcThreads, lds}, true, MpcKernel::kHandle};
    k.probe = {{rk.probe, r.name, kMpcThreads, lds}, true, MpcKernel::kHandle};
    if (!h->flat_adjoint) {
      k.adjoint = {{rk.adjoint, r.adjoint_name, kMpcThreads, lds}, true, MpcKernel::kHandle};
      k.sweep_adjoint = {{rk.sweep_adjoint, r.sweep_adjoint_name, kMpcThreads, lds}, true, MpcKernel::kHandle};
    }
  } else {
    k.solve = {{solve_probe[f][0], flat_name, kMpcThreads, lds}, false, MpcKernel::kHandle};
    k.probe = {{solve_probe[f][1], flat_name, kMpcThreads, lds}, false, MpcKernel::kHandle};
  }
  // the traced solve runs on the flat-vector kernel on every handle
  k.traced = {{traced[f], flat_name, kMpcThreads, flat_lds}, false, MpcKernel::kTrace};
  if (!k.adjoint.kern)
    k.adjoint = {{adjoint[f], "fbstab_mpc_adjoint_kernel<64>", kMpcThreads, flat_lds}, false,
                 h->rec ? MpcKernel::kAdjoint : MpcKernel::kHandle};
  // many right-hand sides on one factorisation: the flat-vector layout on every handle, a record handle in the
  // flat adjoint's scratch (its own is laid out for the record kernel and is not touched)
  k.kkt_multi = {{fbstab_kkt_multi_kernel(h->lay.wglobal), "fbstab_mpc_kkt_multi_kernel<64>", kMpcThreads, flat_lds},
                 false, h->rec ? MpcKernel::kAdjoint : MpcKernel::kHandle};
}
}  // namespace

// An entry of a dense handle's table.  `wave`: a one-wavefront kernel (the wave layout, the handle's scratch as a
// plain pointer); otherwise a four-wavefront kernel on the layout `lay`, the handle's scratch in its KScratchArg
// where the instance keeps K there (`kscratch`).
struct DenseKernel : KernelEntry {
  bool wave = false, kscratch = false;
  const fbk::DenseLayout* lay = nullptr;
};

struct fbstab_dense_solver : SolverBase {
  fbk::DenseLayout lay;
  // one wavefront per QP with the KKT matrix in registers (fb_dense_wave.h): the
  // kernel batches of nz + nl <= 64 run on; `lay` then only serves the traced solve
  bool wave = false;
  fbk::DenseWaveLayout wlay;
  fbk::DenseLayout trace_lay;  // the traced solve's own layout, where the handle's K fits the LDS
  // What this handle launches (dense_resolve_kernels).  traced, probe: null where the layout does not serve them;
  // kkt_multi: the many-right-hand-side kernel beside the adjoint kernel (fb_dense_kkt_multi.hip).
  struct {
    DenseKernel solve, traced, probe, adjoint, kkt_multi;
  } kern;
};

namespace {
// The one place that knows which compiled kernel serves which operation of a dense handle, with what block, LDS
// size, layout and scratch: read once, when the handle is created, behind the layouts and FBSTAB_HIP_DENSE_THREADS.
void dense_resolve_kernels(fbstab_dense_solver* h) {
  const fbk::DenseLayout& L = h->lay;
  // [0] the one-wavefront policy; the four-wavefront policy with [1] NT = 64, [2] K and the iterate vectors in global
  // scratch (DenseLayout::v_global), [3] K there (k_global), [4] everything in LDS.  The probe: K in LDS only; the
  // traced solve: [2], [3], or the LDS instance on a layout of its own.  (Named in the order the compiler has always
  // met them: the code of some kernels of this file depends on it - tools/diff_device_code.py.)
  const int i = h->wave ? 0 : h->threads == 64 ? 1 : L.v_global ? 2 : L.k_global ? 3 : 4;
  const void* const solve[] = {kernel_ptr(fbstab_dense_wave_kernel<false>), kernel_ptr(fbstab_dense_kernel<64>),
                               kernel_ptr(fbstab_dense_kernel<kDenseThreads, false, true, true>),
                               kernel_ptr(fbstab_dense_kernel<kDenseThreads, false, true>),
                               kernel_ptr(fbstab_dense_kernel<kDenseThreads>)};
  const void* const wave_probe = kernel_ptr(fbstab_dense_wave_kernel<true>);
  const void* const traced[] = {kernel_ptr(fbstab_dense_kernel<kDenseThreads, true, true, true>),
                                kernel_ptr(fbstab_dense_kernel<kDenseThreads, true, true>),
                                kernel_ptr(fbstab_dense_kernel<kDenseThreads, true>)};
  const void* const probe[] = {wave_probe, kernel_ptr(fbstab_dense_probe_kernel<64>), nullptr, nullptr,
                               kernel_ptr(fbstab_dense_probe_kernel<kDenseThreads>)};
  const void* const adjoint[] = {kernel_ptr(fbstab_dense_wave_adjoint_kernel),
                                 kernel_ptr(fbstab_dense_adjoint_kernel<64>),
                                 kernel_ptr(fbstab_dense_adjoint_kernel<kDenseThreads, true, true>),
                                 kernel_ptr(fbstab_dense_adjoint_kernel<kDenseThreads, true>),
                                 kernel_ptr(fbstab_dense_adjoint_kernel<kDenseThreads>)};
  const fbk::DenseLayout* lay = h->wave ? nullptr : &h->lay;
  const bool ks = L.k_global != 0;  // (never on a one-wavefront handle: its K is 64 x 64 at the most)
  h->kern.solve = {{solve[i], "", h->threads, h->lds_bytes}, h->wave, ks, lay};
  h->kern.probe = {{probe[i], "", h->threads, h->lds_bytes}, h->wave, ks, lay};
  h->kern.adjoint = {{adjoint[i], "", h->threads, h->lds_bytes}, h->wave, ks, lay};
  h->kern.kkt_multi = {{fbstab_dense_kkt_multi_kernel_for(i), "", h->threads, h->lds_bytes}, h->wave, ks, lay};
  if (L.k_global) {
    h->kern.traced = {{traced[L.v_global ? 0 : 1], "", h->threads, h->lds_bytes}, false, true, &h->lay};
  } else {
    // the traced instance is the four-wavefront kernel with a layout of its own (left null where that one does
    // not fit: the traced solve refuses the call)
    h->trace_lay.init(L.nz, L.nl, L.nv, kDenseThreads);
    const int tlds = h->trace_lay.lds_doubles * (int)sizeof(double);
    if (!h->trace_lay.k_global && tlds <= kLdsLimitBytes)
      h->kern.traced = {{traced[2], "", kDenseThreads, tlds}, false, false, &h->trace_lay};
  }
}

// Launches a solve, traced solve or (one-wavefront handles) probe entry: one argument list for the one-wavefront
// kernels - `dbg`: the probe's io, or null -, one for the four-wavefront kernels - `dbg`: the trace buffer, or null.
int launch_dense(fbstab_dense_solver* h, DenseKernel& e, int grid, hipStream_t s, fbstab_dense_batch_t a,
                 fbstab_var_batch_t x, fbstab_solver_out_t* out, int batch, double* dbg) {
  if (e.wave) {
    void* args[] = {&h->wlay, &a, &x, &out, &h->opts, &h->counter, &batch, &h->scratch, &dbg};
    return launch_entry(e, grid, args, s);
  }
  // (the untraced instances take an empty TraceArg, the ones with K in LDS an empty KScratchArg)
  TraceArg<true> trace{dbg};
  TraceArg<false> no_trace;
  KScratchArg<true> ks{h->scratch};
  KScratchArg<false> no_ks;
  void* args[] = {const_cast<fbk::DenseLayout*>(e.lay), &a, &x, &out, &h->opts, &h->counter, &batch,
                  dbg ? (void*)&trace : (void*)&no_trace, e.kscratch ? (void*)&ks : (void*)&no_ks};
  return launch_entry(e, grid, args, s);
}
}  // namespace

extern "C" {

const char* fbstab_hip_last_error(void) { return g_error.c_str(); }

int fbstab_hip_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

// ---------------------------------------------------------------------------
int fbstab_hip_mpc_create(int N, int nx, int nu, int nc, int max_batch, int device,
                          fbstab_mpc_handle_t* handle) {
  return fbstab_hip_mpc_create_in_flight(N, nx, nu, nc, max_batch, device, 1, handle);
}

int fbstab_hip_mpc_create_in_flight(int N, int nx, int nu, int nc, int max_batch, int device, int handles_in_flight,
                                    fbstab_mpc_handle_t* handle) {
  if (!handle) return fail(FBSTAB_HIP_ERR_ARGUMENT, "null handle pointer");
  if (handles_in_flight < 1 || handles_in_flight > 64) return fail(FBSTAB_HIP_ERR_ARGUMENT, "handles_in_flight must be in 1..64");
  *handle = nullptr;
  // fbstab_mpc.cc:62-65
  if (N < 1 || nx < 1 || nu < 1 || nc < 1)
    return fail(FBSTAB_HIP_ERR_ARGUMENT, "In FBstabMpc::FBstabMpc: problem sizes must be positive.");
  if (max_batch < 1) return fail(FBSTAB_HIP_ERR_ARGUMENT, "max_batch must be positive");
  std::unique_ptr<fbstab_mpc_solver> s(new (std::nothrow) fbstab_mpc_solver());
  if (!s) return fail(FBSTAB_HIP_ERR_DEVICE, "out of host memory");
  const fbk::CreateKnobs knobs = fbk::create_knobs();
  s->threads = kMpcThreads;
  s->lay.init(N, nx, nu, nc, s->threads);
  s->lds_bytes = s->lay.launch_lds_doubles * (int)sizeof(double);
  if (!knobs.generic) s->rec = record_instance_for(nx, nu, nc);
  if (s->rec) {
    s->exact = nx == s->rec->nx && nu == s->rec->nu && nc == s->rec->nc;
    s->qps_per_wg = s->rec->qps_per_wg;
    s->flat_adjoint = knobs.flat_adjoint >= 0 ? knobs.flat_adjoint > 0 : s->rec->qps_per_wg != 4;
    s->lds_bytes = s->rec->lds_bytes(N);
  }
  s->lds_bytes += knobs.lds_pad_bytes;
  if (s->lds_bytes > kLdsLimitBytes)  // (not reached: the flat-vector layout moves to global scratch first)
    return fail(FBSTAB_HIP_ERR_UNSUPPORTED, "stage vectors do not fit the 160 KiB LDS budget");
  RC_TRY(s->common_init(device, max_batch));
  mpc_resolve_kernels(s.get());
  int occupancy = 0, cus = 0;
  RC_TRY(s->occupancy(s->kern.solve, &occupancy, &cus));
  const fbk::LaunchPlan plan =
      fbk::mpc_plan(cus, occupancy, handles_in_flight, fbk::hw_queues_hint(), s->rec != nullptr, s->qps_per_wg, max_batch,
                    s->rec ? s->rec->ws_doubles(N) : (long long)s->lay.ws_doubles, knobs);
  s->workgroups = plan.workgroups;
  s->scratch_bytes = plan.scratch_bytes;
  hipError_t e = hipMalloc(&s->scratch, (size_t)s->scratch_bytes);
  if (e != hipSuccess) return fail(FBSTAB_HIP_ERR_DEVICE, std::string("scratch allocation: ") + hipGetErrorString(e));
  s->queue_order = s->rec != nullptr && fbk::queue_order_knob();
  if (s->queue_order) HIP_TRY(hipMalloc(&s->order, sizeof(int) * fbk::queue_order_ints(max_batch)));
  const fbk::MpcLayout& L = s->lay;
  s->arr_len = {(long long)(N + 1) * nx * nx, (long long)(N + 1) * nu * nu,
                (long long)(N + 1) * nu * nx, (long long)(N + 1) * nx, (long long)(N + 1) * nu,
                (long long)N * nx * nx, (long long)N * nx * nu, (long long)N * nx,
                (long long)(N + 1) * nc * nx, (long long)(N + 1) * nc * nu,
                (long long)(N + 1) * nc, (long long)nx};
  s->var_len[0] = L.nz; s->var_len[1] = L.nl; s->var_len[2] = L.nv; s->var_len[3] = L.nv;
  *handle = s.release();
  return FBSTAB_HIP_OK;
}

int fbstab_hip_mpc_destroy(fbstab_mpc_handle_t h) {
  delete h;
  return FBSTAB_HIP_OK;
}

int fbstab_hip_mpc_set_options(fbstab_mpc_handle_t h, const fbstab_options_t* o) {
  if (!h || !o) return fail(FBSTAB_HIP_ERR_ARGUMENT, "null argument");
  h->opts = *o;
  fbstab_options_validate(&h->opts);  // UpdateParameters -> ValidateOptions
  return FBSTAB_HIP_OK;
}
int fbstab_hip_mpc_get_options(fbstab_mpc_handle_t h, fbstab_options_t* o) {
  if (!h || !o) return fail(FBSTAB_HIP_ERR_ARGUMENT, "null argument");
  *o = h->opts;
  return FBSTAB_HIP_OK;
}

// solve_batch; with d_trace != nullptr the ONE QP of the call runs on the traced
// instance of the flat-vector kernel instead (fbstab_hip_mpc_solve_traced).
// norms != nullptr: the component norms of the summary block follow the solve
// (fbstab_hip_mpc_solve_batch_final); they live where `out` lives.
static int mpc_solve_impl(fbstab_mpc_handle_t h, int batch, const fbstab_mpc_batch_t* data,
                          const fbstab_var_batch_t* x, fbstab_solver_out_t* out, int flags,
                          void* stream, double* d_trace, double* norms = nullptr) {
  auto launch = [=](hipStream_t s, const fbstab_mpc_batch_t& a, const fbstab_var_batch_t& v,
                    fbstab_solver_out_t* d_out) -> int {
    // FBSTAB_HIP_KEEP_MATRICES (record handles): one QP per slot, slot = QP index
    const bool keep = !d_trace && h->rec && (flags & FBSTAB_HIP_KEEP_MATRICES) &&
                      (flags & FBSTAB_HIP_DEVICE_POINTERS) && fbk::slots_hold(batch, h->workgroups, h->qps_per_wg);
    const bool reuse = keep && h->kept_batch == batch;
    MpcKernel& e = d_trace ? h->kern.traced : keep ? h->kern.solve_keep : h->kern.solve;
    // (the traced solve: the call's one QP on one workgroup, `d_trace` in the probe's place)
    const int grid = keep ? fbk::keep_grid(batch, h->qps_per_wg) : h->batch_grid(e, batch);
    // The batch solve of a record instance, packed: its tickets go out in the order the previous solve of this
    // batch left (longest QP first; the kernel's `dbg`, which the untraced batch instance has no other use for),
    // and its own Newton counts are sorted behind it for the next one (fb_queue_order_plan.h)
    const bool record_batch_solve = !d_trace && !keep && e.record;
    const bool spread = fbk::record_spreads(batch, grid);
    const bool ordered = fbk::queue_order_applies(h->queue_order, record_batch_solve, spread, batch, h->order_batch);
    double* const dbg = ordered ? reinterpret_cast<double*>(h->order) : d_trace;
    RC_TRY(launch_mpc(h, e, grid, s, a, v, d_out, batch, dbg, reuse));
    if (!d_trace) h->kept_batch = keep ? batch : -1;  // (the traced solve leaves the slots alone)
    if (fbk::queue_order_sorts(h->queue_order, record_batch_solve, spread, batch)) {
      h->order_batch = -1;  // (until the kernel that writes the new one is queued)
      hipLaunchKernelGGL(fbk::fbstab_mpc_queue_order_kernel, dim3(1), dim3(fbk::kQueueOrderThreads), 0, s, d_out, batch,
                         h->order, h->order + h->max_batch);
      HIP_TRY(hipGetLastError());
      h->order_batch = batch;
    }
    return FBSTAB_HIP_OK;
  };
  auto launch_norms = [=](hipStream_t s, const fbstab_mpc_batch_t& a, const fbstab_var_batch_t& v, double* dn) {
    const MpcNormArgs na = {a, v, h->lay.N, h->lay.nx, h->lay.nu, h->lay.nc};
    hipLaunchKernelGGL(fbstab_mpc_final_norms_kernel, dim3(batch), dim3(64), 0, s, na, h->opts, dn, batch);
  };
  return solve_run(h, batch, data, x, out, flags, stream, norms, launch, launch_norms);
}

int fbstab_hip_mpc_solve_batch_final(fbstab_mpc_handle_t h, int batch, const fbstab_mpc_batch_t* data,
                                     const fbstab_var_batch_t* x, fbstab_solver_out_t* out, double* norms,
                                     int flags, void* stream) {
  if (!norms) return fail(FBSTAB_HIP_ERR_ARGUMENT, "null norms pointer");
  return mpc_solve_impl(h, batch, data, x, out, flags, stream, nullptr, norms);
}

int fbstab_hip_mpc_solve_batch(fbstab_mpc_handle_t h, int batch, const fbstab_mpc_batch_t* data,
                               const fbstab_var_batch_t* x, fbstab_solver_out_t* out, int flags,
                               void* stream) {
  return mpc_solve_impl(h, batch, data, x, out, flags, stream, nullptr);
}

int fbstab_hip_mpc_solve_traced(fbstab_mpc_handle_t h, const fbstab_mpc_batch_t* data,
                                const fbstab_var_batch_t* x, fbstab_solver_out_t* out,
                                fbstab_trace_record_t* trace, int capacity, int* count) {
  if (!h) return fail(FBSTAB_HIP_ERR_ARGUMENT, "null solver handle");
  TraceBuf tb;
  int rc = tb.open(h->device, trace, capacity, count);
  if (rc != FBSTAB_HIP_OK) return rc;
  rc = mpc_solve_impl(h, 1, data, x, out, FBSTAB_HIP_HOST_POINTERS, nullptr, tb.dev());
  if (rc != FBSTAB_HIP_OK) return rc;
  return tb.close(trace, capacity, count);
}

// What the sweeps' host stages (fb_sweep_stage.h) read of a handle.
static SweepShape sweep_shape(const fbstab_mpc_solver* h) {
  if (!h) return SweepShape{};
  return SweepShape{h->lay.N, h->lay.nx, h->lay.nu, h->lay.nc, h->rec != nullptr, h->qps_per_wg,
                    h->kern.sweep_adjoint.kern != nullptr};
}

// BASELINE configs[4]: `steps` closed-loop steps without a host round trip in
// between - solve, plant step, solve, ... queued on one stream: sweep_run on the real launches.
// (`log`: fbstab_hip_mpc_receding_sweep_logged; null: nothing is logged.  `sc`:
// fbstab_hip_mpc_receding_sweep_scenario; null: no disturbance, no shift)
static int mpc_receding_sweep_impl(fbstab_mpc_handle_t h, int batch, const fbstab_mpc_batch_t* data,
                                   const fbstab_var_batch_t* x, fbstab_solver_out_t* out,
                                   const fbstab_receding_plant_t* plant, int steps, int retire, double* u_log,
                                   unsigned long long* stats, float* kernel_ms, void* stream,
                                   const fbstab_sweep_log_t* log, const fbstab_sweep_scenario_t* sc = nullptr) {
  // (the callables run behind sweep_run's checks: h, data, x and plant are there)
  auto x0 = [=] { return const_cast<double*>(data->base[FBSTAB_MPC_x0]); };
  auto fill_args = [=](SweepArgs* sa, unsigned long long* d_stats, int* d_ret) {
    const fbk::MpcLayout& L = h->lay;
    sa->A = plant->A; sa->B = plant->B; sa->sA = plant->stride_A; sa->sB = plant->stride_B;
    sa->x0 = x0(); sa->sx0 = data->stride[FBSTAB_MPC_x0];
    sa->u_log = u_log; sa->stats = d_stats;
    sa->steps = steps; sa->retire = retire;
    sa->nx = L.nx; sa->nu = L.nu; sa->nz = L.nz; sa->nl = L.nl; sa->nv = L.nv;
    sa->log_z = log ? log->z : nullptr; sa->log_l = log ? log->l : nullptr; sa->log_v = log ? log->v : nullptr;
    sa->log_x0 = log ? log->x0 : nullptr; sa->log_eflag = log ? log->eflag : nullptr;
    sa->w = sc ? sc->w : nullptr; sa->shift = sc && sc->shift == 1 ? 1 : 0; sa->N = L.N; sa->nc = L.nc;
    sa->lpq = 64 / h->qps_per_wg; sa->cnt = d_ret;
    for (int i = 0; i < 3; i++) { sa->xb[i] = x->base[i]; sa->sxb[i] = x->stride[i]; }
  };
  auto one_launch = [=](hipStream_t s, double* d_sa) -> int {
    HIP_TRY(hipMemsetAsync(h->counter, 0, kQueueBytes, s));
    RC_TRY(h->begin_timed(s));
    RC_TRY(launch_mpc(h, h->kern.solve_keep, fbk::keep_grid(batch, h->qps_per_wg), s, *data, *x, out, batch, d_sa, false));
    RC_TRY(h->end_timed(s));
    h->kept_batch = batch;
    return FBSTAB_HIP_OK;
  };
  auto solve = [=](hipStream_t s, int k) {
    if (k == 0) h->kept_batch = -1;  // the first step builds the matrix copies
    return mpc_solve_impl(h, batch, data, x, out, FBSTAB_HIP_DEVICE_POINTERS | FBSTAB_HIP_ASYNC | FBSTAB_HIP_KEEP_MATRICES,
                          s, nullptr);
  };
  auto plant_step = [=](hipStream_t s, const SweepStep& st, int* d_ret, double* d_xtmp) {
    const fbk::MpcLayout& L = h->lay;
    const SweepLogStep lg = {st.z, st.l, st.v, st.x0, st.eflag};
    hipLaunchKernelGGL(fbstab_receding_plant_kernel, dim3((batch + 63) / 64), dim3(64), 0, s, batch, L.nx, L.nu,
                       L.nz, L.nl, L.nv, plant->A, plant->stride_A, plant->B, plant->stride_B, x0(),
                       data->stride[FBSTAB_MPC_x0], *x, out, d_ret, retire, st.u_log, st.stats, d_xtmp, lg, st.w,
                       st.shift_stages, L.nc);
  };
  return sweep_run<SweepArgs>(h, sweep_shape(h), batch, data, x, out, plant, steps, u_log, stats, kernel_ms, stream,
                              log, sc, fill_args, one_launch, solve, plant_step);
}

int fbstab_hip_mpc_receding_sweep(fbstab_mpc_handle_t h, int batch, const fbstab_mpc_batch_t* data,
                                  const fbstab_var_batch_t* x, fbstab_solver_out_t* out,
                                  const fbstab_receding_plant_t* plant, int steps, int retire,
                                  double* u_log, unsigned long long* stats, float* kernel_ms, void* stream) {
  return mpc_receding_sweep_impl(h, batch, data, x, out, plant, steps, retire, u_log, stats, kernel_ms, stream, nullptr);
}

int fbstab_hip_mpc_receding_sweep_logged(fbstab_mpc_handle_t h, int batch, const fbstab_mpc_batch_t* data,
                                         const fbstab_var_batch_t* x, fbstab_solver_out_t* out,
                                         const fbstab_receding_plant_t* plant, int steps, int retire,
                                         double* u_log, unsigned long long* stats, float* kernel_ms, void* stream,
                                         const fbstab_sweep_log_t* log) {
  return mpc_receding_sweep_impl(h, batch, data, x, out, plant, steps, retire, u_log, stats, kernel_ms, stream, log);
}

int fbstab_hip_mpc_receding_sweep_scenario(fbstab_mpc_handle_t h, int batch, const fbstab_mpc_batch_t* data,
                                           const fbstab_var_batch_t* x, fbstab_solver_out_t* out,
                                           const fbstab_receding_plant_t* plant, int steps, int retire,
                                           double* u_log, unsigned long long* stats, float* kernel_ms, void* stream,
                                           const fbstab_sweep_log_t* log, const fbstab_sweep_scenario_t* scenario) {
  return mpc_receding_sweep_impl(h, batch, data, x, out, plant, steps, retire, u_log, stats, kernel_ms, stream, log,
                                 scenario);
}

// Diagnostics for the tests: one Newton step of the device path at (x, xbar,
// sigma0) for ONE QP given by host pointers.  io holds [zb, lb, vb] on input
// and [dz, dl, dv, adz, wz, wl, rz, rl, ok] on output
// (2*nz + 2*nl + 2*nv + nz + nl + 1 doubles).
int fbstab_hip_mpc_debug_newton(fbstab_mpc_handle_t h, const fbstab_mpc_batch_t* data,
                                const fbstab_var_batch_t* x, double* io) {
  if (!h || !data || !x || !io) return fail(FBSTAB_HIP_ERR_ARGUMENT, "null argument");
  auto launch = [h](const fbstab_mpc_batch_t& a, const fbstab_var_batch_t& v, double* d_io) -> int {
    HIP_TRY(hipMemsetAsync(h->counter, 0, kQueueBytes, h->stream));
    h->kept_batch = -1;  // the probe runs in slot 0 and overwrites its matrix copies
    return launch_mpc(h, h->kern.probe, 1, h->stream, a, v, h->d_out, 1, d_io, false);
  };
  return probe_run(h, data, x, io, launch);
}

// Reverse-mode derivative of the solution map at returned points (include/fbstab_hip.h).  One launch of
// fbstab_mpc_adjoint_kernel: the Newton matrix of RiccatiLinearSolver::Initialize at x = xbar = the point
// (riccati_linear_solver.cc:77-210), one Solve (:212-344) with the adjoint's right-hand side, one contraction.
// `reduced`: fbstab_hip_mpc_adjoint_batch_reduced - gradient slots of stride 0 are summed over the batch by the
// kernels of fb_grad_reduce.h behind the adjoint's launch (`out`: the solve's records, or null).
// mpc_adjoint_launch is the launch alone, on the staged arguments of `st` (fbstab_hip_mpc_tangent_batch runs it
// behind its direction kernel).
// grad_reduce_launch: the two launches of fb_grad_reduce.h behind a reduced adjoint's launch of either kind, on what
// AdjointStage::reduce filled - the partial sums, then the sums into the reduced slots.
static int grad_reduce_launch(const GradReduceArgs& ra, const GradReduceOut& ro, hipStream_t s) {
  const int tiles = grad_reduce_tiles(ra.plan), chunks = (int)grad_reduce_chunks(ra.batch);
  hipLaunchKernelGGL(fbstab_grad_reduce_kernel, dim3(tiles * chunks), dim3(64), 0, s, ra);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(fbstab_grad_reduce_finish_kernel, dim3(tiles), dim3(256), 0, s, ra.plan,
                     static_cast<const double*>(ra.scratch), chunks, ro);
  HIP_TRY(hipGetLastError());
  return FBSTAB_HIP_OK;
}

static int mpc_adjoint_launch(fbstab_mpc_handle_t h, int batch, AdjointLaunchArgs& st, double sigma) {
  hipStream_t s = st.s;
  const fbk::MpcLayout& L = h->lay;
  fbstab_var_batch_t &v = st.v, &sd = st.sd, &ad = st.ad;
  int* d_st = st.d_st;
  double sig = sigma_or_default(sigma);
  double alpha = h->opts.alpha;
  HIP_TRY(hipMemsetAsync(h->counter, 0, kQueueBytes, s));
  MpcKernel& e = h->kern.adjoint;
  // record instances: the adjoint on the record, in the handle's own slots (their matrix copies are
  // overwritten: the next FBSTAB_HIP_KEEP_MATRICES solve rebuilds them)
  if (e.record) h->kept_batch = -1;
  MpcBatchPtrs d = record_data(h, st.a);
  AdjointArgs aa;
  aa.grad = st.g;
  for (int i = 0; i < 3; i++) {  // (three slots wide: no y)
    aa.seed[i] = sd.base[i]; aa.sstride[i] = sd.stride[i];
    aa.adj[i] = ad.base[i]; aa.astride[i] = ad.stride[i];
  }
  aa.status = d_st;
  aa.sigma = sig;
  aa.alpha = alpha;
  int N = L.N;
  void* record_args[] = {&d, &v, &aa, &h->scratch, &h->counter, &batch, &N};
  // the flat-vector kernel, one QP per workgroup
  double* scratch;
  RC_TRY(flat_workspace(h, e, &scratch));
  void* flat_args[] = {const_cast<fbk::MpcLayout*>(&L), &st.a, &v, &sd, &st.g, &ad, &d_st, &sig, &alpha, &scratch,
                       &h->counter, &batch};
  RC_TRY(h->begin_timed(s));
  RC_TRY(launch_entry(e, h->batch_grid(e, batch), e.record ? record_args : flat_args, s));
  return h->end_timed(s);
}

static int mpc_adjoint_impl(fbstab_mpc_handle_t h, int batch, const fbstab_mpc_batch_t* data,
                            const fbstab_var_batch_t* x, const fbstab_var_batch_t* seed, double sigma,
                            const fbstab_mpc_grad_batch_t* grad, const fbstab_var_batch_t* adj, int* status,
                            const fbstab_solver_out_t* out, int flags, void* stream, bool reduced) {
  int rc = check_common(h, batch, data, x, status, h ? h->max_batch : 0);
  if (rc != FBSTAB_HIP_OK) return rc;
  if (!seed || !grad) return fail(FBSTAB_HIP_ERR_ARGUMENT, "null argument");
  const fbk::MpcLayout& L = h->lay;
  return adjoint_run(h, batch, data, x, seed, sigma, grad, adj, status, out, flags, stream, reduced,
                     grad_reduce_plan_mpc(L.N, L.nx, L.nu, L.nc), mpc_adjoint_launch, grad_reduce_launch);
}

int fbstab_hip_mpc_adjoint_batch(fbstab_mpc_handle_t h, int batch, const fbstab_mpc_batch_t* data,
                                 const fbstab_var_batch_t* x, const fbstab_var_batch_t* seed, double sigma,
                                 const fbstab_mpc_grad_batch_t* grad, const fbstab_var_batch_t* adj, int* status,
                                 int flags, void* stream) {
  return mpc_adjoint_impl(h, batch, data, x, seed, sigma, grad, adj, status, nullptr, flags, stream, false);
}

int fbstab_hip_mpc_adjoint_batch_reduced(fbstab_mpc_handle_t h, int batch, const fbstab_mpc_batch_t* data,
                                         const fbstab_var_batch_t* x, const fbstab_var_batch_t* seed, double sigma,
                                         const fbstab_mpc_grad_batch_t* grad, const fbstab_var_batch_t* adj,
                                         int* status, const fbstab_solver_out_t* out, int flags, void* stream) {
  return mpc_adjoint_impl(h, batch, data, x, seed, sigma, grad, adj, status, out, flags, stream, true);
}

// Reverse mode through a logged receding-horizon sweep (include/fbstab_hip.h has the recursion).  Handles on a
// record adjoint: one launch of fbstab_mpc_r16_sweep_adjoint_kernel; every other handle, and
// FBSTAB_HIP_SWEEP_ADJOINT_PER_STEP=1: per step the costate kernel, the handle's adjoint launch, the costate kernel.
int fbstab_hip_mpc_receding_sweep_adjoint(fbstab_mpc_handle_t h, int batch, const fbstab_mpc_batch_t* data,
                                          const fbstab_receding_plant_t* plant, int steps, int retire,
                                          const fbstab_sweep_log_t* log, const double* gu, const double* gx,
                                          double sigma, const fbstab_mpc_grad_batch_t* grad, double* mu_log,
                                          int* status, void* stream) {
  (void)retire;  // (what it did to the sweep is in the log: eflag -1)
  // (the callables run behind sweep_adjoint_run's checks: h, plant, log and grad are there)
  auto one_launch = [=](hipStream_t s, const fbstab_mpc_batch_t& a, double* seed) -> int {
    h->kept_batch = -1;  // the slots' matrix copies are overwritten
    MpcKernel& e = h->kern.sweep_adjoint;
    HIP_TRY(hipMemsetAsync(h->counter, 0, kQueueBytes, s));
    MpcBatchPtrs d = record_data(h, a);
    SweepAdjointArgs aa;
    aa.grad = *grad;
    aa.A = plant->A; aa.B = plant->B; aa.sA = plant->stride_A; aa.sB = plant->stride_B;
    aa.lz = log->z; aa.ll = log->l; aa.lv = log->v; aa.le = log->eflag;
    aa.gu = gu; aa.gx = gx;
    aa.mu_log = mu_log; aa.status = status; aa.seed = seed;
    aa.steps = steps; aa.sigma = sigma_or_default(sigma); aa.alpha = h->opts.alpha;
    // (as the adjoint: a batch that does not outnumber the workgroups runs one trajectory per wavefront)
    int N = h->lay.N, b = batch;
    void* args[] = {&d, &aa, &h->scratch, &h->counter, &b, &N};
    return launch_timed(h, e, h->batch_grid(e, batch), args, s);
  };
  auto costate = [=](hipStream_t s, const SweepCostateStep& c, int phase, int last) {
    if (phase == 0) h->kept_batch = -1;  // (as above, whichever kernel the adjoint launches run on)
    SweepCostateArgs ca;
    ca.A = plant->A; ca.B = plant->B; ca.sA = plant->stride_A; ca.sB = plant->stride_B;
    ca.eflag = c.eflag; ca.gu = c.gu; ca.gx = c.gx; ca.mu_log = c.mu_log;
    ca.grad = *grad;
    for (int i = 0; i < FBSTAB_MPC_NSEQ; i++) { ca.tmp[i] = c.tmp[i]; ca.len[i] = c.len[i]; }
    ca.seed = c.seed; ca.lam = c.lam; ca.atm = c.atm;
    ca.tmp_status = c.tmp_status;
    ca.status = status;
    ca.nx = h->lay.nx; ca.nu = h->lay.nu; ca.nz = h->lay.nz;
    hipLaunchKernelGGL(fbstab_sweep_costate_kernel, dim3(batch), dim3(64), 0, s, ca, phase, last);
  };
  auto adjoint = [=](AdjointLaunchArgs& st, double sig) { return mpc_adjoint_launch(h, batch, st, sig); };
  SweepScratch none;
  return sweep_adjoint_run(h, sweep_shape(h), h ? h->sweep : none, batch, data, plant, steps, log, gu, gx, sigma, grad,
                           mu_log, status, stream, one_launch, costate, adjoint);
}

// Name of what the next fbstab_hip_mpc_receding_sweep_adjoint of this handle launches (diagnostics, tests, tools).
const char* fbstab_hip_mpc_sweep_adjoint_kernel_name(fbstab_mpc_handle_t h) {
  if (!h) return "";
  return sweep_adjoint_in_one_launch(sweep_shape(h)) ? h->kern.sweep_adjoint.name : "fbstab_sweep_costate_kernel";
}

// Forward-mode derivative of the solution map (include/fbstab_hip.h): fbstab_tangent_rhs_kernel forms the seeds
// (gz, gl, gv) from the perturbations and the points, and the adjoint's launch, unchanged, solves
// V (dz, dl, dv) = (gz, -gl, -C gv) for them on the same stream - no gradient slot, adj = dx.
int fbstab_hip_mpc_tangent_batch(fbstab_mpc_handle_t h, int batch, const fbstab_mpc_batch_t* data,
                                 const fbstab_var_batch_t* x, const fbstab_mpc_batch_t* ddata, double sigma,
                                 const fbstab_var_batch_t* dx, const fbstab_var_batch_t* rhs, int* status, int flags,
                                 void* stream) {
  int rc = check_common(h, batch, data, x, status, h ? h->max_batch : 0);
  if (rc != FBSTAB_HIP_OK) return rc;
  if (!ddata || !dx) return fail(FBSTAB_HIP_ERR_ARGUMENT, "null argument");
  rc = TangentStage::check(h, batch, ddata->base, ddata->stride, dx, rhs);
  if (rc != FBSTAB_HIP_OK) return rc;
  const fbk::MpcLayout& L = h->lay;
  MpcTangentLds o;
  o.init(L.nx, L.nu, L.nc);
  const int lds = o.total * (int)sizeof(double);
  if (lds > kLdsLimitBytes)
    return fail(FBSTAB_HIP_ERR_UNSUPPORTED, "the perturbation images of one stage do not fit the LDS");
  if ((long long)batch * (L.N + 1) > 0x7fffffffLL)
    return fail(FBSTAB_HIP_ERR_ARGUMENT, "batch x stages exceeds the grid limit");
  auto launch_dir = [&](const fbstab_mpc_batch_t& dir, const AdjointLaunchArgs& st) {
    hipLaunchKernelGGL(fbstab_tangent_rhs_kernel, dim3(batch * (L.N + 1)), dim3(64), (size_t)lds, st.s, L.N, L.nx, L.nu,
                       L.nc, o, dir, st.v, st.sd);
  };
  return tangent_run(h, batch, data, x, ddata, sigma, dx, rhs, status, flags, stream,
                     reinterpret_cast<const void*>(fbstab_tangent_rhs_kernel), launch_dir, mpc_adjoint_launch);
}

// ---- many right-hand sides on one factorisation (include/fbstab_hip.h; fb_kkt_multi.h) --------------------------
namespace {
// Both entry points behind what needs no handle, on multi_run (fb_host_stage.h).  seed == nullptr: the x0 mode (nrhs =
// nx, the seeds generated in the kernel); step may be null there, and gain (null, or nu x nx per QP) is served there
// only.
int kkt_multi_run(fbstab_mpc_handle_t h, int batch, const fbstab_mpc_batch_t* data, const fbstab_var_batch_t* x,
                  int nrhs, const fbstab_multi_var_batch_t* seed, double sigma, const fbstab_multi_var_batch_t* step,
                  double* gain, long long gain_stride, int* status, int flags, void* stream) {
  int x0m = seed ? 0 : 1;
  auto sizes = [&](int* n, long long* gain_len) {
    if (x0m) *n = h->lay.nx;
    *gain_len = (long long)h->lay.nu * h->lay.nx;
    return (int)FBSTAB_HIP_OK;
  };
  auto launch = [&](MultiLaunchArgs<fbstab_mpc_batch_t>& k) -> int {
    double sig = sigma_or_default(sigma);
    double alpha = h->opts.alpha;
    HIP_TRY(hipMemsetAsync(h->counter, 0, kQueueBytes, k.s));
    MpcKernel& e = h->kern.kkt_multi;
    // (the flat adjoint's scratch on a record handle, allocated here by the first call that needs it; the handle's
    // own scratch and kept_batch stay as they are)
    double* scratch;
    RC_TRY(flat_workspace(h, e, &scratch));
    void* args[] = {&h->lay, &k.a, &k.v, &k.sd, &k.st, &k.gain, &k.gain_stride, &k.d_st, &k.nrhs, &x0m, &sig, &alpha,
                    &scratch, &h->counter, &batch};
    return launch_timed(h, e, h->batch_grid(e, batch), args, k.s);
  };
  return multi_run(h, batch, data, x, nrhs, seed, step, gain, gain_stride, status, flags, stream, sizes, launch);
}
}  // namespace

int fbstab_hip_mpc_kkt_solve_batch(fbstab_mpc_handle_t h, int batch, const fbstab_mpc_batch_t* data,
                                   const fbstab_var_batch_t* x, int nrhs, const fbstab_multi_var_batch_t* seed,
                                   double sigma, const fbstab_multi_var_batch_t* step, int* status, int flags,
                                   void* stream) {
  // what needs no handle comes first
  if (nrhs < 1) return fail(FBSTAB_HIP_ERR_ARGUMENT, "kkt solve: fewer than one right-hand side");
  if (!seed || !step) return fail(FBSTAB_HIP_ERR_ARGUMENT, "kkt solve: null seed or step block");
  if (!seed->base[0]) return fail(FBSTAB_HIP_ERR_ARGUMENT, "null seed pointer (z)");
  int rc = check_multi_strides(seed, nullptr, batch, nrhs, true);
  if (rc != FBSTAB_HIP_OK) return rc;
  rc = check_multi_strides(step, nullptr, batch, nrhs, false);
  if (rc != FBSTAB_HIP_OK) return rc;
  return kkt_multi_run(h, batch, data, x, nrhs, seed, sigma, step, nullptr, 0, status, flags, stream);
}

int fbstab_hip_mpc_x0_sensitivity_batch(fbstab_mpc_handle_t h, int batch, const fbstab_mpc_batch_t* data,
                                        const fbstab_var_batch_t* x, double sigma,
                                        const fbstab_multi_var_batch_t* step, double* gain, long long gain_stride,
                                        int* status, int flags, void* stream) {
  // (nrhs = nx takes the handle: every stride is checked behind it)
  return kkt_multi_run(h, batch, data, x, 0, nullptr, sigma, step, gain, gain_stride, status, flags, stream);
}

// ---- the condensed route (include/fbstab_hip.h): the runs of fb_condense_stage.h on the real launches -----------
int fbstab_hip_mpc_condensed_sizes(int N, int nx, int nu, int nc, int* nz, int* nv, long long* lds_bytes) {
  return condensed_sizes(N, nx, nu, nc, nz, nv, lds_bytes);
}

int fbstab_hip_mpc_condense_batch(int N, int nx, int nu, int nc, int batch, const fbstab_mpc_batch_t* data, int what,
                                  const fbstab_dense_out_batch_t* dense, int device, void* stream) {
  return condense_run(N, nx, nu, nc, batch, data, what, dense, device, stream, condense_gpu);
}

int fbstab_hip_mpc_expand_batch(int N, int nx, int nu, int nc, int batch, const fbstab_mpc_batch_t* data,
                                const fbstab_var_batch_t* xc, const fbstab_var_batch_t* x, int device, void* stream) {
  return expand_run(N, nx, nu, nc, batch, data, xc, x, device, stream, condense_gpu);
}

int fbstab_hip_mpc_condensed_adjoint_batch(fbstab_dense_handle_t h, int N, int nx, int nu, int nc, int batch,
                                           const fbstab_mpc_batch_t* data, const fbstab_dense_batch_t* dense,
                                           const fbstab_var_batch_t* x, const fbstab_var_batch_t* seed, double sigma,
                                           const fbstab_mpc_grad_batch_t* grad, const fbstab_var_batch_t* adj,
                                           double* work, int* status, void* stream) {
  return condensed_adjoint_run(h, N, nx, nu, nc, batch, data, dense, x, seed, sigma, grad, adj, work, status, stream,
                               condense_gpu, condense_dense_adjoint(h));
}

int fbstab_hip_mpc_condensed_tangent_batch(fbstab_dense_handle_t h, int N, int nx, int nu, int nc, int batch,
                                           const fbstab_mpc_batch_t* data, const fbstab_dense_batch_t* dense,
                                           const fbstab_var_batch_t* x, const fbstab_mpc_batch_t* ddata, double sigma,
                                           const fbstab_var_batch_t* dx, const fbstab_var_batch_t* rhs, double* work,
                                           int* status, void* stream) {
  return condensed_tangent_run(h, N, nx, nu, nc, batch, data, dense, x, ddata, sigma, dx, rhs, work, status, stream,
                               condense_gpu, condense_dense_adjoint(h), condense_tangent_direction);
}

int fbstab_hip_mpc_condensed_multi_sizes(int N, int nx, int nu, int nc, int nrhs, int rhs_per_group,
                                         int* rhs_per_group_used, long long* lds_bytes,
                                         long long* work_doubles_per_qp) {
  return condensed_multi_sizes(N, nx, nu, nc, nrhs, rhs_per_group, rhs_per_group_used, lds_bytes, work_doubles_per_qp);
}

int fbstab_hip_mpc_condensed_kkt_solve_batch(fbstab_dense_handle_t h, int N, int nx, int nu, int nc, int batch,
                                             const fbstab_mpc_batch_t* data, const fbstab_dense_batch_t* dense,
                                             const fbstab_var_batch_t* x, int nrhs,
                                             const fbstab_multi_var_batch_t* seed, double sigma,
                                             const fbstab_multi_var_batch_t* step, int rhs_per_group, double* work,
                                             int* status, void* stream) {
  return condensed_multi_run(h, N, nx, nu, nc, batch, data, dense, x, false, nrhs, seed, sigma, step, nullptr, 0,
                             rhs_per_group, work, status, stream, condense_gpu, condense_dense_multi(h));
}

int fbstab_hip_mpc_condensed_x0_sensitivity_batch(fbstab_dense_handle_t h, int N, int nx, int nu, int nc, int batch,
                                                  const fbstab_mpc_batch_t* data, const fbstab_dense_batch_t* dense,
                                                  const fbstab_var_batch_t* x, double sigma,
                                                  const fbstab_multi_var_batch_t* step, double* gain,
                                                  long long gain_stride, int rhs_per_group, double* work, int* status,
                                                  void* stream) {
  return condensed_multi_run(h, N, nx, nu, nc, batch, data, dense, x, true, nx, nullptr, sigma, step, gain, gain_stride,
                             rhs_per_group, work, status, stream, condense_gpu, condense_dense_multi(h));
}

int fbstab_hip_mpc_condensed_sweep_sizes(int N, int nx, int nu, int nc, int traj_per_group, int shared_map,
                                         int* traj_per_group_used, long long* lds_bytes,
                                         long long* work_doubles_per_traj) {
  return condensed_sweep_sizes("condensed sweep", N, nx, nu, nc, traj_per_group, shared_map, traj_per_group_used,
                               lds_bytes, work_doubles_per_traj, nullptr, false);
}

int fbstab_hip_mpc_condensed_x0_map_batch(int N, int nx, int nu, int nc, int batch, const fbstab_mpc_batch_t* data,
                                          double* map, long long map_stride, int device, void* stream) {
  return condensed_x0_map_run(N, nx, nu, nc, batch, data, map, map_stride, device, stream, condense_gpu);
}

int fbstab_hip_mpc_condensed_receding_sweep(fbstab_dense_handle_t h, int N, int nx, int nu, int nc, int batch,
                                            const fbstab_mpc_batch_t* data, const fbstab_dense_batch_t* dense,
                                            const fbstab_condensed_map_t* map, const fbstab_var_batch_t* x,
                                            fbstab_solver_out_t* out, const fbstab_receding_plant_t* plant, int steps,
                                            int retire, const fbstab_sweep_scenario_t* scenario, int mode,
                                            const fbstab_condensed_sweep_log_t* log, int traj_per_group, double* work,
                                            void* stream) {
  const auto dense_solve = [h](int b, const fbstab_dense_batch_t* dc, const fbstab_var_batch_t* xc,
                               fbstab_solver_out_t* o, hipStream_t s) {
    return fbstab_hip_dense_solve_batch(h, b, dc, xc, o, kCondenseDenseFlags, (void*)s);
  };
  return condensed_sweep_run(h, N, nx, nu, nc, batch, data, dense, map, x, out, plant, steps, retire, scenario, mode, log,
                             traj_per_group, work, stream, condense_gpu, dense_solve);
}

int fbstab_hip_mpc_condensed_reference_sizes(int N, int nx, int nu, int nc, int steps, int refs_per_group,
                                             int* refs_per_group_used, long long* lds_bytes) {
  return condensed_reference_sizes(N, nx, nu, nc, steps, refs_per_group, refs_per_group_used, lds_bytes);
}

int fbstab_hip_mpc_condensed_reference_images_batch(int N, int nx, int nu, int nc, int batch, int steps,
                                                    const fbstab_mpc_batch_t* data,
                                                    const fbstab_condensed_refs_t* refs,
                                                    const fbstab_condensed_ref_images_t* images, int refs_per_group,
                                                    int device, void* stream) {
  return condensed_reference_images_run(N, nx, nu, nc, batch, steps, data, refs, images, refs_per_group, device, stream,
                                        condense_gpu);
}

int fbstab_hip_mpc_condensed_tracking_sweep(fbstab_dense_handle_t h, int N, int nx, int nu, int nc, int batch,
                                            const fbstab_mpc_batch_t* data, const fbstab_dense_batch_t* dense,
                                            const fbstab_condensed_map_t* map, const fbstab_var_batch_t* x,
                                            fbstab_solver_out_t* out, const fbstab_receding_plant_t* plant, int steps,
                                            int retire, const fbstab_sweep_scenario_t* scenario, int mode,
                                            const fbstab_condensed_sweep_log_t* log,
                                            const fbstab_condensed_refs_t* refs,
                                            const fbstab_condensed_ref_images_t* images, int traj_per_group,
                                            double* work, void* stream) {
  const auto dense_solve = [h](int b, const fbstab_dense_batch_t* dc, const fbstab_var_batch_t* xc,
                               fbstab_solver_out_t* o, hipStream_t s) {
    return fbstab_hip_dense_solve_batch(h, b, dc, xc, o, kCondenseDenseFlags, (void*)s);
  };
  return condensed_tracking_sweep_run(h, N, nx, nu, nc, batch, data, dense, map, x, out, plant, steps, retire, scenario,
                                      mode, log, refs, images, traj_per_group, work, stream, condense_gpu, dense_solve);
}

int fbstab_hip_mpc_condensed_sweep_adjoint_sizes(int N, int nx, int nu, int nc, int traj_per_group, int shared_map,
                                                 int* traj_per_group_used, long long* lds_bytes,
                                                 long long* work_doubles_per_traj,
                                                 long long* work_doubles_per_traj_grad) {
  return condensed_sweep_sizes("condensed sweep adjoint", N, nx, nu, nc, traj_per_group, shared_map,
                               traj_per_group_used, lds_bytes, work_doubles_per_traj, work_doubles_per_traj_grad, true);
}

int fbstab_hip_mpc_condensed_receding_sweep_adjoint(
    fbstab_dense_handle_t h, int N, int nx, int nu, int nc, int batch, const fbstab_mpc_batch_t* data,
    const fbstab_dense_batch_t* dense, const fbstab_condensed_map_t* map, const fbstab_receding_plant_t* plant,
    int steps, int retire, const fbstab_condensed_sweep_log_t* log, const double* gu, const double* gx, double sigma,
    const fbstab_mpc_grad_batch_t* grad, double* gf0, double* gb0, double* mu_log, int* status, int mode,
    int traj_per_group, double* work, void* stream) {
  (void)retire;  // (the logged eflag of -1 carries it)
  return condensed_sweep_adjoint_run(h, N, nx, nu, nc, batch, data, dense, map, plant, steps, log, gu, gx, sigma, grad,
                                     gf0, gb0, mu_log, status, mode, traj_per_group, work, stream, condense_gpu,
                                     condense_dense_adjoint(h));
}

int fbstab_hip_mpc_condensed_tracking_sweep_adjoint(
    fbstab_dense_handle_t h, int N, int nx, int nu, int nc, int batch, const fbstab_mpc_batch_t* data,
    const fbstab_dense_batch_t* dense, const fbstab_condensed_map_t* map, const fbstab_receding_plant_t* plant,
    int steps, int retire, const fbstab_condensed_sweep_log_t* log, const double* gu, const double* gx, double sigma,
    const fbstab_mpc_grad_batch_t* grad, double* mu_log, int* status, int mode, const fbstab_condensed_refs_t* refs,
    const fbstab_condensed_ref_images_t* images, const fbstab_condensed_ref_grad_t* ref_grad, int traj_per_group,
    double* work, void* stream) {
  (void)retire;  // (the logged eflag of -1 carries it)
  return condensed_tracking_sweep_adjoint_run(h, N, nx, nu, nc, batch, data, dense, map, plant, steps, log, gu, gx,
                                              sigma, grad, nullptr, nullptr, mu_log, status, mode, refs, images,
                                              ref_grad, traj_per_group, work, stream, condense_gpu,
                                              condense_dense_adjoint(h));
}

int fbstab_hip_mpc_condensed_sweep_tangent_sizes(int N, int nx, int nu, int nc, int traj_per_group, int shared_map,
                                                 int* traj_per_group_used, long long* lds_bytes,
                                                 long long* work_doubles_per_traj) {
  return condensed_sweep_tangent_sizes(N, nx, nu, nc, traj_per_group, shared_map, traj_per_group_used, lds_bytes,
                                       work_doubles_per_traj);
}

int fbstab_hip_mpc_condensed_receding_sweep_tangent(
    fbstab_dense_handle_t h, int N, int nx, int nu, int nc, int batch, const fbstab_dense_batch_t* dense,
    const fbstab_condensed_map_t* map, const fbstab_condensed_ref_images_t* images,
    const fbstab_receding_plant_t* plant, int steps, const fbstab_condensed_sweep_log_t* log,
    const fbstab_condensed_sweep_dir_t* dir, double sigma, double* du, double* dx, int* status, int traj_per_group,
    double* work, void* stream) {
  return condensed_sweep_tangent_run(h, N, nx, nu, nc, batch, dense, map, images, plant, steps, log, dir, sigma, du, dx,
                                     status, traj_per_group, work, stream, condense_gpu, condense_dense_adjoint(h));
}

// Diagnostic builds (-DFB_STAMP): per-phase shader cycles summed over waves;
// zeros otherwise.  reset != 0 clears the counters after reading.
int fbstab_hip_debug_stamps(unsigned long long* out32, int reset) {
  if (!out32) return fail(FBSTAB_HIP_ERR_ARGUMENT, "null argument");
  memset(out32, 0, 32 * sizeof(unsigned long long));
#if defined(FB_ANY_STAMP)
  HIP_TRY(hipMemcpyFromSymbol(out32, HIP_SYMBOL(fbk::g_stamps), 32 * sizeof(unsigned long long)));
  if (reset) {
    unsigned long long z[32] = {0};
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(fbk::g_stamps), z, sizeof(z)));
  }
#else
  (void)reset;
#endif
  return FBSTAB_HIP_OK;
}

double fbstab_hip_mpc_last_kernel_ms(fbstab_mpc_handle_t h) { return h ? h->last_kernel_ms() : -1.0; }

int fbstab_hip_mpc_query(fbstab_mpc_handle_t h, long long* scratch_bytes, int* lds_bytes,
                         int* workgroups, int* threads) {
  if (!h) return fail(FBSTAB_HIP_ERR_ARGUMENT, "null solver handle");
  if (scratch_bytes) *scratch_bytes = h->scratch_bytes;
  if (lds_bytes) *lds_bytes = h->lds_bytes;
  if (workgroups) *workgroups = h->workgroups;
  if (threads) *threads = h->threads;
  return FBSTAB_HIP_OK;
}

// Name of the kernel batches of this handle run on (diagnostics, tests).
const char* fbstab_hip_mpc_kernel_name(fbstab_mpc_handle_t h) {
  if (!h) return "";
  return h->kern.solve.name;
}

// Name of the kernel the next fbstab_hip_mpc_adjoint_batch of this handle launches (diagnostics, tests, tools).
const char* fbstab_hip_mpc_adjoint_kernel_name(fbstab_mpc_handle_t h) {
  if (!h) return "";
  return h->kern.adjoint.name;
}

int fbstab_hip_mpc_refined_steps(fbstab_mpc_handle_t h, long long* steps) {
  if (!h) return fail(FBSTAB_HIP_ERR_ARGUMENT, "null solver handle");
  if (!steps) return fail(FBSTAB_HIP_ERR_ARGUMENT, "null output pointer");
  *steps = -1;
  if (!h->timed) return FBSTAB_HIP_OK;
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipEventSynchronize(h->ev1));
  int n = 0;  // word 1 of the queue block (zeroed before every launch): R16Queue::count_refinement, fb_mpc.h
  HIP_TRY(hipMemcpy(&n, h->counter + 1, sizeof(n), hipMemcpyDeviceToHost));
  *steps = n;
  return FBSTAB_HIP_OK;
}

int fbstab_hip_mpc_queue_order(fbstab_mpc_handle_t h, int* order, int capacity, int* n) {
  if (!h) return fail(FBSTAB_HIP_ERR_ARGUMENT, "null solver handle");
  if (!n) return fail(FBSTAB_HIP_ERR_ARGUMENT, "null output pointer");
  *n = 0;
  if (h->order_batch < 0) return FBSTAB_HIP_OK;
  if (!order || capacity < h->order_batch) return fail(FBSTAB_HIP_ERR_ARGUMENT, "order array smaller than the stored order");
  HIP_TRY(hipSetDevice(h->device));
  // (waits for the solve whose counts the order holds and for the kernel behind it: both are inside the timed
  // section of their call, on whatever stream it ran)
  if (h->timed) HIP_TRY(hipEventSynchronize(h->ev1));
  HIP_TRY(hipMemcpy(order, h->order, sizeof(int) * (size_t)h->order_batch, hipMemcpyDeviceToHost));
  *n = h->order_batch;
  return FBSTAB_HIP_OK;
}

// ---------------------------------------------------------------------------
int fbstab_hip_dense_create(int nz, int nl, int nv, int max_batch, int device,
                            fbstab_dense_handle_t* handle) {
  if (!handle) return fail(FBSTAB_HIP_ERR_ARGUMENT, "null handle pointer");
  *handle = nullptr;
  // fbstab_dense.cc:19-23
  if (nz < 1 || nv < 1 || nl < 0)
    return fail(FBSTAB_HIP_ERR_ARGUMENT, "In FBstabDense::FBstabDense: nz and nv must be positive, nl nonnegative.");
  if (max_batch < 1) return fail(FBSTAB_HIP_ERR_ARGUMENT, "max_batch must be positive");
  std::unique_ptr<fbstab_dense_solver> s(new (std::nothrow) fbstab_dense_solver());
  if (!s) return fail(FBSTAB_HIP_ERR_DEVICE, "out of host memory");
  const fbk::CreateKnobs knobs = fbk::create_knobs();
  // nz + nl <= 64: one wavefront per QP for every phase, the KKT matrix in registers,
  // up to eight QPs per CU (fb_dense_wave.h).  Otherwise four wavefronts per QP with
  // K in LDS or, beyond nz + nl ~ 140, in global scratch (fb_dense.h).
  // FBSTAB_HIP_DENSE_THREADS=256 forces the four-wavefront kernel (comparisons);
  // =64 its one-wavefront instance with K in LDS.
  s->threads = kDenseThreads;
  s->wlay.init(nz, nl, nv);
  s->wave = s->wlay.fits();
  const int forced_threads = fbk::dense_threads_choice(knobs, nz, nl);
  if (forced_threads) s->wave = false;
  if (forced_threads == 64) s->threads = 64;
  // (initial values of what fbstab_hip_dense_set_factorisation sets per handle)
  static_assert(fbk::kDenseOrderAuto == FBSTAB_HIP_DENSE_ORDER_AUTO &&
                    fbk::kDenseOrderPivoted == FBSTAB_HIP_DENSE_ORDER_PIVOTED &&
                    fbk::kDenseOrderNatural == FBSTAB_HIP_DENSE_ORDER_NATURAL,
                "fb_launch_plan.h names the public header's orders");
  if (knobs.dense_order >= 0) s->wlay.order = knobs.dense_order;
  if (knobs.dense_spread_bits > 0) s->wlay.spread_bits = knobs.dense_spread_bits;
  if (knobs.dense_sticky >= 0) s->wlay.sticky = knobs.dense_sticky;
  if (knobs.dense_act_bits >= 0) s->wlay.act_bits = knobs.dense_act_bits;
  s->lay.init(nz, nl, nv, s->threads);
  if (s->threads == 64 && (s->lay.k_global || !s->lay.a_lds)) {  // does not fit that way
    s->threads = kDenseThreads;
    s->lay.init(nz, nl, nv, s->threads);
  }
  s->lds_bytes = s->lay.lds_doubles * (int)sizeof(double);
  if (s->wave) {
    s->threads = 64;
    s->lay.init(nz, nl, nv, kDenseThreads);  // (the traced solve's layout)
    s->lds_bytes = s->wlay.lds_doubles * (int)sizeof(double);
  }
  if (s->lds_bytes > kLdsLimitBytes)  // (not reached: the vectors move to global scratch first)
    return fail(FBSTAB_HIP_ERR_UNSUPPORTED, "the iterate vectors do not fit the 160 KiB LDS budget");
  RC_TRY(s->common_init(device, max_batch));
  dense_resolve_kernels(s.get());
  int occupancy = 0, cus = 0;
  RC_TRY(s->occupancy(s->kern.solve, &occupancy, &cus));
  const fbk::LaunchPlan plan = fbk::dense_plan(cus, occupancy, max_batch, s->wave, s->wlay.ws_doubles, s->lay.k_global != 0,
                                               (long long)s->lay.k_doubles + s->lay.v_doubles, knobs);
  s->workgroups = plan.workgroups;
  s->scratch_bytes = plan.scratch_bytes;
  if (s->scratch_bytes > 0) {
    hipError_t e = hipMalloc(&s->scratch, (size_t)s->scratch_bytes);
    // (fb_dense_wave.h relies on the multiplier rows past nz + nl being zero)
    if (e == hipSuccess && s->wave) e = hipMemset(s->scratch, 0, (size_t)s->scratch_bytes);
    if (e != hipSuccess) return fail(FBSTAB_HIP_ERR_DEVICE, std::string("scratch allocation: ") + hipGetErrorString(e));
  }
  s->arr_len = {(long long)nz * nz, (long long)nz, (long long)nl * nz, (long long)nl,
                (long long)nv * nz, (long long)nv};
  s->var_len[0] = nz; s->var_len[1] = nl; s->var_len[2] = nv; s->var_len[3] = nv;
  *handle = s.release();
  return FBSTAB_HIP_OK;
}

int fbstab_hip_dense_destroy(fbstab_dense_handle_t h) {
  delete h;
  return FBSTAB_HIP_OK;
}

int fbstab_hip_dense_set_options(fbstab_dense_handle_t h, const fbstab_options_t* o) {
  if (!h || !o) return fail(FBSTAB_HIP_ERR_ARGUMENT, "null argument");
  h->opts = *o;
  fbstab_options_validate(&h->opts);
  return FBSTAB_HIP_OK;
}
int fbstab_hip_dense_get_options(fbstab_dense_handle_t h, fbstab_options_t* o) {
  if (!h || !o) return fail(FBSTAB_HIP_ERR_ARGUMENT, "null argument");
  *o = h->opts;
  return FBSTAB_HIP_OK;
}

static int dense_solve_impl(fbstab_dense_handle_t h, int batch, const fbstab_dense_batch_t* data,
                            const fbstab_var_batch_t* x, fbstab_solver_out_t* out, int flags,
                            void* stream, double* d_trace, double* norms = nullptr) {
  auto launch = [=](hipStream_t s, const fbstab_dense_batch_t& a, const fbstab_var_batch_t& v,
                    fbstab_solver_out_t* d_out) -> int {
    DenseKernel& e = d_trace ? h->kern.traced : h->kern.solve;
    if (!e.kern) return fail(FBSTAB_HIP_ERR_UNSUPPORTED, "traced dense solve: layout does not fit");
    return launch_dense(h, e, fbk::dense_grid(batch, h->workgroups), s, a, v, d_out, batch, d_trace);
  };
  auto launch_norms = [=](hipStream_t s, const fbstab_dense_batch_t& a, const fbstab_var_batch_t& v, double* dn) {
    const DenseNormArgs na = {a, v, h->lay.nz, h->lay.nl, h->lay.nv};
    hipLaunchKernelGGL(fbstab_dense_final_norms_kernel, dim3(batch), dim3(64), 0, s, na, h->opts, dn, batch);
  };
  return solve_run(h, batch, data, x, out, flags, stream, norms, launch, launch_norms);
}

int fbstab_hip_dense_solve_batch_final(fbstab_dense_handle_t h, int batch, const fbstab_dense_batch_t* data,
                                       const fbstab_var_batch_t* x, fbstab_solver_out_t* out, double* norms,
                                       int flags, void* stream) {
  if (!norms) return fail(FBSTAB_HIP_ERR_ARGUMENT, "null norms pointer");
  return dense_solve_impl(h, batch, data, x, out, flags, stream, nullptr, norms);
}

int fbstab_hip_dense_solve_batch(fbstab_dense_handle_t h, int batch,
                                 const fbstab_dense_batch_t* data, const fbstab_var_batch_t* x,
                                 fbstab_solver_out_t* out, int flags, void* stream) {
  return dense_solve_impl(h, batch, data, x, out, flags, stream, nullptr);
}

int fbstab_hip_dense_solve_traced(fbstab_dense_handle_t h, const fbstab_dense_batch_t* data,
                                  const fbstab_var_batch_t* x, fbstab_solver_out_t* out,
                                  fbstab_trace_record_t* trace, int capacity, int* count) {
  if (!h) return fail(FBSTAB_HIP_ERR_ARGUMENT, "null solver handle");
  TraceBuf tb;
  int rc = tb.open(h->device, trace, capacity, count);
  if (rc != FBSTAB_HIP_OK) return rc;
  rc = dense_solve_impl(h, 1, data, x, out, FBSTAB_HIP_HOST_POINTERS, nullptr, tb.dev());
  if (rc != FBSTAB_HIP_OK) return rc;
  return tb.close(trace, capacity, count);
}

// Diagnostics for the tests: one Newton step of the dense device path
// (DenseCholeskySolver::Initialize + Solve, dense_cholesky_solver.cc:32-127) at
// (x, xbar, sigma0) for ONE QP given by host pointers; io as in
// fbstab_hip_mpc_debug_newton.  K in LDS only (nz + nl up to ~140).
int fbstab_hip_dense_debug_newton(fbstab_dense_handle_t h, const fbstab_dense_batch_t* data,
                                  const fbstab_var_batch_t* x, double* io) {
  if (!h || !data || !x || !io) return fail(FBSTAB_HIP_ERR_ARGUMENT, "null argument");
  if (!h->wave && h->lay.k_global) return fail(FBSTAB_HIP_ERR_UNSUPPORTED, "dense probe: K must fit the LDS");
  auto launch = [h](const fbstab_dense_batch_t& a, const fbstab_var_batch_t& v, double* d_io) -> int {
    DenseKernel& e = h->kern.probe;
    if (e.wave) return launch_dense(h, e, 1, h->stream, a, v, nullptr, 1, d_io);
    void* args[] = {const_cast<fbk::DenseLayout*>(e.lay), const_cast<fbstab_dense_batch_t*>(&a),
                    const_cast<fbstab_var_batch_t*>(&v), &h->opts, &d_io};
    return launch_entry(e, 1, args, h->stream);
  };
  return probe_run(h, data, x, io, launch);
}

// Reverse-mode derivative of the dense solution map at returned points (include/fbstab_hip.h).  One launch of the
// adjoint kernel that matches the handle's solve kernel: the Newton matrix of DenseCholeskySolver::Initialize at
// x = xbar = the point (dense_cholesky_solver.cc:32-79), one Solve (:81-127) with the adjoint's right-hand side,
// one contraction.
// `reduced`: fbstab_hip_dense_adjoint_batch_reduced, as mpc_adjoint_impl.
// dense_adjoint_launch is the launch alone, on the staged arguments of `st` (fbstab_hip_dense_tangent_batch runs it
// behind its direction kernel).
static int dense_adjoint_launch(fbstab_dense_handle_t h, int batch, AdjointLaunchArgs& st, double sigma) {
  hipStream_t s = st.s;
  fbstab_dense_batch_t a = narrowed<fbstab_dense_batch_t>(st.a);
  fbstab_dense_grad_batch_t g = narrowed<fbstab_dense_grad_batch_t>(st.g);
  fbstab_var_batch_t &v = st.v, &sd = st.sd, &ad = st.ad;
  int* d_st = st.d_st;
  double sig = sigma_or_default(sigma);
  double alpha = h->opts.alpha;
  // the queue word alone: the words from kDenseFallbackSlot on still describe the last solve
  // (fbstab_hip_dense_get_factorisation)
  HIP_TRY(hipMemsetAsync(h->counter, 0, sizeof(int) * kDenseFallbackSlot, s));
  DenseKernel& e = h->kern.adjoint;
  KScratchArg<true> ks{h->scratch};
  KScratchArg<false> no_ks;
  void* wave_args[] = {&h->wlay, &a, &v, &sd, &g, &ad, &d_st, &sig, &alpha, &h->counter, &batch, &h->scratch};
  void* args[] = {&h->lay, &a, &v, &sd, &g, &ad, &d_st, &sig, &alpha, &h->counter, &batch,
                  e.kscratch ? (void*)&ks : (void*)&no_ks};
  RC_TRY(h->begin_timed(s));
  RC_TRY(launch_entry(e, fbk::dense_grid(batch, h->workgroups), e.wave ? wave_args : args, s));
  return h->end_timed(s);
}

static int dense_adjoint_impl(fbstab_dense_handle_t h, int batch, const fbstab_dense_batch_t* data,
                              const fbstab_var_batch_t* x, const fbstab_var_batch_t* seed, double sigma,
                              const fbstab_dense_grad_batch_t* grad, const fbstab_var_batch_t* adj, int* status,
                              const fbstab_solver_out_t* out, int flags, void* stream, bool reduced) {
  // what needs no handle comes first: the argument blocks, the one seed that is required, and strides that no
  // handle accepts (nz and nv are positive: z, v, H, f, A, b are never empty)
  if (!data || !x || !seed || !grad || !status) return fail(FBSTAB_HIP_ERR_ARGUMENT, "null argument");
  if (!seed->base[0]) return fail(FBSTAB_HIP_ERR_ARGUMENT, "null seed pointer (z)");
  if (batch > 1) {
    for (int i = 0; i < 3; i += 2) {
      if (x->stride[i] < 1) return fail(FBSTAB_HIP_ERR_ARGUMENT, "variable stride smaller than the vector length");
      if (seed->base[i] && seed->stride[i] < 1)
        return fail(FBSTAB_HIP_ERR_ARGUMENT, "seed stride smaller than the vector length");
      if (adj && adj->base[i] && adj->stride[i] < 1)
        return fail(FBSTAB_HIP_ERR_ARGUMENT, "adjoint stride smaller than the vector length");
    }
    for (int i : {FBSTAB_DENSE_H, FBSTAB_DENSE_f, FBSTAB_DENSE_A, FBSTAB_DENSE_b})
      if (grad->base[i] && grad->stride[i] < 1 && !(reduced && grad->stride[i] == 0))
        return fail(FBSTAB_HIP_ERR_ARGUMENT, "gradient stride smaller than the array length");
  }
  int rc = check_common(h, batch, data, x, status, h ? h->max_batch : 0);
  if (rc != FBSTAB_HIP_OK) return rc;
  return adjoint_run(h, batch, data, x, seed, sigma, grad, adj, status, out, flags, stream, reduced,
                     grad_reduce_plan_dense((int)h->var_len[0], (int)h->var_len[1], (int)h->var_len[2]),
                     dense_adjoint_launch, grad_reduce_launch);
}

int fbstab_hip_dense_adjoint_batch(fbstab_dense_handle_t h, int batch, const fbstab_dense_batch_t* data,
                                   const fbstab_var_batch_t* x, const fbstab_var_batch_t* seed, double sigma,
                                   const fbstab_dense_grad_batch_t* grad, const fbstab_var_batch_t* adj, int* status,
                                   int flags, void* stream) {
  return dense_adjoint_impl(h, batch, data, x, seed, sigma, grad, adj, status, nullptr, flags, stream, false);
}

int fbstab_hip_dense_adjoint_batch_reduced(fbstab_dense_handle_t h, int batch, const fbstab_dense_batch_t* data,
                                           const fbstab_var_batch_t* x, const fbstab_var_batch_t* seed, double sigma,
                                           const fbstab_dense_grad_batch_t* grad, const fbstab_var_batch_t* adj,
                                           int* status, const fbstab_solver_out_t* out, int flags, void* stream) {
  return dense_adjoint_impl(h, batch, data, x, seed, sigma, grad, adj, status, out, flags, stream, true);
}

// Forward-mode derivative of the dense solution map (include/fbstab_hip.h): as fbstab_hip_mpc_tangent_batch, with
// fbstab_dense_tangent_rhs_kernel and the dense adjoint's launch.  What needs no handle is checked first, as there.
int fbstab_hip_dense_tangent_batch(fbstab_dense_handle_t h, int batch, const fbstab_dense_batch_t* data,
                                   const fbstab_var_batch_t* x, const fbstab_dense_batch_t* ddata, double sigma,
                                   const fbstab_var_batch_t* dx, const fbstab_var_batch_t* rhs, int* status,
                                   int flags, void* stream) {
  if (!data || !x || !ddata || !dx || !status) return fail(FBSTAB_HIP_ERR_ARGUMENT, "null argument");
  if (batch > 1) {
    for (int i = 0; i < 3; i += 2) {
      if (x->stride[i] < 1) return fail(FBSTAB_HIP_ERR_ARGUMENT, "variable stride smaller than the vector length");
      if (dx->base[i] && dx->stride[i] < 1)
        return fail(FBSTAB_HIP_ERR_ARGUMENT, "adjoint stride smaller than the vector length");
    }
    for (int i : {FBSTAB_DENSE_H, FBSTAB_DENSE_f, FBSTAB_DENSE_A, FBSTAB_DENSE_b})
      if (ddata->base[i] && ddata->stride[i] < 0)
        return fail(FBSTAB_HIP_ERR_ARGUMENT, "perturbation stride is neither 0 nor at least the array length");
  }
  int rc = check_common(h, batch, data, x, status, h ? h->max_batch : 0);
  if (rc != FBSTAB_HIP_OK) return rc;
  rc = TangentStage::check(h, batch, ddata->base, ddata->stride, dx, rhs);
  if (rc != FBSTAB_HIP_OK) return rc;
  const int nz = (int)h->var_len[0], nl = (int)h->var_len[1], nv = (int)h->var_len[2];
  DenseTangentLds o;
  // (64 KB needs no attribute and leaves room for two workgroups per CU; shapes with more rows take what there is)
  if (!o.init(nz, nl, nv, 64 * 1024 / (int)sizeof(double)) && !o.init(nz, nl, nv, kLdsLimitBytes / (int)sizeof(double)))
    return fail(FBSTAB_HIP_ERR_UNSUPPORTED, "not one column of the perturbation images fits the LDS");
  const int lds = o.total * (int)sizeof(double);
  auto launch_dir = [&](const fbstab_mpc_batch_t& dir, const AdjointLaunchArgs& st) {
    hipLaunchKernelGGL(fbstab_dense_tangent_rhs_kernel, dim3(batch), dim3(kDenseTangentThreads), (size_t)lds, st.s, nz,
                       nl, nv, o, narrowed<fbstab_dense_batch_t>(dir), st.v, st.sd);
  };
  return tangent_run(h, batch, data, x, ddata, sigma, dx, rhs, status, flags, stream,
                     reinterpret_cast<const void*>(fbstab_dense_tangent_rhs_kernel), launch_dir, dense_adjoint_launch);
}

// ---- many right-hand sides on one factorisation of the dense Newton matrix (include/fbstab_hip.h;
// fb_dense_kkt_multi.h) ----------------------------------------------------------------------------------------
namespace {
// Both entry points behind what needs no handle, on multi_run (fb_host_stage.h).  seed == nullptr: the Jacobian mode
// (nrhs = the length of f, h or b, the seeds generated in the kernel).  One launch of the kernel beside the handle's
// adjoint kernel, in the handle's own scratch.
int dense_kkt_multi_run(fbstab_dense_handle_t h, int batch, const fbstab_dense_batch_t* data,
                        const fbstab_var_batch_t* x, int nrhs, const fbstab_multi_var_batch_t* seed, int wrt,
                        double sigma, const fbstab_multi_var_batch_t* step, int* status, int flags, void* stream) {
  if (seed) wrt = fbk::kDenseKktSeeded;
  auto sizes = [&](int* n, long long*) {
    if (seed) return (int)FBSTAB_HIP_OK;
    const long long* vlen = h->var_len;
    if (wrt == FBSTAB_DENSE_h && vlen[1] == 0)
      return fail(FBSTAB_HIP_ERR_ARGUMENT, "dense jacobian: wrt = h on a handle without equality constraints");
    *n = (int)(wrt == FBSTAB_DENSE_f ? vlen[0] : wrt == FBSTAB_DENSE_h ? vlen[1] : vlen[2]);
    return (int)FBSTAB_HIP_OK;
  };
  auto launch = [&](MultiLaunchArgs<fbstab_dense_batch_t>& k) -> int {
    double sig = sigma_or_default(sigma);
    double alpha = h->opts.alpha;
    // the queue word alone, as the dense adjoint: the words from kDenseFallbackSlot on still describe the last solve
    HIP_TRY(hipMemsetAsync(h->counter, 0, sizeof(int) * kDenseFallbackSlot, k.s));
    DenseKernel& e = h->kern.kkt_multi;
    void* args[] = {e.wave ? (void*)&h->wlay : (void*)&h->lay, &k.a, &k.v, &k.sd, &k.st, &k.d_st, &k.nrhs, &wrt, &sig,
                    &alpha, &h->counter, &batch, &h->scratch};
    return launch_timed(h, e, fbk::dense_grid(batch, h->workgroups), args, k.s);
  };
  return multi_run(h, batch, data, x, nrhs, seed, step, nullptr, 0, status, flags, stream, sizes, launch);
}
}  // namespace

int fbstab_hip_dense_kkt_solve_batch(fbstab_dense_handle_t h, int batch, const fbstab_dense_batch_t* data,
                                     const fbstab_var_batch_t* x, int nrhs, const fbstab_multi_var_batch_t* seed,
                                     double sigma, const fbstab_multi_var_batch_t* step, int* status, int flags,
                                     void* stream) {
  // what needs no handle comes first
  if (nrhs < 1) return fail(FBSTAB_HIP_ERR_ARGUMENT, "dense kkt solve: fewer than one right-hand side");
  if (!seed || !step) return fail(FBSTAB_HIP_ERR_ARGUMENT, "dense kkt solve: null seed or step block");
  if (!data || !x || !status) return fail(FBSTAB_HIP_ERR_ARGUMENT, "null argument");
  if (!seed->base[0]) return fail(FBSTAB_HIP_ERR_ARGUMENT, "null seed pointer (z)");
  int rc = check_multi_strides(seed, nullptr, batch, nrhs, true);
  if (rc != FBSTAB_HIP_OK) return rc;
  rc = check_multi_strides(step, nullptr, batch, nrhs, false);
  if (rc != FBSTAB_HIP_OK) return rc;
  return dense_kkt_multi_run(h, batch, data, x, nrhs, seed, 0, sigma, step, status, flags, stream);
}

int fbstab_hip_dense_jacobian_batch(fbstab_dense_handle_t h, int batch, const fbstab_dense_batch_t* data,
                                    const fbstab_var_batch_t* x, int wrt, double sigma,
                                    const fbstab_multi_var_batch_t* step, int* status, int flags, void* stream) {
  // what needs no handle comes first (nrhs takes the handle: the step strides are checked behind it)
  if (wrt != FBSTAB_DENSE_f && wrt != FBSTAB_DENSE_h && wrt != FBSTAB_DENSE_b)
    return fail(FBSTAB_HIP_ERR_ARGUMENT, "dense jacobian: wrt must be FBSTAB_DENSE_f, FBSTAB_DENSE_h or FBSTAB_DENSE_b");
  if (!step) return fail(FBSTAB_HIP_ERR_ARGUMENT, "dense jacobian: null step block");
  if (!data || !x || !status) return fail(FBSTAB_HIP_ERR_ARGUMENT, "null argument");
  // (every Jacobian has at least one column: a stride that fails for one vector of length 1 fails for every handle)
  int rc = check_multi_strides(step, nullptr, batch, 1, false);
  if (rc != FBSTAB_HIP_OK) return rc;
  return dense_kkt_multi_run(h, batch, data, x, 0, nullptr, wrt, sigma, step, status, flags, stream);
}

double fbstab_hip_dense_last_kernel_ms(fbstab_dense_handle_t h) { return h ? h->last_kernel_ms() : -1.0; }

int fbstab_hip_dense_set_factorisation(fbstab_dense_handle_t h, int order, int spread_bits) {
  if (!h) return fail(FBSTAB_HIP_ERR_ARGUMENT, "null solver handle");
  if (order != FBSTAB_HIP_DENSE_ORDER_AUTO && order != FBSTAB_HIP_DENSE_ORDER_PIVOTED &&
      order != FBSTAB_HIP_DENSE_ORDER_NATURAL)
    return fail(FBSTAB_HIP_ERR_ARGUMENT, "fbstab_hip_dense_set_factorisation: unknown elimination order");
  if (spread_bits < 0 || spread_bits > 2046)
    return fail(FBSTAB_HIP_ERR_ARGUMENT, "fbstab_hip_dense_set_factorisation: spread_bits out of range");
  h->wlay.order = order;
  if (spread_bits > 0) h->wlay.spread_bits = spread_bits;
  return FBSTAB_HIP_OK;
}

int fbstab_hip_dense_get_factorisation(fbstab_dense_handle_t h, int* order, int* spread_bits,
                                       long long* pivoted_steps) {
  if (!h) return fail(FBSTAB_HIP_ERR_ARGUMENT, "null solver handle");
  // (handles that run the four-wavefront kernels always pivot)
  if (order) *order = h->wave ? h->wlay.order : FBSTAB_HIP_DENSE_ORDER_PIVOTED;
  if (spread_bits) *spread_bits = h->wlay.spread_bits;
  if (pivoted_steps) {
    *pivoted_steps = -1;
    if (h->wave && h->timed) {
      HIP_TRY(hipSetDevice(h->device));
      HIP_TRY(hipEventSynchronize(h->ev1));
      int n[2] = {0, 0};  // natural-order attempts handed on; steps of QPs that stayed pivoted after one
      HIP_TRY(hipMemcpy(n, h->counter + kDenseFallbackSlot, sizeof(n), hipMemcpyDeviceToHost));
      *pivoted_steps = (long long)n[0] + n[1];
    }
  }
  return FBSTAB_HIP_OK;
}

int fbstab_hip_dense_query(fbstab_dense_handle_t h, long long* scratch_bytes, int* lds_bytes,
                           int* workgroups, int* threads) {
  if (!h) return fail(FBSTAB_HIP_ERR_ARGUMENT, "null solver handle");
  if (scratch_bytes) *scratch_bytes = h->scratch_bytes;
  if (lds_bytes) *lds_bytes = h->lds_bytes;
  if (workgroups) *workgroups = h->workgroups;
  if (threads) *threads = h->threads;
  return FBSTAB_HIP_OK;
}

}  // extern "C"

#include "fb_shard.h"
