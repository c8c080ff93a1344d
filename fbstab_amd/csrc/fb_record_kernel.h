// The record kernels' entry point and queue (fb_mpc_r16.h holds the numerics), shared by
// the translation units of the library: every instance <NX, NU, NC, R> is compiled in a
// file of its own (rec_*.hip, a minute or two each, in parallel under `make -j`) and
// hands fbstab_hip.hip a RecordInstance with the addresses of its kernels (a padded and an exact set: three of
// the solve, the adjoint and the sweep adjoint each).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "../../include/fbstab_hip.h"
#include "fb_adjoint.h"
#include "fb_algorithm.h"
#include "fb_mpc_r16.h"

#if defined(FB_STAMP) || defined(FB_CLOCKSTAMP)
#define FB_ANY_STAMP 1
#endif

// The kernels of one flavour of an instance: batch solve, FBSTAB_HIP_KEEP_MATRICES solve, Newton-step probe,
// fbstab_hip_mpc_adjoint_batch on the record (fbstab_mpc_r16_adjoint_kernel) and
// fbstab_hip_mpc_receding_sweep_adjoint on the record (fbstab_mpc_r16_sweep_adjoint_kernel).
struct RecordKernels {
  const void *solve, *solve_keep, *probe, *adjoint, *sweep_adjoint;
};

// One compiled instance of the record kernel family: its entry points and its footprint.
struct RecordInstance {
  const char* name;
  int nx, nu, nc;        // largest problem it runs (smaller ones zero-padded)
  int qps_per_wg;
  int (*lds_bytes)(int N);
  long long (*ws_doubles)(int N);
  RecordKernels padded;  // kernels of the padded instance
  RecordKernels exact;   // problem == instance shape
  const char* adjoint_name;        // the names the adjoint and the sweep adjoint are reported under
  const char* sweep_adjoint_name;
};

// Arguments of the record adjoint kernel (fbstab_hip_mpc_adjoint_batch): the seeds (gz, gl, gv; gl and gv may be
// null), the gradient slots (FBSTAB_MPC_* order; null: not wanted), the adjoint (dz, dl, dv; null slots skipped),
// the per-QP status, sigma and the options' alpha.
struct AdjointArgs {
  const double* seed[3];
  long long sstride[3];
  fbstab_mpc_grad_batch_t grad;
  double* adj[3];
  long long astride[3];
  int* status;
  double sigma, alpha;
};
// (kernel-argument offsets are part of the instruction stream)
static_assert(offsetof(AdjointArgs, grad) == 48 && offsetof(AdjointArgs, adj) == 240 && sizeof(AdjointArgs) == 312,
              "AdjointArgs: seed[3], sstride[3], the gradient block, adj[3], astride[3], status, sigma, alpha");

// Arguments of the sweep adjoint kernel (fbstab_hip_mpc_receding_sweep_adjoint): the plant, the log of the sweep
// ([steps][batch][n] each), the seeds gu, gx (null: zero), the gradient slots (null: not wanted; the x0 slot
// receives the final costate), mu_log (or null), the per-trajectory count of failed factorisations, and `seed`:
// nz doubles per row slot of the grid, zero outside the u0 entries, where a row stages the seed vector of a step.
struct SweepAdjointArgs {
  const double *A, *B;  // column-major, as SweepArgs
  long long sA, sB;
  const double *lz, *ll, *lv;
  const int* le;
  const double *gu, *gx;
  fbstab_mpc_grad_batch_t grad;
  double* mu_log;
  int* status;
  double* seed;
  int steps;
  double sigma, alpha;
};
static_assert(offsetof(SweepAdjointArgs, grad) == 80 && offsetof(SweepAdjointArgs, mu_log) == 272,
              "SweepAdjointArgs: the gradient block behind gx");

namespace {

using namespace fbk;

// Diagnostic probe (tests only): one Newton step at (x, xbar, sigma) instead of
// a solve.  dbg holds [zb, lb, vb] on input and receives
// [dz, dl, dv, adz, wz, wl, rz, rl, ok].
template <class P, class C>
__device__ __forceinline__ void newton_probe(P& p, const C& ctx, const fbstab_options_t& opts, double* dbg) {
  p.load_guess(ctx);
  if constexpr (P::kOwnVectorOps) {
    p.choose_costate_form(opts.sigma0);
    p.probe_set_xbar(ctx, dbg);
    p.residual(ctx);
    double a, b, lin2;
    const bool ok = p.newton_step(ctx, opts.sigma0, opts.alpha, &a, &b, &lin2);
    // the solver's own rule for refining a step (Solver::wants_refinement: an option, off by default), no
    // inner tolerance in play
    Solver<P, C> rule(p, ctx, opts);
    if (ok && rule.wants_refinement(lin2, opts.abs_tol, opts.abs_tol))
      p.refine_step(ctx, opts.sigma0, opts.alpha, &a, &b, &lin2);
    ctx.sync();
    p.probe_dump(ctx, dbg, ok);
    return;
  } else {
  const int nz = p.nz, nl = p.nl, nv = p.nv;
  for (int i = ctx.tid; i < nz; i += C::nt) p.zb[i] = dbg[i];
  for (int i = ctx.tid; i < nl; i += C::nt) p.lb[i] = dbg[nz + i];
  for (int i = ctx.tid; i < nv; i += C::nt) p.vb[i] = dbg[nz + nl + i];
  ctx.sync();
  p.residual(ctx);
  bool ok;
  if constexpr (P::kFusedTrial) {
    double a, b;
    ok = p.newton_step(ctx, opts.sigma0, opts.alpha, &a, &b);
  } else {
    ok = p.newton_step(ctx, opts.sigma0, opts.alpha);
    if constexpr (can_refine_of<P>::value) {  // the solver's own rule (Solver::wants_refinement)
      Solver<P, C> rule(p, ctx, opts);
      if (ok && opts.reserved > 0 && rule.wants_refinement(p.linear_residual2(ctx, opts.sigma0), opts.abs_tol, opts.abs_tol))
        p.refine_step(ctx, opts.sigma0);
    }
  }
  ctx.sync();
  double* o = dbg;
  for (int i = ctx.tid; i < nz; i += C::nt) o[i] = p.dz[i];
  o += nz;
  for (int i = ctx.tid; i < nl; i += C::nt) o[i] = p.dl[i];
  o += nl;
  for (int i = ctx.tid; i < nv; i += C::nt) o[i] = p.dv[i];
  o += nv;
  for (int i = ctx.tid; i < nv; i += C::nt) o[i] = p.adz[i];
  o += nv;
  for (int i = ctx.tid; i < nz; i += C::nt) o[i] = p.wz[i];
  o += nz;
  for (int i = ctx.tid; i < nl; i += C::nt) o[i] = p.wl[i];
  o += nl;
  for (int i = ctx.tid; i < nz; i += C::nt) o[i] = p.rz[i];
  o += nz;
  for (int i = ctx.tid; i < nl; i += C::nt) o[i] = p.rl[i];
  o += nl;
  if (ctx.tid == 0) o[0] = ok ? 1.0 : 0.0;
  }
}

// Record-based 16-lane kernel (fb_mpc_r16.h): four QPs per wavefront, rows pull
// QP indices from the shared counter.  scratch: rows * ws_doubles(N).
// One queue object per 16-lane row; every function is called by the whole row and
// returns row-uniform values.  Nothing in here waits for another wavefront.
// (The queue block is kQueueBytes long: fb_launch_plan.h.)

// The receding-horizon sweep as ONE launch of a KEEP instance (fbstab_hip_mpc_receding_sweep):
// a row then solves ITS trajectory `steps` times, advancing the plant in between, and
// never waits for another trajectory - a batch launch per step lasts as long as its
// slowest QP, and a trajectory that runs to the iteration limit before it is retired
// holds up the other 4095 for a hundred solves' worth of time.  Lives in device memory;
// the kernel gets the pointer through its (otherwise unused) probe argument.
struct SweepArgs {
  const double* A;  // simulation model x+ = A x + B u0 (ocp_generator.h:31-38), column-major
  const double* B;
  long long sA, sB;     // doubles between trajectories (0: one plant for all)
  double* x0;           // the batch's initial states, advanced in place
  long long sx0;
  double* u_log;        // NULL or [steps][batch][nu]
  unsigned long long* stats;  // [steps][4]
  int steps, retire;
  int nx, nu, nz, nl, nv;
  // fbstab_hip_mpc_receding_sweep_logged: NULL, or [steps][batch][nz | nl | nv | nx] and [steps][batch]
  double *log_z, *log_l, *log_v, *log_x0;
  int* log_eflag;
  // fbstab_hip_mpc_receding_sweep_scenario: NULL, or the disturbances [steps][batch][nx] (x+ = A x + B u0 + w_k),
  // and whether the point a step returned is moved one stage towards the present before it is the next guess
  // (N, nc: the stage blocks of z, l and v are nx + nu, nx and nc long).  What the move needs it finds HERE, not
  // in registers held across the plant step (receding_plant_step: its register footprint): the lanes of a row,
  // the (z, l, v) slots of the caller's x once more, and cnt, [batch] ints zeroed before the launch, the number
  // of steps each trajectory has behind it.
  const double* w;
  int shift, N, nc, lpq;
  int* cnt;
  double* xb[3];
  long long sxb[3];
};

// Blocks 1 .. N of `a` (b doubles each) moved onto blocks 0 .. N-1, in place, by the lanes of a row: lane t takes the
// entries e = t, t + lpq, ... of a block and walks each of them through the stages in ascending order, so that an
// address is overwritten by the lane that read it, after it read it (one loop: no exec mask nests in another).
__device__ __forceinline__ void shift_stage_blocks(double* a, int b, int N, int t, int lpq) {
  int e = t, i = 0;
  while (e < b && N > 0) {
    a[i * b + e] = a[(i + 1) * b + e];
    if (++i == N) {
      i = 0;
      e += lpq;
    }
  }
}

// Closed-loop step of trajectory q after its solve number `step`, by the lanes of its
// row (t = lane within the row, lpq = lanes per row): retirement, statistics, u0 and
// x0 <- A x0 + B u0 - what fbstab_receding_plant_kernel does for a whole batch between
// two launches.  Returns the updated `retired` flag.  A real call: inlined into the
// solver loop its temporaries cost the sweeps 60 spilled registers.
// Scenario sweeps: w_k is added behind the fma chain (not for a parked trajectory, which stays at the origin), and
// with `shift` the returned point becomes the next step's guess moved by one stage, z_i <- z_(i+1), l_i <- l_(i+1),
// v_i <- v_(i+1) for i < N (stage N keeps its values; not behind the last step: x holds what that step returned).
// The copy is in place, stage by stage through a register: entry e of a stage block belongs to lane e mod lpq in
// EVERY stage, so the one lane that reads an address is the one that overwrites it, later in its own program order.
// REGISTER FOOTPRINT: the solve kernels are compiled knowing which registers this function writes (inter-procedural
// register allocation: values they hold across the call sit in the others), so their instructions change when the
// set does.  It is v0-v31, s0-s11, s30-s31 and vcc, and stays that: the columns of A and of B are summed on either
// side of a fence (B's pointers are loaded when A's are dead), the shift keeps nothing in registers across the
// plant step (SweepArgs), and v29, which the allocator now happens to leave out, is named as written.
__device__ __noinline__ bool receding_plant_step(const SweepArgs* sweep, const fbstab_var_batch_t* x,
                                                 const fbstab_solver_out_t* out, int batch, int q, int step, int t,
                                                 int lpq, bool gone) {
  const SweepArgs& a = *sweep;
  // the solve's own stores (solution, SolverOut) are read back by other lanes
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  const int eflag = out[q].eflag, newton = out[q].newton_iters;
  double* z = var_at(*x, 0, q);
  if (a.retire && !gone && eflag != FBSTAB_SUCCESS) {
    gone = true;
    double* l = var_at(*x, 1, q);
    double* v = var_at(*x, 2, q);
    for (int i = t; i < a.nz; i += lpq) z[i] = 0.0;
    for (int i = t; i < a.nl; i += lpq) l[i] = 0.0;
    for (int i = t; i < a.nv; i += lpq) v[i] = 0.0;
  }
  if (t == 0) {
    unsigned long long* st = a.stats + 4 * (long long)step;
    atomicAdd(&st[0], (unsigned long long)newton);
    atomicAdd(&st[1], (unsigned long long)(eflag == FBSTAB_SUCCESS ? 1 : 0));
    atomicAdd(&st[2], (unsigned long long)(gone ? 1 : 0));
    atomicMax(&st[3], (unsigned long long)newton);
  }
  if (a.u_log && t < a.nu) a.u_log[((long long)step * batch + q) * a.nu + t] = gone ? 0.0 : z[a.nx + t];
  double* xs = a.x0 + q * a.sx0;
  {
    // the log of the backward pass: the point this step returned (zeros once retired), the state it was solved
    // for and its eflag
    const long long kq = (long long)step * batch + q;
    if (a.log_z)
      for (int i = t; i < a.nz; i += lpq) a.log_z[kq * a.nz + i] = gone ? 0.0 : z[i];
    if (a.log_l) {
      const double* l = var_at(*x, 1, q);
      for (int i = t; i < a.nl; i += lpq) a.log_l[kq * a.nl + i] = gone ? 0.0 : l[i];
    }
    if (a.log_v) {
      const double* v = var_at(*x, 2, q);
      for (int i = t; i < a.nv; i += lpq) a.log_v[kq * a.nv + i] = gone ? 0.0 : v[i];
    }
    if (a.log_x0 && t < a.nx) a.log_x0[kq * a.nx + t] = xs[t];
    if (a.log_eflag && t == 0) a.log_eflag[kq] = gone ? -1 : eflag;
  }
  double acc = 0.0;  // (nx <= lanes of the row: one entry per lane)
  if (t < a.nx) {
    const double* Aq = a.A + q * a.sA;
    for (int c = 0; c < a.nx; c++) acc = fma(Aq[t + c * a.nx], xs[c], acc);
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  if (t < a.nx) {
    const double* Bq = a.B + q * a.sB;
    for (int j = 0; j < a.nu; j++) acc = fma(Bq[t + j * a.nx], gone ? 0.0 : z[a.nx + j], acc);
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");  // every lane has read x0 (and u0, and logged the point)
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  if (t < a.nx) {
    if (a.w) acc = acc + a.w[((long long)step * batch + q) * a.nx + t];
    xs[t] = gone ? 0.0 : acc;
  }
  const int count = a.cnt[q] + 1;  // (= step + 1)
  if (a.shift != 0 & count < a.steps) {
    shift_stage_blocks(a.xb[0] + q * a.sxb[0], a.nx + a.nu, a.N, t, a.lpq);
    shift_stage_blocks(a.xb[1] + q * a.sxb[1], a.nx, a.N, t, a.lpq);
    shift_stage_blocks(a.xb[2] + q * a.sxb[2], a.nc, a.N, t, a.lpq);
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  if (t == 0) a.cnt[q] = count;  // (every lane has read it)
  asm volatile("" ::: "v29");
  return gone;
}

// ORDERED (the batch solve kernels): ticket t of the queue word is QP order[t] where the launch brings an order -
// the handle's QP indices by descending Newton count of its previous solve of this batch, longest first, so that
// the launch drains on its shortest QPs (fb_queue_order.h; null: index order).
template <class P, bool KEEP, bool ORDERED = false>
struct R16Queue {
  // Only launch-uniform values live in here (SGPRs): the sweeps have no registers
  // to spare (a handful of VGPRs held across the Newton step turned 2 spilled
  // registers into 44).
  const MpcBatchPtrs* data;
  const fbstab_var_batch_t* x;
  int* ctl;  // ctl[0]: next QP index
  double* scratch;
  int batch, N;
  bool reuse;
  bool taken = false;  // (KEEP) this row has had its one QP
  // (KEEP, sweep) solves of this row's trajectory finished so far; bit 30: retired
  int swept = 0;
  const SweepArgs* sweep = nullptr;
  fbstab_solver_out_t* out = nullptr;
  const int* order = nullptr;  // (ORDERED) [batch], a permutation of 0 .. batch-1, or null

  static __device__ __forceinline__ int tid() { return threadIdx.x & (P::LPQ - 1); }
  static __device__ __forceinline__ int row() { return threadIdx.x / P::LPQ; }  // QP slot of the wavefront
  static __device__ __forceinline__ int home() { return blockIdx.x * P::kQpPerWave + row(); }
  static __device__ __forceinline__ lds_ptr lds() {
    extern __shared__ __attribute__((aligned(16))) double smem_[];
    return (lds_ptr)smem_ + P::kPackArea + row() * P::kLdsPerRow;
  }
  // this row's image in the wavefront's matrix-copy area (in front of the rows' own regions)
  static __device__ __forceinline__ lds_ptr pack_lds() {
    extern __shared__ __attribute__((aligned(16))) double smem_[];
    return (lds_ptr)smem_ + row() * P::kPackQp;
  }
  // Twenty spare doubles of the row's LDS region: the solver loop parks its scalars
  // there while a Newton step and its line search run (Solver::solve_stream).
  static __device__ __forceinline__ lds_ptr save_area() { return lds() + P::kLdsDoubles + 4; }
  // the row's table of matrix-copy offsets, behind the four row regions
  __device__ __forceinline__ typename P::lds_iptr lpo() const {
    extern __shared__ __attribute__((aligned(16))) double smem_[];
    return (typename P::lds_iptr)((lds_ptr)smem_ + P::kPackArea + P::kQpPerWave * P::kLdsPerRow) + row() * P::lpo_ints(N);
  }
  __device__ __forceinline__ double* slot_ptr(long slot) const { return scratch + slot * P::ws_doubles(N); }
  // ctl[1]: Newton steps of this launch that were refined (fbstab_hip_mpc_refined_steps)
  __device__ __forceinline__ void count_refinement() const {
    if (tid() == 0) atomicAdd(&ctl[1], 1);
  }

  // Sweep: the rows of a wavefront start every step of their trajectories together
  // (Solver::solve_stream, kPause) - warm-started steps are mostly passes over the
  // records, which four rows out of step would run one after the other.
  static constexpr bool kCanAlignRows = KEEP;  // (the batch instances compile the plain loop)
  __device__ __forceinline__ bool align_rows() const { return sweep != nullptr; }
  // Binds the policy to the next QP of the queue, in this row's own slot.
  __device__ __forceinline__ int fetch(P& pp) {
    int q = 0;
    if constexpr (KEEP) {
      q = home();
      if (sweep) {
        if (q >= batch) return -1;
        const int done = swept & 0xffff;
        bool gone = (swept & (1 << 30)) != 0;
        if (done > 0) gone = receding_plant_step(sweep, x, out, batch, q, done - 1, tid(), P::LPQ, gone);
        if (done >= sweep->steps) return -1;
        swept = (done + 1) | (gone ? (1 << 30) : 0);
        pp.bind(slot_ptr(home()), lds(), pack_lds(), lpo(), data, x, q, N, tid());
        pp.reuse = reuse || done > 0;
        return q;
      }
      if (taken) return -1;
      taken = true;
    } else {
      // a batch that does not outnumber the launch's wavefronts: one QP per wavefront (fbstab_hip.hip sizes
      // the grid to the batch then); the other rows only lend their lanes to the cooperative passes
      if (batch <= (int)gridDim.x && row() != 0) return -1;
      if (tid() == 0) {
        q = atomicAdd(&ctl[0], 1);
        // (the ticket is checked before it indexes: the rows that find the queue dry hold tickets past the batch)
        if constexpr (ORDERED)
          if (order != nullptr && q < batch) q = order[q];
      }
      q = bcri<P::LPQ / 16, 0>(q);
    }
    if (q >= batch) return -1;
    pp.bind(slot_ptr(home()), lds(), pack_lds(), lpo(), data, x, q, N, tid());
    if constexpr (KEEP) pp.reuse = reuse;
    return q;
  }
};

// KEEP (FBSTAB_HIP_KEEP_MATRICES): QP q is solved in slot q, so that the slot's
// matrix copies survive from call to call; `reuse` says they are valid already.
// FB_R16_REG_CAP: the register budget of the kernel, arch VGPRs + AGPRs, in units of TWO registers (the
// compiler doubles "amdgpu-num-vgpr" on the unified file of gfx90a and later, and gives a function without
// MFMA all 256 arch VGPRs first): 248 = 496 registers.  One wavefront holds its SIMD for the whole launch;
// at 496 of the SIMD's 512 registers sixteen stay free and the small kernels a caller queues between two
// solves (the fill kernel behind hipMemsetAsync / torch's zero_()) find room beside it - at 504 they wait for a
// whole launch to end, and eight launches in flight run one after the other: 630 k -> 250 k QP/s
// (LABNOTES R6.3; tools/check_vgpr_budget.py is the build's gate on the result).
#ifndef FB_R16_REG_CAP
#define FB_R16_REG_CAP 248
#endif
#if FB_R16_REG_CAP > 0
#define FB_R16_REG_ATTR __attribute__((amdgpu_num_vgpr(FB_R16_REG_CAP)))
#else
#define FB_R16_REG_ATTR
#endif
template <int NX, int NU, int NC, bool DBG, bool EXACT, bool KEEP = false, int R = 1>
__global__ __launch_bounds__(64, 1) FB_R16_REG_ATTR void fbstab_mpc_r16_kernel(
    MpcBatchPtrs data, fbstab_var_batch_t x, fbstab_solver_out_t* out, fbstab_options_t opts, double* scratch,
    int* counter, int batch, int N, int reuse, double* dbg) {
  typedef MpcR16<NX, NU, NC, EXACT, KEEP, R> P;
  extern __shared__ __attribute__((aligned(16))) double smem[];
#if defined(FB_ANY_STAMP)
  const long long clk0 = __builtin_readcyclecounter(), rt0 = wall_clock64();
#endif
  const int lane = threadIdx.x;
  typename P::C ctx;
  ctx.tid = lane & (P::LPQ - 1);
  P p;
  // (the batch solve instance has no other use for `dbg`: the order of its queue, or null - fbstab_hip.hip)
  constexpr bool kOrdered = !KEEP && !DBG;
  R16Queue<P, KEEP, kOrdered> qu;
  if constexpr (kOrdered) qu.order = reinterpret_cast<const int*>(dbg);
  qu.data = &data;
  qu.x = &x;
  qu.ctl = counter;
  qu.scratch = scratch;
  qu.batch = batch;
  qu.N = N;
  qu.reuse = reuse != 0;
  if constexpr (KEEP && !DBG) {
    qu.sweep = reinterpret_cast<const SweepArgs*>(dbg);
    qu.out = out;
  }
  p.bind_idle(qu.lds(), qu.pack_lds(), qu.lpo(), N);  // (what the rows' unbound policy objects did: DESIGN.md section 7)
  if constexpr (DBG) {
    if (qu.fetch(p) >= 0) newton_probe(p, ctx, opts, dbg);
  } else {
    Solver<P, typename P::C> solver(p, ctx, opts);
    solver.solve_stream(qu, out);
  }
#if defined(FB_ANY_STAMP)
  // shader clock actually delivered to this wavefront: s_memtime vs the 100 MHz counter
  if (threadIdx.x == 0) {
    atomicAdd(&g_stamps[28], (unsigned long long)(__builtin_readcyclecounter() - clk0));
    atomicAdd(&g_stamps[29], (unsigned long long)(wall_clock64() - rt0));
  }
#endif
}

// The adjoint of fbstab_hip_mpc_adjoint_batch on the record instances (R: 16-lane rows per QP, as the solve
// kernel's): rows - row pairs - pull QPs from the counter as the solve's do; per QP the record is packed with the
// point as x = xbar (load_guess), one Newton step runs with the adjoint's right-hand side (MpcR16::adjoint_step: the
// solver's factor and sweeps, barrier_terms<true>), and the QP's lanes contract (dz, dl, dv) - left flat in the
// slot's matrix-copy region, which nothing reads after the step - with the point into the gradients
// (fb_adjoint.h).  The slot's matrix copies are overwritten: a FBSTAB_HIP_KEEP_MATRICES solve after it rebuilds
// them (fbstab_hip.hip resets kept_batch).
template <int NX, int NU, int NC, bool EXACT, int R>
__global__ __launch_bounds__(64, 1) FB_R16_REG_ATTR void fbstab_mpc_r16_adjoint_kernel(
    MpcBatchPtrs data, fbstab_var_batch_t x, AdjointArgs a, double* scratch, int* counter, int batch, int N) {
  typedef MpcR16<NX, NU, NC, EXACT, false, R> P;
  typename P::C ctx;
  ctx.tid = threadIdx.x & (P::LPQ - 1);
  P p;
  R16Queue<P, false> qu;
  qu.data = &data;
  qu.x = &x;
  qu.ctl = counter;
  qu.scratch = scratch;
  qu.batch = batch;
  qu.N = N;
  qu.reuse = false;
  p.bind_idle(qu.lds(), qu.pack_lds(), qu.lpo(), N);
  const int nx = EXACT ? NX : data.nx, nu = EXACT ? NU : data.nu, nc = EXACT ? NC : data.nc;
  const long nz = (long)(N + 1) * (nx + nu), nl = (long)(N + 1) * nx;
  for (;;) {
    const long q = qu.fetch(p);
    if (q < 0) break;
    // (this kernel's slots stay written out: mpc_grad_or_null and slot_or_null in their place re-schedule the exact
    // <12,4,32> and <24,8,32> instances - LABNOTES)
    auto at = [q](auto* b, long long s) { return b ? b + q * s : nullptr; };
    p.load_guess(ctx);
    p.choose_costate_form(a.sigma);
    double* const flat = qu.slot_ptr(qu.home()) + P::hdr_doubles(N);
    const bool ok = p.adjoint_step(ctx, a.sigma, a.alpha, at(a.seed[0], a.sstride[0]), at(a.seed[1], a.sstride[1]),
                                   at(a.seed[2], a.sstride[2]), flat);
    // the lanes' stores of the step are read by the row's other lanes
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    MpcGrad G;
    G.Q = at(a.grad.base[FBSTAB_MPC_Q], a.grad.stride[FBSTAB_MPC_Q]);
    G.R = at(a.grad.base[FBSTAB_MPC_R], a.grad.stride[FBSTAB_MPC_R]);
    G.S = at(a.grad.base[FBSTAB_MPC_S], a.grad.stride[FBSTAB_MPC_S]);
    G.q = at(a.grad.base[FBSTAB_MPC_q], a.grad.stride[FBSTAB_MPC_q]);
    G.r = at(a.grad.base[FBSTAB_MPC_r], a.grad.stride[FBSTAB_MPC_r]);
    G.A = at(a.grad.base[FBSTAB_MPC_A], a.grad.stride[FBSTAB_MPC_A]);
    G.B = at(a.grad.base[FBSTAB_MPC_B], a.grad.stride[FBSTAB_MPC_B]);
    G.c = at(a.grad.base[FBSTAB_MPC_c], a.grad.stride[FBSTAB_MPC_c]);
    G.E = at(a.grad.base[FBSTAB_MPC_E], a.grad.stride[FBSTAB_MPC_E]);
    G.L = at(a.grad.base[FBSTAB_MPC_L], a.grad.stride[FBSTAB_MPC_L]);
    G.d = at(a.grad.base[FBSTAB_MPC_d], a.grad.stride[FBSTAB_MPC_d]);
    G.x0 = at(a.grad.base[FBSTAB_MPC_x0], a.grad.stride[FBSTAB_MPC_x0]);
    mpc_adjoint_contract(ctx, N, nx, nu, nc, x.base[0] + q * x.stride[0], x.base[1] + q * x.stride[1],
                         x.base[2] + q * x.stride[2], flat, flat + nz, flat + nz + nl, G, ok, at(a.adj[0], a.astride[0]),
                         at(a.adj[1], a.astride[1]), at(a.adj[2], a.astride[2]));
    if (ctx.tid == 0) a.status[q] = ok ? 0 : 1;
    // (the next QP of this row packs its record over the flat step the contraction has read)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  }
}

// The adjoint of a whole receding-horizon sweep (fbstab_hip_mpc_receding_sweep_adjoint) on the record instances:
// rows - row pairs - pull TRAJECTORIES from the counter, and the row that owns trajectory q takes the costate
// backwards through its logged steps k = steps-1 .. 0 (include/fbstab_hip.h has the recursion): per step that
// counts, the adjoint kernel's work at the logged point - bind, load_guess, choose_costate_form, adjoint_step with
// the seed gu[k] + B'mu on the u0 entries - and the contraction ADDED into the trajectory's own gradient slots, by
// the lanes that zeroed them.  Lane t < nx carries lambda_t and mu_t in registers (the other lanes' entries come
// by shuffle within the row); the seed vector lives in the row slot's share of a.seed, which is zero outside the u0
// entries from the host's memset on.  No atomics, one fixed order: the same inputs give the same bits.
template <int NX, int NU, int NC, bool EXACT, int R>
__global__ __launch_bounds__(64, 1) FB_R16_REG_ATTR void fbstab_mpc_r16_sweep_adjoint_kernel(
    MpcBatchPtrs data, SweepAdjointArgs a, double* scratch, int* counter, int batch, int N) {
  typedef MpcR16<NX, NU, NC, EXACT, false, R> P;
  typename P::C ctx;
  ctx.tid = threadIdx.x & (P::LPQ - 1);
  P p;
  fbstab_var_batch_t xk;  // the logged point of the step in hand
  for (int i = 0; i < 4; i++) { xk.base[i] = nullptr; xk.stride[i] = 0; }
  R16Queue<P, false> qu;
  qu.data = &data;
  qu.x = &xk;
  qu.ctl = counter;
  qu.scratch = scratch;
  qu.batch = batch;
  qu.N = N;
  qu.reuse = false;
  p.bind_idle(qu.lds(), qu.pack_lds(), qu.lpo(), N);
  const int nx = EXACT ? NX : data.nx, nu = EXACT ? NU : data.nu, nc = EXACT ? NC : data.nc;
  const long nz = (long)(N + 1) * (nx + nu), nl = (long)(N + 1) * nx, nv = (long)(N + 1) * nc;
  const int t = ctx.tid;
  for (;;) {
    const long q = qu.fetch(p);
    if (q < 0) break;
    MpcGrad G = mpc_grad_or_null(a.grad, q);
    G.x0 = nullptr;  // (receives the final costate, below)
    {
      // zeros, by the lanes that add to the entries later (mpc_adjoint_contract's mapping)
      const int sq = nx * nx, sr = nu * nu, su = nu * nx, se = nc * nx, sl = nc * nu;
      auto zero = [t](double* g, long n) {
        if (g)
          for (long e = t; e < n; e += P::C::nt) g[e] = 0.0;
      };
      zero(G.Q, (long)(N + 1) * sq); zero(G.R, (long)(N + 1) * sr); zero(G.S, (long)(N + 1) * su);
      zero(G.q, (long)(N + 1) * nx); zero(G.r, (long)(N + 1) * nu); zero(G.A, (long)N * sq);
      zero(G.B, (long)N * su); zero(G.c, (long)N * nx); zero(G.E, (long)(N + 1) * se);
      zero(G.L, (long)(N + 1) * sl); zero(G.d, (long)(N + 1) * nc);
    }
    const double* Aq = a.A + q * a.sA;
    const double* Bq = a.B + q * a.sB;
    double* const seed = a.seed + (long)qu.home() * nz;
    double* const flat = qu.slot_ptr(qu.home()) + P::hdr_doubles(N);
    double lam = 0.0;  // lambda_t on the lanes t < nx
    int failed = 0;
    for (int k = a.steps - 1; k >= 0; k--) {
      const long long kq = (long long)k * batch + q;
      double mu = 0.0;
      if (t < nx) {
        mu = (a.gx ? a.gx[kq * nx + t] : 0.0) + lam;
        if (a.mu_log) a.mu_log[kq * nx + t] = mu;
      }
      const int e = a.le[kq];
      if (e == -1) {  // retired at or before this step: x_(k+1) and u_k are the constant 0
        lam = 0.0;
        continue;
      }
      // A'mu on the lanes t < nx, B'mu on the lanes t < nu
      double atm = 0.0, btm = 0.0;
      for (int r = 0; r < nx; r++) {
        const double mr = __shfl(mu, r, P::LPQ);
        if (t < nx) atm = fma(Aq[r + t * nx], mr, atm);
        if (t < nu) btm = fma(Bq[r + t * nx], mr, btm);
      }
      if (e != FBSTAB_SUCCESS) {  // the returned point is no solution: u_k is a constant
        lam = atm;
        continue;
      }
      if (t < nu) seed[nx + t] = (a.gu ? a.gu[kq * nu + t] : 0.0) + btm;
      xk.base[0] = const_cast<double*>(a.lz) + (long long)k * batch * nz; xk.stride[0] = nz;
      xk.base[1] = const_cast<double*>(a.ll) + (long long)k * batch * nl; xk.stride[1] = nl;
      xk.base[2] = const_cast<double*>(a.lv) + (long long)k * batch * nv; xk.stride[2] = nv;
      // the seed's stores are read by the row's other lanes
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
      p.bind(qu.slot_ptr(qu.home()), qu.lds(), qu.pack_lds(), qu.lpo(), &data, &xk, q, N, t);
      p.load_guess(ctx);
      p.choose_costate_form(a.sigma);
      const bool ok = p.adjoint_step(ctx, a.sigma, a.alpha, seed, nullptr, nullptr, flat);
      // the lanes' stores of the step are read by the row's other lanes
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
      if (ok) {
        mpc_adjoint_contract<true>(ctx, N, nx, nu, nc, xk.base[0] + q * nz, xk.base[1] + q * nl, xk.base[2] + q * nv,
                                   flat, flat + nz, flat + nz + nl, G, true, nullptr, nullptr, nullptr);
        lam = t < nx ? atm - flat[nz + t] : 0.0;
      } else {
        failed++;
        lam = atm;
      }
      // (the next step of this row packs its record over the flat step the contraction has read)
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
    if (a.grad.base[FBSTAB_MPC_x0] && t < nx) a.grad.base[FBSTAB_MPC_x0][q * a.grad.stride[FBSTAB_MPC_x0] + t] = lam;
    if (t == 0) a.status[q] = failed;
  }
}

template <int NX, int NU, int NC, int R>
long long r16_ws_doubles(int N) { return fbk::MpcR16<NX, NU, NC, true, false, R>::ws_doubles(N); }
template <int NX, int NU, int NC, int R>
int r16_lds_bytes(int N) {
  typedef fbk::MpcR16<NX, NU, NC, true, false, R> P;
  return (P::kPackArea + P::kQpPerWave * P::kLdsPerRow) * (int)sizeof(double) + P::kQpPerWave * P::lpo_ints(N) * (int)sizeof(int);
}
// The address of a kernel as the launch API and the handles' tables take it.
template <class Kernel>
const void* kernel_ptr(Kernel* k) { return reinterpret_cast<const void*>(k); }

// The solve kernels of one flavour.
template <int NX, int NU, int NC, int R, bool EXACT>
void r16_solve_kernels(RecordKernels* k) {
  k->solve = kernel_ptr(fbstab_mpc_r16_kernel<NX, NU, NC, false, EXACT, false, R>);
  k->solve_keep = kernel_ptr(fbstab_mpc_r16_kernel<NX, NU, NC, false, EXACT, true, R>);
  k->probe = kernel_ptr(fbstab_mpc_r16_kernel<NX, NU, NC, true, EXACT, false, R>);
}
// R: 16-lane rows of the wavefront per QP (1: four QPs per wavefront, stage width
// <= 16; 2: two QPs per wavefront, stage width <= 32)
template <int NX, int NU, int NC, int R = 1>
RecordInstance r16_instance(const char* name, const char* adjoint_name, const char* sweep_adjoint_name) {
  RecordInstance r;
  r.name = name;
  r.adjoint_name = adjoint_name;
  r.sweep_adjoint_name = sweep_adjoint_name;
  r.nx = NX; r.nu = NU; r.nc = NC;
  r.qps_per_wg = 4 / R;
  r.lds_bytes = r16_lds_bytes<NX, NU, NC, R>;
  r.ws_doubles = r16_ws_doubles<NX, NU, NC, R>;
  // (the kernels are named in the order the compiler has always met them - the solve kernels of both flavours, the
  // adjoints, the sweep adjoints: the code of some solve kernels, and the build's register report, depend on it;
  // tools/diff_device_code.py)
  r16_solve_kernels<NX, NU, NC, R, false>(&r.padded);
  r16_solve_kernels<NX, NU, NC, R, true>(&r.exact);
  r.padded.adjoint = kernel_ptr(fbstab_mpc_r16_adjoint_kernel<NX, NU, NC, false, R>);
  r.exact.adjoint = kernel_ptr(fbstab_mpc_r16_adjoint_kernel<NX, NU, NC, true, R>);
  r.padded.sweep_adjoint = kernel_ptr(fbstab_mpc_r16_sweep_adjoint_kernel<NX, NU, NC, false, R>);
  r.exact.sweep_adjoint = kernel_ptr(fbstab_mpc_r16_sweep_adjoint_kernel<NX, NU, NC, true, R>);
  return r;
}

}  // namespace

// Defines the factory of one instance (one per rec_*.hip); fbstab_hip.hip lists them.
#define FB_RECORD_INSTANCE(NX, NU, NC, R, NAME)                                              \
  __attribute__((visibility("hidden"))) RecordInstance fbstab_record_instance_##NX##_##NU##_##NC##_##R() { \
    return r16_instance<NX, NU, NC, R>(NAME, "fbstab_mpc_r16_adjoint_kernel<" #NX "," #NU "," #NC ">", \
                                       "fbstab_mpc_r16_sweep_adjoint_kernel<" #NX "," #NU "," #NC ">"); \
  }
#define FB_RECORD_INSTANCE_DECL(NX, NU, NC, R) \
  __attribute__((visibility("hidden"))) RecordInstance fbstab_record_instance_##NX##_##NU##_##NC##_##R();
