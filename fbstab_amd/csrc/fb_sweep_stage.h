// Host staging of the closed-loop sweeps of an MPC handle (include/fbstab_hip.h: fbstab_hip_mpc_receding_sweep,
// _logged, _scenario, fbstab_hip_mpc_receding_sweep_adjoint): the argument checks, the buffers and events of a call,
// the choice between one launch and one launch per step, the per-step offsets into the [steps][batch][n] logs and
// the carve-up of the handle's per-step scratch.  As fb_host_stage.h: no device code and no kernel header - the
// launches are passed in by fbstab_hip.hip, which fills the kernels' argument structs (SweepArgs, SweepLogStep,
// SweepCostateArgs, SweepAdjointArgs) from the plain values handed over here - and tests/test_host_stage.py runs it
// on the CPU, host lambdas in the kernels' place, under the address sanitizer.
#pragma once

#include "fb_host_stage.h"

namespace {

// What the sweeps read of an MPC handle beside its SolverBase (all zero for a null handle: the checks refuse it
// before any of this is read).
struct SweepShape {
  int N = 0, nx = 0, nu = 0, nc = 0;
  bool record = false;   // a record instance serves the handle: the sweep can be one launch
  int qps_per_wg = 1;
  bool adjoint_kernel = false;  // ... and so can its adjoint (the handle has the one-launch kernel)
};

// The sweep adjoint's scratch, which the MPC handle owns and frees, allocated by the first call that needs it: the
// seed vectors of the one-launch kernel (fbk::sweep_seed_bytes) and the per-step form's image of one step
// (sweep_tmp_doubles per QP of max_batch).
struct SweepScratch {
  double* seed = nullptr;
  double* tmp = nullptr;
};

// Step k's share of the caller's arrays, as the plant kernel behind the step's solve takes it.
struct SweepStep {
  int k = 0;
  double *z = nullptr, *l = nullptr, *v = nullptr, *x0 = nullptr;  // the log's [batch][n] of the step (null: not logged)
  int* eflag = nullptr;
  double* u_log = nullptr;            // [batch][nu], or null
  const double* w = nullptr;          // the step's disturbances [batch][nx], or null
  unsigned long long* stats = nullptr;  // the step's four counters (device)
  int shift_stages = 0;               // N: the warm start is shifted behind this step; 0: no shift, and the last step
};

// fbstab_hip_mpc_receding_sweep[_logged | _scenario] (`log`, `sc`: null where the entry point has none).  Record
// handles with a slot per trajectory: `Args` (SweepArgs) is filled by `fill_args(&args, d_stats, d_retired)`, copied to
// the device, and `one_launch(s, d_args)` is the whole sweep - the queue block zeroed, the timed launch.  Otherwise,
// per step, `solve(s, k)` (the KEEP solve on device pointers, asynchronous; k == 0 builds the matrix copies) and
// `plant_step(s, step, d_retired, d_xtmp)`.
template <class Args, class FillArgs, class OneLaunch, class Solve, class PlantStep>
int sweep_run(SolverBase* h, const SweepShape& sp, int batch, const fbstab_mpc_batch_t* data,
              const fbstab_var_batch_t* x, fbstab_solver_out_t* out, const fbstab_receding_plant_t* plant, int steps,
              double* u_log, unsigned long long* stats, float* kernel_ms, void* stream, const fbstab_sweep_log_t* log,
              const fbstab_sweep_scenario_t* sc, FillArgs fill_args, OneLaunch one_launch, Solve solve,
              PlantStep plant_step) {
  int rc = check_common(h, batch, data, x, out, h ? h->max_batch : 0);
  if (rc != FBSTAB_HIP_OK) return rc;
  if (!plant || !plant->A || !plant->B || steps < 0)
    return fail(FBSTAB_HIP_ERR_ARGUMENT, "plant matrices and a non-negative step count are required");
  if (sc && sc->shift != 0 && sc->shift != 1)
    return fail(FBSTAB_HIP_ERR_ARGUMENT, "receding sweep scenario: shift is 0 or 1");
  const double* w = sc ? sc->w : nullptr;
  const bool shift = sc && sc->shift == 1;
  for (int i = 0; i < FBSTAB_MPC_NSEQ; i++)
    if (!data->base[i]) return fail(FBSTAB_HIP_ERR_ARGUMENT, "null problem data pointer");
  for (int i = 0; i < 4; i++)
    if (!x->base[i]) return fail(FBSTAB_HIP_ERR_ARGUMENT, "null variable pointer");
  // x0 is advanced in place, one state per trajectory: a shared x0 would be written by all of them
  if (batch > 1 && data->stride[FBSTAB_MPC_x0] < sp.nx)
    return fail(FBSTAB_HIP_ERR_ARGUMENT, "receding sweep: every trajectory needs its own x0 (stride >= nx)");
  rc = h->check_solve_strides(data->stride, x->stride, batch, FBSTAB_MPC_x0);
  if (rc != FBSTAB_HIP_OK) return rc;
  if (batch == 0 || steps == 0) return FBSTAB_HIP_OK;
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t s = stream ? (hipStream_t)stream : h->stream;
  DevBuf d_ret, d_stats;
  const size_t stats_bytes = sizeof(unsigned long long) * 4 * (size_t)steps;
  HIP_TRY(hipMalloc(&d_ret.p, sizeof(int) * (size_t)batch));
  HIP_TRY(hipMalloc(&d_stats.p, stats_bytes));
  HIP_TRY(hipMemsetAsync(d_ret.p, 0, sizeof(int) * (size_t)batch, s));
  HIP_TRY(hipMemsetAsync(d_stats.p, 0, stats_bytes, s));
  int* const retired = static_cast<int*>(d_ret.p);
  unsigned long long* const dev_stats = static_cast<unsigned long long*>(d_stats.p);
  std::vector<hipEvent_t> ev;
  struct EvGuard {
    std::vector<hipEvent_t>& e;
    ~EvGuard() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
  } guard{ev};
  if (kernel_ms) {
    ev.resize(2 * (size_t)steps, nullptr);
    for (auto& e : ev) HIP_TRY(hipEventCreate(&e));
  }
  // Record kernels: the whole sweep is ONE launch of the KEEP instance, every row looping over its own trajectory
  // (FBSTAB_HIP_SWEEP_PER_STEP=1 keeps the launch per step below, which the flat-vector kernel always uses).
  if (sweep_in_one_launch(sp.record, batch, h->workgroups, sp.qps_per_wg, steps, sweep_per_step())) {
    Args args;  // (lives until the stream has been waited for)
    fill_args(&args, dev_stats, retired);
    DevBuf d_args;
    HIP_TRY(hipMalloc(&d_args.p, sizeof(Args)));
    HIP_TRY(hipMemcpyAsync(d_args.p, &args, sizeof(Args), hipMemcpyHostToDevice, s));
    RC_TRY(one_launch(s, static_cast<double*>(d_args.p)));
    if (stats) HIP_TRY(hipMemcpyAsync(stats, dev_stats, stats_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (kernel_ms) {  // one launch: every step is charged its share
      float ms = 0.f;
      HIP_TRY(hipEventElapsedTime(&ms, h->ev0, h->ev1));
      for (int k = 0; k < steps; k++) kernel_ms[k] = ms / (float)steps;
    }
    return FBSTAB_HIP_OK;
  }
  const long long nz = h->var_len[0], nl = h->var_len[1], nv = h->var_len[2];
  DevBuf d_xtmp;  // the plant step's new states, for more than 64 of them per trajectory
  if (sp.nx > 64) HIP_TRY(hipMalloc(&d_xtmp.p, sizeof(double) * (size_t)batch * sp.nx));
  for (int k = 0; k < steps; k++) {
    if (kernel_ms) HIP_TRY(hipEventRecord(ev[2 * k], s));
    RC_TRY(solve(s, k));
    if (kernel_ms) HIP_TRY(hipEventRecord(ev[2 * k + 1], s));
    const long long kb = (long long)k * batch;
    SweepStep st;
    st.k = k;
    if (log) {
      st.z = log->z ? log->z + kb * nz : nullptr;
      st.l = log->l ? log->l + kb * nl : nullptr;
      st.v = log->v ? log->v + kb * nv : nullptr;
      st.x0 = log->x0 ? log->x0 + kb * sp.nx : nullptr;
      st.eflag = log->eflag ? log->eflag + kb : nullptr;
    }
    st.u_log = u_log ? u_log + kb * sp.nu : nullptr;
    st.w = w ? w + kb * sp.nx : nullptr;
    st.stats = dev_stats + 4 * k;
    st.shift_stages = shift && k + 1 < steps ? sp.N : 0;
    plant_step(s, st, retired, static_cast<double*>(d_xtmp.p));
  }
  HIP_TRY(hipGetLastError());
  if (stats) HIP_TRY(hipMemcpyAsync(stats, dev_stats, stats_bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (kernel_ms)
    for (int k = 0; k < steps; k++) HIP_TRY(hipEventElapsedTime(&kernel_ms[k], ev[2 * k], ev[2 * k + 1]));
  return FBSTAB_HIP_OK;
}

// ---- reverse mode through a logged sweep --------------------------------------------------------------------------
// Handles with the one-launch kernel take it unless FBSTAB_HIP_SWEEP_ADJOINT_PER_STEP=1 says otherwise.
inline bool sweep_adjoint_in_one_launch(const SweepShape& sp) { return sp.adjoint_kernel && !sweep_adjoint_per_step(); }

// The per-step form's scratch per QP: the image of one step (every sequence), the seed vector, lambda / mu, A'mu and
// the step's status word, in a double's place.
inline long long sweep_tmp_doubles(const SolverBase* h, int nx) {
  long long img = 0;
  for (long long n : h->arr_len) img += n;
  return img + h->var_len[0] + 2 * nx + 1;
}

// What the costate kernel reads of that scratch and of step k's share of the caller's arrays (phase 0: no step yet).
struct SweepCostateStep {
  const double* tmp[FBSTAB_MPC_NSEQ];  // the image of one step (null where the caller takes no gradient; x0 always)
  long long len[FBSTAB_MPC_NSEQ];
  double *seed = nullptr, *lam = nullptr, *atm = nullptr;  // [batch][nz], [batch][nx], [batch][nx]
  int* tmp_status = nullptr;
  const int* eflag = nullptr;                  // step k's [batch]
  const double *gu = nullptr, *gx = nullptr;   // step k's [batch][nu | nx], or null
  double* mu_log = nullptr;                    // step k's [batch][nx], or null
};

// fbstab_hip_mpc_receding_sweep_adjoint.  One launch: `one_launch(s, a, seed)` on the problem data `a` (the x0 slot
// pointing at the logged z) and the handle's zeroed seed vectors - the queue block zeroed, the timed launch.  Per step:
// `costate(s, c, 0, 0)`, then for k = steps - 1 .. 0 `costate(s, c, 1, 0)`, `adjoint(st, sigma)` (the handle's adjoint
// launch on step k of the log, its gradients into the scratch image) and `costate(s, c, 2, k == 0)`.
template <class OneLaunch, class Costate, class Adjoint>
int sweep_adjoint_run(SolverBase* h, const SweepShape& sp, SweepScratch& scratch, int batch,
                      const fbstab_mpc_batch_t* data, const fbstab_receding_plant_t* plant, int steps,
                      const fbstab_sweep_log_t* log, const double* gu, const double* gx, double sigma,
                      const fbstab_mpc_grad_batch_t* grad, double* mu_log, int* status, void* stream,
                      OneLaunch one_launch, Costate costate, Adjoint adjoint) {
  // what needs no handle comes first
  if (!log) return fail(FBSTAB_HIP_ERR_ARGUMENT, "sweep adjoint: null log");
  if (!log->z || !log->l || !log->v || !log->eflag)
    return fail(FBSTAB_HIP_ERR_ARGUMENT, "sweep adjoint: the log's z, l, v and eflag are required");
  if (steps < 0) return fail(FBSTAB_HIP_ERR_ARGUMENT, "sweep adjoint: negative step count");
  if (!data || !grad || !status) return fail(FBSTAB_HIP_ERR_ARGUMENT, "null argument");
  if (!plant || !plant->A || !plant->B) return fail(FBSTAB_HIP_ERR_ARGUMENT, "sweep adjoint: plant matrices are required");
  for (int i = 0; i < FBSTAB_MPC_NSEQ; i++)
    if (batch > 1 && grad->base[i] && grad->stride[i] == 0)
      return fail(FBSTAB_HIP_ERR_ARGUMENT,
                  "sweep adjoint: a gradient slot of stride 0 (summed over the batch) is not served");
  if (!h) return fail(FBSTAB_HIP_ERR_ARGUMENT, "null solver handle");
  if (batch < 0 || batch > h->max_batch)
    return fail(FBSTAB_HIP_ERR_ARGUMENT, "batch exceeds the max_batch the handle was created with");
  for (int i = 0; i < FBSTAB_MPC_NSEQ; i++) {
    if (i != FBSTAB_MPC_x0 && !data->base[i]) return fail(FBSTAB_HIP_ERR_ARGUMENT, "null problem data pointer");
    if (batch > 1 && i != FBSTAB_MPC_x0 && data->stride[i] != 0 && data->stride[i] < h->arr_len[i])
      return fail(FBSTAB_HIP_ERR_ARGUMENT, "problem data stride smaller than the array length");
    if (batch > 1 && grad->base[i] && grad->stride[i] < h->arr_len[i])
      return fail(FBSTAB_HIP_ERR_ARGUMENT, "gradient stride smaller than the array length");
  }
  if (batch == 0) return FBSTAB_HIP_OK;
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t s = stream ? (hipStream_t)stream : h->stream;
  const double sig = sigma_or_default(sigma);
  const long long nz = h->var_len[0], nl = h->var_len[1], nv = h->var_len[2];
  // the kernels' problem data: the x0 slot, which the Newton matrix at x = xbar does not depend on, points at the
  // states of the logged z (the record packs read SOMETHING there)
  fbstab_mpc_batch_t a = *data;
  if (batch == 1)
    for (int i = 0; i < FBSTAB_MPC_NSEQ; i++) a.stride[i] = 0;
  a.base[FBSTAB_MPC_x0] = log->z;
  a.stride[FBSTAB_MPC_x0] = nz;
  if (sweep_adjoint_in_one_launch(sp)) {
    const size_t seed_bytes = sweep_seed_bytes(nz, h->workgroups, sp.qps_per_wg);
    if (!scratch.seed) HIP_TRY(hipMalloc(&scratch.seed, seed_bytes));
    HIP_TRY(hipMemsetAsync(scratch.seed, 0, seed_bytes, s));
    RC_TRY(one_launch(s, a, scratch.seed));
    HIP_TRY(hipStreamSynchronize(s));
    return FBSTAB_HIP_OK;
  }
  if (!scratch.tmp)
    HIP_TRY(hipMalloc(&scratch.tmp, sizeof(double) * (size_t)sweep_tmp_doubles(h, sp.nx) * (size_t)h->max_batch));
  SweepCostateStep c;
  AdjointLaunchArgs st;
  double* w = scratch.tmp;
  st.a = a;
  for (int i = 0; i < FBSTAB_MPC_NSEQ; i++) {
    const bool wanted = grad->base[i] != nullptr || i == FBSTAB_MPC_x0;
    c.len[i] = h->arr_len[i];
    c.tmp[i] = wanted ? w : nullptr;
    st.g.base[i] = wanted ? w : nullptr; st.g.stride[i] = h->arr_len[i];
    w += h->arr_len[i] * h->max_batch;
  }
  c.seed = w; w += nz * h->max_batch;
  c.lam = w; w += (long long)sp.nx * h->max_batch;
  c.atm = w; w += (long long)sp.nx * h->max_batch;
  c.tmp_status = reinterpret_cast<int*>(w);
  st.v = st.sd = st.ad = fbstab_var_batch_t{};
  st.sd.base[0] = c.seed; st.sd.stride[0] = nz;
  st.d_st = c.tmp_status;
  st.s = s;
  costate(s, c, 0, 0);
  HIP_TRY(hipGetLastError());
  for (int k = steps - 1; k >= 0; k--) {
    const long long kb = (long long)k * batch;
    c.eflag = log->eflag + kb;
    c.gu = gu ? gu + kb * sp.nu : nullptr;
    c.gx = gx ? gx + kb * sp.nx : nullptr;
    c.mu_log = mu_log ? mu_log + kb * sp.nx : nullptr;
    costate(s, c, 1, 0);
    HIP_TRY(hipGetLastError());
    st.v.base[0] = log->z + kb * nz; st.v.stride[0] = nz;
    st.v.base[1] = log->l + kb * nl; st.v.stride[1] = nl;
    st.v.base[2] = log->v + kb * nv; st.v.stride[2] = nv;
    RC_TRY(adjoint(st, sig));
    costate(s, c, 2, k == 0 ? 1 : 0);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipStreamSynchronize(s));
  return FBSTAB_HIP_OK;
}

}  // namespace
