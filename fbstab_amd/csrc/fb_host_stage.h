// Host staging of the C-ABI (include/fbstab_hip.h): what every entry point of fbstab_hip.hip does around its
// launches - the error text, a handle's buffers, the callers' arrays in and out, the stride rules that take the
// handle's lengths.  No device code and no kernel header: the launches themselves are passed in by fbstab_hip.hip,
// so tests/test_host_stage.py compiles this header with the host compiler over a heap-backed <hip/hip_runtime.h>
// (tests/hostsim/runtime_shim) and runs it, host lambdas in the kernels' place, under the address sanitizer.
#pragma once

#include <hip/hip_runtime.h>

#include <chrono>
#include <string>
#include <vector>

#include "../../include/fbstab_hip.h"
#include "fb_grad_reduce_plan.h"
#include "fb_launch_plan.h"

namespace {

using namespace fbk;

// ---------------------------------------------------------------------------
thread_local std::string g_error;

inline int fail(int code, const std::string& msg) {
  g_error = msg;
  return code;
}

#define HIP_TRY(expr)                                                                  \
  do {                                                                                 \
    hipError_t e_ = (expr);                                                            \
    if (e_ != hipSuccess)                                                              \
      return fail(FBSTAB_HIP_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

#define RC_TRY(expr)                        \
  do {                                      \
    int rc_ = (expr);                       \
    if (rc_ != FBSTAB_HIP_OK) return rc_;   \
  } while (0)

// sigma of the derivative entry points: what the caller gave, or the reference's default sigma0
// (fbstab_algorithm-impl.h:34), whatever the handle's options say
constexpr double kDefaultSigma = 1e-8;
inline double sigma_or_default(double sigma) { return sigma > 0.0 ? sigma : kDefaultSigma; }

// One operation of a handle (solve, traced solve, probe, adjoint, ...) as the handle's creation resolved it
// (mpc_resolve_kernels, dense_resolve_kernels): the launch sites read the entry, and none of them asks the layout,
// the record instance or the environment again which compiled kernel serves the handle.
struct KernelEntry {
  const void* kern = nullptr;  // null: this handle does not run the operation
  const char* name = "";       // what the *_kernel_name functions report (the operations that have one)
  int block = 0;
  int lds = 0;           // dynamic LDS bytes of the launch
  bool lds_set = false;  // this handle has set the kernel's LDS attribute to `lds` (as tan_ready below: the attribute
                         // belongs to the kernel, and the value of the handle that set it last stands)
};

inline hipError_t set_lds_attribute(KernelEntry& e) {
  const hipError_t err = hipFuncSetAttribute(e.kern, hipFuncAttributeMaxDynamicSharedMemorySize, e.lds);
  e.lds_set = err == hipSuccess;
  return err;
}

// Launches an entry; the first launch of a handle's entry sets the LDS attribute.
inline int launch_entry(KernelEntry& e, int grid, void** args, hipStream_t s) {
  if (!e.lds_set) HIP_TRY(set_lds_attribute(e));
  HIP_TRY(hipLaunchKernel(e.kern, dim3(grid), dim3(e.block), args, (size_t)e.lds, s));
  return FBSTAB_HIP_OK;
}

// State shared by both solver kinds.
struct SolverBase {
  int device = 0;
  int max_batch = 0;
  int threads = 0;
  int lds_bytes = 0;
  int workgroups = 0;
  long long scratch_bytes = 0;
  fbstab_options_t opts;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  bool timed = false;
  int* counter = nullptr;
  double* scratch = nullptr;
  // staging for host-pointer calls
  std::vector<double*> d_arr;  // problem arrays
  std::vector<long long> arr_len;
  double* d_var[4] = {nullptr, nullptr, nullptr, nullptr};
  long long var_len[4] = {0, 0, 0, 0};
  fbstab_solver_out_t* d_out = nullptr;
  fbstab_solver_out_t* d_out_only = nullptr;  // FBSTAB_HIP_OUT_ON_HOST: device side of the records

  int ensure_out() {
    if (!d_out_only) HIP_TRY(hipMalloc(&d_out_only, sizeof(fbstab_solver_out_t) * (size_t)max_batch));
    return FBSTAB_HIP_OK;
  }
  double* d_norms = nullptr;  // fbstab_hip_*_solve_batch_final: device side of the norms returned to the host
  int ensure_norms() {
    if (!d_norms) HIP_TRY(hipMalloc(&d_norms, sizeof(double) * 4 * (size_t)max_batch));
    return FBSTAB_HIP_OK;
  }
  // workspace of the traced flat-vector MPC solve (kept from call to call)
  double* trace_ws = nullptr;
  // fbstab_hip_*_adjoint_batch_reduced (fb_grad_reduce.h), allocated by the first such call and held until destroy:
  // the adjoint steps of a caller who does not take them, max_batch x (nz + nl + nv) doubles, and the partial sums,
  // grad_reduce_scratch_doubles(plan, max_batch)
  // (red_adj is also where fbstab_hip_*_tangent_batch keeps the seeds between its two launches: ensure_seeds)
  double* red_adj = nullptr;
  double* red_scratch = nullptr;
  // the direction kernel's LDS attribute is set (to the limit: the attribute belongs to the kernel, not to the
  // handle, and handles of other shapes launch the same kernel)
  bool tan_ready = false;
  int ensure_seeds() {
    if (!red_adj)
      HIP_TRY(hipMalloc(&red_adj, sizeof(double) * (size_t)(var_len[0] + var_len[1] + var_len[2]) * max_batch));
    return FBSTAB_HIP_OK;
  }
  int ensure_reduce(const GradReducePlan& plan) {
    int rc = ensure_seeds();
    if (rc != FBSTAB_HIP_OK) return rc;
    if (!red_scratch)
      HIP_TRY(hipMalloc(&red_scratch, sizeof(double) * (size_t)grad_reduce_scratch_doubles(plan, max_batch)));
    return FBSTAB_HIP_OK;
  }

  SolverBase() = default;
  SolverBase(const SolverBase&) = delete;
  SolverBase& operator=(const SolverBase&) = delete;
  // Everything the handle holds on the device, whichever call allocated it (a handle whose creation failed half
  // way included).
  ~SolverBase() {
    (void)hipSetDevice(device);
    for (double* p : d_arr)
      if (p) (void)hipFree(p);
    for (int i = 0; i < 4; i++)
      if (d_var[i]) (void)hipFree(d_var[i]);
    if (d_out) (void)hipFree(d_out);
    if (d_out_only) (void)hipFree(d_out_only);
    if (d_norms) (void)hipFree(d_norms);
    if (trace_ws) (void)hipFree(trace_ws);
    if (red_adj) (void)hipFree(red_adj);
    if (red_scratch) (void)hipFree(red_scratch);
    if (scratch) (void)hipFree(scratch);
    if (counter) (void)hipFree(counter);
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    if (stream) (void)hipStreamDestroy(stream);
  }

  int common_init(int dev, int maxb) {
    device = dev;
    max_batch = maxb;
    fbstab_options_default(&opts);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
      return fail(FBSTAB_HIP_ERR_DEVICE, "no HIP device available (this library has no CPU path)");
    if (dev < 0 || dev >= ndev) return fail(FBSTAB_HIP_ERR_ARGUMENT, "bad device index");
    HIP_TRY(hipSetDevice(dev));
    // A blocking stream: ordered against the device's null stream in both
    // directions, so a caller that prepared its device arrays on the null stream
    // (and passes stream = NULL) needs no extra synchronisation.
    HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamDefault));
    HIP_TRY(hipEventCreate(&ev0));
    HIP_TRY(hipEventCreate(&ev1));
    HIP_TRY(hipMalloc(&counter, kQueueBytes));  // queue counter
    return FBSTAB_HIP_OK;
  }

  // Creation: the resident workgroups per CU of the kernel batches are launched with - its LDS attribute set; the
  // handle's other kernels get theirs with their first launch - and the device's CUs.
  int occupancy(KernelEntry& e, int* per_cu, int* cus) {
    hipError_t err = set_lds_attribute(e);
    if (err == hipSuccess) err = hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, e.kern, e.block, e.lds);
    hipDeviceProp_t prop;
    if (err == hipSuccess) err = hipGetDeviceProperties(&prop, device);
    if (err != hipSuccess)
      return fail(FBSTAB_HIP_ERR_DEVICE, std::string("occupancy query: ") + hipGetErrorString(err));
    *cus = prop.multiProcessorCount;
    return FBSTAB_HIP_OK;
  }

  // Lazily allocated staging for host-pointer calls.
  int ensure_staging() {
    if (d_out) return FBSTAB_HIP_OK;
    d_arr.assign(arr_len.size(), nullptr);
    for (size_t i = 0; i < arr_len.size(); i++)
      HIP_TRY(hipMalloc(&d_arr[i], sizeof(double) * (size_t)(arr_len[i] > 0 ? arr_len[i] : 1) * max_batch));
    for (int i = 0; i < 4; i++)
      HIP_TRY(hipMalloc(&d_var[i], sizeof(double) * (size_t)(var_len[i] > 0 ? var_len[i] : 1) * max_batch));
    HIP_TRY(hipMalloc(&d_out, sizeof(fbstab_solver_out_t) * (size_t)max_batch));
    return FBSTAB_HIP_OK;
  }

  // Host batch array -> packed device array (stride = len); stride 0 is kept.  One QP is at the base whatever the
  // stride says (include/fbstab_hip.h): the length stands in for it, here and in `download`.
  int upload(const double* host, long long stride, long long len, int batch, double* dev,
             long long* dev_stride, hipStream_t s) {
    if (len == 0) {
      *dev_stride = 0;
      return FBSTAB_HIP_OK;
    }
    if (batch == 1) stride = len;
    if (stride == 0) {
      HIP_TRY(hipMemcpyAsync(dev, host, sizeof(double) * len, hipMemcpyHostToDevice, s));
      *dev_stride = 0;
    } else if (stride == len) {
      HIP_TRY(hipMemcpyAsync(dev, host, sizeof(double) * len * batch, hipMemcpyHostToDevice, s));
      *dev_stride = len;
    } else {
      HIP_TRY(hipMemcpy2DAsync(dev, sizeof(double) * len, host, sizeof(double) * stride,
                               sizeof(double) * len, batch, hipMemcpyHostToDevice, s));
      *dev_stride = len;
    }
    return FBSTAB_HIP_OK;
  }
  int download(double* host, long long stride, long long len, int batch, const double* dev,
               hipStream_t s) {
    if (len == 0) return FBSTAB_HIP_OK;
    if (batch == 1) stride = len;
    if (stride == len) {
      HIP_TRY(hipMemcpyAsync(host, dev, sizeof(double) * len * batch, hipMemcpyDeviceToHost, s));
    } else {
      HIP_TRY(hipMemcpy2DAsync(host, sizeof(double) * stride, dev, sizeof(double) * len,
                               sizeof(double) * len, batch, hipMemcpyDeviceToHost, s));
    }
    return FBSTAB_HIP_OK;
  }

  // ---- staging shared by the solves, the adjoints and the Newton probes of both kinds ----
  // `out`, `norms` and the adjoints' `status` are host arrays for host-pointer calls and with FBSTAB_HIP_OUT_ON_HOST.
  static bool out_on_host(int flags) {
    return !(flags & FBSTAB_HIP_DEVICE_POINTERS) || (flags & FBSTAB_HIP_OUT_ON_HOST);
  }

  // The stride rule of the caller's problem arrays, on both pointer paths: with batch > 1 an array is shared by the
  // batch (stride 0) or every QP has its own (stride >= length; a negative stride is neither).  `skip`: a slot with
  // a rule of its own (the sweeps' x0), or -1.
  int check_data_strides(const long long* stride, int batch, int skip = -1) const {
    for (int i = 0; i < (int)arr_len.size(); i++)
      if (batch > 1 && i != skip && stride[i] != 0 && stride[i] < arr_len[i])
        return fail(FBSTAB_HIP_ERR_ARGUMENT, "problem data stride smaller than the array length");
    return FBSTAB_HIP_OK;
  }

  // The stride rule of a solve, before any device call: the problem arrays, and all of (z, l, v, y).
  int check_solve_strides(const long long* data_stride, const long long* var_stride, int batch, int skip = -1) const {
    int rc = check_data_strides(data_stride, batch, skip);
    for (int i = 0; i < 4 && rc == FBSTAB_HIP_OK; i++) rc = check_var_stride(var_stride, i, batch);
    return rc;
  }

  // Problem arrays in: the caller's arr_len.size() base / stride pairs -> the kernel-side ones (the caller has
  // checked the strides).  Device pointers pass through; host arrays are packed into d_arr.
  int stage_arrays(const double* const* base, const long long* stride, int batch, bool dev_ptrs, hipStream_t s,
                   const double** kbase, long long* kstride) {
    const int n = (int)arr_len.size();
    if (dev_ptrs) {
      for (int i = 0; i < n; i++) { kbase[i] = base[i]; kstride[i] = stride[i]; }
      return FBSTAB_HIP_OK;
    }
    int rc = ensure_staging();
    if (rc != FBSTAB_HIP_OK) return rc;
    for (int i = 0; i < n; i++) {
      rc = upload(base[i], stride[i], arr_len[i], batch, d_arr[i], &kstride[i], s);
      if (rc != FBSTAB_HIP_OK) return rc;
      kbase[i] = d_arr[i];
    }
    return FBSTAB_HIP_OK;
  }

  // The stride rule of the caller's (z, l, v, y): with batch > 1 every QP has its own vectors.
  int check_var_stride(const long long* stride, int i, int batch) const {
    if (batch > 1 && stride[i] < var_len[i])
      return fail(FBSTAB_HIP_ERR_ARGUMENT, "variable stride smaller than the vector length");
    return FBSTAB_HIP_OK;
  }

  // Variables in: the first n vectors of the caller's (z, l, v, y) -> v (the others null).  Device pointers pass
  // through; host vectors go to d_var, z, l, v uploaded (y is output only).  The caller has checked the strides.
  int stage_vars(double* const* base, const long long* stride, int n, int batch, bool dev_ptrs,
                 hipStream_t s, fbstab_var_batch_t* v) {
    *v = fbstab_var_batch_t{};
    if (dev_ptrs) {
      for (int i = 0; i < n; i++) { v->base[i] = base[i]; v->stride[i] = stride[i]; }
      return FBSTAB_HIP_OK;
    }
    int rc = ensure_staging();
    if (rc != FBSTAB_HIP_OK) return rc;
    for (int i = 0; i < n; i++) {
      if (i < 3) {
        long long st;
        rc = upload(base[i], stride[i] ? stride[i] : var_len[i], var_len[i], batch, d_var[i], &st, s);
        if (rc != FBSTAB_HIP_OK) return rc;
      }
      v->base[i] = d_var[i];
      v->stride[i] = var_len[i];
    }
    return FBSTAB_HIP_OK;
  }

  // Where the solve kernel writes its records: `out` itself, or the device side of a host `out`.
  int stage_out(fbstab_solver_out_t* out, int flags, fbstab_solver_out_t** dev_out) {
    *dev_out = out;
    if (!(flags & FBSTAB_HIP_DEVICE_POINTERS)) {
      int rc = ensure_staging();
      if (rc != FBSTAB_HIP_OK) return rc;
      *dev_out = d_out;
    } else if (flags & FBSTAB_HIP_OUT_ON_HOST) {
      int rc = ensure_out();
      if (rc != FBSTAB_HIP_OK) return rc;
      *dev_out = d_out_only;
    }
    return FBSTAB_HIP_OK;
  }

  // Solve tail, before the final-norms kernel: where that kernel writes (`norms` lives where `out` lives).
  int stage_norms(double* norms, int flags, double** dev_norms) {
    *dev_norms = norms;
    if (out_on_host(flags)) {
      int rc = ensure_norms();
      if (rc != FBSTAB_HIP_OK) return rc;
      *dev_norms = d_norms;
    }
    return FBSTAB_HIP_OK;
  }

  // Solve tail, after it: norms, solution and records back to a host caller, who also gets the wall time of the
  // call from t0 on; the wait that the flags ask for.
  int finish_solve(const fbstab_var_batch_t* x, fbstab_solver_out_t* out, const fbstab_solver_out_t* dev_out,
                   double* norms, int batch, int flags, std::chrono::high_resolution_clock::time_point t0,
                   hipStream_t s) {
    if (norms && out_on_host(flags))
      HIP_TRY(hipMemcpyAsync(norms, d_norms, sizeof(double) * 4 * (size_t)batch, hipMemcpyDeviceToHost, s));
    if (!(flags & FBSTAB_HIP_DEVICE_POINTERS)) {
      for (int i = 0; i < 4; i++) {
        int rc = download(x->base[i], x->stride[i] ? x->stride[i] : var_len[i], var_len[i], batch, d_var[i], s);
        if (rc != FBSTAB_HIP_OK) return rc;
      }
    }
    if (out_on_host(flags)) {
      HIP_TRY(hipMemcpyAsync(out, dev_out, sizeof(fbstab_solver_out_t) * batch, hipMemcpyDeviceToHost, s));
      HIP_TRY(hipStreamSynchronize(s));
      const double dt = std::chrono::duration<double>(std::chrono::high_resolution_clock::now() - t0).count();
      for (int i = 0; i < batch; i++) out[i].solve_time = dt;
    } else if (!(flags & FBSTAB_HIP_ASYNC)) {
      HIP_TRY(hipStreamSynchronize(s));
    }
    return FBSTAB_HIP_OK;
  }

  // The bracket of the launch that last_kernel_ms reports: ev0 in front of it; behind it the launch's error,
  // ev1, and the mark that there is a time to report.
  int begin_timed(hipStream_t s) {
    HIP_TRY(hipEventRecord(ev0, s));
    return FBSTAB_HIP_OK;
  }
  int end_timed(hipStream_t s) {
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev1, s));
    timed = true;
    return FBSTAB_HIP_OK;
  }

  double last_kernel_ms() {
    if (!timed) return -1.0;
    (void)hipSetDevice(device);
    float ms = -1.f;
    if (hipEventSynchronize(ev1) != hipSuccess) return -1.0;
    if (hipEventElapsedTime(&ms, ev0, ev1) != hipSuccess) return -1.0;
    return (double)ms;
  }
};

// A handle's timed launch of an entry: the bracket of last_kernel_ms around launch_entry.
inline int launch_timed(SolverBase* h, KernelEntry& e, int grid, void** args, hipStream_t s) {
  RC_TRY(h->begin_timed(s));
  RC_TRY(launch_entry(e, grid, args, s));
  return h->end_timed(s);
}

// Device allocation released at scope exit.
struct DevBuf {
  void* p = nullptr;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { if (p) (void)hipFree(p); }
};

// Device side of fbstab_hip_*_solve_traced: 8 header doubles (record count,
// capacity) followed by the records (see Solver::emit in fb_algorithm.h).
struct TraceBuf {
  DevBuf buf;
  double* dev() const { return static_cast<double*>(buf.p); }
  int open(int device, const fbstab_trace_record_t* trace, int capacity, const int* count) {
    static_assert(sizeof(fbstab_trace_record_t) == 8 * sizeof(double), "record = 8 doubles");
    if (!trace || !count || capacity < 1)
      return fail(FBSTAB_HIP_ERR_ARGUMENT, "trace buffer, its capacity and the count pointer are required");
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipMalloc(&buf.p, sizeof(double) * 8 * ((size_t)capacity + 1)));
    const double hdr[8] = {0.0, (double)capacity, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    HIP_TRY(hipMemcpy(buf.p, hdr, sizeof(hdr), hipMemcpyHostToDevice));
    return FBSTAB_HIP_OK;
  }
  // the solve has synchronised its stream by now (host-pointer call)
  int close(fbstab_trace_record_t* trace, int capacity, int* count) {
    double hdr[8];
    HIP_TRY(hipMemcpy(hdr, buf.p, sizeof(hdr), hipMemcpyDeviceToHost));
    *count = (int)hdr[0];
    const int n = *count < capacity ? *count : capacity;
    if (n > 0)
      HIP_TRY(hipMemcpy(trace, dev() + 8, sizeof(fbstab_trace_record_t) * (size_t)n, hipMemcpyDeviceToHost));
    return FBSTAB_HIP_OK;
  }
};

// What an adjoint launch reads (mpc_adjoint_launch, dense_adjoint_launch): the kernel-side arguments, as
// AdjointStage::open stages them or as a caller whose arrays all live on the device fills them itself (the per-step
// sweep adjoint).  (The 12-slot blocks serve both kinds: a dense launch takes their first six slots, `narrowed`.)
struct AdjointLaunchArgs {
  fbstab_mpc_batch_t a;          // problem arrays
  fbstab_mpc_grad_batch_t g;     // their gradients (null: not asked for, or summed over the batch)
  fbstab_var_batch_t v, sd, ad;  // point, seeds, adjoints
  int* d_st = nullptr;           // status
  hipStream_t s = nullptr;
};

// The two launches of fb_grad_reduce.h behind a reduced adjoint's launch, on the arguments AdjointStage::reduce fills.
typedef int (*GradReduceLaunch)(const GradReduceArgs&, const GradReduceOut&, hipStream_t);

// Host side of fbstab_hip_*_adjoint_batch around the launch: `open` validates what takes the handle's lengths and
// stages the caller's arrays, `close` brings the results back.  In between `k` holds the kernel-side
// arguments.  (The `> 0` guards on arr_len / var_len act on dense handles with nl == 0 only: every length of an MPC
// handle is positive, fbstab_hip_mpc_create_in_flight refuses N, nx, nu, nc < 1.)
struct AdjointStage {
  static constexpr int kMaxArrays = FBSTAB_MPC_NSEQ;
  static_assert(FBSTAB_DENSE_NARR <= kMaxArrays, "one slot per problem array of either kind");
  AdjointLaunchArgs k;
  double* r_base[kMaxArrays];  // fbstab_hip_*_adjoint_batch_reduced: where the sum over the batch goes (null: per QP)
  bool any_reduced = false;

  // data, grad: base[] / stride[] of the caller's fbstab_*_batch_t and fbstab_*_grad_batch_t (h->arr_len.size()
  // slots).  With batch == 0 nothing is staged and the caller returns.  `reduced`: a gradient slot of stride 0 is
  // ONE array, the sum over the batch (otherwise refused like every stride below the length).  `seed` null: the
  // seeds are the library's own, device arrays that the caller puts into `k.sd` behind this call (TangentStage).
  int open(SolverBase* h, int batch, const double* const* data_base, const long long* data_stride,
           const fbstab_var_batch_t* x, const fbstab_var_batch_t* seed, double* const* grad_base,
           const long long* grad_stride, const fbstab_var_batch_t* adj, int* status, int flags, void* stream,
           bool reduced = false) {
    const int n = (int)h->arr_len.size();
    const long long* vlen = h->var_len;
    for (int i = 0; i < n; i++)
      if (!data_base[i] && h->arr_len[i] > 0) return fail(FBSTAB_HIP_ERR_ARGUMENT, "null problem data pointer");
    for (int i = 0; i < 3; i++)
      if (!x->base[i] && vlen[i] > 0) return fail(FBSTAB_HIP_ERR_ARGUMENT, "null variable pointer");
    // (the dense entry point has refused this one already)
    if (seed && !seed->base[0]) return fail(FBSTAB_HIP_ERR_ARGUMENT, "null seed pointer (z)");
    // strides: every QP its own slot (a gradient or adjoint shared by the batch would be written by all of them)
    for (int i = 0; i < 3; i++) {
      int rc = h->check_var_stride(x->stride, i, batch);
      if (rc != FBSTAB_HIP_OK) return rc;
      if (batch > 1 && seed && seed->base[i] && seed->stride[i] < vlen[i])
        return fail(FBSTAB_HIP_ERR_ARGUMENT, "seed stride smaller than the vector length");
      if (batch > 1 && adj && adj->base[i] && adj->stride[i] < vlen[i])
        return fail(FBSTAB_HIP_ERR_ARGUMENT, "adjoint stride smaller than the vector length");
    }
    {
      int rc = h->check_data_strides(data_stride, batch);
      if (rc != FBSTAB_HIP_OK) return rc;
    }
    for (int i = 0; i < n; i++)
      if (batch > 1 && grad_base[i] && grad_stride[i] < h->arr_len[i] && !(reduced && grad_stride[i] == 0))
        return fail(FBSTAB_HIP_ERR_ARGUMENT, "gradient stride smaller than the array length");
    for (int i = 0; i < kMaxArrays; i++) r_base[i] = nullptr;
    if (batch == 0) return FBSTAB_HIP_OK;
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = k.s = stream ? (hipStream_t)stream : h->stream;
    h_ = h; batch_ = batch; grad_base_ = grad_base; grad_stride_ = grad_stride; adj_ = adj; status_ = status;
    flags_ = flags;
    const bool dev_ptrs = (flags & FBSTAB_HIP_DEVICE_POINTERS) != 0;
    int rc = h->stage_arrays(data_base, data_stride, batch, dev_ptrs, s, k.a.base, k.a.stride);
    if (rc != FBSTAB_HIP_OK) return rc;
    rc = h->stage_vars(x->base, x->stride, 3, batch, dev_ptrs, s, &k.v);
    if (rc != FBSTAB_HIP_OK) return rc;
    fbstab_var_batch_t &sd = k.sd, &ad = k.ad;
    fbstab_mpc_grad_batch_t& g = k.g;
    sd = ad = fbstab_var_batch_t{};
    for (int i = 0; i < 3; i++) {
      if (vlen[i] == 0) continue;
      if (dev_ptrs) {
        if (seed) { sd.base[i] = seed->base[i]; sd.stride[i] = seed->stride[i]; }
        if (adj) { ad.base[i] = adj->base[i]; ad.stride[i] = adj->stride[i]; }
        continue;
      }
      if (seed && seed->base[i]) {
        HIP_TRY(hipMalloc(&d_seed[i].p, sizeof(double) * (size_t)vlen[i] * batch));
        sd.base[i] = static_cast<double*>(d_seed[i].p);
        rc = h->upload(seed->base[i], seed->stride[i] ? seed->stride[i] : vlen[i], vlen[i], batch, sd.base[i],
                       &sd.stride[i], s);
        if (rc != FBSTAB_HIP_OK) return rc;
      }
      if (adj && adj->base[i]) {
        HIP_TRY(hipMalloc(&d_adj[i].p, sizeof(double) * (size_t)vlen[i] * batch));
        ad.base[i] = static_cast<double*>(d_adj[i].p); ad.stride[i] = vlen[i];
      }
    }
    for (int i = 0; i < n; i++) {
      const bool asked = grad_base[i] && h->arr_len[i] > 0;  // (nl == 0: the G and h slots are ignored)
      if (asked && reduced && grad_stride[i] == 0) {
        // the adjoint kernel does not write this image: fb_grad_reduce.h forms its sum from (x, adj)
        g.base[i] = nullptr; g.stride[i] = 0;
        r_base[i] = grad_base[i];
        if (!dev_ptrs) {
          HIP_TRY(hipMalloc(&d_grad[i].p, sizeof(double) * (size_t)h->arr_len[i]));
          r_base[i] = static_cast<double*>(d_grad[i].p);
        }
        any_reduced = true;
      } else if (dev_ptrs) {
        g.base[i] = asked ? grad_base[i] : nullptr; g.stride[i] = grad_stride[i];
      } else if (asked) {
        HIP_TRY(hipMalloc(&d_grad[i].p, sizeof(double) * (size_t)h->arr_len[i] * batch));
        g.base[i] = static_cast<double*>(d_grad[i].p); g.stride[i] = h->arr_len[i];
      } else {
        g.base[i] = nullptr; g.stride[i] = 0;
      }
    }
    k.d_st = status;
    if (SolverBase::out_on_host(flags)) {
      HIP_TRY(hipMalloc(&d_status.p, sizeof(int) * (size_t)batch));
      k.d_st = static_cast<int*>(d_status.p);
    }
    return FBSTAB_HIP_OK;
  }

  // fbstab_hip_*_adjoint_batch_reduced with a slot to sum, before the adjoint's launch: the handle's buffers, and
  // the adjoint steps the caller does not take go to the handle's own (the sums are formed from them).
  int open_reduce(const GradReducePlan& plan) {
    int rc = h_->ensure_reduce(plan);
    if (rc != FBSTAB_HIP_OK) return rc;
    double* own = h_->red_adj;
    for (int i = 0; i < 3; i++) {
      if (!k.ad.base[i] && h_->var_len[i] > 0) { k.ad.base[i] = own; k.ad.stride[i] = h_->var_len[i]; }
      own += h_->var_len[i] * h_->max_batch;
    }
    return FBSTAB_HIP_OK;
  }
  // ... and after it, on the same stream: the partial sums, then the sums into the reduced slots (`launch`).  `out`:
  // null, or the solve's records, living where `status` lives.
  int reduce(const GradReducePlan& plan, const fbstab_solver_out_t* out, GradReduceLaunch launch) {
    GradReduceArgs ra;
    ra.plan = plan;
    for (int i = 0; i < 3; i++) {
      ra.x[i] = k.v.base[i]; ra.xs[i] = k.v.stride[i];
      ra.p[i] = k.ad.base[i]; ra.ps[i] = k.ad.stride[i];
    }
    ra.status = k.d_st;
    ra.out = out;
    if (out && SolverBase::out_on_host(flags_)) {
      HIP_TRY(hipMalloc(&d_out.p, sizeof(fbstab_solver_out_t) * (size_t)batch_));
      HIP_TRY(hipMemcpyAsync(d_out.p, out, sizeof(fbstab_solver_out_t) * (size_t)batch_, hipMemcpyHostToDevice, k.s));
      ra.out = static_cast<const fbstab_solver_out_t*>(d_out.p);
    }
    ra.scratch = h_->red_scratch;
    ra.batch = batch_;
    GradReduceOut ro;
    for (int i = 0; i < kGradReduceMaxSeq; i++) ro.base[i] = i < kMaxArrays ? r_base[i] : nullptr;
    return launch(ra, ro, k.s);
  }

  int close() {
    hipStream_t s = k.s;
    if (!(flags_ & FBSTAB_HIP_DEVICE_POINTERS)) {
      for (size_t i = 0; i < h_->arr_len.size(); i++)
        if (k.g.base[i]) {
          int rc = h_->download(grad_base_[i], grad_stride_[i] ? grad_stride_[i] : h_->arr_len[i], h_->arr_len[i],
                                batch_, k.g.base[i], s);
          if (rc != FBSTAB_HIP_OK) return rc;
        } else if (r_base[i]) {
          int rc = h_->download(grad_base_[i], h_->arr_len[i], h_->arr_len[i], 1, r_base[i], s);
          if (rc != FBSTAB_HIP_OK) return rc;
        }
      for (int i = 0; i < 3; i++)
        if (k.ad.base[i] && adj_ && adj_->base[i]) {  // (a reduced call may have pointed the others at the handle's own)
          int rc = h_->download(adj_->base[i], adj_->stride[i] ? adj_->stride[i] : h_->var_len[i], h_->var_len[i],
                                batch_, k.ad.base[i], s);
          if (rc != FBSTAB_HIP_OK) return rc;
        }
    }
    const bool status_host = SolverBase::out_on_host(flags_);
    if (status_host) HIP_TRY(hipMemcpyAsync(status_, k.d_st, sizeof(int) * (size_t)batch_, hipMemcpyDeviceToHost, s));
    if (status_host || !(flags_ & FBSTAB_HIP_ASYNC)) HIP_TRY(hipStreamSynchronize(s));
    return FBSTAB_HIP_OK;
  }

 private:
  DevBuf d_seed[3], d_adj[3], d_grad[kMaxArrays], d_status, d_out;
  // what `close` copies back to, and how
  SolverBase* h_ = nullptr;
  int batch_ = 0, flags_ = 0;
  double* const* grad_base_ = nullptr;
  const long long* grad_stride_ = nullptr;
  const fbstab_var_batch_t* adj_ = nullptr;
  int* status_ = nullptr;
};

// Host side of fbstab_hip_*_tangent_batch around the direction kernel's launch, beside the AdjointStage that serves
// the adjoint launch behind it (opened with no seeds, no gradients and adj = dx): `check` validates the
// perturbations and the result blocks, `open` stages the perturbations and says where the seeds live (st->sd),
// `close` brings a host caller's rhs back (before AdjointStage::close, which waits for the stream).
struct TangentStage {
  static constexpr int kMaxArrays = AdjointStage::kMaxArrays;
  fbstab_mpc_batch_t p;  // perturbations, kernel side (null: zero)

  // no gradient is asked of the adjoint launch
  static double* const* no_grads() {
    static double* const none[kMaxArrays] = {};
    return none;
  }
  static const long long* no_strides() {
    static const long long none[kMaxArrays] = {};
    return none;
  }

  // Before any device call.  dir: base[] / stride[] of the caller's perturbation block (null slots: zero; with
  // batch > 1 a stride of 0 is one direction for all QPs, anything else below the length is refused); dx: every
  // slot of a vector that is not empty; rhs: null, or the same.
  static int check(const SolverBase* h, int batch, const double* const* dir_base, const long long* dir_stride,
                   const fbstab_var_batch_t* dx, const fbstab_var_batch_t* rhs) {
    const int n = (int)h->arr_len.size();
    for (int i = 0; i < n; i++)
      if (batch > 1 && dir_base[i] && dir_stride[i] != 0 && dir_stride[i] < h->arr_len[i])
        return fail(FBSTAB_HIP_ERR_ARGUMENT, "perturbation stride is neither 0 nor at least the array length");
    for (int i = 0; i < 3; i++) {
      if (h->var_len[i] == 0) continue;
      if (!dx->base[i]) return fail(FBSTAB_HIP_ERR_ARGUMENT, "null tangent pointer (dx)");
      if (rhs && !rhs->base[i]) return fail(FBSTAB_HIP_ERR_ARGUMENT, "null right-hand side pointer (rhs)");
      if (batch > 1 && rhs && rhs->stride[i] < h->var_len[i])
        return fail(FBSTAB_HIP_ERR_ARGUMENT, "right-hand side stride smaller than the vector length");
    }
    return FBSTAB_HIP_OK;
  }

  // Behind AdjointStage::open (same stream).  The seeds go to the caller's rhs where that is device memory, and to
  // the handle's buffer (SolverBase::ensure_seeds) otherwise.
  int open(SolverBase* h, int batch, const double* const* dir_base, const long long* dir_stride,
           const fbstab_var_batch_t* rhs, int flags, AdjointLaunchArgs* st) {
    h_ = h; batch_ = batch; rhs_ = rhs; st_ = st;
    host_ = !(flags & FBSTAB_HIP_DEVICE_POINTERS);
    const int n = (int)h->arr_len.size();
    p = fbstab_mpc_batch_t{};
    for (int i = 0; i < n; i++) {
      if (!dir_base[i] || h->arr_len[i] == 0) continue;
      // (one QP: its direction is at the base, whatever the stride says)
      const long long stride = batch > 1 ? dir_stride[i] : h->arr_len[i];
      if (!host_) {
        p.base[i] = dir_base[i]; p.stride[i] = stride;
        continue;
      }
      HIP_TRY(hipMalloc(&d_dir[i].p, sizeof(double) * (size_t)h->arr_len[i] * (stride == 0 ? 1 : batch)));
      int rc = h->upload(dir_base[i], stride, h->arr_len[i], batch, static_cast<double*>(d_dir[i].p), &p.stride[i],
                         st->s);
      if (rc != FBSTAB_HIP_OK) return rc;
      p.base[i] = static_cast<double*>(d_dir[i].p);
    }
    const bool own = host_ || !rhs;
    if (own) {
      int rc = h->ensure_seeds();
      if (rc != FBSTAB_HIP_OK) return rc;
    }
    double* buf = h->red_adj;
    for (int i = 0; i < 3; i++) {
      if (h->var_len[i] > 0) {
        st->sd.base[i] = own ? buf : rhs->base[i];
        st->sd.stride[i] = own ? h->var_len[i] : rhs->stride[i];
      }
      buf += h->var_len[i] * h->max_batch;
    }
    return FBSTAB_HIP_OK;
  }

  int close() {
    if (!host_ || !rhs_) return FBSTAB_HIP_OK;
    for (int i = 0; i < 3; i++) {
      int rc = h_->download(rhs_->base[i], rhs_->stride[i] ? rhs_->stride[i] : h_->var_len[i], h_->var_len[i], batch_,
                            st_->sd.base[i], st_->s);
      if (rc != FBSTAB_HIP_OK) return rc;
    }
    return FBSTAB_HIP_OK;
  }

 private:
  DevBuf d_dir[kMaxArrays];
  SolverBase* h_ = nullptr;
  AdjointLaunchArgs* st_ = nullptr;
  const fbstab_var_batch_t* rhs_ = nullptr;
  int batch_ = 0;
  bool host_ = false;
};

// The dense launches' view of a stage's 12-slot block: its first six slots.
template <class Narrow, class Wide>
Narrow narrowed(const Wide& w) {
  Narrow n;
  for (int i = 0; i < FBSTAB_DENSE_NARR; i++) { n.base[i] = w.base[i]; n.stride[i] = w.stride[i]; }
  return n;
}

// What fbstab_hip_*_adjoint_batch[_reduced] of both kinds do behind their own argument checks: stage, launch
// (`launch`: mpc_adjoint_launch or dense_adjoint_launch), with a slot to sum the reduction around the launch
// (`launch_reduce`), and bring the results back.
template <class Handle, class Data, class Grad>
int adjoint_run(Handle h, int batch, const Data* data, const fbstab_var_batch_t* x,
                       const fbstab_var_batch_t* seed, double sigma, const Grad* grad, const fbstab_var_batch_t* adj,
                       int* status, const fbstab_solver_out_t* out, int flags, void* stream, bool reduced,
                       const GradReducePlan& plan, int (*launch)(Handle, int, AdjointLaunchArgs&, double),
                       GradReduceLaunch launch_reduce) {
  AdjointStage st;
  int rc = st.open(h, batch, data->base, data->stride, x, seed, grad->base, grad->stride, adj, status, flags, stream,
                   reduced);
  if (rc != FBSTAB_HIP_OK || batch == 0) return rc;
  if (st.any_reduced) RC_TRY(st.open_reduce(plan));
  RC_TRY(launch(h, batch, st.k, sigma));
  if (st.any_reduced) RC_TRY(st.reduce(plan, out, launch_reduce));
  return st.close();
}

// ... and fbstab_hip_*_tangent_batch behind their checks and their LDS layout: the adjoint's staging with no seeds,
// no gradients and adj = dx, the perturbations, the direction kernel (`kern`, launched by `launch_dir` on the staged
// perturbations, points and seeds), the adjoint's launch behind it, and the results back.
template <class Handle, class Data, class LaunchDir>
int tangent_run(Handle h, int batch, const Data* data, const fbstab_var_batch_t* x, const Data* ddata,
                       double sigma, const fbstab_var_batch_t* dx, const fbstab_var_batch_t* rhs, int* status, int flags,
                       void* stream, const void* kern, LaunchDir launch_dir,
                       int (*launch)(Handle, int, AdjointLaunchArgs&, double)) {
  AdjointStage st;
  int rc = st.open(h, batch, data->base, data->stride, x, nullptr, TangentStage::no_grads(), TangentStage::no_strides(),
                   dx, status, flags, stream);
  if (rc != FBSTAB_HIP_OK || batch == 0) return rc;
  TangentStage ts;
  RC_TRY(ts.open(h, batch, ddata->base, ddata->stride, rhs, flags, &st.k));
  if (!h->tan_ready) {
    HIP_TRY(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsLimitBytes));
    h->tan_ready = true;
  }
  launch_dir(ts.p, st.k);
  HIP_TRY(hipGetLastError());
  RC_TRY(launch(h, batch, st.k, sigma));
  RC_TRY(ts.close());
  return st.close();
}

// ... the solves of both kinds (batch, batch_final, traced): the argument checks, the staging, the queue block zeroed
// (the queue word, the refinement count, the dense kDenseFallbackSlot counters), the timed launch
// (`launch(s, a, v, d_out)`), with `norms` the final-norms kernel behind it (`launch_norms(s, a, v, d_norms)`), and
// the results back.
template <class Handle, class Data, class Launch, class LaunchNorms>
int solve_run(Handle h, int batch, const Data* data, const fbstab_var_batch_t* x, fbstab_solver_out_t* out, int flags,
              void* stream, double* norms, Launch launch, LaunchNorms launch_norms) {
  int rc = check_common(h, batch, data, x, out, h ? h->max_batch : 0);
  if (rc != FBSTAB_HIP_OK) return rc;
  for (size_t i = 0; i < h->arr_len.size(); i++)  // (nl == 0: the G and h slots of a dense handle are empty)
    if (!data->base[i] && h->arr_len[i] > 0) return fail(FBSTAB_HIP_ERR_ARGUMENT, "null problem data pointer");
  for (int i = 0; i < 4; i++)
    if (!x->base[i] && h->var_len[i] > 0) return fail(FBSTAB_HIP_ERR_ARGUMENT, "null variable pointer");
  rc = h->check_solve_strides(data->stride, x->stride, batch);
  if (rc != FBSTAB_HIP_OK) return rc;
  if (batch == 0) return FBSTAB_HIP_OK;
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t s = stream ? (hipStream_t)stream : h->stream;
  const bool dev_ptrs = (flags & FBSTAB_HIP_DEVICE_POINTERS) != 0;
  const auto t0 = std::chrono::high_resolution_clock::now();
  Data a;
  fbstab_var_batch_t v;
  fbstab_solver_out_t* d_out;
  RC_TRY(h->stage_arrays(data->base, data->stride, batch, dev_ptrs, s, a.base, a.stride));
  RC_TRY(h->stage_vars(x->base, x->stride, 4, batch, dev_ptrs, s, &v));
  RC_TRY(h->stage_out(out, flags, &d_out));
  HIP_TRY(hipMemsetAsync(h->counter, 0, kQueueBytes, s));
  RC_TRY(h->begin_timed(s));
  RC_TRY(launch(s, a, v, d_out));
  RC_TRY(h->end_timed(s));
  if (norms) {
    double* dn;
    RC_TRY(h->stage_norms(norms, flags, &dn));
    launch_norms(s, a, v, dn);
    HIP_TRY(hipGetLastError());
  }
  return h->finish_solve(x, out, d_out, norms, batch, flags, t0, s);
}

// ... and fbstab_hip_*_debug_newton: ONE QP given by host pointers is staged, io goes in, `launch(a, v, d_io)` puts
// the probe on the handle's stream, io comes back.
template <class Data, class Launch>
int probe_run(SolverBase* h, const Data* data, const fbstab_var_batch_t* x, double* io, Launch launch) {
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  Data a;
  fbstab_var_batch_t v;
  // (one packed QP whatever strides the caller wrote: the lengths stand in for them)
  RC_TRY(h->stage_arrays(data->base, h->arr_len.data(), 1, false, s, a.base, a.stride));
  RC_TRY(h->stage_vars(x->base, h->var_len, 4, 1, false, s, &v));
  const long long nz = h->var_len[0], nl = h->var_len[1], nv = h->var_len[2];
  const size_t n_io = (size_t)(3 * nz + 3 * nl + 2 * nv + 1);
  DevBuf d_io_buf;
  HIP_TRY(hipMalloc(&d_io_buf.p, n_io * sizeof(double)));
  double* d_io = static_cast<double*>(d_io_buf.p);
  HIP_TRY(hipMemcpyAsync(d_io, io, sizeof(double) * (nz + nl + nv), hipMemcpyHostToDevice, s));
  RC_TRY(launch(a, v, d_io));
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(io, d_io, sizeof(double) * n_io, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return FBSTAB_HIP_OK;
}

inline int check_common(const void* handle, int batch, const void* data, const fbstab_var_batch_t* x,
                        const void* out, int max_batch) {
  if (!handle) return fail(FBSTAB_HIP_ERR_ARGUMENT, "null solver handle");
  if (!data || !x || !out) return fail(FBSTAB_HIP_ERR_ARGUMENT, "null argument");
  if (batch < 0 || batch > max_batch)
    return fail(FBSTAB_HIP_ERR_ARGUMENT, "batch exceeds the max_batch the handle was created with");
  return FBSTAB_HIP_OK;
}

// ---- many right-hand sides on one factorisation (include/fbstab_hip.h; fb_kkt_multi.h) --------------------------
// The stride rule of a seed or step block, slot by slot: with batch > 1 or nrhs > 1, rhs_stride >= len[i] and
// stride >= (nrhs - 1) rhs_stride + len[i], or for a seed stride 0.  len == nullptr: before the handle is looked at,
// with the one length that no slot undercuts (1) - what fails here fails for every handle.
inline int check_multi_strides(const fbstab_multi_var_batch_t* b, const long long* len, int batch, int nrhs,
                               bool seed) {
  for (int i = 0; i < 3; i++) {
    if (!b->base[i]) continue;
    const long long n = len ? len[i] : 1;
    if (nrhs > 1 && b->rhs_stride[i] < n)
      return fail(FBSTAB_HIP_ERR_ARGUMENT, seed ? "seed rhs_stride smaller than the vector length"
                                                : "step rhs_stride smaller than the vector length");
    const long long span = (nrhs > 1 ? (nrhs - 1) * b->rhs_stride[i] : 0) + n;
    if (batch > 1 && b->stride[i] < span && !(seed && b->stride[i] == 0))
      return fail(FBSTAB_HIP_ERR_ARGUMENT, seed ? "seed stride smaller than the right-hand sides of one QP"
                                                : "step stride smaller than the right-hand sides of one QP");
  }
  return FBSTAB_HIP_OK;
}

// Kernel side of a caller's seed or step block.  Device pointers pass through (one QP: it is at the base; one
// right-hand side: rhs_stride is not read).  A host block is staged packed, [QP][rhs][len], in allocations of the call:
// `open` uploads a seed block (upload = true) or only allocates, `download` brings a step block back, vector by
// vector, so that the doubles between a QP's vectors stay as they are.
struct MultiStage {
  fbstab_multi_var_batch_t k{};
  DevBuf buf[3];

  static int copy(double* dst, long long dpitch, const double* src, long long spitch, long long len, long long rows,
                  hipMemcpyKind kind, hipStream_t s) {
    HIP_TRY(hipMemcpy2DAsync(dst, sizeof(double) * dpitch, src, sizeof(double) * spitch, sizeof(double) * len, rows,
                             kind, s));
    return FBSTAB_HIP_OK;
  }
  int open(const fbstab_multi_var_batch_t* b, const long long* len, int batch, int nrhs, bool dev_ptrs, bool upload,
           hipStream_t s) {
    for (int i = 0; i < 3; i++) {
      if (!b || !b->base[i] || len[i] == 0) continue;
      const long long rs = nrhs > 1 ? b->rhs_stride[i] : len[i];
      const long long st = batch > 1 ? b->stride[i] : 0;
      if (dev_ptrs) {
        k.base[i] = b->base[i]; k.stride[i] = st; k.rhs_stride[i] = rs;
        continue;
      }
      const long long nq = st == 0 ? 1 : batch;
      HIP_TRY(hipMalloc(&buf[i].p, sizeof(double) * (size_t)(len[i] * nrhs * nq)));
      k.base[i] = static_cast<double*>(buf[i].p);
      k.stride[i] = st == 0 ? 0 : len[i] * nrhs;
      k.rhs_stride[i] = len[i];
      if (!upload) continue;
      if (nq == 1 || st == nrhs * rs) {
        RC_TRY(copy(k.base[i], len[i], b->base[i], rs, len[i], nq * nrhs, hipMemcpyHostToDevice, s));
      } else {
        for (long long q = 0; q < nq; q++)
          RC_TRY(copy(k.base[i] + q * len[i] * nrhs, len[i], b->base[i] + q * st, rs, len[i], nrhs,
                      hipMemcpyHostToDevice, s));
      }
    }
    return FBSTAB_HIP_OK;
  }
  int download(const fbstab_multi_var_batch_t* b, const long long* len, int batch, int nrhs, hipStream_t s) {
    for (int i = 0; i < 3; i++) {
      if (!buf[i].p) continue;
      const long long rs = nrhs > 1 ? b->rhs_stride[i] : len[i];
      const long long st = batch > 1 ? b->stride[i] : 0;
      if (batch == 1 || st == nrhs * rs) {
        RC_TRY(copy(b->base[i], rs, k.base[i], len[i], len[i], (long long)batch * nrhs, hipMemcpyDeviceToHost, s));
      } else {
        for (long long q = 0; q < batch; q++)
          RC_TRY(copy(b->base[i] + q * st, rs, k.base[i] + q * len[i] * nrhs, len[i], len[i], nrhs,
                      hipMemcpyDeviceToHost, s));
      }
    }
    return FBSTAB_HIP_OK;
  }
};

// What a many-right-hand-side launch reads: the kernel-side arguments as multi_run staged them.
template <class Data>
struct MultiLaunchArgs {
  Data a;                          // problem arrays
  fbstab_var_batch_t v;            // point
  fbstab_multi_var_batch_t sd, st; // seeds (all null in the generated-seed modes), steps
  double* gain = nullptr;          // the extra per-QP output block (null: not asked for, or a kind without one)
  long long gain_stride = 0;
  int* d_st = nullptr;             // status
  int nrhs = 0;
  hipStream_t s = nullptr;
};

// ... and fbstab_hip_mpc_kkt_solve_batch / _x0_sensitivity_batch and fbstab_hip_dense_kkt_solve_batch /
// _jacobian_batch behind the checks that need no handle: the argument checks in the order all four have always made
// them, the staging of the arrays, the point, the seed and step blocks, `gain` (MPC's nu x nx per QP; null for
// dense) and the status, `launch(k)` - the counter block zeroed, the argument list, the timed launch - and the results
// back.  `sizes(&nrhs, &gain_len)` runs behind check_common and in front of every other check: the generated-seed
// modes (seed == nullptr) take nrhs from the handle there (and dense refuses wrt = h without equality constraints),
// MPC says how long a gain is.  A seed or step slot of a vector of length 0 is dropped, whatever it holds (dense
// handles with nl == 0; every length of an MPC handle is positive).  step == nullptr: no step is asked for (x0 mode).
template <class Handle, class Data, class Sizes, class Launch>
int multi_run(Handle h, int batch, const Data* data, const fbstab_var_batch_t* x, int nrhs,
              const fbstab_multi_var_batch_t* seed, const fbstab_multi_var_batch_t* step, double* gain,
              long long gain_stride, int* status, int flags, void* stream, Sizes sizes, Launch launch) {
  RC_TRY(check_common(h, batch, data, x, status, h ? h->max_batch : 0));
  long long glen = 0;
  RC_TRY(sizes(&nrhs, &glen));
  const long long* vlen = h->var_len;
  for (size_t i = 0; i < h->arr_len.size(); i++)  // (nl == 0: the G and h slots are empty)
    if (!data->base[i] && h->arr_len[i] > 0) return fail(FBSTAB_HIP_ERR_ARGUMENT, "null problem data pointer");
  for (int i = 0; i < 3; i++)
    if (!x->base[i] && vlen[i] > 0) return fail(FBSTAB_HIP_ERR_ARGUMENT, "null variable pointer");
  for (int i = 0; i < 3; i++) RC_TRY(h->check_var_stride(x->stride, i, batch));
  fbstab_multi_var_batch_t sd_in{}, st_in{};
  if (seed) sd_in = *seed;
  if (step) st_in = *step;
  for (int i = 0; i < 3; i++)
    if (vlen[i] == 0) sd_in.base[i] = st_in.base[i] = nullptr;
  RC_TRY(check_multi_strides(&sd_in, vlen, batch, nrhs, true));
  RC_TRY(check_multi_strides(&st_in, vlen, batch, nrhs, false));
  if (batch > 1 && gain && gain_stride < glen) return fail(FBSTAB_HIP_ERR_ARGUMENT, "gain stride smaller than nu x nx");
  RC_TRY(h->check_data_strides(data->stride, batch));
  if (batch == 0) return FBSTAB_HIP_OK;
  HIP_TRY(hipSetDevice(h->device));
  MultiLaunchArgs<Data> k;
  hipStream_t s = k.s = stream ? (hipStream_t)stream : h->stream;
  const bool dev_ptrs = (flags & FBSTAB_HIP_DEVICE_POINTERS) != 0;
  RC_TRY(h->stage_arrays(data->base, data->stride, batch, dev_ptrs, s, k.a.base, k.a.stride));
  RC_TRY(h->stage_vars(x->base, x->stride, 3, batch, dev_ptrs, s, &k.v));
  MultiStage sd, st;
  RC_TRY(sd.open(&sd_in, vlen, batch, nrhs, dev_ptrs, true, s));
  RC_TRY(st.open(&st_in, vlen, batch, nrhs, dev_ptrs, false, s));
  k.sd = sd.k;
  k.st = st.k;
  DevBuf d_gain, d_status;
  k.gain = gain;
  k.gain_stride = batch > 1 ? gain_stride : 0;
  if (gain && !dev_ptrs) {
    HIP_TRY(hipMalloc(&d_gain.p, sizeof(double) * (size_t)glen * batch));
    k.gain = static_cast<double*>(d_gain.p);
    k.gain_stride = glen;
  }
  k.d_st = status;
  const bool status_host = SolverBase::out_on_host(flags);
  if (status_host) {
    HIP_TRY(hipMalloc(&d_status.p, sizeof(int) * (size_t)batch));
    k.d_st = static_cast<int*>(d_status.p);
  }
  k.nrhs = nrhs;
  RC_TRY(launch(k));
  if (!dev_ptrs) {
    RC_TRY(st.download(&st_in, vlen, batch, nrhs, s));
    if (gain) RC_TRY(h->download(gain, gain_stride, glen, batch, k.gain, s));
  }
  if (status_host) HIP_TRY(hipMemcpyAsync(status, k.d_st, sizeof(int) * (size_t)batch, hipMemcpyDeviceToHost, s));
  if (status_host || !(flags & FBSTAB_HIP_ASYNC)) HIP_TRY(hipStreamSynchronize(s));
  return FBSTAB_HIP_OK;
}

}  // namespace
