// Host side of the condensed MPC route (include/fbstab_hip.h: fbstab_hip_mpc_condense_batch to
// fbstab_hip_mpc_condensed_receding_sweep_tangent): the argument checks, the blocks as the kernels take them, the
// callers' work arrays (fb_condense_plan.h) and the order of the launches.  As fb_host_stage.h: no device code and no
// kernel header.  What reaches a kernel or the dense handle is passed in by fbstab_hip.hip as a callable -
//   launch(id, grid, lds_bytes, args, stream)                                    kernel `id` of fb_condense_plan.h's enums
//   dense_solve(batch, dc, xc, out, stream)                                      fbstab_hip_dense_solve_batch
//   dense_adjoint(batch, dc, xc, seeds, sigma, adj, status, stream)              fbstab_hip_dense_adjoint_batch
//   dense_multi(batch, dc, xc, nrhs, seeds, sigma, step, status, stream)         fbstab_hip_dense_kkt_solve_batch
//   direction(N, nx, nu, nc, batch, dir, x, seeds, stream)                       the direction kernel of the forward mode
// (on the handle, device pointers, asynchronous) - so tests/test_condense_stage.py compiles this header with the host
// compiler over tests/hostsim/runtime_shim and runs it, host lambdas in their place, under the address sanitizer.
#pragma once

#include "fb_condense_plan.h"
#include "fb_host_stage.h"

namespace {

// ---- what the entry points share ------------------------------------------------------------------------------------
struct CondenseShape {
  int N, nx, nu, nc;
  long long len[FBSTAB_MPC_NSEQ];
  long long nz, nv;
};
// A refused argument (`who`: the entry point's name in front of its messages, here and below).
inline int condense_bad(const char* who, const char* what) {
  return fail(FBSTAB_HIP_ERR_ARGUMENT, std::string(who) + ": " + what);
}
// What both calls check before any device call: the sizes, the batch, the data block and its strides.
inline int condense_check(int N, int nx, int nu, int nc, int batch, const fbstab_mpc_batch_t* data, CondenseShape* sh) {
  if (N < 1 || nx < 1 || nu < 1 || nc < 1) return condense_bad("condense", "problem sizes must be positive");
  if (batch < 0) return condense_bad("condense", "negative batch");
  if (!data) return condense_bad("condense", "null problem data block");
  const long long n1 = N + 1;
  const long long len[FBSTAB_MPC_NSEQ] = {n1 * nx * nx, n1 * nu * nu, n1 * nu * nx, n1 * nx, n1 * nu,
                                          (long long)N * nx * nx, (long long)N * nx * nu, (long long)N * nx,
                                          n1 * nc * nx, n1 * nc * nu, n1 * nc, nx};
  *sh = CondenseShape{N, nx, nu, nc, {}, n1 * nu, n1 * nc};
  for (int i = 0; i < FBSTAB_MPC_NSEQ; i++) {
    sh->len[i] = len[i];
    if (!data->base[i]) return condense_bad("condense", "null problem data pointer");
    if (batch > 1 && data->stride[i] != 0 && data->stride[i] < len[i])
      return condense_bad("condense", "problem data stride smaller than the array length");
  }
  return FBSTAB_HIP_OK;
}
// ... and after it: the device ...
inline int condense_device_exists(const char* who, int device) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n < 1) return fail(FBSTAB_HIP_ERR_DEVICE, std::string(who) + ": no HIP device");
  if (device < 0 || device >= n) return fail(FBSTAB_HIP_ERR_DEVICE, std::string(who) + ": no such device");
  return FBSTAB_HIP_OK;
}
// ... then the LDS rule.  *lds: the dynamic LDS bytes of a launch.
inline int condense_device(const CondenseShape& sh, int device, CondenseLds* o, int* lds) {
  RC_TRY(condense_device_exists("condense", device));
  o->init(sh.N, sh.nx, sh.nu, sh.nc);
  if ((long long)o->total * 8 > kLdsLimitBytes)
    return fail(FBSTAB_HIP_ERR_UNSUPPORTED, "condense: the stage images and dx/du of a horizon do not fit the 160 KiB LDS budget");
  *lds = o->total * 8;
  HIP_TRY(hipSetDevice(device));
  return FBSTAB_HIP_OK;
}

// The launch of every kernel of the route: `kernel_of(id, &threads)` is the getter of the id's unit; a launch of more
// than 64 KiB of dynamic LDS raises the kernel's limit first.
template <class KernelOf, class Id>
int condense_launch(KernelOf kernel_of, Id id, int grid, long long lds, void** args, hipStream_t s) {
  int threads = 0;
  const void* kern = kernel_of(id, &threads);
  if (lds > 64 * 1024) HIP_TRY(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsLimitBytes));
  HIP_TRY(hipLaunchKernel(kern, dim3(grid), dim3(threads), args, (size_t)lds, s));
  return FBSTAB_HIP_OK;
}

// The condensed images H, f, A, b of a caller: no null pointer, with batch > 1 every QP its own (stride >= length) or,
// for the matrices alone, one image for the batch (stride 0).  *dc: the block as the kernels and the dense handle
// take it - with batch == 1 the caller's strides are not read.
inline int condense_check_images(const char* who, const CondenseShape& sh, int batch, const fbstab_dense_batch_t* dense,
                                 fbstab_dense_batch_t* dc) {
  const long long dlen[FBSTAB_DENSE_NARR] = {sh.nz * sh.nz, sh.nz, 0, 0, sh.nv * sh.nz, sh.nv};
  *dc = fbstab_dense_batch_t{};
  for (int i : {FBSTAB_DENSE_H, FBSTAB_DENSE_f, FBSTAB_DENSE_A, FBSTAB_DENSE_b}) {
    const bool matrix = i == FBSTAB_DENSE_H || i == FBSTAB_DENSE_A;
    if (!dense->base[i]) return condense_bad(who, "null pointer in the condensed images");
    if (batch > 1 && dense->stride[i] < dlen[i] && !(matrix && dense->stride[i] == 0))
      return condense_bad(who, "stride of a condensed image smaller than the array length");
    dc->base[i] = dense->base[i];
    dc->stride[i] = batch > 1 ? dense->stride[i] : dlen[i];
  }
  return FBSTAB_HIP_OK;
}

// The dense handle that serves the condensed QP, behind everything that needs no handle.
inline int condense_check_handle(const char* who, const SolverBase* h, const CondenseShape& sh, int batch) {
  if (!h) return condense_bad(who, "null dense solver handle");
  if (h->var_len[0] != sh.nz || h->var_len[1] != 0 || h->var_len[2] != sh.nv)
    return condense_bad(who, "the dense handle is not one of ((N + 1) nu, 0, (N + 1) nc)");
  if (batch > h->max_batch) return condense_bad(who, "batch exceeds the max_batch the handle was created with");
  return FBSTAB_HIP_OK;
}

// The plant of a sweep: one for the batch (stride 0) or every trajectory its own.
inline int condense_check_plant(const char* who, const fbstab_receding_plant_t* plant, int nx, int nu, int batch) {
  if (batch > 1 && ((plant->stride_A != 0 && plant->stride_A < (long long)nx * nx) ||
                    (plant->stride_B != 0 && plant->stride_B < (long long)nx * nu)))
    return condense_bad(who, "plant stride smaller than the matrix");
  return FBSTAB_HIP_OK;
}

// The affine map of a sweep in AFFINE mode (the other mode does not look at it).
inline int condense_check_map(const char* who, bool affine, const fbstab_condensed_map_t* map, const CondenseShape& sh,
                              int batch) {
  if (!affine) return FBSTAB_HIP_OK;
  if (!map) return condense_bad(who, "AFFINE mode needs the map");
  if (!map->M || !map->f0 || !map->b0) return condense_bad(who, "null pointer in the map");
  if (batch > 1 && ((map->stride_M != 0 && map->stride_M < (sh.nz + sh.nv) * sh.nx) ||
                    (map->stride_f0 != 0 && map->stride_f0 < sh.nz) || (map->stride_b0 != 0 && map->stride_b0 < sh.nv)))
    return condense_bad(who, "stride of the map smaller than the array length");
  return FBSTAB_HIP_OK;
}

// One model for the batch: stride 0 on every one of Q, R, S, A, B, E, L.
inline bool condense_shared_model(const fbstab_mpc_batch_t* data) {
  bool shared = true;
  for (int i : {FBSTAB_MPC_Q, FBSTAB_MPC_R, FBSTAB_MPC_S, FBSTAB_MPC_A, FBSTAB_MPC_B, FBSTAB_MPC_E, FBSTAB_MPC_L})
    shared = shared && data->stride[i] == 0;
  return shared;
}

// What every *_sizes function begins with: its outputs zeroed, positive sizes, the function's own arguments
// (`bad_arg`: null, or what is wrong with the first of them that is), condensed sizes that fit an int.
inline int condense_sizes_prologue(const char* who, int N, int nx, int nu, int nc, const char* bad_arg,
                                   std::initializer_list<int*> ints, std::initializer_list<long long*> longs) {
  for (int* p : ints)
    if (p) *p = 0;
  for (long long* p : longs)
    if (p) *p = 0;
  if (N < 1 || nx < 1 || nu < 1 || nc < 1) return condense_bad(who, "problem sizes must be positive");
  if (bad_arg) return fail(FBSTAB_HIP_ERR_ARGUMENT, std::string(who) + ": " + bad_arg);
  if ((long long)(N + 1) * nu > 0x7fffffff || (long long)(N + 1) * nc > 0x7fffffff)
    return fail(FBSTAB_HIP_ERR_UNSUPPORTED, "condense: the condensed sizes do not fit an int");
  return FBSTAB_HIP_OK;
}

// One dense adjoint step (dU, dv) of the seeds (gU, gv; gv null: zero) at the condensed point xc, refined once
// (fb_condense_adjoint.h): the dense adjoint, the residual kernel, the dense adjoint of (rU, 0) into (eU, ev), the
// correction kernel.  st1, st2: where the two dense launches report.
template <class Launch, class DenseAdjoint>
int condense_refined_step(Launch launch, DenseAdjoint dense_adjoint, const CondenseShape& sh, int batch,
                          const fbstab_dense_batch_t& dc, const fbstab_var_batch_t& xc, double* gv, double sigma,
                          CondenseAdjointWork& wk, int* st1, int* st2, hipStream_t s) {
  fbstab_var_batch_t sc = {}, ac = {};
  sc.base[0] = wk.gU; sc.stride[0] = sh.nz;
  sc.base[2] = gv; sc.stride[2] = sh.nv;
  ac.base[0] = wk.dU; ac.stride[0] = sh.nz;
  ac.base[2] = wk.dv; ac.stride[2] = sh.nv;
  RC_TRY(dense_adjoint(batch, &dc, &xc, &sc, sigma, &ac, st1, s));
  int nzc = (int)sh.nz, nvc = (int)sh.nv;
  const double *Hc = dc.base[FBSTAB_DENSE_H], *Ac = dc.base[FBSTAB_DENSE_A];
  long long sH = dc.stride[FBSTAB_DENSE_H], sA = dc.stride[FBSTAB_DENSE_A];
  double sg = sigma_or_default(sigma);  // (the rule of fbstab_hip_dense_adjoint_batch)
  void* rargs[] = {&nzc, &nvc, &Hc, &sH, &Ac, &sA, &sg, &wk};
  RC_TRY(launch(kCondenseAdjResidual, batch, 0, rargs, s));
  sc.base[0] = wk.rU;
  sc.base[2] = nullptr;
  ac.base[0] = wk.eU;
  ac.base[2] = wk.ev;
  RC_TRY(dense_adjoint(batch, &dc, &xc, &sc, sigma, &ac, st2, s));
  void* cargs[] = {&nzc, &nvc, &wk};
  return launch(kCondenseAdjCorrect, batch, 0, cargs, s);
}

// ---- condensing (fb_condense.h) -----------------------------------------------------------------------------------
inline int condensed_sizes(int N, int nx, int nu, int nc, int* nz, int* nv, long long* lds_bytes) {
  RC_TRY(condense_sizes_prologue("condense", N, nx, nu, nc, nullptr, {nz, nv}, {lds_bytes}));
  if (nz) *nz = (N + 1) * nu;
  if (nv) *nv = (N + 1) * nc;
  CondenseLds o;
  o.init(N, nx, nu, nc);
  if ((long long)o.total * 8 > kLdsLimitBytes)
    return fail(FBSTAB_HIP_ERR_UNSUPPORTED, "condense: the stage images and dx/du of a horizon do not fit the 160 KiB LDS budget");
  if (lds_bytes) *lds_bytes = (long long)o.total * 8;
  return FBSTAB_HIP_OK;
}

template <class Launch>
int condense_run(int N, int nx, int nu, int nc, int batch, const fbstab_mpc_batch_t* data, int what,
                 const fbstab_dense_out_batch_t* dense, int device, void* stream, Launch launch) {
  CondenseShape sh;
  RC_TRY(condense_check(N, nx, nu, nc, batch, data, &sh));
  if (what < FBSTAB_CONDENSE_MATRICES || what > FBSTAB_CONDENSE_ALL)
    return condense_bad("condense", "`what` must be MATRICES (1), VECTORS (2) or ALL (3)");
  if (!dense) return condense_bad("condense", "null output block");
  const bool mats = (what & FBSTAB_CONDENSE_MATRICES) != 0, vecs = (what & FBSTAB_CONDENSE_VECTORS) != 0;
  const bool shared_model = condense_shared_model(data);
  const long long olen[FBSTAB_DENSE_NARR] = {sh.nz * sh.nz, sh.nz, 0, 0, sh.nv * sh.nz, sh.nv};
  fbstab_dense_out_batch_t out = {};
  for (int i : {FBSTAB_DENSE_H, FBSTAB_DENSE_f, FBSTAB_DENSE_A, FBSTAB_DENSE_b}) {
    const bool matrix = i == FBSTAB_DENSE_H || i == FBSTAB_DENSE_A;
    if (matrix ? !mats : !vecs) continue;
    if (!dense->base[i]) return condense_bad("condense", "null pointer in a selected output slot");
    if (batch > 1 && dense->stride[i] < olen[i]) {
      if (!matrix || dense->stride[i] != 0)
        return condense_bad("condense", "output stride smaller than the array length");
      if (!shared_model)
        return condense_bad("condense", "output stride 0 needs stride 0 on every one of Q, R, S, A, B, E, L");
    }
    out.base[i] = dense->base[i];
    out.stride[i] = batch > 1 ? dense->stride[i] : olen[i];
  }
  if (batch == 0) return FBSTAB_HIP_OK;
  CondenseLds o;
  int lds = 0;
  RC_TRY(condense_device(sh, device, &o, &lds));
  hipStream_t s = (hipStream_t)stream;
  fbstab_mpc_batch_t a = *data;
  void* args[] = {&N, &nx, &nu, &nc, &o, &a, &out};
  if (mats) {
    // (one image of each for a batch that shares its model: QP 0 alone is launched)
    const bool one = out.stride[FBSTAB_DENSE_H] == 0 && out.stride[FBSTAB_DENSE_A] == 0;
    RC_TRY(launch(kCondenseMatrices, (one ? 1 : batch) * (N + 1), lds, args, s));
  }
  if (vecs) RC_TRY(launch(kCondenseVectors, batch, lds, args, s));
  return FBSTAB_HIP_OK;
}

template <class Launch>
int expand_run(int N, int nx, int nu, int nc, int batch, const fbstab_mpc_batch_t* data, const fbstab_var_batch_t* xc,
               const fbstab_var_batch_t* x, int device, void* stream, Launch launch) {
  CondenseShape sh;
  RC_TRY(condense_check(N, nx, nu, nc, batch, data, &sh));
  if (!xc || !x) return condense_bad("expand", "null variable block");
  if (!xc->base[0] || !xc->base[2]) return condense_bad("expand", "null U or v pointer");
  if (x->base[3] && !xc->base[3]) return condense_bad("expand", "y is wanted and the condensed y is null");
  const long long clen[4] = {sh.nz, 0, sh.nv, sh.nv};
  const long long xlen[4] = {(long long)(N + 1) * (nx + nu), (long long)(N + 1) * nx, sh.nv, sh.nv};
  fbstab_var_batch_t in = {}, outv = {};
  for (int i = 0; i < 4; i++) {
    if (i != 1 && xc->base[i]) {
      if (batch > 1 && xc->stride[i] < clen[i])
        return condense_bad("expand", "stride of the condensed point smaller than the vector length");
      in.base[i] = xc->base[i];
      in.stride[i] = batch > 1 ? xc->stride[i] : clen[i];
    }
    if (x->base[i]) {
      if (batch > 1 && x->stride[i] < xlen[i])
        return condense_bad("expand", "variable stride smaller than the vector length");
      outv.base[i] = x->base[i];
      outv.stride[i] = batch > 1 ? x->stride[i] : xlen[i];
    }
  }
  if (batch == 0) return FBSTAB_HIP_OK;
  CondenseLds o;
  int lds = 0;
  RC_TRY(condense_device(sh, device, &o, &lds));
  fbstab_mpc_batch_t a = *data;
  void* args[] = {&N, &nx, &nu, &nc, &o, &a, &in, &outv};
  return launch(kCondenseExpand, batch, lds, args, (hipStream_t)stream);
}

// ---- reverse mode (fb_condense_adjoint.h) ---------------------------------------------------------------------------
// The seed kernel, the refined dense adjoint step on the condensed QP, the finish kernel - six launches on one stream.
// condensed_adjoint_queue is those six behind every check, on the blocks as the kernels take them (xv, sd, ad: the
// point, the seeds, and where the step goes - null slots skipped); the forward mode below queues them as well.
template <class Launch, class DenseAdjoint>
int condensed_adjoint_queue(const CondenseShape& sh, int batch, CondenseLds o, int lds, fbstab_mpc_batch_t a,
                            const fbstab_dense_batch_t& dc, fbstab_var_batch_t xv, fbstab_var_batch_t sd, double sigma,
                            fbstab_mpc_grad_batch_t g, fbstab_var_batch_t ad, CondenseAdjointWork wk, int* status,
                            hipStream_t s, Launch launch, DenseAdjoint dense_adjoint) {
  int N = sh.N, nx = sh.nx, nu = sh.nu, nc = sh.nc;
  {
    void* args[] = {&N, &nx, &nu, &nc, &o, &a, &xv, &sd, &wk};
    RC_TRY(launch(kCondenseAdjSeed, batch, lds, args, s));
  }
  // the dense adjoint at (U, v): no gradients of the condensed data
  fbstab_var_batch_t xc = {};
  xc.base[0] = wk.U; xc.stride[0] = sh.nz;
  xc.base[2] = xv.base[2]; xc.stride[2] = xv.stride[2];
  RC_TRY(condense_refined_step(launch, dense_adjoint, sh, batch, dc, xc, wk.gv, sigma, wk, status, status, s));
  const int* st = status;
  void* args[] = {&N, &nx, &nu, &nc, &o, &a, &xv, &sd, &wk, &g, &ad, &st};
  return launch(kCondenseAdjFinish, batch, lds, args, s);
}

template <class Launch, class DenseAdjoint>
int condensed_adjoint_run(SolverBase* h, int N, int nx, int nu, int nc, int batch, const fbstab_mpc_batch_t* data,
                          const fbstab_dense_batch_t* dense, const fbstab_var_batch_t* x,
                          const fbstab_var_batch_t* seed, double sigma, const fbstab_mpc_grad_batch_t* grad,
                          const fbstab_var_batch_t* adj, double* work, int* status, void* stream, Launch launch,
                          DenseAdjoint dense_adjoint) {
  // what needs no handle comes first, in the order of fbstab_hip_mpc_condense_batch
  CondenseShape sh;
  RC_TRY(condense_check(N, nx, nu, nc, batch, data, &sh));
  if (!dense || !x || !seed || !grad || !work || !status) return condense_bad("condensed adjoint", "null argument");
  fbstab_dense_batch_t dc;
  RC_TRY(condense_check_images("condensed adjoint", sh, batch, dense, &dc));
  const long long xlen[3] = {(long long)(N + 1) * (nx + nu), (long long)(N + 1) * nx, sh.nv};
  if (!seed->base[0]) return condense_bad("condensed adjoint", "null seed pointer (z)");
  for (int i = 0; i < 3; i++) {
    if (!x->base[i]) return condense_bad("condensed adjoint", "null variable pointer");
    if (batch > 1 && x->stride[i] < xlen[i])
      return condense_bad("condensed adjoint", "variable stride smaller than the vector length");
    if (batch > 1 && seed->base[i] && seed->stride[i] < xlen[i])
      return condense_bad("condensed adjoint", "seed stride smaller than the vector length");
    if (batch > 1 && adj && adj->base[i] && adj->stride[i] < xlen[i])
      return condense_bad("condensed adjoint", "adjoint stride smaller than the vector length");
  }
  for (int i = 0; i < FBSTAB_MPC_NSEQ; i++)
    if (batch > 1 && grad->base[i] && grad->stride[i] < sh.len[i])
      return condense_bad("condensed adjoint", "gradient stride smaller than the array length");
  // ... then the handle
  RC_TRY(condense_check_handle("condensed adjoint", h, sh, batch));
  if (batch == 0) return FBSTAB_HIP_OK;
  CondenseLds o;
  int lds = 0;
  RC_TRY(condense_device(sh, h->device, &o, &lds));
  hipStream_t s = stream ? (hipStream_t)stream : h->stream;
  // the blocks as the kernels take them: with batch == 1 the strides are not read by the caller's rule
  fbstab_var_batch_t xv = {}, sd = {}, ad = {};
  for (int i = 0; i < 3; i++) {
    xv.base[i] = x->base[i]; xv.stride[i] = batch > 1 ? x->stride[i] : xlen[i];
    sd.base[i] = seed->base[i]; sd.stride[i] = batch > 1 ? seed->stride[i] : xlen[i];
    if (adj) { ad.base[i] = adj->base[i]; ad.stride[i] = batch > 1 ? adj->stride[i] : xlen[i]; }
  }
  CondenseAdjointWork wk = CondenseAdjointCarve(sh.nz, sh.nv, work, batch).wk;
  return condensed_adjoint_queue(sh, batch, o, lds, *data, dc, xv, sd, sigma, *grad, ad, wk, status, s, launch,
                                 dense_adjoint);
}

// ---- forward mode (fb_tangent.h's direction on this route's blocks, then the adjoint's launches) ----------------------
// `direction(N, nx, nu, nc, batch, dir, x, seeds, stream)`: the direction kernel of fb_condense_tangent.hip on the grid
// batch x (N + 1), behind its own two refusals (its LDS layout is a kernel header's: this header does not see it).
// Seven launches on one stream: the direction, then condensed_adjoint_queue on the seeds it wrote, no gradient slot,
// adj = dx.
template <class Launch, class DenseAdjoint, class Direction>
int condensed_tangent_run(SolverBase* h, int N, int nx, int nu, int nc, int batch, const fbstab_mpc_batch_t* data,
                          const fbstab_dense_batch_t* dense, const fbstab_var_batch_t* x,
                          const fbstab_mpc_batch_t* ddata, double sigma, const fbstab_var_batch_t* dx,
                          const fbstab_var_batch_t* rhs, double* work, int* status, void* stream, Launch launch,
                          DenseAdjoint dense_adjoint, Direction direction) {
  // what needs no handle comes first, in the order of fbstab_hip_mpc_condense_batch
  CondenseShape sh = {};
  RC_TRY(condense_check(N, nx, nu, nc, batch, data, &sh));
  if (!dense || !x || !ddata || !dx || !work || !status) return condense_bad("condensed tangent", "null argument");
  fbstab_dense_batch_t dc;
  RC_TRY(condense_check_images("condensed tangent", sh, batch, dense, &dc));
  const long long xlen[3] = {(long long)(N + 1) * (nx + nu), (long long)(N + 1) * nx, sh.nv};
  for (int i = 0; i < 3; i++) {
    if (!x->base[i]) return condense_bad("condensed tangent", "null variable pointer");
    if (batch > 1 && x->stride[i] < xlen[i])
      return condense_bad("condensed tangent", "variable stride smaller than the vector length");
    if (!dx->base[i]) return condense_bad("condensed tangent", "null tangent pointer (dx)");
    if (batch > 1 && dx->stride[i] < xlen[i])
      return condense_bad("condensed tangent", "tangent stride smaller than the vector length");
    if (rhs && !rhs->base[i]) return condense_bad("condensed tangent", "null right-hand side pointer (rhs)");
    if (batch > 1 && rhs && rhs->stride[i] < xlen[i])
      return condense_bad("condensed tangent", "right-hand side stride smaller than the vector length");
  }
  for (int i = 0; i < FBSTAB_MPC_NSEQ; i++)
    if (batch > 1 && ddata->base[i] && ddata->stride[i] != 0 && ddata->stride[i] < sh.len[i])
      return condense_bad("condensed tangent", "perturbation stride is neither 0 nor at least the array length");
  // ... then the handle
  RC_TRY(condense_check_handle("condensed tangent", h, sh, batch));
  if (batch == 0) return FBSTAB_HIP_OK;
  CondenseLds o;
  int lds = 0;
  RC_TRY(condense_device(sh, h->device, &o, &lds));
  hipStream_t s = stream ? (hipStream_t)stream : h->stream;
  // the blocks as the kernels take them: with batch == 1 the strides are not read by the caller's rule; the seeds in
  // the caller's rhs, or in the tail of the work array (which is not addressed where rhs is given)
  const CondenseTangentCarve wk(sh.nz, sh.nv, xlen[0], xlen[1], work, batch);
  double* const tail[3] = {wk.gz, wk.gl, wk.gv};
  fbstab_mpc_batch_t dir = {};
  for (int i = 0; i < FBSTAB_MPC_NSEQ; i++) {
    if (!ddata->base[i]) continue;
    dir.base[i] = ddata->base[i];
    dir.stride[i] = batch > 1 ? ddata->stride[i] : sh.len[i];
  }
  fbstab_var_batch_t xv = {}, sd = {}, ad = {};
  for (int i = 0; i < 3; i++) {
    xv.base[i] = x->base[i]; xv.stride[i] = batch > 1 ? x->stride[i] : xlen[i];
    ad.base[i] = dx->base[i]; ad.stride[i] = batch > 1 ? dx->stride[i] : xlen[i];
    sd.base[i] = rhs ? rhs->base[i] : tail[i];
    sd.stride[i] = rhs && batch > 1 ? rhs->stride[i] : xlen[i];
  }
  RC_TRY(direction(N, nx, nu, nc, batch, dir, xv, sd, s));
  return condensed_adjoint_queue(sh, batch, o, lds, *data, dc, xv, sd, sigma, fbstab_mpc_grad_batch_t{}, ad, wk.wk,
                                 status, s, launch, dense_adjoint);
}

// ---- many right-hand sides (fb_condense_multi.h) ----------------------------------------------------------------------
struct CondenseMultiPlan {
  CondenseLds o;
  int R;
  long long per, lds_bytes, work;
};
// What fbstab_hip_mpc_condensed_multi_sizes documents, behind its argument checks.
inline int condense_multi_plan(int N, int nx, int nu, int nc, int nrhs, int rhs_per_group, CondenseMultiPlan* p) {
  p->o.init(N, nx, nu, nc);
  if (p->o.total == 0x3fffffff || (long long)p->o.carry * 8 > kLdsLimitBytes)
    return fail(FBSTAB_HIP_ERR_UNSUPPORTED, "condensed multi: the stage images do not fit the 160 KiB LDS budget");
  p->per = condense_multi_per(N, nx, nu, nc);
  p->R = rhs_per_group > 0 ? (rhs_per_group < nrhs ? rhs_per_group : nrhs)
                           : condense_multi_rule(nx, nrhs, p->o.carry, p->per);
  p->lds_bytes = 8 * ((long long)p->o.carry + p->R * p->per);
  if (p->lds_bytes > kLdsLimitBytes)
    return fail(FBSTAB_HIP_ERR_UNSUPPORTED,
                "condensed multi: the stage images and rhs_per_group copies of a right-hand side's vectors do not fit the 160 KiB LDS budget");
  p->work = CondenseMultiCarve((long long)(N + 1) * nu, (long long)(N + 1) * nc, nrhs, nullptr, 0).per;
  return FBSTAB_HIP_OK;
}

inline int condensed_multi_sizes(int N, int nx, int nu, int nc, int nrhs, int rhs_per_group, int* rhs_per_group_used,
                                 long long* lds_bytes, long long* work_doubles_per_qp) {
  const char* bad = nrhs < 1 ? "fewer than one right-hand side" : rhs_per_group < 0 ? "negative rhs_per_group" : nullptr;
  RC_TRY(condense_sizes_prologue("condensed multi", N, nx, nu, nc, bad, {rhs_per_group_used},
                                 {lds_bytes, work_doubles_per_qp}));
  CondenseMultiPlan pl;
  RC_TRY(condense_multi_plan(N, nx, nu, nc, nrhs, rhs_per_group, &pl));
  if (rhs_per_group_used) *rhs_per_group_used = pl.R;
  if (lds_bytes) *lds_bytes = pl.lds_bytes;
  if (work_doubles_per_qp) *work_doubles_per_qp = pl.work;
  return FBSTAB_HIP_OK;
}

// Both entry points: fbstab_hip_mpc_condensed_kkt_solve_batch, and with x0_mode the _x0_sensitivity_batch (nrhs = nx, no
// seed block: the seeds are generated in the kernels; step may be null there, and gain - null, or nu x nx per QP - is
// served there only).  (The refined step is condense_refined_step's sequence on the multi kernels and the dense
// multi-solve, with other argument lists.)
template <class Launch, class DenseMulti>
int condensed_multi_run(SolverBase* h, int N, int nx, int nu, int nc, int batch, const fbstab_mpc_batch_t* data,
                        const fbstab_dense_batch_t* dense, const fbstab_var_batch_t* x, bool x0_mode, int nrhs,
                        const fbstab_multi_var_batch_t* seed, double sigma, const fbstab_multi_var_batch_t* step,
                        double* gain, long long gain_stride, int rhs_per_group, double* work, int* status,
                        void* stream, Launch launch, DenseMulti dense_multi) {
  // what needs no handle comes first, in the order of fbstab_hip_mpc_condense_batch, then that of
  // fbstab_hip_mpc_kkt_solve_batch
  CondenseShape sh;
  RC_TRY(condense_check(N, nx, nu, nc, batch, data, &sh));
  if (x0_mode) {
    if (!step && !gain) return condense_bad("condensed x0 sensitivity", "both step and gain are null");
  } else {
    if (nrhs < 1) return condense_bad("condensed kkt solve", "fewer than one right-hand side");
    if (!seed || !step) return condense_bad("condensed kkt solve", "null seed or step block");
    if (!seed->base[0]) return condense_bad("condensed kkt solve", "null seed pointer (z)");
  }
  if (!dense || !x || !work || !status) return condense_bad("condensed multi", "null argument");
  fbstab_dense_batch_t dc;
  RC_TRY(condense_check_images("condensed multi", sh, batch, dense, &dc));
  const long long xlen[3] = {(long long)(N + 1) * (nx + nu), (long long)(N + 1) * nx, sh.nv};
  for (int i = 0; i < 3; i++) {
    if (!x->base[i]) return condense_bad("condensed multi", "null variable pointer");
    if (batch > 1 && x->stride[i] < xlen[i])
      return condense_bad("condensed multi", "variable stride smaller than the vector length");
  }
  if (seed) RC_TRY(check_multi_strides(seed, xlen, batch, nrhs, true));
  if (step) RC_TRY(check_multi_strides(step, xlen, batch, nrhs, false));
  const long long glen = (long long)nu * nx;
  if (batch > 1 && gain && gain_stride < glen)
    return condense_bad("condensed multi", "gain stride smaller than nu x nx");
  if (rhs_per_group < 0) return condense_bad("condensed multi", "negative rhs_per_group");
  // ... then the handle
  RC_TRY(condense_check_handle("condensed multi", h, sh, batch));
  if (batch == 0) return FBSTAB_HIP_OK;
  // ... the device, then the LDS rule
  RC_TRY(condense_device_exists("condensed multi", h->device));
  CondenseMultiPlan pl;
  RC_TRY(condense_multi_plan(N, nx, nu, nc, nrhs, rhs_per_group, &pl));
  const long long groups = (nrhs + pl.R - 1) / pl.R;
  if (groups * batch > 0x7fffffffLL)
    return condense_bad("condensed multi", "batch x groups of right-hand sides exceeds the grid limit");
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t s = stream ? (hipStream_t)stream : h->stream;
  // the blocks as the kernels take them: with batch == 1 or nrhs == 1 the strides are not read by the caller's rule
  fbstab_mpc_batch_t a = *data;
  fbstab_var_batch_t xv = {};
  fbstab_multi_var_batch_t sd = {}, st = {};
  for (int i = 0; i < 3; i++) {
    xv.base[i] = x->base[i]; xv.stride[i] = batch > 1 ? x->stride[i] : xlen[i];
    for (int which = 0; which < 2; which++) {
      const fbstab_multi_var_batch_t* b = which ? step : seed;
      fbstab_multi_var_batch_t& k = which ? st : sd;
      if (!b || !b->base[i]) continue;
      k.base[i] = b->base[i];
      k.rhs_stride[i] = nrhs > 1 ? b->rhs_stride[i] : xlen[i];
      k.stride[i] = batch > 1 ? b->stride[i] : (nrhs - 1) * k.rhs_stride[i] + xlen[i];
    }
  }
  CondenseMultiWork wk = CondenseMultiCarve(sh.nz, sh.nv, nrhs, work, batch).wk;
  const int grid = (int)(groups * batch);
  int R = pl.R, x0m = x0_mode ? 1 : 0;
  long long per = pl.per;
  {
    void* args[] = {&N, &nx, &nu, &nc, &pl.o, &nrhs, &R, &per, &x0m, &a, &xv, &sd, &wk};
    RC_TRY(launch(kCondenseMultiSeed, grid, pl.lds_bytes, args, s));
  }
  {
    // the dense multi-solve at (U, v): first the seeds (gU, gv_c), step = (dU, dv); then, behind the residual kernel,
    // the seeds (rU, 0), step = (eU, ev), which the correction kernel adds.
    fbstab_var_batch_t xc = {};
    xc.base[0] = wk.U; xc.stride[0] = sh.nz;
    xc.base[2] = xv.base[2]; xc.stride[2] = xv.stride[2];
    fbstab_multi_var_batch_t sc = {}, ac = {};
    sc.base[0] = wk.gU; sc.stride[0] = sh.nz * nrhs; sc.rhs_stride[0] = sh.nz;
    sc.base[2] = wk.gv; sc.stride[2] = sh.nv * nrhs; sc.rhs_stride[2] = sh.nv;
    ac.base[0] = wk.dU; ac.stride[0] = sh.nz * nrhs; ac.rhs_stride[0] = sh.nz;
    ac.base[2] = wk.dv; ac.stride[2] = sh.nv * nrhs; ac.rhs_stride[2] = sh.nv;
    RC_TRY(dense_multi(batch, &dc, &xc, nrhs, &sc, sigma, &ac, status, s));
    int nzc = (int)sh.nz, nvc = (int)sh.nv;
    const double *Hc = dc.base[FBSTAB_DENSE_H], *Ac = dc.base[FBSTAB_DENSE_A];
    long long sH = dc.stride[FBSTAB_DENSE_H], sA = dc.stride[FBSTAB_DENSE_A];
    double sg = sigma_or_default(sigma);  // (the rule of fbstab_hip_dense_kkt_solve_batch)
    void* rargs[] = {&nzc, &nvc, &nrhs, &R, &Hc, &sH, &Ac, &sA, &sg, &wk};
    RC_TRY(launch(kCondenseMultiResidual, grid, 0, rargs, s));
    sc.base[0] = wk.rU;
    sc.base[2] = nullptr;
    ac.base[0] = wk.eU;
    ac.base[2] = wk.ev;
    RC_TRY(dense_multi(batch, &dc, &xc, nrhs, &sc, sigma, &ac, status, s));
    long long gs = batch > 1 ? gain_stride : glen;
    const int* stq = status;
    void* cargs[] = {&nzc, &nvc, &nu, &nrhs, &R, &wk, &gain, &gs, &stq};
    RC_TRY(launch(kCondenseMultiCorrect, grid, 0, cargs, s));
  }
  if (!step) return FBSTAB_HIP_OK;  // (gain alone: the finish launch is not queued)
  const int* stq = status;
  void* args[] = {&N, &nx, &nu, &nc, &pl.o, &nrhs, &R, &per, &x0m, &a, &sd, &wk, &st, &stq};
  return launch(kCondenseMultiFinish, grid, pl.lds_bytes, args, s);
}

// ---- per-step references (fb_condense_refs.h) -------------------------------------------------------------------------
struct CondenseRefsPlan {
  CondenseLds o;
  int R;
  long long per, lds_bytes;
};
// What fbstab_hip_mpc_condensed_reference_sizes documents, behind its argument checks: the rule for R is
// condense_multi_rule's on the references of one trajectory.
inline int condense_refs_plan(int N, int nx, int nu, int nc, int steps, int refs_per_group, CondenseRefsPlan* p) {
  p->o.init(N, nx, nu, nc);
  if (p->o.total == 0x3fffffff || (long long)p->o.carry * 8 > kLdsLimitBytes)
    return fail(FBSTAB_HIP_ERR_UNSUPPORTED, "condensed references: the stage images do not fit the 160 KiB LDS budget");
  p->per = condense_refs_per(N, nx);
  p->R = refs_per_group > 0 ? (refs_per_group < steps ? refs_per_group : steps)
                            : condense_multi_rule(nx, steps, p->o.carry, p->per);
  p->lds_bytes = 8 * ((long long)p->o.carry + p->R * p->per);
  if (p->lds_bytes > kLdsLimitBytes)
    return fail(FBSTAB_HIP_ERR_UNSUPPORTED,
                "condensed references: the stage images and refs_per_group copies of a reference's vectors do not fit the 160 KiB LDS budget");
  return FBSTAB_HIP_OK;
}

inline int condensed_reference_sizes(int N, int nx, int nu, int nc, int steps, int refs_per_group,
                                     int* refs_per_group_used, long long* lds_bytes) {
  const char* bad = steps < 1 ? "fewer than one step" : refs_per_group < 0 ? "negative refs_per_group" : nullptr;
  RC_TRY(condense_sizes_prologue("condensed references", N, nx, nu, nc, bad, {refs_per_group_used}, {lds_bytes}));
  CondenseRefsPlan pl;
  RC_TRY(condense_refs_plan(N, nx, nu, nc, steps, refs_per_group, &pl));
  if (refs_per_group_used) *refs_per_group_used = pl.R;
  if (lds_bytes) *lds_bytes = pl.lds_bytes;
  return FBSTAB_HIP_OK;
}

// The slots of fbstab_condensed_refs_t in fbstab_mpc_batch_t.
constexpr int kCondenseRefSeq[4] = {FBSTAB_MPC_q, FBSTAB_MPC_r, FBSTAB_MPC_c, FBSTAB_MPC_d};

// The references of a caller (null: every sequence is `data`'s at every step): no negative step or stride, with
// batch > 1 every trajectory its own rows (stride >= length) or one for all (0).  *rr: the block without a null slot -
// where the caller gave no sequence, `data`'s with step 0 - and, with batch == 1, without the caller's strides.
inline int condense_check_refs(const char* who, const CondenseShape& sh, int batch, const fbstab_mpc_batch_t* data,
                               const fbstab_condensed_refs_t* refs, fbstab_condensed_refs_t* rr) {
  *rr = fbstab_condensed_refs_t{};
  for (int i = 0; i < 4; i++) {
    const int seq = kCondenseRefSeq[i];
    if (!refs || !refs->base[i]) {
      rr->base[i] = data->base[seq];
      rr->stride[i] = batch > 1 ? data->stride[seq] : 0;
      continue;
    }
    if (refs->step[i] < 0) return condense_bad(who, "negative step in the references");
    if (refs->stride[i] < 0) return condense_bad(who, "negative stride in the references");
    if (batch > 1 && refs->stride[i] != 0 && refs->stride[i] < sh.len[seq])
      return condense_bad(who, "trajectory stride of a reference is neither 0 nor at least the sequence length");
    rr->base[i] = refs->base[i];
    rr->step[i] = refs->step[i];
    rr->stride[i] = batch > 1 ? refs->stride[i] : 0;
  }
  return FBSTAB_HIP_OK;
}

// `data` with the sequences of step k of the (checked) references in the place of q, r, c, d.
inline fbstab_mpc_batch_t condense_data_at_step(fbstab_mpc_batch_t a, const fbstab_condensed_refs_t& rr, long long k) {
  for (int i = 0; i < 4; i++) {
    a.base[kCondenseRefSeq[i]] = rr.base[i] + k * rr.step[i];
    a.stride[kCondenseRefSeq[i]] = rr.stride[i];
  }
  return a;
}

// The images f0_k, b0_k of a caller that a sweep READS (writing: condensed_reference_images_run's own check).
inline int condense_check_ref_images(const char* who, const CondenseShape& sh, int batch,
                                     const fbstab_condensed_ref_images_t* images) {
  if (!images) return condense_bad(who, "AFFINE mode with references needs their images");
  if (!images->f0 || !images->b0) return condense_bad(who, "null pointer in the reference images");
  if (images->step_f0 < 0 || images->step_b0 < 0) return condense_bad(who, "negative step in the reference images");
  if (batch > 1 && ((images->stride_f0 != 0 && images->stride_f0 < sh.nz) ||
                    (images->stride_b0 != 0 && images->stride_b0 < sh.nv)))
    return condense_bad(who, "trajectory stride of the reference images is neither 0 nor at least the length");
  return FBSTAB_HIP_OK;
}

// What both tracking calls check behind the map, in front of the handle: the map (with references in AFFINE mode M
// alone is looked at: f0 and b0 are the references' images), the references, their images.
inline int condense_check_tracking(const char* who, bool affine, const fbstab_condensed_map_t* map,
                                   const CondenseShape& sh, int batch, const fbstab_mpc_batch_t* data,
                                   const fbstab_condensed_refs_t* refs, const fbstab_condensed_ref_images_t* images,
                                   fbstab_condensed_refs_t* rr) {
  *rr = fbstab_condensed_refs_t{};
  if (!refs) return condense_check_map(who, affine, map, sh, batch);
  if (affine) {
    if (!map || !map->M) return condense_bad(who, "AFFINE mode needs the map");
    if (batch > 1 && map->stride_M != 0 && map->stride_M < (sh.nz + sh.nv) * sh.nx)
      return condense_bad(who, "stride of the map smaller than the array length");
  }
  RC_TRY(condense_check_refs(who, sh, batch, data, refs, rr));
  if (affine) RC_TRY(condense_check_ref_images(who, sh, batch, images));
  return FBSTAB_HIP_OK;
}

// fbstab_hip_mpc_condensed_reference_images_batch: one launch on the grid batch x ceil(steps / R).
template <class Launch>
int condensed_reference_images_run(int N, int nx, int nu, int nc, int batch, int steps, const fbstab_mpc_batch_t* data,
                                   const fbstab_condensed_refs_t* refs, const fbstab_condensed_ref_images_t* images,
                                   int refs_per_group, int device, void* stream, Launch launch) {
  CondenseShape sh;
  RC_TRY(condense_check(N, nx, nu, nc, batch, data, &sh));
  if (steps < 0) return condense_bad("condensed references", "negative step count");
  if (refs_per_group < 0) return condense_bad("condensed references", "negative refs_per_group");
  fbstab_condensed_refs_t rr;
  RC_TRY(condense_check_refs("condensed references", sh, batch, data, refs, &rr));
  if (!images || !images->f0 || !images->b0) return condense_bad("condensed references", "null output pointer");
  // every (step, trajectory) writes rows of its own
  if (steps > 1 && (images->step_f0 < sh.nz || images->step_b0 < sh.nv))
    return condense_bad("condensed references", "output step smaller than the image");
  if (batch > 1 && (images->stride_f0 < sh.nz || images->stride_b0 < sh.nv))
    return condense_bad("condensed references", "output stride smaller than the image");
  if (batch == 0 || steps == 0) return FBSTAB_HIP_OK;
  // ... the device, then the LDS rule
  RC_TRY(condense_device_exists("condensed references", device));
  CondenseRefsPlan pl;
  RC_TRY(condense_refs_plan(N, nx, nu, nc, steps, refs_per_group, &pl));
  const long long groups = (steps + pl.R - 1) / pl.R;
  if (groups * batch > 0x7fffffffLL)
    return condense_bad("condensed references", "batch x groups of steps exceeds the grid limit");
  HIP_TRY(hipSetDevice(device));
  // the blocks as the kernel takes them: with batch == 1 or steps == 1 the caller's strides and steps are not read
  fbstab_mpc_batch_t a = *data;
  fbstab_condensed_ref_images_t im = *images;
  if (batch == 1) im.stride_f0 = im.stride_b0 = 0;
  if (steps == 1) {
    im.step_f0 = im.step_b0 = 0;
    for (int i = 0; i < 4; i++) rr.step[i] = 0;
  }
  int R = pl.R;
  long long per = pl.per;
  void* args[] = {&N, &nx, &nu, &nc, &pl.o, &steps, &R, &per, &a, &rr, &im};
  return launch(kCondenseRefsImages, (int)(groups * batch), pl.lds_bytes, args, (hipStream_t)stream);
}

// ---- the condensed route in closed loop (fb_condense_sweep.h) ---------------------------------------------------------
// What fbstab_hip_mpc_condensed_sweep_sizes documents, behind its argument checks.
inline int condense_sweep_plan(int N, int nx, int nu, int nc, int traj_per_group, bool stage_m, CondenseSweepLds* L) {
  L->init(N, nx, nu, nc, traj_per_group, stage_m);
  if ((long long)L->total * 8 > kLdsLimitBytes)
    return fail(FBSTAB_HIP_ERR_UNSUPPORTED,
                "condensed sweep: traj_per_group copies of a trajectory's vectors do not fit the 160 KiB LDS budget");
  return FBSTAB_HIP_OK;
}

// The *_sizes functions of the sweep (work_grad == nullptr) and of its adjoint: `work` without, `work_grad` with the
// finish kernel.
inline int condensed_sweep_sizes(const char* who, int N, int nx, int nu, int nc, int traj_per_group, int shared_map,
                                 int* traj_per_group_used, long long* lds_bytes, long long* work, long long* work_grad,
                                 bool adjoint) {
  RC_TRY(condense_sizes_prologue(who, N, nx, nu, nc, traj_per_group < 0 ? "negative traj_per_group" : nullptr,
                                 {traj_per_group_used}, {lds_bytes, work, work_grad}));
  CondenseSweepLds L;
  RC_TRY(condense_sweep_plan(N, nx, nu, nc, traj_per_group, shared_map != 0, &L));
  if (traj_per_group_used) *traj_per_group_used = L.T;
  if (lds_bytes) *lds_bytes = (long long)L.total * 8;
  const long long nz = (long long)(N + 1) * nu, nv = (long long)(N + 1) * nc;
  if (work) *work = adjoint ? CondenseSweepAdjCarve(N, nx, nu, nc, false, nullptr, 0).per
                            : CondenseSweepCarve(nz, nv, nx, nullptr, 0).per;
  if (work_grad) *work_grad = CondenseSweepAdjCarve(N, nx, nu, nc, true, nullptr, 0).per;
  return FBSTAB_HIP_OK;
}

template <class Launch>
int condensed_x0_map_run(int N, int nx, int nu, int nc, int batch, const fbstab_mpc_batch_t* data, double* map,
                         long long map_stride, int device, void* stream, Launch launch) {
  CondenseShape sh;
  RC_TRY(condense_check(N, nx, nu, nc, batch, data, &sh));
  if (!map) return condense_bad("condensed x0 map", "null output pointer");
  const long long len = (sh.nz + sh.nv) * nx;
  if (batch > 1 && map_stride < len) {
    if (map_stride != 0) return condense_bad("condensed x0 map", "output stride smaller than the image");
    if (!condense_shared_model(data))
      return condense_bad("condensed x0 map", "output stride 0 needs stride 0 on every one of Q, R, S, A, B, E, L");
  }
  if (batch == 0) return FBSTAB_HIP_OK;
  CondenseLds o;
  int lds = 0;
  RC_TRY(condense_device(sh, device, &o, &lds));
  fbstab_mpc_batch_t a = *data;
  long long ms = batch > 1 ? map_stride : len;
  const int blocks = (nx + nu - 1) / nu;
  if ((long long)batch * blocks > 0x7fffffff)
    return condense_bad("condensed x0 map", "batch x column blocks exceeds the grid limit");
  void* args[] = {&N, &nx, &nu, &nc, &o, &a, &map, &ms};
  return launch(kCondenseSweepX0Map, (ms == 0 ? 1 : batch) * blocks, lds, args, (hipStream_t)stream);
}

// Both sweeps: fbstab_hip_mpc_condensed_receding_sweep (refs == nullptr: `images` is not looked at) and
// fbstab_hip_mpc_condensed_tracking_sweep, where step k is the QP of the references' step k - per-step pointers into
// the references and their images, the launches and their order are the same.
template <class Launch, class DenseSolve>
int condensed_tracking_sweep_run(SolverBase* h, int N, int nx, int nu, int nc, int batch,
                                 const fbstab_mpc_batch_t* data, const fbstab_dense_batch_t* dense,
                                 const fbstab_condensed_map_t* map, const fbstab_var_batch_t* x,
                                 fbstab_solver_out_t* out, const fbstab_receding_plant_t* plant, int steps, int retire,
                                 const fbstab_sweep_scenario_t* scenario, int mode,
                                 const fbstab_condensed_sweep_log_t* log, const fbstab_condensed_refs_t* refs,
                                 const fbstab_condensed_ref_images_t* images, int traj_per_group, double* work,
                                 void* stream, Launch launch, DenseSolve dense_solve) {
  // what needs no handle comes first, in the order of fbstab_hip_mpc_condense_batch
  CondenseShape sh;
  RC_TRY(condense_check(N, nx, nu, nc, batch, data, &sh));
  if (!dense || !x || !out || !plant || !work) return condense_bad("condensed sweep", "null argument");
  if (!plant->A || !plant->B) return condense_bad("condensed sweep", "null plant matrix");
  if (steps < 0) return condense_bad("condensed sweep", "negative step count");
  if (scenario && scenario->shift != 0 && scenario->shift != 1)
    return condense_bad("condensed sweep", "shift is 0 or 1");
  if (mode != FBSTAB_CONDENSED_SWEEP_AFFINE && mode != FBSTAB_CONDENSED_SWEEP_RECONDENSE)
    return condense_bad("condensed sweep", "`mode` must be AFFINE (0) or RECONDENSE (1)");
  if (traj_per_group < 0) return condense_bad("condensed sweep", "negative traj_per_group");
  if (batch > 1 && data->stride[FBSTAB_MPC_x0] < nx)
    return condense_bad("condensed sweep", "every trajectory needs its own x0 (stride >= nx)");
  fbstab_dense_batch_t dc;
  RC_TRY(condense_check_images("condensed sweep", sh, batch, dense, &dc));
  const long long xlen[4] = {(long long)(N + 1) * (nx + nu), (long long)(N + 1) * nx, sh.nv, sh.nv};
  for (int i = 0; i < 4; i++) {
    if (!x->base[i]) return condense_bad("condensed sweep", "null variable pointer");
    if (batch > 1 && x->stride[i] < xlen[i])
      return condense_bad("condensed sweep", "variable stride smaller than the vector length");
  }
  RC_TRY(condense_check_plant("condensed sweep", plant, nx, nu, batch));
  const bool affine = mode == FBSTAB_CONDENSED_SWEEP_AFFINE;
  // ... the map and the references, in front of the handle
  fbstab_condensed_refs_t rr;
  RC_TRY(condense_check_tracking("condensed sweep", affine, map, sh, batch, data, refs, images, &rr));
  // ... then the handle
  RC_TRY(condense_check_handle("condensed sweep", h, sh, batch));
  if (batch == 0 || steps == 0) return FBSTAB_HIP_OK;
  CondenseLds o;
  int lds = 0;
  RC_TRY(condense_device(sh, h->device, &o, &lds));
  const bool shared_m = affine && (batch == 1 || map->stride_M == 0);
  CondenseSweepLds L;
  RC_TRY(condense_sweep_plan(N, nx, nu, nc, traj_per_group, shared_m, &L));
  if (L.T > batch) L.init(N, nx, nu, nc, batch, shared_m);
  hipStream_t s = stream ? (hipStream_t)stream : h->stream;
  const bool one = batch == 1;
  // the work arrays, and the blocks as the kernels take them (with batch == 1 the caller's strides are not read)
  CondenseSweepCarve wk(sh.nz, sh.nv, nx, work, batch);
  fbstab_mpc_batch_t a = *data;
  fbstab_var_batch_t xv = {};
  for (int i = 0; i < 4; i++) { xv.base[i] = x->base[i]; xv.stride[i] = one ? xlen[i] : x->stride[i]; }
  fbstab_dense_out_batch_t dvec = {};  // (the VECTORS launch of RECONDENSE mode writes f and b)
  for (int i : {FBSTAB_DENSE_f, FBSTAB_DENSE_b}) {
    dvec.base[i] = const_cast<double*>(dc.base[i]);
    dvec.stride[i] = dc.stride[i];
  }
  fbstab_var_batch_t xc = {};
  xc.base[0] = wk.U; xc.stride[0] = sh.nz;
  xc.base[2] = wk.v; xc.stride[2] = sh.nv;
  xc.base[3] = wk.y; xc.stride[3] = sh.nv;
  {
    void* args[] = {&N, &nx, &nu, &nc, &xv, &wk.U, &wk.v, &wk.gone};
    RC_TRY(launch(kCondenseSweepBegin, batch, 0, args, s));
  }
  CondenseSweepStep st = {};
  st.N = N; st.nx = nx; st.nu = nu; st.nc = nc; st.batch = batch;
  st.retire = retire != 0;
  st.out = out; st.gone = wk.gone; st.U = wk.U; st.v = wk.v;
  st.x0 = const_cast<double*>(data->base[FBSTAB_MPC_x0]);
  st.sx0 = one ? nx : data->stride[FBSTAB_MPC_x0];
  st.Ap = plant->A; st.Bp = plant->B;
  st.sAp = one ? 0 : plant->stride_A; st.sBp = one ? 0 : plant->stride_B;
  if (affine) {
    st.M = map->M; st.sM = one ? 0 : map->stride_M;
    if (refs) {
      st.sf0 = one ? 0 : images->stride_f0;
      st.sb0 = one ? 0 : images->stride_b0;
    } else {
      st.f0 = map->f0; st.sf0 = one ? 0 : map->stride_f0;
      st.b0 = map->b0; st.sb0 = one ? 0 : map->stride_b0;
    }
  }
  st.f = dvec.base[FBSTAB_DENSE_f]; st.sf = dvec.stride[FBSTAB_DENSE_f];
  st.b = dvec.base[FBSTAB_DENSE_b]; st.sb = dvec.stride[FBSTAB_DENSE_b];
  const bool shift = scenario && scenario->shift == 1;
  const double* w = scenario ? scenario->w : nullptr;
  const int groups = (batch + L.T - 1) / L.T;
  for (int k = 0; k < steps; k++) {
    const bool last = k + 1 == steps;
    RC_TRY(dense_solve(batch, &dc, &xc, out, s));
    const long long kb = (long long)k * batch;
    st.shift = shift && !last;
    st.affine = affine && !last;
    st.xkeep = last ? wk.xkeep : nullptr;
    st.w = w ? w + kb * nx : nullptr;
    st.u_log = log && log->u ? log->u + kb * nu : nullptr;
    st.x_log = log && log->x ? log->x + kb * nx : nullptr;
    st.U_log = log && log->U ? log->U + kb * sh.nz : nullptr;
    st.v_log = log && log->v ? log->v + kb * sh.nv : nullptr;
    st.eflag_log = log && log->eflag ? log->eflag + kb : nullptr;
    st.newton_log = log && log->newton ? log->newton + kb : nullptr;
    if (refs && affine && !last) {  // the vectors of step k + 1 from the images of step k + 1
      st.f0 = images->f0 + (k + 1) * images->step_f0;
      st.b0 = images->b0 + (k + 1) * images->step_b0;
    }
    void* sargs[] = {&st, &L};
    RC_TRY(launch(kCondenseSweepStep, groups, L.total * 8, sargs, s));
    if (!affine && !last) {
      fbstab_mpc_batch_t an = refs ? condense_data_at_step(a, rr, k + 1) : a;
      void* vargs[] = {&N, &nx, &nu, &nc, &o, &an, &dvec};
      RC_TRY(launch(kCondenseVectors, batch, lds, vargs, s));
    }
  }
  // the point of the last step, at the state it was solved for
  fbstab_mpc_batch_t al = refs ? condense_data_at_step(a, rr, steps - 1) : a;
  al.base[FBSTAB_MPC_x0] = wk.xkeep;
  al.stride[FBSTAB_MPC_x0] = nx;
  void* eargs[] = {&N, &nx, &nu, &nc, &o, &al, &xc, &xv};
  return launch(kCondenseExpand, batch, lds, eargs, s);
}

template <class Launch, class DenseSolve>
int condensed_sweep_run(SolverBase* h, int N, int nx, int nu, int nc, int batch, const fbstab_mpc_batch_t* data,
                        const fbstab_dense_batch_t* dense, const fbstab_condensed_map_t* map,
                        const fbstab_var_batch_t* x, fbstab_solver_out_t* out, const fbstab_receding_plant_t* plant,
                        int steps, int retire, const fbstab_sweep_scenario_t* scenario, int mode,
                        const fbstab_condensed_sweep_log_t* log, int traj_per_group, double* work, void* stream,
                        Launch launch, DenseSolve dense_solve) {
  return condensed_tracking_sweep_run(h, N, nx, nu, nc, batch, data, dense, map, x, out, plant, steps, retire, scenario,
                                      mode, log, nullptr, nullptr, traj_per_group, work, stream, launch, dense_solve);
}

// ---- reverse mode through that sweep (fb_condense_sweep_adjoint.h) --------------------------------------------------
// Both adjoints: fbstab_hip_mpc_condensed_receding_sweep_adjoint (refs == nullptr: `images` and `ref_grad` are not
// looked at) and fbstab_hip_mpc_condensed_tracking_sweep_adjoint (gf0 == gb0 == nullptr), where every launch of step k
// is handed the pointers of step k: the images f0[k], b0[k] or the VECTORS launch's q, r, c, d, the finish kernel's data
// block, and for a sequence that moves its gradient's rows of step k (zeroed by one begin launch per step in front of
// the recursion, so that a step the finish kernel leaves alone holds zeros).
template <class Launch, class DenseAdjoint>
int condensed_tracking_sweep_adjoint_run(SolverBase* h, int N, int nx, int nu, int nc, int batch,
                                         const fbstab_mpc_batch_t* data, const fbstab_dense_batch_t* dense,
                                         const fbstab_condensed_map_t* map, const fbstab_receding_plant_t* plant,
                                         int steps, const fbstab_condensed_sweep_log_t* log, const double* gu,
                                         const double* gx, double sigma, const fbstab_mpc_grad_batch_t* grad,
                                         double* gf0, double* gb0, double* mu_log, int* status, int mode,
                                         const fbstab_condensed_refs_t* refs,
                                         const fbstab_condensed_ref_images_t* images,
                                         const fbstab_condensed_ref_grad_t* ref_grad, int traj_per_group, double* work,
                                         void* stream, Launch launch, DenseAdjoint dense_adjoint) {
  // what needs no handle comes first, in the order of fbstab_hip_mpc_condensed_receding_sweep
  CondenseShape sh;
  RC_TRY(condense_check(N, nx, nu, nc, batch, data, &sh));
  if (!dense || !plant || !log || !grad || !status || !work)
    return condense_bad("condensed sweep adjoint", "null argument");
  if (!plant->A || !plant->B) return condense_bad("condensed sweep adjoint", "null plant matrix");
  if (steps < 0) return condense_bad("condensed sweep adjoint", "negative step count");
  if (mode != FBSTAB_CONDENSED_SWEEP_AFFINE && mode != FBSTAB_CONDENSED_SWEEP_RECONDENSE)
    return condense_bad("condensed sweep adjoint", "`mode` must be AFFINE (0) or RECONDENSE (1)");
  if (traj_per_group < 0) return condense_bad("condensed sweep adjoint", "negative traj_per_group");
  fbstab_dense_batch_t dc;
  RC_TRY(condense_check_images("condensed sweep adjoint", sh, batch, dense, &dc));
  RC_TRY(condense_check_plant("condensed sweep adjoint", plant, nx, nu, batch));
  if (!log->x || !log->U || !log->v || !log->eflag)
    return condense_bad("condensed sweep adjoint", "the x, U, v and eflag logs are required");
  bool data_grads = false;
  for (int i = 0; i < FBSTAB_MPC_NSEQ; i++) {
    if (!grad->base[i]) continue;
    if (batch > 1 && grad->stride[i] < sh.len[i])
      return condense_bad("condensed sweep adjoint", "gradient stride smaller than the array length (sums over the batch are the caller's)");
    if (i != FBSTAB_MPC_x0) data_grads = true;
  }
  const bool affine = mode == FBSTAB_CONDENSED_SWEEP_AFFINE;
  // ... the map and the references, in front of the handle
  fbstab_condensed_refs_t rr;
  RC_TRY(condense_check_tracking("condensed sweep adjoint", affine, map, sh, batch, data, refs, images, &rr));
  fbstab_condensed_ref_grad_t rg = {};
  if (refs)
    for (int i = 0; i < 4; i++) {
      const int seq = kCondenseRefSeq[i];
      const bool moves = refs->base[i] != nullptr;
      if (moves && grad->base[seq])
        return condense_bad("condensed sweep adjoint", "the summed gradient slot of a sequence that moves (its gradient is per step: ref_grad)");
      if (!ref_grad || !ref_grad->base[i]) continue;
      if (!moves)
        return condense_bad("condensed sweep adjoint", "per-step gradient of a sequence that does not move (its gradient is the summed slot of grad)");
      if ((steps > 1 && ref_grad->step[i] < sh.len[seq]) || (batch > 1 && ref_grad->stride[i] < sh.len[seq]))
        return condense_bad("condensed sweep adjoint", "every step and trajectory needs its own rows of a per-step gradient (step, stride >= length)");
      rg.base[i] = ref_grad->base[i];
      rg.step[i] = steps > 1 ? ref_grad->step[i] : 0;
      rg.stride[i] = batch > 1 ? ref_grad->stride[i] : sh.len[seq];
      data_grads = true;
    }
  // ... then the handle
  RC_TRY(condense_check_handle("condensed sweep adjoint", h, sh, batch));
  if (batch == 0) return FBSTAB_HIP_OK;
  CondenseLds o;
  int lds = 0;
  RC_TRY(condense_device(sh, h->device, &o, &lds));
  const bool shared_m = affine && (batch == 1 || map->stride_M == 0);
  CondenseSweepLds L;
  RC_TRY(condense_sweep_plan(N, nx, nu, nc, traj_per_group, shared_m, &L));
  if (L.T > batch) L.init(N, nx, nu, nc, batch, shared_m);
  hipStream_t s = stream ? (hipStream_t)stream : h->stream;
  const bool one = batch == 1;
  const bool finish = data_grads || !affine;
  CondenseSweepAdjCarve wk(N, nx, nu, nc, finish, work, batch);
  fbstab_mpc_grad_batch_t g = *grad;
  if (one)
    for (int i = 0; i < FBSTAB_MPC_NSEQ; i++) g.stride[i] = sh.len[i];
  {
    void* args[] = {&N, &nx, &nu, &nc, &g, &wk.gz, &gf0, &gb0, &status};
    RC_TRY(launch(kCondenseSweepAdjBegin, batch, 0, args, s));
  }
  // the rows of step k of the per-step gradients, as a gradient block (null where none is wanted)
  const auto ref_rows = [&rg](fbstab_mpc_grad_batch_t* to, long long k) {
    bool any = false;
    for (int i = 0; i < 4; i++) {
      if (!rg.base[i]) continue;
      to->base[kCondenseRefSeq[i]] = rg.base[i] + k * rg.step[i];
      to->stride[kCondenseRefSeq[i]] = rg.stride[i];
      any = true;
    }
    return any;
  };
  for (int k = 0; k < steps; k++) {  // (status is zeroed once more: nothing has counted yet)
    fbstab_mpc_grad_batch_t gk = {};
    if (!ref_rows(&gk, k)) break;
    double* none = nullptr;
    void* args[] = {&N, &nx, &nu, &nc, &gk, &none, &none, &none, &status};
    RC_TRY(launch(kCondenseSweepAdjBegin, batch, 0, args, s));
  }
  if (steps == 0) return FBSTAB_HIP_OK;
  fbstab_mpc_batch_t a = *data;
  a.stride[FBSTAB_MPC_x0] = nx;
  fbstab_dense_out_batch_t dvec = {};
  for (int i : {FBSTAB_DENSE_f, FBSTAB_DENSE_b}) {
    dvec.base[i] = const_cast<double*>(dc.base[i]);
    dvec.stride[i] = dc.stride[i];
  }
  CondenseSweepAdjStep st = {};
  st.N = N; st.nx = nx; st.nu = nu; st.nc = nc; st.batch = batch;
  st.affine = affine;
  st.st1 = wk.st1; st.st2 = wk.st2; st.status = status;
  st.dU = wk.wk.dU; st.dv = wk.wk.dv;
  st.dl0 = affine ? nullptr : wk.dl0;
  st.mu = wk.mu;
  st.Ap = plant->A; st.Bp = plant->B;
  st.sAp = one ? 0 : plant->stride_A; st.sBp = one ? 0 : plant->stride_B;
  st.gU = wk.wk.gU;
  if (affine) {
    st.M = map->M; st.sM = one ? 0 : map->stride_M;
    if (refs) {
      st.sf0 = one ? 0 : images->stride_f0;
      st.sb0 = one ? 0 : images->stride_b0;
    } else {
      st.f0 = map->f0; st.sf0 = one ? 0 : map->stride_f0;
      st.b0 = map->b0; st.sb0 = one ? 0 : map->stride_b0;
    }
  }
  st.f = dvec.base[FBSTAB_DENSE_f]; st.sf = dvec.stride[FBSTAB_DENSE_f];
  st.b = dvec.base[FBSTAB_DENSE_b]; st.sb = dvec.stride[FBSTAB_DENSE_b];
  st.gf0 = gf0; st.gb0 = gb0;
  st.gx0 = g.base[FBSTAB_MPC_x0]; st.sgx0 = g.stride[FBSTAB_MPC_x0];
  fbstab_mpc_grad_batch_t gfin = g;
  gfin.base[FBSTAB_MPC_x0] = nullptr;
  CondenseSweepAdjFinish fin = {};
  fin.dU = wk.wk.dU; fin.dv = wk.wk.dv; fin.st1 = wk.st1; fin.st2 = wk.st2;
  fin.z = wk.z; fin.l = wk.l; fin.gz = wk.gz; fin.dl0 = st.dl0;
  const int groups = (batch + L.T - 1) / L.T;
  for (int k = steps - 1; k >= -1; k--) {
    const long long kb = (long long)k * batch;
    st.close = k + 1 < steps;
    st.open = k >= 0;
    st.eflag_close = st.close ? log->eflag + kb + batch : nullptr;
    st.eflag_open = st.open ? log->eflag + kb : nullptr;
    st.gu = st.open && gu ? gu + kb * nu : nullptr;
    st.gx = st.open && gx ? gx + kb * nx : nullptr;
    st.mu_log = st.open && mu_log ? mu_log + kb * nx : nullptr;
    st.x_log = st.open ? log->x + kb * nx : nullptr;
    if (refs && affine && st.open) {  // opening step k: the images of step k
      st.f0 = images->f0 + k * images->step_f0;
      st.b0 = images->b0 + k * images->step_b0;
    }
    void* sargs[] = {&st, &L};
    RC_TRY(launch(kCondenseSweepAdjStep, groups, L.total * 8, sargs, s));
    if (k < 0) break;
    if (refs) {  // step k's sequences, for the VECTORS launch and the finish kernel
      const fbstab_mpc_batch_t ak = condense_data_at_step(a, rr, k);
      for (int i = 0; i < 4; i++) {
        a.base[kCondenseRefSeq[i]] = ak.base[kCondenseRefSeq[i]];
        a.stride[kCondenseRefSeq[i]] = ak.stride[kCondenseRefSeq[i]];
      }
      ref_rows(&gfin, k);
    }
    if (!affine) {
      a.base[FBSTAB_MPC_x0] = log->x + kb * nx;
      void* vargs[] = {&N, &nx, &nu, &nc, &o, &a, &dvec};
      RC_TRY(launch(kCondenseVectors, batch, lds, vargs, s));
    }
    // the dense adjoint at the logged (U_k, v_k), read where they lie, and one step of refinement of its step
    fbstab_var_batch_t xc = {};
    xc.base[0] = log->U + kb * sh.nz; xc.stride[0] = sh.nz;
    xc.base[2] = log->v + kb * sh.nv; xc.stride[2] = sh.nv;
    RC_TRY(condense_refined_step(launch, dense_adjoint, sh, batch, dc, xc, nullptr, sigma, wk.wk, wk.st1, wk.st2, s));
    if (finish) {
      fin.x = log->x + kb * nx;
      fin.U = log->U + kb * sh.nz;
      fin.v = log->v + kb * sh.nv;
      fin.eflag = log->eflag + kb;
      void* fargs[] = {&N, &nx, &nu, &nc, &o, &a, &fin, &gfin};
      RC_TRY(launch(kCondenseSweepAdjFinish, batch, lds, fargs, s));
    }
  }
  return FBSTAB_HIP_OK;
}

template <class Launch, class DenseAdjoint>
int condensed_sweep_adjoint_run(SolverBase* h, int N, int nx, int nu, int nc, int batch, const fbstab_mpc_batch_t* data,
                                const fbstab_dense_batch_t* dense, const fbstab_condensed_map_t* map,
                                const fbstab_receding_plant_t* plant, int steps,
                                const fbstab_condensed_sweep_log_t* log, const double* gu, const double* gx,
                                double sigma, const fbstab_mpc_grad_batch_t* grad, double* gf0, double* gb0,
                                double* mu_log, int* status, int mode, int traj_per_group, double* work, void* stream,
                                Launch launch, DenseAdjoint dense_adjoint) {
  return condensed_tracking_sweep_adjoint_run(h, N, nx, nu, nc, batch, data, dense, map, plant, steps, log, gu, gx,
                                              sigma, grad, gf0, gb0, mu_log, status, mode, nullptr, nullptr, nullptr,
                                              traj_per_group, work, stream, launch, dense_adjoint);
}

// ---- forward mode through that sweep (fb_condense_sweep_tangent.h) ---------------------------------------------------
// What fbstab_hip_mpc_condensed_sweep_tangent_sizes documents.
inline int condensed_sweep_tangent_sizes(int N, int nx, int nu, int nc, int traj_per_group, int shared_map,
                                         int* traj_per_group_used, long long* lds_bytes, long long* work) {
  RC_TRY(condense_sizes_prologue("condensed sweep tangent", N, nx, nu, nc,
                                 traj_per_group < 0 ? "negative traj_per_group" : nullptr, {traj_per_group_used},
                                 {lds_bytes, work}));
  CondenseSweepLds L;
  RC_TRY(condense_sweep_plan(N, nx, nu, nc, traj_per_group, shared_map != 0, &L));
  if (traj_per_group_used) *traj_per_group_used = L.T;
  if (lds_bytes) *lds_bytes = (long long)L.total * 8;
  if (work) *work = CondenseSweepTanCarve(N, nx, nu, nc, nullptr, 0).per;
  return FBSTAB_HIP_OK;
}

// fbstab_hip_mpc_condensed_receding_sweep_tangent: steps + 1 launches of the step kernel - the first only opens step
// 0, the last only closes step steps - 1 - and between two of them condense_refined_step at the logged (U_k, v_k) on
// the seeds the launch in front wrote.  Every launch is handed the pointers of the step it closes (dw[k], du[k], dx[k])
// and of the step it opens (x_log, the images f0, b0 and their directions).  AFFINE mode always: there is no `data`.
template <class Launch, class DenseAdjoint>
int condensed_sweep_tangent_run(SolverBase* h, int N, int nx, int nu, int nc, int batch,
                                const fbstab_dense_batch_t* dense, const fbstab_condensed_map_t* map,
                                const fbstab_condensed_ref_images_t* images, const fbstab_receding_plant_t* plant,
                                int steps, const fbstab_condensed_sweep_log_t* log,
                                const fbstab_condensed_sweep_dir_t* dir, double sigma, double* du, double* dx,
                                int* status, int traj_per_group, double* work, void* stream, Launch launch,
                                DenseAdjoint dense_adjoint) {
  const char* who = "condensed sweep tangent";
  // what needs no handle comes first, in the order of fbstab_hip_mpc_condensed_receding_sweep_adjoint
  if (N < 1 || nx < 1 || nu < 1 || nc < 1) return condense_bad(who, "problem sizes must be positive");
  if (batch < 0) return condense_bad(who, "negative batch");
  if (!dense || !plant || !log || !dir || !status || !work) return condense_bad(who, "null argument");
  if (!du && !dx) return condense_bad(who, "both du and dx are null");
  if (!plant->A || !plant->B) return condense_bad(who, "null plant matrix");
  if (steps < 0) return condense_bad(who, "negative step count");
  if (traj_per_group < 0) return condense_bad(who, "negative traj_per_group");
  CondenseShape sh = {};
  sh.N = N; sh.nx = nx; sh.nu = nu; sh.nc = nc;
  sh.nz = (long long)(N + 1) * nu; sh.nv = (long long)(N + 1) * nc;
  fbstab_dense_batch_t dc;
  RC_TRY(condense_check_images(who, sh, batch, dense, &dc));
  RC_TRY(condense_check_plant(who, plant, nx, nu, batch));
  if (!log->x || !log->U || !log->v || !log->eflag) return condense_bad(who, "the x, U, v and eflag logs are required");
  // the directions: a step below 0, or with batch > 1 a stride below the length that is not 0
  if (dir->step_df0 < 0 || dir->step_db0 < 0) return condense_bad(who, "negative step in the directions");
  if (batch > 1 && ((dir->dx0 && dir->stride_dx0 != 0 && dir->stride_dx0 < nx) ||
                    (dir->df0 && dir->stride_df0 != 0 && dir->stride_df0 < sh.nz) ||
                    (dir->db0 && dir->stride_db0 != 0 && dir->stride_db0 < sh.nv)))
    return condense_bad(who, "trajectory stride of a direction is neither 0 nor at least the length");
  // ... the map and the images, in front of the handle (with images M alone is looked at)
  if (images) {
    if (!map || !map->M) return condense_bad(who, "AFFINE mode needs the map");
    if (batch > 1 && map->stride_M != 0 && map->stride_M < (sh.nz + sh.nv) * sh.nx)
      return condense_bad(who, "stride of the map smaller than the array length");
    RC_TRY(condense_check_ref_images(who, sh, batch, images));
  } else {
    RC_TRY(condense_check_map(who, true, map, sh, batch));
  }
  // ... then the handle
  RC_TRY(condense_check_handle(who, h, sh, batch));
  if (batch == 0) return FBSTAB_HIP_OK;
  RC_TRY(condense_device_exists(who, h->device));
  const bool shared_m = batch == 1 || map->stride_M == 0;
  CondenseSweepLds L;
  RC_TRY(condense_sweep_plan(N, nx, nu, nc, traj_per_group, shared_m, &L));
  if (L.T > batch) L.init(N, nx, nu, nc, batch, shared_m);
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t s = stream ? (hipStream_t)stream : h->stream;
  const bool one = batch == 1;
  CondenseSweepTanCarve wk(N, nx, nu, nc, work, batch);
  CondenseSweepTanStep st = {};
  st.N = N; st.nx = nx; st.nu = nu; st.nc = nc; st.batch = batch;
  st.st1 = wk.st1; st.st2 = wk.st2; st.status = status;
  st.dU = wk.wk.dU; st.dx = wk.dx;
  st.dx0 = dir->dx0; st.sdx0 = one ? 0 : dir->stride_dx0;
  st.Ap = plant->A; st.Bp = plant->B;
  st.sAp = one ? 0 : plant->stride_A; st.sBp = one ? 0 : plant->stride_B;
  st.M = map->M; st.sM = one ? 0 : map->stride_M;
  if (images) {
    st.sf0 = one ? 0 : images->stride_f0;
    st.sb0 = one ? 0 : images->stride_b0;
  } else {
    st.f0 = map->f0; st.sf0 = one ? 0 : map->stride_f0;
    st.b0 = map->b0; st.sb0 = one ? 0 : map->stride_b0;
  }
  st.f = const_cast<double*>(dc.base[FBSTAB_DENSE_f]); st.sf = dc.stride[FBSTAB_DENSE_f];
  st.b = const_cast<double*>(dc.base[FBSTAB_DENSE_b]); st.sb = dc.stride[FBSTAB_DENSE_b];
  st.sdf0 = one ? 0 : dir->stride_df0;
  st.sdb0 = one ? 0 : dir->stride_db0;
  st.gU = wk.wk.gU; st.gv = wk.wk.gv;
  const int groups = (batch + L.T - 1) / L.T;
  for (int k = -1; k < steps; k++) {  // the launch that closes step k and opens step k + 1
    const long long kb = (long long)k * batch, kn = (long long)(k + 1) * batch;
    st.close = k >= 0;
    st.open = k + 1 < steps;
    st.eflag_close = st.close ? log->eflag + kb : nullptr;
    st.dw = st.close && dir->dw ? dir->dw + kb * nx : nullptr;
    st.du_out = st.close && du ? du + kb * nu : nullptr;
    st.dx_out = st.close && dx ? dx + kb * nx : nullptr;
    st.eflag_open = st.open ? log->eflag + kn : nullptr;
    st.x_log = st.open ? log->x + kn * nx : nullptr;
    if (images && st.open) {
      st.f0 = images->f0 + (k + 1) * images->step_f0;
      st.b0 = images->b0 + (k + 1) * images->step_b0;
    }
    st.df0 = st.open && dir->df0 ? dir->df0 + (k + 1) * dir->step_df0 : nullptr;
    st.db0 = st.open && dir->db0 ? dir->db0 + (k + 1) * dir->step_db0 : nullptr;
    void* sargs[] = {&st, &L};
    RC_TRY(launch(kCondenseSweepTanStep, groups, L.total * 8, sargs, s));
    if (!st.open) break;
    // the dense adjoint at the logged (U, v) of the opened step, read where they lie, refined once
    fbstab_var_batch_t xc = {};
    xc.base[0] = log->U + kn * sh.nz; xc.stride[0] = sh.nz;
    xc.base[2] = log->v + kn * sh.nv; xc.stride[2] = sh.nv;
    RC_TRY(condense_refined_step(launch, dense_adjoint, sh, batch, dc, xc, wk.wk.gv, sigma, wk.wk, wk.st1, wk.st2, s));
  }
  return FBSTAB_HIP_OK;
}

}  // namespace
