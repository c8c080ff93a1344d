/*
 * C-ABI of the MI355X-native batched FBstab solver (libfbstab_hip.so).
 *
 * This is the drop-in boundary for the reference's inner-loop path: one call
 * solves a whole batch of QPs with the FBstab algorithm running entirely on
 * the GPU (one QP per workgroup).  Each entry point names the reference
 * interface it stands in for (paths relative to dliaomcp/fbstab):
 *
 *   fbstab_hip_mpc_create / _destroy    FBstabMpc::FBstabMpc(N,nx,nu,nc) / dtor
 *                                       fbstab/fbstab_mpc.h:165, fbstab_mpc.cc:61-89
 *   fbstab_hip_mpc_set_options          FBstabMpc::UpdateOptions, fbstab_mpc.h:202,
 *                                       fbstab_mpc.cc:96-100 (-> UpdateParameters +
 *                                       ValidateOptions, fbstab_algorithm-impl.h:307-332)
 *   fbstab_hip_mpc_solve_batch          FBstabMpc::Solve(qp, &x), fbstab_mpc.h:181-195
 *                                       (batch == 1 with host pointers is exactly one
 *                                       reference Solve call)
 *   fbstab_hip_mpc_solve_batch_final    the same Solve at Display::FINAL, the reference's default
 *                                       level: the batch kernels, then the |rz| |rl| |rv| and
 *                                       tolerance of the summary block PrintFinal prints
 *                                       (fbstab_algorithm-impl.h:493-541)
 *   fbstab_hip_mpc_solve_traced         the same Solve with Display::ITER / ITER_DETAILED:
 *                                       the numbers of PrintIterLine, PrintDetailedHeader/
 *                                       Line/Footer and PrintFinal
 *                                       (fbstab_algorithm-impl.h:411-541) as records
 *   fbstab_hip_dense_create / _destroy  FBstabDense::FBstabDense(nz,nl,nv),
 *                                       fbstab/fbstab_dense.h:122, fbstab_dense.cc:18-42
 *   fbstab_hip_dense_set_options        FBstabDense::UpdateOptions, fbstab_dense.h:158
 *   fbstab_hip_dense_solve_batch        FBstabDense::Solve(qp, &x), fbstab_dense.h:136-149
 *   fbstab_hip_dense_solve_traced       as fbstab_hip_mpc_solve_traced
 *
 * Data layout is the reference's: every MPC sequence is a MatrixSequence image
 * data[k*nr*nc + j*nr + i] (tools/matrix_sequence.h:81-83), dense matrices are
 * column-major (Eigen::MatrixXd).  A batch is described by one base pointer
 * and one stride (in doubles) per array: QP b lives at base + b*stride, so both
 * "array of structures" (all sequences of a QP contiguous) and "structure of
 * arrays" placements work, and a stride of 0 shares an array across the batch.
 * A batch of one QP lives at the base pointers: no entry point reads a stride
 * when batch == 1 (but for the gradient slots of fbstab_hip_*_adjoint_batch_reduced,
 * where a stride of 0 asks for the sum over the batch at every batch size).
 *
 * Error behaviour: no exception crosses this boundary.  Functions return
 * FBSTAB_HIP_OK or an error code and fbstab_hip_last_error() describes the
 * failure (the C++ facade in include/fbstab/ turns these into the
 * std::runtime_error the reference throws).  Per-QP outcomes are reported in
 * fbstab_solver_out_t::eflag; a per-QP factorisation failure, where the
 * reference would throw out of Solve (fbstab_algorithm-impl.h:263-274), is
 * reported as FBSTAB_DIVERGENCE for that QP only.
 *
 * There is no CPU execution path in this library: without a usable HIP device
 * every create call fails with FBSTAB_HIP_ERR_DEVICE.
 */
#ifndef FBSTAB_HIP_H_
#define FBSTAB_HIP_H_

#include "fbstab_types.h"

#ifdef __cplusplus
extern "C" {
#endif

enum fbstab_hip_status {
  FBSTAB_HIP_OK = 0,
  FBSTAB_HIP_ERR_ARGUMENT = 1,    /* null pointer, non-positive size, batch > max_batch */
  FBSTAB_HIP_ERR_DEVICE = 2,      /* HIP runtime error / no device */
  FBSTAB_HIP_ERR_UNSUPPORTED = 3  /* problem does not fit the on-chip budget */
};

/* Where the caller's arrays live, and whether the call may return before the
 * GPU has finished (device memory only; the caller then syncs the stream). */
enum fbstab_hip_flags {
  FBSTAB_HIP_HOST_POINTERS = 0,
  FBSTAB_HIP_DEVICE_POINTERS = 1,
  FBSTAB_HIP_ASYNC = 2,
  /* Receding-horizon hint (MPC, device pointers): the matrix sequences
   * Q, R, S, A, B, E, L of every QP of this call are the ones of the previous
   * call on this handle that carried the flag (same batch size); only
   * q, r, c, d, x0 and the initial guess may have changed.  The library then
   * keeps its per-QP copies of the matrices between calls instead of
   * rebuilding them.  The first flagged call, and a flagged call after an
   * unflagged one, build them.  Ignored where it cannot be honoured (batch
   * larger than the resident QP slots, kernels without such copies); results
   * are the same with or without it. */
  FBSTAB_HIP_KEEP_MATRICES = 4,
  /* With FBSTAB_HIP_DEVICE_POINTERS: `out` is a HOST array all the same.  The call
   * then waits for the solve and copies the SolverOut records back (the zero-copy
   * single-QP path of the C++ facade: ProblemDataRef / VariableRef over device
   * memory, fbstab_mpc.h:90-150, with the SolverOut returned by value). */
  FBSTAB_HIP_OUT_ON_HOST = 8
};

/* Index of each MPC sequence in fbstab_mpc_batch_t (FBstabMpc::ProblemData
 * member order, fbstab/fbstab_mpc.h:67-81). */
enum fbstab_mpc_seq {
  FBSTAB_MPC_Q = 0, FBSTAB_MPC_R, FBSTAB_MPC_S, FBSTAB_MPC_q, FBSTAB_MPC_r,
  FBSTAB_MPC_A, FBSTAB_MPC_B, FBSTAB_MPC_c, FBSTAB_MPC_E, FBSTAB_MPC_L,
  FBSTAB_MPC_d, FBSTAB_MPC_x0, FBSTAB_MPC_NSEQ
};

/* Index of each dense array (FBstabDense::ProblemData, fbstab_dense.h:55-64). */
enum fbstab_dense_arr {
  FBSTAB_DENSE_H = 0, FBSTAB_DENSE_f, FBSTAB_DENSE_G, FBSTAB_DENSE_h,
  FBSTAB_DENSE_A, FBSTAB_DENSE_b, FBSTAB_DENSE_NARR
};

typedef struct fbstab_mpc_batch_t {
  const double* base[FBSTAB_MPC_NSEQ];
  long long stride[FBSTAB_MPC_NSEQ]; /* doubles between consecutive QPs */
} fbstab_mpc_batch_t;

typedef struct fbstab_dense_batch_t {
  const double* base[FBSTAB_DENSE_NARR];
  long long stride[FBSTAB_DENSE_NARR];
} fbstab_dense_batch_t;

/* Initial guess in (z, l, v), solution out (z, l, v, y); y is ignored on input
 * (FBstabMpc::Variable, fbstab_mpc.h:126-136; fbstab_algorithm-impl.h:334-347). */
typedef struct fbstab_var_batch_t {
  double* base[4];       /* z, l, v, y */
  long long stride[4];
} fbstab_var_batch_t;

typedef struct fbstab_mpc_solver* fbstab_mpc_handle_t;
typedef struct fbstab_dense_solver* fbstab_dense_handle_t;

const char* fbstab_hip_last_error(void);
int fbstab_hip_device_count(void);

/* ---- MPC ---------------------------------------------------------------- */
int fbstab_hip_mpc_create(int N, int nx, int nu, int nc, int max_batch, int device,
                          fbstab_mpc_handle_t* handle);
/* The same for a caller that keeps `handles_in_flight` handles busy on this device at the same time - one
 * batch each, every handle on a stream of its own (the reference has no counterpart: FBstabMpc is a
 * single-threaded CPU object, fbstab/fbstab_mpc.h:56-60).  A batch launch is a persistent grid that pulls QPs
 * from a queue; alone on the device it wants every resident wavefront slot (four workgroups per CU on the
 * BASELINE shape), but with several launches in flight the others fill the device and a launch does better
 * with its share: each row of a wavefront then gets more QPs of the batch and the tail of the launch - rows
 * that have run out of QPs while their wavefront's last one finishes - shrinks (rows busy 0.95 instead of 0.82
 * per Newton step at eight in flight; +2.7 % throughput, and a quarter of the scratch memory: 0.44 instead
 * of 1.75 GB per handle).  handles_in_flight = 1 is fbstab_hip_mpc_create.
 * The rule (fbstab_amd/csrc/fb_in_flight.h): with `resident` workgroups per CU from the occupancy query,
 *     concurrent = min(handles_in_flight, hw_queues)      launches that can really run side by side
 *     per CU     = ceil(2 * resident / concurrent)        clamped to [1, resident], and for
 *                                                         handles_in_flight >= 2 to max(1, resident / 2)
 * so that the launches in flight want TWICE the resident slots between them: the workgroups that wait take
 * the SIMDs a launch frees when it runs into its tail.  Streams that share a hardware queue run their launches
 * one after the other, so `hw_queues` counts what can overlap: it is what the HIP runtime of this process was
 * told, GPU_MAX_HW_QUEUES read (only read; 1..32, unset or unparsable = 4, HIP's default) at handle creation -
 * a hint about how many of the caller's streams run side by side.  On the BASELINE shape (resident = 4): eight
 * in flight on eight queues one workgroup per CU, 0.44 GB of scratch per handle; eight in flight on four
 * queues, or four in flight, two per CU and 0.87 GB; two in flight two per CU; a handle that shares the device
 * never keeps more than half the grid.  A caller whose streams share queues for other reasons can force a
 * share with FBSTAB_HIP_WGS_PER_CU in the environment at handle creation.
 * What the share costs a handle that is then used ALONE: it keeps its fraction of the grid - a quarter of
 * the workgroups at handles_in_flight = 8 on eight queues (never fewer than one per CU), so a lone launch fills
 * a quarter of the chip - and fbstab_hip_mpc_receding_sweep, whose one-launch form needs batch <= workgroups x QPs per
 * workgroup, falls back to one launch per step at a batch that much smaller (same results, bitwise; slower).
 * fbstab_hip_mpc_query reports the handle's `workgroups` and `scratch_bytes` as created, so a caller can see
 * the share it got.  Values outside 1..64 are refused (FBSTAB_HIP_ERR_ARGUMENT).
 * The share is a hint measured on the BASELINE shape.  Shapes of the widest record instance (stage width up
 * to 32 with up to 16 constraint rows) did better as a stream of batches with
 * every handle keeping the whole grid (handles_in_flight = 1 on each of eight handles: 28 k against 24 k
 * QPs/sec on (30,20,6,16)) - measure both on a new shape. */
int fbstab_hip_mpc_create_in_flight(int N, int nx, int nu, int nc, int max_batch, int device,
                                    int handles_in_flight, fbstab_mpc_handle_t* handle);
int fbstab_hip_mpc_destroy(fbstab_mpc_handle_t handle);
int fbstab_hip_mpc_set_options(fbstab_mpc_handle_t handle, const fbstab_options_t* options);
int fbstab_hip_mpc_get_options(fbstab_mpc_handle_t handle, fbstab_options_t* options);
/* stream: a hipStream_t, or NULL for the handle's own stream, which is a blocking
 * stream (ordered against the device's null stream both ways).  With
 * FBSTAB_HIP_DEVICE_POINTERS the caller's arrays must be ready on the stream the
 * call runs on: work queued on another non-blocking stream needs an event.
 * Strides, with batch > 1 (host and device pointers alike, checked before anything
 * is queued; the same rule holds for fbstab_hip_mpc_solve_batch_final, the receding
 * sweeps, the dense solves and the sharded entry points, which call these):
 *   x:    every QP has its own z, l, v and y: a stride below the vector length is
 *         FBSTAB_HIP_ERR_ARGUMENT.
 *   data: a stride of 0 shares the array, a stride of at least the array length gives
 *         every QP its own; any other stride, a negative one included, is
 *         FBSTAB_HIP_ERR_ARGUMENT.  (The sweeps advance x0 in place: its stride is at
 *         least nx.) */
int fbstab_hip_mpc_solve_batch(fbstab_mpc_handle_t handle, int batch,
                               const fbstab_mpc_batch_t* data, const fbstab_var_batch_t* x,
                               fbstab_solver_out_t* out, int flags, void* stream);
/* fbstab_hip_mpc_solve_batch followed, on the same stream, by the numbers of the
 * summary block the reference prints at Display::FINAL (PrintFinal,
 * fbstab_algorithm-impl.h:493-541): norms[4 q .. 4 q + 3] = {|rz|, |rl|, |rv|} of the
 * penalised natural residual (full_residual.cc:99-109) at the point QP q returned, and
 * the stopping tolerance abs_tol + rel_tol (1 + ||(f, h, b)||) (impl:137).  `norms` lives
 * where `out` lives (host for host-pointer calls and with FBSTAB_HIP_OUT_ON_HOST, device
 * otherwise).  Same kernels, same iteration counts as solve_batch.  For SUCCESS and the
 * Newton-iteration limit these are the numbers the reference prints (its rk_ is evaluated
 * at the returned point, impl:162-170, :188-199); for infeasibility exits (impl:204-212:
 * the certificate is returned, rk_ belongs to x(k)) and the proximal-iteration limit
 * (impl:219-223: rk_ is one iteration old) the reference prints a residual of a point the
 * solve does not return - callers that need that text use solve_traced. */
int fbstab_hip_mpc_solve_batch_final(fbstab_mpc_handle_t handle, int batch,
                                     const fbstab_mpc_batch_t* data, const fbstab_var_batch_t* x,
                                     fbstab_solver_out_t* out, double* norms, int flags, void* stream);
/* ONE QP given by host pointers, solved synchronously, with the per-iteration
 * display of the reference returned as data: every line the reference's
 * Display::ITER and ITER_DETAILED levels would print during this solve
 * (fbstab_algorithm-impl.h:155-172, :250-257, :381) becomes one
 * fbstab_trace_record_t, in the reference's print order; the caller formats
 * the kinds its display level shows (the C++ facade does, PrintTrace in
 * include/fbstab/fbstab_algorithm.h).  At most `capacity` records are stored;
 * *count receives the number produced.  Runs on the flat-vector kernel (one
 * QP per wavefront) whatever kernel the handle uses for batches, so iteration
 * counts can differ from a solve_batch call within the tolerance the parity
 * tests state. */
int fbstab_hip_mpc_solve_traced(fbstab_mpc_handle_t handle, const fbstab_mpc_batch_t* data,
                                const fbstab_var_batch_t* x, fbstab_solver_out_t* out,
                                fbstab_trace_record_t* trace, int capacity, int* count);
/* Warm-started receding-horizon sweep on the device (BASELINE configs[4]): `steps`
 * closed-loop steps of `batch` independent trajectories queued on one stream with
 * no host round trip in between.  Step k solves the batch as
 * fbstab_hip_mpc_solve_batch would (FBstabMpc::Solve, fbstab_mpc.h:181-195, with
 * the previous step's (z, l, v) as the initial guess, unshifted - what a caller of
 * the reference gets by passing the same Variable again, fbstab_algorithm-impl.h:140)
 * and then advances every trajectory's initial state with the simulation model the
 * reference's generator hands out (OcpGenerator::SimulationInputs,
 * fbstab/test/ocp_generator.h:31-38):  x0 <- A x0 + B u0,  u0 = the first input of
 * the solution.  All pointers are DEVICE pointers; data->base[FBSTAB_MPC_x0] is
 * updated in place (it must be writable), x holds the last step's solution on
 * return, out its SolverOut records.  The matrix sequences must not change during
 * the sweep (FBSTAB_HIP_KEEP_MATRICES semantics).
 *   retire != 0: a trajectory whose solve does not end in SUCCESS is parked at the
 *                origin for the rest of the sweep (x0 = 0, zero guess, u0 = 0).
 *   u_log:   NULL or device array [steps][batch][nu] receiving every u0.
 *   stats:   NULL or HOST array [steps][4]: sum of Newton iterations, solves ended in
 *            SUCCESS, trajectories retired so far, largest Newton count of the step.
 *   kernel_ms: NULL or HOST array [steps]: device time of each step's solve.
 * Shapes served by a record kernel run the whole sweep as ONE launch in which every
 * trajectory advances at its own pace (no trajectory waits for the slowest solve of a
 * step; same results per trajectory and per step); kernel_ms[k] is then the launch
 * time / steps for every k.  Other shapes (or FBSTAB_HIP_SWEEP_PER_STEP=1) queue one
 * solve launch and one plant launch per step.
 * Synchronous: returns when the sweep has finished. */
typedef struct fbstab_receding_plant_t {
  const double* A;      /* nx x nx, column-major */
  const double* B;      /* nx x nu, column-major */
  long long stride_A;   /* doubles between trajectories; 0 = one plant for all */
  long long stride_B;
} fbstab_receding_plant_t;
int fbstab_hip_mpc_receding_sweep(fbstab_mpc_handle_t handle, int batch, const fbstab_mpc_batch_t* data,
                                  const fbstab_var_batch_t* x, fbstab_solver_out_t* out,
                                  const fbstab_receding_plant_t* plant, int steps, int retire,
                                  double* u_log, unsigned long long* stats, float* kernel_ms,
                                  void* stream);

/* Device time of the solver kernel in the most recent solve_batch call on this
 * handle, measured with HIP events on the stream it ran on (ms; < 0 if none). */
double fbstab_hip_mpc_last_kernel_ms(fbstab_mpc_handle_t handle);
/* Bytes of device scratch and of LDS per workgroup the handle uses, and the
 * number of resident workgroups it launches (for DESIGN.md / diagnostics).  (Record kernels, round 6: a batch
 * of no more QPs than `workgroups` is spread one QP per wavefront - a handle created for a small max_batch
 * therefore keeps one workgroup, and four QP slots of scratch, per QP - LABNOTES R6.6.) */
int fbstab_hip_mpc_query(fbstab_mpc_handle_t handle, long long* scratch_bytes,
                         int* lds_bytes, int* workgroups, int* threads);

/* Name of the kernel instance this handle's batches run on, e.g.
 * "fbstab_mpc_r16_kernel<12,4,20>" (record kernel, four QPs per wavefront) or
 * "fbstab_mpc_kernel<64>" (any shape, one QP per wavefront). */
const char* fbstab_hip_mpc_kernel_name(fbstab_mpc_handle_t handle);

/* Iterative refinement of the Newton steps - an option, OFF by default (fbstab_options_t::reserved = 0).
 * The kernels measure with every Newton step what the linear solve left of the Newton system (the z and l
 * share of the first line-search trial's norm).  With reserved = k > 0 a step whose leftover exceeds
 * 2^(1 - k) of the tolerance the solver's next tests compare against is solved once more for its
 * residual with the same factors and corrected (eps |V| |dx| in every block row afterwards): a linear
 * solve more accurate than RiccatiLinearSolver::Solve's (fbstab/components/riccati_linear_solver.cc:
 * 212-344), hence not the default - iteration counts then part from the reference's where the reference's
 * own rounding decides a stopping test.  This call returns the number of Newton steps of the most recent
 * solve_batch / receding_sweep call that were refined (waits for that launch; -1 if there was none;
 * 0 with the option off). */
int fbstab_hip_mpc_refined_steps(fbstab_mpc_handle_t handle, long long* steps);

/* The longest-first queue of a record handle.  The rows of a packed batch launch pull QP indices from a queue,
 * and a wavefront lives until the slowest of its rows is done; with the longest QPs handed out first a launch
 * drains on its shortest ones.  A record handle therefore remembers the Newton counts of its last packed
 * fbstab_hip_mpc_solve_batch[_final] - one kernel of one workgroup behind the solve sorts the QP indices by them,
 * descending, ascending index inside equal counts - and the next such solve of the SAME batch size hands its queue
 * tickets out in that order: the case of a controller that calls the handle with the same plants one time step
 * later, whose counts follow the previous step's (rank correlation 0.9).  The order is a hint and nothing else: a
 * QP's results do not depend on when or where in the launch it is solved, bit for bit, so a stale order costs the
 * gain only.  A solve of another batch size installs its own order; spread launches (batch <= the handle's
 * workgroups), FBSTAB_HIP_KEEP_MATRICES solves, sweeps, adjoints, tangents, many-right-hand-side solves and probes
 * neither use nor change it.  FBSTAB_HIP_QUEUE_ORDER=0 in the environment when the handle is created switches it
 * off.  Footprint: max_batch + 1024 ints.
 * This call copies the stored order to the host array `order` of `capacity` ints (waits for the solve that
 * produced it): *n = its batch size, or 0 where the handle holds none (then `order` may be NULL). */
int fbstab_hip_mpc_queue_order(fbstab_mpc_handle_t handle, int* order, int capacity, int* n);

/* Diagnostics used by the parity tests: runs ONE Newton step of the device path
 * (LinearSolver::Initialize + Solve of the reference, abstract_components.h:291-338)
 * for a single QP given by host pointers.  io: [zbar, lbar, vbar] in,
 * [dz, dl, dv, A*dz, W_z, W_l, r_z, r_l, ok] out. */
int fbstab_hip_mpc_debug_newton(fbstab_mpc_handle_t handle, const fbstab_mpc_batch_t* data,
                                const fbstab_var_batch_t* x, double* io);

/* ---- derivatives of the solution map (no counterpart in the reference) ------
 * Gradients dL/d(data) of a loss L of the solutions (z, l, v) of a batch, given the seeds
 * (gz, gl, gv) = dL/d(z, l, v) at the returned points x.  One launch, one QP per workgroup:
 * at x = xbar = the point the reference's Newton matrix
 *   V = [H + sigma I, G', A'; -G, sigma I, 0; -C A, 0, mus]
 * (RiccatiLinearSolver::Initialize, fbstab/components/riccati_linear_solver.cc:77-210; the
 * inner residual's Jacobian, full_residual.cc:49-74, C = d phi / d y and mus = d phi / d v
 * + sigma C of the penalised FB function with options.alpha) is factored once, and one
 * Solve (:212-344) with the right-hand side (gz, -gl, -C gv) gives (dz, dl, dv).  For the QP
 * min 1/2 z'Hz + f'z s.t. Gz = h, Az <= b (mpc_data.cc: G = [-I; A B -I; ...], h = -(x0, c),
 * A = blockdiag([E L]), b = -d) that is f_bar = -dz, h_bar = dl, b_bar = dv,
 * H_bar = -(dz z' + z dz')/2, G_bar = -(dl z' + l dz'), A_bar = -(dv z' + v dz'), returned per
 * sequence in the layout of fbstab_mpc_batch_t (Q and R: the gradient of the symmetric part).
 * This is the derivative of the solution map with V regularised by sigma (a bias of
 * O(sigma); at a strictly complementary point it tends to the active-set derivative as
 * sigma -> 0).  sigma <= 0 selects 1e-8, the reference's default sigma0
 * (fbstab_algorithm-impl.h:34), whatever the handle's options say.
 *   x:      the points, (z, l, v) (the y slot is not read).
 *   seed:   (gz, gl, gv); the l and v slots may be NULL (zero).
 *   grad:   one slot per sequence, strides as in fbstab_mpc_batch_t; a NULL slot is not
 *           computed.  Every slot that is not NULL is written.
 *   adj:    NULL, or (dz, dl, dv) (its NULL slots are skipped).
 *   status: per QP, 0, or 1 where a factorisation failed (its gradients and adj are zero).
 *           It lives where solve_batch's `out` lives (host for host-pointer calls and with
 *           FBSTAB_HIP_OUT_ON_HOST, device otherwise).
 * Flags, streams and validation are those of fbstab_hip_mpc_solve_batch; every QP needs
 * its own slots in x, seed, grad and adj (stride >= length when batch > 1).  Kernels: every
 * record instance (the one-row <12,4,20>, <12,4,32> and the row-pair <18,5,10>, <24,8,16>,
 * <24,8,32>) has an adjoint on its own records (fbstab_mpc_r16_adjoint_kernel: in the handle's
 * scratch, with the solve's LDS and grid; the slots' matrix copies are rebuilt by the next
 * FBSTAB_HIP_KEEP_MATRICES solve); the flat-vector kernel's shapes run the flat-vector adjoint
 * (fbstab_mpc_adjoint_kernel) in the handle's workspace.  Which of the two a RECORD handle
 * runs is fixed when it is created: by default the one-row instances run their record
 * adjoint and the row-pair instances the flat-vector adjoint (their record adjoint has not
 * been timed against it on wide workloads yet); FBSTAB_HIP_FLAT_ADJOINT=0 in the environment
 * at creation selects the record adjoint on every record handle, =1 the flat-vector adjoint.
 * fbstab_hip_mpc_adjoint_kernel_name names the kernel the next call launches.
 * A record handle on the flat-vector adjoint allocates that kernel's scratch at its first
 * call: MpcLayout::ws_doubles (fb_mpc.h; the iterate vectors and the per-stage factor record:
 * 58 k doubles = 463 KB at (N, nx, nu, nc) = (30, 18, 5, 10), 101 k at (30, 24, 8, 16)) per
 * workgroup, times the handle's workgroups, held until destroy and not counted in
 * fbstab_hip_mpc_query's scratch_bytes.  The record adjoint allocates nothing.
 * fbstab_hip_mpc_last_kernel_ms then reports this launch. */
typedef struct fbstab_mpc_grad_batch_t {
  double* base[FBSTAB_MPC_NSEQ];
  long long stride[FBSTAB_MPC_NSEQ];
} fbstab_mpc_grad_batch_t;
int fbstab_hip_mpc_adjoint_batch(fbstab_mpc_handle_t handle, int batch, const fbstab_mpc_batch_t* data,
                                 const fbstab_var_batch_t* x, const fbstab_var_batch_t* seed, double sigma,
                                 const fbstab_mpc_grad_batch_t* grad, const fbstab_var_batch_t* adj,
                                 int* status, int flags, void* stream);
/* Name of the kernel the next fbstab_hip_mpc_adjoint_batch of this handle launches. */
const char* fbstab_hip_mpc_adjoint_kernel_name(fbstab_mpc_handle_t handle);
/* fbstab_hip_mpc_adjoint_batch for data shared by the batch: gradients SUMMED over the batch.  The
 * learning workloads these gradients exist for (a differentiable MPC, an OptNet-style layer) share
 * the matrices among all QPs of a batch (a data stride of 0), and what they need is
 * sum_b dL/d(data_b): ONE array, not `batch` images that are written and then read again for the sum.
 * Everything is as in fbstab_hip_mpc_adjoint_batch - validation order, flags, streams, host staging,
 * batch == 0, the adjoint kernel and fbstab_hip_mpc_last_kernel_ms, which reports the adjoint's
 * launch as there - except:
 *   grad:   a slot whose stride is at least the array length is a per-QP gradient, computed by the
 *           same kernel and bitwise what fbstab_hip_mpc_adjoint_batch returns.  A slot whose stride
 *           is 0 receives ONE array, the sum over the batch (a host-pointer call downloads one array).
 *           Any mix is allowed; with batch > 1 a stride strictly between 0 and the length, or below
 *           0, is FBSTAB_HIP_ERR_ARGUMENT.
 *   out:    NULL, or the SolverOut records of the solve that produced x, living where `status` lives.
 *           QPs whose eflag is not FBSTAB_SUCCESS are left out of every reduced slot, and so are QPs
 *           whose adjoint status is 1, with or without `out` (their points may hold anything, NaN
 *           included: they are not read into the sum).  Per-QP slots do not depend on `out`.
 * The adjoint kernel runs with the reduced slots NULL, so it does not write those images, and with
 * adj = the caller's, or where the caller takes none a buffer of the handle's.  Two more launches
 * on the same stream then form the sums from (x, adj) on the matrix cores (fb_grad_reduce.h:
 * fbstab_grad_reduce_kernel, v_mfma_f64_16x16x4, one wavefront per 16 x 16 tile of a stage's
 * -(P'Z + X'DZ) and per chunk of 128 QPs; fbstab_grad_reduce_finish_kernel adds a tile's chunks).
 * The order of every sum is fixed by the shape and the batch size alone - no atomics, nothing that
 * depends on the grid, the CU count or the handle - so the same inputs give the same bits.
 * Memory: the first reduced call of a handle allocates, and holds until destroy, max_batch x
 * (nz + nl + nv) doubles for the adjoint steps (97.5 MB at (N, nx, nu, nc) = (30, 12, 4, 20) and
 * max_batch 8192) and tiles x ceil(max_batch / 128) x 272 doubles for the partial sums (94 tiles
 * there: 13.1 MB); as for the flat adjoint's scratch, fbstab_hip_mpc_query's scratch_bytes does
 * not count them. */
int fbstab_hip_mpc_adjoint_batch_reduced(fbstab_mpc_handle_t handle, int batch, const fbstab_mpc_batch_t* data,
                                         const fbstab_var_batch_t* x, const fbstab_var_batch_t* seed,
                                         double sigma, const fbstab_mpc_grad_batch_t* grad,
                                         const fbstab_var_batch_t* adj, int* status,
                                         const fbstab_solver_out_t* out, int flags, void* stream);

/* ---- the closed loop's derivative: a logged sweep and its adjoint through time ------------------------------
 * fbstab_hip_mpc_receding_sweep_logged is fbstab_hip_mpc_receding_sweep (same arguments, same results bit for
 * bit; log == NULL is that function) that also records what the backward pass needs, per step k and trajectory:
 * the point (z_k, l_k, v_k) the step returned, the state x_k it was solved for and its eflag.  All DEVICE
 * arrays; a NULL slot is not logged.  A retired trajectory (retire != 0) logs a zero point and eflag -1 at and
 * after its retirement step.  The one-launch and the per-step form log bitwise-equal arrays.  Footprint:
 * steps x batch x (nz + nl + nv + nx) doubles - 9.8 GB for 4096 trajectories x 200 steps at (N, nx, nu, nc) =
 * (30, 12, 4, 20). */
typedef struct fbstab_sweep_log_t {
  double *z, *l, *v;   /* [steps][batch][nz | nl | nv] */
  double* x0;          /* [steps][batch][nx]: x_k */
  int* eflag;          /* [steps][batch]; -1 once the trajectory is retired */
} fbstab_sweep_log_t;
int fbstab_hip_mpc_receding_sweep_logged(fbstab_mpc_handle_t handle, int batch, const fbstab_mpc_batch_t* data,
                                         const fbstab_var_batch_t* x, fbstab_solver_out_t* out,
                                         const fbstab_receding_plant_t* plant, int steps, int retire,
                                         double* u_log, unsigned long long* stats, float* kernel_ms,
                                         void* stream, const fbstab_sweep_log_t* log);

/* ---- closed-loop scenarios: a disturbed plant and a shifted warm start -----------------------------------------
 * fbstab_hip_mpc_receding_sweep_scenario is fbstab_hip_mpc_receding_sweep_logged with two options of the step
 * between two solves.  scenario == NULL, or w == NULL with shift == 0, IS that function: the same launches, the
 * same bits.  Everything else - arguments, validation, retirement, statistics, the log, the two forms of the
 * sweep (bitwise equal to each other here as well) - is as there.
 *   w:     Monte-Carlo over disturbance realisations: x_(k+1) = A x_k + B u_k + w_k, one addition behind the sum
 *          over the columns of A and B.  A parked trajectory (retire != 0) stays at the origin: w is not added.
 *          A failed step of an unretired trajectory advances with the u_0 it returned, as ever, plus w_k.
 *          log->x0[k] remains the state step k was solved for; w_(steps-1) enters the x0 left in `data`.
 *   shift: 1 moves the point step k returned one stage towards the present before it is step k + 1's guess, as
 *          receding-horizon controllers do: z_i <- z_(i+1) in blocks of nx + nu, l_i <- l_(i+1) in blocks of nx,
 *          v_i <- v_(i+1) in blocks of nc for i = 0 .. N-1; stage N keeps its values; y is ignored on input and
 *          is not touched.  The move follows the step's retirement handling, statistics, u_log and log writes -
 *          the log and u_log hold returned points, unshifted - and does not follow the last step: x on return is
 *          the last step's solution as it was returned.  Values other than 0 and 1 are FBSTAB_HIP_ERR_ARGUMENT,
 *          before anything is queued.
 * Which way the shift cuts is a property of the problem.  On a time-invariant horizon under a persistent
 * disturbance it saves most of the Newton steps (the tables of DESIGN.md 4.3: a quarter to a half of the
 * unshifted count); on random time-varying horizons, whose stage i + 1 says nothing about stage i, the shifted
 * point is the WORSE guess (two to three times the count).  Hence an option, off by default. */
typedef struct fbstab_sweep_scenario_t {
  const double* w;  /* NULL, or DEVICE array [steps][batch][nx]: x_(k+1) = A x_k + B u_k + w_k */
  int shift;        /* 0: the previous point is the next guess as it stands
                       1: it is moved one stage towards the present first */
} fbstab_sweep_scenario_t;
int fbstab_hip_mpc_receding_sweep_scenario(fbstab_mpc_handle_t handle, int batch, const fbstab_mpc_batch_t* data,
                                           const fbstab_var_batch_t* x, fbstab_solver_out_t* out,
                                           const fbstab_receding_plant_t* plant, int steps, int retire,
                                           double* u_log, unsigned long long* stats, float* kernel_ms,
                                           void* stream, const fbstab_sweep_log_t* log,
                                           const fbstab_sweep_scenario_t* scenario);

/* Reverse mode through the sweep.  With u_k = entries [nx, nx + nu) of z_k and x_(k+1) = A x_k + B u_k, the seeds
 * gu[k] = dL/du_k ([steps][batch][nu]) and gx[k] = dL/dx_(k+1) ([steps][batch][nx]; either may be NULL: zero) are
 * taken backwards along every trajectory.  Start with lambda = 0 and for k = steps-1 .. 0:
 *   mu = gx[k] + lambda                             (mu_log[k] = mu where mu_log is given)
 *   eflag_log[k] == -1 (retired):       lambda <- 0
 *   eflag_log[k] != FBSTAB_SUCCESS:     lambda <- A'mu          (the point is no solution: u_k is a constant)
 *   otherwise one adjoint (fbstab_hip_mpc_adjoint_batch's, same sigma rule) at the logged point with the seed
 *   gu[k] + B'mu on the u0 entries of z and zero elsewhere:
 *     factorisation failed:             status += 1, lambda <- A'mu
 *     else every wanted sequence's gradient += that adjoint's gradient table, lambda <- A'mu - dl[0:nx].
 * The x0 slot of `grad` receives the final lambda = dL/dx_0 (not a sum over the steps); every other slot is the
 * sum over the steps, added last step first without atomics (the same inputs give the same bits).  The plant's
 * own gradients are left to the caller: A_bar = sum_k mu_k x_k', B_bar = sum_k mu_k u_k' from mu_log and the logs.
 * All pointers are DEVICE pointers.  Every non-NULL grad slot is written (zeros for a trajectory without a
 * contributing step) and needs stride >= length when batch > 1 (stride 0 is FBSTAB_HIP_ERR_ARGUMENT: sums over
 * the batch are the caller's).  data->base[FBSTAB_MPC_x0] is not read.  log->z, l, v and eflag are required.
 * status: [batch], the number of steps whose factorisation failed.
 * Handles whose fbstab_hip_mpc_adjoint_kernel_name is a record adjoint run ONE launch of
 * fbstab_mpc_r16_sweep_adjoint_kernel, every row (pair) taking a trajectory through all its steps; it needs
 * rows x nz doubles for the seed vectors, allocated at the first call and held until destroy.  Every other
 * handle, and every handle with FBSTAB_HIP_SWEEP_ADJOINT_PER_STEP=1 in the environment of the call, queues per
 * step fbstab_sweep_costate_kernel, the handle's adjoint launch into a per-QP image of the handle's own
 * (max_batch x (all 12 sequences + nz + 2 nx) doubles, allocated at the first call) and the costate kernel again.
 * fbstab_hip_mpc_sweep_adjoint_kernel_name names what the next call launches.  Synchronous.
 * The recursion holds as it stands for the disturbed plant x_(k+1) = A x_k + B u_k + w_k of
 * fbstab_hip_mpc_receding_sweep_scenario (w_k enters x_(k+1) with the identity), and for the shifted warm start
 * (the guess is not an argument of the solution map): dL/dw_k = mu_log[k] where eflag_log[k] != -1, zero otherwise.
 * Not served: gradients summed over the batch, forward mode through the sweep, seeds on the rest of z_k, l_k,
 * v_k. */
int fbstab_hip_mpc_receding_sweep_adjoint(fbstab_mpc_handle_t handle, int batch, const fbstab_mpc_batch_t* data,
                                          const fbstab_receding_plant_t* plant, int steps, int retire,
                                          const fbstab_sweep_log_t* log, const double* gu, const double* gx,
                                          double sigma, const fbstab_mpc_grad_batch_t* grad, double* mu_log,
                                          int* status, void* stream);
const char* fbstab_hip_mpc_sweep_adjoint_kernel_name(fbstab_mpc_handle_t handle);

/* Forward mode of the same derivative: the tangent (dz, dl, dv) = J dtheta of the solutions for a perturbation
 * dtheta of the problem data - the first-order update of a plan when the state or a forecast moves (a warm start
 * for the next solve), a column of the feedback gain du0/dx0 per unit direction dx0, a disturbance direction
 * through the controller.  At a returned point with xbar = x the matrix V above is the Jacobian of the inner
 * residual F, and the tangent system is
 *   V (dz, dl, dv) = -dF/dtheta dtheta = (gz, -gl, -C gv),
 *   gz = -(dH z + df + dG' l + dA' v)      gl = dh - dG z      gv = db - dA z
 * with dH the symmetric part of the perturbation: exactly the adjoint's system for the seeds (gz, gl, gv).  In
 * MPC terms (the constant -I blocks of G have no perturbation), stage by stage,
 *   gz[x_i u_i] = -( sym[dQ_i dS_i'; dS_i dR_i] (x_i, u_i) + (dq_i, dr_i) + d[A_i B_i]' l_(i+1) + d[E_i L_i]' v_i )
 *   gl[l_0] = -dx0     gl[l_(i+1)] = -dc_i - d[A_i B_i] (x_i, u_i)     gv[v_i] = -dd_i - d[E_i L_i] (x_i, u_i)
 * (stage N has no [A B] term).  Two launches on one stream: fbstab_tangent_rhs_kernel (fb_tangent.h: one
 * wavefront per QP and stage; every perturbation image is read once, no atomics, every sum in an order fixed by
 * the shape, so a QP's seeds do not depend on the batch or the grid) writes the seeds, and the launch of
 * fbstab_hip_mpc_adjoint_batch - the same kernel selection, no gradient slot, adj = dx - solves for them.  dQ and
 * dR enter through their symmetric part (dQ + dQ')/2, the part the adjoint returns the gradient of, so that
 * <seed, J dtheta> = sum_k <grad_k, dtheta_k> for any direction; dS enters as dS x on the u rows and dS' u on
 * the x rows.
 *   x:      the points, (z, l, v) (the y slot is not read).
 *   ddata:  the perturbations, one slot per sequence in the layout of `data`.  A NULL slot is a zero
 *           perturbation (not read, not multiplied); stride 0 is one direction shared by the batch; stride >=
 *           length is a direction per QP.  With batch > 1 any other stride is FBSTAB_HIP_ERR_ARGUMENT.
 *   dx:     receives (dz, dl, dv); the y slot is unused.  Every QP needs its own slot, as for adj.
 *   rhs:    NULL, or receives the seeds (gz, gl, gv) (all three slots, strides as for dx).  On a device-pointer
 *           call the direction kernel writes them into the caller's arrays and the adjoint reads them there.
 *   status: as fbstab_hip_mpc_adjoint_batch: 1 where a factorisation failed; that QP's dx is zero.
 * sigma, flags, streams, host staging, batch == 0 and validation are those of fbstab_hip_mpc_adjoint_batch;
 * fbstab_hip_mpc_last_kernel_ms reports the adjoint kernel's launch, as there; a FBSTAB_HIP_KEEP_MATRICES solve
 * behind it rebuilds its copies as behind an adjoint call.  Memory: without a device rhs the seeds live in a
 * buffer of the handle, max_batch x (nz + nl + nv) doubles, allocated by the first call that needs it and held
 * until destroy - the SAME allocation as the adjoint steps of fbstab_hip_mpc_adjoint_batch_reduced (neither call
 * needs it once it has returned), not counted by fbstab_hip_mpc_query.  A shape whose stage images (nx + nu +
 * nc) x (nx + nu) + nx x (nx + nu) doubles exceed 160 KB of LDS is FBSTAB_HIP_ERR_UNSUPPORTED. */
int fbstab_hip_mpc_tangent_batch(fbstab_mpc_handle_t handle, int batch, const fbstab_mpc_batch_t* data,
                                 const fbstab_var_batch_t* x, const fbstab_mpc_batch_t* ddata, double sigma,
                                 const fbstab_var_batch_t* dx, const fbstab_var_batch_t* rhs,
                                 int* status, int flags, void* stream);

/* ---- many right-hand sides: factor V once, solve for nrhs of them -----------------------------------------------
 * The adjoint and the tangent above return one vector per factorisation of V.  The matrices their users ask for -
 * the local feedback law du0/dx0 (nu x nx) and the whole plan's sensitivity dz/dx0, or several loss seeds at the
 * same solutions - cost them one factorisation per column or row.  In the Riccati solver the factorisation of a
 * stage is the O(nx^3) part and the vector recursions of a Solve are O(nx^2); these two calls factor V once per QP
 * and run the recursions once per right-hand side (fb_kkt_multi.h; fbstab_mpc_kkt_multi_kernel, one QP per
 * workgroup on the flat-vector layout, on EVERY handle).
 *
 * fbstab_hip_mpc_kkt_solve_batch: slot k of `step` is what fbstab_hip_mpc_adjoint_batch(..., adj) returns for
 * seed k, V (dz, dl, dv) = (gz, -gl, -C gv).  Right-hand side 0 is that call's arithmetic to the bit; the others run
 * the same recursions on the same factors, without the matrix work.
 *   nrhs:   right-hand sides per QP, >= 1 (below: FBSTAB_HIP_ERR_ARGUMENT).
 *   seed:   nrhs vectors (gz, gl, gv) per QP: vector k of QP q of slot i at base[i] + q stride[i] + k rhs_stride[i].
 *           The l and v slots may be NULL (zero).  A slot with stride 0 is ONE block of nrhs vectors shared by the
 *           batch (the identity on the u0 rows, say).
 *   step:   nrhs vectors (dz, dl, dv) per QP, laid out the same way; NULL slots are skipped.  Every QP needs its own.
 *   strides, with batch > 1 or nrhs > 1: rhs_stride >= length, and stride >= (nrhs - 1) rhs_stride + length (or 0
 *           for a seed slot); anything else is FBSTAB_HIP_ERR_ARGUMENT.  The doubles between a QP's vectors
 *           (rhs_stride > length) are not written.
 *   status: per QP, 0, or 1 where the factorisation failed: every right-hand side's step of that QP is zero.
 * fbstab_hip_mpc_x0_sensitivity_batch: nrhs = nx, right-hand side j the tangent's for dx0 = e_j (gz = 0, gl = -e_j
 * in the l_0 block, gv = 0), generated in the kernel: slot j of `step` is fbstab_hip_mpc_tangent_batch's dx for the
 * direction x0 = e_j, bitwise what fbstab_hip_mpc_kkt_solve_batch returns for those seeds.
 *   step:   NULL, or as above with nrhs = nx; NULL slots are skipped.
 *   gain:   NULL, or nu x nx doubles per QP (QP q at gain + q gain_stride, gain_stride >= nu nx when batch > 1),
 *           column-major: du0/dx0, the u0 rows of stage 0 of the dz columns, written by the kernel whether or not
 *           the dz slot is taken.  At a point where no constraint is active this is -K_0 of the Riccati recursion.
 * sigma, flags, streams, host-pointer staging (a host-pointer call stages the seed and step blocks packed, in
 * allocations of the call), where `status` lives, batch == 0 (OK, nothing is queued) are those of
 * fbstab_hip_mpc_adjoint_batch.  Validation: what needs no handle comes first - nrhs, the NULL blocks, a NULL z seed,
 * strides no length could satisfy - then the handle and what takes its lengths; everything before any device call.
 * Memory: the kernel runs in the flat-vector workspace (MpcLayout::ws_doubles per workgroup).  A flat-vector handle
 * has it.  A record handle runs it in the scratch of the flat-vector adjoint, which a record handle whose adjoint is
 * on the record (fbstab_hip_mpc_adjoint_kernel_name) has not allocated yet: the first call then allocates it, as
 * documented for the flat adjoint above (ws_doubles x the handle's workgroups, held until destroy, not counted in
 * fbstab_hip_mpc_query's scratch_bytes).  The record handle's own scratch is not touched: the matrix copies of a
 * FBSTAB_HIP_KEEP_MATRICES solve stay valid across these calls.  fbstab_hip_mpc_last_kernel_ms reports the launch. */
typedef struct fbstab_multi_var_batch_t { /* nrhs vectors (z, l, v) per QP */
  double* base[3];
  long long stride[3];     /* between QPs */
  long long rhs_stride[3]; /* between the vectors of one QP */
} fbstab_multi_var_batch_t;
int fbstab_hip_mpc_kkt_solve_batch(fbstab_mpc_handle_t handle, int batch, const fbstab_mpc_batch_t* data,
                                   const fbstab_var_batch_t* x, int nrhs, const fbstab_multi_var_batch_t* seed,
                                   double sigma, const fbstab_multi_var_batch_t* step, int* status, int flags,
                                   void* stream);
int fbstab_hip_mpc_x0_sensitivity_batch(fbstab_mpc_handle_t handle, int batch, const fbstab_mpc_batch_t* data,
                                        const fbstab_var_batch_t* x, double sigma,
                                        const fbstab_multi_var_batch_t* step, double* gain, long long gain_stride,
                                        int* status, int flags, void* stream);

/* ---- condensing: an MPC QP as a dense QP in its inputs, on the device --------------------------------------
 * For state-heavy shapes (nx above what a record instance takes, few inputs, a short horizon) the states can be
 * eliminated through the dynamics: with U = (u_0 .. u_N), u_i at [i nu, (i + 1) nu) - the u entries of z in their
 * order - and z = T U + t (xbar_0 = x0, xbar_(i+1) = A_i xbar_i + c_i, x_i = xbar_i + sum_(j<i) A_(i-1) .. A_(j+1)
 * B_j u_j) the MPC QP (H, f, G, h, A, b of mpc_data.cc) becomes the dense QP
 *   H_c = T'HT (nz x nz, column-major)   f_c = T'(Ht + f)   A_c = AT (nv x nz, column-major)   b_c = b - At
 * with nz = (N + 1) nu variables, no equalities and the nv = (N + 1) nc inequalities of the MPC QP in their order
 * (v_c = v and y_c = b_c - A_c U = b - Az, entry for entry), which a dense handle (nz, 0, nv) solves.  The
 * constant of the cost is dropped.  H_c is symmetric bit for bit: the blocks on and below the diagonal are
 * computed (Q_i and R_i are taken as symmetric, the diagonal blocks read the lower triangle of R_i) and mirrored.
 * The calls need no handle.  EVERY pointer is a DEVICE pointer (there is no host staging); the work is queued on
 * `stream` (NULL: the null stream of `device`) and the call returns, as a solve does under FBSTAB_HIP_ASYNC.
 *
 * fbstab_hip_mpc_condensed_sizes: nz and nv, and the dynamic LDS one workgroup of the kernels needs,
 *   lds_bytes = 8 (2 e(ldx nx) + e(ldx nu) + e(ldc nx) + e(ldu nx) + e(ldc nu) + e(ldu nu)
 *                  + e(max((N + 2) e(ldx nu), (N + 1)(nx + nu + nc) + 2 nx + 8)))
 *   with ldx = nx | 1, ldc = nc | 1, ldu = nu | 1 and e(n) = n rounded up to an even number:
 *   the images of one stage, and X_k = dx/du_k of a horizon.  A shape that needs more than 160 KB is
 *   FBSTAB_HIP_ERR_UNSUPPORTED (lds_bytes = 0), here and in the two calls below.  Output pointers may be NULL.
 * fbstab_hip_mpc_condense_batch:
 *   data:  as for fbstab_hip_mpc_solve_batch (all 12 sequences, a stride of 0 or at least the length).
 *   what:  FBSTAB_CONDENSE_MATRICES writes H and A only, FBSTAB_CONDENSE_VECTORS f and b only - the receding-
 *          horizon case, where only x0, q, r, c, d moved: a kernel of its own, O(N nx^2) per QP - and
 *          FBSTAB_CONDENSE_ALL all four; what VECTORS writes is bitwise what ALL writes into f and b.
 *   dense: the slots of H, f, A, b that `what` selects (the G and h slots are ignored: nl = 0; slots not
 *          selected may be NULL and are not touched).  A stride is at least the array length, except that H
 *          and A may have stride 0 when every one of Q, R, S, A, B, E, L has stride 0: ONE image is then
 *          computed, for a batch that shares its model (fbstab_hip_dense_solve_batch takes such a block).
 *          Anything else is FBSTAB_HIP_ERR_ARGUMENT.  The doubles between two QPs' images are not written.
 * fbstab_hip_mpc_expand_batch: the point of the MPC QP from the one of the condensed QP.
 *   xc:    base[0] = U, base[2] = v_c, base[3] = y_c (needed where x->base[3] is given); the l slot is unused.
 *   x:     receives (z, l, v, y): x_0 = x0, x_(i+1) = A_i x_i + B_i u_i + c_i, z the interleaved (x_i, u_i),
 *          v = v_c and y = y_c bit for bit, and the costates from the x rows of Hz + f + G'l + A'v = 0:
 *          l_i = Q_i x_i + S_i'u_i + q_i + E_i'v_i + A_i'l_(i+1), i = N .. 0.  NULL slots are skipped.
 *   The map is applied to whatever the dense solve returned.  It does NOT translate certificates: after an
 *   infeasibility exit of the condensed solve, v and y are the dense solve's and z and l certify nothing.
 * Both: sizes below 1, batch < 0, a NULL block or a NULL pointer that is needed, a stride outside the rules (with
 * batch > 1) and `what` outside 1..3 are FBSTAB_HIP_ERR_ARGUMENT, all checked before any device call; then the
 * device is checked (FBSTAB_HIP_ERR_DEVICE where there is none), then the LDS rule.  batch == 0 returns OK and
 * queues nothing.  Deterministic: one thread owns each output entry and sums it in an order the shape alone
 * fixes; a QP's bits do not depend on the batch it is in.  Not here: host pointers, sharded calls, partial
 * condensing, the C++ facade.  Derivatives on this route: the two sections below (the adjoint; many right-hand
 * sides and the x0 sensitivity). */
enum fbstab_condense_what { FBSTAB_CONDENSE_MATRICES = 1, FBSTAB_CONDENSE_VECTORS = 2, FBSTAB_CONDENSE_ALL = 3 };
typedef struct fbstab_dense_out_batch_t {
  double* base[FBSTAB_DENSE_NARR];
  long long stride[FBSTAB_DENSE_NARR];
} fbstab_dense_out_batch_t;
int fbstab_hip_mpc_condensed_sizes(int N, int nx, int nu, int nc, int* nz, int* nv, long long* lds_bytes);
int fbstab_hip_mpc_condense_batch(int N, int nx, int nu, int nc, int batch, const fbstab_mpc_batch_t* data, int what,
                                  const fbstab_dense_out_batch_t* dense, int device, void* stream);
int fbstab_hip_mpc_expand_batch(int N, int nx, int nu, int nc, int batch, const fbstab_mpc_batch_t* data,
                                const fbstab_var_batch_t* xc, const fbstab_var_batch_t* x, int device, void* stream);

/* ---- the derivative of the condensed route -------------------------------------------------------------------
 * fbstab_hip_mpc_adjoint_batch for points that the condensed route returned, at the cost of that route: the adjoint
 * system V (dz, dl, dv) = (gz, -gl, -C gv) is the QP's own optimality system with the same matrices and the vectors
 *   q_i := -gz_x_i   r_i := -gz_u_i   x0 := -gl_0   c_i := -gl_(i+1)   d_i := -gv_i,
 * so it condenses as the QP does.  Six launches on one stream:
 *   1. fbstab_mpc_condense_seed_kernel: (f~, b~) = what FBSTAB_CONDENSE_VECTORS computes for those vectors; the
 *      seeds of the dense adjoint are gU = -f~ and gv_c = b~.  It also writes U, the u blocks of z.
 *   2. the launch of fbstab_hip_dense_adjoint_batch on the condensed QP (H_c, f_c, A_c, b_c) at (U, v) with the
 *      seeds (gU, gv_c): (dU, dv).  (y_c = y and v_c = v entry for entry: C and mus are those of the MPC QP.)
 *      Then one step of iterative refinement of that step: the dense adjoint eliminates dv into a matrix that
 *      carries 1 / sigma on active rows, so the z rows of its system come back with a residual at eps / sigma.
 *      fbstab_mpc_condensed_adjoint_residual_kernel computes rU = gU - (H_c dU + sigma dU + A_c'dv), the dense
 *      adjoint runs again with the seeds (rU, 0), and fbstab_mpc_condensed_adjoint_correct_kernel adds its step
 *      (eU, ev) to (dU, dv): what is left is eps / sigma of the correction.
 *   3. fbstab_mpc_condensed_adjoint_finish_kernel: (dz, dl) = what fbstab_hip_mpc_expand_batch computes for those
 *      vectors at (dU, dv) - dx_0 = -gl_0, dx_(i+1) = A_i dx_i + B_i du_i - gl_(i+1),
 *      dl_i = Q_i dx_i + S_i'du_i - gz_x_i + E_i'dv_i + A_i'dl_(i+1) - and the contraction of
 *      fbstab_hip_mpc_adjoint_batch: the gradients of the 12 sequences in the layout of fbstab_mpc_batch_t.
 * The step satisfies the u rows and the v rows of the MPC system exactly; the x rows are off by sigma dx and the
 * equality rows by sigma dl, so its residual is sigma ||(dx, dl)||_2: the derivative of the solution map with V
 * regularised in the condensed variables, a bias of O(sigma) like that of fbstab_hip_mpc_adjoint_batch (the two
 * agree to O(sigma), not bit for bit).
 *   handle: the dense handle ((N + 1) nu, 0, (N + 1) nc) that solves the condensed QP; the work runs on its device.
 *   data:   the MPC data, as for fbstab_hip_mpc_condense_batch.
 *   dense:  the condensed images H_c, f_c, A_c, b_c (the G and h slots are ignored); H_c and A_c may have stride
 *           0 for a batch that shares its model, as in the solve.
 *   x:      the point (z, l, v) of the MPC QP (the y slot is not read).
 *   seed:   (gz, gl, gv) in the MPC layout; the l and v slots may be NULL (zero).
 *   sigma:  as for fbstab_hip_dense_adjoint_batch (<= 0 selects 1e-8).
 *   grad:   one slot per sequence; a NULL slot is not computed, every other slot is written.
 *   adj:    NULL, or (dz, dl, dv) (its NULL slots are skipped).
 *   work:   caller-provided DEVICE memory, batch x (5 (N + 1) nu + 3 (N + 1) nc) doubles: U, gU, dU of
 *           (N + 1) nu and gv_c, dv of (N + 1) nc doubles per QP, then the refinement's rU, eU of (N + 1) nu and ev
 *           of (N + 1) nc, each one packed array of the batch in this order.  Nothing is allocated by the call.
 *   status: per QP, DEVICE memory: the dense adjoint's, 0, or 1 where its factorisation failed (the gradients
 *           and adj of that QP are zero).
 * EVERY pointer is a DEVICE pointer; the work is queued on `stream` (NULL: the handle's stream) and the call
 * returns.  All of these are FBSTAB_HIP_ERR_ARGUMENT and checked before any device call, what needs no handle
 * first, in the order of fbstab_hip_mpc_condense_batch: sizes below 1, batch < 0, a NULL block or a NULL pointer
 * that is needed, a stride below the length with batch > 1 (0 is allowed on the data and on H_c, A_c); then a NULL
 * handle, a handle whose (nz, nl, nv) is not ((N + 1) nu, 0, (N + 1) nc), and a batch above its max_batch.  Then
 * the device is checked, then the LDS rule of fbstab_hip_mpc_condensed_sizes (the seed and finish kernels run in that
 * layout; the two kernels of the refinement step use no LDS).
 * batch == 0 returns OK and queues nothing.  Deterministic as the condensing kernels are.  Not here: sums over the
 * batch on the device (the _reduced form; forward mode, the x0 sensitivities and many seeds per factorisation are the
 * sections below), the C++ facade, sharded calls, and certificates of
 * infeasibility, which this route does not translate. */
int fbstab_hip_mpc_condensed_adjoint_batch(fbstab_dense_handle_t handle, int N, int nx, int nu, int nc, int batch,
                                           const fbstab_mpc_batch_t* data, const fbstab_dense_batch_t* dense,
                                           const fbstab_var_batch_t* x, const fbstab_var_batch_t* seed,
                                           double sigma, const fbstab_mpc_grad_batch_t* grad,
                                           const fbstab_var_batch_t* adj, double* work, int* status, void* stream);

/* ---- the condensed route: forward mode ------------------------------------------------------------------------------
 * fbstab_hip_mpc_tangent_batch for points that the condensed route returned, at the cost of that route: the tangent
 * (dz, dl, dv) = J dtheta of the solution map along a perturbation `ddata` of the 12 sequences.  Seven launches on
 * one stream:
 *   1. fbstab_mpc_condensed_tangent_rhs_kernel, grid batch x (N + 1), one workgroup per (QP, stage): the seeds
 *      (gz, gl, gv) of the tangent system V dx = (gz, -gl, -C gv) from the perturbation and the point - the device
 *      function of fbstab_hip_mpc_tangent_batch's direction kernel (fb_tangent.h), and its bits;
 *   2. - 7. the six launches of fbstab_hip_mpc_condensed_adjoint_batch, unchanged, on those seeds, with every gradient
 *      slot NULL and adj = dx.
 * The step is the adjoint's: V regularised in the condensed variables alone, a bias of O(sigma), and dual to the
 * adjoint's gradient table, <g, J dtheta> = sum_k <grad_k(g), dtheta_k>, up to rounding.
 *   handle, data, dense, x, sigma, status, stream: exactly as for fbstab_hip_mpc_condensed_adjoint_batch.
 *   ddata: as for fbstab_hip_mpc_tangent_batch - one slot per sequence; a NULL slot is a zero perturbation, neither
 *          read nor multiplied; stride 0 is one direction shared by the batch, any other stride below the length with
 *          batch > 1 is FBSTAB_HIP_ERR_ARGUMENT.  dQ and dR enter through their symmetric part.
 *   dx:    receives (dz, dl, dv); all three slots are needed (the y slot is unused).
 *   rhs:   NULL, or it receives the seeds (gz, gl, gv) (all three slots): the direction kernel writes them into the
 *          caller's arrays and the chain reads them there.  With rhs NULL they live in the tail of `work`.
 *   work:  caller-provided DEVICE memory, batch x (5 (N + 1) nu + 3 (N + 1) nc + nz + nl + nv) doubles with nz =
 *          (N + 1)(nx + nu), nl = (N + 1) nx, nv = (N + 1) nc: the adjoint's work array, then gz, gl, gv, each one
 *          packed array of the batch in this order.  Nothing is allocated by the call.
 *   status: per QP, 0, or 1 where the dense factorisation failed (dx of that QP is zero), as in the adjoint.
 * EVERY pointer is a DEVICE pointer; the work is queued on `stream` and the call returns.  Deterministic: a QP's bits
 * depend on its own inputs and the shape alone, not on the batch, its place in it, or the grid.
 * Checked in this order, everything before any device call: what needs no handle, in the order of
 * fbstab_hip_mpc_condense_batch - the sizes, the batch and the data block; a NULL dense, x, ddata, dx, work or status;
 * the condensed images; per vector the point's, dx's and rhs's pointer and stride; the strides of ddata - then the
 * handle (NULL, not ((N + 1) nu, 0, (N + 1) nc), batch above max_batch).  batch == 0 returns OK and queues nothing.
 * Then the device, then the LDS rule of fbstab_hip_mpc_condensed_sizes, then the direction kernel's own limits: its
 * stage layout (fb_tangent.h: MpcTangentLds) above 160 KB is FBSTAB_HIP_ERR_UNSUPPORTED, batch x (N + 1) above
 * INT_MAX is FBSTAB_HIP_ERR_ARGUMENT.
 * Not here: several directions per factorisation, the device-side reduced form, the C++ facade, sharded calls,
 * certificates of infeasibility.  (Forward mode through the closed-loop sweep:
 * fbstab_hip_mpc_condensed_receding_sweep_tangent.) */
int fbstab_hip_mpc_condensed_tangent_batch(fbstab_dense_handle_t handle, int N, int nx, int nu, int nc, int batch,
                                           const fbstab_mpc_batch_t* data, const fbstab_dense_batch_t* dense,
                                           const fbstab_var_batch_t* x, const fbstab_mpc_batch_t* ddata, double sigma,
                                           const fbstab_var_batch_t* dx, const fbstab_var_batch_t* rhs, double* work,
                                           int* status, void* stream);

/* ---- the condensed route: many right-hand sides per factorisation, and the x0 sensitivity ------------------------
 * fbstab_hip_mpc_kkt_solve_batch and fbstab_hip_mpc_x0_sensitivity_batch for points that the condensed route
 * returned, at the cost of that route.  The adjoint system condenses as the QP does (the section above), and
 * fbstab_hip_dense_kkt_solve_batch factors the condensed K once for nrhs right-hand sides; these calls put the two
 * maps around it for many right-hand sides at once (fb_condense_multi.h).  Six launches on one stream, every
 * kernel of this section on the grid batch x ceil(nrhs / R), R right-hand sides per workgroup:
 *   1. fbstab_mpc_condense_multi_seed_kernel: (gU, gv_c) of every right-hand side, the map of
 *      fbstab_mpc_condense_seed_kernel.  A stage's images are staged into LDS once per workgroup and used by its R
 *      right-hand sides; thread (row r, right-hand side k) owns entry r of right-hand side k.  The workgroup that
 *      holds right-hand side 0 also writes U.
 *   2. fbstab_hip_dense_kkt_solve_batch (device pointers, async, nrhs) on (gU, gv_c): (dU, dv);
 *   3. fbstab_mpc_condense_multi_residual_kernel: rU = gU - (H_c dU + sigma dU + A_c'dv) per right-hand side;
 *   4. the dense multi-solve again on (rU, 0): (eU, ev);
 *   5. fbstab_mpc_condense_multi_correct_kernel: (dU, dv) += (eU, ev), and `gain` in x0 mode;
 *   6. fbstab_mpc_condense_multi_finish_kernel: the sweeps of fbstab_mpc_condensed_adjoint_finish_kernel without
 *      the contraction - dx_0 = -gl_0, dx_(i+1) = A_i dx_i + B_i du_i - gl_(i+1), then dl backwards - written into
 *      the caller's step slots.  Not queued when the x0 call is asked for `gain` alone (step == NULL).
 * The refinement step (3 - 5) is the adjoint's, for its reason: the dense multi-solve leaves eps / sigma on the z rows.
 * fbstab_hip_mpc_condensed_kkt_solve_batch: slot k of `step` is what fbstab_hip_mpc_condensed_adjoint_batch(..., adj)
 *   solves for seed k - the condensed chain with its O(sigma) bias, not the flat-vector system.  A right-hand side's
 *   bits depend on its seed, the QP's data and the shape alone: not on its slot, the other seeds, nrhs, the batch or
 *   rhs_per_group.
 * fbstab_hip_mpc_condensed_x0_sensitivity_batch: nrhs = nx, right-hand side j the tangent's for dx0 = e_j (gz = 0,
 *   gl = -e_j in the l_0 block, gv = 0: the signs of fbstab_hip_mpc_x0_sensitivity_batch), generated in the kernels:
 *   bitwise what the kkt-solve entry returns for those explicit seeds.
 *   step:  NULL, or nrhs = nx vectors per QP; NULL slots are skipped.  step and gain both NULL: ARGUMENT.
 *   gain:  NULL, or nu x nx doubles per QP, column-major (QP q at gain + q gain_stride, gain_stride >= nu nx when
 *          batch > 1): du0/dx0, the u_0 rows of dU, bitwise the u_0 rows of the dz columns.
 * nrhs, seed, step, their strides (stride, rhs_stride, NULL l / v seed slots, a seed slot of stride 0 shared by the
 * batch, the untouched doubles between vectors) and gain's layout: those of fbstab_hip_mpc_kkt_solve_batch /
 * _x0_sensitivity_batch, word for word, with the lengths of the MPC QP ((N + 1)(nx + nu), (N + 1) nx, (N + 1) nc).
 * handle, data, dense, x, sigma, status (1: every slot of every right-hand side of that QP is zero), DEVICE
 * pointers only, the stream, batch == 0: those of fbstab_hip_mpc_condensed_adjoint_batch.
 *   rhs_per_group: R.  0: the library's rule, R = clamp(256 / nx, 1, nrhs), lowered until lds_bytes <= 80 KB (two
 *          workgroups per CU).  A value above nrhs is nrhs.  Below 0: ARGUMENT.  R changes speed, never results.
 *   work:  caller-provided DEVICE memory, batch x work_doubles_per_qp doubles: U of (N + 1) nu doubles per QP, then
 *          gU, dU, rU, eU of nrhs (N + 1) nu and gv_c, dv, ev of nrhs (N + 1) nc, each one packed [batch][nrhs][n]
 *          array in this order.  Nothing is allocated by the call.
 * fbstab_hip_mpc_condensed_multi_sizes: what the calls will use, with e(n) = n rounded up to even:
 *   per       = max(e((N + 1) nx) + 2 e(nx),  e((N + 1)(nx + nu)) + e((N + 1) nc) + 2 e(nx))   (one right-hand side's
 *               vectors in the seed and in the finish kernel)
 *   window    = 2 e(ldx nx) + e(ldx nu) + e(ldc nx) + e(ldu nx) + e(ldc nu) + e(ldu nu), ldx = nx | 1, ldc = nc | 1,
 *               ldu = nu | 1: the stage window of fbstab_hip_mpc_condensed_sizes
 *   lds_bytes = 8 (window + rhs_per_group_used per)
 *   work_doubles_per_qp = (N + 1) nu + nrhs (4 (N + 1) nu + 3 (N + 1) nc)
 *   Sizes or nrhs below 1 and rhs_per_group below 0 are FBSTAB_HIP_ERR_ARGUMENT; lds_bytes above 160 KB is
 *   FBSTAB_HIP_ERR_UNSUPPORTED (outputs 0).  Output pointers may be NULL.  Pass nrhs = nx for the x0 call.
 * Validation of the two calls, everything before any device call: what needs no handle first - the sizes, the batch
 * and the data block as fbstab_hip_mpc_condense_batch; nrhs, the NULL blocks and a NULL z seed (kkt solve), step and
 * gain both NULL (x0); NULL dense, x, work, status; the condensed images; x; the seed and step strides; gain_stride;
 * rhs_per_group < 0 - then the handle (NULL, not ((N + 1) nu, 0, (N + 1) nc), batch above max_batch), then the
 * device, then the LDS rule (FBSTAB_HIP_ERR_UNSUPPORTED).
 * Not here: the device-side reduced form, a dense factor kept between
 * the two dense launches, the C++ facade, sharded calls, certificates of infeasibility. */
int fbstab_hip_mpc_condensed_multi_sizes(int N, int nx, int nu, int nc, int nrhs, int rhs_per_group,
                                         int* rhs_per_group_used, long long* lds_bytes,
                                         long long* work_doubles_per_qp);
int fbstab_hip_mpc_condensed_kkt_solve_batch(fbstab_dense_handle_t handle, int N, int nx, int nu, int nc, int batch,
                                             const fbstab_mpc_batch_t* data, const fbstab_dense_batch_t* dense,
                                             const fbstab_var_batch_t* x, int nrhs,
                                             const fbstab_multi_var_batch_t* seed, double sigma,
                                             const fbstab_multi_var_batch_t* step, int rhs_per_group, double* work,
                                             int* status, void* stream);
int fbstab_hip_mpc_condensed_x0_sensitivity_batch(fbstab_dense_handle_t handle, int N, int nx, int nu, int nc,
                                                  int batch, const fbstab_mpc_batch_t* data,
                                                  const fbstab_dense_batch_t* dense, const fbstab_var_batch_t* x,
                                                  double sigma, const fbstab_multi_var_batch_t* step, double* gain,
                                                  long long gain_stride, int rhs_per_group, double* work, int* status,
                                                  void* stream);

/* ---- the condensed route in closed loop: sweeps on an affine map of x0 ---------------------------------------------
 * In a receding-horizon sweep the matrix sequences and q, r, c, d stand and only x0 moves: H_c and A_c stand, and
 *   f_c(x) = f_c(0) + F x     b_c(x) = b_c(0) + G x      F: (N + 1) nu x nx,  G: (N + 1) nc x nx
 * (the explicit-MPC form of the condensed QP; fb_condense_sweep.h has the derivation).  Re-condensing for a new state
 * is then one ((N + 1)(nu + nc)) x nx matrix-vector product per trajectory, fused into the plant step.
 *
 * fbstab_hip_mpc_condensed_x0_map_batch: the image M = [F; G] of every QP, once per sweep, O(N nx^3) per QP.
 *   map:   ne x nx doubles per QP, ne = (N + 1)(nu + nc), COLUMN-MAJOR with leading dimension ne: rows 0 .. (N + 1) nu
 *          are F in the order of U, the rest G in the order of v.  QP q at map + q map_stride, map_stride >= ne nx with
 *          batch > 1, or 0 where every one of Q, R, S, A, B, E, L has stride 0: ONE image is then computed, bitwise the
 *          image of QP 0.  The doubles between two images are not written.
 *   G[i] = -E_i Phi_i,  F[k] = S_k Phi_k + B_k' P_(k+1),  P_i = Q_i Phi_i + A_i' P_(i+1) (P_(N+1) = 0; no B' term at
 *   k = N),  Phi_0 = I, Phi_(i+1) = A_i Phi_i.  One workgroup per (QP, block of at most nu columns of x0), in the LDS
 *   layout of fbstab_hip_mpc_condensed_sizes, which stays the only shape limit.
 *   f_c(0) and b_c(0) are fbstab_hip_mpc_condense_batch(VECTORS) with the x0 slot pointing at nx zeros, stride 0.
 *   Validation: that of fbstab_hip_mpc_condense_batch, then a NULL map and map_stride (ARGUMENT), before any device
 *   call; then the device, then the LDS rule.  batch == 0 returns OK and queues nothing.
 *
 * fbstab_hip_mpc_condensed_receding_sweep: `steps` closed-loop steps on one stream without a host round trip -
 * per step the dense solve (device pointers, FBSTAB_HIP_ASYNC) and fbstab_mpc_condensed_sweep_step_kernel, which for
 * the T trajectories of a workgroup
 *   1. reads eflag and newton_iters of the dense `out` record; with retire != 0 a trajectory whose solve did not end
 *      in SUCCESS is gone for the rest of the sweep: U = 0, v = 0, u0 = 0, x = 0, and a logged eflag of -1;
 *   2. writes the logs that are given;
 *   3. advances the plant, x+ = A_p x + B_p u0 (+ w_k), summed in the order of fbstab_hip_mpc_receding_sweep's plant
 *      step, and writes it in place into data->base[FBSTAB_MPC_x0];
 *   4. with scenario->shift == 1 moves U and v one stage towards the present (U[i] <- U[i+1], v[i] <- v[i+1], i < N;
 *      stage N keeps its values);
 *   5. AFFINE mode: f_c[e] = f_c(0)[e] + sum_j F[e][j] x+[j], b_c likewise, j ascending, one thread per entry.  A
 *      shared M (stride 0) is staged into LDS once per workgroup with the leading dimension ne | 1 where it fits
 *      beside one trajectory in 80 KB, and is read from memory otherwise, as every per-QP M is.
 *      RECONDENSE mode: the VECTORS launch of fbstab_hip_mpc_condense_batch is queued behind the step kernel instead:
 *      the sweep is then bitwise a loop over the public calls.
 * 4 and 5 do not follow the last step: on return dense->f and dense->b are those of the LAST step's QP.  One
 * fbstab_hip_mpc_expand_batch, with x0 pointing at the work copy of the state the last step was solved for, follows.
 *   handle: the dense handle ((N + 1) nu, 0, (N + 1) nc).
 *   data:   the MPC data; every trajectory needs its own x0 (stride >= nx with batch > 1), advanced in place to the
 *           state behind the last step.  The other sequences are read by RECONDENSE mode and the final expand.
 *   dense:  the images H_c, f_c, A_c, b_c as fbstab_hip_mpc_condensed_adjoint_batch takes them.  On entry they are
 *           those of `data` (fbstab_hip_mpc_condense_batch(ALL)); f_c and b_c (stride >= length with batch > 1) are
 *           overwritten before every step but the first.
 *   map:    M, f0 = f_c(0), b0 = b_c(0); stride 0 shares one array among the batch, otherwise >= the length with
 *           batch > 1.  May be NULL in RECONDENSE mode.
 *   x:      (z, l, v, y) of the MPC QP.  The guess is read as the condensed solve reads it - U = the u blocks of z,
 *           and v - and on return x holds the expanded point of the LAST step (zeros of U and v for a gone trajectory).
 *   out:    DEVICE array of batch records: the dense solver's of the last step.
 *   plant:  DEVICE matrices as for fbstab_hip_mpc_receding_sweep.
 *   scenario: NULL, or (w, shift) as for fbstab_hip_mpc_receding_sweep_scenario.
 *   mode:   FBSTAB_CONDENSED_SWEEP_AFFINE or FBSTAB_CONDENSED_SWEEP_RECONDENSE.
 *   log:    NULL, or DEVICE arrays, NULL slots not logged: u [steps][batch][nu], x [steps][batch][nx] (the state the
 *           step was solved for), U [steps][batch][(N + 1) nu] and v [steps][batch][(N + 1) nc] (the returned condensed
 *           point, zero once gone), eflag and newton (int32 [steps][batch]; eflag -1 once gone).  There is no host
 *           `stats` array: the logs carry what it carried.
 *   traj_per_group: T.  0: the library's rule, ceil(1024 / ne) clamped to 1 .. 64 and lowered until the workgroup's
 *           LDS is at most 80 KB.  T changes speed and never a bit of any result, and neither does the batch a
 *           trajectory sits in.  Below 0: ARGUMENT.
 *   work:   caller-provided DEVICE memory, batch x work_doubles_per_traj doubles: U, v, y of the dense solve, the
 *           state of the last step, the gone flags - packed arrays of the batch in this order.  Nothing is allocated.
 * EVERY pointer is a DEVICE pointer.  Asynchronous: steps x (dense solve, step kernel[, vectors launch]) and the
 * expand are queued on `stream` (NULL: the handle's stream) and the call returns; nothing synchronises with the host.
 * Every argument error is FBSTAB_HIP_ERR_ARGUMENT and checked before any device call, what needs no handle first:
 * the sizes, the batch and the data block as fbstab_hip_mpc_condense_batch; NULL dense, x, out, plant, work; steps < 0;
 * shift outside 0..1; mode outside its enum; traj_per_group < 0; the x0 stride; the condensed images; x; the plant; the
 * map (NULL in AFFINE mode, NULL slots, strides) - then the handle (NULL, not ((N + 1) nu, 0, (N + 1) nc), batch above
 * max_batch).  batch == 0 or steps == 0 returns OK here and queues nothing.  Then the device, then the LDS rule of
 * fbstab_hip_mpc_condensed_sizes.
 * fbstab_hip_mpc_condensed_sweep_sizes: what the sweep will use for traj_per_group (shared_map != 0: one M with
 * stride 0 in AFFINE mode, which is staged into LDS; 0: per-QP images or RECONDENSE mode), with e(n) = n rounded up
 * to even:
 *   lds_bytes = 8 (staged M: e((ne | 1) nx)  +  T (2 e(nx) + e((N + 1) nu) + e((N + 1) nc) + 2))
 *   work_doubles_per_traj = (N + 1) nu + 2 (N + 1) nc + nx + 1
 *   Sizes below 1 and traj_per_group below 0 are ARGUMENT; lds_bytes above 160 KB (a traj_per_group the caller chose)
 *   is FBSTAB_HIP_ERR_UNSUPPORTED (outputs 0).  Output pointers may be NULL.
 * Not here: sharded sweeps, the C++ facade.  (Per-step references - q, r, c, d that move along the sweep - are
 * fbstab_hip_mpc_condensed_tracking_sweep, and the derivative through the sweep is the section below: this call's logs
 * are its base.) */
enum fbstab_condensed_sweep_mode { FBSTAB_CONDENSED_SWEEP_AFFINE = 0, FBSTAB_CONDENSED_SWEEP_RECONDENSE = 1 };
typedef struct fbstab_condensed_map_t {
  const double* M;      /* [F; G], ne x nx column-major */
  const double* f0;     /* f_c(0), (N + 1) nu */
  const double* b0;     /* b_c(0), (N + 1) nc */
  long long stride_M, stride_f0, stride_b0;   /* doubles between trajectories; 0 = one for all */
} fbstab_condensed_map_t;
typedef struct fbstab_condensed_sweep_log_t {
  double *u, *x, *U, *v;
  int *eflag, *newton;
} fbstab_condensed_sweep_log_t;
int fbstab_hip_mpc_condensed_sweep_sizes(int N, int nx, int nu, int nc, int traj_per_group, int shared_map,
                                         int* traj_per_group_used, long long* lds_bytes,
                                         long long* work_doubles_per_traj);
int fbstab_hip_mpc_condensed_x0_map_batch(int N, int nx, int nu, int nc, int batch, const fbstab_mpc_batch_t* data,
                                          double* map, long long map_stride, int device, void* stream);
int fbstab_hip_mpc_condensed_receding_sweep(fbstab_dense_handle_t handle, int N, int nx, int nu, int nc, int batch,
                                            const fbstab_mpc_batch_t* data, const fbstab_dense_batch_t* dense,
                                            const fbstab_condensed_map_t* map, const fbstab_var_batch_t* x,
                                            fbstab_solver_out_t* out, const fbstab_receding_plant_t* plant, int steps,
                                            int retire, const fbstab_sweep_scenario_t* scenario, int mode,
                                            const fbstab_condensed_sweep_log_t* log, int traj_per_group, double* work,
                                            void* stream);

/* ---- the condensed route in closed loop: reverse mode through the sweep -------------------------------------------
 * fbstab_hip_mpc_receding_sweep_adjoint for sweeps of fbstab_hip_mpc_condensed_receding_sweep, at the cost of that
 * route.  With u_k = U_k[0:nu] and x_(k+1) = A_p x_k + B_p u_k (+ w_k), the seeds gu[k] = dL/du_k ([steps][batch][nu])
 * and gx[k] = dL/dx_(k+1) ([steps][batch][nx]; either may be NULL: zero) are taken backwards along every trajectory.
 * Start with lambda = 0 and for k = steps-1 .. 0:
 *   mu = gx[k] + lambda                             (mu_log[k] = mu where mu_log is given)
 *   eflag_log[k] == -1 (retired):       lambda <- 0
 *   eflag_log[k] != FBSTAB_SUCCESS:     lambda <- A_p'mu
 *   otherwise one dense adjoint (fbstab_hip_dense_adjoint_batch's, same sigma rule) of the condensed QP at the logged
 *   (U_k, v_k) with the seed gU = (gu[k] + B_p'mu, 0, .., 0) and gv_c = 0 - the seed map of
 *   fbstab_hip_mpc_condensed_adjoint_batch is the identity on a seed that lives on u_0 alone, so no seed kernel runs -
 *   refined once exactly as that call refines it (residual kernel, the dense adjoint again, correction kernel):
 *     a factorisation failed in either launch:   status += 1, lambda <- A_p'mu
 *     else                                       lambda <- A_p'mu + F'(-dU) + G'dv.
 * The dense adjoint's gradients are f_bar = -dU and b_bar = dv, and f_c = f0 + F x, b_c = b0 + G x: F'(-dU) + G'dv is
 * -dl[0:nx] of fbstab_hip_mpc_condensed_adjoint_batch's finish, without the finish.  The affine map M = [F; G] that
 * makes the forward step one matrix-vector product makes the backward step its transpose.
 * fbstab_mpc_condensed_sweep_adjoint_step_kernel (T trajectories per workgroup in the LDS layout of the forward step
 * kernel) is launched steps + 1 times: one launch CLOSES step k + 1 - the case rule and
 * lambda[j] = sum_r A_p[r][j] mu[r] + sum_e M[e][j] g[e], g = [-dU; dv], e ascending, one thread per (trajectory, j) -
 * and OPENS step k: mu, the seed, and f_c, b_c of step k from x_log[k] with the forward kernel's loop and summation
 * order.  Between two launches: the dense adjoint, fbstab_mpc_condensed_adjoint_residual_kernel, the dense adjoint
 * again, fbstab_mpc_condensed_adjoint_correct_kernel, and - only where a gradient other than x0's is wanted, or in
 * RECONDENSE mode - fbstab_mpc_condensed_sweep_adjoint_finish_kernel (one workgroup per trajectory in the LDS layout of
 * fbstab_hip_mpc_condensed_sizes): the logged point is expanded with x0 := x_log[k] into scratch in `work`, and the
 * finish of fbstab_hip_mpc_condensed_adjoint_batch ADDS the step's gradients to the slots, by the thread that zeroed
 * the entry (fbstab_mpc_condensed_sweep_adjoint_begin_kernel, before the first step).
 *   handle, data, dense, map, plant: as fbstab_hip_mpc_condensed_receding_sweep takes them.  data's x0 slot is not read.
 *           dense's H_c and A_c are read; f_c and b_c (stride >= length with batch > 1) are per-trajectory scratch
 *           that the call overwrites.  map may be NULL in RECONDENSE mode.
 *   retire: the forward's (the logged eflag of -1 carries what it did).
 *   log:    the forward's; x, U, v and eflag are required.  U and v are read where they lie, no copy is made.
 *   grad:   one slot per sequence, NULL: not computed.  The x0 slot receives the final lambda = dL/dx_0 (not a sum
 *           over the steps); every other slot is the sum over the contributing steps, last step first, without atomics
 *           (the same inputs give the same bits).  Every non-NULL slot is written (zeros for a trajectory without a
 *           contributing step) and needs stride >= length with batch > 1 (stride 0 is FBSTAB_HIP_ERR_ARGUMENT: sums over
 *           the batch are the caller's).
 *   gf0, gb0: NULL, or packed [batch][(N + 1) nu], [batch][(N + 1) nc]: the sums of f_bar = -dU and b_bar = dv over the
 *           contributing steps, the gradients of the map's f0 and b0.
 *   mu_log: NULL, or [steps][batch][nx].  dL/dw_k = mu_log[k] where eflag_log[k] != -1, zero otherwise; the plant's own
 *           gradients are the caller's: A_bar = sum_k mu_k x_k', B_bar = sum_k mu_k u_k'.
 *   status: [batch], the number of steps whose factorisation failed.
 *   mode:   FBSTAB_CONDENSED_SWEEP_AFFINE: f_c, b_c of a step and lambda through the map.
 *           FBSTAB_CONDENSED_SWEEP_RECONDENSE: the VECTORS launch of fbstab_hip_mpc_condense_batch is queued with the
 *           x0 slot on x_log[k] - a step then sees bit for bit the images a loop over the public calls gives it - the
 *           finish kernel runs at every step, and lambda <- A_p'mu - dl[0:nx] with its dl.
 *   traj_per_group: T of the step kernel, as in the forward call: it changes speed, never a bit.
 *   work:   caller-provided DEVICE memory, batch x work_doubles_per_traj doubles (the _grad figure where a gradient
 *           other than x0's is wanted or in RECONDENSE mode), packed arrays of the batch.  Nothing is allocated.
 * EVERY pointer is a DEVICE pointer.  Asynchronous: everything is queued on `stream` (NULL: the handle's stream) and the
 * call returns.  Every argument error is FBSTAB_HIP_ERR_ARGUMENT and checked before any device call, what needs no
 * handle first, in the order of fbstab_hip_mpc_condensed_receding_sweep: the sizes, the batch and the data block; NULL
 * dense, plant, log, grad, status, work; steps < 0; mode; traj_per_group < 0; the condensed images; the plant; the
 * required log slots; the gradient strides; the map (AFFINE mode) - then the handle.  batch == 0 returns OK and queues
 * nothing; steps == 0 writes zeros to every non-NULL output slot and returns OK.
 * fbstab_hip_mpc_condensed_sweep_adjoint_sizes: with e(n) = n rounded up to even, nzc = (N + 1) nu, nv = (N + 1) nc,
 *   lds_bytes = that of fbstab_hip_mpc_condensed_sweep_sizes (the step kernel; shared_map as there)
 *   work_doubles_per_traj      = 4 nzc + 2 nv + 2 nx + 1     (gU, dU, rU, eU; dv, ev; mu, -dl0; two status words)
 *   work_doubles_per_traj_grad = that + 2 (N + 1)(nx + nu) + (N + 1) nx       (z and the zeros of gz; l)
 * Not here: the device-side reduced form for shared parameters, seeds on the rest of U_k and v_k, reuse of the forward
 * call's images and map, sharded calls, the C++ facade.  (Per-step references:
 * fbstab_hip_mpc_condensed_tracking_sweep_adjoint; forward mode through the sweep:
 * fbstab_hip_mpc_condensed_receding_sweep_tangent.) */
int fbstab_hip_mpc_condensed_sweep_adjoint_sizes(int N, int nx, int nu, int nc, int traj_per_group, int shared_map,
                                                 int* traj_per_group_used, long long* lds_bytes,
                                                 long long* work_doubles_per_traj,
                                                 long long* work_doubles_per_traj_grad);
int fbstab_hip_mpc_condensed_receding_sweep_adjoint(
    fbstab_dense_handle_t handle, int N, int nx, int nu, int nc, int batch, const fbstab_mpc_batch_t* data,
    const fbstab_dense_batch_t* dense, const fbstab_condensed_map_t* map, const fbstab_receding_plant_t* plant,
    int steps, int retire, const fbstab_condensed_sweep_log_t* log, const double* gu, const double* gx, double sigma,
    const fbstab_mpc_grad_batch_t* grad, double* gf0, double* gb0, double* mu_log, int* status, int mode,
    int traj_per_group, double* work, void* stream);

/* ---- the condensed route in closed loop: sweeps that track per-step references -------------------------------------
 * A controller that follows a moving set-point, a previewed trajectory or time-of-day bounds has q_k, r_k, d_k (and
 * sometimes c_k) that change at every closed-loop step.  H_c, A_c and the map M = [F; G] do not depend on q, r, c, d,
 * so step k solves
 *   f_c,k(x) = f0_k + F x        b_c,k(x) = b0_k + G x
 * with (f0_k, b0_k) what fbstab_hip_mpc_condense_batch(VECTORS) gives for x0 = 0 and the step's q_k, r_k, c_k, d_k.
 *
 * fbstab_condensed_refs_t: the sequences of every step.  Slot i (0 .. 3: q, r, c, d) of step k and trajectory b is at
 * base[i] + k step[i] + b stride[i]; a NULL base is the sequence of `data` at every step.  step >= 0, and windows may
 * overlap (the references are only read): step nx over one array of (steps + N) nx doubles is a sliding window over a
 * longer reference.  stride: 0 shares the rows among the batch, otherwise >= the sequence length with batch > 1.
 * fbstab_condensed_ref_images_t: f0_k at f0 + k step_f0 + b stride_f0, b0_k likewise.
 *
 * fbstab_hip_mpc_condensed_reference_images_batch: the images of all steps in ONE launch of
 * fbstab_mpc_condense_reference_kernel on the grid batch x ceil(steps / R): a workgroup serves R steps of one
 * trajectory, stages each stage's A, Q, S, B, E once for all of them and runs thread (row, reference).  Per reference
 * the operations and their order are those of the VECTORS kernel: the images are bit for bit those of
 * fbstab_hip_mpc_condense_batch(VECTORS) on the step's data with the x0 slot on a block of zeros, and neither R, the
 * batch nor the neighbouring steps change a bit.  Handle-free, DEVICE pointers only, asynchronous on `stream`.
 *   data:   the MPC data; its matrix sequences are read, q, r, c, d where refs has no slot, and x0 (checked like every
 *           slot) is not read.
 *   refs:   as above; NULL: every step is `data`'s.
 *   images: the outputs; every (step, trajectory) needs rows of its own: step >= the length with steps > 1 and stride
 *           >= the length with batch > 1.  The doubles between two images are not written.
 *   refs_per_group: R.  0: the library's rule, clamp(256 / nx, 1, steps), lowered until the LDS is at most 80 KB.
 * Validation (FBSTAB_HIP_ERR_ARGUMENT, before any device call): that of fbstab_hip_mpc_condense_batch; steps < 0;
 * refs_per_group < 0; the references (negative step or stride, a stride below the length that is not 0); the outputs.
 * batch == 0 or steps == 0 returns OK and queues nothing.  Then the device, then the LDS rule.
 * fbstab_hip_mpc_condensed_reference_sizes: what that call will use, with e(n) = n rounded up to even, ldx = nx | 1,
 * ldc = nc | 1, ldu = nu | 1:
 *   lds_bytes = 8 (2 e(ldx nx) + e(ldx nu) + e(ldc nx) + e(ldu nx) + e(ldc nu) + e(ldu nu)      the stage images
 *                  + R (e((N + 1) nx) + 2 e(nx)))                                    per reference: xbar and two p
 *   Sizes or steps below 1 and refs_per_group below 0 are ARGUMENT; lds_bytes above 160 KB is
 *   FBSTAB_HIP_ERR_UNSUPPORTED (outputs 0).  Output pointers may be NULL.
 *
 * fbstab_hip_mpc_condensed_tracking_sweep: fbstab_hip_mpc_condensed_receding_sweep where step k solves the QP of the
 * references' step k.  The arguments are that call's, plus
 *   refs:   the references of `steps` steps.  NULL: the call IS fbstab_hip_mpc_condensed_receding_sweep, bit for bit
 *           (`images` is not looked at).
 *   images: AFFINE mode with refs: f0_k, b0_k of every step as the call above writes them; they are READ (a stride of
 *           0 shares them among the batch).  map->f0 and map->b0 are then not looked at; map->M is.
 * On entry dense->f, dense->b are those of step 0's QP.  AFFINE mode: the step kernel of step k forms the vectors of
 * step k + 1 from f0[k + 1], b0[k + 1].  RECONDENSE mode: the VECTORS launch behind step k reads step k + 1's
 * sequences - the sweep is bitwise a loop over the public calls with the step's sequences.  The final expand uses the
 * LAST step's sequences.  The kernels are those of fbstab_hip_mpc_condensed_receding_sweep: only the pointers a launch
 * is handed differ.  Validation: that call's, in its order; in front of the handle checks the references as above, and
 * in AFFINE mode NULL images, NULL f0 or b0, negative steps, and strides below the length that are not 0.
 *
 * fbstab_hip_mpc_condensed_tracking_sweep_adjoint: fbstab_hip_mpc_condensed_receding_sweep_adjoint through a sweep of
 * the call above.  The lambda recursion does not change (M is the same at every step); the arguments are that call's
 * without gf0 and gb0, plus
 *   refs, images: the forward's.  NULL refs: the call IS the existing adjoint with gf0 = gb0 = NULL, bit for bit.
 *   ref_grad: NULL, or one slot per q, r, c, d, NULL where not wanted: dL/d(sequence of step k, trajectory b) at
 *           base[i] + k step[i] + b stride[i].  Every (step, trajectory) needs rows of its own: step >= the length with
 *           steps > 1, stride >= the length with batch > 1.  EVERY entry is written: a retired step, a step that did
 *           not end in SUCCESS and a step with a failed factorisation get zeros (one launch of the begin kernel per
 *           step zeroes the rows in front of the recursion).  A slot of a sequence that does not move (refs->base[i]
 *           NULL) is ARGUMENT: its gradient is grad's summed slot.
 *   grad:   as there for x0, the seven matrix sequences and those of q, r, c, d that do not move - summed over the
 *           contributing steps.  The slot of a sequence that moves is ARGUMENT.
 * Opening step k uses f0[k], b0[k]; in RECONDENSE mode the VECTORS launch uses step k's sequences.  The finish kernel at
 * step k sees step k's sequences (the expansion of the logged point needs q_k and c_k) and, for a sequence that
 * moves, step k's rows of ref_grad.  x0, mu_log, status and the case rule are unchanged, and so is the device code:
 * only the pointers a launch is handed differ.  Validation: the existing adjoint's, in its order; the references, their
 * images and ref_grad in front of the handle checks.
 * Not here: references on the record-kernel sweep, per-step gf0 / gb0, the device-side reduced form, sharded sweeps,
 * the C++ facade.  (Forward mode through a tracking sweep: fbstab_hip_mpc_condensed_receding_sweep_tangent with
 * `images`.) */
typedef struct fbstab_condensed_refs_t {       /* per-step q, r, c, d */
  const double* base[4];      /* q, r, c, d; NULL: the sequence of `data` at every step */
  long long step[4];          /* doubles between steps (>= 0; overlapping windows are allowed: read-only) */
  long long stride[4];        /* doubles between trajectories; 0 = one for all */
} fbstab_condensed_refs_t;
typedef struct fbstab_condensed_ref_images_t { /* f0_k, b0_k */
  double *f0, *b0;
  long long step_f0, step_b0, stride_f0, stride_b0;
} fbstab_condensed_ref_images_t;
typedef struct fbstab_condensed_ref_grad_t {   /* dL/d(q_k, r_k, c_k, d_k) */
  double* base[4];            /* NULL: not wanted */
  long long step[4];          /* doubles between steps (>= the length) */
  long long stride[4];        /* doubles between trajectories (>= the length) */
} fbstab_condensed_ref_grad_t;
int fbstab_hip_mpc_condensed_reference_sizes(int N, int nx, int nu, int nc, int steps, int refs_per_group,
                                             int* refs_per_group_used, long long* lds_bytes);
int fbstab_hip_mpc_condensed_reference_images_batch(int N, int nx, int nu, int nc, int batch, int steps,
                                                    const fbstab_mpc_batch_t* data,
                                                    const fbstab_condensed_refs_t* refs,
                                                    const fbstab_condensed_ref_images_t* images, int refs_per_group,
                                                    int device, void* stream);
int fbstab_hip_mpc_condensed_tracking_sweep(fbstab_dense_handle_t handle, int N, int nx, int nu, int nc, int batch,
                                            const fbstab_mpc_batch_t* data, const fbstab_dense_batch_t* dense,
                                            const fbstab_condensed_map_t* map, const fbstab_var_batch_t* x,
                                            fbstab_solver_out_t* out, const fbstab_receding_plant_t* plant, int steps,
                                            int retire, const fbstab_sweep_scenario_t* scenario, int mode,
                                            const fbstab_condensed_sweep_log_t* log,
                                            const fbstab_condensed_refs_t* refs,
                                            const fbstab_condensed_ref_images_t* images, int traj_per_group,
                                            double* work, void* stream);
int fbstab_hip_mpc_condensed_tracking_sweep_adjoint(
    fbstab_dense_handle_t handle, int N, int nx, int nu, int nc, int batch, const fbstab_mpc_batch_t* data,
    const fbstab_dense_batch_t* dense, const fbstab_condensed_map_t* map, const fbstab_receding_plant_t* plant,
    int steps, int retire, const fbstab_condensed_sweep_log_t* log, const double* gu, const double* gx, double sigma,
    const fbstab_mpc_grad_batch_t* grad, double* mu_log, int* status, int mode, const fbstab_condensed_refs_t* refs,
    const fbstab_condensed_ref_images_t* images, const fbstab_condensed_ref_grad_t* ref_grad, int traj_per_group,
    double* work, void* stream);

/* ---- the condensed route in closed loop: forward mode through the sweep -------------------------------------------
 * How does the whole closed-loop trajectory move along ONE direction of x0, the disturbances and the vectors of the
 * condensed QP?  The forward-mode counterpart of fbstab_hip_mpc_condensed_receding_sweep_adjoint (and, with `images`,
 * of fbstab_hip_mpc_condensed_tracking_sweep_adjoint), on the same logs.  AFFINE mode is the contract: step k solved
 * (H_c, f_c = f0_k + F x_k, A_c, b_c = b0_k + G x_k), u_k = U_k[0:nu], x_(k+1) = A_p x_k + B_p u_k (+ w_k).
 * fbstab_condensed_sweep_dir_t, the directions:
 *   dx0:    [batch][nx] at dx0 + b stride_dx0 (stride 0: one for the batch); NULL: zero.
 *   dw:     [steps][batch][nx], packed; NULL: zero.
 *   df0, db0: the directions of f0_k, b0_k in the layout of fbstab_condensed_ref_images_t: step k, trajectory b at
 *           df0 + k step_df0 + b stride_df0.  A step of 0: one direction for all steps; a stride of 0: shared by the
 *           batch; NULL: zero.
 * Start with dx = dx0 and for k = 0 .. steps-1:
 *   eflag_log[k] == -1 (retired):       du_k = 0, dx <- 0             (the parked state is the constant 0; dw_k is not
 *                                                                      added)
 *   eflag_log[k] != FBSTAB_SUCCESS:     du_k = 0, dx <- A_p dx + dw_k (u_k is a constant, as in the adjoint's case rule)
 *   otherwise df_c = df0_k + F dx, db_c = db0_k + G dx and one dense adjoint (fbstab_hip_dense_adjoint_batch's, same
 *   sigma rule) of the condensed QP at the logged (U_k, v_k) with the seeds gU = -df_c, gv_c = db_c - the seeds
 *   fbstab_hip_dense_tangent_batch forms for (df, db) - refined once exactly as fbstab_hip_mpc_condensed_adjoint_batch
 *   refines it (residual kernel, the dense adjoint again, correction kernel):
 *     a factorisation failed in either launch:   status += 1, du_k = 0, dx <- A_p dx + dw_k
 *     else                                       du_k = dU[0:nu], dx <- A_p dx + B_p du_k + dw_k
 *   du[k] = du_k, dx[k] = dx (= dx_(k+1)).
 * This is the transpose of the adjoint's recursion, case for case: with that call's seeds and results on the same log
 *   sum_k <gu_k, du_k> + <gx_k, dx_(k+1)> = <lambda_0, dx0> + sum_k <mu_k, dw_k> [k not retired] + <gf0, df0> + <gb0, db0>
 * (df0, db0 one direction for all steps; with per-step directions the last two terms are sums over the steps of the
 * per-step gradients).  Directions of the plant are the caller's: they enter as dw_k += dA_p x_k + dB_p u_k.  Directions
 * of q, r, c, d - of `data` or of per-step references - reach df0_k, db0_k through
 * fbstab_hip_mpc_condensed_reference_images_batch on the direction sequences (the images are linear in those four
 * sequences; every slot must be given there, zeros where nothing moves: a NULL slot means `data`'s sequence).
 * fbstab_mpc_condensed_sweep_tangent_step_kernel (T trajectories per workgroup in the LDS layout of the forward step
 * kernel; a shared M is staged once per workgroup) is launched steps + 1 times: one launch CLOSES step k - the case
 * rule, du_k, and dx+ in the summation order of the forward kernel's plant step - and OPENS step k + 1: f_c, b_c of that
 * step from x_log[k + 1] with the forward kernel's loop and summation order (the dense handle needs b_c at the point),
 * and the seeds from dx+; both products with M are formed in one pass over a row of M, one thread per (row,
 * trajectory), j ascending.  Between two launches: the dense adjoint, fbstab_mpc_condensed_adjoint_residual_kernel,
 * the dense adjoint again, fbstab_mpc_condensed_adjoint_correct_kernel.  No atomics: the same inputs give the same
 * bits, and a trajectory's bits depend on its own inputs and the shape alone.
 *   handle, dense, map, plant: as fbstab_hip_mpc_condensed_receding_sweep_adjoint takes them.  dense's H_c and A_c are
 *           read; f_c and b_c (stride >= length with batch > 1) are per-trajectory scratch that the call overwrites.
 *           The map is always needed: a sweep that ran in RECONDENSE mode is differentiated through the map of
 *           fbstab_hip_mpc_condensed_x0_map_batch.
 *   images: NULL: map->f0, map->b0 at every step.  Otherwise the forward's f0_k, b0_k (they are READ; map->f0 and
 *           map->b0 are then not looked at).
 *   log:    the forward's; x, U, v and eflag are required.  U and v are read where they lie, no copy is made.
 *   du, dx: [steps][batch][nu], [steps][batch][nx], packed; one of them may be NULL.  Every entry is written.
 *   status: [batch], the number of steps whose factorisation failed.
 *   traj_per_group: T of the step kernel, as in the forward call: it changes speed, never a bit.
 *   work:   caller-provided DEVICE memory, batch x work_doubles_per_traj doubles, packed arrays of the batch.  Nothing
 *           is allocated.
 * EVERY pointer is a DEVICE pointer.  Asynchronous: everything is queued on `stream` (NULL: the handle's stream) and the
 * call returns.  Every argument error is FBSTAB_HIP_ERR_ARGUMENT and checked before any device call, what needs no
 * handle first, in the order of fbstab_hip_mpc_condensed_receding_sweep_adjoint: the sizes, the batch; NULL dense,
 * plant, log, dir, status, work; du and dx both NULL; a NULL plant matrix; steps < 0; traj_per_group < 0; the condensed
 * images; the plant; the required log slots; the directions (a negative step; with batch > 1 a stride below the length
 * that is not 0); the map; the images - then the handle.  batch == 0 returns OK and queues nothing; steps == 0 writes
 * status = 0 and nothing else.
 * fbstab_hip_mpc_condensed_sweep_tangent_sizes: with nzc = (N + 1) nu, nv = (N + 1) nc,
 *   lds_bytes = that of fbstab_hip_mpc_condensed_sweep_sizes (the step kernel; shared_map as there)
 *   work_doubles_per_traj = 4 nzc + 3 nv + nx + 1      (gU, dU, rU, eU; gv_c, dv, ev; dx; two status words)
 * Not here: directions on the matrix sequences, several directions per factorisation, RECONDENSE mode, the reduced
 * form, sharded sweeps, the C++ facade, the record-kernel sweep. */
typedef struct fbstab_condensed_sweep_dir_t {
  const double* dx0;
  long long stride_dx0;
  const double* dw;
  const double *df0, *db0;
  long long step_df0, step_db0, stride_df0, stride_db0;
} fbstab_condensed_sweep_dir_t;
int fbstab_hip_mpc_condensed_sweep_tangent_sizes(int N, int nx, int nu, int nc, int traj_per_group, int shared_map,
                                                 int* traj_per_group_used, long long* lds_bytes,
                                                 long long* work_doubles_per_traj);
int fbstab_hip_mpc_condensed_receding_sweep_tangent(
    fbstab_dense_handle_t handle, int N, int nx, int nu, int nc, int batch, const fbstab_dense_batch_t* dense,
    const fbstab_condensed_map_t* map, const fbstab_condensed_ref_images_t* images,
    const fbstab_receding_plant_t* plant, int steps, const fbstab_condensed_sweep_log_t* log,
    const fbstab_condensed_sweep_dir_t* dir, double sigma, double* du, double* dx, int* status, int traj_per_group,
    double* work, void* stream);

/* Diagnostic builds only (-DFB_STAMP): in-kernel per-phase cycle counters. */
int fbstab_hip_debug_stamps(unsigned long long* out32, int reset);

/* ---- several GPUs of one node, one process --------------------------------
 * The path shards embarrassingly: QP q of a batch depends on nothing but its own data
 * (FBstabMpc::Solve is a pure function of qp and the guess, fbstab/fbstab_mpc.h:181-195).
 * A shard group names the devices; handles[d] is a solver created on devices[d]; shard d
 * is the contiguous block of counts[d] QPs behind the shards 0 .. d-1, its arrays
 * (data[d], x[d], out[d]) resident on device d.  The shards run side by side without
 * any exchange, then the solutions (z, l, v, y) and SolverOut records of all shards go to
 * root_x / root_out on devices[root] in ONE RCCL operation (grouped ncclSend / ncclRecv
 * over xGMI; the root's own shard is a device copy).  The solution arrays are packed
 * (stride = length) or column slices of one record per QP, with the same layout on the
 * root.  Synchronous.  No counterpart in the reference, which is single-threaded. */
typedef struct fbstab_shard_group* fbstab_shard_group_t;
int fbstab_hip_shard_group_create(int ndev, const int* devices, fbstab_shard_group_t* group);
int fbstab_hip_shard_group_destroy(fbstab_shard_group_t group);
/* collectives issued so far and send/recv pairs inside them (tests, diagnostics) */
int fbstab_hip_shard_group_stats(fbstab_shard_group_t group, long long* gathers, long long* rccl_ops);
int fbstab_hip_mpc_solve_batch_sharded(fbstab_shard_group_t group, const fbstab_mpc_handle_t* handles,
                                       const int* counts, const fbstab_mpc_batch_t* data,
                                       const fbstab_var_batch_t* x, fbstab_solver_out_t* const* out,
                                       int root, const fbstab_var_batch_t* root_x,
                                       fbstab_solver_out_t* root_out);
/* BASELINE configs[4] sharded by trajectory: fbstab_hip_mpc_receding_sweep on every
 * device at once, then ONE collective that brings the applied inputs to the root:
 * shard d's [steps][counts[d]][nu] log at root_u_log + steps * nu * (counts[0] + ... +
 * counts[d-1]).  stats (host, may be NULL): per step, summed over the shards. */
int fbstab_hip_mpc_receding_sweep_sharded(fbstab_shard_group_t group, const fbstab_mpc_handle_t* handles,
                                          const int* counts, const fbstab_mpc_batch_t* data,
                                          const fbstab_var_batch_t* x, fbstab_solver_out_t* const* out,
                                          const fbstab_receding_plant_t* plants, int steps, int retire,
                                          double* const* u_log, int root, double* root_u_log,
                                          unsigned long long* stats);

/* ---- dense -------------------------------------------------------------- */
/* Environment read by fbstab_hip_dense_create (developer / comparison switches):
 *   FBSTAB_HIP_DENSE_ORDER=pivoted|auto|natural   initial value of fbstab_hip_dense_set_factorisation's `order`
 *   FBSTAB_HIP_DENSE_SPREAD_BITS, _ACT_BITS       the two thresholds of the AUTO order
 *   FBSTAB_HIP_DENSE_THREADS=256 the four-wavefront kernel (always pivoted) for every shape */
int fbstab_hip_dense_create(int nz, int nl, int nv, int max_batch, int device,
                            fbstab_dense_handle_t* handle);
int fbstab_hip_dense_destroy(fbstab_dense_handle_t handle);
/* Elimination order of the LDL' factorisation of the Newton system's KKT matrix
 * (DenseCholeskySolver::Initialize, dense_cholesky_solver.cc:70-79: Eigen::LDLT, symmetric
 * pivoting on the largest remaining |diagonal|).
 *   FBSTAB_HIP_DENSE_ORDER_PIVOTED (default)  Eigen's rule at every Newton step: the
 *       reference's order of rounding errors.  Exit flags, proximal and Newton counts equal
 *       the CPU restatement's on every QP of every test and of three fuzz families built to
 *       be degenerate (tools/fuzz_dense.py, 3017 QPs; profiles/r04_a_dense_order_choice.txt).
 *   FBSTAB_HIP_DENSE_ORDER_NATURAL  handles with nz + nl <= 64 (one wavefront per QP, the
 *       matrix in registers) eliminate in the natural order instead: K is quasi-definite,
 *       every order factors it, and a compile-time order is 1.6 x faster per launch on
 *       BASELINE configs[1].  The systems are the same, the rounding is not: a step's error
 *       in the directions where K is small grows with the spread of the pivots, and about
 *       one per cent of the QPs of the degenerate fuzz families then take a different
 *       number of proximal or Newton iterations (same solutions to the tolerance; none of
 *       the 4096 QPs of configs[1] differs).  A zero, denormal, infinite or NaN pivot still
 *       goes to the pivoted path, whose verdict is Eigen's.
 *   FBSTAB_HIP_DENSE_ORDER_AUTO  natural order until a QP shows itself ill-conditioned, then
 *       Eigen's rule for the rest of that QP's solve: at the first Newton step whose
 *       natural-order pivots span more than `spread_bits` binary orders of magnitude
 *       (max |d_k| / min |d_k| >= 2^spread_bits; that step is factored again), or at whose
 *       iterate at least nz - nl inequality rows carry a barrier weight above
 *       2^-act_bits / sigma (more active rows than free variables: a degenerate vertex).
 *       At the defaults (32, 20) configs[1] runs at the natural order's speed and the
 *       degenerate families differ on 0.4 % of their QPs; spread_bits = 30 costs configs[1]
 *       12 % and leaves 0.13 %.  No threshold that keeps the speed closes the gap - the
 *       sensitive steps have the pivot spread of ordinary ones - which is why the default
 *       is the reference's order and this one is the caller's choice.
 * spread_bits: 1..2046, or 0 to keep the current value.  Handles on the four-wavefront
 * kernels (nz + nl > 64) always pivot; the call is accepted and has no effect there. */
enum fbstab_hip_dense_order {
  FBSTAB_HIP_DENSE_ORDER_AUTO = 0,
  FBSTAB_HIP_DENSE_ORDER_PIVOTED = 1,
  FBSTAB_HIP_DENSE_ORDER_NATURAL = 2
};
int fbstab_hip_dense_set_factorisation(fbstab_dense_handle_t handle, int order, int spread_bits);
/* The settings in force and (pivoted_steps, may be NULL; waits for the handle's last launch)
 * the number of Newton steps of the most recent solve_batch call that AUTO handed to the
 * pivoted factorisation; -1 where that does not apply. */
int fbstab_hip_dense_get_factorisation(fbstab_dense_handle_t handle, int* order, int* spread_bits,
                                       long long* pivoted_steps);
int fbstab_hip_dense_set_options(fbstab_dense_handle_t handle, const fbstab_options_t* options);
int fbstab_hip_dense_get_options(fbstab_dense_handle_t handle, fbstab_options_t* options);
int fbstab_hip_dense_solve_batch(fbstab_dense_handle_t handle, int batch,
                                 const fbstab_dense_batch_t* data,
                                 const fbstab_var_batch_t* x, fbstab_solver_out_t* out,
                                 int flags, void* stream);
/* As fbstab_hip_mpc_solve_batch_final (FBstabDense::Solve at Display::FINAL). */
int fbstab_hip_dense_solve_batch_final(fbstab_dense_handle_t handle, int batch,
                                       const fbstab_dense_batch_t* data, const fbstab_var_batch_t* x,
                                       fbstab_solver_out_t* out, double* norms, int flags, void* stream);
int fbstab_hip_dense_solve_traced(fbstab_dense_handle_t handle, const fbstab_dense_batch_t* data,
                                  const fbstab_var_batch_t* x, fbstab_solver_out_t* out,
                                  fbstab_trace_record_t* trace, int capacity, int* count);
/* As fbstab_hip_mpc_solve_batch_sharded (FBstabDense::Solve, fbstab/fbstab_dense.h:136-149). */
int fbstab_hip_dense_solve_batch_sharded(fbstab_shard_group_t group, const fbstab_dense_handle_t* handles,
                                         const int* counts, const fbstab_dense_batch_t* data,
                                         const fbstab_var_batch_t* x, fbstab_solver_out_t* const* out,
                                         int root, const fbstab_var_batch_t* root_x,
                                         fbstab_solver_out_t* root_out);
/* As fbstab_hip_mpc_debug_newton, for the dense path (DenseCholeskySolver::Initialize +
 * Solve, dense_cholesky_solver.cc:32-127).  io: [zbar, lbar, vbar] in,
 * [dz, dl, dv, A*dz, W_z, W_l, r_z, r_l, ok] out. */
int fbstab_hip_dense_debug_newton(fbstab_dense_handle_t handle, const fbstab_dense_batch_t* data,
                                  const fbstab_var_batch_t* x, double* io);
/* Derivatives of the dense solution map: fbstab_hip_mpc_adjoint_batch for FBstabDense's QP
 *   min 1/2 z'Hz + f'z  s.t. Gz = h, Az <= b
 * (the OptNet-style QP layer).  At x = xbar = the returned point the Newton matrix of
 * DenseCholeskySolver::Initialize (fbstab/components/dense_cholesky_solver.cc:32-79),
 *   V = [H + sigma I, G', A'; -G, sigma I, 0; -C A, 0, mus],
 * C = d phi / d y and mus = d phi / d v + sigma C of the penalised FB function with options.alpha,
 * is factored once, and one Solve (:81-127) with the right-hand side (gz, -gl, -C gv) gives
 * (dz, dl, dv).  The gradients of the six arrays of fbstab_dense_batch_t are
 *   f_bar = -dz        h_bar = dl        b_bar = dv
 *   H_bar = -(dz z' + z dz')/2   (the gradient of the symmetric part, as for Q and R)
 *   G_bar = -(dl z' + l dz')     A_bar = -(dv z' + v dz')
 * column-major like the inputs: H_bar[r + c nz], G_bar[r + c nl], A_bar[r + c nv].  (h and b enter
 * the dense data directly, not negated as in the MPC mapping.)  sigma <= 0 selects 1e-8 whatever
 * the handle's options say.
 *   x:      the points, (z, l, v) (the y slot is not read).
 *   seed:   (gz, gl, gv); the l and v slots may be NULL (zero).
 *   grad:   one slot per array, strides as in fbstab_dense_batch_t; a NULL slot is not computed.
 *           Every slot that is not NULL is written.
 *   adj:    NULL, or (dz, dl, dv) (its NULL slots are skipped).
 *   status: per QP, 0, or 1 where the factorisation failed (its gradients and adj are zero).  It
 *           lives where solve_batch's `out` lives (host for host-pointer calls and with
 *           FBSTAB_HIP_OUT_ON_HOST, device otherwise).
 * Flags, streams, host staging and validation are those of fbstab_hip_dense_solve_batch; every QP
 * needs its own slots in x, seed, grad and adj (with batch > 1 a stride below the vector or array
 * length is FBSTAB_HIP_ERR_ARGUMENT).  Handles with nl == 0 ignore the G and h slots (and the l
 * slots of x, seed and adj).  batch == 0 returns OK.  All validation runs before any device call;
 * what needs no handle is checked first - the argument blocks, the z seed, and strides below 1 on
 * the slots that are never empty (z, v; H, f, A, b) - then the handle and the lengths it knows.
 * Kernels: one per solve kernel.  Handles with nz + nl <= 64 run fbstab_dense_wave_adjoint_kernel
 * (one wavefront per QP, K in registers, the handle's own scratch); it ALWAYS factors by the pivoted
 * rule, whatever fbstab_hip_dense_set_factorisation says - at a solution the active rows carry
 * Gamma ~ 1 / sigma, the case AUTO hands to the pivoted path anyway, and a gradient should not
 * depend on a speed option - and leaves fbstab_hip_dense_get_factorisation's pivoted_steps
 * describing the last SOLVE.  The other handles run fbstab_dense_adjoint_kernel<NT, KGLOBAL,
 * VGLOBAL>, the instance that matches their solve kernel.
 * fbstab_hip_dense_last_kernel_ms then reports this launch. */
typedef struct fbstab_dense_grad_batch_t {
  double* base[FBSTAB_DENSE_NARR];
  long long stride[FBSTAB_DENSE_NARR];
} fbstab_dense_grad_batch_t;
int fbstab_hip_dense_adjoint_batch(fbstab_dense_handle_t handle, int batch, const fbstab_dense_batch_t* data,
                                   const fbstab_var_batch_t* x, const fbstab_var_batch_t* seed, double sigma,
                                   const fbstab_dense_grad_batch_t* grad, const fbstab_var_batch_t* adj,
                                   int* status, int flags, void* stream);
/* fbstab_hip_dense_adjoint_batch with gradients summed over the batch, for arrays the batch shares:
 * fbstab_hip_mpc_adjoint_batch_reduced for the dense QP.  A grad slot of stride 0 receives ONE
 * array, sum_b of the per-QP gradient (H_bar, G_bar, A_bar column-major as there); slots of stride
 * >= length are per QP and bitwise those of fbstab_hip_dense_adjoint_batch; with batch > 1 any other
 * stride is FBSTAB_HIP_ERR_ARGUMENT, checked where fbstab_hip_dense_adjoint_batch checks strides.
 * `out` (NULL, or the solve's records, living where `status` lives) and the adjoint status leave QPs
 * out of the sums as there.  Kernels, determinism and fbstab_hip_dense_last_kernel_ms: as there, the
 * tiles those of M = -(P'Z + X'DZ), (nz + nl + nv) x nz.  Memory held from the first reduced call
 * until destroy, not counted by fbstab_hip_dense_query: max_batch x (nz + nl + nv) doubles and
 * tiles x ceil(max_batch / 128) x 272 doubles (at (50, 10, 100) and max_batch 4096: 5.2 MB and, with
 * 40 tiles, 2.8 MB). */
int fbstab_hip_dense_adjoint_batch_reduced(fbstab_dense_handle_t handle, int batch,
                                           const fbstab_dense_batch_t* data, const fbstab_var_batch_t* x,
                                           const fbstab_var_batch_t* seed, double sigma,
                                           const fbstab_dense_grad_batch_t* grad, const fbstab_var_batch_t* adj,
                                           int* status, const fbstab_solver_out_t* out, int flags, void* stream);
/* fbstab_hip_mpc_tangent_batch for the dense QP: (dz, dl, dv) = J dtheta for perturbations (dH, df, dG, dh, dA,
 * db) in the layout of fbstab_dense_batch_t, from V (dz, dl, dv) = (gz, -gl, -C gv) with
 *   gz = -(sym(dH) z + df + dG' l + dA' v)      gl = dh - dG z      gv = db - dA z
 * (h and b enter the dense data directly).  fbstab_dense_tangent_rhs_kernel (fb_tangent.h: one workgroup per QP,
 * the images walked once in blocks of columns, row and column sums from the same block in LDS; no atomics, sums
 * in an order fixed by the shape) writes the seeds, the launch of fbstab_hip_dense_adjoint_batch solves for them.
 * ddata, dx, rhs, status, sigma, flags, streams, host staging, batch == 0, the seed buffer (the allocation of
 * fbstab_hip_dense_adjoint_batch_reduced's adjoint steps) and fbstab_hip_dense_last_kernel_ms: as there;
 * validation as fbstab_hip_dense_adjoint_batch (what needs no handle first).  Handles with nl == 0 ignore the G
 * and h slots and the l slots of x, dx and rhs. */
int fbstab_hip_dense_tangent_batch(fbstab_dense_handle_t handle, int batch, const fbstab_dense_batch_t* data,
                                   const fbstab_var_batch_t* x, const fbstab_dense_batch_t* ddata, double sigma,
                                   const fbstab_var_batch_t* dx, const fbstab_var_batch_t* rhs,
                                   int* status, int flags, void* stream);
/* ---- many right-hand sides on the dense QP: factor V once, solve for nrhs of them ---------------------------------
 * fbstab_hip_mpc_kkt_solve_batch and fbstab_hip_mpc_x0_sensitivity_batch for the dense QP.  The matrices a user of
 * the layer asks for - dz/db, dz/df, dz/dh, or several loss seeds at the same solutions - cost one factorisation per
 * column through the adjoint and the tangent above.  DenseCholeskySolver::Initialize is O(nz^2 nv + n^3) (A'Gamma A
 * and the LDL' of the n = nz + nl matrix K), a Solve O(n^2 + nz nv); these two calls factor once per QP and run the
 * vector part of the step once per right-hand side (fb_dense_kkt_multi.h).
 *
 * fbstab_hip_dense_kkt_solve_batch: slot k of `step` is the solution of V (dz, dl, dv) = (gz_k, -gl_k, -C gv_k) at
 * x = xbar = the point, what fbstab_hip_dense_adjoint_batch(..., adj) solves for seed k.
 *   nrhs, seed, step, their strides and `status`: those of fbstab_hip_mpc_kkt_solve_batch, word for word - vector k
 *   of QP q of slot i at base[i] + q stride[i] + k rhs_stride[i]; NULL l and v seed slots are zero; a seed slot of
 *   stride 0 is one block shared by the batch; NULL step slots are skipped; with batch > 1 or nrhs > 1
 *   rhs_stride >= length and stride >= (nrhs - 1) rhs_stride + length, anything else FBSTAB_HIP_ERR_ARGUMENT; the
 *   doubles between a QP's vectors are not written; nrhs < 1 is FBSTAB_HIP_ERR_ARGUMENT; status[q] = 1 where the
 *   factorisation failed, and every right-hand side's step of that QP is then zero.
 * fbstab_hip_dense_jacobian_batch: the right-hand sides are the unit seeds of one array, generated in the kernel with
 * the tangent's signs (gz = -df, gl = dh, gv = db), so that row k of `step` is fbstab_hip_dense_tangent_batch's dx for
 * the perturbation e_k of that array - bitwise what fbstab_hip_dense_kkt_solve_batch returns for those seeds:
 *   wrt = FBSTAB_DENSE_f: nrhs = nz, gz = -e_k;   FBSTAB_DENSE_h: nrhs = nl, gl = e_k;   FBSTAB_DENSE_b: nrhs = nv,
 *   gv = e_k.  A matrix index (H, G, A) or anything else is FBSTAB_HIP_ERR_ARGUMENT, and so is FBSTAB_DENSE_h on a
 *   handle with nl == 0.
 *   step: as above with that nrhs.  A caller who wants only dz/db (nv x nz per QP) passes NULL for the l and v
 *   slots: the dv slot of wrt = b alone is nv x nv doubles per QP, which at large nv (the shapes whose iterate
 *   vectors already live in global scratch) is most of the memory and the write traffic of the call.
 * Kernels: fbstab_dense_wave_kkt_multi_kernel and fbstab_dense_kkt_multi_kernel<NT, KGLOBAL, VGLOBAL>, the instance
 * beside the handle's adjoint kernel, picked by the same handle state, in the handle's own scratch.  On the
 * four-wavefront instances right-hand side 0 is the adjoint's own arithmetic and the others re-run its vector part
 * on the stored factors.  On the one-wavefront kernel (nz + nl <= 64) every right-hand side, number 0 included, takes
 * one path behind one pivoted factorisation (whatever fbstab_hip_dense_set_factorisation says, pivoted_steps left
 * alone): a seed's step depends neither on its slot nor on the other seeds, and is the adjoint kernel's to the
 * same accuracy, not to the bit.
 * sigma (<= 0 selects 1e-8), flags, streams, where `status` lives, nl == 0 (the l slots are ignored), batch == 0 (OK,
 * nothing is queued) are those of fbstab_hip_dense_adjoint_batch; a host-pointer call stages the seed and step blocks
 * packed, in allocations of the call, as the MPC calls do.  Validation: what needs no handle comes first - nrhs or
 * wrt, the NULL blocks, a NULL z seed, strides no length could satisfy - then the handle and what takes its lengths;
 * everything before any device call.  fbstab_hip_dense_last_kernel_ms reports the launch. */
int fbstab_hip_dense_kkt_solve_batch(fbstab_dense_handle_t handle, int batch, const fbstab_dense_batch_t* data,
                                     const fbstab_var_batch_t* x, int nrhs, const fbstab_multi_var_batch_t* seed,
                                     double sigma, const fbstab_multi_var_batch_t* step, int* status, int flags,
                                     void* stream);
int fbstab_hip_dense_jacobian_batch(fbstab_dense_handle_t handle, int batch, const fbstab_dense_batch_t* data,
                                    const fbstab_var_batch_t* x, int wrt, double sigma,
                                    const fbstab_multi_var_batch_t* step, int* status, int flags, void* stream);
double fbstab_hip_dense_last_kernel_ms(fbstab_dense_handle_t handle);
int fbstab_hip_dense_query(fbstab_dense_handle_t handle, long long* scratch_bytes,
                           int* lds_bytes, int* workgroups, int* threads);

#ifdef __cplusplus
}
#endif

#endif /* FBSTAB_HIP_H_ */
