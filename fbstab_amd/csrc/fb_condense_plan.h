// The condensed MPC route's layouts and sizes (fb_condense*.h, fb_condense_stage.h): what the kernels and the host
// both read - where the stage images lie in LDS, the structs a launch takes by value, the kernels' numbers, and how a
// caller's work array is divided.  Plain structs and size rules: no kernel code, nothing of the runtime, so that the
// host stage and its CPU driver (tests/hostsim/condense_stage_driver.cc) take it without a kernel header.
#pragma once

#include "../../include/fbstab_hip.h"

namespace fbk {

// ---- the kernels, as their unit's getter numbers them (fbstab_condense_kernel(which, &threads)) ---------------------
enum CondenseKernel { kCondenseMatrices = 0, kCondenseVectors = 1, kCondenseExpand = 2 };            // fb_condense.hip
enum CondenseAdjointKernel { kCondenseAdjSeed = 0, kCondenseAdjFinish = 1, kCondenseAdjResidual = 2,
                             kCondenseAdjCorrect = 3 };                                     // fb_condense_adjoint.hip
enum CondenseMultiKernel { kCondenseMultiSeed = 0, kCondenseMultiFinish = 1, kCondenseMultiResidual = 2,
                           kCondenseMultiCorrect = 3 };                                       // fb_condense_multi.hip
enum CondenseSweepKernel { kCondenseSweepX0Map = 0, kCondenseSweepStep = 1, kCondenseSweepBegin = 2 };  // fb_condense_sweep.hip
enum CondenseSweepAdjKernel { kCondenseSweepAdjStep = 0, kCondenseSweepAdjFinish = 1,
                              kCondenseSweepAdjBegin = 2 };                           // fb_condense_sweep_adjoint.hip
enum CondenseTangentKernel { kCondenseTangentRhs = 0 };                                    // fb_condense_tangent.hip
enum CondenseRefsKernel { kCondenseRefsImages = 0 };                                          // fb_condense_refs.hip
enum CondenseSweepTanKernel { kCondenseSweepTanStep = 0 };                            // fb_condense_sweep_tangent.hip

// ---- fb_condense.h ----------------------------------------------------------------------------------------------
inline int condense_ld(int rows) { return rows | 1; }

// Where the images of one stage and what is carried from stage to stage lie in w (offsets in doubles, all even).
//   window: A, Q (ldx x nx each), B (ldx x nu), E (ldc x nx), S (ldu x nx), L (ldc x nu), R (ldu x nu)
//   carry:  the larger of  (N + 2) ldx nu                       - X_k^(k+1 .. N) and two P (condense_matrices)
//                     and  (N + 1) (nx + nu + nc) + 2 nx        - x, u, v of every stage and two p / l (the others)
// with ldx = nx | 1, ldc = nc | 1, ldu = nu | 1 and every piece rounded up to an even number of doubles.
struct CondenseLds {
  int ldx, ldc, ldu;
  int A, Q, B, E, S, L, R, carry, total;
  void init(int N, int nx, int nu, int nc) {
    ldx = condense_ld(nx); ldc = condense_ld(nc); ldu = condense_ld(nu);
    long long o = 0;
    auto take = [&o](long long n) { const long long at = o; o += n + (n & 1); return (int)at; };
    A = take((long long)ldx * nx); Q = take((long long)ldx * nx); B = take((long long)ldx * nu);
    E = take((long long)ldc * nx); S = take((long long)ldu * nx); L = take((long long)ldc * nu);
    R = take((long long)ldu * nu);
    const long long m = (long long)(N + 2) * (ldx * nu + ((ldx * nu) & 1));
    const long long v = (long long)(N + 1) * (nx + nu + nc) + 2LL * nx + 8;  // (each of the 5 pieces even)
    carry = take(m > v ? m : v);
    total = o > 0x3fffffff ? 0x3fffffff : (int)o;
  }
};

// ---- fb_condense_adjoint.h --------------------------------------------------------------------------------------
// The caller's work array, per QP: U, gU, dU of (N + 1) nu doubles and gv_c, dv of (N + 1) nc, then the refinement's
// rU, eU of (N + 1) nu and ev of (N + 1) nc, each one packed array of the batch (QP q at base + q * length).
struct CondenseAdjointWork {
  double *U, *gU, *dU, *gv, *dv, *rU, *eU, *ev;
};

// ---- fb_condense_multi.h ----------------------------------------------------------------------------------------
// Doubles of one right-hand side's copy of the carry region (even).
inline long long condense_multi_per(int N, int nx, int nu, int nc) {
  auto e = [](long long n) { return n + (n & 1); };
  const long long n1 = N + 1;
  const long long seed = e(n1 * nx) + 2 * e(nx);
  const long long fin = e(n1 * (nx + nu)) + e(n1 * nc) + 2 * e(nx);
  return seed > fin ? seed : fin;
}

// The library's rule for the right-hand sides per workgroup: clamp(256 / nx, 1, nrhs), lowered until the launch's
// dynamic LDS - `window` doubles of stage images and R copies of `per` - lets two workgroups share a CU (80 KB).
inline int condense_multi_rule(int nx, int nrhs, long long window, long long per) {
  int R = 256 / nx;
  if (R > nrhs) R = nrhs;
  if (R < 1) R = 1;
  while (R > 1 && (window + R * per) * 8 > 80 * 1024) R--;
  return R;
}

// The caller's work array: U of (N + 1) nu doubles per QP, then gU, dU, rU, eU of nrhs (N + 1) nu and gv_c, dv, ev of
// nrhs (N + 1) nc, each one packed [batch][nrhs][n] array.
struct CondenseMultiWork {
  double *U, *gU, *dU, *rU, *eU, *gv, *dv, *ev;
};

// ---- fb_condense_refs.h -----------------------------------------------------------------------------------------
// Doubles of one reference's copy of the carry region (even): what condense_vectors carries - xbar_i of every stage
// and two p.
inline long long condense_refs_per(int N, int nx) {
  auto e = [](long long n) { return n + (n & 1); };
  return e((long long)(N + 1) * nx) + 2 * e(nx);
}

// The q, r, c, d of one trajectory at the first reference of a workgroup: reference kk at + kk * step (0: one sequence
// for every step).
struct CondenseRefSeqs {
  const double *q, *r, *c, *d;
  long long sq, sr, sc, sd;
};

// ---- fb_condense_sweep.h ----------------------------------------------------------------------------------------
// Where the pieces of a workgroup of T trajectories lie in w (offsets in doubles, all even): the shared image M with
// leading dimension ldm = ne | 1 (m_lds: it is staged; 0: every M is read from memory), then per trajectory the state
// the step was solved for, the next state, U, v, and a word for `gone`.
constexpr long long condense_sweep_even(long long n) { return n + (n & 1); }
struct CondenseSweepLds {
  int ldm, m_lds, T;
  int M, x, xn, U, v, gone, total;
  long long m_doubles, per;
  // T = 0 asks for the rule: ceil(1024 / ne) trajectories (four rounds of the 256 threads over the entries of f_c and
  // b_c, so that staging a shared M costs a fraction of using it), at most 64, lowered until the workgroup takes no
  // more than 80 KB (two workgroups per CU).  A shared M is staged where it leaves room for one trajectory in 80 KB.
  void init(int N, int nx, int nu, int nc, int want_T, bool stage_m) {
    const long long nzc = (long long)(N + 1) * nu, nv = (long long)(N + 1) * nc, ne = nzc + nv;
    const long long budget = 80 * 1024 / 8;
    per = 2 * condense_sweep_even(nx) + condense_sweep_even(nzc) + condense_sweep_even(nv) + 2;
    ldm = (int)(ne | 1);
    m_doubles = condense_sweep_even((long long)ldm * nx);
    m_lds = (stage_m && m_doubles + per <= budget) ? 1 : 0;
    const long long m = m_lds ? m_doubles : 0;
    long long t = want_T;
    if (t <= 0) {
      t = (1024 + ne - 1) / ne;
      if (t > 64) t = 64;
      while (t > 1 && m + t * per > budget) t--;
    }
    if (t < 1) t = 1;
    T = (int)t;
    long long at = 0;
    auto take = [&at](long long n) { const long long a = at; at += n; return (int)(a > 0x3fffffff ? 0x3fffffff : a); };
    M = take(m);
    x = take((long long)T * condense_sweep_even(nx));
    xn = take((long long)T * condense_sweep_even(nx));
    U = take((long long)T * condense_sweep_even(nzc));
    v = take((long long)T * condense_sweep_even(nv));
    gone = take(2LL * T);
    total = at > 0x3fffffff ? 0x3fffffff : (int)at;
  }
};

// What one launch of the step kernel works on: step k's shares of the logs (null: not logged), and the packed work
// arrays U [batch][nzc], v [batch][nv], gone [batch] the dense solve reads its guess from and writes its point to.
struct CondenseSweepStep {
  int N, nx, nu, nc, batch;
  int retire, shift, affine;     // shift, affine: 0 behind the last step
  const fbstab_solver_out_t* out;
  int* gone;
  double *U, *v;
  double* x0; long long sx0;     // the caller's x0, advanced in place
  double* xkeep;                 // null, or [batch][nx]: receives the state the step was solved for
  const double *Ap, *Bp; long long sAp, sBp;
  const double* w;               // null, or this step's disturbances [batch][nx]
  double *u_log, *x_log, *U_log, *v_log;
  int *eflag_log, *newton_log;
  const double* M; long long sM;
  const double* f0; long long sf0;
  const double* b0; long long sb0;
  double* f; long long sf;
  double* b; long long sb;
};

// ---- fb_condense_sweep_adjoint.h --------------------------------------------------------------------------------
// What one launch of the step kernel works on.  close / open: which parts run (the first launch only opens, the last
// only closes).  The arrays of the closed step k + 1 and of the opened step k are their shares of the logs.
struct CondenseSweepAdjStep {
  int N, nx, nu, nc, batch;
  int close, open, affine;        // affine: lambda through M and f_c, b_c from the map; 0: dl0 and the vectors launch
  const int* eflag_close;         // eflag_log[k + 1]
  const int* eflag_open;          // eflag_log[k]
  const int *st1, *st2;           // the dense adjoint's status of both launches of step k + 1
  int* status;                    // [batch], += 1 where either is set on a step that would contribute
  const double *dU, *dv;          // the refined dense step of step k + 1, packed [batch][nzc], [batch][nv]
  double* dl0;                    // affine == 0: [batch][nx], -dl[0:nx] of the finish of step k + 1; zeroed by open
  double* mu;                     // [batch][nx]: mu of the open step, read back by the close of the next launch
  const double *Ap, *Bp; long long sAp, sBp;
  const double *gu, *gx;          // gu[k] [batch][nu], gx[k] [batch][nx]; null: zero
  double* mu_log;                 // null, or mu_log[k]
  double* gU;                     // [batch][nzc]: the seed of the dense adjoint of step k
  const double* x_log;            // x_log[k]
  const double* M; long long sM;
  const double* f0; long long sf0;
  const double* b0; long long sb0;
  double* f; long long sf;
  double* b; long long sb;
  double *gf0, *gb0;              // null, or packed [batch][nzc], [batch][nv]: sums of -dU and dv
  double* gx0; long long sgx0;    // null, or the x0 slot: the final lambda (written by the launch that does not open)
};

// What the finish kernel reads of one step: the logged point, the dense step, and who contributes.
struct CondenseSweepAdjFinish {
  const double *x, *U, *v;        // x_log[k], U_log[k], v_log[k], packed
  const double *dU, *dv;          // the refined dense step, packed
  const int *eflag, *st1, *st2;   // eflag_log[k] and the dense adjoint's status of both launches
  double *z, *l, *gz;             // scratch [batch][nz], [batch][nl], and the zeros [batch][nz]
  double* dl0;                    // null, or [batch][nx] (zero on entry): receives -dl[0:nx]
};

// ---- fb_condense_sweep_tangent.h --------------------------------------------------------------------------------
// What one launch of the step kernel works on.  close / open: which parts run (the first launch only opens, the last
// only closes).  The arrays of the closed step k and of the opened step k + 1 are their shares of the logs, of the
// directions and of the outputs.
struct CondenseSweepTanStep {
  int N, nx, nu, nc, batch;
  int close, open;
  const int* eflag_close;         // eflag_log[k]
  const int* eflag_open;          // eflag_log[k + 1]
  const int *st1, *st2;           // the dense adjoint's status of both launches of step k
  int* status;                    // [batch]: zeroed by the launch that does not close, += 1 as in the adjoint
  const double* dU;               // the refined dense step of step k, packed [batch][nzc]
  double* dx;                     // [batch][nx]: the direction of the state, carried from launch to launch
  const double* dx0; long long sdx0;  // read by the launch that does not close (null: zero)
  const double *Ap, *Bp; long long sAp, sBp;
  const double* dw;               // null (zero), or dw[k] [batch][nx]
  double *du_out, *dx_out;        // null, or du_out[k] [batch][nu], dx_out[k] [batch][nx]
  const double* x_log;            // x_log[k + 1]
  const double* M; long long sM;
  const double* f0; long long sf0;
  const double* b0; long long sb0;
  double* f; long long sf;
  double* b; long long sb;
  const double* df0; long long sdf0;  // null (zero), or the directions of f0, b0 of step k + 1
  const double* db0; long long sdb0;
  double *gU, *gv;                // [batch][nzc], [batch][nv]: the seeds of the dense adjoint of step k + 1
};

// ---- the callers' work arrays -------------------------------------------------------------------------------------
// A work array is packed pieces, [batch][n] each, one behind the other.  Each struct below is the ONE description of
// an array: constructed on (work, batch) it holds the pieces and `per`, the doubles of one QP or trajectory that the
// *_sizes functions report; on (nullptr, 0) `per` alone means something.
struct CondenseCarve {
  double* at;
  long long batch, per;
  double* take(long long n) {
    double* const p = at;
    per += n;
    if (at) at += n * batch;
    return p;
  }
  // [batch] ints in the doubles of take(1): an int is half a double, so one double per QP holds one int per QP -
  // and a second array of [batch] ints behind it (take_ints(1) + batch).
  int* take_ints() { return reinterpret_cast<int*>(take(1)); }
};

// fbstab_hip_mpc_condensed_adjoint_batch: 5 (N + 1) nu + 3 (N + 1) nc doubles per QP.
struct CondenseAdjointCarve {
  CondenseAdjointWork wk;
  long long per;
  CondenseAdjointCarve(long long nz, long long nv, double* work, int batch) {
    CondenseCarve c = {work, batch, 0};
    wk.U = c.take(nz); wk.gU = c.take(nz); wk.dU = c.take(nz);
    wk.gv = c.take(nv); wk.dv = c.take(nv);
    wk.rU = c.take(nz); wk.eU = c.take(nz); wk.ev = c.take(nv);
    per = c.per;
  }
};

// fbstab_hip_mpc_condensed_tangent_batch: the adjoint's work (`adjoint`, carved as above), then the seeds gz, gl, gv of
// the MPC QP's lengths nzf = (N + 1)(nx + nu), nlf = (N + 1) nx and nv - the tail the call uses where the caller gives
// no rhs block.
struct CondenseTangentCarve {
  CondenseAdjointWork wk;
  double *gz, *gl, *gv;
  long long per;
  CondenseTangentCarve(long long nz, long long nv, long long nzf, long long nlf, double* work, int batch) {
    const CondenseAdjointCarve adjoint(nz, nv, work, batch);
    wk = adjoint.wk;
    CondenseCarve c = {work ? work + adjoint.per * batch : nullptr, batch, adjoint.per};
    gz = c.take(nzf); gl = c.take(nlf); gv = c.take(nv);
    per = c.per;
  }
};

// fbstab_hip_mpc_condensed_multi_sizes: (N + 1) nu + nrhs (4 (N + 1) nu + 3 (N + 1) nc).
struct CondenseMultiCarve {
  CondenseMultiWork wk;
  long long per;
  CondenseMultiCarve(long long nz, long long nv, int nrhs, double* work, int batch) {
    CondenseCarve c = {work, batch, 0};
    wk.U = c.take(nz);
    wk.gU = c.take(nz * nrhs); wk.dU = c.take(nz * nrhs); wk.rU = c.take(nz * nrhs); wk.eU = c.take(nz * nrhs);
    wk.gv = c.take(nv * nrhs); wk.dv = c.take(nv * nrhs); wk.ev = c.take(nv * nrhs);
    per = c.per;
  }
};

// fbstab_hip_mpc_condensed_sweep_sizes: the condensed point (U, v, y), the state the last step was solved for, and
// `gone`, [batch] ints.
struct CondenseSweepCarve {
  double *U, *v, *y, *xkeep;
  int* gone;
  long long per;
  CondenseSweepCarve(long long nz, long long nv, int nx, double* work, int batch) {
    CondenseCarve c = {work, batch, 0};
    U = c.take(nz); v = c.take(nv); y = c.take(nv); xkeep = c.take(nx);
    gone = c.take_ints();
    per = c.per;
  }
};

// fbstab_hip_mpc_condensed_sweep_adjoint_sizes: the seed, the dense step and its refinement (wk; its U and gv are
// not used), mu, -dl[0:nx], the two status words st1 and st2 ([batch] ints each, in ONE double per trajectory); with
// the finish kernel also the expanded point (z, l) and the zeros it reads for gz (null without it).
struct CondenseSweepAdjCarve {
  CondenseAdjointWork wk;
  double *mu, *dl0, *z, *gz, *l;
  int *st1, *st2;
  long long per;
  CondenseSweepAdjCarve(int N, int nx, int nu, int nc, bool finish, double* work, int batch) {
    const long long nz = (long long)(N + 1) * nu, nv = (long long)(N + 1) * nc;
    CondenseCarve c = {work, batch, 0};
    wk = CondenseAdjointWork{};
    wk.gU = c.take(nz); wk.dU = c.take(nz); wk.rU = c.take(nz); wk.eU = c.take(nz);
    wk.dv = c.take(nv); wk.ev = c.take(nv);
    mu = c.take(nx); dl0 = c.take(nx);
    st1 = c.take_ints();
    st2 = st1 ? st1 + batch : nullptr;
    z = gz = l = nullptr;
    if (finish) {
      z = c.take((long long)(N + 1) * (nx + nu)); gz = c.take((long long)(N + 1) * (nx + nu));
      l = c.take((long long)(N + 1) * nx);
    }
    per = c.per;
  }
};

// fbstab_hip_mpc_condensed_sweep_tangent_sizes: the seeds, the dense step and its refinement (wk; its U is not
// used), the carried direction of the state, the two status words st1 and st2 ([batch] ints each, in ONE double per
// trajectory).
struct CondenseSweepTanCarve {
  CondenseAdjointWork wk;
  double* dx;
  int *st1, *st2;
  long long per;
  CondenseSweepTanCarve(int N, int nx, int nu, int nc, double* work, int batch) {
    const long long nz = (long long)(N + 1) * nu, nv = (long long)(N + 1) * nc;
    CondenseCarve c = {work, batch, 0};
    wk = CondenseAdjointWork{};
    wk.gU = c.take(nz); wk.dU = c.take(nz); wk.rU = c.take(nz); wk.eU = c.take(nz);
    wk.gv = c.take(nv); wk.dv = c.take(nv); wk.ev = c.take(nv);
    dx = c.take(nx);
    st1 = c.take_ints();
    st2 = st1 ? st1 + batch : nullptr;
    per = c.per;
  }
};

}  // namespace fbk
