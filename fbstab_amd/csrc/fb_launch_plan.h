// How a handle is sized and how each of its launches is shaped: the environment knobs the C-ABI unit reads, the
// workgroup count and scratch size a handle is created with, and the grid of every batch launch - the decisions of
// fbstab_hip.hip, as pure host functions (no HIP types: tests/test_launch_plan.py compiles this header with the
// host compiler alone and checks every rule as a table; fb_in_flight.h, which this builds on, holds the share
// rule of handles that run side by side).
//
// A batch launch is a persistent grid that pulls QPs from a queue (fb_in_flight.h).  A handle keeps `workgroups`
// of them, never more than its max_batch can use, and scratch memory for every QP slot of that grid: a record
// kernel (fb_mpc_r16.h) solves qps_per_wg QPs per one-wavefront workgroup, four 16-lane rows or two row pairs;
// every other kernel one QP per workgroup.
#pragma once
#include <cstdlib>
#include <cstring>

#include "fb_in_flight.h"

namespace fbk {

// What the host staging (fb_host_stage.h) and the launch sites share with the kernels of the C-ABI unit:
// the queue block of a handle (the queue word, the refinement count, the dense counters below), allocated at
// creation and zeroed before every launch ...
constexpr size_t kQueueBytes = 8 * sizeof(int);
// ... the word of it in which the one-wavefront dense kernel counts the Newton steps it handed to the pivoted
// factorisation ...
constexpr int kDenseFallbackSlot = 4;
// ... and the dynamic LDS a workgroup may ask for.
constexpr int kLdsLimitBytes = 160 * 1024;

// ---------------------------------------------------------------------------------------------------------------
// The knobs: every FBSTAB_HIP_* variable the C-ABI unit reads (the shard knobs are fb_shard.h's own).  DESIGN.md
// section 4.6 has the table.  All of them are developer and test switches; each is parsed by the expression its
// first use was written with, oddities included (atoi: text that is no number reads as 0).

// Read once per handle, when it is created.
struct CreateKnobs {
  // FBSTAB_HIP_GENERIC=1 forces the flat-vector kernel (comparisons, tests)
  bool generic = false;
  // FBSTAB_HIP_FLAT_ADJOINT: 1 - the flat-vector adjoint on a record handle; 0 - its record adjoint; -1 (unset or
  // empty) - the record adjoint on the one-row instances and the flat-vector adjoint on the row-pair instances,
  // whose record adjoint has not been timed against it on the wide workloads yet
  int flat_adjoint = -1;
  // FBSTAB_HIP_LDS_PAD_BYTES: extra (unused) LDS per workgroup, to lower the number of resident wavefronts in
  // occupancy experiments; whole 16-byte units
  int lds_pad_bytes = 0;
  // FBSTAB_HIP_WGS_PER_CU=n > 0: n workgroups per CU, whatever the occupancy and the share rule say (a caller whose
  // streams share hardware queues for reasons the rule cannot see: fb_in_flight.h)
  int wgs_per_cu = 0;
  // FBSTAB_HIP_MAX_WORKGROUPS=n > 0 caps the grid, so that small batches pack every row of a record kernel and
  // re-fetch, and one workgroup of a dense kernel solves several QPs in turn (tests)
  int max_workgroups = 0;
  // FBSTAB_HIP_DENSE_THREADS, as a number (dense_threads_choice below says what is honoured)
  int dense_threads = 0;
  // Initial values of what fbstab_hip_dense_set_factorisation sets per handle (the default is the reference's
  // order): FBSTAB_HIP_DENSE_ORDER=pivoted | auto | natural, as the value of the public header's
  // FBSTAB_HIP_DENSE_ORDER_* (kDenseOrder* below), FBSTAB_HIP_DENSE_SPREAD_BITS (> 0), FBSTAB_HIP_DENSE_STICKY
  // (0 / 1) and FBSTAB_HIP_DENSE_ACT_BITS (0..999).  -1, and spread bits 0: the layout's default stands.
  int dense_order = -1;
  int dense_spread_bits = 0;
  int dense_sticky = -1;
  int dense_act_bits = -1;
};

constexpr int kDenseOrderAuto = 0, kDenseOrderPivoted = 1, kDenseOrderNatural = 2;

// The variables' values as text, nullptr: unset.
struct CreateKnobText {
  const char *generic = nullptr, *flat_adjoint = nullptr, *lds_pad_bytes = nullptr, *wgs_per_cu = nullptr,
             *max_workgroups = nullptr, *dense_threads = nullptr, *dense_order = nullptr,
             *dense_spread_bits = nullptr, *dense_sticky = nullptr, *dense_act_bits = nullptr;
};

// atoi of a variable that may be unset (0 then), kept where it is positive
inline int positive_or_zero(const char* text) { return text && atoi(text) > 0 ? atoi(text) : 0; }

inline CreateKnobs create_knobs_from(const CreateKnobText& t) {
  CreateKnobs k;
  k.generic = t.generic && atoi(t.generic) > 0;
  if (t.flat_adjoint && *t.flat_adjoint) k.flat_adjoint = atoi(t.flat_adjoint) > 0 ? 1 : 0;
  k.lds_pad_bytes = positive_or_zero(t.lds_pad_bytes) & ~15;
  k.wgs_per_cu = positive_or_zero(t.wgs_per_cu);
  k.max_workgroups = positive_or_zero(t.max_workgroups);
  k.dense_threads = t.dense_threads ? atoi(t.dense_threads) : 0;
  if (t.dense_order && !strcmp(t.dense_order, "auto")) k.dense_order = kDenseOrderAuto;
  if (t.dense_order && !strcmp(t.dense_order, "natural")) k.dense_order = kDenseOrderNatural;
  if (t.dense_order && !strcmp(t.dense_order, "pivoted")) k.dense_order = kDenseOrderPivoted;
  k.dense_spread_bits = positive_or_zero(t.dense_spread_bits);
  if (t.dense_sticky) k.dense_sticky = atoi(t.dense_sticky) != 0 ? 1 : 0;
  if (t.dense_act_bits && atoi(t.dense_act_bits) >= 0 && atoi(t.dense_act_bits) < 1000)
    k.dense_act_bits = atoi(t.dense_act_bits);
  return k;
}

inline CreateKnobs create_knobs() {
  CreateKnobText t;
  t.generic = getenv("FBSTAB_HIP_GENERIC");
  t.flat_adjoint = getenv("FBSTAB_HIP_FLAT_ADJOINT");
  t.lds_pad_bytes = getenv("FBSTAB_HIP_LDS_PAD_BYTES");
  t.wgs_per_cu = getenv("FBSTAB_HIP_WGS_PER_CU");
  t.max_workgroups = getenv("FBSTAB_HIP_MAX_WORKGROUPS");
  t.dense_threads = getenv("FBSTAB_HIP_DENSE_THREADS");
  t.dense_order = getenv("FBSTAB_HIP_DENSE_ORDER");
  t.dense_spread_bits = getenv("FBSTAB_HIP_DENSE_SPREAD_BITS");
  t.dense_sticky = getenv("FBSTAB_HIP_DENSE_STICKY");
  t.dense_act_bits = getenv("FBSTAB_HIP_DENSE_ACT_BITS");
  return create_knobs_from(t);
}

// What a dense handle makes of FBSTAB_HIP_DENSE_THREADS: 256 - the four-wavefront kernel on a problem the
// one-wavefront kernel would take (comparisons); 64 - the four-wavefront kernel's one-wavefront instance with K in
// LDS, for nz + nl <= 64 only; 0 - the knob does not apply.
inline int dense_threads_choice(const CreateKnobs& k, int nz, int nl) {
  if (k.dense_threads == 64 && nz + nl <= 64) return 64;
  return k.dense_threads == 256 ? 256 : 0;
}

// Read at every call of a sweep entry point (tests switch them between two calls on one handle):
// FBSTAB_HIP_SWEEP_PER_STEP=1 keeps the receding sweep of a record handle on one launch per step, which the
// flat-vector kernel always uses; FBSTAB_HIP_SWEEP_ADJOINT_PER_STEP=1 does the same to the sweep adjoint.
inline bool sweep_per_step_from(const char* text) { return text && atoi(text) != 0; }
inline bool sweep_per_step() { return sweep_per_step_from(getenv("FBSTAB_HIP_SWEEP_PER_STEP")); }
inline bool sweep_adjoint_per_step_from(const char* text) { return text && atoi(text) != 0; }
inline bool sweep_adjoint_per_step() {
  return sweep_adjoint_per_step_from(getenv("FBSTAB_HIP_SWEEP_ADJOINT_PER_STEP"));
}

// ---------------------------------------------------------------------------------------------------------------
// Geometry at creation.

struct LaunchPlan {
  int workgroups = 0;
  long long scratch_bytes = 0;
};

// the resident workgroups per CU the plans count with: the occupancy query's answer, in 1..8
inline int resident_per_cu(int occupancy) { return occupancy < 1 ? 1 : occupancy > 8 ? 8 : occupancy; }

inline int capped_workgroups(int workgroups, const CreateKnobs& k) {
  return k.max_workgroups > 0 && workgroups > k.max_workgroups ? k.max_workgroups : workgroups;
}

// An MPC handle.  `occupancy`: workgroups of the solve kernel a CU holds; `record`: the handle runs on a record
// instance of `qps_per_wg` QPs per workgroup (1 on the flat-vector kernel); `ws_doubles`: scratch of one QP slot.
inline LaunchPlan mpc_plan(int cus, int occupancy, int handles_in_flight, int hw_queues, bool record,
                           int qps_per_wg, int max_batch, long long ws_doubles, const CreateKnobs& k) {
  // a handle that shares the device with others takes its share of the resident workgroups (and of the
  // scratch memory that goes with them), at least one per CU: the launches that can really run beside it - no
  // more than the process has hardware queues - want twice the resident slots between them, so that waiting
  // workgroups fill the SIMDs a launch frees in its tail (fb_in_flight.h)
  int per_cu = in_flight_wgs_per_cu(resident_per_cu(occupancy), handles_in_flight, hw_queues);
  if (k.wgs_per_cu > 0) per_cu = k.wgs_per_cu;
  LaunchPlan p;
  p.workgroups = cus * per_cu;
  // (record kernels: a batch that does not outnumber the grid is SPREAD, one QP per wavefront - batch_grid below -,
  // so a handle for a small max_batch keeps one workgroup per QP rather than one per four)
  const int need = record ? max_batch : (max_batch + qps_per_wg - 1) / qps_per_wg;
  if (p.workgroups > need) p.workgroups = need;
  p.workgroups = capped_workgroups(p.workgroups, k);
  p.scratch_bytes = ws_doubles * 8 * p.workgroups * qps_per_wg;
  return p;
}

// A dense handle: one QP per workgroup at a time, and no share rule (there is no dense create_in_flight).  Scratch:
// `wave` (the one-wavefront kernel, fb_dense_wave.h) - A' and the multipliers of every workgroup, ws_doubles each;
// `k_global` (fb_dense.h) - K and, where they are there too, the iterate vectors of every workgroup, kv_doubles
// each; a four-wavefront kernel with everything in LDS has none.
inline LaunchPlan dense_plan(int cus, int occupancy, int max_batch, bool wave, long long ws_doubles, bool k_global,
                             long long kv_doubles, const CreateKnobs& k) {
  const int per_cu = k.wgs_per_cu > 0 ? k.wgs_per_cu : resident_per_cu(occupancy);
  LaunchPlan p;
  p.workgroups = cus * per_cu;
  if (p.workgroups > max_batch) p.workgroups = max_batch;
  p.workgroups = capped_workgroups(p.workgroups, k);
  if (wave)
    p.scratch_bytes = 8 * ws_doubles * p.workgroups;
  else if (k_global)
    p.scratch_bytes = 8 * kv_doubles * p.workgroups;
  return p;
}

// ---------------------------------------------------------------------------------------------------------------
// Geometry per launch.

// Grid of an MPC batch launch on a kernel of `per_wg` QPs per workgroup.  Record kernels, a batch of no more QPs
// than the handle has workgroups: one QP per WAVEFRONT (row 0 of each; fb_record_kernel.h, R16Queue::fetch) instead
// of four - the rows of a wavefront share its program counter and its cooperative passes, so four QPs on one
// wavefront finish with the slowest of them and queue for each other's passes, while the chip has SIMDs to spare
// (LABNOTES round 6: batch 16, 7.9 -> ms below).  (The flat-vector kernels run one QP per workgroup, on record
// handles too: with per_wg = 1 the same rule gives them min(batch, workgroups).)
inline int batch_grid(int batch, int workgroups, int per_wg) {
  int grid = (batch + per_wg - 1) / per_wg;
  if (batch <= workgroups) grid = batch;
  return grid > workgroups ? workgroups : grid;
}

// The spread has a partner on the device: R16Queue::fetch gives a QP to row 0 of each wavefront only when
// `batch <= gridDim.x`.  It sees the grid, not the handle's workgroups, so the two agree because batch_grid
// returns `batch` exactly when batch <= workgroups and less than `batch` otherwise:
//     record_spreads(batch, batch_grid(batch, workgroups, per_wg))  ==  (batch <= workgroups)
// for every per_wg (tests/test_launch_plan.py checks the table).  A grid rule that breaks this leaves rows idle
// in a packed launch, or packs a launch whose scratch was sized for the spread.  (Host only: the device states its
// condition itself.)
inline bool record_spreads(int batch, int grid) { return batch <= grid; }

// ... and of a FBSTAB_HIP_KEEP_MATRICES launch, the one-launch sweep included: QP q in slot q, every row taken.
inline int keep_grid(int batch, int qps_per_wg) { return (batch + qps_per_wg - 1) / qps_per_wg; }

// Grid of a dense batch launch: one QP per workgroup at a time.
inline int dense_grid(int batch, int workgroups) { return workgroups < batch ? workgroups : batch; }

// One QP per slot, slot = QP index: what a FBSTAB_HIP_KEEP_MATRICES launch and the one-launch sweeps need of the
// handle's grid (the slots are what mpc_plan sized the scratch for).
inline bool slots_hold(int batch, int workgroups, int qps_per_wg) { return batch <= workgroups * qps_per_wg; }

// Record handles: the whole receding sweep is ONE launch of the KEEP instance, every row looping over its own
// trajectory - where every trajectory has a slot and the step count fits the 16 bits a row counts its steps in
// (R16Queue::fetch, `swept`); `per_step`: sweep_per_step() above.
inline bool sweep_in_one_launch(bool record, int batch, int workgroups, int qps_per_wg, int steps, bool per_step) {
  return record && slots_hold(batch, workgroups, qps_per_wg) && steps < 0xffff && !per_step;
}

// The seed vectors of the one-launch sweep adjoint: nz doubles per QP slot of the handle's grid.
inline size_t sweep_seed_bytes(long long nz, int workgroups, int qps_per_wg) {
  return sizeof(double) * (size_t)nz * (size_t)workgroups * (size_t)qps_per_wg;
}

}  // namespace fbk
