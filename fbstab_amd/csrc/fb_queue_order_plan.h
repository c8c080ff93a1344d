// When a record handle hands its queue tickets out longest-first: the rule behind the order that
// fbstab_mpc_queue_order_kernel (fb_queue_order.h) leaves behind a batch solve, as pure host functions (no HIP
// types: tests/test_queue_order_plan.py compiles this header with the host compiler alone).
//
// The rows of a packed record launch pull QP indices 0, 1, 2, ... from the queue word, and a wavefront lives until
// the slowest of its rows is done: when the queue runs dry the rows stand at random points of QPs of 5 to 98 Newton
// steps, and the idle rows of a live wavefront are the launch's `packing` loss (LABNOTES R7.1: 0.82 at 1024
// workgroups).  Handing the LONGEST QPs out first leaves only short ones for the drain.  Nothing known before a
// solve carries the lengths; the previous solve of the same batch does (a controller that serves a fleet calls the
// handle with the same plants one time step later: rank correlation 0.91-0.93 between consecutive steps).  So a
// handle remembers, per QP index, the Newton count of its last packed batch solve, sorted descending, and the next
// solve of the SAME batch size translates ticket t into QP order[t].  The order is a hint: a QP's bits do not
// depend on the row, the wavefront or the neighbours that solve it, so a stale order costs the gain and no more.
#pragma once
#include <cstdlib>

namespace fbk {

// FBSTAB_HIP_QUEUE_ORDER as text (nullptr: unset) -> whether a handle keeps and uses the order: on unless the
// variable holds a number that is 0 (atoi, as the knobs of fb_launch_plan.h: text that is no number reads as 0;
// empty: unset).  Read once per MPC handle, when it is created, like the knobs of that header's CreateKnobs - and
// here, not there, because this header stands alone: the staging header's include closure (fb_launch_plan.h,
// fb_in_flight.h) and the list of variables fb_launch_plan.h reads are both pinned by tests.
inline bool queue_order_knob_from(const char* text) { return !(text && *text) || atoi(text) != 0; }
inline bool queue_order_knob() { return queue_order_knob_from(getenv("FBSTAB_HIP_QUEUE_ORDER")); }

// A launch whose Newton counts become the handle's order: a batch solve of a record instance that is packed
// (`spread`: record_spreads of fb_launch_plan.h - one QP per wavefront, no queue to order), on a handle with the
// knob on.  KEEP solves, sweeps, adjoints, tangents, multi-RHS solves and probes are no `record_batch_solve`.
inline bool queue_order_sorts(bool knob, bool record_batch_solve, bool spread, int batch) {
  return knob && record_batch_solve && !spread && batch >= 1;
}

// ... and a launch that hands its tickets out in the stored order: one whose own counts will be sorted, of the
// batch size the stored order was made for (`order_batch`, -1: none).
inline bool queue_order_applies(bool knob, bool record_batch_solve, bool spread, int batch, int order_batch) {
  return queue_order_sorts(knob, record_batch_solve, spread, batch) && order_batch == batch;
}

// The stored order's batch size after a launch on the handle: a launch that sorts installs its own, anything else
// leaves what there was.
inline int queue_order_batch_after(bool sorts, int batch, int order_batch) { return sorts ? batch : order_batch; }

}  // namespace fbk
