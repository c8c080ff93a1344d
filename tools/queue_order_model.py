#!/usr/bin/env python3
"""The queue of a record launch as a model on the CPU: what the order in which QPs are handed out does to `packing`
(useful row-steps / row slots of the live wavefronts) and to the length of a launch.  LABNOTES R7.1 has the tables
this prints beside what the device measured; fb_queue_order_plan.h is the rule it led to.

The model: a wavefront has 4 rows; one time unit is one wave-level Newton step; a row that finishes its QP takes the
next ticket of the launch's counter (rows that finish in the same step in row order); a wavefront exits when the
counter is dry and all its rows are idle, and only then is its SIMD slot free for a waiting workgroup.  It ignores
the cooperative passes between the steps (their cost follows the number of calls, not packing) and the order in
which wavefronts really reach the counter.  The Newton counts are the oracle's for the benchmark's batch (they are
the device's: the parity tests), about 10 s for 8192 QPs.

usage: tools/queue_order_model.py [--batch 8192] [--closed-loop 2048]
  table 1  one launch alone, 1024 / 512 / 256 workgroups: packing and duration, index order against longest-first
  table 2  launches in flight on 1024 SIMD slots: streams share hardware queues, a stream's launches follow each other
  table 3  (--closed-loop B > 0) B plants stepped through three closed-loop steps, x+ = A x + B u0, each step solved
           cold: the rank correlation of consecutive steps' counts, and packing when a step's queue is ordered by the
           previous step's counts"""
import argparse
import heapq
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROWS = 4
SLOTS = 1024  # one-wavefront workgroups the chip holds: 256 CUs x 4 SIMDs


def one_launch(lengths, workgroups, start=None):
    """`lengths`: the QPs' Newton counts in ticket order.  `start`: per workgroup, the step at which it starts (default
    0).  -> (exit step of every workgroup, busy row-steps)."""
    start = np.zeros(workgroups, dtype=np.int64) if start is None else np.asarray(start, dtype=np.int64)
    free = [(int(start[w]), w * ROWS + r) for w in range(workgroups) for r in range(ROWS)]
    heapq.heapify(free)
    end = start.copy()
    for n in lengths:
        t, row = heapq.heappop(free)
        t += int(n)
        end[row // ROWS] = max(end[row // ROWS], t)
        heapq.heappush(free, (t, row))
    return end, int(np.sum(lengths))


def packing_alone(lengths, workgroups):
    end, busy = one_launch(lengths, workgroups)
    return busy / float(ROWS * end.sum()), int(end.max())


def in_flight(lengths, queues, lanes, workgroups, launches_per_lane=6):
    """`lanes` streams on `queues` hardware queues (stream s on queue s mod queues), every stream launching the batch
    again and again; a queue starts its next launch when the previous one has exited altogether; the workgroups
    of a started launch take SIMD slots as they come free, launches in the order they started.  Starts staggered by
    a quarter of a launch.  -> busy row-steps / all row slots between the first and the last launch's middle."""
    order = [(k * lanes + s) for k in range(launches_per_lane) for s in range(lanes)]  # issue order of the launches
    queue_free = [0] * queues
    slots = [0] * SLOTS
    heapq.heapify(slots)
    alone = one_launch(lengths, workgroups)[0].max()
    spans = []
    for i, launch in enumerate(order):
        s = launch % lanes
        q = s % queues
        t0 = max(queue_free[q], (i * alone) // (4 * lanes) if i < lanes else 0)
        starts = []
        for _ in range(workgroups):
            starts.append(max(t0, heapq.heappop(slots)))
        end, busy = one_launch(lengths, workgroups, start=np.array(sorted(starts)))
        for e in end:
            heapq.heappush(slots, int(e))
        queue_free[q] = int(end.max())
        spans.append((sorted(starts), end, busy))
    # steady state: the row slots of all SIMDs over the window of the middle launches
    lo = min(s[0][0] for s in spans[lanes:2 * lanes])
    hi = min(s[0][0] for s in spans[-lanes:])
    busy = 0.0
    for starts, end, b in spans:
        a, e = starts[0], int(end.max())
        if e <= lo or a >= hi:
            continue
        busy += b * (min(e, hi) - max(a, lo)) / float(e - a)  # (a launch's work spread evenly over its span)
    return busy / float(ROWS * SLOTS * (hi - lo))


def spearman(a, b):
    ra, rb = np.argsort(np.argsort(a, kind="stable")), np.argsort(np.argsort(b, kind="stable"))
    return float(np.corrcoef(ra, rb)[0, 1])


def longest_first(lengths, by=None):
    """The order kernel's sort: descending by `by` (default: the lengths themselves) clamped to [0, 255], stable."""
    key = np.clip(lengths if by is None else by, 0, 255)
    return np.asarray(lengths)[np.argsort(-key, kind="stable")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--closed-loop", type=int, default=0, metavar="B")
    args = ap.parse_args()
    from tools import fixtures as fx
    from oracle.oracle_py import Oracle
    orc = Oracle(False)
    nt = orc.num_threads()
    p = fx.synthetic_mpc_batch(args.batch)
    n = orc.solve_mpc(p, nthreads=nt)[4]["newton_iters"].astype(np.int64)
    print("batch %d: Newton counts %d .. %d, mean %.2f, sum %d" % (args.batch, n.min(), n.max(), n.mean(), n.sum()))
    print("\ntable 1: one launch alone                      index order        longest-first")
    for w in (1024, 512, 256):
        (pa, da), (pb, db) = packing_alone(n, w), packing_alone(longest_first(n), w)
        print("  %4d workgroups: packing %.3f -> %.3f   duration %3d -> %3d steps   wave-level steps %d -> %d"
              % (w, pa, pb, da, db, round(n.sum() / (ROWS * pa)), round(n.sum() / (ROWS * pb))))
    print("\ntable 2: launches in flight on %d SIMD slots, busy row-steps / all row slots" % SLOTS)
    for queues, lanes, w in ((8, 8, 256), (4, 8, 256), (4, 8, 512)):
        print("  %d queues, %d lanes, %3d workgroups per launch: %.3f -> %.3f"
              % (queues, lanes, w, in_flight(n, queues, lanes, w), in_flight(longest_first(n), queues, lanes, w)))
    if args.closed_loop > 0:
        B = args.closed_loop
        A, Bm = fx.quadrotor_model()
        q = fx.synthetic_mpc_batch(B)
        nx, nu = q.nx, q.nu
        counts = []
        for _ in range(4):
            z, _, _, _, out = orc.solve_mpc(q, nthreads=nt)
            counts.append(out["newton_iters"].astype(np.int64))
            x0 = q.arrays["x0"]
            q.arrays["x0"] = np.ascontiguousarray(x0 @ A.T + z[:, nx:nx + nu] @ Bm.T)
        print("\ntable 3: %d plants, closed loop, every step solved cold" % B)
        print("  rank correlation of consecutive steps' counts: " +
              ", ".join("%.2f" % spearman(a, b) for a, b in zip(counts, counts[1:])))
        cur, prev = counts[1], counts[0]
        print("  rows, QPs per row        index order   by previous step   perfect knowledge")
        for rows in (1024, 512, 256):
            w = rows // ROWS
            print("  %4d rows, %d per row:       %.3f           %.3f               %.3f"
                  % (rows, B // rows, packing_alone(cur, w)[0], packing_alone(longest_first(cur, by=prev), w)[0],
                     packing_alone(longest_first(cur), w)[0]))
        print("  a lone launch of %d rows: %d -> %d steps" % (1024, packing_alone(cur, 256)[1],
                                                             packing_alone(longest_first(cur, by=prev), 256)[1]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
