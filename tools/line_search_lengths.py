#!/usr/bin/env python3
"""The line search of a record launch as a model on the CPU: how many step lengths a Newton step rejects (f) on the
benchmark's QPs, and what that makes of the number of cooperative trial passes when a pass evaluates K lengths.
LABNOTES R7.2 has what this prints beside what the device measured (the counts agree; fewer passes were not faster
ones); kCoopLineSearchTrials (fb_algorithm.h) is the constant it was written to choose.

The model: the first length (t = 1) comes with the Newton step; a step that fails f sufficient-decrease tests needs
the norms at t beta, ..., t beta^f (the one after the last allowed test is taken as it is, and its norms are the next
loop-top values), K of them per pass: ceil(f / K) passes.  Every pass serves one QP with the whole wavefront, so the
launch's wave-level calls are the sum over its QPs.  f is read off the oracle's trace: a FBSTAB_TRACE_DETAILED_LINE
record of inner iteration i >= 1 carries the step length t = beta^f the step before it was taken with.  (A step that
is the last of its proximal iteration by max_inner_iters has no such record; none of the benchmark's QPs has one.)
About 10 ms per QP and core.

usage: tools/line_search_lengths.py [--batch 8192] [--first-id 0] [--procs P]"""
import argparse
import math
import multiprocessing
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KS = (4, 6, 8, 12)
DETAILED_LINE = 3  # fbstab_trace_kind (include/fbstab_types.h)


def fails_of_records(records, beta):
    """f of every Newton step of one traced solve, in order (`records`: Oracle.solve_display()[6])."""
    rec = np.asarray(records)
    t = rec[(rec[:, 0] == DETAILED_LINE) & (rec[:, 1] >= 1), 3]
    f = np.rint(np.log(t) / math.log(beta)).astype(np.int64)
    assert (f >= 0).all()
    return f


def fails_of_problem(oracle, prob, opts=None):
    """f of every Newton step of every QP of `prob` (an MpcProblem), QP after QP."""
    from oracle.oracle_py import default_options
    from tools import fixtures as fx
    opts = opts or default_options()
    out = []
    for b in range(prob.batch):
        one = fx.MpcProblem(*prob.sizes())
        one.arrays = {k: np.ascontiguousarray(v[b:b + 1]) for k, v in prob.arrays.items()}
        out.append(fails_of_records(oracle.solve_display(one, opts=opts, trace_cap=1 << 16)[6], opts.beta))
    return np.concatenate(out) if out else np.zeros(0, dtype=np.int64)


def histogram(f, top=None):
    return np.bincount(f, minlength=(int(f.max()) if top is None else top) + 1)


def passes(f, K):
    """Cooperative trial passes of the steps `f` at K lengths per pass."""
    return int(((np.asarray(f) + K - 1) // K).sum())


def passes_per_step(f, K):
    return passes(f, K) / float(len(f))


def _chunk(args):
    first, count = args
    from oracle.oracle_py import Oracle
    from tools import fixtures as fx
    return fails_of_problem(Oracle(False), fx.synthetic_mpc_batch(count, first_id=first))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--first-id", type=int, default=0)
    ap.add_argument("--procs", type=int, default=min(16, os.cpu_count() or 1))
    args = ap.parse_args()
    from oracle.oracle_py import Oracle
    Oracle(False)  # (builds the library where it is missing, before the workers look for it)
    step = 32
    jobs = [(args.first_id + a, min(step, args.batch - a)) for a in range(0, args.batch, step)]
    with multiprocessing.Pool(args.procs) as pool:
        f = np.concatenate(pool.map(_chunk, jobs))
    h = histogram(f, top=20)
    n = len(f)
    print("batch %d (ids %d ..): %d Newton steps, %d rejected step lengths = %.2f per step"
          % (args.batch, args.first_id, n, int(f.sum()), f.sum() / float(n)))
    print("\ntable 1: failed sufficient-decrease tests per Newton step (f)")
    print("  f      " + " ".join("%6d" % i for i in range(len(h))))
    print("  steps  " + " ".join("%6d" % c for c in h))
    print("  share  " + " ".join("%6.3f" % (c / float(n)) for c in h))
    groups = ((0, 0), (1, 4), (5, 8), (9, 12), (13, 16), (17, 20))
    print("  " + ", ".join("f %s: %.3f" % ("%d" % a if a == b else "%d-%d" % (a, b), h[a:b + 1].sum() / float(n))
                           for a, b in groups))
    print("\ntable 2: cooperative trial passes at K step lengths per pass (sum of ceil(f / K))")
    base = passes(f, 4)
    for K in KS:
        print("  K = %2d: %.3f passes per step, %7d wave-level passes in the launch (%+.1f %% against K = 4)"
              % (K, passes_per_step(f, K), passes(f, K), 100.0 * (passes(f, K) - base) / base))
    return 0


if __name__ == "__main__":
    sys.exit(main())
