#!/usr/bin/env python3
"""The condensed route for MPC QPs (fbstab_amd/condense.py: CondensedMpc) against FBstabMpcBatch.Solve on the same
QPs, device tensors, one GPU, one process, at three workloads:
  flat_10_40_3_6      (N, nx, nu, nc) = (10, 40, 3, 6), 2048 QPs: a shape the flat-vector MPC kernel serves; condensed
                      it is dense (33, 0, 66), the one-wavefront dense kernel
  record_15_12_4_20   (15, 12, 4, 20), 2048 QPs: a shape a record kernel serves; condensed (64, 0, 320)
  lti_10_40_3_6       the first shape time-invariant with ONE model shared by 2048 QPs (stride-0 matrices, one image
                      of H_c and A_c) and per-QP x0 and d: Solve(recondense="vectors")
The QPs are tools/fixtures.random_ltv_mpc with dyn_noise = 0.05 (at the default 0.15 the open loop of nx = 40 grows
by three orders of magnitude over the horizon).  Every call is warmed once, then timed --reps times with torch events
on torch's current stream, the two sides and the parts ALTERNATING within a round; median, min and max in ms.
  (a) the kernels: Condense "all", Condense "vectors", expand
  (b) CondensedMpc.Solve from a cold start - and its parts: condense as the workload asks, the dense solve, expand -
      against FBstabMpcBatch.Solve from a cold start; `all_converged` of each side, `condensed_over_mpc` the ratio of
      the medians.
Prints one JSON line (profiles/condense_bench.json) with the library's sha256.

usage: python tools/condense_bench.py [--reps 7] [--batch 2048]"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def lti_problem(rng, batch, N, nx, nu, nc):
    """One random model over the horizon, shared ((1, len) matrix sequences); x0, q, r, c, d per QP, d strictly
    feasible along the free response."""
    from tools import fixtures as fx
    p = fx.random_ltv_mpc(rng, 1, N, nx, nu, nc, dyn_noise=0.05)
    a = {}
    for k, n in (("Q", nx * nx), ("R", nu * nu), ("S", nu * nx), ("A", nx * nx), ("B", nx * nu), ("E", nc * nx),
                 ("L", nc * nu)):
        stages = p.arrays[k].shape[1] // n
        a[k] = np.tile(p.arrays[k][:, :n], (1, stages))
    a["q"] = 0.1 * rng.standard_normal((batch, (N + 1) * nx))
    a["r"] = 0.1 * rng.standard_normal((batch, (N + 1) * nu))
    a["c"] = 0.05 * rng.standard_normal((batch, N * nx))
    a["x0"] = 0.5 * rng.standard_normal((batch, nx))
    A = a["A"][0, :nx * nx].reshape(nx, nx).T
    E = a["E"][0, :nc * nx].reshape(nx, nc).T
    d = np.zeros((batch, N + 1, nc))
    x = a["x0"].copy()
    for i in range(N + 1):
        d[:, i] = -(x @ E.T) - (0.2 + 0.8 * rng.random((batch, nc)))
        if i < N:
            x = x @ A.T + a["c"][:, i * nx:(i + 1) * nx]
    a["d"] = d.reshape(batch, -1)
    q = fx.MpcProblem(N, nx, nu, nc)
    q.arrays = {k: np.ascontiguousarray(v) for k, v in a.items()}
    return q


def stats(ms):
    return dict(median_ms=float(np.median(ms)), min_ms=float(np.min(ms)), max_ms=float(np.max(ms)))


def run(name, p, recondense, reps):
    import torch
    from fbstab_amd import hip_api
    from fbstab_amd.condense import CondensedMpc
    dev = torch.device("cuda:0")
    B = p.arrays["x0"].shape[0]
    N, nx, nu, nc = p.sizes()
    data = {k: torch.from_numpy(np.ascontiguousarray(a)).to(dev) for k, a in p.arrays.items()}
    s = CondensedMpc(N, nx, nu, nc, max_batch=B)
    m = hip_api.FBstabMpcBatch(N, nx, nu, nc, max_batch=B)
    zeros = lambda n: torch.zeros((B, n), dtype=torch.float64, device=dev)
    nz, nl, nv, nzc = s.nz, s.nl, s.nv, s.nzc
    state = {}

    def cold():
        return zeros(nz), zeros(nl), zeros(nv), zeros(nv)

    def condensed_solve():
        x = cold()
        state["c_out"] = s.Solve(data, *x, recondense=recondense)
        state["c_x"] = x

    def mpc_solve():
        x = cold()
        state["m_out"] = m.Solve(data, *x)

    def dense_solve():
        img = s._img
        state["d_x"] = (zeros(nzc), torch.zeros((B, 0), dtype=torch.float64, device=dev), zeros(nv), zeros(nv))
        s.dense.Solve(dict(H=img["H"], f=img["f"], A=img["A"], b=img["b"]), *state["d_x"], async_=True)

    def expand():
        U, _, v, y = state["d_x"]
        s._expand(data, U, v, y, *cold())

    calls = dict(condense_all=lambda: s.Condense(data, "all"), condense_vectors=lambda: s.Condense(data, "vectors"),
                 dense_solve=dense_solve, expand=expand, condensed_solve=condensed_solve, mpc_solve=mpc_solve)
    times = {k: [] for k in calls}
    for r in range(reps + 1):   # (round 0 warms)
        for k, f in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            if r:
                times[k].append(e0.elapsed_time(e1))
    oc, om = hip_api.out_to_numpy(state["c_out"]), hip_api.out_to_numpy(state["m_out"])
    res = {k: stats(v) for k, v in times.items()}
    res.update(shape=[N, nx, nu, nc], batch=B, dense_shape=[nzc, 0, nv], recondense=recondense,
               condense_in_solve="condense_" + recondense,
               mpc_kernel=m.kernel_name(), lds_bytes=s.lds_bytes,
               condensed_all_converged=bool((oc["eflag"] == 0).all()), mpc_all_converged=bool((om["eflag"] == 0).all()),
               condensed_success=int((oc["eflag"] == 0).sum()), mpc_success=int((om["eflag"] == 0).sum()),
               condensed_newton_mean=float(oc["newton_iters"].mean()), mpc_newton_mean=float(om["newton_iters"].mean()),
               condensed_over_mpc=res["condensed_solve"]["median_ms"] / res["mpc_solve"]["median_ms"])
    s.close()
    m.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--batch", type=int, default=2048)
    a = ap.parse_args()
    assert a.reps >= 5
    from fbstab_amd import hip_api
    from tools import fixtures as fx
    hip_api.load_library()
    rng = np.random.default_rng(2024)
    line = dict(tool="condense_bench", reps=a.reps,
                library_sha256=hashlib.sha256(open(hip_api.current_library_path(), "rb").read()).hexdigest())
    line["flat_10_40_3_6"] = run("flat", fx.random_ltv_mpc(rng, a.batch, 10, 40, 3, 6, dyn_noise=0.05), "all", a.reps)
    line["record_15_12_4_20"] = run("record", fx.random_ltv_mpc(rng, a.batch, 15, 12, 4, 20, dyn_noise=0.05), "all",
                                    a.reps)
    line["lti_10_40_3_6"] = run("lti", lti_problem(rng, a.batch, 10, 40, 3, 6), "vectors", a.reps)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
