#!/usr/bin/env python3
"""The Jacobians dz/df and dz/db of a batch of dense solutions, two ways, at BASELINE configs[1]'s shape (nz, nl, nv) =
(50, 10, 100) (the one-wavefront kernel) and at (90, 12, 77) (four wavefronts, K in LDS), device tensors, one GPU:
  (a) one factorisation per column: ONE fbstab_hip_dense_adjoint_batch call on the points replicated nrhs-fold (the
      data too) with the unit seed of column k on copy k - a handle of max_batch = batch x nrhs;
  (b) one factorisation per QP: ONE fbstab_hip_dense_jacobian_batch call (dz, dl, dv wanted, as (a) returns them).
Each shape at a full grid (batch = the workgroups of a max_batch = 4096 handle: every workgroup one QP) and at a
quarter of it.  One fresh child process per (shape, batch) under a time limit of its own; after a child that failed,
faulted or ran out of time no further child is started on the GPU.  A child solves once, warms every call once, then
times --reps rounds in which the calls ALTERNATE (a_f, b_f, a_b, b_b, and fbstab_hip_dense_kkt_solve_batch with ONE
seed: a factorisation and one solve on the many-right-hand-side kernel).  Times: torch events around the whole call
on torch's current stream (the allocation of the results included, as a caller pays it), and the handle's
last_kernel_ms; medians.  From the kernel times of (b) at nrhs right-hand sides and of the one-seed call,
T(n) = F + n R per QP in flight: `resolve_over_factor` is R / F, the cost of one further right-hand side as a fraction
of a factorisation.  Prints one JSON line (profiles/dense_kkt_multi_bench.json) with the library's sha256; `b_over_a`
is (b)'s call over (a)'s, `b_faster` says whether (b)'s median is below (a)'s by more than the larger spread of the two.

usage: python tools/dense_kkt_multi_bench.py [--reps 5]"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"config1_50_10_100": (50, 10, 100), "four_wavefronts_90_12_77": (90, 12, 77)}
GRID_MAX_BATCH = 4096   # (BASELINE configs[1]: the handle whose grid the batches are sized by)
FRACTIONS = {"grid_full": 1, "grid_quarter": 4}
CHILD_SECONDS = 420   # one child: set-up, one solve, (reps + 1) x 5 calls


def child(name, fraction, reps):
    import torch
    from fbstab_amd import hip_api
    from tools import fixtures as fx
    dev = torch.device("cuda:0")
    nz, nl, nv = SHAPES[name]
    s = hip_api.FBstabDenseBatch(nz, nl, nv, max_batch=GRID_MAX_BATCH)
    B = max(s.query()["workgroups"] // FRACTIONS[fraction], 1)
    p = fx.synthetic_dense_batch(B, nz, nl, nv)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    data = {k: t(a) for k, a in p.arrays.items()}
    zeros = lambda n: torch.zeros((B, n), dtype=torch.float64, device=dev)
    z, l, v, y = zeros(nz), zeros(nl), zeros(nv), zeros(nv)
    out = s.Solve(data, z, l, v, y)
    torch.cuda.synchronize()
    calls, handles = {}, {}
    eye = lambda n, sign: (sign * torch.eye(n, dtype=torch.float64, device=dev)).repeat(B, 1).contiguous()
    for wrt, n in (("f", nz), ("b", nv)):
        rep = lambda a, n=n: a.repeat_interleave(n, dim=0).contiguous()
        h = hip_api.FBstabDenseBatch(nz, nl, nv, max_batch=B * n)
        rdata = {k: rep(a) for k, a in data.items()}
        rx = tuple(rep(a) for a in (z, l, v))
        gz = eye(nz, -1.0) if wrt == "f" else torch.zeros((B * n, nz), dtype=torch.float64, device=dev)
        gv = eye(nv, 1.0) if wrt == "b" else None
        calls["a_" + wrt] = lambda h=h, rdata=rdata, rx=rx, gz=gz, gv=gv: h.Adjoint(rdata, *rx, gz, None, gv, want=(), adj=True)
        calls["b_" + wrt] = lambda wrt=wrt: s.Jacobian(data, z, l, v, wrt=wrt, want=("dz", "dl", "dv"))
        handles["a_" + wrt], handles["b_" + wrt] = h, s
    one = torch.ones((B, 1, nz), dtype=torch.float64, device=dev)
    calls["b_one_seed"] = lambda: s.KktSolve(data, z, l, v, one)
    handles["b_one_seed"] = s
    ms = {k: [] for k in calls}
    kernel_ms = {k: [] for k in calls}
    check, bad = {}, {}
    for _ in range(reps + 1):   # (the first round warms the code objects and the handles' buffers)
        for k, call in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g = call()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1))
            kernel_ms[k].append(handles[k].last_kernel_ms())
            bad[k] = int((g["status"] != 0).sum().item())
            check[k] = float(g["dz"].abs().sum().item())
            del g
    med = lambda a: round(float(np.median(a[1:])), 3)
    print(json.dumps({"workload": name, "fraction": fraction, "shape": [nz, nl, nv], "batch": B,
                      "columns": {"f": nz, "b": nv}, "call_ms": {k: med(a) for k, a in ms.items()},
                      "call_ms_all": {k: [round(x, 3) for x in a[1:]] for k, a in ms.items()},
                      "kernel_ms": {k: med(a) for k, a in kernel_ms.items()},
                      "kernel_ms_all": {k: [round(x, 3) for x in a[1:]] for k, a in kernel_ms.items()},
                      "abs_sum_dz": check, "status_nonzero": bad, "launch": s.query(),
                      "success": int((hip_api.out_to_numpy(out)["eflag"] == 0).sum())}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--child", nargs=2, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], a.child[1], a.reps)
    from fbstab_amd import hip_api
    hip_api.load_library()
    with open(hip_api.current_library_path(), "rb") as f:
        sha = hashlib.sha256(f.read()).hexdigest()
    res = {"library_sha256": sha, "rounds_timed": a.reps, "workloads": {}}
    for name in SHAPES:
        for fraction in FRACTIONS:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", name, fraction, "--reps", str(a.reps)]
            what = "%s (%s)" % (name, fraction)
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_SECONDS)
            except subprocess.TimeoutExpired as e:
                sys.stderr.write(str(e.stdout or "")[-2000:] + str(e.stderr or "")[-4000:])
                raise SystemExit("dense_kkt_multi_bench: %s did not end within %d s; stopping" % (what, CHILD_SECONDS))
            if r.returncode != 0:
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                raise SystemExit("dense_kkt_multi_bench: %s ended with status %d; stopping" % (what, r.returncode))
            c = json.loads(r.stdout.strip().splitlines()[-1])
            row = {"shape": c["shape"], "batch": c["batch"], "launch": c["launch"], "success": c["success"],
                   "one_seed_call_ms": c["call_ms"]["b_one_seed"], "one_seed_kernel_ms": c["kernel_ms"]["b_one_seed"],
                   "abs_sum_dz": c["abs_sum_dz"], "status_nonzero": c["status_nonzero"]}
            for wrt, n in c["columns"].items():
                ka, kb = "a_" + wrt, "b_" + wrt
                spread = max(max(c["call_ms_all"][k]) - min(c["call_ms_all"][k]) for k in (ka, kb))
                # T(n) = F + n R from the kernel times of the n-column call and of the one-seed call
                R = (c["kernel_ms"][kb] - c["kernel_ms"]["b_one_seed"]) / (n - 1)
                F = c["kernel_ms"]["b_one_seed"] - R
                row["wrt_" + wrt] = {
                    "columns": n, "a_call_ms": c["call_ms"][ka], "a_call_ms_all": c["call_ms_all"][ka],
                    "a_kernel_ms": c["kernel_ms"][ka], "b_call_ms": c["call_ms"][kb],
                    "b_call_ms_all": c["call_ms_all"][kb], "b_kernel_ms": c["kernel_ms"][kb],
                    "b_over_a": round(c["call_ms"][kb] / c["call_ms"][ka], 4),
                    "b_kernel_over_a_kernel": round(c["kernel_ms"][kb] / c["kernel_ms"][ka], 4),
                    "larger_spread_ms": round(spread, 3), "b_faster": c["call_ms"][kb] + spread < c["call_ms"][ka],
                    "resolve_ms": round(R, 5), "factor_ms": round(F, 5),
                    "resolve_over_factor": round(R / F, 4) if F > 0 else None}
            res["workloads"][name + "_" + fraction] = row
    print(json.dumps(res))


if __name__ == "__main__":
    main()
