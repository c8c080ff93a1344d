#!/usr/bin/env python3
"""The Jacobian dz/dx0 of a batch of solutions, two ways, at the headline shape (N, nx, nu, nc) = (30, 12, 4, 20) and
at one wide shape, (30, 20, 6, 16), device tensors, one GPU:
  (a) one factorisation per column: ONE fbstab_hip_mpc_tangent_batch call on the points replicated nx-fold (the data
      too) with the direction x0 = e_j on copy j - a handle of max_batch = batch x nx;
  (b) one factorisation per QP: ONE fbstab_hip_mpc_x0_sensitivity_batch call (dz, dl, dv and the gain wanted).
Each way in a fresh child process under a time limit of its own; after a child that failed, faulted or ran out of time
no further child is started on the GPU.  A child solves once, then makes --reps + 1 calls (the first warms the code
objects and the handle's buffers).  Times: torch events around the whole call on torch's current stream (the allocation
of the results included, as a caller pays it), and the handle's last_kernel_ms (the adjoint kernel's launch of (a), the
one launch of (b)); medians.  Prints one JSON line (profiles/kkt_multi_bench.json) with the library's sha256;
`b_over_a` is (b)'s call over (a)'s, `b_faster` says whether (b)'s median is below (a)'s by more than the larger
spread of the two.

usage: python tools/kkt_multi_bench.py [--reps 5]"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# name -> (shape, QPs): (a) runs QPs x nx of them.  (b) is one QP per workgroup: the wide shape also at a batch that
# gives every workgroup of a handle's grid (1024 on one MI355X) a QP.
WORKLOADS = {"headline_30_12_4_20": ((30, 12, 4, 20), 1024), "wide_30_20_6_16": ((30, 20, 6, 16), 256),
             "wide_30_20_6_16_grid_full": ((30, 20, 6, 16), 1024)}
WAYS = ("tangent_replicated", "x0_sensitivity")
CHILD_SECONDS = 300   # one child: set-up, one solve, reps + 1 calls


def problem(name):
    from tools import fixtures as fx
    shape, B = WORKLOADS[name]
    if name.startswith("headline"):
        return fx.synthetic_mpc_batch(B)
    one = fx.random_ltv_mpc(np.random.default_rng(5), 64, *shape)   # (bench.py's wide LTV workload, tiled)
    p = fx.MpcProblem(*shape)
    p.arrays = {k: np.ascontiguousarray(np.tile(a, (B // 64, 1))) for k, a in one.arrays.items()}
    return p


def child(name, way, reps):
    import torch
    from fbstab_amd import hip_api
    dev = torch.device("cuda:0")
    p = problem(name)
    B, nx = p.batch, p.nx
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    data = {k: t(a) for k, a in p.arrays.items()}
    s = hip_api.FBstabMpcBatch(*p.sizes(), max_batch=B)
    zeros = lambda n: torch.zeros((B, n), dtype=torch.float64, device=dev)
    z, l, v, y = zeros(p.nz), zeros(p.nl), zeros(p.nv), zeros(p.nv)
    out = s.Solve(data, z, l, v, y)
    torch.cuda.synchronize()
    if way == "tangent_replicated":
        rep = lambda a: a.repeat_interleave(nx, dim=0).contiguous()
        h = hip_api.FBstabMpcBatch(*p.sizes(), max_batch=B * nx)
        rdata = {k: rep(a) for k, a in data.items()}
        rx = tuple(rep(a) for a in (z, l, v))
        dirs = {"x0": torch.eye(nx, dtype=torch.float64, device=dev).repeat(B, 1).contiguous()}
        call = lambda: h.Tangent(rdata, *rx, dirs)
        kernel = h.adjoint_kernel_name()
    else:
        h = s
        call = lambda: h.X0Sensitivity(data, z, l, v, want=("dz", "dl", "dv", "gain"))
        kernel = "fbstab_mpc_kkt_multi_kernel<64>"
    torch.cuda.synchronize()
    ms, kernel_ms = [], []
    for _ in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g = call()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
        kernel_ms.append(h.last_kernel_ms())
        status_nonzero = int((g["status"] != 0).sum().item())
        check = float(g["dz"].abs().sum().item())
        del g
    ms, kernel_ms = ms[1:], kernel_ms[1:]
    print(json.dumps({"workload": name, "way": way, "shape": list(p.sizes()), "batch": B, "columns": nx,
                      "kernel": kernel, "call_ms": round(float(np.median(ms)), 3),
                      "call_ms_all": [round(x, 3) for x in ms], "kernel_ms": round(float(np.median(kernel_ms)), 3),
                      "kernel_ms_all": [round(x, 3) for x in kernel_ms], "abs_sum_dz": check,
                      "status_nonzero": status_nonzero, "launch": h.query(),
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
    res = {"library_sha256": sha, "launches_timed": a.reps, "workloads": {}}
    for name in WORKLOADS:
        runs = {}
        for way in WAYS:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", name, way, "--reps", str(a.reps)]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_SECONDS)
            except subprocess.TimeoutExpired as e:
                sys.stderr.write(str(e.stdout or "")[-2000:] + str(e.stderr or "")[-4000:])
                raise SystemExit("kkt_multi_bench: %s (%s) did not end within %d s; stopping" % (name, way, CHILD_SECONDS))
            if r.returncode != 0:
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                raise SystemExit("kkt_multi_bench: %s (%s) ended with status %d; stopping" % (name, way, r.returncode))
            runs[way] = json.loads(r.stdout.strip().splitlines()[-1])
        ta, xb = runs["tangent_replicated"], runs["x0_sensitivity"]
        spread = max(max(r["call_ms_all"]) - min(r["call_ms_all"]) for r in (ta, xb))
        res["workloads"][name] = {
            "shape": ta["shape"], "batch": ta["batch"], "columns": ta["columns"],
            "a_kernel": ta["kernel"], "a_call_ms": ta["call_ms"], "a_call_ms_all": ta["call_ms_all"],
            "a_kernel_ms": ta["kernel_ms"], "a_launch": ta["launch"],
            "b_kernel": xb["kernel"], "b_call_ms": xb["call_ms"], "b_call_ms_all": xb["call_ms_all"],
            "b_kernel_ms": xb["kernel_ms"], "b_launch": xb["launch"],
            "b_over_a": round(xb["call_ms"] / ta["call_ms"], 4),
            "b_kernel_over_a_kernel": round(xb["kernel_ms"] / ta["kernel_ms"], 4),
            "larger_spread_ms": round(spread, 3), "b_faster": xb["call_ms"] + spread < ta["call_ms"],
            "abs_sum_dz": [ta["abs_sum_dz"], xb["abs_sum_dz"]],
            "status_nonzero": [ta["status_nonzero"], xb["status_nonzero"]], "success": ta["success"]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
