#!/usr/bin/env python3
"""Backward (fbstab_hip_mpc_adjoint_batch) against forward (solve_batch) kernel time on BASELINE configs[2]:
8192 synthetic QPs of N = 30, nx = 12, nu = 4, nc = 20, device tensors, one GPU.  Both times are the handle's
last_kernel_ms (HIP events around the one launch); the median of --reps launches each.  Prints one JSON line.

usage: python tools/adjoint_bench.py [--batch 8192] [--reps 5] [--generic]
       python tools/adjoint_bench.py --dense [--batch 4096] [--reps 5]
--generic: FBSTAB_HIP_GENERIC=1, forward and adjoint on the flat-vector kernels (default: the record instance
<12,4,20> and its own adjoint).
--dense: fbstab_hip_dense_adjoint_batch against fbstab_hip_dense_solve_batch on BASELINE configs[1] instead: 4096
synthetic dense QPs of nz = 50, nl = 10, nv = 100 (the one-wavefront kernels)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def dense(batch, reps):
    import torch
    from tools import fixtures as fx
    from fbstab_amd import hip_api
    dev = torch.device("cuda:0")
    nz, nl, nv = 50, 10, 100
    p = fx.synthetic_dense_batch(batch, nz, nl, nv)
    data = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in p.arrays.items()}
    s = hip_api.FBstabDenseBatch(nz, nl, nv, max_batch=batch)
    zeros = lambda n: torch.zeros((batch, n), dtype=torch.float64, device=dev)
    fwd, bwd = [], []
    rng = np.random.default_rng(0)
    seeds = [torch.from_numpy(rng.standard_normal((batch, n))).to(dev) for n in (nz, nl, nv)]
    for _ in range(reps + 1):
        z, l, v, y = zeros(nz), zeros(nl), zeros(nv), zeros(nv)
        out = s.Solve(data, z, l, v, y)
        torch.cuda.synchronize()
        fwd.append(s.last_kernel_ms())
        g = s.Adjoint(data, z, l, v, *seeds)
        torch.cuda.synchronize()
        bwd.append(s.last_kernel_ms())
    fwd, bwd = fwd[1:], bwd[1:]   # (the first pair warms the code objects)
    ok = int((hip_api.out_to_numpy(out)["eflag"] == 0).sum())
    f, b = float(np.median(fwd)), float(np.median(bwd))
    wave = s.query()["threads"] == 64
    grad_bytes = 8 * sum(s.arr_len) * batch
    print(json.dumps({"workload": "BASELINE configs[1]", "batch": batch,
                      "forward_kernel": "fbstab_dense_wave_kernel" if wave else "fbstab_dense_kernel<256>",
                      "adjoint_kernel": "fbstab_dense_wave_adjoint_kernel" if wave else "fbstab_dense_adjoint_kernel<256>",
                      "forward_ms": round(f, 3), "backward_ms": round(b, 3), "backward_over_forward": round(b / f, 4),
                      "forward_ms_all": [round(t, 3) for t in fwd], "backward_ms_all": [round(t, 3) for t in bwd],
                      "gradient_bytes": grad_bytes, "success": ok,
                      "adjoint_status_nonzero": int((g["status"] != 0).sum().item())}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--generic", action="store_true")
    ap.add_argument("--dense", action="store_true")
    a = ap.parse_args()
    if a.dense:
        return dense(a.batch or 4096, a.reps)
    a.batch = a.batch or 8192
    if a.generic:
        os.environ["FBSTAB_HIP_GENERIC"] = "1"
    import torch
    from tools import fixtures as fx
    from fbstab_amd import hip_api
    dev = torch.device("cuda:0")
    p = fx.synthetic_mpc_batch(a.batch)
    data = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in p.arrays.items()}
    s = hip_api.FBstabMpcBatch(*p.sizes(), max_batch=a.batch)
    zeros = lambda n: torch.zeros((a.batch, n), dtype=torch.float64, device=dev)
    fwd, bwd = [], []
    rng = np.random.default_rng(0)
    seeds = [torch.from_numpy(rng.standard_normal((a.batch, n))).to(dev) for n in (p.nz, p.nl, p.nv)]
    for _ in range(a.reps + 1):
        z, l, v, y = zeros(p.nz), zeros(p.nl), zeros(p.nv), zeros(p.nv)
        out = s.Solve(data, z, l, v, y)
        torch.cuda.synchronize()
        fwd.append(s.last_kernel_ms())
        g = s.Adjoint(data, z, l, v, *seeds)
        torch.cuda.synchronize()
        bwd.append(s.last_kernel_ms())
    fwd, bwd = fwd[1:], bwd[1:]   # (the first pair warms the code objects and the adjoint's scratch)
    ok = int((hip_api.out_to_numpy(out)["eflag"] == 0).sum())
    f, b = float(np.median(fwd)), float(np.median(bwd))
    kn = s.kernel_name()   # (the one-row record instances run their own adjoint; every other handle the flat-vector one)
    adj_kernel = kn.replace("r16_kernel", "r16_adjoint_kernel") if kn.startswith("fbstab_mpc_r16_kernel<12,4,") \
        else "fbstab_mpc_adjoint_kernel<64>"
    print(json.dumps({"workload": "BASELINE configs[2]", "batch": a.batch, "forward_kernel": s.kernel_name(),
                      "adjoint_kernel": adj_kernel, "forward_ms": round(f, 3),
                      "backward_ms": round(b, 3), "backward_over_forward": round(b / f, 4),
                      "forward_ms_all": [round(t, 3) for t in fwd], "backward_ms_all": [round(t, 3) for t in bwd],
                      "success": ok, "adjoint_status_nonzero": int((g["status"] != 0).sum().item())}))


if __name__ == "__main__":
    main()
