#!/usr/bin/env python3
"""Backward (fbstab_hip_mpc_adjoint_batch) against forward (solve_batch) kernel time on BASELINE configs[2]:
8192 synthetic QPs of N = 30, nx = 12, nu = 4, nc = 20, device tensors, one GPU.  Both times are the handle's
last_kernel_ms (HIP events around the one launch); the median of --reps launches each.  Prints one JSON line.

usage: python tools/adjoint_bench.py [--batch 8192] [--reps 5] [--generic]
       python tools/adjoint_bench.py --dense [--batch 4096] [--reps 5]
       python tools/adjoint_bench.py --wide [--reps 5]
       python tools/adjoint_bench.py --reduced [--reps 5]
       python tools/adjoint_bench.py --tangent [--dense] [--reps 5]
       python tools/adjoint_bench.py --sweep [--batch 4096] [--steps 50] [--reps 5]
--generic: FBSTAB_HIP_GENERIC=1, forward and adjoint on the flat-vector kernels (default: the record instance
<12,4,20> and its own adjoint).
--dense: fbstab_hip_dense_adjoint_batch against fbstab_hip_dense_solve_batch on BASELINE configs[1] instead: 4096
synthetic dense QPs of nz = 50, nl = 10, nv = 100 (the one-wavefront kernels).
--wide: the two workloads of bench.py's `wide` block, built the way bench_wide builds them - the reference's
reactor at N = 80 on <18,5,10> with 1024 QPs, and 2048 QPs of (30, 20, 6, 16) on <24,8,16> - on the row-pair record
instances: the forward solve, the record adjoint (FBSTAB_HIP_FLAT_ADJOINT=0) and the flat-vector adjoint on a handle
of the same shape (FBSTAB_HIP_FLAT_ADJOINT=1), every setting in a fresh process of its own.  One JSON line with both workloads and the
library's sha256.
--reduced: the backward of a layer whose matrices are shared by the batch, on BASELINE configs[2] (8192 QPs, all twelve
sequences wanted) and configs[1] (4096 dense QPs): fbstab_hip_*_adjoint_batch with per-QP slots followed by
torch.sum(dim=0) of every matrix gradient, against ONE fbstab_hip_*_adjoint_batch_reduced call with the matrix slots
reduced.  Times are torch events around the whole backward on torch's current stream (allocation of the outputs
included, as a caller pays it), the median of --reps launches; the two ways alternate, each in a fresh process.  One
JSON line (profiles/reduced_adjoint_bench.json) with the library's sha256; `not_slower` says whether the reduced call
is within the spread of the launches of the per-QP way.
--tangent: the forward mode against the reverse mode it mirrors, on BASELINE configs[2] (8192 QPs) or, with --dense,
configs[1] (4096 dense QPs), each way in a fresh process, the median of --reps launches:
  (a) fbstab_hip_*_adjoint_batch with all per-QP gradient slots wanted: the adjoint kernel's launch
      (last_kernel_ms), and the whole call between torch events (the allocation of the gradients included);
  (b) fbstab_hip_*_tangent_batch with per-QP perturbations of all arrays: the whole call between torch events
      (direction kernel, queue reset and adjoint kernel; the three result vectors are allocated inside);
  (c) the direction kernel alone: (b)'s call minus its adjoint kernel's launch - an upper bound, the queue reset
      and the launch gaps are in it - and the bytes it reads and writes over that time.
`not_slower`: (b) <= (a)'s kernel + the spread of (a)'s launches.  One JSON line (profiles/tangent_bench.json) with
the library's sha256.
--sweep: the closed loop's derivative on BASELINE configs[4]'s shape, 4096 trajectories x 50 steps in one process, the
four calls interleaved launch by launch: the unlogged sweep, the logged sweep (fbstab_hip_mpc_receding_sweep_logged),
the one-launch backward of that log (fbstab_mpc_r16_sweep_adjoint_kernel, all twelve slots wanted and mu_log) and the
per-step backward of the same log (FBSTAB_HIP_SWEEP_ADJOINT_PER_STEP=1).  Wall time of each (synchronous) call, the
median of --reps launches after one that warms the code objects and the handle's buffers.  One JSON line
(profiles/sweep_adjoint_bench.json) with the library's sha256; `one_launch_faster`: the one-launch median is below
the per-step median by more than the larger spread of the two."""
import argparse
import hashlib
import json
import os
import subprocess
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


WIDE = ("reactor_N80", "ltv_30_20_6_16")
CHILD_SECONDS = 300   # one child of --wide: set-up, six solves and six adjoints of one workload


def wide_problem(name):
    """bench.py: bench_wide's workloads."""
    from tools import fixtures as fx
    if name == "ltv_30_20_6_16":
        one = fx.random_ltv_mpc(np.random.default_rng(5), 64, 30, 20, 6, 16)
        p = fx.MpcProblem(30, 20, 6, 16)
        p.arrays = {k: np.ascontiguousarray(np.tile(a, (32, 1))) for k, a in one.arrays.items()}
        return p
    gen = fx.OcpGenerator()
    gen.CopolymerizationReactor(80)
    one = gen.GetFBstabInput()
    N, nx, nu, nc = one.sizes()
    B = 1024
    rng = np.random.default_rng(3)
    p = fx.MpcProblem(N, nx, nu, nc)
    p.arrays = {k: np.ascontiguousarray(np.broadcast_to(a, (B, a.shape[1]))).copy() for k, a in one.arrays.items()}
    p.arrays["x0"] = p.arrays["x0"] * (1.0 + 0.2 * rng.standard_normal((B, nx)))
    return p


def wide_child(name, reps):
    """One workload on one handle of this process (FBSTAB_HIP_FLAT_ADJOINT as the parent set it)."""
    import torch
    from fbstab_amd import hip_api
    dev = torch.device("cuda:0")
    p = wide_problem(name)
    B = p.batch
    data = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in p.arrays.items()}
    s = hip_api.FBstabMpcBatch(*p.sizes(), max_batch=B)
    zeros = lambda n: torch.zeros((B, n), dtype=torch.float64, device=dev)
    rng = np.random.default_rng(0)
    seeds = [torch.from_numpy(rng.standard_normal((B, n))).to(dev) for n in (p.nz, p.nl, p.nv)]
    fwd, bwd = [], []
    free0 = torch.cuda.mem_get_info(dev)[0]
    for _ in range(reps + 1):
        z, l, v, y = zeros(p.nz), zeros(p.nl), zeros(p.nv), zeros(p.nv)
        out = s.Solve(data, z, l, v, y)
        torch.cuda.synchronize()
        fwd.append(s.last_kernel_ms())
        g = s.Adjoint(data, z, l, v, *seeds)
        torch.cuda.synchronize()
        bwd.append(s.last_kernel_ms())
    fwd, bwd = fwd[1:], bwd[1:]   # (the first pair warms the code objects and, with the knob, the adjoint's scratch)
    eflag = hip_api.out_to_numpy(out)["eflag"]
    st = g["status"].cpu().numpy()
    dq = g["q"].cpu().numpy()
    print(json.dumps({"workload": name, "shape": list(p.sizes()), "batch": B, "forward_kernel": s.kernel_name(),
                      "adjoint_kernel": s.adjoint_kernel_name(), "forward_ms": round(float(np.median(fwd)), 3),
                      "adjoint_ms": round(float(np.median(bwd)), 3),
                      "forward_ms_all": [round(t, 3) for t in fwd], "adjoint_ms_all": [round(t, 3) for t in bwd],
                      "success": int((eflag == 0).sum()), "adjoint_status_nonzero": int((st != 0).sum()),
                      "grad_q_abs_sum_of_solved": float(np.abs(dq[eflag == 0]).sum()),
                      "launch": s.query(),
                      "device_bytes_taken_by_the_calls": int(free0 - torch.cuda.mem_get_info(dev)[0])}))


def wide(reps):
    from fbstab_amd import hip_api
    hip_api.load_library()
    with open(hip_api.current_library_path(), "rb") as f:
        sha = hashlib.sha256(f.read()).hexdigest()
    res = {"library_sha256": sha, "launches_timed": reps, "workloads": {}}
    for name in WIDE:
        runs = {}
        for key, knob in (("record", "0"), ("flat", "1")):
            env = dict(os.environ, FBSTAB_HIP_FLAT_ADJOINT=knob)
            # every child under a time limit of its own; after one that failed, faulted or ran out of time no
            # further child is started on the GPU
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--wide-child", name, "--reps", str(reps)],
                                   env=env, capture_output=True, text=True, timeout=CHILD_SECONDS)
            except subprocess.TimeoutExpired as e:
                sys.stderr.write(str(e.stdout or "")[-2000:] + str(e.stderr or "")[-4000:])
                raise SystemExit("adjoint_bench --wide: %s (%s) did not end within %d s; stopping" % (name, key, CHILD_SECONDS))
            if r.returncode != 0:
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                raise SystemExit("adjoint_bench --wide: %s (%s) ended with status %d; stopping" % (name, key, r.returncode))
            runs[key] = json.loads(r.stdout.strip().splitlines()[-1])
        rec, flat = runs["record"], runs["flat"]
        res["workloads"][name] = {
            "shape": rec["shape"], "batch": rec["batch"], "forward_kernel": rec["forward_kernel"],
            "forward_ms": rec["forward_ms"], "forward_ms_all": rec["forward_ms_all"],
            "record_adjoint_kernel": rec["adjoint_kernel"], "record_adjoint_ms": rec["adjoint_ms"],
            "record_adjoint_ms_all": rec["adjoint_ms_all"],
            "flat_adjoint_kernel": flat["adjoint_kernel"], "flat_adjoint_ms": flat["adjoint_ms"],
            "flat_adjoint_ms_all": flat["adjoint_ms_all"],
            "flat_over_record": round(flat["adjoint_ms"] / rec["adjoint_ms"], 3),
            "record_adjoint_over_forward": round(rec["adjoint_ms"] / rec["forward_ms"], 4),
            "success": rec["success"], "adjoint_status_nonzero": [rec["adjoint_status_nonzero"], flat["adjoint_status_nonzero"]],
            "grad_q_abs_sum_of_solved": [rec["grad_q_abs_sum_of_solved"], flat["grad_q_abs_sum_of_solved"]],
            "launch": rec["launch"],
            "device_bytes_taken_by_the_calls": [rec["device_bytes_taken_by_the_calls"], flat["device_bytes_taken_by_the_calls"]]}
    print(json.dumps(res))


REDUCED = {"mpc_30_12_4_20": 8192, "dense_50_10_100": 4096}
REDUCED_WAYS = ("per_qp_then_sum", "reduced")


def reduced_child(name, way, reps):
    """One workload, one way, in this process: solve once, then reps + 1 backward passes (the first warms up)."""
    import torch
    from tools import fixtures as fx
    from fbstab_amd import hip_api
    dev = torch.device("cuda:0")
    B = REDUCED[name]
    if name.startswith("dense"):
        p = fx.synthetic_dense_batch(B, 50, 10, 100)
        s = hip_api.FBstabDenseBatch(50, 10, 100, max_batch=B)
        names = hip_api.DENSE_ARR
    else:
        p = fx.synthetic_mpc_batch(B)
        s = hip_api.FBstabMpcBatch(*p.sizes(), max_batch=B)
        names = hip_api.MPC_SEQ
    matrices = tuple(k for k in names if k.isupper())   # (the matrices are the names in capitals)
    data = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in p.arrays.items()}
    zeros = lambda n: torch.zeros((B, n), dtype=torch.float64, device=dev)
    z, l, v, y = zeros(p.nz), zeros(p.nl), zeros(p.nv), zeros(p.nv)
    out = s.Solve(data, z, l, v, y)
    rng = np.random.default_rng(0)
    seeds = [torch.from_numpy(rng.standard_normal((B, n))).to(dev) for n in (p.nz, p.nl, p.nv)]
    torch.cuda.synchronize()
    ms, kernel_ms = [], []
    for _ in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        if way == "reduced":
            g = s.Adjoint(data, z, l, v, *seeds, reduce=matrices)
            sums = {k: g[k] for k in matrices}
        else:
            g = s.Adjoint(data, z, l, v, *seeds)
            sums = {k: torch.sum(g[k], dim=0, keepdim=True) for k in matrices}
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
        kernel_ms.append(s.last_kernel_ms())
        check = float(sum(t.abs().sum().item() for t in sums.values()))
        del g, sums
    ms, kernel_ms = ms[1:], kernel_ms[1:]
    print(json.dumps({"workload": name, "way": way, "batch": B, "ms": round(float(np.median(ms)), 3),
                      "ms_all": [round(t, 3) for t in ms], "adjoint_kernel_ms": round(float(np.median(kernel_ms)), 3),
                      "matrix_gradient_abs_sum": check,
                      "success": int((hip_api.out_to_numpy(out)["eflag"] == 0).sum())}))


def reduced(reps):
    from fbstab_amd import hip_api
    hip_api.load_library()
    with open(hip_api.current_library_path(), "rb") as f:
        sha = hashlib.sha256(f.read()).hexdigest()
    res = {"library_sha256": sha, "launches_timed": reps, "workloads": {}}
    for name in REDUCED:
        runs = {}
        for way in REDUCED_WAYS:
            # every child under a time limit of its own; after one that failed, faulted or ran out of time no
            # further child is started on the GPU
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--reduced-child", name, way, "--reps",
                                    str(reps)], capture_output=True, text=True, timeout=CHILD_SECONDS)
            except subprocess.TimeoutExpired as e:
                sys.stderr.write(str(e.stdout or "")[-2000:] + str(e.stderr or "")[-4000:])
                raise SystemExit("adjoint_bench --reduced: %s (%s) did not end within %d s; stopping" % (name, way, CHILD_SECONDS))
            if r.returncode != 0:
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                raise SystemExit("adjoint_bench --reduced: %s (%s) ended with status %d; stopping" % (name, way, r.returncode))
            runs[way] = json.loads(r.stdout.strip().splitlines()[-1])
        par, red = runs["per_qp_then_sum"], runs["reduced"]
        spread = max(par["ms_all"]) - min(par["ms_all"])
        res["workloads"][name] = {
            "batch": par["batch"], "per_qp_then_sum_ms": par["ms"], "per_qp_then_sum_ms_all": par["ms_all"],
            "reduced_ms": red["ms"], "reduced_ms_all": red["ms_all"],
            "adjoint_kernel_ms": [par["adjoint_kernel_ms"], red["adjoint_kernel_ms"]],
            "reduced_over_per_qp_then_sum": round(red["ms"] / par["ms"], 4),
            "spread_of_the_per_qp_launches_ms": round(spread, 3), "not_slower": red["ms"] <= par["ms"] + spread,
            "matrix_gradient_abs_sum": [par["matrix_gradient_abs_sum"], red["matrix_gradient_abs_sum"]],
            "success": par["success"]}
    print(json.dumps(res))


TANGENT_WAYS = ("adjoint_all_slots", "tangent_all_slots")


def tangent_child(way, dense_, reps):
    """One way in this process: solve once, then reps + 1 calls (the first warms up)."""
    import torch
    from tools import fixtures as fx
    from fbstab_amd import hip_api
    dev = torch.device("cuda:0")
    if dense_:
        B = 4096
        p = fx.synthetic_dense_batch(B, 50, 10, 100)
        s = hip_api.FBstabDenseBatch(50, 10, 100, max_batch=B)
        lens = s.arr_len
    else:
        B = 8192
        p = fx.synthetic_mpc_batch(B)
        s = hip_api.FBstabMpcBatch(*p.sizes(), max_batch=B)
        lens = s.seq_len
    data = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in p.arrays.items()}
    zeros = lambda n: torch.zeros((B, n), dtype=torch.float64, device=dev)
    z, l, v, y = zeros(p.nz), zeros(p.nl), zeros(p.nv), zeros(p.nv)
    out = s.Solve(data, z, l, v, y)
    gen = torch.Generator(device=dev).manual_seed(0)
    rand = lambda n: torch.randn((B, n), dtype=torch.float64, device=dev, generator=gen)
    seeds = [rand(n) for n in (p.nz, p.nl, p.nv)]
    dirs = {k: rand(a.shape[1]) for k, a in data.items()} if way == "tangent_all_slots" else None
    torch.cuda.synchronize()
    ms, kernel_ms = [], []
    for _ in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        if way == "tangent_all_slots":
            g = s.Tangent(data, z, l, v, dirs)
            check = g["dz"]
        else:
            g = s.Adjoint(data, z, l, v, *seeds, adj=True)
            check = g["dz"]
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
        kernel_ms.append(s.last_kernel_ms())
        status_nonzero = int((g["status"] != 0).sum().item())
        check = float(check.abs().sum().item())
        del g
    ms, kernel_ms = ms[1:], kernel_ms[1:]
    # what the direction kernel moves: every image once, the point, and the seeds it writes
    image_bytes = 8 * sum(lens) * B
    print(json.dumps({"way": way, "batch": B, "call_ms": round(float(np.median(ms)), 3),
                      "call_ms_all": [round(t, 3) for t in ms], "adjoint_kernel_ms": round(float(np.median(kernel_ms)), 3),
                      "adjoint_kernel_ms_all": [round(t, 3) for t in kernel_ms],
                      "adjoint_kernel": s.adjoint_kernel_name() if not dense_ else "dense",
                      "image_bytes_per_qp": 8 * sum(lens), "image_bytes": image_bytes,
                      "vector_bytes": 8 * 2 * (p.nz + p.nl + p.nv) * B, "abs_sum_dz": check,
                      "status_nonzero": status_nonzero,
                      "success": int((hip_api.out_to_numpy(out)["eflag"] == 0).sum())}))


def tangent(dense_, reps):
    from fbstab_amd import hip_api
    hip_api.load_library()
    with open(hip_api.current_library_path(), "rb") as f:
        sha = hashlib.sha256(f.read()).hexdigest()
    runs = {}
    for way in TANGENT_WAYS:
        # every child under a time limit of its own; after one that failed, faulted or ran out of time no further
        # child is started on the GPU
        cmd = [sys.executable, os.path.abspath(__file__), "--tangent-child", way, "--reps", str(reps)]
        try:
            r = subprocess.run(cmd + (["--dense"] if dense_ else []), capture_output=True, text=True, timeout=CHILD_SECONDS)
        except subprocess.TimeoutExpired as e:
            sys.stderr.write(str(e.stdout or "")[-2000:] + str(e.stderr or "")[-4000:])
            raise SystemExit("adjoint_bench --tangent: %s did not end within %d s; stopping" % (way, CHILD_SECONDS))
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            raise SystemExit("adjoint_bench --tangent: %s ended with status %d; stopping" % (way, r.returncode))
        runs[way] = json.loads(r.stdout.strip().splitlines()[-1])
    a, b = runs["adjoint_all_slots"], runs["tangent_all_slots"]
    spread = max(a["adjoint_kernel_ms_all"]) - min(a["adjoint_kernel_ms_all"])
    direction_ms = b["call_ms"] - b["adjoint_kernel_ms"]
    moved = b["image_bytes"] + b["vector_bytes"]
    print(json.dumps({
        "library_sha256": sha, "launches_timed": reps,
        "workload": "BASELINE configs[1]" if dense_ else "BASELINE configs[2]", "batch": a["batch"],
        "adjoint_kernel": a["adjoint_kernel"],
        "a_adjoint_all_slots_kernel_ms": a["adjoint_kernel_ms"], "a_kernel_ms_all": a["adjoint_kernel_ms_all"],
        "a_call_ms": a["call_ms"], "a_call_ms_all": a["call_ms_all"],
        "b_tangent_call_ms": b["call_ms"], "b_call_ms_all": b["call_ms_all"],
        "b_adjoint_kernel_ms": b["adjoint_kernel_ms"],
        "c_direction_ms_upper_bound": round(direction_ms, 3), "c_bytes": moved,
        "c_tb_per_s_lower_bound": round(moved / (direction_ms * 1e-3) / 1e12, 3) if direction_ms > 0 else None,
        "image_bytes_per_qp": b["image_bytes_per_qp"],
        "spread_of_a_ms": round(spread, 3), "b_over_a": round(b["call_ms"] / a["adjoint_kernel_ms"], 4),
        "not_slower": b["call_ms"] <= a["adjoint_kernel_ms"] + spread,
        "status_nonzero": [a["status_nonzero"], b["status_nonzero"]], "abs_sum_dz": [a["abs_sum_dz"], b["abs_sum_dz"]],
        "success": a["success"]}))


def sweep(batch, steps, reps):
    import time
    import torch
    from tools import fixtures as fx
    from fbstab_amd import hip_api
    dev = torch.device("cuda:0")
    with open(hip_api.current_library_path(), "rb") as f:
        sha = hashlib.sha256(f.read()).hexdigest()
    p = fx.synthetic_mpc_batch(batch)
    A, B = fx.quadrotor_model()
    host = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in p.arrays.items()}
    data = {k: t.to(dev) for k, t in host.items()}
    s = hip_api.FBstabMpcBatch(*p.sizes(), max_batch=batch)
    zeros = lambda n: torch.zeros((batch, n), dtype=torch.float64, device=dev)
    rng = np.random.default_rng(0)
    gu = torch.from_numpy(rng.standard_normal((steps, batch, p.nu))).to(dev)
    gx = torch.from_numpy(rng.standard_normal((steps, batch, p.nx))).to(dev)
    t = {"sweep": [], "sweep_logged": [], "adjoint_one_launch": [], "adjoint_per_step": []}
    names, checks = {}, {}

    def timed(key, fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        t[key].append((time.perf_counter() - t0) * 1e3)
        return r

    def forward(log):
        data["x0"].copy_(host["x0"])
        z, l, v, y = zeros(p.nz), zeros(p.nl), zeros(p.nv), zeros(p.nv)
        return timed("sweep_logged" if log else "sweep",
                     lambda: s.RecedingSweep(data, z, l, v, y, A, B, steps, retire=True, log=log))

    for _ in range(reps + 1):
        plain = forward(False)
        r = forward(True)
        for key, env in (("adjoint_one_launch", "0"), ("adjoint_per_step", "1")):
            os.environ["FBSTAB_HIP_SWEEP_ADJOINT_PER_STEP"] = env
            names[key] = s.sweep_adjoint_kernel_name()
            g = timed(key, lambda: s.RecedingSweepAdjoint(data, A, B, steps, r, gu=gu, gx=gx, mu=True))
            checks[key] = [float(g["q"].abs().sum().item()), float(g["x0"].abs().sum().item()),
                           int((g["status"] != 0).sum().item())]
            del g
    os.environ.pop("FBSTAB_HIP_SWEEP_ADJOINT_PER_STEP")
    t = {k: v[1:] for k, v in t.items()}
    med = {k: float(np.median(v)) for k, v in t.items()}
    spread = {k: max(v) - min(v) for k, v in t.items()}
    a, b = "adjoint_one_launch", "adjoint_per_step"
    log_doubles = steps * batch * (p.nz + p.nl + p.nv + p.nx)
    print(json.dumps({
        "library_sha256": sha, "launches_timed": reps, "workload": "BASELINE configs[4] shape", "batch": batch,
        "steps": steps, "forward_kernel": s.kernel_name(), "kernels": names,
        "ms": {k: round(v, 3) for k, v in med.items()}, "ms_all": {k: [round(x, 3) for x in v] for k, v in t.items()},
        "spread_ms": {k: round(v, 3) for k, v in spread.items()},
        "logged_over_unlogged": round(med["sweep_logged"] / med["sweep"], 4),
        "one_launch_over_per_step": round(med[a] / med[b], 4),
        "one_launch_faster": med[a] + max(spread[a], spread[b]) < med[b],
        "log_bytes": 8 * log_doubles, "retired": int(r["stats"]["retired_total"][-1]),
        "success_last_step": int(r["stats"]["success"][-1]), "abs_sum_q_x0_status_nonzero": checks}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--generic", action="store_true")
    ap.add_argument("--dense", action="store_true")
    ap.add_argument("--wide", action="store_true")
    ap.add_argument("--wide-child", choices=WIDE, help=argparse.SUPPRESS)
    ap.add_argument("--reduced", action="store_true")
    ap.add_argument("--reduced-child", nargs=2, help=argparse.SUPPRESS)
    ap.add_argument("--tangent", action="store_true")
    ap.add_argument("--tangent-child", choices=TANGENT_WAYS, help=argparse.SUPPRESS)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--steps", type=int, default=50)
    a = ap.parse_args()
    if a.sweep:
        return sweep(a.batch or 4096, a.steps, a.reps)
    if a.tangent_child:
        return tangent_child(a.tangent_child, a.dense, a.reps)
    if a.tangent:
        return tangent(a.dense, a.reps)
    if a.reduced_child:
        return reduced_child(a.reduced_child[0], a.reduced_child[1], a.reps)
    if a.reduced:
        return reduced(a.reps)
    if a.wide_child:
        return wide_child(a.wide_child, a.reps)
    if a.wide:
        return wide(a.reps)
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
    adj_kernel = s.adjoint_kernel_name()
    print(json.dumps({"workload": "BASELINE configs[2]", "batch": a.batch, "forward_kernel": s.kernel_name(),
                      "adjoint_kernel": adj_kernel, "forward_ms": round(f, 3),
                      "backward_ms": round(b, 3), "backward_over_forward": round(b / f, 4),
                      "forward_ms_all": [round(t, 3) for t in fwd], "backward_ms_all": [round(t, 3) for t in bwd],
                      "success": ok, "adjoint_status_nonzero": int((g["status"] != 0).sum().item())}))


if __name__ == "__main__":
    main()
