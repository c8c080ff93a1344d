#!/usr/bin/env python3
"""The adjoint of the condensed route (fbstab_amd/condense.py: CondensedMpc.Adjoint, fbstab_hip_mpc_condensed_adjoint_batch)
at (N, nx, nu, nc) = (10, 40, 3, 6), 2048 QPs (tools/fixtures.random_ltv_mpc, dyn_noise = 0.05, as
tools/condense_bench.py), device tensors, one GPU, one process.  The points are those of CondensedMpc.Solve, the seeds
random, all 12 gradients asked for.  Every call is warmed once, then timed --reps times with torch events on torch's
current stream, the calls ALTERNATING within a round; median, min and max in ms:
  condensed_adjoint     CondensedMpc.Adjoint: the seed kernel, the dense adjoint, its refinement step (the residual
                        kernel, the dense adjoint again, the correction kernel), the finish kernel (and the
                        allocation of the gradients, as in every Adjoint of the package)
  dense_adjoint_call    FBstabDenseBatch.Adjoint alone on the condensed QP at (U, v), no gradients, adj = (dU, dv)
  condensed_solve       CondensedMpc.Solve from a cold start, recondense="all"
  mpc_adjoint           FBstabMpcBatch.Adjoint at the same points and seeds (the flat-vector adjoint at this shape)
`kernels`: the device time of each kernel inside condensed_adjoint, from torch.profiler's kernel records (summed over
its `launches` in a call, median over the reps; null where the profiler gives no kernel records) - the split of the
call into seed, dense adjoint (both launches), residual, correction and finish.  `mpc_over_condensed`: the ratio of the two adjoints' medians.
Prints one JSON line (profiles/condense_adjoint_bench.json) with the library's sha256.

usage: python tools/condense_adjoint_bench.py [--reps 7] [--batch 2048]"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KERNELS = dict(seed="fbstab_mpc_condense_seed_kernel", dense_adjoint="fbstab_dense",
               residual="fbstab_mpc_condensed_adjoint_residual_kernel", correct="fbstab_mpc_condensed_adjoint_correct_kernel",
               finish="fbstab_mpc_condensed_adjoint_finish_kernel")


def stats(ms):
    return dict(median_ms=float(np.median(ms)), min_ms=float(np.min(ms)), max_ms=float(np.max(ms)))


def kernel_split(call, reps):
    """Device time per call of each kernel of ``call``, from torch.profiler; None where it records none."""
    import torch
    try:
        from torch.profiler import ProfilerActivity, profile
        call()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(reps):
                call()
            torch.cuda.synchronize()
        found = {k: [] for k in KERNELS}
        for e in prof.events():
            us = getattr(e, "device_time_total", None)
            if us is None:
                us = getattr(e, "cuda_time_total", 0.0)
            for k, word in KERNELS.items():
                if word in e.name and us > 0:
                    found[k].append(us / 1000.0)
        if not all(v and len(v) % reps == 0 for v in found.values()):
            return None
        # (the dense adjoint runs twice in a call: the launches of one call are summed)
        return {k: dict(stats(np.asarray(v).reshape(reps, -1).sum(1)), launches=len(v) // reps) for k, v in found.items()}
    except Exception as err:  # (a build of torch without the tracer)
        print("condense_adjoint_bench: no kernel records (%s)" % err, file=sys.stderr)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--batch", type=int, default=2048)
    a = ap.parse_args()
    assert a.reps >= 5
    import torch
    from fbstab_amd import hip_api
    from fbstab_amd.condense import CondensedMpc
    from tools import fixtures as fx
    hip_api.load_library()
    rng = np.random.default_rng(2024)
    N, nx, nu, nc = 10, 40, 3, 6
    B = a.batch
    p = fx.random_ltv_mpc(rng, B, N, nx, nu, nc, dyn_noise=0.05)
    dev = torch.device("cuda:0")
    data = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in p.arrays.items()}
    cm = CondensedMpc(N, nx, nu, nc, max_batch=B)
    m = hip_api.FBstabMpcBatch(N, nx, nu, nc, max_batch=B)
    zeros = lambda n: torch.zeros((B, n), dtype=torch.float64, device=dev)
    x = [zeros(cm.nz), zeros(cm.nl), zeros(cm.nv), zeros(cm.nv)]
    out = hip_api.out_to_numpy(cm.Solve(data, *x))
    z, l, v = x[:3]
    gz, gl, gv = (torch.from_numpy(rng.standard_normal(t.shape)).to(dev) for t in (z, l, v))
    U = z.view(B, N + 1, nx + nu)[:, :, nx:].reshape(B, cm.nzc).contiguous()
    l0 = torch.zeros((B, 0), dtype=torch.float64, device=dev)
    gU, gvc = (torch.from_numpy(rng.standard_normal(t.shape)).to(dev) for t in (U, v))
    state = {}

    def condensed_adjoint():
        state["c"] = cm.Adjoint(data, z, l, v, gz, gl, gv)

    def dense_adjoint_call():
        img = cm._img
        cm.dense.Adjoint(dict(H=img["H"], f=img["f"], G=l0, h=l0, A=img["A"], b=img["b"]), U, l0, v, gU, None, gvc,
                         want=(), adj=True, async_=True)

    def condensed_solve():
        cm.Solve(data, zeros(cm.nz), zeros(cm.nl), zeros(cm.nv), zeros(cm.nv), recondense="all")

    def mpc_adjoint():
        state["m"] = m.Adjoint(data, z, l, v, gz, gl, gv)

    calls = dict(condensed_adjoint=condensed_adjoint, dense_adjoint_call=dense_adjoint_call,
                 condensed_solve=condensed_solve, mpc_adjoint=mpc_adjoint)
    times = {k: [] for k in calls}
    for r in range(a.reps + 1):   # (round 0 warms)
        for k, f in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            if r:
                times[k].append(e0.elapsed_time(e1))
    line = dict(tool="condense_adjoint_bench", reps=a.reps, shape=[N, nx, nu, nc], batch=B, dense_shape=[cm.nzc, 0, cm.nv],
                library_sha256=hashlib.sha256(open(hip_api.current_library_path(), "rb").read()).hexdigest(),
                lds_bytes=cm.lds_bytes, mpc_adjoint_kernel=m.adjoint_kernel_name(),
                solve_success=int((out["eflag"] == 0).sum()),
                condensed_status_ok=int((state["c"]["status"] == 0).sum().item()),
                mpc_status_ok=int((state["m"]["status"] == 0).sum().item()))
    line.update({k: stats(v) for k, v in times.items()})
    # the distance of the two adjoints' gradients on the QPs both sides solved (the O(sigma) bias and the two
    # roundings; cond(V) decides its size)
    keep = torch.from_numpy(out["eflag"] == 0).to(dev) & (state["c"]["status"] == 0) & (state["m"]["status"] == 0)
    rel = {}
    for k in ("q", "r", "x0", "d"):
        cg, mg = state["c"][k][keep], state["m"][k][keep]
        rel[k] = float(((cg - mg).abs().amax(1) / mg.abs().amax(1).clamp_min(1.0)).median().item())
    line["median_relative_distance"] = rel
    state.clear()
    cm.Condense(data)
    line["kernels"] = kernel_split(lambda: cm.Adjoint(data, z, l, v, gz, gl, gv), a.reps)
    line["mpc_over_condensed"] = line["mpc_adjoint"]["median_ms"] / line["condensed_adjoint"]["median_ms"]
    line["adjoint_over_solve"] = line["condensed_adjoint"]["median_ms"] / line["condensed_solve"]["median_ms"]
    cm.close()
    m.close()
    print(json.dumps(line))


if __name__ == "__main__":
    main()
