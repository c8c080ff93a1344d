#!/usr/bin/env python3
"""The x0 sensitivity of the condensed route (fbstab_amd/condense.py: CondensedMpc.X0Sensitivity,
fbstab_hip_mpc_condensed_x0_sensitivity_batch) against what the package had before it, device tensors, one GPU, one
process.  Shapes: (N, nx, nu, nc) = (10, 40, 3, 6), the headline shape of the condensed route, with 2048 and 256 QPs,
and (15, 12, 4, 20), a record shape where the route is expected to lose, with 2048 (tools/fixtures.random_ltv_mpc,
dyn_noise = 0.05, as tools/condense_bench.py).  The points are those of CondensedMpc.Solve.  Every call is warmed once,
then timed --reps times with torch events on torch's current stream, the calls ALTERNATING within a round; median, min
and max in ms:
  x0_full        (a) CondensedMpc.X0Sensitivity with dz, dl, dv and gain (and the allocation of the outputs and of the
                 work array, as in every derivative call of the package)
  x0_gain        (a) ... with gain alone: no finish launch, no step buffers
  mpc_x0         (b) FBstabMpcBatch.X0Sensitivity at the same points, dz, dl, dv and gain: what a user had before
  adjoint_nx     (c) ONE CondensedMpc.Adjoint(adj=True, want=()) call on `comparator_points` of the points replicated
                 nx-fold with the unit seeds of x0 (batch = comparator_points x nx): the comparator of the two earlier
                 multi-solve benches.  comparator_points is min(batch, --comparator-points): replicating the DATA of
                 2048 QPs 40-fold is 24 GB; the ratios below are per point.
`kernels`: the device time of each kernel inside x0_full, from torch.profiler's kernel records (summed over its
launches in a call, median over the reps; null where the profiler gives no kernel records).
`r_sweep` (first shape and batch only): x0_full with rhs_per_group in {1, 2, 4, the rule's value}.
Ratios: `mpc_over_full` = (b) / (a), `adjoint_nx_over_full` = (c) per point / (a) per point; above 1 the new call wins.
Prints one JSON line (profiles/condense_multi_bench.json) with the library's sha256.

usage: python tools/condense_multi_bench.py [--reps 7] [--comparator-points 256]"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KERNELS = dict(seed="fbstab_mpc_condense_multi_seed_kernel", dense_multi_solve="fbstab_dense",
               residual="fbstab_mpc_condense_multi_residual_kernel", correct="fbstab_mpc_condense_multi_correct_kernel",
               finish="fbstab_mpc_condense_multi_finish_kernel")
CASES = (((10, 40, 3, 6), 2048), ((10, 40, 3, 6), 256), ((15, 12, 4, 20), 2048))
ALL = ("dz", "dl", "dv", "gain")


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
        # (the dense multi-solve runs twice in a call: the launches of one call are summed)
        return {k: dict(stats(np.asarray(v).reshape(reps, -1).sum(1)), launches=len(v) // reps) for k, v in found.items()}
    except Exception as err:  # (a build of torch without the tracer)
        print("condense_multi_bench: no kernel records (%s)" % err, file=sys.stderr)
        return None


def timed(calls, reps):
    import torch
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
    return {k: stats(v) for k, v in times.items()}


def one_case(shape, B, reps, points, sweep):
    import torch
    from fbstab_amd import hip_api
    from fbstab_amd.condense import CondensedMpc, condensed_multi_sizes
    from tools import fixtures as fx
    N, nx, nu, nc = shape
    rng = np.random.default_rng(2024)
    p = fx.random_ltv_mpc(rng, B, N, nx, nu, nc, dyn_noise=0.05)
    dev = torch.device("cuda:0")
    data = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in p.arrays.items()}
    cm = CondensedMpc(N, nx, nu, nc, max_batch=B)
    m = hip_api.FBstabMpcBatch(N, nx, nu, nc, max_batch=B)
    zeros = lambda n: torch.zeros((B, n), dtype=torch.float64, device=dev)
    x = [zeros(cm.nz), zeros(cm.nl), zeros(cm.nv), zeros(cm.nv)]
    out = hip_api.out_to_numpy(cm.Solve(data, *x))
    z, l, v = x[:3]
    # (c): the first Bc points, each nx times, with the unit seeds of x0 (gz = 0, gl = -e_j in the l_0 block)
    Bc = min(B, points)
    rep = lambda t: t[:Bc].repeat_interleave(nx, dim=0).contiguous()
    cdata = {k: rep(t) for k, t in data.items()}
    cz, cl, cv = rep(z), rep(l), rep(v)
    cgz = torch.zeros_like(cz)
    cgl = torch.zeros_like(cl)
    cgl.view(Bc, nx, -1)[:, torch.arange(nx), torch.arange(nx)] = -1.0
    cc = CondensedMpc(N, nx, nu, nc, max_batch=Bc * nx)
    cc.Condense(cdata)
    state = {}

    def x0_full():
        state["a"] = cm.X0Sensitivity(data, z, l, v, want=ALL)

    def x0_gain():
        state["g"] = cm.X0Sensitivity(data, z, l, v, want=("gain",))

    def mpc_x0():
        state["b"] = m.X0Sensitivity(data, z, l, v, want=ALL)

    def adjoint_nx():
        state["c"] = cc.Adjoint(cdata, cz, cl, cv, cgz, cgl, None, want=(), adj=True)

    res = dict(shape=list(shape), batch=B, comparator_points=Bc, comparator_batch=Bc * nx,
               solve_success=int((out["eflag"] == 0).sum()),
               sizes=condensed_multi_sizes(N, nx, nu, nc, nx), mpc_kernel=m.adjoint_kernel_name())
    res.update(timed(dict(x0_full=x0_full, x0_gain=x0_gain, mpc_x0=mpc_x0, adjoint_nx=adjoint_nx), reps))
    a, b, c = state["a"], state["b"], state["c"]
    res["status_ok"] = dict(x0_full=int((a["status"] == 0).sum().item()), mpc_x0=int((b["status"] == 0).sum().item()),
                            adjoint_nx=int((c["status"] == 0).sum().item()))
    # what the three computed, on the QPs all solved: the median over QPs of the largest distance relative to max|dz|
    keep = torch.from_numpy(out["eflag"] == 0).to(dev) & (a["status"] == 0) & (b["status"] == 0)
    rel = lambda s, t: float(((s - t).abs().amax((1, 2)) / t.abs().amax((1, 2)).clamp_min(1.0)).median().item())
    res["median_relative_distance"] = dict(
        dz_full_vs_mpc=rel(a["dz"][keep], b["dz"][keep]),
        gain_full_vs_mpc=rel(a["gain"][keep].contiguous(), b["gain"][keep].contiguous()),
        dz_full_vs_adjoint_nx=rel(a["dz"][:Bc], c["dz"].view(Bc, nx, -1)))
    res["gain_alone_equals_gain_bitwise"] = bool(torch.equal(state["g"]["gain"], a["gain"]))
    res["mpc_over_full"] = res["mpc_x0"]["median_ms"] / res["x0_full"]["median_ms"]
    res["mpc_over_gain"] = res["mpc_x0"]["median_ms"] / res["x0_gain"]["median_ms"]
    res["adjoint_nx_over_full"] = (res["adjoint_nx"]["median_ms"] / Bc) / (res["x0_full"]["median_ms"] / B)
    res["adjoint_nx_over_gain"] = (res["adjoint_nx"]["median_ms"] / Bc) / (res["x0_gain"]["median_ms"] / B)
    state.clear()
    res["kernels"] = kernel_split(lambda: cm.X0Sensitivity(data, z, l, v, want=ALL), reps)
    if sweep:
        rule = res["sizes"]["rhs_per_group"]
        values = sorted({1, 2, 4, rule})
        calls = {("R%d" % R): (lambda R=R: cm.X0Sensitivity(data, z, l, v, want=ALL, rhs_per_group=R)) for R in values}
        res["r_sweep"] = dict(rule=rule, **timed(calls, reps))
        ref = cm.X0Sensitivity(data, z, l, v, want=ALL)
        res["r_sweep"]["same_bits"] = all(
            torch.equal(cm.X0Sensitivity(data, z, l, v, want=ALL, rhs_per_group=R)[k], ref[k]) for R in values for k in ALL)
    cc.close()
    cm.close()
    m.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--comparator-points", type=int, default=256)
    a = ap.parse_args()
    assert a.reps >= 5
    from fbstab_amd import hip_api
    hip_api.load_library()
    line = dict(tool="condense_multi_bench", reps=a.reps,
                library_sha256=hashlib.sha256(open(hip_api.current_library_path(), "rb").read()).hexdigest(),
                cases=[one_case(shape, B, a.reps, a.comparator_points, i == 0) for i, (shape, B) in enumerate(CASES)])
    print(json.dumps(line))


if __name__ == "__main__":
    main()
