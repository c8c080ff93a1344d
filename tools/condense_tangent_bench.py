#!/usr/bin/env python3
"""The forward mode of the condensed route (fbstab_amd/condense.py: CondensedMpc.Tangent,
fbstab_hip_mpc_condensed_tangent_batch) at (N, nx, nu, nc) = (10, 40, 3, 6), 2048 QPs (tools/fixtures.random_ltv_mpc,
dyn_noise = 0.05, as tools/condense_adjoint_bench.py), device tensors, one GPU, one process.  The points are those of
CondensedMpc.Solve; all 12 sequences are perturbed, every QP in its own random direction.  Every call is warmed once,
then timed --reps times with torch events on torch's current stream, the calls ALTERNATING within a round; median,
min and max in ms:
  condensed_tangent     CondensedMpc.Tangent: the direction kernel, then the adjoint's six launches (and the
                        allocation of the results, as in every call of the package)
  condensed_adjoint     CondensedMpc.Adjoint with all 12 gradients at the same points, random seeds
  mpc_tangent           FBstabMpcBatch.Tangent at the same points and directions (the flat-vector kernels at this shape)
`kernels`: the device time of each kernel inside condensed_tangent, from torch.profiler's kernel records (summed over
its `launches` in a call, median over the reps; null where the profiler gives no kernel records); `direction` is the
direction kernel, and `direction_threads` its workgroup size as its name in the records says.
`tangent_over_adjoint`, `mpc_over_condensed`: ratios of medians of THIS run.  `slower_than_adjoint`: the tangent's
median exceeds the adjoint's by more than the spread (max - min) of the adjoint's reps.
Prints one JSON line (profiles/condense_tangent_bench.json) with the library's sha256.

usage: python tools/condense_tangent_bench.py [--reps 7] [--batch 2048]"""
import argparse
import hashlib
import json
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DIRECTION = "fbstab_mpc_condensed_tangent_rhs_kernel"
KERNELS = dict(direction=DIRECTION, seed="fbstab_mpc_condense_seed_kernel", dense_adjoint="fbstab_dense",
               residual="fbstab_mpc_condensed_adjoint_residual_kernel", correct="fbstab_mpc_condensed_adjoint_correct_kernel",
               finish="fbstab_mpc_condensed_adjoint_finish_kernel")


def stats(ms):
    return dict(median_ms=float(np.median(ms)), min_ms=float(np.min(ms)), max_ms=float(np.max(ms)))


def kernel_split(call, reps):
    """(device time per call of each kernel of ``call``, the direction kernel's thread count), from torch.profiler;
    (None, None) where it records none."""
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
        threads = None
        for e in prof.events():
            us = getattr(e, "device_time_total", None)
            if us is None:
                us = getattr(e, "cuda_time_total", 0.0)
            for k, word in KERNELS.items():
                if word in e.name and us > 0:
                    found[k].append(us / 1000.0)
            nt = re.search(DIRECTION + r"<(\d+)", e.name)
            if nt:
                threads = int(nt.group(1))
        if not all(v and len(v) % reps == 0 for v in found.values()):
            return None, None
        # (the dense adjoint runs twice in a call: the launches of one call are summed)
        return {k: dict(stats(np.asarray(v).reshape(reps, -1).sum(1)), launches=len(v) // reps)
                for k, v in found.items()}, threads
    except Exception as err:  # (a build of torch without the tracer)
        print("condense_tangent_bench: no kernel records (%s)" % err, file=sys.stderr)
        return None, None


def setup(batch):
    """-> dict: the route and the MPC handle at the bench shape, the data, the solved points, directions and seeds."""
    import torch
    from fbstab_amd import hip_api
    from fbstab_amd.condense import CondensedMpc
    from tools import fixtures as fx
    hip_api.load_library()
    rng = np.random.default_rng(2024)
    N, nx, nu, nc = 10, 40, 3, 6
    p = fx.random_ltv_mpc(rng, batch, N, nx, nu, nc, dyn_noise=0.05)
    dev = torch.device("cuda:0")
    data = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in p.arrays.items()}
    cm = CondensedMpc(N, nx, nu, nc, max_batch=batch)
    m = hip_api.FBstabMpcBatch(N, nx, nu, nc, max_batch=batch)
    zeros = lambda n: torch.zeros((batch, n), dtype=torch.float64, device=dev)
    x = [zeros(cm.nz), zeros(cm.nl), zeros(cm.nv), zeros(cm.nv)]
    out = hip_api.out_to_numpy(cm.Solve(data, *x))
    seeds = tuple(torch.from_numpy(rng.standard_normal(t.shape)).to(dev) for t in x[:3])
    d = {k: torch.from_numpy(rng.standard_normal(v.shape)).to(dev) for k, v in p.arrays.items()}
    return dict(shape=[N, nx, nu, nc], cm=cm, m=m, data=data, x=x[:3], out=out, seeds=seeds, d=d)


def timed_rounds(calls, reps):
    """name -> the ms of ``reps`` rounds, the calls alternating within a round; round 0 warms."""
    import torch
    times = {k: [] for k in calls}
    for r in range(reps + 1):
        for k, f in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            if r:
                times[k].append(e0.elapsed_time(e1))
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--batch", type=int, default=2048)
    a = ap.parse_args()
    assert a.reps >= 5
    from fbstab_amd import hip_api
    s = setup(a.batch)
    cm, m, data, (z, l, v), d = s["cm"], s["m"], s["data"], s["x"], s["d"]
    state = {}

    def condensed_tangent():
        state["t"] = cm.Tangent(data, z, l, v, d)

    def condensed_adjoint():
        state["a"] = cm.Adjoint(data, z, l, v, *s["seeds"])

    def mpc_tangent():
        state["m"] = m.Tangent(data, z, l, v, d)

    times = timed_rounds(dict(condensed_tangent=condensed_tangent, condensed_adjoint=condensed_adjoint,
                              mpc_tangent=mpc_tangent), a.reps)
    line = dict(tool="condense_tangent_bench", reps=a.reps, shape=s["shape"], batch=a.batch,
                dense_shape=[cm.nzc, 0, cm.nv],
                library_sha256=hashlib.sha256(open(hip_api.current_library_path(), "rb").read()).hexdigest(),
                lds_bytes=cm.lds_bytes, solve_success=int((s["out"]["eflag"] == 0).sum()),
                condensed_status_ok=int((state["t"]["status"] == 0).sum().item()),
                mpc_status_ok=int((state["m"]["status"] == 0).sum().item()))
    line.update({k: stats(t) for k, t in times.items()})
    # the distance of the two tangents on the QPs both sides solved (the O(sigma) bias and the two roundings)
    import torch
    keep = torch.from_numpy(s["out"]["eflag"] == 0).to(z.device) & (state["t"]["status"] == 0) & (state["m"]["status"] == 0)
    line["median_relative_distance"] = {
        k: float(((state["t"][k][keep] - state["m"][k][keep]).abs().amax(1)
                  / state["m"][k][keep].abs().amax(1).clamp_min(1.0)).median().item()) for k in ("dz", "dl", "dv")}
    state.clear()
    line["kernels"], line["direction_threads"] = kernel_split(lambda: cm.Tangent(data, z, l, v, d), a.reps)
    ta, ad = line["condensed_tangent"], line["condensed_adjoint"]
    line["tangent_over_adjoint"] = ta["median_ms"] / ad["median_ms"]
    line["mpc_over_condensed"] = line["mpc_tangent"]["median_ms"] / ta["median_ms"]
    line["slower_than_adjoint"] = bool(ta["median_ms"] - ad["median_ms"] > ad["max_ms"] - ad["min_ms"])
    cm.close()
    m.close()
    print(json.dumps(line))


if __name__ == "__main__":
    main()
