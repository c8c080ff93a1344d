#!/usr/bin/env python3
"""What the scenario options of the receding-horizon sweep cost and save (fbstab_hip_mpc_receding_sweep_scenario):
BASELINE configs[4] - 4096 trajectories x 200 steps of the quadrotor loop, retirement on - in ONE process, the four
runs interleaved launch by launch, one warm-up round, then the median of ``--reps`` (5) rounds:

  a  the plain sweep (no scenario)
  b  shift = 1, no disturbance
  c  w = position noise of sd 1e-2 on states 0..2, shift = 0
  d  the same w, shift = 1

Per run: the wall time of the (synchronous) call, the per-step ``newton_sum`` and the final ``retired_total``.  With
``--parent-lib PATH`` (another build of the library, e.g. the parent commit's) the plain sweep is also timed on that
build, interleaved in the same rounds, as run ``p``: the plain sweep may be slower than the parent only within the
spread of the parent's own repetitions.  Prints one JSON line carrying the sha256 of the library (and of the parent
build): profiles/sweep_scenario_bench.json.

usage: python tools/sweep_scenario_bench.py [--batch 4096] [--steps 200] [--reps 5] [--parent-lib PATH]"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _sha(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    a = ap.parse_args()
    import torch
    from tools import fixtures as fx
    from fbstab_amd import hip_api
    dev = torch.device("cuda:0")
    batch, steps = a.batch, a.steps
    p = fx.synthetic_mpc_batch(batch)
    A, B = fx.quadrotor_model()
    host = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in p.arrays.items()}
    data = {k: t.to(dev) for k, t in host.items()}
    w = np.zeros((steps, batch, p.nx))
    w[:, :, 0:3] = 1e-2 * np.random.default_rng(5).standard_normal((steps, batch, 3))
    w = torch.from_numpy(w).to(dev)
    solvers = {"head": hip_api.FBstabMpcBatch(*p.sizes(), max_batch=batch)}
    if a.parent_lib:
        with hip_api.library(a.parent_lib):
            solvers["parent"] = hip_api.FBstabMpcBatch(*p.sizes(), max_batch=batch)
    runs = {"a": ("head", {}), "b": ("head", dict(shift=True)), "c": ("head", dict(w=w)),
            "d": ("head", dict(w=w, shift=True))}
    if a.parent_lib:
        runs["p"] = ("parent", {})
    zeros = lambda n: torch.zeros((batch, n), dtype=torch.float64, device=dev)
    ms = {k: [] for k in runs}
    last = {}
    for _ in range(a.reps + 1):
        for key, (which, kw) in runs.items():
            data["x0"].copy_(host["x0"])
            z, l, v, y = zeros(p.nz), zeros(p.nl), zeros(p.nv), zeros(p.nv)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = solvers[which].RecedingSweep(data, z, l, v, y, A, B, steps, retire=True, **kw)
            torch.cuda.synchronize()
            ms[key].append((time.perf_counter() - t0) * 1e3)
            last[key] = r["stats"]
    ms = {k: v[1:] for k, v in ms.items()}
    med = {k: float(np.median(v)) for k, v in ms.items()}
    spread = {k: max(v) - min(v) for k, v in ms.items()}
    line = {
        "library_sha256": _sha(hip_api.current_library_path()), "workload": "BASELINE configs[4]", "batch": batch,
        "steps": steps, "launches_timed": a.reps, "kernel": solvers["head"].kernel_name(),
        "runs": {"a": "plain", "b": "shift", "c": "w", "d": "w + shift", "p": "plain, parent build"},
        "ms": {k: round(v, 3) for k, v in med.items()},
        "ms_all": {k: [round(x, 3) for x in v] for k, v in ms.items()},
        "spread_ms": {k: round(v, 3) for k, v in spread.items()},
        "qp_per_s": {k: round(batch * steps / (v * 1e-3)) for k, v in med.items()},
        "newton_total": {k: int(s["newton_sum"].sum()) for k, s in last.items()},
        "newton_sum_per_step": {k: s["newton_sum"].tolist() for k, s in last.items()},
        "retired_total": {k: int(s["retired_total"][-1]) for k, s in last.items()},
        "d_over_c": round(med["d"] / med["c"], 4), "b_over_a": round(med["b"] / med["a"], 4),
        "c_over_a": round(med["c"] / med["a"], 4)}
    if a.parent_lib:
        line["parent_library_sha256"] = _sha(a.parent_lib)
        line["a_over_parent"] = round(med["a"] / med["p"], 4)
        line["a_within_parent_spread"] = bool(med["a"] <= med["p"] + spread["p"])
    print(json.dumps(line))
    for s in solvers.values():
        s.close()


if __name__ == "__main__":
    main()
