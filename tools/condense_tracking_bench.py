#!/usr/bin/env python3
"""Closed-loop sweeps of the condensed route that track per-step references (fbstab_amd/condense.py:
CondensedMpc.ReferenceImages, RecedingSweep(ref=...), RecedingSweepAdjoint(ref=...)) against what the package had
before them: one GPU, the problem of tools/condense_sweep_bench.py - (N, nx, nu, nc) = (10, 40, 3, 6), 2048
trajectories of ONE shared model, 50 steps from a zero guess - with references for all four of q, r, c, d that every
trajectory has for itself, (steps, batch, len) each: q and r move by a tenth of their scale, c by 0.001, and d only
loosens the constraints.  Every timed call is warmed once, then timed --reps times with torch events on torch's
current stream; median, min and max in ms.
  images       1. ReferenceImages for refs_per_group in {1, 2, 4, the rule}, against `vectors_launches`: `steps`
                  VECTORS launches of fbstab_hip_mpc_condense_batch with x0 on zeros (what there was before), and
                  whether all of them agree bit for bit
  sweeps       2. tracked_affine (the images included) and tracked_recondense, against python_loop - per step
                  Solve(recondense="vectors") with the step's references swapped in and a torch plant step - and
                  against untracked_affine, the sweep without references (the floor)
  adjoint      3. tracked_adjoint: RecedingSweepAdjoint(ref=...) with all four per-step gradients, against
                  python_backward: loss.backward() through the Python loop of autograd.solve_condensed_mpc (its forward
                  pass is timed apart: python_forward)
Each step below is a child process of its own under `timeout`, one after the other; a step that fails ends the run and
nothing more is started.  Writes profiles/condense_tracking_bench.json (one JSON line, with the library's sha256).

usage: python tools/condense_tracking_bench.py [--reps 7] [--steps 50] [--batch 2048]"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.condense_sweep_bench import SHAPE, _point, _setup, timed  # noqa: E402

STEPS = ("images", "sweeps", "adjoint")
STEP_TIMEOUT_S = dict(images=240, sweeps=420, adjoint=420)
REF = ("q", "r", "c", "d")


def references(d, steps, B):
    """name -> (steps, B, len) device tensors around the data's own (shared) sequences."""
    import torch
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(31)
    ref = {}
    for k in REF:
        a = d[k]
        g = torch.randn((steps, B, a.shape[1]), dtype=torch.float64, device="cuda:0", generator=gen)
        if k in ("q", "r"):
            ref[k] = a[None] + 0.01 * g
        elif k == "c":
            ref[k] = a[None] + 0.001 * g
        else:
            ref[k] = a[None] - 0.02 * g.abs()
    return ref


def step_images(a):
    import torch
    from fbstab_amd.condense import condensed_reference_sizes
    B, steps = a.batch, a.steps
    cm, d, A, Bm, x0 = _setup(B)
    ref = references(d, steps, B)
    rule = condensed_reference_sizes(*SHAPE, steps, 0)
    values = sorted({1, 2, 4, rule["refs_per_group"]})
    res = dict(rule=rule)
    got = {}
    for R in values:
        def run(R=R):
            got[R] = cm.ReferenceImages(d, ref, refs_per_group=R)
        res["R%d" % R] = dict(timed(run, a.reps), sizes=condensed_reference_sizes(*SHAPE, steps, R))
    d0 = dict(d)
    d0["x0"] = torch.zeros((B, SHAPE[1]), dtype=torch.float64, device="cuda:0")
    f0 = torch.empty((steps, B, cm.nzc), dtype=torch.float64, device="cuda:0")
    b0 = torch.empty((steps, B, cm.nv), dtype=torch.float64, device="cuda:0")

    def launches():
        for k in range(steps):
            dk = dict(d0)
            for n in REF:
                dk[n] = ref[n][k]
            img = cm.Condense(dk, "vectors")
            f0[k], b0[k] = img["f"], img["b"]
    res["vectors_launches"] = timed(launches, a.reps)
    torch.cuda.synchronize()
    res["same_bits"] = all(torch.equal(got[R]["f0"], f0) and torch.equal(got[R]["b0"], b0) for R in values)
    best = min(values, key=lambda R: res["R%d" % R]["median_ms"])
    res["best"] = best
    res["rule_over_best"] = res["R%d" % rule["refs_per_group"]]["median_ms"] / res["R%d" % best]["median_ms"]
    res["rule_over_vectors_launches"] = res["R%d" % rule["refs_per_group"]]["median_ms"] / res["vectors_launches"]["median_ms"]
    return res


def step_sweeps(a):
    import torch
    B, steps = a.batch, a.steps
    cm, d, A, Bm, x0 = _setup(B)
    N, nx, nu, nc = SHAPE
    ref = references(d, steps, B)
    state = {}

    def sweep(name, mode, r):
        d["x0"] = x0.clone()
        state[name] = cm.RecedingSweep(d, *_point(cm, B), A, Bm, steps, mode=mode, ref=r)

    def python_loop():
        dk = dict(d)
        dk["x0"] = x0.clone()
        z, l, v, y = _point(cm, B)
        for n in REF:
            dk[n] = ref[n][0]
        cm.Condense(dk)
        us = []
        for k in range(steps):
            for n in REF:
                dk[n] = ref[n][k]
            cm.Solve(dk, z, l, v, y, recondense="vectors")
            u0 = z[:, nx:nx + nu]
            us.append(u0.clone())
            dk["x0"] = dk["x0"] @ A.T + u0 @ Bm.T
        state["loop_u"] = torch.stack(us)

    res = dict(tracked_affine=timed(lambda: sweep("ta", "affine", ref), a.reps),
               tracked_recondense=timed(lambda: sweep("tr", "recondense", ref), a.reps),
               python_loop=timed(python_loop, a.reps),
               untracked_affine=timed(lambda: sweep("ua", "affine", None), a.reps))
    torch.cuda.synchronize()
    ua, ur = state["ta"]["u"], state["tr"]["u"]
    res["retired"] = int((state["ta"]["eflag"][-1] == -1).sum().item())
    res["success_all_steps"] = int((state["ta"]["eflag"] == 0).all(0).sum().item())
    gap = lambda s, t: float(((s - t).abs().max() / (1.0 + t.abs().max())).item())
    ok = (state["tr"]["eflag"] == 0).all(0)   # (the Python loop does not retire: compared where no step failed)
    res["u_gap"] = dict(affine_vs_recondense=gap(ua, ur), python_loop_vs_recondense=gap(state["loop_u"][:, ok], ur[:, ok]),
                        tracked_vs_untracked=gap(ua, state["ua"]["u"]))
    for k in ("tracked_affine", "tracked_recondense"):
        res[k + "_over_python_loop"] = res[k]["median_ms"] / res["python_loop"]["median_ms"]
    res["tracked_affine_over_untracked_affine"] = res["tracked_affine"]["median_ms"] / res["untracked_affine"]["median_ms"]
    return res


def step_adjoint(a):
    import torch
    from fbstab_amd import autograd as ag
    B, steps = a.batch, a.steps
    cm, d, A, Bm, x0 = _setup(B)
    N, nx, nu, nc = SHAPE
    ref = references(d, steps, B)
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(5)
    cu = torch.randn((steps, B, nu), dtype=torch.float64, device="cuda:0", generator=gen)
    cx = torch.randn((steps, B, nx), dtype=torch.float64, device="cuda:0", generator=gen)
    d["x0"] = x0.clone()
    fw = cm.RecedingSweep(d, *_point(cm, B), A, Bm, steps, log=("x", "U", "v"), ref=ref)
    log = {k: fw[k] for k in ("x", "U", "v", "eflag")}
    state = {}

    def tracked():
        state["g"] = cm.RecedingSweepAdjoint(d, A, Bm, steps, log, gu=cu, gx=cx, want=REF, ref=ref)

    def python_forward(grad=False):
        leaves = {n: ref[n].detach().clone().requires_grad_(grad) for n in REF}
        x = x0.clone()
        loss = torch.zeros((), dtype=torch.float64, device="cuda:0")
        for k in range(steps):
            dk = dict(d)
            dk["x0"] = x
            for n in REF:
                dk[n] = leaves[n][k]
            z = ag.solve_condensed_mpc(cm, dk)[0]
            u0 = z[:, nx:nx + nu]
            x = x @ A.T + u0 @ Bm.T
            loss = loss + (cu[k] * u0).sum() + (cx[k] * x).sum()
        return loss, leaves

    def python_backward():
        loss, leaves = python_forward(True)
        loss.backward()
        state["pg"] = {n: leaves[n].grad for n in REF}

    res = dict(tracked_adjoint=timed(tracked, a.reps), python_forward=timed(python_forward, a.reps),
               python_backward=timed(python_backward, a.reps))
    torch.cuda.synchronize()
    res["status_nonzero"] = int((state["g"]["status"] != 0).sum().item())
    # (the loop solves every step from a cold guess and the sweep from a warm one - the same solutions to the tolerance -
    # and it does not retire: compared on the trajectories without a failed step)
    ok = (fw["eflag"] == 0).all(0)
    res["compared_trajectories"] = int(ok.sum().item())
    res["grad_gap_vs_python"] = {n: float(((state["g"][n][:, ok] - state["pg"][n][:, ok]).abs().max() /
                                           (1e-300 + state["pg"][n][:, ok].abs().max())).item()) for n in REF}
    res["tracked_adjoint_over_python_backward"] = res["tracked_adjoint"]["median_ms"] / res["python_backward"]["median_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--step", choices=STEPS, help="(internal) run one step in this process and print its JSON")
    a = ap.parse_args()
    assert a.reps >= 5
    if a.step:
        print("RESULT " + json.dumps(globals()["step_" + a.step](a)))
        return 0
    # the driver: it never opens the GPU itself; each step is a fresh child under a time limit of its own
    from fbstab_amd import hip_api
    line = dict(tool="condense_tracking_bench", shape=list(SHAPE), batch=a.batch, steps=a.steps, reps=a.reps,
                library_sha256=hashlib.sha256(open(hip_api.LIB_PATH, "rb").read()).hexdigest())
    for step in STEPS:
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S[step]), sys.executable, os.path.abspath(__file__), "--step", step,
               "--reps", str(a.reps), "--steps", str(a.steps), "--batch", str(a.batch)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, cwd=ROOT)
        got = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not got:
            print("condense_tracking_bench: step %s ended with status %d; nothing more is started" % (step, r.returncode),
                  file=sys.stderr)
            return r.returncode or 1
        line[step] = json.loads(got[-1][len("RESULT "):])
    text = json.dumps(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "condense_tracking_bench.json"), "w") as f:
        f.write(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
