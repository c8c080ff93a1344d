#!/usr/bin/env python3
"""Forward mode through the closed-loop sweep of the condensed route (fbstab_amd/condense.py:
CondensedMpc.RecedingSweepTangent, fbstab_hip_mpc_condensed_receding_sweep_tangent) beside its neighbours: the set-up
of tools/condense_sweep_bench.py - one GPU, (N, nx, nu, nc) = (10, 40, 3, 6), 2048 trajectories of ONE time-invariant
model shared by the batch, 50 steps from a zero guess, retirement on - and one random direction of x0 and of the
disturbances.  Every timed call is warmed once, then timed --reps times with torch events on torch's current stream;
median, min and max in ms of WHOLE calls (with the condensing, the map call and every allocation of the call), all in
ONE process:
  tangent_dx0_dw   (a) RecedingSweepTangent(dx0, dw)
  adjoint_x0_mu    (b) RecedingSweepAdjoint(want=(), mu=True): dL/dx0 and the costates alone - the same launch structure
  forward_logged   (c) RecedingSweep(mode="affine", log=("x", "U", "v"))
  loop_forward_ad  (d) today's way: torch.autograd.forward_ad through a Python loop of autograd.solve_condensed_mpc and a
                   torch plant step, the same direction (primal and tangent in one pass)
(d) runs at --loop-steps steps (default: all of them); where that is fewer than --steps its figure is SCALED linearly and
labelled so.  No ratio is a pass criterion: the four times and (a)/(b), (a)/(d) are written down as they come.  The
measuring process is a child under `timeout`; the driver never opens the GPU itself.  Writes
profiles/condense_sweep_tangent_bench.json (one JSON line, with the library's sha256).

usage: python tools/condense_sweep_tangent_bench.py [--reps 7] [--steps 50] [--batch 2048] [--loop-steps 50]"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.condense_sweep_bench import SHAPE, _point, _setup, stats, timed  # noqa: E402

TIMEOUT_S = 540


def measure(a):
    import torch
    import torch.autograd.forward_ad as fwAD
    from fbstab_amd import autograd as ag
    N, nx, nu, nc = SHAPE
    B, steps = a.batch, a.steps
    cm, d, A, Bm, x0 = _setup(B)
    rng = np.random.default_rng(7)
    to = lambda arr: torch.from_numpy(arr).to("cuda:0")
    cu, cx = to(rng.standard_normal((steps, B, nu))), to(rng.standard_normal((steps, B, nx)))
    dx0, dw = to(rng.standard_normal((B, nx))), to(rng.standard_normal((steps, B, nx)))
    state = {}

    def forward():
        d["x0"] = x0.clone()
        state["fwd"] = cm.RecedingSweep(d, *_point(cm, B), A, Bm, steps, log=("x", "U", "v"))

    res = dict(forward_logged=timed(forward, a.reps))
    log = {k: state["fwd"][k] for k in ("x", "U", "v", "eflag")}

    def tangent():
        state["t"] = cm.RecedingSweepTangent(d, A, Bm, steps, log, dx0=dx0, dw=dw)

    def adjoint():
        state["b"] = cm.RecedingSweepAdjoint(d, A, Bm, steps, log, gu=cu, gx=cx, mu=True, want=())

    res["tangent_dx0_dw"] = timed(tangent, a.reps)
    res["adjoint_x0_mu"] = timed(adjoint, a.reps)
    torch.cuda.synchronize()
    fwd, t, b = state["fwd"], state["t"], state["b"]
    res["retired"] = int((fwd["eflag"][-1] == -1).sum().item())
    res["status_nonzero"] = int((t["status"] != 0).sum().item())
    # duality of (a) and (b) on the same log, relative to the sum of the magnitudes of the terms
    mu = torch.where((fwd["eflag"] == -1)[:, :, None], torch.zeros_like(b["mu"]), b["mu"])
    lhs = (cu * t["du"]).sum() + (cx * t["dx"]).sum()
    rhs = (b["x0"] * dx0).sum() + (mu * dw).sum()
    mag = (cu * t["du"]).abs().sum() + (cx * t["dx"]).abs().sum() + (b["x0"] * dx0).abs().sum() + (mu * dw).abs().sum()
    res["duality_gap"] = float(((lhs - rhs).abs() / mag).item())
    res["tangent_loss"] = float(lhs.item())
    per_traj = (cu * t["du"]).sum(dim=(0, 2)) + (cx * t["dx"]).sum(dim=(0, 2))
    alive = fwd["eflag"][-1] != -1
    # (d): forward_ad through the Python loop, the same direction; the loop does not retire
    ls = a.loop_steps
    ms = []
    for r in range(a.reps + 1):   # (round 0 warms)
        e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        e[0].record()
        with fwAD.dual_level():
            xk = fwAD.make_dual(x0.clone(), dx0)
            loss = torch.zeros(B, dtype=torch.float64, device="cuda:0")
            for k in range(ls):
                data = dict(d)
                data["x0"] = xk
                z, l, v, out = ag.solve_condensed_mpc(cm, data)
                u0 = z[:, nx:nx + nu]
                xk = xk @ A.T + u0 @ Bm.T + fwAD.make_dual(torch.zeros_like(dw[k]), dw[k])
                loss = loss + (cu[k] * u0).sum(dim=1) + (cx[k] * xk).sum(dim=1)
            dl = fwAD.unpack_dual(loss).tangent
        e[1].record()
        e[1].synchronize()
        if r:
            ms.append(e[0].elapsed_time(e[1]))
        state["loop_loss"], state["loop_per_traj"] = float(dl.sum().item()), dl.detach().clone()
    scale = steps / ls
    res["loop_forward_ad"] = stats(ms)
    res["loop_label"] = "measured at %d steps" % ls + ("" if scale == 1 else ", SCALED linearly to %d" % steps)
    res["loop_forward_ad_scaled_ms"] = res["loop_forward_ad"]["median_ms"] * scale
    res["loop_tangent_loss"] = state["loop_loss"]
    if scale == 1:   # the loop does not retire: the two differentiate the same loop on the trajectories that stay
        res["tangent_loss_unretired"] = float(per_traj[alive].sum().item())
        res["loop_tangent_loss_unretired"] = float(state["loop_per_traj"][alive].sum().item())
        res["loop_vs_sweep_gap_unretired"] = float(((per_traj - state["loop_per_traj"])[alive].abs().max()
                                                    / per_traj[alive].abs().max()).item())
    ta = res["tangent_dx0_dw"]["median_ms"]
    res["tangent_over_adjoint_x0_mu"] = ta / res["adjoint_x0_mu"]["median_ms"]
    res["tangent_over_forward"] = ta / res["forward_logged"]["median_ms"]
    res["tangent_over_loop_forward_ad"] = ta / res["loop_forward_ad_scaled_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--loop-steps", type=int, default=0, help="steps of the Python loop (0: --steps)")
    ap.add_argument("--measure", action="store_true", help="(internal) measure in this process and print the JSON")
    a = ap.parse_args()
    assert a.reps >= 5
    a.loop_steps = a.loop_steps or a.steps
    if a.measure:
        print("RESULT " + json.dumps(measure(a)))
        return 0
    from fbstab_amd import hip_api
    line = dict(tool="condense_sweep_tangent_bench", shape=list(SHAPE), batch=a.batch, steps=a.steps, reps=a.reps,
                library_sha256=hashlib.sha256(open(hip_api.LIB_PATH, "rb").read()).hexdigest())
    cmd = ["timeout", "-k", "10", str(TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--measure",
           "--reps", str(a.reps), "--steps", str(a.steps), "--batch", str(a.batch), "--loop-steps", str(a.loop_steps)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, cwd=ROOT)
    got = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    if r.returncode != 0 or not got:
        print("condense_sweep_tangent_bench: the measuring process ended with status %d" % r.returncode, file=sys.stderr)
        return r.returncode or 1
    line.update(json.loads(got[-1][len("RESULT "):]))
    text = json.dumps(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "condense_sweep_tangent_bench.json"), "w") as f:
        f.write(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
