#!/usr/bin/env python3
"""The adjoint through the closed-loop sweep of the condensed route (fbstab_amd/condense.py:
CondensedMpc.RecedingSweepAdjoint, fbstab_hip_mpc_condensed_receding_sweep_adjoint) against what the package had before
it: the set-up of tools/condense_sweep_bench.py - one GPU, (N, nx, nu, nc) = (10, 40, 3, 6), 2048 trajectories of ONE
time-invariant model shared by the batch, 50 steps from a zero guess, retirement on - and a random linear loss
L = <cu, u> + <cx, x>.  Every timed call is warmed once, then timed --reps times with torch events on torch's current
stream; median, min and max in ms of WHOLE calls (with the condensing, the map call and every allocation of the call):
  forward_logged   (a) RecedingSweep(mode="affine", log=("x", "U", "v"))
  adjoint_x0_mu    (b) RecedingSweepAdjoint(want=(), mu=True): dL/dx0 and the costates alone (no finish kernel)
  adjoint_all      (c) RecedingSweepAdjoint(want = the 11 other sequences, mu=True), mode="affine"
  adjoint_all_recondense  (f) the same in mode="recondense"
  loop_backward    (d) today's way: loss.backward() through a Python loop of autograd.solve_condensed_mpc and a torch
                   plant step, every one of the 12 sequences requiring a gradient
  loop_forward     (e) the forward pass of (d)
(d) and (e) run at --loop-steps steps (default: all of them); where that is fewer than --steps the figures are SCALED
linearly and labelled so.  `condition`: (c) is not slower than (d) by more than the spread (max - min) of (d)'s runs.
Each step below is a child process of its own under `timeout`, one after the other; a step that fails ends the run and
nothing more is started.  Writes profiles/condense_sweep_adjoint_bench.json (one JSON line, with the library's sha256).

usage: python tools/condense_sweep_adjoint_bench.py [--reps 7] [--steps 50] [--batch 2048] [--loop-steps 50]"""
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

STEPS = ("sweep", "loop")
STEP_TIMEOUT_S = dict(sweep=420, loop=480)


def _loss_seeds(B, steps):
    import torch
    N, nx, nu, nc = SHAPE
    rng = np.random.default_rng(7)
    to = lambda a: torch.from_numpy(a).to("cuda:0")
    return to(rng.standard_normal((steps, B, nu))), to(rng.standard_normal((steps, B, nx)))


def step_sweep(a):
    import torch
    from fbstab_amd.hip_api import MPC_SEQ
    B, steps = a.batch, a.steps
    cm, d, A, Bm, x0 = _setup(B)
    cu, cx = _loss_seeds(B, steps)
    state = {}

    def forward():
        d["x0"] = x0.clone()
        state["fwd"] = cm.RecedingSweep(d, *_point(cm, B), A, Bm, steps, log=("x", "U", "v"))

    res = dict(forward_logged=timed(forward, a.reps))
    log = {k: state["fwd"][k] for k in ("x", "U", "v", "eflag")}
    rest = tuple(k for k in MPC_SEQ if k != "x0")

    def adjoint(key, **kw):
        state[key] = cm.RecedingSweepAdjoint(d, A, Bm, steps, log, gu=cu, gx=cx, mu=True, **kw)

    res["adjoint_x0_mu"] = timed(lambda: adjoint("b", want=()), a.reps)
    res["adjoint_all"] = timed(lambda: adjoint("c", want=rest), a.reps)
    res["adjoint_all_recondense"] = timed(lambda: adjoint("f", want=rest, mode="recondense"), a.reps)
    torch.cuda.synchronize()
    fwd = state["fwd"]
    xs = torch.cat([fwd["x"][1:], d["x0"][None]], 0)
    res["loss"] = float(((cu * fwd["u"]).sum() + (cx * xs).sum()).item())
    res["retired"] = int((fwd["eflag"][-1] == -1).sum().item())
    res["status_nonzero"] = int((state["c"]["status"] != 0).sum().item())
    gap = lambda s, t: float(((s - t).abs().max() / (1e-300 + t.abs().max())).item())
    res["x0_gap_b_vs_c"] = gap(state["b"]["x0"], state["c"]["x0"])
    res["gap_recondense_vs_affine"] = {k: gap(state["f"][k], state["c"][k]) for k in ("x0", "q", "Q", "d")}
    res["grad_sums"] = {k: float(state["c"][k].sum().item()) for k in ("x0", "q", "Q", "d")}
    res["adjoint_x0_mu_over_forward"] = res["adjoint_x0_mu"]["median_ms"] / res["forward_logged"]["median_ms"]
    res["adjoint_all_over_forward"] = res["adjoint_all"]["median_ms"] / res["forward_logged"]["median_ms"]
    return res


def step_loop(a):
    import torch
    from fbstab_amd import autograd as ag
    from fbstab_amd.hip_api import MPC_SEQ
    B, steps = a.batch, a.loop_steps
    cm, d, A, Bm, x0 = _setup(B)
    cu, cx = _loss_seeds(B, a.steps)
    fw, bw, state = [], [], {}
    for r in range(a.reps + 1):   # (round 0 warms)
        leaves = {k: d[k].clone().requires_grad_(True) for k in MPC_SEQ if k != "x0"}
        xk = x0.clone().requires_grad_(True)
        leaves["x0"] = xk
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        loss = 0.0
        for k in range(steps):
            data = dict(leaves)
            data["x0"] = xk
            z, l, v, out = ag.solve_condensed_mpc(cm, data)
            u0 = z[:, SHAPE[1]:SHAPE[1] + SHAPE[2]]
            xk = xk @ A.T + u0 @ Bm.T
            loss = loss + (cu[k] * u0).sum() + (cx[k] * xk).sum()
        e[1].record()
        loss.backward()
        e[2].record()
        e[2].synchronize()
        if r:
            fw.append(e[0].elapsed_time(e[1]))
            bw.append(e[1].elapsed_time(e[2]))
        state = dict(loss=float(loss.item()), grad_sums={k: float(leaves[k].grad.sum().item()) for k in ("x0", "q", "Q", "d")})
    scale = a.steps / steps
    res = dict(loop_forward=stats(fw), loop_backward=stats(bw), steps=steps, **state)
    res["label"] = "measured at %d steps" % steps + ("" if scale == 1 else ", SCALED linearly to %d" % a.steps)
    res["loop_forward_scaled_ms"] = res["loop_forward"]["median_ms"] * scale
    res["loop_backward_scaled_ms"] = res["loop_backward"]["median_ms"] * scale
    res["loop_backward_spread_scaled_ms"] = (res["loop_backward"]["max_ms"] - res["loop_backward"]["min_ms"]) * scale
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--loop-steps", type=int, default=0, help="steps of the Python loop (0: --steps)")
    ap.add_argument("--step", choices=STEPS, help="(internal) run one step in this process and print its JSON")
    a = ap.parse_args()
    assert a.reps >= 5
    a.loop_steps = a.loop_steps or a.steps
    if a.step:
        print("RESULT " + json.dumps(globals()["step_" + a.step](a)))
        return 0
    # the driver: it never opens the GPU itself; each step is a fresh child under a time limit of its own
    from fbstab_amd import hip_api
    line = dict(tool="condense_sweep_adjoint_bench", shape=list(SHAPE), batch=a.batch, steps=a.steps, reps=a.reps,
                library_sha256=hashlib.sha256(open(hip_api.LIB_PATH, "rb").read()).hexdigest())
    for step in STEPS:
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S[step]), sys.executable, os.path.abspath(__file__), "--step", step,
               "--reps", str(a.reps), "--steps", str(a.steps), "--batch", str(a.batch), "--loop-steps", str(a.loop_steps)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, cwd=ROOT)
        got = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not got:
            print("condense_sweep_adjoint_bench: step %s ended with status %d; nothing more is started"
                  % (step, r.returncode), file=sys.stderr)
            return r.returncode or 1
        line[step] = json.loads(got[-1][len("RESULT "):])
    line.update(line.pop("sweep"))
    lp = line["loop"]
    line["adjoint_all_over_loop_backward"] = line["adjoint_all"]["median_ms"] / lp["loop_backward_scaled_ms"]
    line["condition"] = dict(loop_backward_spread_ms=lp["loop_backward_spread_scaled_ms"],
                             met=bool(line["adjoint_all"]["median_ms"]
                                      <= lp["loop_backward_scaled_ms"] + lp["loop_backward_spread_scaled_ms"]))
    text = json.dumps(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "condense_sweep_adjoint_bench.json"), "w") as f:
        f.write(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
