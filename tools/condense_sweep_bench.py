#!/usr/bin/env python3
"""The closed-loop sweep of the condensed route (fbstab_amd/condense.py: CondensedMpc.RecedingSweep,
fbstab_hip_mpc_condensed_receding_sweep) against what the package had before it: one GPU, (N, nx, nu, nc) =
(10, 40, 3, 6), 2048 trajectories of ONE time-invariant model shared by the batch (`problem` below: a stable random
plant that is also the simulation model, constraints with slack at the origin), 50 steps
from a zero guess (a cold first step), no disturbance, no shift, retirement on.  Every timed call is warmed once, then
timed --reps times with torch events on torch's current stream; median, min and max in ms of the WHOLE sweep:
  affine       (a) RecedingSweep(mode="affine") - with the condensing, the map call and every allocation of the call
  recondense   (b) RecedingSweep(mode="recondense")
  python_loop  (c) the way before this call: Condense once, then per step CondensedMpc.Solve(recondense="vectors") and
               a torch plant step x0 <- x0 A' + u0 B'
  mpc_sweep    (d) FBstabMpcBatch.RecedingSweep at the same shape for --mpc-steps steps (the flat-vector kernel), SCALED
               to 50 steps: `scaled_to_steps_ms`
  map          the one-off fbstab_hip_mpc_condensed_x0_map_batch + f_c(0), b_c(0) (CondensedMpc.X0Map)
  t_sweep      (a) for traj_per_group in {rule / 2, rule, 2 rule}, and whether the bits agree
Ratios: `affine_over_recondense` = (a) / (b), `affine_over_python_loop` = (a) / (c): below 1 the new call wins.
`condition`: (a) is not slower than (c) by more than the spread (max - min) of (c)'s runs.
Each step below is a child process of its own under `timeout`, one after the other; a step that fails ends the run and
nothing more is started.  Writes profiles/condense_sweep_bench.json (one JSON line, with the library's sha256).

usage: python tools/condense_sweep_bench.py [--reps 7] [--steps 50] [--batch 2048] [--mpc-steps 3]"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPE = (10, 40, 3, 6)
SLACK, X0, ESCALE = 0.05, 0.5, 0.02    # the constraints' slack at the origin (SLACK .. 2 SLACK) and the scales of the initial states and of E
STEPS = ("sweeps", "t_sweep", "mpc_sweep")
STEP_TIMEOUT_S = dict(sweeps=420, t_sweep=240, mpc_sweep=420)


def stats(ms):
    return dict(median_ms=float(np.median(ms)), min_ms=float(np.min(ms)), max_ms=float(np.max(ms)))


def timed(f, reps):
    import torch
    ms = []
    for r in range(reps + 1):   # (round 0 warms)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        f()
        e1.record()
        e1.synchronize()
        if r:
            ms.append(e0.elapsed_time(e1))
    return stats(ms)


def problem(B):
    """(data: shared (1, len) sequences and x0 (B, nx), A, B row-major) as numpy arrays: a stable random plant
    (spectral radius 0.95), a positive definite stage cost, small linear terms, c = 0, and nc random constraint rows
    per stage with a slack of SLACK .. 2 SLACK at the origin: the origin is strictly feasible, and from initial states
    of scale X0 several rows are active over the first steps of a sweep (checked with the oracle on the CPU: every
    solve of 16 trajectories ends in SUCCESS)."""
    N, nx, nu, nc = SHAPE
    ns = nx + nu
    rng = np.random.default_rng(2024)
    A = np.eye(nx) + 0.05 * rng.standard_normal((nx, nx))
    A *= 0.95 / np.abs(np.linalg.eigvals(A)).max()
    Bm = 0.5 * rng.standard_normal((nx, nu))
    M = rng.standard_normal((ns, ns))
    H = M.T @ M / ns + 0.5 * np.eye(ns)
    E = rng.standard_normal((nc, nx)) * (rng.random((nc, nx)) < 0.4) * ESCALE
    L = rng.standard_normal((nc, nu)) * (rng.random((nc, nu)) < 0.6)
    img = lambda W, n: np.tile(np.ascontiguousarray(W.T).reshape(1, -1), (1, n))     # column-major, n stages
    data = dict(Q=img(H[:nx, :nx], N + 1), R=img(H[nx:, nx:], N + 1), S=img(H[nx:, :nx], N + 1),
                q=np.tile(0.1 * rng.standard_normal((1, nx)), (1, N + 1)),
                r=np.tile(0.1 * rng.standard_normal((1, nu)), (1, N + 1)),
                A=img(A, N), B=img(Bm, N), c=np.zeros((1, N * nx)), E=img(E, N + 1), L=img(L, N + 1),
                d=np.tile(-SLACK * (1.0 + rng.random((1, nc))), (1, N + 1)))
    data["x0"] = X0 * rng.standard_normal((B, nx))
    return data, np.ascontiguousarray(A), np.ascontiguousarray(Bm)


def _setup(B):
    import torch
    from fbstab_amd.condense import CondensedMpc
    data, A, Bm = problem(B)
    dev = torch.device("cuda:0")
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d = {k: to(a) for k, a in data.items()}
    cm = CondensedMpc(*SHAPE, max_batch=B)
    return cm, d, to(A), to(Bm), to(data["x0"])


def _point(cm, B):
    import torch
    return [torch.zeros((B, n), dtype=torch.float64, device="cuda:0") for n in (cm.nz, cm.nl, cm.nv, cm.nv)]


def step_sweeps(a):
    import torch
    B, steps = a.batch, a.steps
    cm, d, A, Bm, x0 = _setup(B)
    N, nx, nu, nc = SHAPE
    state = {}

    def sweep(mode, T=0):
        d["x0"] = x0.clone()
        state[mode] = cm.RecedingSweep(d, *_point(cm, B), A, Bm, steps, mode=mode, traj_per_group=T)

    def python_loop():
        d["x0"] = x0.clone()
        z, l, v, y = _point(cm, B)
        cm.Condense(d)
        us = []
        for k in range(steps):
            cm.Solve(d, z, l, v, y, recondense="vectors")
            u0 = z[:, nx:nx + nu]
            us.append(u0.clone())
            d["x0"] = d["x0"] @ A.T + u0 @ Bm.T
        state["loop_u"] = torch.stack(us)

    res = dict(affine=timed(lambda: sweep("affine"), a.reps), recondense=timed(lambda: sweep("recondense"), a.reps),
               python_loop=timed(python_loop, a.reps), map=timed(lambda: cm.X0Map(d), a.reps))
    torch.cuda.synchronize()
    ua, ur = state["affine"]["u"], state["recondense"]["u"]
    res["retired"] = int((state["affine"]["eflag"][-1] == -1).sum().item())
    res["success_all_steps"] = int((state["affine"]["eflag"] == 0).all(0).sum().item())
    res["newton_per_step_mean"] = float(state["affine"]["newton"].double().mean().item())
    gap = lambda s, t: float(((s - t).abs().max() / (1.0 + t.abs().max())).item())
    res["u_gap"] = dict(affine_vs_recondense=gap(ua, ur), python_loop_vs_recondense=gap(state["loop_u"], ur))
    res["affine_over_recondense"] = res["affine"]["median_ms"] / res["recondense"]["median_ms"]
    res["affine_over_python_loop"] = res["affine"]["median_ms"] / res["python_loop"]["median_ms"]
    spread = res["python_loop"]["max_ms"] - res["python_loop"]["min_ms"]
    res["condition"] = dict(python_loop_spread_ms=spread,
                            met=bool(res["affine"]["median_ms"] <= res["python_loop"]["median_ms"] + spread))
    return res


def step_t_sweep(a):
    import torch
    from fbstab_amd.condense import condensed_sweep_sizes
    B, steps = a.batch, a.steps
    cm, d, A, Bm, x0 = _setup(B)
    rule = condensed_sweep_sizes(*SHAPE, 0, True)
    values = sorted({max(1, rule["traj_per_group"] // 2), rule["traj_per_group"], 2 * rule["traj_per_group"]})
    res = dict(rule=rule)
    us = {}
    for T in values:
        def run(T=T):
            d["x0"] = x0.clone()
            us[T] = cm.RecedingSweep(d, *_point(cm, B), A, Bm, steps, traj_per_group=T)["u"]
        res["T%d" % T] = dict(timed(run, a.reps), sizes=condensed_sweep_sizes(*SHAPE, T, True))
    torch.cuda.synchronize()
    res["same_bits"] = all(torch.equal(us[T], us[values[0]]) for T in values)
    return res


def step_mpc_sweep(a):
    import torch
    from fbstab_amd import hip_api
    B = a.batch
    data, A, Bm = problem(B)
    dev = torch.device("cuda:0")
    d = {k: torch.from_numpy(np.broadcast_to(v, (B, v.shape[1])).copy(order="C")).to(dev) for k, v in data.items()}
    x0 = d["x0"].clone()
    m = hip_api.FBstabMpcBatch(*SHAPE, max_batch=B)
    N, nx, nu, nc = SHAPE
    lens = ((N + 1) * (nx + nu), (N + 1) * nx, (N + 1) * nc, (N + 1) * nc)

    def run():
        d["x0"] = x0.clone()
        m.RecedingSweep(d, *[torch.zeros((B, n), dtype=torch.float64, device=dev) for n in lens], A.copy(), Bm.copy(),
                        a.mpc_steps)

    res = dict(timed(run, a.reps), steps=a.mpc_steps)
    res["scaled_to_steps_ms"] = res["median_ms"] * a.steps / a.mpc_steps
    res["label"] = "SCALED from %d steps to %d" % (a.mpc_steps, a.steps)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--mpc-steps", type=int, default=3)
    ap.add_argument("--step", choices=STEPS, help="(internal) run one step in this process and print its JSON")
    a = ap.parse_args()
    assert a.reps >= 5
    if a.step:
        print("RESULT " + json.dumps(globals()["step_" + a.step](a)))
        return 0
    # the driver: it never opens the GPU itself; each step is a fresh child under a time limit of its own
    from fbstab_amd import hip_api
    line = dict(tool="condense_sweep_bench", shape=list(SHAPE), batch=a.batch, steps=a.steps, reps=a.reps,
                library_sha256=hashlib.sha256(open(hip_api.LIB_PATH, "rb").read()).hexdigest())
    for step in STEPS:
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S[step]), sys.executable, os.path.abspath(__file__), "--step", step,
               "--reps", str(a.reps), "--steps", str(a.steps), "--batch", str(a.batch), "--mpc-steps", str(a.mpc_steps)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, cwd=ROOT)
        got = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not got:
            print("condense_sweep_bench: step %s ended with status %d; nothing more is started" % (step, r.returncode),
                  file=sys.stderr)
            return r.returncode or 1
        line[step] = json.loads(got[-1][len("RESULT "):])
    line.update(line.pop("sweeps"))
    line["affine_over_mpc_sweep_scaled"] = line["affine"]["median_ms"] / line["mpc_sweep"]["scaled_to_steps_ms"]
    text = json.dumps(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "condense_sweep_bench.json"), "w") as f:
        f.write(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
