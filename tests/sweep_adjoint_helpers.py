"""Shared helpers of the sweep-adjoint tests (fbstab_hip_mpc_receding_sweep_adjoint): the backward recursion
through a logged receding-horizon sweep in numpy, with the per-step adjoint pluggable (the oracle's linear solver,
or the device's own ``Adjoint`` at the logged points), over the log of tests/closed_loop.logged_closed_loop or the
device's, and the bars and the problem the CPU and GPU tests share.

The recursion (include/fbstab_hip.h): with u_k = z_k[nx:nx+nu] and x_(k+1) = A x_k + B u_k, start with lambda = 0
and for k = T-1 .. 0:  mu = gx[k] + lambda;  eflag -1: lambda <- 0;  eflag != 0: lambda <- A'mu;  otherwise one
adjoint at the logged point with the seed gu[k] + B'mu on the u0 entries of z: a failed factorisation counts in
``status`` and gives lambda <- A'mu, a good one adds its gradient table to the sums and gives
lambda <- A'mu - dl[0:nx].  The x0 slot is the final lambda."""
import numpy as np

from fbstab_amd.hip_api import MPC_SEQ
from tools import fixtures as fx
from tests import helpers as H
from tests import linear_reference as LR


def reference_sweep_adjoint(adjoint_fn, p, A, B, log, gu, gx, retire=True):
    """``adjoint_fn(k, x, gz, active) -> (status, grads)``: the adjoints of step k's batch at the points
    ``x = (z, l, v)`` (``(batch, n)``) for the seeds ``gz`` (``(batch, nz)``; gl = gv = 0): ``status`` ``(batch,)``
    and ``grads`` name -> ``(batch, len)`` for the 12 sequences (rows outside ``active`` are not looked at).
    ``A``/``B``: the plant, row-major; ``log``: dict of ``z, l, v`` ``(T, batch, n)`` and ``eflag`` ``(T, batch)``;
    ``gu``/``gx``: ``(T, batch, nu | nx)`` or None.  ``retire`` only documents how the log was made: a retired
    step carries eflag -1.  Returns ``(grads, status, mu)``."""
    N, nx, nu, nc = p.sizes()
    T, Bn = log["eflag"].shape
    lens = p.seq_lengths()
    grads = {k: np.zeros((Bn, lens[k])) for k in MPC_SEQ}
    status = np.zeros(Bn, dtype=np.int32)
    mu_log = np.zeros((T, Bn, nx))
    lam = np.zeros((Bn, nx))
    for k in range(T - 1, -1, -1):
        mu = (gx[k] if gx is not None else 0.0) + lam
        mu_log[k] = mu
        e = log["eflag"][k]
        atm = mu @ A                      # rows: A'mu
        s = (gu[k] if gu is not None else 0.0) + mu @ B
        gz = np.zeros((Bn, p.nz))
        gz[:, nx:nx + nu] = s
        active = e == 0
        st, tab = (adjoint_fn(k, (log["z"][k], log["l"][k], log["v"][k]), gz, active) if active.any()
                   else (np.zeros(Bn, dtype=np.int32), None))
        for q in range(Bn):
            if e[q] == -1:
                lam[q] = 0.0
            elif e[q] != 0:
                lam[q] = atm[q]
            elif st[q] != 0:
                status[q] += 1
                lam[q] = atm[q]
            else:
                for name in MPC_SEQ:
                    if name != "x0":
                        grads[name][q] += tab[name][q]
                lam[q] = atm[q] + tab["x0"][q]      # (the table's x0 entry is -dl[0:nx])
    grads["x0"] = lam.copy()
    return grads, status, mu_log


def oracle_step_adjoint(oracle, p, sigma=LR.SIGMA):
    """The per-step adjoint from the oracle's RiccatiLinearSolver and the gradient table in numpy."""
    lens = p.seq_lengths()

    def fn(k, x, gz, active):
        grads = {name: np.zeros((p.batch, lens[name])) for name in MPC_SEQ}
        for q in np.flatnonzero(active):
            xq = tuple(t[q] for t in x)
            step = LR.oracle_adjoint(oracle, p, q, xq, (gz[q], np.zeros(p.nl), np.zeros(p.nv)), sigma)
            tab = LR.mpc_gradient_table(LR.one_qp(p, q), xq, step)
            for name in MPC_SEQ:
                grads[name][q] = tab[name]
        return np.zeros(p.batch, dtype=np.int32), grads
    return fn


def device_step_adjoint(solver, p, sigma=0.0):
    """The per-step adjoint from the device's own ``Adjoint`` at the logged points (host arrays)."""
    def fn(k, x, gz, active):
        g = solver.Adjoint(p.arrays, *(np.ascontiguousarray(t) for t in x), np.ascontiguousarray(gz), sigma=sigma)
        return g["status"], g
    return fn


def spread_bars(oracle, oracle_fma, p, A, B, log, gu, gx):
    """Per sequence: ten times the spread between the two roundings of the reference (the oracle and its
    fused-multiply-add build as per-step adjoints of the same recursion at the same logged points), relative to
    the gradient's largest entry, the largest over the trajectories.  Returns (bars, spreads)."""
    a = reference_sweep_adjoint(oracle_step_adjoint(oracle, p), p, A, B, log, gu, gx)[0]
    b = reference_sweep_adjoint(oracle_step_adjoint(oracle_fma, p), p, A, B, log, gu, gx)[0]
    spread = {}
    for k in MPC_SEQ:
        top = np.abs(a[k]).max(axis=1)
        rel = np.abs(a[k] - b[k]).max(axis=1) / np.where(top > 0, top, 1.0)
        spread[k] = float(rel.max())
    return {k: 10.0 * s for k, s in spread.items()}, spread


def assert_within(got, ref, bars, what, rows=None):
    for k in MPC_SEQ:
        for q in (range(ref[k].shape[0]) if rows is None else rows):
            top = np.abs(ref[k][q]).max()
            err = np.abs(got[k][q] - ref[k][q]).max() / (top if top > 0 else 1.0)
            assert err <= bars[k], (what, k, q, err, bars[k])


def strictly_complementary(p, log, tol=1e-3):
    """Trajectories whose every step ended in SUCCESS at a point with max(y, v) >= tol on every row."""
    T, Bn = log["eflag"].shape
    N, nx, nu, nc = p.sizes()
    good = []
    for q in range(Bn):
        ok = True
        for k in range(T):
            arr = {name: a[q:q + 1] for name, a in p.arrays.items()}
            arr["x0"] = log["x"][k][q:q + 1]
            one = fx.MpcProblem(N, nx, nu, nc, arr)
            Am, bv = H.mpc_explicit(one, 0)[4:]
            y = bv - Am @ log["z"][k][q]
            ok = ok and log["eflag"][k][q] == 0 and np.maximum(y, log["v"][k][q]).min() >= tol
        if ok:
            good.append(q)
    return good


def sym_direction(rng, n, stages):
    M = rng.standard_normal((stages, n, n))
    return (M + np.transpose(M, (0, 2, 1))).reshape(stages, -1).reshape(-1) / 2


FD_SHAPE = (6, 4, 2, 6)
FD_STEPS = 3
FD_TRAJ = 8
# (2024, the first seed tried, and 2029 each hold a trajectory whose inputs are pinned by active constraints at
# every step: its cost gradients are exactly zero, and the rule below then compares the O(sigma) bias of the
# regularised adjoint with itself.  Seeds 2025-2028 and 2030-2032 pass on the oracle with margins of 5 to 100.)
FD_SEED = 2025
FD_H = 1e-5
FD_NAMES = ("q", "r", "d", "x0", "Q")


def fd_problem():
    """The problem of the central-difference tests: 8 random LTV QPs of shape (6, 4, 2, 6), a random stable plant,
    a random linear loss in (u, x) and one direction per tested sequence."""
    rng = np.random.default_rng(FD_SEED)
    N, nx, nu, nc = FD_SHAPE
    p = fx.random_ltv_mpc(rng, FD_TRAJ, *FD_SHAPE)
    A = 0.9 * np.eye(nx) + 0.1 * rng.standard_normal((nx, nx))
    B = 0.3 * rng.standard_normal((nx, nu))
    cu = rng.standard_normal((FD_STEPS, FD_TRAJ, nu))
    cx = rng.standard_normal((FD_STEPS, FD_TRAJ, nx))
    lens = p.seq_lengths()
    dirs = {k: (sym_direction(rng, nx, N + 1) if k == "Q" else rng.standard_normal(lens[k])) for k in FD_NAMES}
    return p, A, B, cu, cx, dirs


def fd_check(run, grads, good, p, cu, cx, dirs):
    """Central differences of L = <cu, u> + <cx, x> along ``dirs`` against ``grads`` for the trajectories
    ``good``, under |fd - ad| <= 1e-4 max(|ad|, 1e-2 sum|grad|).  ``run(problem) -> (u, x)``: the closed loop,
    u ``(T, batch, nu)`` and x ``(T, batch, nx)`` the states AFTER each step.  Returns the figures."""
    N, nx, nu, nc = p.sizes()
    figures = []
    for name in FD_NAMES:
        L = []
        for sg in (1.0, -1.0):
            arr = {k: a.copy() for k, a in p.arrays.items()}
            arr[name] = arr[name] + sg * FD_H * dirs[name][None]
            u, x = run(fx.MpcProblem(N, nx, nu, nc, arr))
            L.append((cu * u).sum(axis=(0, 2)) + (cx * x).sum(axis=(0, 2)))
        fd = (L[0] - L[1]) / (2 * FD_H)
        for q in good:
            ad = float(grads[name][q] @ dirs[name])
            bound = 1e-4 * max(abs(ad), 1e-2 * np.abs(grads[name][q]).sum())
            figures.append((name, q, fd[q], ad, bound))
    return figures
