"""Warm-started receding-horizon sweep (BASELINE.json config 5): many closed-loop
trajectories, each step solving the same MPC QP with a new initial state
``x0 <- A x0 + B u0*`` and the previous solution ``(z, l, v)`` as the initial
guess, UNSHIFTED (the reference has no shift logic; its OcpGenerator only
exposes the simulation matrices, fbstab/test/ocp_generator.h:31-38).

``solve(x0, z, l, v) -> (z, l, v, y, out)`` is any batched solver: the HIP
library (arrays may stay on the device between steps) or, in the tests, the
oracle.  Arrays are ``(trajectories, n)`` numpy or torch, used through the
operations both support.

``logged_closed_loop`` is the sweep the device runs (fbstab_hip_mpc_receding_sweep*, include/fbstab_hip.h) in numpy,
around any batched ``solve`` (``oracle_solve``, or the device a step at a time), with a log: step k solves for x_k
from the previous point, retirement parks a trajectory at the origin with a zero point, the returned point is
logged, x_(k+1) = A x_k + B u_k + w_k (not for a parked trajectory), and with ``shift`` the point is moved one stage
towards the present - z_i <- z_(i+1), l_i <- l_(i+1), v_i <- v_(i+1) for i < N, stage N keeping its values - before
it is the next guess, except behind the last step.
"""
from __future__ import annotations

from typing import Callable, Dict, List

import numpy as np

from tools import fixtures as fx


def closed_loop(solve: Callable, x0, z, l, v, A, B, nx: int, nu: int, steps: int) -> List[Dict]:
    """Runs ``steps`` MPC steps.  ``A``/``B`` are (nx,nx)/(nx,nu) arrays of the
    same kind as ``x0``.  Returns per-step records (copies of x0, u0, out)."""
    log = []
    for k in range(steps):
        z, l, v, y, out = solve(x0, z, l, v)
        u0 = z[:, nx:nx + nu]
        log.append(dict(x0=x0.clone() if hasattr(x0, "clone") else x0.copy(),
                        u0=u0.clone() if hasattr(u0, "clone") else u0.copy(), out=out))
        x0 = x0 @ A.T + u0 @ B.T
    return log


def shift_point(z, l, v, sizes):
    """(z, l, v) ``(batch, n)`` moved one stage towards the present, in place (numpy arrays or torch tensors: slice
    copies from a clone of the source, so that no copy reads what it has written)."""
    N, nx, nu, nc = sizes
    for a, b in ((z, nx + nu), (l, nx), (v, nc)):
        src = a[:, b:].clone() if hasattr(a, "clone") else a[:, b:].copy()
        a[:, :N * b] = src
    return z, l, v


def logged_closed_loop(solve, p, A, B, steps, w=None, shift=False, retire=True, guess=None):
    """``solve(x0, z, l, v) -> (z, l, v, y, out)`` on ``(batch, n)`` numpy arrays, ``out`` a record array with
    eflag, newton_iters, prox_iters.  ``p``: the fixtures.MpcProblem whose x0 starts the loop; ``A``/``B`` row-major;
    ``w`` ``(steps, batch, nx)`` or None.  Returns the log:
    ``z, l, v`` (returned points, unshifted; zeros once retired), ``eflag`` (-1 once retired), ``x`` (the states the
    steps were solved for), ``u``, ``x_end`` - plus ``newton`` and ``prox`` ``(steps, batch)``, ``raw_eflag`` and
    ``point``: the (z, l, v) left behind the last step (unshifted)."""
    sizes = p.sizes()
    N, nx, nu, nc = sizes
    Bn = p.batch
    x0 = p.arrays["x0"].copy()
    z, l, v = ((np.zeros((Bn, p.nz)), np.zeros((Bn, p.nl)), np.zeros((Bn, p.nv))) if guess is None
               else tuple(a.copy() for a in guess))
    gone = np.zeros(Bn, dtype=bool)
    log = dict(z=[], l=[], v=[], eflag=[], x=[], u=[], newton=[], prox=[], raw_eflag=[])
    for k in range(steps):
        z, l, v, y, out = solve(x0, z, l, v)
        z, l, v = z.copy(), l.copy(), v.copy()
        if retire:
            gone = gone | (out["eflag"] != 0)
        z[gone] = 0.0; l[gone] = 0.0; v[gone] = 0.0
        u = z[:, nx:nx + nu].copy()
        log["z"].append(z.copy()); log["l"].append(l.copy()); log["v"].append(v.copy())
        log["eflag"].append(np.where(gone, -1, out["eflag"]).astype(np.int32))
        log["raw_eflag"].append(np.asarray(out["eflag"]).astype(np.int32))
        log["newton"].append(np.asarray(out["newton_iters"]).astype(np.int64))
        log["prox"].append(np.asarray(out["prox_iters"]).astype(np.int64))
        log["x"].append(x0.copy()); log["u"].append(u)
        x0 = x0 @ A.T + u @ B.T
        if w is not None:
            x0 = x0 + w[k]
        x0[gone] = 0.0
        if shift and k + 1 < steps:
            shift_point(z, l, v, sizes)
    res = {k: np.stack(a) for k, a in log.items()}
    res["x_end"] = x0
    res["point"] = (z, l, v)
    return res


def oracle_solve(oracle, p, opts=None):
    """``solve`` of ``logged_closed_loop`` with the oracle on ``p``'s data."""
    N, nx, nu, nc = p.sizes()

    def solve(x0, z, l, v):
        arr = dict(p.arrays)
        arr["x0"] = np.ascontiguousarray(x0)
        return oracle.solve_mpc(fx.MpcProblem(N, nx, nu, nc, arr), x0guess=(z, l, v), opts=opts,
                                nthreads=oracle.num_threads())
    return solve
