"""Shared helpers of the adjoint tests (fbstab_hip_mpc_adjoint_batch): the adjoint system's residual in
extended precision, the gradient table in numpy, and the oracle's solve of the same system."""
import numpy as np

from tools import fixtures as fx
from tests import helpers as H

MPC_SEQ = ("Q", "R", "S", "q", "r", "A", "B", "c", "E", "L", "d", "x0")
SIGMA = 1e-8


def one_qp(p, q):
    """QP ``q`` of an MpcProblem as a problem of its own."""
    return fx.MpcProblem(p.N, p.nx, p.nu, p.nc, {k: np.ascontiguousarray(a[q:q + 1]) for k, a in p.arrays.items()})


def fb_derivatives(p, q, x, sigma=SIGMA, alpha=0.95):
    """(C, mus) = (d phi / d y, d phi / d v + sigma C) of the penalised FB function at the point x = xbar of
    QP ``q``, in longdouble (the formulas of helpers.newton_system_residual)."""
    LD = np.longdouble
    _, _, _, _, A, b = (m.astype(LD) for m in H.mpc_explicit(p, q))
    z, l, v = (np.asarray(t).astype(LD) for t in x)
    sig, al = LD(sigma), LD(alpha)
    ys = b - A @ z
    rr = np.sqrt(ys * ys + v * v)
    c0 = al * (1 - 1 / np.sqrt(LD(2)))
    safe = np.where(rr > 0, rr, 1)
    gam = np.where(rr < 1e-13, c0, al * (1 - ys / safe))
    mu = np.where(rr < 1e-13, c0, al * (1 - v / safe))
    pos = (rr >= 1e-13) & (ys > 0) & (v > 0)
    gam = np.where(pos, gam + (1 - al) * v, gam)
    mu = np.where(pos, mu + (1 - al) * ys, mu)
    return gam, mu + sig * gam


def adjoint_residual(p, q, x, step, seeds, sigma=SIGMA, alpha=0.95):
    """2-norm, in longdouble, of V (dz, dl, dv) - (gz, -gl, -C.gv) at x = xbar (the system the adjoint solves;
    V as in helpers.newton_system_residual)."""
    LD = np.longdouble
    Hm, _, G, _, A, _ = (m.astype(LD) for m in H.mpc_explicit(p, q))
    C, mus = fb_derivatives(p, q, x, sigma, alpha)
    sig = LD(sigma)
    gz, gl, gv = (np.asarray(t).astype(LD) for t in seeds)
    dz, dl, dv = (np.asarray(t).astype(LD) for t in step)
    e1 = Hm @ dz + sig * dz + G.T @ dl + A.T @ dv - gz
    e2 = -G @ dz + sig * dl + gl
    e3 = -C * (A @ dz) + mus * dv + C * gv
    return float(np.sqrt((e1 * e1).sum() + (e2 * e2).sum() + (e3 * e3).sum()))


def oracle_adjoint(oracle, p, q, x, seeds, sigma=SIGMA, alpha=0.95):
    """(dz, dl, dv) of the oracle's RiccatiLinearSolver for the adjoint's right-hand side (gz, -gl, -C.gv), with
    C from the oracle's own probe at x = xbar: its ``gamma`` is RiccatiLinearSolver::gamma_, d phi / d y itself
    (riccati_linear_solver.cc:91-98; Gamma_ = gamma_ / mus_ is the quotient)."""
    one = one_qp(p, q)
    z, l, v = x
    nz, nl, nv = p.nz, p.nl, p.nv
    pr = oracle.probe(one, z, l, v, z, l, v, sigma, alpha, r=np.zeros(nz + nl + nv), want_dx=True)
    C = pr["gamma"]
    gz, gl, gv = seeds
    r = np.concatenate([gz, -np.asarray(gl), -C * gv])
    pr = oracle.probe(one, z, l, v, z, l, v, sigma, alpha, r=r, want_dx=True)
    assert pr["rc"] == 0
    dx = pr["dx"]
    return dx[:nz], dx[nz:nz + nl], dx[nz + nl:nz + nl + nv]


def gradient_table(p, x, step):
    """The gradients of the 12 sequences of ONE QP from its point x = (z, l, v) and adjoint (dz, dl, dv), in the
    reference layout (column-major stage matrices, stage-major)."""
    N, nx, nu, nc = p.sizes()
    ns = nx + nu
    z, l, v = (np.asarray(t, dtype=np.float64) for t in x)
    dz, dl, dv = (np.asarray(t, dtype=np.float64) for t in step)
    Z, DZ = z.reshape(N + 1, ns), dz.reshape(N + 1, ns)
    X, U, DX, DU = Z[:, :nx], Z[:, nx:], DZ[:, :nx], DZ[:, nx:]
    Lm, DL = l.reshape(N + 1, nx), dl.reshape(N + 1, nx)
    V, DV = v.reshape(N + 1, nc), dv.reshape(N + 1, nc)
    outer = lambda a, b: a[:, :, None] * b[:, None, :]
    cm = lambda M: np.transpose(M, (0, 2, 1)).reshape(-1)   # (stage, row, col) -> column-major stage images
    return dict(
        Q=cm(-0.5 * (outer(DX, X) + outer(X, DX))), R=cm(-0.5 * (outer(DU, U) + outer(U, DU))),
        S=cm(-(outer(DU, X) + outer(U, DX))), q=-DX.reshape(-1), r=-DU.reshape(-1),
        A=cm(-(outer(DL[1:], X[:-1]) + outer(Lm[1:], DX[:-1]))), B=cm(-(outer(DL[1:], U[:-1]) + outer(Lm[1:], DU[:-1]))),
        c=-DL[1:].reshape(-1), E=cm(-(outer(DV, X) + outer(V, DX))), L=cm(-(outer(DV, U) + outer(V, DU))),
        d=-DV.reshape(-1), x0=-DL[0].copy())


def random_seeds(rng, p, batch=None):
    B = p.batch if batch is None else batch
    return (rng.standard_normal((B, p.nz)), rng.standard_normal((B, p.nl)), rng.standard_normal((B, p.nv)))
