"""The reference of the linearised system V (dz, dl, dv) = (gz, -gl, -C.gv) that the adjoint and tangent entry
points solve (fbstab_hip_*_adjoint_batch, fbstab_hip_*_tangent_batch), for both kinds of QP (a fixtures.MpcProblem
or a fixtures.DenseProblem): the system's residual in extended precision, the oracle's solve of the same system, the
two gradient tables in numpy, the acceptance rule of the host and the GPU tests, and what the dense
central-difference tests need."""
import numpy as np

from fbstab_amd.hip_api import MPC_SEQ, DENSE_ARR
from tools import fixtures as fx
from tests import helpers as H
from tests.helpers import is_mpc

SIGMA = 1e-8
LD = np.longdouble


def names_of(p):
    return MPC_SEQ if is_mpc(p) else DENSE_ARR


def lengths_of(p):
    if is_mpc(p):
        return p.seq_lengths()
    return dict(H=p.nz * p.nz, f=p.nz, G=p.nl * p.nz, h=p.nl, A=p.nv * p.nz, b=p.nv)


def explicit(p, q):
    """(H, f, G, h, A, b) of QP ``q`` as explicit matrices."""
    return (H.mpc_explicit if is_mpc(p) else H.dense_explicit)(p, q)


def problem_like(p, arrays):
    """A problem of ``p``'s kind and shape whose data are ``arrays``."""
    if is_mpc(p):
        return fx.MpcProblem(p.N, p.nx, p.nu, p.nc, arrays)
    one = fx.DenseProblem(p.nz, p.nl, p.nv)
    one.arrays = arrays
    return one


def one_qp(p, q):
    """QP ``q`` of a problem as a problem of its own."""
    return problem_like(p, {k: np.ascontiguousarray(a[q:q + 1]) for k, a in p.arrays.items()})


def fb_derivatives(p, q, x, sigma=SIGMA, alpha=0.95):
    """(C, mus) = (d phi / d y, d phi / d v + sigma C) of the penalised FB function at the point x = xbar of
    QP ``q``, in longdouble (the formulas of helpers.newton_system_residual; pfb_gradient of fb_common.h;
    dense_cholesky_solver.cc:54-61)."""
    _, _, _, _, A, b = (np.asarray(m).astype(LD) for m in explicit(p, q))
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
    Hm, _, G, _, A, _ = (np.asarray(m).astype(LD) for m in explicit(p, q))
    C, mus = fb_derivatives(p, q, x, sigma, alpha)
    sig = LD(sigma)
    gz, gl, gv = (np.asarray(t).astype(LD) for t in seeds)
    dz, dl, dv = (np.asarray(t).astype(LD) for t in step)
    e1 = Hm @ dz + sig * dz + G.T @ dl + A.T @ dv - gz
    e2 = -G @ dz + sig * dl + gl
    e3 = -C * (A @ dz) + mus * dv + C * gv
    return float(np.sqrt((e1 * e1).sum() + (e2 * e2).sum() + (e3 * e3).sum()))


def oracle_adjoint(oracle, p, q, x, seeds, sigma=SIGMA, alpha=0.95):
    """(dz, dl, dv) of the oracle's linear solver (RiccatiLinearSolver or DenseCholeskySolver) for the adjoint's
    right-hand side (gz, -gl, -C.gv), with C from the oracle's own probe at x = xbar: its ``gamma`` is
    RiccatiLinearSolver::gamma_, d phi / d y itself (riccati_linear_solver.cc:91-98; Gamma_ = gamma_ / mus_ is the
    quotient)."""
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


def random_seeds(rng, p, batch=None):
    B = p.batch if batch is None else batch
    return (rng.standard_normal((B, p.nz)), rng.standard_normal((B, p.nl)), rng.standard_normal((B, p.nv)))


def mpc_gradient_table(p, x, step):
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


def dense_gradient_table(nz, nl, nv, x, step):
    """The gradients of the six arrays of ONE QP from its point x = (z, l, v) and adjoint (dz, dl, dv), the
    matrices as column-major images."""
    z, l, v = (np.asarray(t, dtype=np.float64) for t in x)
    dz, dl, dv = (np.asarray(t, dtype=np.float64) for t in step)
    cm = lambda M: M.T.reshape(-1)
    return dict(H=cm(-0.5 * (np.outer(dz, z) + np.outer(z, dz))), f=-dz, G=cm(-(np.outer(dl, z) + np.outer(l, dz))),
                h=dl.copy(), A=cm(-(np.outer(dv, z) + np.outer(v, dz))), b=dv.copy())


def check_step_and_table(p, q, x, seeds, step, grads, ref, probe_oracle=None):
    """The binding rule of the host and the GPU tests for one QP: the residual of V d = (gz, -gl, -C.gv) within
    3 x the oracle's (both in longdouble), and the gradients equal to the table applied to the returned adjoint
    (rtol 1e-13).  With ``probe_oracle`` (the MPC tests) also: the step within the forward error of the oracle's
    ``ref``, and the residual's own (C, mus) those of the oracle's RiccatiLinearSolver.  Returns (residual,
    oracle's residual)."""
    if probe_oracle is not None:
        z, l, v = x
        pr = probe_oracle.probe(one_qp(p, q), z, l, v, z, l, v, SIGMA, 0.95, r=np.zeros(p.nz + p.nl + p.nv), want_dx=True)
        C, mus = fb_derivatives(p, q, x)
        # (rows where both precisions take the same branch of the FB function: away from its switch at |(y, v)| =
        # 1e-13, and y of the same sign - on an active row y is zero to rounding, and the penalty term's kink at
        # y = 0 moves C by (1 - alpha) v with its sign)
        Am, bv = (m.astype(LD) for m in explicit(p, q)[4:])
        ys = bv - Am @ z.astype(LD)
        rr = np.hypot(pr["x_y"], v)
        far = ((rr >= 1e-12) | (rr < 1e-14)) & (np.sign(pr["x_y"]) == np.sign(ys.astype(np.float64)))
        assert far.sum() >= len(far) // 2
        np.testing.assert_allclose(C.astype(np.float64)[far], pr["gamma"][far], rtol=1e-12, atol=1e-13)
        np.testing.assert_allclose(mus.astype(np.float64)[far], pr["mus"][far], rtol=1e-12, atol=1e-13)
    r_dev = adjoint_residual(p, q, x, step, seeds)
    r_orc = adjoint_residual(p, q, x, ref, seeds)
    assert r_dev <= 3 * r_orc, (q, r_dev, r_orc)
    smax = max(np.abs(np.concatenate(step)).max(), 1.0)
    if probe_oracle is not None:
        assert np.abs(np.concatenate(step) - np.concatenate(ref)).max() <= 1e-5 * smax, q  # (forward error, cond(V) ~ 1e11)
    scale = smax * max(np.abs(np.concatenate(x)).max(), 1.0)
    tab = mpc_gradient_table(p, x, step) if is_mpc(p) else dense_gradient_table(p.nz, p.nl, p.nv, x, step)
    for k in names_of(p):
        np.testing.assert_allclose(grads[k], tab[k], rtol=1e-13, atol=1e-15 * scale, err_msg=k)
    return r_dev, r_orc


def check_mpc_batch(oracle, p, x, seeds, res):
    """``check_step_and_table`` with the MPC extras on every QP of ``res`` = Adjoint(..., adj=True): status 0, the
    device's residual within 3 x the oracle's, its step within the forward error of the oracle's, the residual's
    own (C, mus) those of the oracle's RiccatiLinearSolver, and the gradient table."""
    assert (res["status"] == 0).all()
    for q in range(p.batch):
        xq = tuple(t[q] for t in x)
        sq = tuple(t[q] for t in seeds)
        step = tuple(res[k][q] for k in ("dz", "dl", "dv"))
        ref = oracle_adjoint(oracle, p, q, xq, sq)
        check_step_and_table(p, q, xq, sq, step, {k: res[k][q] for k in MPC_SEQ}, ref, probe_oracle=oracle)


# -- central differences of the dense solution map -------------------------------------------------------------
def strict_qps(p, z, v, tol=1e-3):
    """QPs of the batch that are strictly complementary at ``tol`` (every row: y or v >= tol) and have fewer than
    nz active rows plus equalities, with their active sets (rows with v >= tol)."""
    out = []
    for q in range(p.batch):
        _, _, _, _, A, b = H.dense_explicit(p, q)
        y = b - A @ z[q]
        if np.maximum(y, v[q]).min() < tol:
            continue
        act = v[q] >= tol
        if act.sum() + p.nl < p.nz:
            out.append((q, act))
    return out


def active_set_solve(arr, nz, nl, nv, act):
    """(z, l, v) of the equality-constrained QP with the rows ``act`` of A held as equalities (the solution map
    near a strictly complementary point)."""
    Hm = arr["H"].reshape(nz, nz).T
    G = arr["G"].reshape(nz, nl).T
    A = arr["A"].reshape(nz, nv).T
    Aa = A[act]
    na = int(act.sum())
    K = np.block([[Hm, G.T, Aa.T], [G, np.zeros((nl, nl)), np.zeros((nl, na))],
                  [Aa, np.zeros((na, nl)), np.zeros((na, na))]])
    rhs = np.concatenate([-arr["f"], arr["h"], arr["b"][act]])
    s = np.linalg.solve(K, rhs)
    v = np.zeros(nv)
    v[act] = s[nz + nl:]
    return s[:nz], s[nz:nz + nl], v


def directions(rng, nz, nl, nv):
    """A random direction for each of the six dense arrays (symmetric for H), as flat column-major images."""
    M = rng.standard_normal((nz, nz))
    return dict(H=((M + M.T) / 2).reshape(-1), f=rng.standard_normal(nz), G=rng.standard_normal(nl * nz),
                h=rng.standard_normal(nl), A=rng.standard_normal(nv * nz), b=rng.standard_normal(nv))
