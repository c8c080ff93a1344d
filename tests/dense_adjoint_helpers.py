"""Shared helpers of the dense adjoint tests (fbstab_hip_dense_adjoint_batch): the adjoint system's residual in
extended precision, the gradient table in numpy, the oracle's solve of the same system, the host build of the
device logic (tests/hostsim/dense_adjoint.cc), and the active-set solve the central differences use."""
import ctypes as C
import os
import subprocess

import numpy as np

from tools import fixtures as fx
from tests import helpers as H

DENSE_ARR = ("H", "f", "G", "h", "A", "b")
SIGMA = 1e-8
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTSIM = os.path.join(ROOT, "tests", "hostsim")
_SO = os.path.join(HOSTSIM, "libhostsim_dense_adjoint.so")


def one_qp(p, q):
    """QP ``q`` of a DenseProblem as a problem of its own."""
    one = fx.DenseProblem(p.nz, p.nl, p.nv)
    one.arrays = {k: np.ascontiguousarray(a[q:q + 1]) for k, a in p.arrays.items()}
    return one


def fb_derivatives(p, q, x, sigma=SIGMA, alpha=0.95):
    """(C, mus) = (d phi / d y, d phi / d v + sigma C) of the penalised FB function at the point x = xbar of
    QP ``q``, in longdouble (pfb_gradient of fb_common.h; dense_cholesky_solver.cc:54-61)."""
    LD = np.longdouble
    _, _, _, _, A, b = (np.asarray(m).astype(LD) for m in H.dense_explicit(p, q))
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
    """2-norm, in longdouble, of V (dz, dl, dv) - (gz, -gl, -C.gv) at x = xbar (the system the adjoint solves)."""
    LD = np.longdouble
    Hm, _, G, _, A, _ = (np.asarray(m).astype(LD) for m in H.dense_explicit(p, q))
    Cc, mus = fb_derivatives(p, q, x, sigma, alpha)
    sig = LD(sigma)
    gz, gl, gv = (np.asarray(t).astype(LD) for t in seeds)
    dz, dl, dv = (np.asarray(t).astype(LD) for t in step)
    e1 = Hm @ dz + sig * dz + G.T @ dl + A.T @ dv - gz
    e2 = -G @ dz + sig * dl + gl
    e3 = -Cc * (A @ dz) + mus * dv + Cc * gv
    return float(np.sqrt((e1 * e1).sum() + (e2 * e2).sum() + (e3 * e3).sum()))


def oracle_adjoint(oracle, p, q, x, seeds, sigma=SIGMA, alpha=0.95):
    """(dz, dl, dv) of the oracle's DenseCholeskySolver for the adjoint's right-hand side (gz, -gl, -C.gv), with
    C from the oracle's own probe at x = xbar (its ``gamma`` is d phi / d y itself)."""
    one = one_qp(p, q)
    z, l, v = x
    nz, nl, nv = p.nz, p.nl, p.nv
    pr = oracle.probe(one, z, l, v, z, l, v, sigma, alpha, r=np.zeros(nz + nl + nv), want_dx=True)
    Cc = pr["gamma"]
    gz, gl, gv = seeds
    r = np.concatenate([gz, -np.asarray(gl), -Cc * gv])
    pr = oracle.probe(one, z, l, v, z, l, v, sigma, alpha, r=r, want_dx=True)
    assert pr["rc"] == 0
    dx = pr["dx"]
    return dx[:nz], dx[nz:nz + nl], dx[nz + nl:nz + nl + nv]


def gradient_table(nz, nl, nv, x, step):
    """The gradients of the six arrays of ONE QP from its point x = (z, l, v) and adjoint (dz, dl, dv), the
    matrices as column-major images."""
    z, l, v = (np.asarray(t, dtype=np.float64) for t in x)
    dz, dl, dv = (np.asarray(t, dtype=np.float64) for t in step)
    cm = lambda M: M.T.reshape(-1)
    return dict(H=cm(-0.5 * (np.outer(dz, z) + np.outer(z, dz))), f=-dz, G=cm(-(np.outer(dl, z) + np.outer(l, dz))),
                h=dl.copy(), A=cm(-(np.outer(dv, z) + np.outer(v, dz))), b=dv.copy())


def random_seeds(rng, p, batch=None):
    B = p.batch if batch is None else batch
    return (rng.standard_normal((B, p.nz)), rng.standard_normal((B, p.nl)), rng.standard_normal((B, p.nv)))


def check_step_and_table(p, q, x, seeds, step, grads, ref):
    """The binding rule of the host and the GPU tests for one QP: the residual of V d = (gz, -gl, -C.gv) within
    3 x the oracle's (both in longdouble), and the six gradients equal to the table applied to the returned
    adjoint (rtol 1e-13).  Returns (residual, oracle's residual)."""
    r_dev = adjoint_residual(p, q, x, step, seeds)
    r_orc = adjoint_residual(p, q, x, ref, seeds)
    assert r_dev <= 3 * r_orc, (q, r_dev, r_orc)
    smax = max(np.abs(np.concatenate(step)).max(), 1.0)
    scale = smax * max(np.abs(np.concatenate(x)).max(), 1.0)
    tab = gradient_table(p.nz, p.nl, p.nv, x, step)
    for k in DENSE_ARR:
        np.testing.assert_allclose(grads[k], tab[k], rtol=1e-13, atol=1e-15 * scale, err_msg=k)
    return r_dev, r_orc


# -- the host build of the device logic ----------------------------------------------------------------------
def _build():
    src = os.path.join(HOSTSIM, "dense_adjoint.cc")
    shim = os.path.join(HOSTSIM, "shim")
    deps = [src, os.path.join(shim, "hip", "hip_runtime.h")] + [
        os.path.join(ROOT, "fbstab_amd", "csrc", f) for f in ("fb_common.h", "fb_adjoint.h", "fb_mpc.h", "fb_dense.h")]
    if os.path.exists(_SO) and all(os.path.getmtime(_SO) >= os.path.getmtime(d) for d in deps):
        return
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I" + shim,
                           "-Wno-attributes", "-Wno-unknown-pragmas", "-o", _SO, src])


class HostDenseAdjoint:
    """DenseProblem<Ctx<1>> of fb_dense.h and dense_adjoint_contract of fb_adjoint.h on one host thread."""

    def __init__(self):
        _build()
        self.lib = C.CDLL(_SO)
        self.lib.hostsim_dense_adjoint.argtypes = [C.c_int] * 3 + [C.c_void_p] * 7 + [C.c_double, C.c_double,
                                                                                       C.c_void_p, C.c_void_p]
        self.lib.hostsim_dense_layout.argtypes = [C.c_int] * 4 + [C.c_void_p]

    def layout(self, nz, nl, nv, nthreads=256):
        """DenseLayout::init(nz, nl, nv, nthreads): dict(wave, k_global, v_global, a_lds, lds_doubles)."""
        out = (C.c_int * 5)()
        self.lib.hostsim_dense_layout(nz, nl, nv, nthreads, out)
        return dict(zip(("wave", "k_global", "v_global", "a_lds", "lds_doubles"), list(out)))

    def adjoint(self, p, q, x, seeds, sigma=SIGMA, alpha=0.95, want=DENSE_ARR):
        """Adjoint of QP ``q`` at x = (z, l, v) for seeds (gz, gl, gv) (gl / gv may be None): (status, (dz, dl,
        dv), gradients)."""
        pad = lambda a: a if a.size else np.zeros(1)
        keep = [pad(np.ascontiguousarray(p.arrays[k][q], dtype=np.float64)) for k in DENSE_ARR]
        data = (C.c_void_p * 6)(*[a.ctypes.data for a in keep])
        lens = dict(H=p.nz * p.nz, f=p.nz, G=p.nl * p.nz, h=p.nl, A=p.nv * p.nz, b=p.nv)
        grads = {k: np.full(lens[k], np.nan) for k in want}
        bufs = {k: pad(g) for k, g in grads.items()}
        gptr = (C.c_void_p * 6)(*[bufs[k].ctypes.data if k in bufs else None for k in DENSE_ARR])
        f64 = lambda a: None if a is None else pad(np.ascontiguousarray(a, dtype=np.float64))
        z, l, v = (f64(t) for t in x)
        gz, gl, gv = (f64(t) for t in seeds)
        adj = np.full(p.nz + p.nl + p.nv, np.nan)
        ptr = lambda a: None if a is None else a.ctypes.data
        st = self.lib.hostsim_dense_adjoint(p.nz, p.nl, p.nv, data, ptr(z), ptr(l), ptr(v), ptr(gz), ptr(gl),
                                            ptr(gv), sigma, alpha, adj.ctypes.data, gptr)
        for k in grads:
            if grads[k].size:
                grads[k] = bufs[k]
        return st, (adj[:p.nz], adj[p.nz:p.nz + p.nl], adj[p.nz + p.nl:]), grads


# -- central differences ---------------------------------------------------------------------------------------
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
    """A random direction for each of the six arrays (symmetric for H), as flat column-major images."""
    M = rng.standard_normal((nz, nz))
    return dict(H=((M + M.T) / 2).reshape(-1), f=rng.standard_normal(nz), G=rng.standard_normal(nl * nz),
                h=rng.standard_normal(nl), A=rng.standard_normal(nv * nz), b=rng.standard_normal(nv))
