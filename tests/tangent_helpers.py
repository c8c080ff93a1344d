"""Shared helpers of the tangent tests (fbstab_hip_*_tangent_batch): the numpy reference of the right-hand side
(gz, gl, gv) in extended precision with its rounding bound, and random directions."""
import numpy as np

from tests.linear_reference import LD, is_mpc, names_of, lengths_of, explicit, problem_like

U = 2.0 ** -53
# Duality of the tangent with the adjoint, |<g, J dtheta> - sum_k <grad_k, dtheta_k>| over the sum of the magnitudes
# of the terms of <g, J dtheta>: 10 x the largest disagreement of the two numbers when both steps come from the
# reference's own linear solver in its two roundings, Oracle() and Oracle(fma=True) (3.57e-9, measured by
# test_tangent_hostsim.py::test_tangent_end_to_end_on_the_host, which recomputes it; the host build of the
# device logic left 1.10e-9 there).  cond(V) ~ 1e11 at sigma = 1e-8 is what both sides of the identity go through.
DUALITY_BAR = 3.6e-8


def _carrier(p, arrays):
    """A one-QP problem of p's shape whose data are ``arrays`` (name -> flat array; absent or None: zeros)."""
    lens = lengths_of(p)
    full = {k: np.zeros((1, lens[k])) for k in names_of(p)}
    for k, a in arrays.items():
        if a is not None:
            full[k] = np.asarray(a, dtype=np.float64).reshape(1, lens[k])
    return problem_like(p, full)


def _explicit(p, arrays):
    """(dH, df, dG, dh, dA, db) of the perturbations ``arrays`` in longdouble: the explicit QP of a problem that
    carries them, minus that of the all-zero problem (which removes the constant -I blocks of the MPC's G)."""
    a = explicit(_carrier(p, arrays), 0)
    b = explicit(_carrier(p, {}), 0)
    return tuple(np.asarray(s).astype(LD) - np.asarray(t).astype(LD) for s, t in zip(a, b))


def _products(p, d):
    """Number of products T in every entry of (gz, gl, gv) for the perturbed names ``d`` (the additive vector
    counts as one; an entry of the symmetric part is two products, dM_rc x_c / 2 and dM_cr x_c / 2)."""
    has = lambda k: d.get(k) is not None
    if not is_mpc(p):
        tz = 2 * p.nz * has("H") + has("f") + p.nl * has("G") + p.nv * has("A")
        return (np.full(p.nz, tz), np.full(p.nl, p.nz * has("G") + has("h")), np.full(p.nv, p.nz * has("A") + has("b")))
    N, nx, nu, nc = p.sizes()
    tz = np.zeros((N + 1, nx + nu))
    tl = np.zeros((N + 1, nx))
    tv = np.full((N + 1, nc), nx * has("E") + nu * has("L") + has("d"))
    for i in range(N + 1):
        dyn = 0 if i == N else 1
        tz[i, :nx] = 2 * nx * has("Q") + nu * has("S") + has("q") + dyn * nx * has("A") + nc * has("E")
        tz[i, nx:] = 2 * nu * has("R") + nx * has("S") + has("r") + dyn * nx * has("B") + nc * has("L")
        tl[i] = has("x0") if i == 0 else nx * has("A") + nu * has("B") + has("c")
    return tz.reshape(-1), tl.reshape(-1), tv.reshape(-1)


def tangent_rhs(p, q, x, d):
    """The seeds of the tangent system for QP ``q`` of ``p``'s shape at x = (z, l, v) and the perturbations ``d``
    (name -> flat array of one QP; absent or None: zero),
        gz = -(sym(dH) z + df + dG' l + dA' v)      gl = dh - dG z      gv = db - dA z,
    in longdouble, and for every entry the bound (T + 4) 2^-53 S of a double-precision evaluation in any order: T
    its number of products (``_products``), S the sum of their magnitudes, the symmetric part taken as
    |d_rc| / 2 + |d_cr| / 2.  Returns ((gz, gl, gv), (bz, bl, bv)).  (``q`` only names the QP in messages: the
    right-hand side does not depend on the problem data.)"""
    dH, df, dG, dh, dA, db = _explicit(p, d)
    z, l, v = (np.asarray(t, dtype=np.float64).astype(LD) for t in x)
    gz = -(0.5 * (dH + dH.T) @ z + df + dG.T @ l + dA.T @ v)
    gl = dh - dG @ z
    gv = db - dA @ z
    aH, aG, aA = np.abs(dH), np.abs(dG), np.abs(dA)
    sz = 0.5 * (aH + aH.T) @ np.abs(z) + np.abs(df) + aG.T @ np.abs(l) + aA.T @ np.abs(v)
    sl = np.abs(dh) + aG @ np.abs(z)
    sv = np.abs(db) + aA @ np.abs(z)
    tz, tl, tv = _products(p, d)
    bound = lambda t, s: ((t + 4) * U * s).astype(np.float64)
    return (gz, gl, gv), (bound(tz, sz), bound(tl, sl), bound(tv, sv))


def assert_rhs(p, q, x, d, got, what=""):
    """``got`` = (gz, gl, gv) in double meets the bound of ``tangent_rhs`` entry by entry.  Returns the largest
    error / bound ratio."""
    ref, bnd = tangent_rhs(p, q, x, d)
    worst = 0.0
    for name, g, r, b in zip(("gz", "gl", "gv"), got, ref, bnd):
        err = np.abs(np.asarray(g).astype(LD) - r).astype(np.float64)
        bad = np.nonzero(~(err <= b))[0]
        assert bad.size == 0, (what, q, name, bad[:5], err[bad[:5]], b[bad[:5]])
        if err.size and (b > 0).any():
            worst = max(worst, float((err[b > 0] / b[b > 0]).max()))
    return worst


def random_directions(rng, p, batch, names=None, shared=()):
    """name -> (batch, len) standard-normal directions for ``names`` (default: all; the matrices NOT symmetric),
    ``(1, len)`` for the names in ``shared``."""
    lens = lengths_of(p)
    names = names_of(p) if names is None else names
    return {k: rng.standard_normal((1 if k in shared else batch, lens[k])) for k in names}


def one_direction(d, q):
    """QP ``q``'s rows of a dict of (B, len) / (1, len) directions."""
    return {k: (None if a is None else a[q if a.shape[0] > 1 else 0]) for k, a in d.items()}


def pairing(names, grads, d, q):
    """sum_k <grads[k], d[k]> of QP ``q`` in longdouble."""
    s = LD(0)
    for k in names:
        if d.get(k) is not None and d[k].size:
            s += np.asarray(grads[k][q] if np.ndim(grads[k]) == 2 else grads[k]).astype(LD) @ one_direction(d, q)[k].astype(LD)
    return s
