"""Shared helpers of the batch-summed gradient tests (fbstab_hip_*_adjoint_batch_reduced): the gradient tables of
fb_adjoint.h summed over a batch in any numpy precision, with the magnitude sum that bounds the rounding error of
such a sum in any order, and the constants of fbstab_amd/csrc/fb_grad_reduce_plan.h."""
import os
import re

import numpy as np

from fbstab_amd.hip_api import MPC_SEQ, DENSE_ARR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fbstab_amd", "csrc")
PLAN_HEADER = os.path.join(CSRC, "fb_grad_reduce_plan.h")

# (the matrices are the names in capitals: Q R S A B E L, and H G A)
MPC_MATRICES = tuple(k for k in MPC_SEQ if k.isupper())
DENSE_MATRICES = tuple(k for k in DENSE_ARR if k.isupper())

DENSE_SHAPES = ((50, 10, 100), (30, 0, 40), (5, 2, 9))
MPC_SHAPES = ((3, 12, 4, 20), (4, 5, 2, 7), (3, 18, 5, 10), (2, 34, 3, 5))


def plan_constant(name):
    """An integer constant of the plan header (``constexpr int name = <expression of integers>;``)."""
    m = re.search(r"constexpr int %s = ([0-9 *+]+);" % name, open(PLAN_HEADER).read())
    assert m, name
    return int(eval(m.group(1)))  # (digits, blanks, * and + only)


def chunk():
    return plan_constant("kGradReduceChunk")


def mpc_lens(N, nx, nu, nc):
    return dict(Q=(N + 1) * nx * nx, R=(N + 1) * nu * nu, S=(N + 1) * nu * nx, q=(N + 1) * nx, r=(N + 1) * nu,
                A=N * nx * nx, B=N * nx * nu, c=N * nx, E=(N + 1) * nc * nx, L=(N + 1) * nc * nu, d=(N + 1) * nc, x0=nx)


def dense_lens(nz, nl, nv):
    return dict(H=nz * nz, f=nz, G=nl * nz, h=nl, A=nv * nz, b=nv)


def _outer(a, w, zc, dzc, scale):
    """(sum_b scale (a_b zc_b' + w_b dzc_b'), sum_b |scale| (|a_b| |zc_b|' + |w_b| |dzc_b|')) as column-major images;
    a, w: (B, m), zc, dzc: (B, n)."""
    val = scale * (a.T @ zc + w.T @ dzc)
    mag = abs(scale) * (np.abs(a).T @ np.abs(zc) + np.abs(w).T @ np.abs(dzc))
    return val.T.reshape(-1), mag.T.reshape(-1)


def _vec(a, sign):
    return sign * a.sum(axis=0), np.abs(a).sum(axis=0)


def dense_sum_table(nz, nl, nv, x, step, keep=None, dtype=np.longdouble):
    """{name: (sum over the batch of the per-QP gradient, sum of the magnitudes of its terms)} from the points
    x = (z, l, v) and adjoint steps (dz, dl, dv), each (B, n); ``keep``: boolean (B,), the QPs that take part."""
    z, l, v, dz, dl, dv = _rows(x, step, keep, dtype)
    return dict(H=_outer(dz, z, z, dz, -0.5), f=_vec(dz, -1), G=_outer(dl, l, z, dz, -1.0), h=_vec(dl, 1),
                A=_outer(dv, v, z, dz, -1.0), b=_vec(dv, 1))


def _rows(x, step, keep, dtype):
    arrs = [np.asarray(t) for t in tuple(x) + tuple(step)]
    if keep is not None:
        arrs = [a[np.asarray(keep, dtype=bool)] for a in arrs]
    return [a.astype(dtype) for a in arrs]


def mpc_sum_table(N, nx, nu, nc, x, step, keep=None, dtype=np.longdouble):
    """The MPC table of fbstab_amd/csrc/fb_adjoint.h, summed over the batch: as dense_sum_table, for the twelve
    sequences (stage matrices column-major, stage after stage)."""
    z, l, v, dz, dl, dv = _rows(x, step, keep, dtype)
    ns = nx + nu
    parts = {k: [] for k in MPC_SEQ}
    for i in range(N + 1):
        xs, dxs = z[:, i * ns:i * ns + nx], dz[:, i * ns:i * ns + nx]
        us, dus = z[:, i * ns + nx:(i + 1) * ns], dz[:, i * ns + nx:(i + 1) * ns]
        vi, dvi = v[:, i * nc:(i + 1) * nc], dv[:, i * nc:(i + 1) * nc]
        parts["Q"].append(_outer(dxs, xs, xs, dxs, -0.5))
        parts["R"].append(_outer(dus, us, us, dus, -0.5))
        parts["S"].append(_outer(dus, us, xs, dxs, -1.0))
        parts["q"].append(_vec(dxs, -1))
        parts["r"].append(_vec(dus, -1))
        if i < N:
            lp, dlp = l[:, (i + 1) * nx:(i + 2) * nx], dl[:, (i + 1) * nx:(i + 2) * nx]
            parts["A"].append(_outer(dlp, lp, xs, dxs, -1.0))
            parts["B"].append(_outer(dlp, lp, us, dus, -1.0))
            parts["c"].append(_vec(dlp, -1))
        parts["E"].append(_outer(dvi, vi, xs, dxs, -1.0))
        parts["L"].append(_outer(dvi, vi, us, dus, -1.0))
        parts["d"].append(_vec(dvi, -1))
    parts["x0"].append(_vec(dl[:, :nx], -1))
    return {k: (np.concatenate([t[0] for t in p]), np.concatenate([t[1] for t in p])) for k, p in parts.items()}


def check_sum(name, got, table, batch):
    """|got - table| <= (2 B + 4) 2^-53 S entry by entry: S the sum over the batch of the magnitudes of the (at
    most two) products of the entry, so that 2 B rounded products summed in ANY order - and the factor, the sign
    and the last rounding to a double - stay within it.  Returns the largest ratio difference / bound."""
    val, mag = table
    got = np.asarray(got).reshape(-1)
    assert got.shape == val.shape, (name, got.shape, val.shape)
    assert np.isfinite(got).all(), name
    diff = np.abs(got.astype(np.longdouble) - val)
    bound = np.longdouble(2 * batch + 4) * np.longdouble(2.0) ** -53 * mag
    bad = diff > bound
    assert not bad.any(), (name, int(bad.sum()), float(diff[bad].max()), float(bound[bad].min()))
    nz = bound > 0
    return float((diff[nz] / bound[nz]).max()) if nz.any() else 0.0
