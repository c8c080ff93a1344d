"""TEST INFRASTRUCTURE ONLY: what tests/test_condense_tangent_cpu.py and tests/test_gpu_condense_tangent.py share -
the forward mode of the condensed route (fbstab_hip_mpc_condensed_tangent_batch) as a chain of the host builds of its
device logic, the duality number, and one call of the C-ABI on device copies with NaN behind every vector."""
import ctypes as C

import numpy as np

from tests import condense_adjoint_helpers as cah
from tests import condense_helpers as ch
from tests import tangent_helpers as TH
from tests.helpers import mpc_explicit

LD = ch.LD
MPC_NAMES = ch.MPC_NAMES
STEP = ("dz", "dl", "dv")
SEEDS = ("gz", "gl", "gv")
NAN = float("nan")


def symmetrised(p, d):
    """``d`` with dQ and dR replaced by their symmetric parts (what a finite difference of the data can move)."""
    d = dict(d)
    for k, n in (("Q", p.nx), ("R", p.nu)):
        M = d[k].reshape(d[k].shape[0], p.N + 1, n, n)
        d[k] = np.ascontiguousarray(0.5 * (M + M.transpose(0, 1, 3, 2))).reshape(d[k].shape)
    return d


def strictness(p, q, z, v):
    """min over the rows of max(y, v) at the point of QP ``q``: the margin of strict complementarity."""
    _, _, _, _, A, b = mpc_explicit(p, q)
    return float(np.maximum(b - A @ z[q], v[q]).min())


class HostChain:
    """The condensed chain on the host for any seeds: HostCondenseAdjoint.seed, the double solve of the condensed
    system V_c (cah.dense_system at the longdouble images of the QP) refined once on its longdouble residual, then
    HostCondenseAdjoint.finish with no gradient slot."""

    def __init__(self, p, q, x, host_adjoint, sigma=cah.SIGMA):
        self.p, self.q, self.x, self.host = p, q, x, host_adjoint
        img = ch.condense_reference(p, q)
        self.V, self.Cg = cah.dense_system(p, q, x, img["H"], img["A"], sigma)
        self.V64 = self.V.astype(np.float64)

    def step(self, seeds):
        gz, gl, gv = seeds
        _, gU, gvc = self.host.seed(self.p, self.q, self.x[0], gz, gl, gv)
        r = np.concatenate([gU.astype(LD), -self.Cg * gvc.astype(LD)])
        s = np.linalg.solve(self.V64, r.astype(np.float64))
        s = s + np.linalg.solve(self.V64, (r - self.V @ s.astype(LD)).astype(np.float64))
        nzc = len(gU)
        _, step = self.host.finish(self.p, self.q, self.x, gz, gl, s[:nzc], s[nzc:], want=())
        return step


def duality_number(g, dx, grads, d):
    """|<g, dx> - sum_k <grads[k], d[k]>| over the sum of the magnitudes of the terms of <g, dx>, in longdouble:
    ``g``, ``dx`` triples of one QP, ``grads`` and ``d`` name -> flat array (a None direction is zero)."""
    gg, xx = np.concatenate(g).astype(LD), np.concatenate(dx).astype(LD)
    other = sum(np.asarray(grads[k]).astype(LD) @ np.asarray(d[k]).astype(LD) for k in MPC_NAMES if d.get(k) is not None)
    return float(abs(gg @ xx - other) / np.abs(gg * xx).sum())


def raw_tangent(hip, handle, p, img, x, d, qps=None, pad=0, rhs=True, sigma=0.0, batch=None):
    """One call of fbstab_hip_mpc_condensed_tangent_batch on device copies (the QPs ``qps`` of ``p``, of the images
    ``img`` and of the point ``x``): dict rc, msg, dz, dl, dv, status, with ``rhs`` gz, gl, gv, and ``work_tail``, the
    doubles of the work array behind its documented length.  Every vector and image carries ``pad`` doubles of NaN
    behind its length, every output is pre-filled with NaN.  ``d``: name -> (batch, len) direction, (1, len) for one
    that travels with stride 0, None or absent for a NULL slot.  A (1, len) array of ``p`` or ``img`` beside more QPs
    is passed with stride 0."""
    import torch
    lib = hip.load_library()
    Bp = p.arrays["x0"].shape[0]
    qps = list(range(Bp)) if qps is None else list(qps)
    B = len(qps)
    N, nx, nu, nc = p.sizes()
    nzc, nv = (N + 1) * nu, (N + 1) * nc
    keep = []

    def dev(a, fill=NAN):
        a = np.asarray(a, dtype=np.float64)
        t = torch.full((a.shape[0], a.shape[1] + pad), fill, dtype=torch.float64, device="cuda")
        t[:, :a.shape[1]] = torch.from_numpy(np.ascontiguousarray(a)).cuda()
        keep.append(t)
        return t

    def block(blk, names, arrays, slots=None):
        for i, k in enumerate(names):
            a = arrays.get(k)
            if a is None:
                continue
            one = a.shape[0] == 1 and Bp > 1
            t = dev(a if a.shape[0] == 1 else a[qps])
            j = i if slots is None else slots[i]
            blk.base[j], blk.stride[j] = t.data_ptr(), (0 if one else t.shape[1])

    data, dirb, dense = hip._MpcBatch(), hip._MpcBatch(), hip._DenseBatch()
    block(data, MPC_NAMES, p.arrays)
    block(dirb, MPC_NAMES, d)
    block(dense, ("H", "f", "A", "b"), img, slots=(0, 1, 4, 5))
    xb, ob, rb = hip._VarBatch(), hip._VarBatch(), hip._VarBatch()
    out = {}
    var_lens = (p.nz, p.nl, p.nv)
    for i, (a, n) in enumerate(zip(x, var_lens)):
        t = dev(a[qps])
        xb.base[i], xb.stride[i] = t.data_ptr(), t.shape[1]
        for names, blk in ((STEP, ob),) + (((SEEDS, rb),) if rhs else ()):
            out[names[i]] = torch.full((B, n + pad), NAN, dtype=torch.float64, device="cuda")
            blk.base[i], blk.stride[i] = out[names[i]].data_ptr(), n + pad
    per = 5 * nzc + 3 * nv + sum(var_lens)
    work = torch.full((B * per + 4,), NAN, dtype=torch.float64, device="cuda")
    status = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    rc = lib.fbstab_hip_mpc_condensed_tangent_batch(
        handle, N, nx, nu, nc, B if batch is None else batch, C.byref(data), C.byref(dense), C.byref(xb),
        C.byref(dirb), C.c_double(sigma), C.byref(ob), C.byref(rb) if rhs else None, C.c_void_p(work.data_ptr()),
        C.c_void_p(status.data_ptr()), None)
    torch.cuda.synchronize()
    res = {k: t.cpu().numpy() for k, t in out.items()}
    w = work.cpu().numpy()
    res["work_tail"] = w[B * per:]
    res["work_seeds"] = w[B * (5 * nzc + 3 * nv):B * per]
    res["status"] = status.cpu().numpy()
    res["rc"] = rc
    res["msg"] = lib.fbstab_hip_last_error().decode()
    return res


def directions(p, seed, names=None, shared=()):
    """Random directions for the batch of ``p`` (tangent_helpers.random_directions), dQ and dR NOT symmetric."""
    return TH.random_directions(np.random.default_rng(seed), p, p.arrays["x0"].shape[0], names, shared)
