"""TEST INFRASTRUCTURE ONLY: what tests/test_condense_adjoint_cpu.py and tests/test_gpu_condense_adjoint.py share -
the pseudo-data problem whose condensing maps are the adjoint's (fb_condense_adjoint.h), the chain seed -> dense
solve -> finish in extended precision, and the host build of the two kernels (tests/hostsim/condense_adjoint.cc)."""
import ctypes as C

import numpy as np

from tests import condense_helpers as ch
from tests import hostsim
from tests import linear_reference as lr
from tools import fixtures as fx

LD = ch.LD
MPC_NAMES = ch.MPC_NAMES
SIGMA = lr.SIGMA


def pseudo_problem(p, gz, gl, gv):
    """The problem with ``p``'s matrices and the vectors q := -gz_x, r := -gz_u, x0 := -gl_0, c := -gl_(i+1),
    d := -gv: its optimality system is the adjoint's.  Seeds are (batch, n) arrays; None is zero."""
    N, nx, nu, nc = p.sizes()
    B = p.batch
    gz = np.asarray(gz, dtype=np.float64).reshape(B, N + 1, nx + nu)
    gl = np.zeros((B, p.nl)) if gl is None else np.asarray(gl, dtype=np.float64)
    gv = np.zeros((B, p.nv)) if gv is None else np.asarray(gv, dtype=np.float64)
    arrays = {k: a.copy() for k, a in p.arrays.items()}
    arrays["q"] = np.ascontiguousarray(-gz[:, :, :nx]).reshape(B, -1)
    arrays["r"] = np.ascontiguousarray(-gz[:, :, nx:]).reshape(B, -1)
    arrays["x0"] = np.ascontiguousarray(-gl[:, :nx])
    arrays["c"] = np.ascontiguousarray(-gl[:, nx:])
    arrays["d"] = np.ascontiguousarray(-gv)
    return fx.MpcProblem(N, nx, nu, nc, arrays)


def seed_reference(pp, q):
    """(gU, gv_c) of QP ``q`` from the pseudo-data problem ``pp`` in longdouble, with the rule's bounds: the images
    ``f`` = -gU and ``b`` = gv_c of condense_reference and condense_bound."""
    ref, bound = ch.condense_reference(pp, q), ch.condense_bound(pp, q)
    return {k: ref[k] for k in ("f", "b")}, {k: bound[k] for k in ("f", "b")}


def dense_system(p, q, x, Hc, Ac, sigma=SIGMA, alpha=0.95):
    """V_c = [H_c + sigma I, A_c'; -C A_c, mus] of the condensed QP at the point, in longdouble (C and mus are those
    of the MPC QP: y_c = y and v_c = v entry for entry)."""
    Cg, mus = lr.fb_derivatives(p, q, x, sigma, alpha)
    nzc = Hc.shape[0]
    top = np.concatenate([Hc + LD(sigma) * np.eye(nzc, dtype=LD), Ac.T], axis=1)
    bot = np.concatenate([-Cg[:, None] * Ac, np.diag(mus)], axis=1)
    return np.concatenate([top, bot], axis=0), Cg


def solve_refined(V, r, sweeps=3):
    """V s = r: numpy's double solve, refined with longdouble residuals."""
    V64 = V.astype(np.float64)
    s = np.linalg.solve(V64, r.astype(np.float64)).astype(LD)
    for _ in range(sweeps):
        s = s + np.linalg.solve(V64, (r - V @ s).astype(np.float64)).astype(LD)
    return s


def chain_reference(p, q, x, seeds, sigma=SIGMA, alpha=0.95):
    """The adjoint step of the condensed route in longdouble: dict gU, gvc, dU and dz, dl, dv.  ``x`` and ``seeds``:
    the vectors of QP ``q``."""
    gz, gl, gv = seeds
    one = lr.one_qp(p, q)
    pp = pseudo_problem(one, gz[None], None if gl is None else gl[None], None if gv is None else gv[None])
    img = ch.condense_reference(pp, 0)
    gU, gvc = -img["f"], img["b"]
    V, Cg = dense_system(p, q, x, img["H"], img["A"], sigma, alpha)
    nzc = len(gU)
    s = solve_refined(V, np.concatenate([gU, -Cg * gvc]))
    dU, dv = s[:nzc], s[nzc:]
    dz, dl, _, _ = ch.expand_reference(pp, 0, dU, dv, dv)
    return dict(gU=gU, gvc=gvc, dU=dU, dz=dz, dl=dl, dv=dv, pseudo=pp)


def mpc_solve_reference(p, q, x, seeds, sigma=SIGMA, alpha=0.95):
    """(dz, dl, dv) of the MPC system V d = (gz, -gl, -C gv) itself, in longdouble (the flat-vector adjoint's step up
    to its rounding): what the chain differs from by the pure sigma bias."""
    Hm, _, G, _, A, _ = (np.asarray(m).astype(LD) for m in lr.explicit(p, q))
    Cg, mus = lr.fb_derivatives(p, q, x, sigma, alpha)
    nz, nl, nv = p.nz, p.nl, p.nv
    sig = LD(sigma)
    V = np.zeros((nz + nl + nv,) * 2, dtype=LD)
    V[:nz, :nz] = Hm + sig * np.eye(nz, dtype=LD)
    V[:nz, nz:nz + nl] = G.T
    V[:nz, nz + nl:] = A.T
    V[nz:nz + nl, :nz] = -G
    V[nz:nz + nl, nz:nz + nl] = sig * np.eye(nl, dtype=LD)
    V[nz + nl:, :nz] = -Cg[:, None] * A
    V[nz + nl:, nz + nl:] = np.diag(mus)
    gz, gl, gv = (np.asarray(t).astype(LD) for t in seeds)
    s = solve_refined(V, np.concatenate([gz, -gl, -Cg * gv]), sweeps=5)
    return s[:nz], s[nz:nz + nl], s[nz + nl:]


def sigma_gap(p, q, x, seeds, sigma=SIGMA):
    """max |chain - MPC solve| over (dz, dl, dv), and max |MPC solve|: the bias of the condensed regularisation."""
    c = chain_reference(p, q, x, seeds, sigma)
    m = mpc_solve_reference(p, q, x, seeds, sigma)
    gap = max(float(np.abs(c[k] - r).max()) for k, r in zip(("dz", "dl", "dv"), m))
    return gap, max(float(np.abs(r).max()) for r in m)


# ---- the device logic on one host thread -----------------------------------------------------------------------
class HostCondenseAdjoint:
    """condense_adjoint_seed / condense_adjoint_finish of fb_condense_adjoint.h with Ctx<1>."""

    def __init__(self):
        self.lib = C.CDLL(hostsim.build("libhostsim_condense_adjoint.so", "condense_adjoint.cc",
                                        ("fb_common.h", "fb_batch.h", "fb_condense_plan.h", "fb_adjoint.h", "fb_condense.h",
                                         "fb_condense_adjoint.h")))
        self.lib.hostsim_condense_adjoint_seed.argtypes = [C.c_int] * 4 + [C.c_void_p] * 8
        self.lib.hostsim_condense_adjoint_finish.argtypes = [C.c_int] * 4 + [C.c_void_p] * 9 + [C.c_int] + [C.c_void_p] * 3

    @staticmethod
    def _data(p, q):
        keep = [np.ascontiguousarray(p.arrays[k][q], dtype=np.float64) for k in MPC_NAMES]
        return keep, (C.c_void_p * 12)(*[a.ctypes.data for a in keep])

    @staticmethod
    def _vec(a):
        return None if a is None else np.ascontiguousarray(a, dtype=np.float64)

    def seed(self, p, q, z, gz, gl=None, gv=None):
        """(U, gU, gv_c) of QP ``q``."""
        keep, data = self._data(p, q)
        nzc = (p.N + 1) * p.nu
        z, gz, gl, gv = (self._vec(a) for a in (z, gz, gl, gv))
        U, gU, gvc = np.full(nzc, np.nan), np.full(nzc, np.nan), np.full(p.nv, np.nan)
        ptr = lambda a: None if a is None else a.ctypes.data
        self.lib.hostsim_condense_adjoint_seed(*p.sizes(), data, ptr(z), ptr(gz), ptr(gl), ptr(gv), ptr(U), ptr(gU),
                                               ptr(gvc))
        return U, gU, gvc

    def residual(self, Hc, Ac, sigma, gU, dU, dv):
        """rU = gU - (H_c dU + sigma dU + A_c' dv) of one QP; ``Hc`` (nzc, nzc) and ``Ac`` (nv, nzc) as matrices."""
        Hc, Ac = (np.asfortranarray(m, dtype=np.float64) for m in (Hc, Ac))
        gU, dU, dv = (self._vec(a) for a in (gU, dU, dv))
        rU = np.full(len(gU), np.nan)
        f = self.lib.hostsim_condense_adjoint_residual
        f.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_double] + [C.c_void_p] * 4
        f.restype = None
        f(len(gU), len(dv), Hc.ctypes.data, Ac.ctypes.data, sigma, gU.ctypes.data, dU.ctypes.data, dv.ctypes.data,
          rU.ctypes.data)
        return rU

    def correct(self, eU, ev, dU, dv):
        """(dU + eU, dv + ev) of one QP."""
        eU, ev = (self._vec(a) for a in (eU, ev))
        dU, dv = (np.array(a, dtype=np.float64) for a in (dU, dv))
        f = self.lib.hostsim_condense_adjoint_correct
        f.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 4
        f.restype = None
        f(len(dU), len(dv), eU.ctypes.data, ev.ctypes.data, dU.ctypes.data, dv.ctypes.data)
        return dU, dv

    def finish(self, p, q, x, gz, gl, dU, dv, want=None, ok=True):
        """(gradients of ``want`` - default all 12 -, (dz, dl, dv)) of QP ``q`` from the dense adjoint's (dU, dv)."""
        keep, data = self._data(p, q)
        lens = p.seq_lengths()
        z, l, v = (self._vec(a) for a in x)
        gz, gl, dU, dv = (self._vec(a) for a in (gz, gl, dU, dv))
        grads = {k: np.full(lens[k], np.nan) for k in (MPC_NAMES if want is None else want)}
        gptr = (C.c_void_p * 12)(*[grads[k].ctypes.data if k in grads else None for k in MPC_NAMES])
        adj = [np.full(n, np.nan) for n in (p.nz, p.nl, p.nv)]
        ptr = lambda a: None if a is None else a.ctypes.data
        self.lib.hostsim_condense_adjoint_finish(*p.sizes(), data, ptr(z), ptr(l), ptr(v), ptr(gz), ptr(gl), ptr(dU),
                                                 ptr(dv), gptr, 1 if ok else 0, *(a.ctypes.data for a in adj))
        return grads, tuple(adj)


def finish_violations(got_dz, got_dl, pp, q, dU, dv):
    """Names of (dz, dl) that miss the expand rule on the pseudo-data problem somewhere."""
    zr, lr_, _, _ = ch.expand_reference(pp, q, dU, dv, dv)
    zb, lb = ch.expand_bound(pp, q, dU, dv, dv)
    bad = []
    if not (np.abs(np.asarray(got_dz).astype(LD) - zr) <= zb).all():
        bad.append("dz")
    if not (np.abs(np.asarray(got_dl).astype(LD) - lr_) <= lb).all():
        bad.append("dl")
    return bad


def seed_violations(gU, gvc, pp, q):
    """Names of (gU, gv_c) that miss the condense rule on the pseudo-data problem somewhere."""
    ref, bound = seed_reference(pp, q)
    got = dict(f=-np.asarray(gU), b=np.asarray(gvc))
    return ch.rule_violations(got, ref, bound, names=("f", "b"))
