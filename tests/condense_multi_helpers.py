"""TEST INFRASTRUCTURE ONLY: what tests/test_condense_multi_cpu.py and tests/test_gpu_condense_multi.py share - the
documented formulas of fbstab_hip_mpc_condensed_multi_sizes, the explicit unit seeds of the x0 mode, the MPC system
in longdouble, and the host build of the kernels' maps (tests/hostsim/condense_multi.cc).  The rounding rules, the
pseudo-data problem and the longdouble chain are those of tests/condense_adjoint_helpers.py."""
import ctypes as C

import numpy as np

from tests import condense_adjoint_helpers as cah
from tests import condense_helpers as ch
from tests import hostsim
from tests import linear_reference as lr

LD = ch.LD
MPC_NAMES = ch.MPC_NAMES


def _e(n):
    return n + (n & 1)


def sizes_formula(N, nx, nu, nc, nrhs, rhs_per_group=0):
    """include/fbstab_hip.h (fbstab_hip_mpc_condensed_multi_sizes), written out: dict rhs_per_group, lds_bytes,
    work_doubles_per_qp, and per and window."""
    n1 = N + 1
    per = max(_e(n1 * nx) + 2 * _e(nx), _e(n1 * (nx + nu)) + _e(n1 * nc) + 2 * _e(nx))
    ldx, ldc, ldu = nx | 1, nc | 1, nu | 1
    window = 2 * _e(ldx * nx) + _e(ldx * nu) + _e(ldc * nx) + _e(ldu * nx) + _e(ldc * nu) + _e(ldu * nu)
    if rhs_per_group > 0:
        R = min(rhs_per_group, nrhs)
    else:
        R = max(1, min(256 // nx, nrhs))
        while R > 1 and 8 * (window + R * per) > 80 * 1024:
            R -= 1
    return dict(rhs_per_group=R, lds_bytes=8 * (window + R * per),
                work_doubles_per_qp=n1 * nu + nrhs * (4 * n1 * nu + 3 * n1 * nc), per=per, window=window)


def x0_seeds(p):
    """The explicit seeds of the x0 mode, one QP's block: gz = 0 (nx, nz), gl = -e_j in the l_0 block (nx, nl),
    gv = 0 (nx, nv)."""
    gl = np.zeros((p.nx, p.nl))
    gl[np.arange(p.nx), np.arange(p.nx)] = -1.0
    return np.zeros((p.nx, p.nz)), gl, np.zeros((p.nx, p.nv))


def mpc_system(p, q, x, sigma=lr.SIGMA, alpha=0.95):
    """(V, C) of the MPC system V d = (gz, -gl, -C gv) at the point, in longdouble: the matrix of
    cah.mpc_solve_reference."""
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
    return V, Cg


class HostCondenseMulti:
    """condense_multi_seed / _finish / _residual / _correct of fb_condense_multi.h with Ctx<1>, one QP, the group
    loop of the grid included."""

    def __init__(self):
        self.lib = C.CDLL(hostsim.build("libhostsim_condense_multi.so", "condense_multi.cc",
                                        ("fb_common.h", "fb_batch.h", "fb_condense_plan.h", "fb_adjoint.h", "fb_condense.h",
                                         "fb_condense_adjoint.h", "fb_condense_multi.h")))
        L = self.lib
        L.hostsim_condense_multi_sizes.argtypes = [C.c_int] * 5 + [C.c_void_p]
        L.hostsim_condense_multi_sizes.restype = None
        L.hostsim_condense_multi_seed.argtypes = [C.c_int] * 4 + [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                                                  C.c_void_p] + [C.c_int] * 3 + [C.c_void_p] * 3
        L.hostsim_condense_multi_finish.argtypes = [C.c_int] * 4 + [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p] + [
            C.c_int] * 3 + [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.hostsim_condense_multi_residual.argtypes = [C.c_int] * 4 + [C.c_void_p, C.c_void_p, C.c_double] + [C.c_void_p] * 4
        L.hostsim_condense_multi_residual.restype = None
        L.hostsim_condense_multi_correct.argtypes = [C.c_int] * 5 + [C.c_void_p] * 5 + [C.c_int]
        L.hostsim_condense_multi_correct.restype = None

    def sizes(self, N, nx, nu, nc, nrhs):
        out = (C.c_longlong * 3)()
        self.lib.hostsim_condense_multi_sizes(N, nx, nu, nc, nrhs, out)
        return dict(per=out[0], window=out[1], rule=out[2])

    @staticmethod
    def _seeds(seeds, rhs_stride):
        """The pointer and stride tables of one QP's seeds ((K, n) arrays, None: a NULL slot; all None: x0 mode)."""
        keep = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in seeds]
        ptrs = (C.c_void_p * 3)(*[None if a is None else a.ctypes.data for a in keep])
        rs = (C.c_longlong * 3)(*[0 if a is None else (a.shape[1] if rhs_stride is None else rhs_stride)
                                  for a in keep])
        return keep, ptrs, rs

    def seed(self, p, q, z, seeds, nrhs, R, groups=-1, rhs_stride=None):
        """(U, gU (nrhs, nzc), gv_c (nrhs, nv)) of QP ``q``; ``seeds`` = (gz, gl, gv) of shape (nrhs, n) each (gl, gv
        may be None), or None for the x0 mode.  Outputs are pre-filled with NaN."""
        data_keep, data = cah.HostCondenseAdjoint._data(p, q)
        nzc = (p.N + 1) * p.nu
        x0 = seeds is None
        keep, ptrs, rs = self._seeds((None, None, None) if x0 else seeds, rhs_stride)
        z = np.ascontiguousarray(z, dtype=np.float64)
        U, gU, gvc = np.full(nzc, np.nan), np.full((nrhs, nzc), np.nan), np.full((nrhs, p.nv), np.nan)
        self.lib.hostsim_condense_multi_seed(*p.sizes(), data, z.ctypes.data, 1 if x0 else 0, ptrs, rs, nrhs, R,
                                             groups, U.ctypes.data, gU.ctypes.data, gvc.ctypes.data)
        return U, gU, gvc

    def finish(self, p, q, seeds, dU, dv, R, groups=-1, ok=True, want=("dz", "dl", "dv")):
        """dict dz (nrhs, nz), dl, dv of QP ``q`` from the dense step's dU (nrhs, nzc), dv (nrhs, nv); slots not in
        ``want`` are NULL.  Outputs are pre-filled with NaN."""
        data_keep, data = cah.HostCondenseAdjoint._data(p, q)
        x0 = seeds is None
        keep, ptrs, rs = self._seeds((None, None, None) if x0 else seeds, None)
        dU, dv = (np.ascontiguousarray(a, dtype=np.float64) for a in (dU, dv))
        nrhs = dU.shape[0]
        out = {k: np.full((nrhs, n), np.nan) for k, n in zip(("dz", "dl", "dv"), (p.nz, p.nl, p.nv)) if k in want}
        sp = (C.c_void_p * 3)(*[out[k].ctypes.data if k in out else None for k in ("dz", "dl", "dv")])
        srs = (C.c_longlong * 3)(p.nz, p.nl, p.nv)
        self.lib.hostsim_condense_multi_finish(*p.sizes(), data, 1 if x0 else 0, ptrs, rs, nrhs, R, groups,
                                               dU.ctypes.data, dv.ctypes.data, 1 if ok else 0, sp, srs)
        return out

    def residual(self, Hc, Ac, sigma, gU, dU, dv, R):
        """rU (nrhs, nzc); ``Hc`` (nzc, nzc) and ``Ac`` (nv, nzc) as matrices."""
        Hc, Ac = (np.asfortranarray(m, dtype=np.float64) for m in (Hc, Ac))
        gU, dU, dv = (np.ascontiguousarray(a, dtype=np.float64) for a in (gU, dU, dv))
        rU = np.full(gU.shape, np.nan)
        self.lib.hostsim_condense_multi_residual(gU.shape[1], dv.shape[1], gU.shape[0], R, Hc.ctypes.data,
                                                 Ac.ctypes.data, sigma, gU.ctypes.data, dU.ctypes.data, dv.ctypes.data,
                                                 rU.ctypes.data)
        return rU

    def correct(self, eU, ev, dU, dv, R, nu, gain=False, ok=True):
        """(dU + eU, dv + ev, gain (nrhs, nu) or None)."""
        eU, ev = (np.ascontiguousarray(a, dtype=np.float64) for a in (eU, ev))
        dU, dv = (np.array(a, dtype=np.float64) for a in (dU, dv))
        g = np.full((dU.shape[0], nu), np.nan) if gain else None
        self.lib.hostsim_condense_multi_correct(dU.shape[1], dv.shape[1], nu, dU.shape[0], R, eU.ctypes.data,
                                                ev.ctypes.data, dU.ctypes.data, dv.ctypes.data,
                                                None if g is None else g.ctypes.data, 1 if ok else 0)
        return dU, dv, g


def slot_problem(p, q, seeds, k):
    """The pseudo-data problem (one QP) of right-hand side ``k`` of QP ``q``: ``seeds`` = (gz, gl, gv) of shape
    (nrhs, n), None is zero."""
    one = lr.one_qp(p, q)
    gz, gl, gv = seeds
    return cah.pseudo_problem(one, gz[k][None], None if gl is None else gl[k][None], None if gv is None else gv[k][None])
