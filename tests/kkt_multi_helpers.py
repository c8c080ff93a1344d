"""TEST INFRASTRUCTURE ONLY: what the CPU and the GPU tests of the many-right-hand-side solves
(fbstab_hip_mpc_kkt_solve_batch, fbstab_hip_mpc_x0_sensitivity_batch) share - the single-threaded host compilation of
fb_kkt_multi.h (tests/hostsim/kkt_multi.cc) and its ctypes wrapper, random seed blocks, and the handle-free calls of
the two entry points."""
import ctypes as C

import numpy as np

from fbstab_amd.hip_api import MPC_SEQ
from tests.hostsim import build
from tests.linear_reference import SIGMA

STEP = ("dz", "dl", "dv")


class HostKktMulti:
    """mpc_kkt_multi of fb_kkt_multi.h for one QP on one host thread."""

    def __init__(self):
        self.lib = C.CDLL(build("libhostsim_kkt_multi.so", "kkt_multi.cc",
                                ("fb_common.h", "fb_batch.h", "fb_adjoint.h", "fb_mpc.h", "fb_kkt_multi.h")))
        self.lib.hostsim_mpc_kkt_multi.argtypes = ([C.c_int] * 4 + [C.c_void_p] * 4 + [C.c_int] * 2 + [C.c_void_p] * 3 +
                                                   [C.c_double] * 2 + [C.c_void_p] * 4)

    def _run(self, p, q, x, nrhs, x0_mode, seeds, want, gain, sigma, alpha):
        keep = [np.ascontiguousarray(p.arrays[k][q], dtype=np.float64) for k in MPC_SEQ]
        data = (C.c_void_p * 12)(*[a.ctypes.data for a in keep])
        f64 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
        ptr = lambda a: None if a is None else a.ctypes.data
        z, l, v = (f64(t) for t in x)
        gz, gl, gv = (f64(t) for t in seeds)
        out = {k: (np.full((nrhs, n), np.nan) if k in want else None) for k, n in zip(STEP, (p.nz, p.nl, p.nv))}
        g = np.full((p.nx, p.nu), np.nan) if gain else None   # (column-major nu x nx)
        st = self.lib.hostsim_mpc_kkt_multi(*p.sizes(), data, ptr(z), ptr(l), ptr(v), nrhs, int(x0_mode), ptr(gz),
                                            ptr(gl), ptr(gv), sigma, alpha, ptr(out["dz"]), ptr(out["dl"]),
                                            ptr(out["dv"]), ptr(g))
        res = {k: a for k, a in out.items() if a is not None}
        res["status"] = st
        if gain:
            res["gain"] = g.T.copy()
        return res

    def solve(self, p, q, x, gz, gl=None, gv=None, sigma=SIGMA, alpha=0.95, want=STEP):
        """QP ``q`` at x = (z, l, v) for the seeds ``gz`` (nrhs, nz), ``gl``, ``gv`` (None: zero): dict with
        ``dz (nrhs, nz)``, ``dl``, ``dv`` and ``status``."""
        return self._run(p, q, x, gz.shape[0], False, (gz, gl, gv), want, False, sigma, alpha)

    def x0_sensitivity(self, p, q, x, sigma=SIGMA, alpha=0.95, want=STEP):
        """The x0 mode: ``dz (nx, nz)``, ``dl``, ``dv``, ``gain (nu, nx)`` and ``status``."""
        return self._run(p, q, x, p.nx, True, (None, None, None), want, True, sigma, alpha)


def random_seed_block(rng, p, nrhs, batch=None):
    """(gz, gl, gv), each ``(batch, nrhs, n)`` (``batch`` None: ``(nrhs, n)``)."""
    lead = (nrhs,) if batch is None else (batch, nrhs)
    return tuple(rng.standard_normal(lead + (n,)) for n in (p.nz, p.nl, p.nv))


def x0_seed_block(p):
    """The seeds of the x0 mode, spelled out: gz = 0, gl = -e_j in the l_0 block, gv = 0, j < nx."""
    gl = np.zeros((p.nx, p.nl))
    gl[np.arange(p.nx), np.arange(p.nx)] = -1.0
    return np.zeros((p.nx, p.nz)), gl, np.zeros((p.nx, p.nv))


def kkt_solve_into(s, data, x, seeds, steps, batch=None):
    """fbstab_hip_mpc_kkt_solve_batch of the solver ``s`` on host arrays as they lie in memory: ``seeds`` and ``steps``
    are (B, K, n) numpy arrays or views (their strides become stride / rhs_stride; ``(K, n)``: shared; None: a NULL
    slot), the steps written in place.  Returns (rc, status)."""
    from fbstab_amd import hip_api
    rows = x[0].shape[0]   # (``batch``: what the call is told, 0 for an empty batch over the same blocks)
    B = rows if batch is None else batch
    K = seeds[0].shape[-2]
    lens = (s.nz, s.nl, s.nv)
    db = hip_api._MpcBatch()
    hip_api._fill_block(db, hip_api.MPC_SEQ, s.seq_len, data, rows, [])
    xb = hip_api._fill_vars(x, lens, None, [])
    sb = hip_api._fill_multi(seeds, lens, rows, K, [], optional=True)
    ob = hip_api._fill_multi(steps, lens, rows, K, [], optional=True, first_required=False)
    status = np.full(rows, -1, dtype=np.int32)
    rc = s._lib.fbstab_hip_mpc_kkt_solve_batch(s._h, B, C.byref(db), C.byref(xb), K, C.byref(sb), 0.0, C.byref(ob),
                                               status.ctypes.data, 0, None)
    return rc, status[:B]


def handle_free_kkt_solve(lib, batch=1, nrhs=2, null=(), seed_z=True, seed=None, step=None):
    """``(rc, message)`` of fbstab_hip_mpc_kkt_solve_batch with a NULL handle and otherwise valid host arguments
    (every slot a buffer, stride 64, rhs_stride 8) except as the case says: ``null`` names blocks passed as NULL,
    ``seed`` / ``step`` are (stride, rhs_stride) for every slot of that block."""
    from fbstab_amd import hip_api
    buf = np.zeros(256)
    status = np.zeros(4, dtype=np.int32)
    data, x = hip_api._MpcBatch(), hip_api._VarBatch()
    for i in range(12):
        data.base[i], data.stride[i] = buf.ctypes.data, 8
    for i in range(4):
        x.base[i], x.stride[i] = buf.ctypes.data, 8

    def multi(strides):
        b = hip_api._MultiVarBatch()
        for i in range(3):
            b.base[i] = buf.ctypes.data
            b.stride[i], b.rhs_stride[i] = strides or (64, 8)
        return b

    blocks = dict(data=data, x=x, seed=multi(seed), step=multi(step))
    if not seed_z:
        blocks["seed"].base[0] = None
    ref = lambda name: None if name in null else C.byref(blocks[name])
    rc = lib.fbstab_hip_mpc_kkt_solve_batch(None, batch, ref("data"), ref("x"), nrhs, ref("seed"), 0.0, ref("step"),
                                            None if "status" in null else status.ctypes.data, 0, None)
    return rc, lib.fbstab_hip_last_error().decode()
