"""TEST INFRASTRUCTURE ONLY: what the CPU and the GPU tests of the dense many-right-hand-side solves
(fbstab_hip_dense_kkt_solve_batch, fbstab_hip_dense_jacobian_batch) share - the single-threaded host compilation of
fb_dense_kkt_multi.h (tests/hostsim/dense_kkt_multi.cc) with its ctypes wrapper and its stand-alone sanitizer build,
random and unit seed blocks, and the handle-free calls of the two entry points."""
import ctypes as C
import os
import subprocess

import numpy as np

from fbstab_amd.hip_api import DENSE_ARR
from tests import hostsim
from tests.linear_reference import SIGMA

STEP = ("dz", "dl", "dv")
WRT = {"f": DENSE_ARR.index("f"), "h": DENSE_ARR.index("h"), "b": DENSE_ARR.index("b")}
HEADERS = ("fb_common.h", "fb_batch.h", "fb_adjoint.h", "fb_mpc.h", "fb_dense.h", "fb_dense_kkt_multi.h")


def _pad(a):
    return a if a.size else np.zeros(max(a.shape[0], 1))


class HostDenseKktMulti:
    """dense_kkt_multi of fb_dense_kkt_multi.h over DenseProblem<Ctx<1>> for one QP on one host thread."""

    def __init__(self):
        self.lib = C.CDLL(hostsim.build("libhostsim_dense_kkt_multi.so", "dense_kkt_multi.cc", HEADERS))
        self.lib.hostsim_dense_kkt_multi.argtypes = ([C.c_int] * 3 + [C.c_void_p] * 4 + [C.c_int] * 2 + [C.c_void_p] * 3 +
                                                     [C.c_double] * 2 + [C.c_void_p] * 3)

    def _run(self, p, q, x, nrhs, wrt, seeds, want, sigma, alpha):
        keep = [_pad(np.ascontiguousarray(p.arrays[k][q], dtype=np.float64)) for k in DENSE_ARR]
        data = (C.c_void_p * 6)(*[a.ctypes.data for a in keep])
        f64 = lambda a: None if a is None else _pad(np.ascontiguousarray(a, dtype=np.float64))
        ptr = lambda a: None if a is None else a.ctypes.data
        z, l, v = (f64(t) for t in x)
        gz, gl, gv = (f64(t) for t in seeds)
        out = {k: (np.full((nrhs, n), np.nan) if k in want else None) for k, n in zip(STEP, (p.nz, p.nl, p.nv))}
        bufs = {k: (None if a is None else _pad(a)) for k, a in out.items()}
        st = self.lib.hostsim_dense_kkt_multi(p.nz, p.nl, p.nv, data, ptr(z), ptr(l), ptr(v), nrhs, wrt, ptr(gz), ptr(gl),
                                              ptr(gv), sigma, alpha, ptr(bufs["dz"]), ptr(bufs["dl"]), ptr(bufs["dv"]))
        res = {k: a for k, a in out.items() if a is not None}
        res["status"] = st
        return res

    def solve(self, p, q, x, gz, gl=None, gv=None, sigma=SIGMA, alpha=0.95, want=STEP):
        """QP ``q`` at x = (z, l, v) for the seeds ``gz`` (nrhs, nz), ``gl``, ``gv`` (None: zero): dict with
        ``dz (nrhs, nz)``, ``dl``, ``dv`` and ``status``."""
        return self._run(p, q, x, gz.shape[0], -1, (gz, gl, gv), want, sigma, alpha)

    def jacobian(self, p, q, x, wrt, sigma=SIGMA, alpha=0.95, want=STEP):
        """The Jacobian mode of ``wrt`` ("f", "h", "b"): ``dz (nrhs, nz)``, ``dl``, ``dv`` and ``status``."""
        nrhs = {"f": p.nz, "h": p.nl, "b": p.nv}[wrt]
        return self._run(p, q, x, nrhs, WRT[wrt], (None, None, None), want, sigma, alpha)


def build_and_run_sanitized():
    """Builds tests/hostsim/dense_kkt_multi.cc as a stand-alone program (its own main: one small QP per layout) with
    the address and undefined-behaviour sanitizers and runs it once on the CPU.  Returns (exit status, output)."""
    here = os.path.dirname(os.path.abspath(hostsim.__file__))
    out_dir = os.path.join(here, "..", "_build")   # (kept out of git, like the other test artefacts)
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "dense_kkt_multi_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", hostsim.NO_CONTRACTION, "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-DDENSE_KKT_MULTI_MAIN", "-I" + os.path.join(here, "shim"),
                           "-Wno-attributes", "-Wno-unknown-pragmas", "-o", exe,
                           os.path.join(here, "dense_kkt_multi.cc")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    return r.returncode, r.stdout


def random_seed_block(rng, p, nrhs, batch=None):
    """(gz, gl, gv), each ``(batch, nrhs, n)`` (``batch`` None: ``(nrhs, n)``)."""
    lead = (nrhs,) if batch is None else (batch, nrhs)
    return tuple(rng.standard_normal(lead + (n,)) for n in (p.nz, p.nl, p.nv))


def unit_seed_block(p, wrt):
    """The seeds of the Jacobian mode, spelled out with the tangent's signs: gz = -e_k (f), gl = e_k (h),
    gv = e_k (b); every other entry +0."""
    n = {"f": p.nz, "h": p.nl, "b": p.nv}[wrt]
    gz, gl, gv = np.zeros((n, p.nz)), np.zeros((n, p.nl)), np.zeros((n, p.nv))
    k = np.arange(n)
    if wrt == "f":
        gz[k, k] = -1.0
    elif wrt == "h":
        gl[k, k] = 1.0
    else:
        gv[k, k] = 1.0
    return gz, gl, gv


def _blocks(s, data, x, rows):
    from fbstab_amd import hip_api
    lens = (s.nz, s.nl, s.nv)
    db = hip_api._DenseBatch()
    hip_api._fill_block(db, hip_api.DENSE_ARR, s.arr_len, data, rows, [])
    xb = hip_api._fill_vars(x, lens, None, [])
    return db, xb, lens


def _live(arrs, lens):
    return tuple(None if n == 0 else a for a, n in zip(arrs, lens))


def kkt_solve_into(s, data, x, seeds, steps, batch=None):
    """fbstab_hip_dense_kkt_solve_batch of the solver ``s`` on host arrays as they lie in memory: ``seeds`` and
    ``steps`` are (B, K, n) numpy arrays or views (their strides become stride / rhs_stride; ``(K, n)``: shared; None:
    a NULL slot), the steps written in place.  Returns (rc, status)."""
    from fbstab_amd import hip_api
    rows = x[0].shape[0]   # (``batch``: what the call is told, 0 for an empty batch over the same blocks)
    B = rows if batch is None else batch
    K = seeds[0].shape[-2]
    db, xb, lens = _blocks(s, data, x, rows)
    sb = hip_api._fill_multi(_live(seeds, lens), lens, rows, K, [], optional=True)
    ob = hip_api._fill_multi(_live(steps, lens), lens, rows, K, [], optional=True, first_required=False)
    status = np.full(rows, -1, dtype=np.int32)
    rc = s._lib.fbstab_hip_dense_kkt_solve_batch(s._h, B, C.byref(db), C.byref(xb), K, C.byref(sb), 0.0, C.byref(ob),
                                                 status.ctypes.data, 0, None)
    return rc, status[:B]


def jacobian_into(s, data, x, wrt, steps, batch=None):
    """fbstab_hip_dense_jacobian_batch the same way: ``wrt`` an int, ``steps`` written in place.  (rc, status)."""
    from fbstab_amd import hip_api
    rows = x[0].shape[0]
    B = rows if batch is None else batch
    K = next(a for a in steps if a is not None).shape[-2]
    db, xb, lens = _blocks(s, data, x, rows)
    ob = hip_api._fill_multi(_live(steps, lens), lens, rows, K, [], optional=True, first_required=False)
    status = np.full(rows, -1, dtype=np.int32)
    rc = s._lib.fbstab_hip_dense_jacobian_batch(s._h, B, C.byref(db), C.byref(xb), wrt, 0.0, C.byref(ob),
                                                status.ctypes.data, 0, None)
    return rc, status[:B]


def _handle_free_blocks(seed, step, seed_z):
    from fbstab_amd import hip_api
    buf = np.zeros(256)
    data, x = hip_api._DenseBatch(), hip_api._VarBatch()
    for i in range(6):
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
    return buf, blocks


def handle_free_kkt_solve(lib, batch=1, nrhs=2, null=(), seed_z=True, seed=None, step=None):
    """``(rc, message)`` of fbstab_hip_dense_kkt_solve_batch with a NULL handle and otherwise valid host arguments
    (every slot a buffer, stride 64, rhs_stride 8) except as the case says: ``null`` names blocks passed as NULL,
    ``seed`` / ``step`` are (stride, rhs_stride) for every slot of that block."""
    buf, blocks = _handle_free_blocks(seed, step, seed_z)
    status = np.zeros(4, dtype=np.int32)
    ref = lambda name: None if name in null else C.byref(blocks[name])
    rc = lib.fbstab_hip_dense_kkt_solve_batch(None, batch, ref("data"), ref("x"), nrhs, ref("seed"), 0.0, ref("step"),
                                              None if "status" in null else status.ctypes.data, 0, None)
    return rc, lib.fbstab_hip_last_error().decode()


def handle_free_jacobian(lib, wrt, batch=1, null=(), step=None):
    """... and of fbstab_hip_dense_jacobian_batch."""
    buf, blocks = _handle_free_blocks(None, step, True)
    status = np.zeros(4, dtype=np.int32)
    ref = lambda name: None if name in null else C.byref(blocks[name])
    rc = lib.fbstab_hip_dense_jacobian_batch(None, batch, ref("data"), ref("x"), wrt, 0.0, ref("step"),
                                             None if "status" in null else status.ctypes.data, 0, None)
    return rc, lib.fbstab_hip_last_error().decode()
