"""CPU-only checks of the sweep adjoint (fbstab_hip_mpc_receding_sweep_logged / _receding_sweep_adjoint): the
exports and the argument validation of the C-ABI without a GPU, and the yardstick of the GPU tests -
tests/sweep_adjoint_helpers.reference_sweep_adjoint - against central differences of the oracle's closed loop."""
import ctypes as C

import numpy as np

from oracle.oracle_py import default_options
from tests import closed_loop as CL
from tests import sweep_adjoint_helpers as SH
from tools import fixtures as fx


def _call(lib, hip_api, log="ok", steps=2, batch=2, zero_stride=None):
    """rc and message of fbstab_hip_mpc_receding_sweep_adjoint with a NULL handle and otherwise valid host
    arguments, except as the case says."""
    buf = np.zeros(64)
    ints = np.zeros(8, dtype=np.int32)
    b, g = hip_api._MpcBatch(), hip_api._MpcGradBatch()
    for i in range(12):
        b.base[i], b.stride[i] = buf.ctypes.data, 8
        g.base[i], g.stride[i] = buf.ctypes.data, 8
    if zero_stride is not None:
        g.stride[zero_stride] = 0
    plant = hip_api._Plant(buf.ctypes.data, buf.ctypes.data, 0, 0)
    lg = hip_api._SweepLog(buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, ints.ctypes.data)
    if log == "no z":
        lg.z = None
    if log == "no eflag":
        lg.eflag = None
    rc = lib.fbstab_hip_mpc_receding_sweep_adjoint(
        None, batch, C.byref(b), C.byref(plant), steps, 1, None if log is None else C.byref(lg), buf.ctypes.data,
        buf.ctypes.data, C.c_double(0.0), C.byref(g), None, ints.ctypes.data, None)
    return rc, lib.fbstab_hip_last_error().decode()


def test_sweep_adjoint_entry_points_are_exported_and_validate_without_gpu():
    from fbstab_amd import hip_api
    lib = hip_api.load_library()
    for sym in ("fbstab_hip_mpc_receding_sweep_logged", "fbstab_hip_mpc_receding_sweep_adjoint",
                "fbstab_hip_mpc_sweep_adjoint_kernel_name"):
        assert sym in hip_api.EXPORTED_SYMBOLS
        getattr(lib, sym)
    assert C.sizeof(hip_api._SweepLog) == 5 * 8
    ARG = 1  # FBSTAB_HIP_ERR_ARGUMENT
    rc, msg = _call(lib, hip_api, log=None)
    assert rc == ARG and "null log" in msg
    for case in ("no z", "no eflag"):
        rc, msg = _call(lib, hip_api, log=case)
        assert rc == ARG and "z, l, v and eflag are required" in msg, case
    rc, msg = _call(lib, hip_api, steps=-1)
    assert rc == ARG and "negative step count" in msg
    rc, msg = _call(lib, hip_api, zero_stride=3)
    assert rc == ARG and "stride 0" in msg
    # one trajectory: the stride is not looked at, and an otherwise valid call gets as far as the handle
    rc, msg = _call(lib, hip_api, batch=1, zero_stride=3)
    assert rc == ARG and "null solver handle" in msg
    rc, msg = _call(lib, hip_api)
    assert rc == ARG and "null solver handle" in msg
    # the logged sweep is the sweep: the same first answer
    assert lib.fbstab_hip_mpc_receding_sweep_logged(None, 1, None, None, None, None, 1, 1, None, None, None, None,
                                                    None) == ARG
    assert b"null solver handle" in lib.fbstab_hip_last_error()
    assert lib.fbstab_hip_mpc_sweep_adjoint_kernel_name(None) == b""


def test_reference_recursion_against_central_differences_of_the_oracles_closed_loop(oracle):
    """Shape (6, 4, 2, 6), 8 trajectories x 3 steps at abs_tol = 1e-11: central differences (h = 1e-5) of a random
    linear loss in (u, x) through tests/closed_loop.py run with the oracle, along random directions of q, r, d, x0
    and a symmetric direction of Q, against reference_sweep_adjoint with the oracle's adjoint, under
    |fd - ad| <= 1e-4 max(|ad|, 1e-2 sum|grad|), on the trajectories strictly complementary at 1e-3 at every
    step (at least 3 of the 8)."""
    p, A, B, cu, cx, dirs = SH.fd_problem()
    N, nx, nu, nc = p.sizes()
    o = default_options(abs_tol=1e-11)
    log = CL.logged_closed_loop(CL.oracle_solve(oracle, p, o), p, A, B, SH.FD_STEPS)
    good = SH.strictly_complementary(p, log)
    assert len(good) >= 3, good
    grads, status, mu = SH.reference_sweep_adjoint(SH.oracle_step_adjoint(oracle, p), p, A, B, log, cu, cx)
    assert (status == 0).all()

    def run(prob):
        def solve(x0, z, l, v):
            arr = dict(prob.arrays)
            arr["x0"] = x0
            return oracle.solve_mpc(fx.MpcProblem(N, nx, nu, nc, arr), x0guess=(z, l, v), opts=o)
        z, l, v = np.zeros((prob.batch, prob.nz)), np.zeros((prob.batch, prob.nl)), np.zeros((prob.batch, prob.nv))
        rec = CL.closed_loop(solve, prob.arrays["x0"].copy(), z, l, v, A, B, nx, nu, SH.FD_STEPS)
        u = np.stack([r["u0"] for r in rec])
        x = np.stack([r["x0"] for r in rec[1:]] + [rec[-1]["x0"] @ A.T + rec[-1]["u0"] @ B.T])
        return u, x

    u, x = run(p)
    assert np.array_equal(u[:, good], log["u"][:, good]) and np.array_equal(x[-1][good], log["x_end"][good])
    figures = SH.fd_check(run, grads, good, p, cu, cx, dirs)
    for name, q, fd, ad, bound in figures:
        print(f"{name:3s} q {q} fd {fd:+.9e} ad {ad:+.9e} |fd-ad| {abs(fd - ad):.2e} bound {bound:.2e}")
    for name, q, fd, ad, bound in figures:
        assert abs(fd - ad) <= bound, (name, q, fd, ad, bound)
