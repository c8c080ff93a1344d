"""What the many-right-hand-side calls and the closed-loop sweeps refuse only after they have looked at a handle
(fbstab_hip_mpc_kkt_solve_batch, _x0_sensitivity_batch, fbstab_hip_dense_kkt_solve_batch, _jacobian_batch,
fbstab_hip_mpc_receding_sweep[_logged | _scenario], fbstab_hip_mpc_receding_sweep_adjoint), on created handles: the
return code, the text of fbstab_hip_last_error, outputs filled with a canary left as they were, and a correct call
on the same handle behind the refusals.  Every call here is refused before any launch; the order of the checks and
the staging around the launches are tests/test_host_stage.py's, on the CPU."""
import ctypes as C

import numpy as np
import pytest

from tests.placement_helpers import CANARY
from tools import fixtures as fx

pytestmark = pytest.mark.gpu

ARG = 1   # FBSTAB_HIP_ERR_ARGUMENT
BATCH_TEXT = "batch exceeds the max_batch the handle was created with"
DATA_TEXT = "problem data stride smaller than the array length"
GRAD_TEXT = "gradient stride smaller than the array length"
X0_TEXT = "receding sweep: every trajectory needs its own x0 (stride >= nx)"
MAX_BATCH, B, STEPS = 3, 2, 2


@pytest.fixture(scope="module")
def hip():
    from fbstab_amd import hip_api
    assert hip_api.load_library().fbstab_hip_device_count() >= 1
    return hip_api


def _canaries(shape):
    return np.full(shape, CANARY, dtype=np.uint64).view(np.float64)


def _untouched(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else a
    return bool((np.ascontiguousarray(a).view(np.uint64) == CANARY).all())


def _refused(lib, rc, text):
    assert rc == ARG and lib.fbstab_hip_last_error().decode() == text, (rc, lib.fbstab_hip_last_error())


def _multi(hip, arrays, lens, K):
    """A step block over ``(B, K, len)`` arrays (None or length 0: a NULL slot)."""
    return hip._fill_multi(tuple(None if n == 0 else a for a, n in zip(arrays, lens)), lens, B, K, [], optional=True,
                           first_required=False)


# ---- MPC: (N, nx, nu, nc) = (2, 2, 1, 1), max_batch 3 -------------------------------------------------------------
@pytest.fixture(scope="module")
def mpc(hip):
    p = fx.random_ltv_mpc(np.random.default_rng(11), B, 2, 2, 1, 1)
    s = hip.FBstabMpcBatch(2, 2, 1, 1, max_batch=MAX_BATCH)
    z, l, v, y = (np.zeros((B, n)) for n in (p.nz, p.nl, p.nv, p.nv))
    out = s.Solve(p.arrays, z, l, v, y)
    assert (out["eflag"] == 0).all(), out["eflag"]
    yield s, p, (z, l, v)
    s.close()


def test_the_mpc_multi_solves_refuse_a_short_gain_stride_and_a_batch_beyond_the_handle(hip, mpc):
    s, p, (z, l, v) = mpc
    lib, lens = s._lib, (s.nz, s.nl, s.nv)
    blk = hip._MpcBatch()
    hip._fill_block(blk, hip.MPC_SEQ, s.seq_len, p.arrays, B, [])
    xb = hip._fill_vars((z, l, v), lens, B, [])
    gain, dz, status = _canaries((B, s.nx, s.nu)), _canaries((B, s.nx, s.nz)), np.full(MAX_BATCH + 1, -1, dtype=np.int32)
    ob = _multi(hip, (dz, None, None), lens, s.nx)

    def x0_sensitivity(batch, gain_stride):
        return lib.fbstab_hip_mpc_x0_sensitivity_batch(s._h, batch, C.byref(blk), C.byref(xb), C.c_double(0.0),
                                                       C.byref(ob), gain.ctypes.data, gain_stride, status.ctypes.data,
                                                       0, None)

    _refused(lib, x0_sensitivity(B, s.nu * s.nx - 1), "gain stride smaller than nu x nx")
    _refused(lib, x0_sensitivity(MAX_BATCH + 1, s.nu * s.nx), BATCH_TEXT)
    seeds = np.ones((B, 1, s.nz))
    sb = _multi(hip, (seeds, None, None), lens, 1)
    dz1 = _canaries((B, 1, s.nz))
    step = _multi(hip, (dz1, None, None), lens, 1)
    _refused(lib, lib.fbstab_hip_mpc_kkt_solve_batch(s._h, MAX_BATCH + 1, C.byref(blk), C.byref(xb), 1, C.byref(sb),
                                                     C.c_double(0.0), C.byref(step), status.ctypes.data, 0, None),
             BATCH_TEXT)
    assert _untouched(gain) and _untouched(dz) and _untouched(dz1) and (status == -1).all()
    # one QP is at the base: its gain stride is not read
    _check = lambda rc: hip._check(lib, rc)
    _check(x0_sensitivity(1, 0))
    assert status[0] == 0 and not _untouched(gain[0]) and _untouched(gain[1])
    res = s.X0Sensitivity(p.arrays, z, l, v)
    assert (res["status"] == 0).all() and np.isfinite(res["dz"]).all() and np.isfinite(res["gain"]).all()
    assert np.array_equal(res["gain"][0], gain[0].T)


def _sweep_state(p):
    import torch
    dev = torch.device("cuda:0")
    data = {k: torch.from_numpy(np.ascontiguousarray(a)).to(dev) for k, a in p.arrays.items()}
    X = [torch.from_numpy(_canaries((B, n)).copy()).to(dev) for n in (p.nz, p.nl, p.nv, p.nv)]
    return dev, data, X


def test_the_sweeps_refuse_a_shared_x0_a_shift_of_two_and_a_batch_beyond_the_handle(hip, mpc):
    import torch
    s, p, _ = mpc
    lib = s._lib
    dev, data, X = _sweep_state(p)
    blk, flags = hip._MpcBatch(), []
    hip._fill_block(blk, hip.MPC_SEQ, s.seq_len, data, B, flags)
    vb = hip._fill_vars(tuple(X), (s.nz, s.nl, s.nv, s.nv), B, flags)
    assert all(flags)
    A, Bp = np.eye(2), np.array([[0.0], [0.1]])
    plant, keep = s._plant(A, Bp, dev)
    out = torch.full((MAX_BATCH + 1, 40), 0xA5, dtype=torch.uint8, device=dev)
    u_log = torch.from_numpy(_canaries((STEPS, B, s.nu)).copy()).to(dev)
    logs = [torch.from_numpy(_canaries((STEPS, B, n)).copy()).to(dev) for n in (s.nz, s.nl, s.nv, s.nx)]
    eflags = torch.full((STEPS, B), -7, dtype=torch.int32, device=dev)
    lg = hip._SweepLog(*[t.data_ptr() for t in logs], eflags.data_ptr())
    sc = hip._SweepScenario(None, 0)

    def sweeps(batch):
        head = (s._h, batch, C.byref(blk), C.byref(vb), out.data_ptr(), C.byref(plant), STEPS, 1, u_log.data_ptr(),
                None, None, None)
        return (lambda: lib.fbstab_hip_mpc_receding_sweep(*head),
                lambda: lib.fbstab_hip_mpc_receding_sweep_logged(*head, C.byref(lg)),
                lambda: lib.fbstab_hip_mpc_receding_sweep_scenario(*head, C.byref(lg), C.byref(sc)))

    x0_slot = hip.MPC_SEQ.index("x0")
    own = blk.stride[x0_slot]
    blk.stride[x0_slot] = 0
    for call in sweeps(B):
        _refused(lib, call(), X0_TEXT)
    blk.stride[x0_slot] = own
    for call in sweeps(MAX_BATCH + 1):
        _refused(lib, call(), BATCH_TEXT)
    sc.shift = 2
    _refused(lib, sweeps(B)[2](), "receding sweep scenario: shift is 0 or 1")
    torch.cuda.synchronize()
    assert all(_untouched(t) for t in X + logs + [u_log]) and (out == 0xA5).all() and (eflags == -7).all()
    assert np.array_equal(data["x0"].cpu().numpy(), p.arrays["x0"])
    # ... and the same handle runs the sweep, logged, with a shift
    X = [torch.zeros_like(t) for t in X]
    r = s.RecedingSweep(data, *X, A, Bp, STEPS, log_inputs=True, log=True, shift=True)
    assert (r["stats"]["newton_sum"] > 0).all() and not any(_untouched(t) for t in X)


def test_the_sweep_adjoint_refuses_summed_and_short_gradient_slots_short_data_and_a_batch_beyond_the_handle(hip, mpc):
    import torch
    s, p, _ = mpc
    lib = s._lib
    dev, data, X = _sweep_state(p)
    A, Bp = np.eye(2), np.array([[0.0], [0.1]])
    r = s.RecedingSweep(data, *[torch.zeros_like(t) for t in X], A, Bp, STEPS, log_inputs=True, log=True)
    data = {k: torch.from_numpy(np.ascontiguousarray(a)).to(dev) for k, a in p.arrays.items()}   # (x0 as it was)
    blk, flags = hip._MpcBatch(), []
    hip._fill_block(blk, hip.MPC_SEQ, s.seq_len, data, B, flags)
    grads = {k: torch.from_numpy(_canaries((B, n)).copy()).to(dev) for k, n in zip(hip.MPC_SEQ, s.seq_len)}
    gb = hip._MpcGradBatch()
    hip._fill_block(gb, hip.MPC_SEQ, s.seq_len, grads, B, flags)
    plant, keep = s._plant(A, Bp, dev)
    lg = hip._SweepLog(r["z_log"].data_ptr(), r["l_log"].data_ptr(), r["v_log"].data_ptr(), r["x_log"].data_ptr(),
                       r["eflag_log"].data_ptr())
    gu = torch.ones((STEPS, B, s.nu), dtype=torch.float64, device=dev)
    status = torch.full((MAX_BATCH + 1,), -1, dtype=torch.int32, device=dev)

    def adjoint(batch):
        return lib.fbstab_hip_mpc_receding_sweep_adjoint(s._h, batch, C.byref(blk), C.byref(plant), STEPS, 1, C.byref(lg),
                                                         gu.data_ptr(), None, C.c_double(0.0), C.byref(gb), None,
                                                         status.data_ptr(), None)

    Q, q = hip.MPC_SEQ.index("Q"), hip.MPC_SEQ.index("q")
    for block, slot, bad, text in (
            (gb, q, 0, "sweep adjoint: a gradient slot of stride 0 (summed over the batch) is not served"),
            (gb, Q, s.seq_len[Q] - 1, GRAD_TEXT), (blk, Q, s.seq_len[Q] - 1, DATA_TEXT)):
        own = block.stride[slot]
        block.stride[slot] = bad
        _refused(lib, adjoint(B), text)
        block.stride[slot] = own
    _refused(lib, adjoint(MAX_BATCH + 1), BATCH_TEXT)
    torch.cuda.synchronize()
    assert all(_untouched(g) for g in grads.values()) and (status == -1).all()
    res = s.RecedingSweepAdjoint(data, A, Bp, STEPS, r, gu=gu)
    assert (res["status"].cpu().numpy() == 0).all() and all(np.isfinite(res[k].cpu().numpy()).all() for k in hip.MPC_SEQ)


# ---- dense: (2, 1, 3) and (2, 0, 3), max_batch 3 ------------------------------------------------------------------
@pytest.mark.parametrize("nl", [1, 0])
def test_the_dense_multi_solves_refuse_a_batch_beyond_the_handle_and_h_without_equality_constraints(hip, nl):
    nz, nv = 2, 3
    p = fx.synthetic_dense_batch(B, nz, nl, nv)
    s = hip.FBstabDenseBatch(nz, nl, nv, max_batch=MAX_BATCH)
    lib, lens = s._lib, (nz, nl, nv)
    z, l, v, y = (np.zeros((B, n)) for n in (nz, nl, nv, nv))
    assert (s.Solve(p.arrays, z, l, v, y)["eflag"] == 0).all()
    blk = hip._DenseBatch()
    hip._fill_block(blk, hip.DENSE_ARR, s.arr_len, p.arrays, B, [])
    xb = hip._fill_vars((z, l, v), lens, B, [])
    dz, status = _canaries((B, nv, nz)), np.full(MAX_BATCH + 1, -1, dtype=np.int32)
    ob = _multi(hip, (dz, None, None), lens, nv)
    jacobian = lambda batch, wrt: lib.fbstab_hip_dense_jacobian_batch(
        s._h, batch, C.byref(blk), C.byref(xb), s.WRT[wrt], C.c_double(0.0), C.byref(ob), status.ctypes.data, 0, None)
    _refused(lib, jacobian(MAX_BATCH + 1, "b"), BATCH_TEXT)
    seeds = np.ones((B, 1, nz))
    sb = _multi(hip, (seeds, None, None), lens, 1)
    _refused(lib, lib.fbstab_hip_dense_kkt_solve_batch(s._h, MAX_BATCH + 1, C.byref(blk), C.byref(xb), 1, C.byref(sb),
                                                       C.c_double(0.0), C.byref(ob), status.ctypes.data, 0, None),
             BATCH_TEXT)
    if nl == 0:
        _refused(lib, jacobian(B, "h"), "dense jacobian: wrt = h on a handle without equality constraints")
        # (the batch is looked at first)
        _refused(lib, jacobian(MAX_BATCH + 1, "h"), BATCH_TEXT)
    assert _untouched(dz) and (status == -1).all()
    hip._check(lib, jacobian(B, "b"))
    res = s.Jacobian(p.arrays, z, l, v, wrt="b")
    assert (status[:B] == 0).all() and (res["status"] == 0).all() and np.array_equal(res["dz"], dz)
    res = s.KktSolve(p.arrays, z, l, v, seeds)
    assert (res["status"] == 0).all() and np.isfinite(res["dz"]).all()
    s.close()
