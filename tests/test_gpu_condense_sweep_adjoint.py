"""The adjoint through the closed-loop sweep of the condensed route on the device
(fbstab_hip_mpc_condensed_receding_sweep_adjoint, ``CondensedMpc.RecedingSweepAdjoint``,
``autograd.closed_loop_condensed_mpc``): one step against ``CondensedMpc.Adjoint``, six steps against the longdouble
recursion of tests/condense_sweep_adjoint_helpers.py, retirement off, determinism and placement, the argument
checks, and autograd."""
import ctypes as C
import functools

import numpy as np
import pytest

from fbstab_amd.hip_api import MPC_SEQ
from tests import condense_helpers as ch
from tests import condense_sweep_adjoint_helpers as sah
from tests import condense_sweep_helpers as csh
from tests import sweep_adjoint_helpers as mah

pytestmark = pytest.mark.gpu
LD = ch.LD
SIX = sah.SIX
DATA_SEQ = tuple(k for k in MPC_SEQ if k != "x0")


@pytest.fixture(scope="module")
def hip():
    from fbstab_amd import hip_api
    hip_api.load_library()
    return hip_api


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


_LIVE = []


@functools.lru_cache(maxsize=None)
def solver(sizes, tag=""):
    from fbstab_amd.condense import CondensedMpc
    _LIVE.append(CondensedMpc(*sizes, max_batch=8))
    return _LIVE[-1]


@pytest.fixture(scope="module", autouse=True)
def _release_the_solvers():
    yield
    import torch
    torch.cuda.synchronize()
    while _LIVE:
        _LIVE.pop().close()
    solver.cache_clear()
    forward.cache_clear()


def _data(p, qps=None, shared=()):
    d = {}
    for k, a in p.arrays.items():
        d[k] = _dev(a[:1] if k in shared else (a if qps is None else a[qps]))
    return d


def seeds(p, steps=SIX, seed=21):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((steps, p.batch, p.nu)), rng.standard_normal((steps, p.batch, p.nx))


@functools.lru_cache(maxsize=None)
def forward(name, mode="affine", shift=False, retire=True, steps=SIX):
    """The device's own logged sweep of ``csh.setup(name)`` from a zero guess, as numpy arrays."""
    import torch
    p, A, B, w = csh.setup(name)
    cm = solver(p.sizes())
    point = [torch.zeros((p.batch, n), dtype=torch.float64, device="cuda") for n in (p.nz, p.nl, p.nv, p.nv)]
    r = cm.RecedingSweep(_data(p), *point, _dev(A), _dev(B), steps, retire=retire, w=_dev(w[:steps]), shift=shift,
                         mode=mode, log=("x", "U", "v"))
    torch.cuda.synchronize()
    return {k: r[k].cpu().numpy() for k in ("u", "x", "U", "v", "eflag")}


def adjoint(name, log, gu, gx, mode="affine", qps=None, shared=(), **kw):
    """``CondensedMpc.RecedingSweepAdjoint`` on device tensors; numpy arrays back."""
    import torch
    p, A, B, w = csh.setup(name)
    cm = solver(p.sizes())
    sel = (lambda a: a) if qps is None else (lambda a: np.ascontiguousarray(a[:, qps]))
    dlog = {k: (torch.from_numpy(sel(log[k])).cuda()) for k in ("x", "U", "v", "eflag")}
    Aq, Bq = (A, B) if qps is None else (A[qps], B[qps])
    kw.setdefault("want", DATA_SEQ)
    kw.setdefault("mu", True)
    g = cm.RecedingSweepAdjoint(_data(p, qps, shared), _dev(Aq), _dev(Bq), log["eflag"].shape[0], dlog,
                                gu=None if gu is None else _dev(sel(gu)), gx=None if gx is None else _dev(sel(gx)),
                                mode=mode, **kw)
    torch.cuda.synchronize()
    return {k: a.cpu().numpy() for k, a in g.items()}


# ---- 1. one step ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "four_wave"])
def test_one_step_equals_the_single_point_adjoint(hip, name):
    """RECONDENSE mode, gx = 0, random gu: the 11 data gradients are, as numbers, those of ``CondensedMpc.Adjoint`` at
    the returned point with the seed on the u_0 entries of gz; status is equal; the x0 gradient lies within the CPU
    rounding bound of that call's x0 gradient (in both modes)."""
    import torch
    p, A, B, w = csh.setup(name)
    N, nx, nu, nc = p.sizes()
    cm = solver(p.sizes())
    log = forward(name, "recondense", steps=1)
    gu, _ = seeds(p, 1)
    g = adjoint(name, log, gu, None, mode="recondense", gf0=True, gb0=True)
    # the single-point adjoint at the expanded returned point
    d = _data(p)
    d["x0"] = _dev(log["x"][0])
    z, l, v, y = cm.Expand(d, _dev(log["U"][0]), _dev(log["v"][0]), _dev(log["v"][0]))
    cm.Condense(d)
    gz = np.zeros((p.batch, N + 1, nx + nu))
    gz[:, 0, nx:] = gu[0]
    ref = cm.Adjoint(d, z, l, v, _dev(gz.reshape(p.batch, -1)), adj=True)
    torch.cuda.synchronize()
    ref = {k: a.cpu().numpy() for k, a in ref.items()}
    ok = log["eflag"][0] == 0
    assert ok.any()
    assert np.array_equal(g["status"], np.where(ok, ref["status"], 0))
    for k in DATA_SEQ:
        assert np.array_equal(g[k][ok], ref[k][ok] + 0.0), k
        assert not g[k][~ok].any(), k
    dU = ref["dz"].reshape(p.batch, N + 1, nx + nu)[:, :, nx:].reshape(p.batch, -1)
    assert np.array_equal(g["gf0"][ok], (0.0 - dU)[ok]) and np.array_equal(g["gb0"][ok], ref["dv"][ok])
    m = cm.X0Map(_data(p))
    M = m["M"].cpu().numpy()
    ga = adjoint(name, log, gu, None, mode="affine")
    for q in np.flatnonzero(ok):
        F, G = csh.map_parts(p, M[q])
        _, S = sah.lambda_reference(A[q], F, G, np.zeros(nx), dU[q], ref["dv"][q], 2)
        bound = sah.lambda_bound((N + 1) * (nu + nc), nx, S).astype(np.float64)
        for got, what in ((g, "recondense"), (ga, "affine")):
            err = np.abs(got["x0"][q] - ref["x0"][q])
            print(name, what, "traj", q, "x0: worst |gap| / bound = %.3g" % float((err / np.where(bound > 0, bound, 1)).max()))
            assert (err <= bound).all(), (what, q)
    for k in DATA_SEQ:   # (the affine mode's f_c, b_c differ from the vectors kernel's in the last bits)
        assert np.allclose(ga[k], g[k], rtol=1e-6, atol=1e-9), k


# ---- 2. six steps ------------------------------------------------------------------------------------------------------
def device_step(p, cm):
    """The per-step adjoint of the recursion from the device's own ``CondensedMpc.Adjoint``: points through ``Expand``
    with x0 := x_log[k]."""
    import torch
    N, nx, nu, nc = p.sizes()

    def fn(k, q, xk, U, v, gU):
        d = {name: _dev(a[q:q + 1]) for name, a in p.arrays.items()}
        d["x0"] = _dev(np.asarray(xk)[None])
        z, l, vv, y = cm.Expand(d, _dev(U[None]), _dev(v[None]), _dev(v[None]))
        cm.Condense(d)
        gz = np.zeros((1, N + 1, nx + nu))
        gz[0, 0, nx:] = np.asarray(gU[:nu], dtype=np.float64)
        r = cm.Adjoint(d, z, l, vv, _dev(gz.reshape(1, -1)), adj=True)
        torch.cuda.synchronize()
        dz = r["dz"].cpu().numpy()[0].reshape(N + 1, nx + nu)
        tab = {name: r[name].cpu().numpy()[0] for name in MPC_SEQ}
        return int(r["status"].cpu().numpy()[0]), dz[:, nx:].reshape(-1), r["dv"].cpu().numpy()[0], tab
    return fn


@pytest.mark.parametrize("shift", [False, True])
@pytest.mark.parametrize("mode", ["affine", "recondense"])
@pytest.mark.parametrize("name", csh.LOOP_FIXTURES)
def test_six_steps_against_the_longdouble_recursion(hip, name, mode, shift):
    """g_ref: the per-gradient relative gap between two numpy recursions at the same logged points, one over the
    device's own per-step ``CondensedMpc.Adjoint``, one over ``chain_reference`` in longdouble.  Each gradient's gap to
    the longdouble recursion is at most 10 max(g_ref, steps 2^-52), relative to its largest entry; status, and mu at
    retired steps, are exact."""
    p, A, B, w = csh.setup(name)
    cm = solver(p.sizes())
    log = forward(name, mode, shift)
    assert {q: k for q, k in csh.retirement(log["eflag"]).items()} == {q: k for q, k in csh.RETIRES[name].items()
                                                                        if k < SIX}
    gu, gx = seeds(p)
    g = adjoint(name, log, gu, gx, mode=mode)
    maps = [(a[1], a[3]) for a in csh.condenser(name).affine()]
    ref, rstatus, rmu = sah.reference_condensed_sweep_adjoint(sah.chain_step(p), p, A, B, maps, log, gu, gx)
    M = cm.X0Map(_data(p))["M"].cpu().numpy()
    dmaps = [csh.map_parts(p, M[q]) for q in range(p.batch)]
    dev, dstatus, _ = sah.reference_condensed_sweep_adjoint(device_step(p, cm), p, A, B, dmaps, log, gu, gx)
    g_ref = sah.rel_gaps(dev, ref)
    gaps = sah.rel_gaps(g, ref)
    floor = SIX * 2.0 ** -52
    for k in MPC_SEQ:
        print("%-17s %-10s shift %d %-2s gap %.3g g_ref %.3g" % (name, mode, shift, k, gaps[k], g_ref[k]))
    assert np.array_equal(g["status"], rstatus) and np.array_equal(dstatus, rstatus)
    for q, k in csh.retirement(log["eflag"]).items():
        assert np.array_equal(g["mu"][k:, q], gx[k:, q])
    for k in MPC_SEQ:
        assert gaps[k] <= 10 * max(g_ref[k], floor), (k, gaps[k], g_ref[k])
    top = float(np.abs(rmu).max())
    assert float(np.abs(g["mu"].astype(LD) - rmu).max()) <= 10 * max(g_ref["x0"], floor) * max(top, 1.0)


# ---- 3. retirement off ---------------------------------------------------------------------------------------------------
def test_without_retirement_a_failed_trajectory_carries_the_plant_chain(hip):
    """retire = 0 on double_integrator: trajectory 2 never reaches a solution; its data gradients are zero and its x0
    gradient is the plant's own chain lambda <- A_p'(gx[k] + lambda), within (nx + 3) 2^-53 per step of the sum of the
    magnitudes."""
    name = "double_integrator"
    p, A, B, w = csh.setup(name)
    nx = p.nx
    log = forward(name, "affine", retire=False)
    assert (log["eflag"][:, 2] != 0).all() and (log["eflag"][:, 2] != -1).all()
    assert (log["eflag"][:, [0, 1, 3, 4]] == 0).all()
    gu, gx = seeds(p)
    g = adjoint(name, log, gu, gx)
    for k in DATA_SEQ:
        assert not g[k][2].any(), k
    assert g["q"][0].any() and g["r"][0].any()
    lam, S = np.zeros(nx, dtype=LD), np.zeros(nx, dtype=LD)
    Al = np.asarray(A[2], dtype=LD)
    for k in range(SIX - 1, -1, -1):
        lam, S = Al.T @ (gx[k, 2] + lam), np.abs(Al).T @ (np.abs(gx[k, 2]) + S)
    assert (np.abs(g["x0"][2].astype(LD) - lam) <= SIX * (nx + 3) * sah.U2 * S).all()
    assert g["status"][2] == 0


# ---- 4. determinism and placement ---------------------------------------------------------------------------------------
def test_grouping_sub_batches_and_null_arguments_change_no_bit(hip):
    name = "small"
    p, A, B, w = csh.setup(name)
    log = forward(name)
    gu, gx = seeds(p)
    base = adjoint(name, log, gu, gx, gf0=True, gb0=True)
    for T in (1, 2):
        r = adjoint(name, log, gu, gx, traj_per_group=T, gf0=True, gb0=True)
        for k in base:
            assert np.array_equal(r[k], base[k]), (T, k)
    rows = [3, 1]
    r = adjoint(name, log, gu, gx, qps=rows)
    for k in base:
        if k in r:
            assert np.array_equal(r[k], base[k][:, rows] if k == "mu" else base[k][rows]), k
    # the x0 gradient alone (no finish kernel, the smaller work array) and without the optional outputs
    r = adjoint(name, log, gu, gx, want=(), mu=False)
    assert set(r) == {"x0", "status"} and np.array_equal(r["x0"], base["x0"])
    # NULL gu, NULL gx: zeros
    zu, zx = np.zeros_like(gu), np.zeros_like(gx)
    for a, b in (((None, gx), (zu, gx)), ((gu, None), (gu, zx))):
        ra, rb = adjoint(name, log, *a), adjoint(name, log, *b)
        for k in ra:
            assert np.array_equal(ra[k], rb[k]), k
    both = adjoint(name, log, None, None)
    assert not any(both[k].any() for k in MPC_SEQ) and not both["mu"].any()


def test_shared_model_with_one_image_equals_per_qp_images(hip):
    """A batch that shares its matrices: ONE M, H_c, A_c (stride 0, M staged into LDS) gives the bits of per-QP
    images."""
    import torch
    name = "small"
    p, A, B, w = csh.setup(name)
    cm = solver(p.sizes())
    arrays = {k: (np.repeat(a[:1], p.batch, axis=0) if k in ch.MATRIX_NAMES else a) for k, a in p.arrays.items()}
    Aq, Bq = np.repeat(A[:1], p.batch, axis=0), np.repeat(B[:1], p.batch, axis=0)
    point = [torch.zeros((p.batch, n), dtype=torch.float64, device="cuda") for n in (p.nz, p.nl, p.nv, p.nv)]
    r = cm.RecedingSweep({k: _dev(a) for k, a in arrays.items()}, *point, _dev(Aq), _dev(Bq), SIX, log=("x", "U", "v"))
    log = {k: r[k] for k in ("x", "U", "v", "eflag")}
    gu, gx = seeds(p)
    res = []
    for shared in (False, True):
        d = {k: _dev(a[:1] if (shared and k in ch.MATRIX_NAMES) else a) for k, a in arrays.items()}
        g = cm.RecedingSweepAdjoint(d, _dev(Aq[0] if shared else Aq), _dev(Bq[0] if shared else Bq), SIX, log,
                                    gu=_dev(gu), gx=_dev(gx), want=DATA_SEQ, mu=True)
        torch.cuda.synchronize()
        res.append({k: a.cpu().numpy() for k, a in g.items()})
    assert (res[0]["status"] == 0).all() and np.abs(res[0]["x0"]).max() > 0
    for k in res[0]:
        assert np.array_equal(res[0][k], res[1][k]), k


def raw_call(hip, name, log, gu, gx, mode=0, pad=0, drop_log=None, zero_stride=None, null_map=False, handle=None,
             steps=None, batch=None, want=DATA_SEQ):
    """fbstab_hip_mpc_condensed_receding_sweep_adjoint itself on ``csh.setup(name)``: (rc, gradients as numpy arrays
    of ``len + pad`` columns pre-filled with NaN, status)."""
    import torch
    from fbstab_amd import condense
    lib = hip.load_library()
    p, A, B, w = csh.setup(name)
    N, nx, nu, nc = p.sizes()
    cm = solver(p.sizes())
    Bn = p.batch
    steps = log["eflag"].shape[0] if steps is None else steps
    d = cm._data(_data(p))
    cm._condense(d, "all")
    m = cm._x0_map(d)
    cmap = hip._CondensedMap(m["M"].data_ptr(), m["f0"].data_ptr(), m["b0"].data_ptr(), m["M"].shape[1], cm.nzc, cm.nv)
    dense = hip._DenseBatch()
    for k in ("H", "f", "A", "b"):
        a, i = cm._img[k], hip.DENSE_ARR.index(k)
        dense.base[i], dense.stride[i] = a.data_ptr(), cm._len[k]
    Ad, Bd = _dev(A.transpose(0, 2, 1)), _dev(B.transpose(0, 2, 1))
    plant = hip._Plant(Ad.data_ptr(), Bd.data_ptr(), nx * nx, nx * nu)
    dl = {k: torch.from_numpy(np.ascontiguousarray(log[k])).cuda() for k in ("x", "U", "v", "eflag")}
    at = lambda k: None if k == drop_log else dl[k].data_ptr()
    lg = hip._CondensedSweepLog(None, at("x"), at("U"), at("v"), at("eflag"), None)
    res = {k: torch.full((Bn, n + pad), np.nan, dtype=torch.float64, device="cuda")
           for k, n in zip(MPC_SEQ, cm.seq_len) if k in want or k == "x0"}
    grad = hip._MpcGradBatch()
    for i, (k, n) in enumerate(zip(MPC_SEQ, cm.seq_len)):
        if k in res:
            grad.base[i], grad.stride[i] = res[k].data_ptr(), (0 if k == zero_stride else n + pad)
    sizes = condense.condensed_sweep_adjoint_sizes(N, nx, nu, nc, 0, False)
    work = torch.empty((Bn, sizes["work_doubles_per_traj_grad"]), dtype=torch.float64, device="cuda")
    status = torch.full((Bn,), 77, dtype=torch.int32, device="cuda")
    gud, gxd = _dev(gu), _dev(gx)
    blk = cm._mpc_block(d, Bn)
    rc = lib.fbstab_hip_mpc_condensed_receding_sweep_adjoint(
        handle if handle is not None else cm.dense._h, N, nx, nu, nc, Bn if batch is None else batch, C.byref(blk),
        C.byref(dense), None if null_map else C.byref(cmap), C.byref(plant), steps, 1, C.byref(lg),
        C.c_void_p(gud.data_ptr()), C.c_void_p(gxd.data_ptr()), C.c_double(0.0), C.byref(grad), None, None, None,
        C.c_void_p(status.data_ptr()), mode, 0, C.c_void_p(work.data_ptr()), None)
    torch.cuda.synchronize()
    return rc, {k: a.cpu().numpy() for k, a in res.items()}, status.cpu().numpy()


def test_padding_between_slots_is_untouched(hip):
    name = "small"
    p, A, B, w = csh.setup(name)
    log = forward(name)
    gu, gx = seeds(p)
    base = adjoint(name, log, gu, gx)
    rc, res, status = raw_call(hip, name, log, gu, gx, pad=3)
    assert rc == 0, hip.load_library().fbstab_hip_last_error()
    for k, a in res.items():
        n = a.shape[1] - 3
        assert np.array_equal(a[:, :n], base[k]), k
        assert np.isnan(a[:, n:]).all(), k
    assert np.array_equal(status, base["status"])


# ---- 5. argument checks ------------------------------------------------------------------------------------------------
def test_argument_checks(hip):
    name = "small"
    p, A, B, w = csh.setup(name)
    log = forward(name)
    gu, gx = seeds(p)
    lib = hip.load_library()
    for kw, text in ((dict(drop_log="U"), b"logs are required"), (dict(drop_log="eflag"), b"logs are required"),
                     (dict(zero_stride="q"), b"gradient stride"), (dict(null_map=True), b"needs the map"),
                     (dict(mode=2), b"`mode`")):
        rc, res, status = raw_call(hip, name, log, gu, gx, **kw)
        assert rc == 1 and text in lib.fbstab_hip_last_error(), (kw, lib.fbstab_hip_last_error())
        assert all(np.isnan(a).all() for a in res.values()) and (status == 77).all(), kw
    other = solver((p.N + 1, p.nx, p.nu, p.nc), "other")
    rc, res, status = raw_call(hip, name, log, gu, gx, handle=other.dense._h)
    assert rc == 1 and b"dense handle is not one of" in lib.fbstab_hip_last_error()
    assert (status == 77).all()
    # a NULL map is fine in RECONDENSE mode
    rc, res, status = raw_call(hip, name, log, gu, gx, mode=1, null_map=True)
    assert rc == 0, lib.fbstab_hip_last_error()
    base = adjoint(name, log, gu, gx, mode="recondense")
    for k, a in res.items():
        assert np.array_equal(a, base[k]), k
    # batch == 0: OK, nothing queued; steps == 0: OK, zeros in every slot
    rc, res, status = raw_call(hip, name, log, gu, gx, batch=0)
    assert rc == 0 and all(np.isnan(a).all() for a in res.values()) and (status == 77).all()
    rc, res, status = raw_call(hip, name, log, gu, gx, steps=0, pad=2)
    assert rc == 0 and not status.any()
    for k, a in res.items():
        assert not a[:, :-2].any() and np.isnan(a[:, -2:]).all(), k
    r = solver(p.sizes()).RecedingSweepAdjoint(
        _data(p), _dev(A), _dev(B), 0, {k: log[k][:0] for k in ("x", "U", "v", "eflag")}, want=("q",), mu=True)
    assert r["mu"].shape == (0, p.batch, p.nx) and isinstance(r["q"], np.ndarray) and not r["q"].any()


# ---- 6. autograd -------------------------------------------------------------------------------------------------------
def test_autograd_backward_is_the_method(hip):
    """``closed_loop_condensed_mpc``: backward is ``RecedingSweepAdjoint``'s output bit for bit, a shared input gets
    the batch sum, w.grad is the masked mu, A.grad and B.grad leave out the costates of retired steps."""
    import torch
    from fbstab_amd import autograd as ag
    name = "double_integrator"             # (one model for all trajectories; trajectory 2 retires at step 0)
    p, A, B, w = csh.setup(name)
    arrays = p.arrays
    assert (arrays["Q"] == arrays["Q"][:1]).all()
    cm = solver(p.sizes())
    data = {k: _dev(a) for k, a in arrays.items()}
    data["Q"] = data["Q"][:1].clone()        # one shared sequence
    for k in ("Q", "q", "d", "x0", "E"):
        data[k].requires_grad_(True)
    At, Bt, wt = _dev(A[0]).requires_grad_(True), _dev(B[0]).requires_grad_(True), _dev(w[:SIX]).requires_grad_(True)
    cu, cx = seeds(p, seed=31)
    u, x, out = ag.closed_loop_condensed_mpc(cm, data, At, Bt, SIX, w=wt)
    ((_dev(cu) * u).sum() + (_dev(cx) * x).sum()).backward()
    torch.cuda.synchronize()
    # the same sweep and the method by hand
    point = [torch.zeros((p.batch, n), dtype=torch.float64, device="cuda") for n in (p.nz, p.nl, p.nv, p.nv)]
    d0 = {k: a.detach().clone() for k, a in data.items()}
    r = cm.RecedingSweep(d0, *point, At.detach(), Bt.detach(), SIX, w=wt.detach(), log=("x", "U", "v"))
    assert np.array_equal(r["u"].cpu().numpy(), u.detach().cpu().numpy())
    g = cm.RecedingSweepAdjoint({k: a.detach() for k, a in data.items()}, At.detach(), Bt.detach(), SIX,
                                {k: r[k] for k in ("x", "U", "v", "eflag")}, gu=_dev(cu), gx=_dev(cx),
                                want=("Q", "q", "d", "E"), mu=True)
    torch.cuda.synchronize()
    for k in ("q", "d", "x0", "E"):
        assert torch.equal(data[k].grad, g[k]), k
    assert torch.equal(data["Q"].grad, g["Q"].sum(0).reshape(data["Q"].shape))
    gone = (r["eflag"] == -1)
    assert gone.any() and not gone.all()
    mu = torch.where(gone[:, :, None], torch.zeros_like(g["mu"]), g["mu"])
    assert torch.equal(wt.grad, mu)
    assert torch.equal(At.grad, torch.einsum("kbi,kbj->ij", mu, r["x"]))
    assert torch.equal(Bt.grad, torch.einsum("kbi,kbj->ij", mu, r["u"]))


def test_central_differences_on_the_device(hip):
    """The CPU test's problem and rule along q and x0 with the forward run through ``CondensedMpc.RecedingSweep`` at
    abs_tol = 1e-11 and the gradients from ``RecedingSweepAdjoint``."""
    import torch
    from oracle.oracle_py import default_options
    from fbstab_amd.condense import CondensedMpc
    from tools import fixtures as fx
    p, A, B, cu, cx, dirs = mah.fd_problem()
    N, nx, nu, nc = p.sizes()
    T = mah.FD_STEPS
    cm = CondensedMpc(*p.sizes(), max_batch=p.batch)
    _LIVE.append(cm)
    cm.dense.UpdateOptions(default_options(abs_tol=1e-11))

    def sweep(problem):
        point = [torch.zeros((p.batch, n), dtype=torch.float64, device="cuda") for n in (p.nz, p.nl, p.nv, p.nv)]
        d = {k: _dev(a) for k, a in problem.arrays.items()}
        r = cm.RecedingSweep(d, *point, _dev(A), _dev(B), T, log=("x", "U", "v"))
        torch.cuda.synchronize()
        return r, d["x0"].cpu().numpy()
    r, x_end = sweep(p)
    log = {k: r[k].cpu().numpy() for k in ("u", "x", "U", "v", "eflag")}
    zs = np.zeros((T, p.batch, p.nz))
    for k in range(T):
        d = {name: _dev(a) for name, a in p.arrays.items()}
        d["x0"] = _dev(log["x"][k])
        zs[k] = cm.Expand(d, _dev(log["U"][k]), _dev(log["v"][k]), _dev(log["v"][k]))[0].cpu().numpy()
    good = mah.strictly_complementary(p, dict(eflag=log["eflag"], x=log["x"], z=zs, v=log["v"]))
    print("strictly complementary:", good)
    assert len(good) >= 5, good
    g = cm.RecedingSweepAdjoint({k: _dev(a) for k, a in p.arrays.items()}, _dev(A), _dev(B), T,
                                {k: r[k] for k in ("x", "U", "v", "eflag")}, gu=_dev(cu), gx=_dev(cx), want=("q",))
    torch.cuda.synchronize()
    grads = {k: g[k].cpu().numpy() for k in ("q", "x0")}
    assert not g["status"].cpu().numpy().any()
    for name in ("q", "x0"):
        L = []
        for sg in (1.0, -1.0):
            arr = {k: a.copy() for k, a in p.arrays.items()}
            arr[name] = arr[name] + sg * mah.FD_H * dirs[name][None]
            rr, xe = sweep(fx.MpcProblem(N, nx, nu, nc, arr))
            u = rr["u"].cpu().numpy()
            x = np.concatenate([rr["x"].cpu().numpy()[1:], xe[None]], 0)
            L.append((cu * u).sum(axis=(0, 2)) + (cx * x).sum(axis=(0, 2)))
        fd = (L[0] - L[1]) / (2 * mah.FD_H)
        for q in good:
            ad = float(grads[name][q] @ dirs[name])
            bound = 1e-4 * max(abs(ad), 1e-2 * np.abs(grads[name][q]).sum())
            print("%-2s traj %d: fd %+.6e ad %+.6e bound %.2e" % (name, q, fd[q], ad, bound))
            assert abs(fd[q] - ad) <= bound, (name, q, fd[q], ad, bound)
