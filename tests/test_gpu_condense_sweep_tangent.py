"""Forward mode through the closed-loop sweep of the condensed route on the device
(fbstab_hip_mpc_condensed_receding_sweep_tangent, ``CondensedMpc.RecedingSweepTangent``, ``forward_ad`` through
``autograd.closed_loop_condensed_mpc``): six steps against the longdouble recursion of
tests/condense_sweep_tangent_helpers.py, duality with ``RecedingSweepAdjoint`` on the same logs, retirement off, the
feedback gain from unit directions of x0, determinism and placement, the argument checks, autograd, and central
differences of the device sweep."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import condense_helpers as ch
from tests import condense_sweep_adjoint_helpers as sah
from tests import condense_sweep_helpers as csh
from tests import condense_sweep_tangent_helpers as sth
from tests import sweep_adjoint_helpers as mah

pytestmark = pytest.mark.gpu
LD = ch.LD
SIX = sth.SIX
REFS = ("q", "r", "c", "d")
FLOOR = SIX * 2.0 ** -52


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
    for f in (solver, forward, six_step_gaps, adjoint_gaps):
        f.cache_clear()


def _data(p, qps=None):
    return {k: _dev(a if qps is None else a[qps]) for k, a in p.arrays.items()}


def directions(p, steps=SIX, seed=41):
    """Random dx0, dw and directions of data's q, r, c, d."""
    rng = np.random.default_rng(seed)
    lens = p.seq_lengths()
    return dict(dx0=rng.standard_normal((p.batch, p.nx)), dw=rng.standard_normal((steps, p.batch, p.nx)),
                ddata={k: rng.standard_normal((p.batch, lens[k])) for k in REFS})


def seeds(p, steps=SIX, seed=21):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((steps, p.batch, p.nu)), rng.standard_normal((steps, p.batch, p.nx))


@functools.lru_cache(maxsize=None)
def forward(name, shift=False, retire=True, steps=SIX, tracked=False):
    """The device's own logged sweep of ``csh.setup(name)`` from a zero guess, as numpy arrays."""
    import torch
    p, A, B, w = csh.setup(name)
    cm = solver(p.sizes())
    point = [torch.zeros((p.batch, n), dtype=torch.float64, device="cuda") for n in (p.nz, p.nl, p.nv, p.nv)]
    ref = {k: _dev(a) for k, a in references(p, steps).items()} if tracked else None
    r = cm.RecedingSweep(_data(p), *point, _dev(A), _dev(B), steps, retire=retire, w=_dev(w[:steps]), shift=shift,
                         log=("x", "U", "v"), ref=ref)
    torch.cuda.synchronize()
    return {k: r[k].cpu().numpy() for k in ("u", "x", "U", "v", "eflag")}


def references(p, steps=SIX):
    """A per-step reference for q, every trajectory its own rows: the fixture's q moved a little at every step, so that
    the loop stays where the fixture's is."""
    rng = np.random.default_rng(51)
    q = p.arrays["q"][None] + 0.05 * rng.standard_normal((steps,) + p.arrays["q"].shape)
    return dict(q=q)


def tangent(name, log, dx0=None, dw=None, ddata=None, qps=None, **kw):
    """``CondensedMpc.RecedingSweepTangent`` on device tensors; numpy arrays back."""
    import torch
    p, A, B, w = csh.setup(name)
    cm = solver(p.sizes())
    sel = (lambda a: a) if qps is None else (lambda a: np.ascontiguousarray(a[:, qps]))
    row = (lambda a: a) if qps is None else (lambda a: np.ascontiguousarray(a[qps]))
    dlog = {k: torch.from_numpy(sel(log[k])).cuda() for k in ("x", "U", "v", "eflag")}
    Aq, Bq = (A, B) if qps is None else (A[qps], B[qps])
    for k in ("dref", "ref"):
        if kw.get(k) is not None:
            kw[k] = {n: _dev(sel(a)) for n, a in kw[k].items()}
    r = cm.RecedingSweepTangent(_data(p, qps), _dev(Aq), _dev(Bq), log["eflag"].shape[0], dlog,
                                dx0=None if dx0 is None else _dev(row(dx0)), dw=None if dw is None else _dev(sel(dw)),
                                ddata=None if ddata is None else {k: _dev(row(a)) for k, a in ddata.items()}, **kw)
    torch.cuda.synchronize()
    return {k: a.cpu().numpy() for k, a in r.items()}


def adjoint(name, log, gu, gx, **kw):
    import torch
    p, A, B, w = csh.setup(name)
    cm = solver(p.sizes())
    dlog = {k: torch.from_numpy(log[k]).cuda() for k in ("x", "U", "v", "eflag")}
    if kw.get("ref") is not None:
        kw["ref"] = {n: _dev(a) for n, a in kw["ref"].items()}
    g = cm.RecedingSweepAdjoint(_data(p), _dev(A), _dev(B), log["eflag"].shape[0], dlog, gu=_dev(gu), gx=_dev(gx),
                                mu=True, **kw)
    torch.cuda.synchronize()
    return {k: a.cpu().numpy() for k, a in g.items()}


# ---- 1. six steps ------------------------------------------------------------------------------------------------------
def device_step(p, cm, ddata):
    """The per-step solve of the recursion from the device's own single-point ``CondensedMpc.Tangent``: the point
    through ``Expand`` with x0 := x_log[k], the direction of x0 the carried dx."""
    import torch
    N, nx, nu, nc = p.sizes()

    def fn(k, q, xk, U, v, dx):
        d = {name: _dev(a[q:q + 1]) for name, a in p.arrays.items()}
        d["x0"] = _dev(np.asarray(xk)[None])
        z, l, vv, y = cm.Expand(d, _dev(U[None]), _dev(v[None]), _dev(v[None]))
        cm.Condense(d)
        dd = {name: _dev(a[q:q + 1]) for name, a in ddata.items()}
        dd["x0"] = _dev(np.asarray(dx, dtype=np.float64)[None])
        r = cm.Tangent(d, z, l, vv, dd)
        torch.cuda.synchronize()
        dz = r["dz"].cpu().numpy()[0].reshape(N + 1, nx + nu)
        return int(r["status"].cpu().numpy()[0]), dz[0, nx:]
    return fn


@functools.lru_cache(maxsize=None)
def six_step_gaps(name, shift):
    """(the device call's result, the longdouble recursion, g_ref per output): g_ref is the relative gap between two
    numpy recursions at the same logged points, one over the device's own per-step ``CondensedMpc.Tangent``, one over
    ``chain_reference`` in longdouble."""
    p, A, B, w = csh.setup(name)
    cm = solver(p.sizes())
    log = forward(name, shift)
    D = directions(p)
    got = tangent(name, log, **D)
    one = lambda k, q: {n: a[q] for n, a in D["ddata"].items()}
    ref = sth.mpc_form_recursion(sth.chain_mpc_step(p, one), p, A, B, log, D["dx0"], D["dw"])
    dev = sth.mpc_form_recursion(device_step(p, cm, D["ddata"]), p, A, B, log, D["dx0"], D["dw"])
    g_ref = dict(du=sth.rel_gap(dev[0], ref[0]), dx=sth.rel_gap(dev[1], ref[1]))
    return got, ref, dev, g_ref


@pytest.mark.parametrize("shift", [False, True])
@pytest.mark.parametrize("name", csh.LOOP_FIXTURES)
def test_six_steps_against_the_longdouble_recursion(hip, name, shift):
    """du and dx lie within 10 max(g_ref, steps 2^-52) of the longdouble recursion, relative to their largest entry;
    status is exact; du and dx are exactly zero at and after a retirement."""
    log = forward(name, shift)
    assert csh.retirement(log["eflag"]) == {q: k for q, k in csh.RETIRES[name].items() if k < SIX}
    got, ref, dev, g_ref = six_step_gaps(name, shift)
    gaps = dict(du=sth.rel_gap(got["du"], ref[0]), dx=sth.rel_gap(got["dx"], ref[1]))
    for k in ("du", "dx"):
        print("%-17s shift %d %s gap %.3g g_ref %.3g" % (name, shift, k, gaps[k], g_ref[k]))
    assert np.array_equal(got["status"], ref[2]) and np.array_equal(dev[2], ref[2])
    for q, k in csh.retirement(log["eflag"]).items():
        assert not got["du"][k:, q].any() and not got["dx"][k:, q].any()
    assert np.abs(got["du"]).max() > 0 and np.abs(got["dx"]).max() > 0
    for k in ("du", "dx"):
        assert gaps[k] <= 10 * max(g_ref[k], FLOOR), (k, gaps[k], g_ref[k])


# ---- 2. duality with the device's adjoint --------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def adjoint_gaps(name):
    """The adjoint twin of ``six_step_gaps``: (the device's RecedingSweepAdjoint, its g_ref over all gradients)."""
    from tests import test_gpu_condense_sweep_adjoint as tsa
    p, A, B, w = csh.setup(name)
    cm = solver(p.sizes())
    log = forward(name)
    gu, gx = seeds(p)
    g = adjoint(name, log, gu, gx, want=REFS)
    maps = [(a[1], a[3]) for a in csh.condenser(name).affine()]
    ref, _, _ = sah.reference_condensed_sweep_adjoint(sah.chain_step(p), p, A, B, maps, log, gu, gx)
    M = cm.X0Map(_data(p))["M"].cpu().numpy()
    dmaps = [csh.map_parts(p, M[q]) for q in range(p.batch)]
    dev, _, _ = sah.reference_condensed_sweep_adjoint(tsa.device_step(p, cm), p, A, B, dmaps, log, gu, gx)
    gaps = sah.rel_gaps(dev, ref)
    return g, max(gaps[k] for k in REFS + ("x0",))


@pytest.mark.parametrize("name", csh.LOOP_FIXTURES)
def test_duality_with_the_devices_adjoint(hip, name):
    """sum_k <gu_k, du_k> + <gx_k, dx_(k+1)> = <lambda_0, dx0> + sum_k <mu_k, dw_k> [not retired] + sum over q, r, c, d
    of <gradient, direction> between the two device calls on the same log, to 10 max(g_ref, steps 2^-52) of the sum of
    the magnitudes of the terms; g_ref: the larger of the two calls' gaps between their device and longdouble
    recursions."""
    p, A, B, w = csh.setup(name)
    log = forward(name)
    gu, gx = seeds(p)
    D = directions(p)
    got, _, _, tg = six_step_gaps(name, False)
    g, ag = adjoint_gaps(name)
    g_ref = max(tg["du"], tg["dx"], ag)
    extra = tuple((g[k], D["ddata"][k]) for k in REFS)
    lhs, rhs, S = sth.duality_sides(gu, gx, got["du"], got["dx"], g["x0"], g["mu"], log["eflag"], D["dx0"], D["dw"],
                                    extra=extra)
    live = S > 0
    bar = 10 * max(g_ref, FLOOR)
    print("%-17s duality: worst |lhs - rhs| / S = %.3g, g_ref tangent %.3g adjoint %.3g, bar %.3g" % (
        name, float((np.abs(lhs - rhs)[live] / S[live]).max()), max(tg.values()), ag, bar))
    assert live.sum() >= p.batch - 1
    assert (np.abs(lhs - rhs) <= bar * S).all(), (lhs, rhs, S)


def test_duality_of_the_tracked_form(hip):
    """The same identity through a sweep that tracks a per-step reference of q: the per-step gradient ``ref_grad``
    against the per-step direction ``dref``, the data's own r, c, d beside it."""
    name = "small"
    p, A, B, w = csh.setup(name)
    log = forward(name, tracked=True)
    ref = references(p)
    gu, gx = seeds(p)
    D = directions(p)
    rng = np.random.default_rng(61)
    dref = dict(q=rng.standard_normal(ref["q"].shape))
    dd = {k: D["ddata"][k] for k in ("r", "c", "d")}
    got = tangent(name, log, D["dx0"], D["dw"], dd, dref=dref, ref=ref)
    g = adjoint(name, log, gu, gx, want=REFS, ref=ref)
    assert g["q"].shape == dref["q"].shape
    _, _, _, tg = six_step_gaps(name, False)
    _, ag = adjoint_gaps(name)
    g_ref = max(tg["du"], tg["dx"], ag)
    extra = tuple((g[k], dd[k]) for k in dd)
    lhs, rhs, S = sth.duality_sides(gu, gx, got["du"], got["dx"], g["x0"], g["mu"], log["eflag"], D["dx0"], D["dw"],
                                    extra=extra)
    t = g["q"].astype(LD) * dref["q"].astype(LD)
    rhs, S = rhs + t.sum(axis=(0, 2)), S + np.abs(t).sum(axis=(0, 2))
    bar = 10 * max(g_ref, FLOOR)
    print("tracked duality: worst |lhs - rhs| / S = %.3g, bar %.3g" % (float((np.abs(lhs - rhs) / S).max()), bar))
    assert np.abs(t).sum() > 0 and (np.abs(lhs - rhs) <= bar * S).all(), (lhs, rhs, S)
    # ... and the reference's direction moves the result
    plain = tangent(name, log, D["dx0"], D["dw"], dd, ref=ref)
    assert not np.array_equal(plain["du"], got["du"])


# ---- 3. retirement off ---------------------------------------------------------------------------------------------------
def test_without_retirement_a_failed_trajectory_carries_the_plant_chain(hip):
    """retire = 0 on double_integrator: trajectory 2 never reaches a solution; its du is zero and its dx is the plant's
    own chain dx <- A_p dx + dw_k, within steps (nx + 3) 2^-53 of the sum of the magnitudes."""
    name = "double_integrator"
    p, A, B, w = csh.setup(name)
    nx = p.nx
    log = forward(name, retire=False)
    assert (log["eflag"][:, 2] != 0).all() and (log["eflag"][:, 2] != -1).all()
    assert (log["eflag"][:, [0, 1, 3, 4]] == 0).all()
    D = directions(p)
    r = tangent(name, log, **D)
    assert not r["du"][:, 2].any() and r["du"][:, 0].any() and r["status"][2] == 0
    d, S = D["dx0"][2].astype(LD), np.abs(D["dx0"][2]).astype(LD)
    Al = np.asarray(A[2], dtype=LD)
    for k in range(SIX):
        d, S = Al @ d + D["dw"][k, 2], np.abs(Al) @ S + np.abs(D["dw"][k, 2])
        assert (np.abs(r["dx"][k, 2].astype(LD) - d) <= SIX * (nx + 3) * sah.U2 * S).all(), k


# ---- 4. the feedback gain ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "four_wave"])
def test_unit_directions_of_x0_give_the_gain_of_x0_sensitivity(hip, name):
    """dx0 = e_j: du[0] is column j of ``X0Sensitivity``'s gain at the point of step 0.  The rule is that of the
    adjoint's one-step test: by duality entry (i, j) of the gain is lambda_0[j] = (F'(-dU) + G'dv)[j] of the adjoint
    step (dU, dv) for the seed e_i on u_0, and the two must agree within (ne + nx + 3) 2^-53 of the sum of the
    magnitudes of that sum's terms."""
    import torch
    p, A, B, w = csh.setup(name)
    N, nx, nu, nc = p.sizes()
    cm = solver(p.sizes())
    log = forward(name, steps=1)
    ok = log["eflag"][0] == 0
    assert ok.any()
    du = np.stack([tangent(name, log, dx0=np.repeat(np.eye(nx)[j:j + 1], p.batch, axis=0))["du"][0] for j in range(nx)],
                  axis=2)                                      # (batch, nu, nx)
    d = _data(p)
    d["x0"] = _dev(log["x"][0])
    z, l, v, y = cm.Expand(d, _dev(log["U"][0]), _dev(log["v"][0]), _dev(log["v"][0]))
    cm.Condense(d)
    gain = cm.X0Sensitivity(d, z, l, v, want=("gain",))["gain"].cpu().numpy()
    M = cm.X0Map(_data(p))["M"].cpu().numpy()
    worst = 0.0
    for i in range(nu):
        gz = np.zeros((p.batch, N + 1, nx + nu))
        gz[:, 0, nx + i] = 1.0
        cm.Condense(d)
        a = cm.Adjoint(d, z, l, v, _dev(gz.reshape(p.batch, -1)), adj=True)
        torch.cuda.synchronize()
        dU = a["dz"].cpu().numpy().reshape(p.batch, N + 1, nx + nu)[:, :, nx:].reshape(p.batch, -1)
        dv = a["dv"].cpu().numpy()
        for q in np.flatnonzero(ok):
            F, G = csh.map_parts(p, M[q])
            _, S = sah.lambda_reference(A[q], F, G, np.zeros(nx), dU[q], dv[q], 2)
            bound = sah.lambda_bound((N + 1) * (nu + nc), nx, S).astype(np.float64)
            err = np.abs(du[q, i] - gain[q, i])
            worst = max(worst, float((err / np.where(bound > 0, bound, 1)).max()))
            print(name, "traj", q, "input", i, "worst |du - gain| / bound = %.3g" % float((err / np.where(bound > 0, bound, 1)).max()))
            assert (err <= bound).all(), (q, i, err, bound)
    assert not du[~ok].any()


# ---- 5. determinism and placement ---------------------------------------------------------------------------------------
def test_grouping_sub_batches_and_null_arguments_change_no_bit(hip):
    name = "small"
    p, A, B, w = csh.setup(name)
    log = forward(name)
    D = directions(p)
    base = tangent(name, log, **D)
    for T in (1, 2):
        r = tangent(name, log, traj_per_group=T, **D)
        for k in base:
            assert np.array_equal(r[k], base[k]), (T, k)
    rows = [3, 1]
    r = tangent(name, log, qps=rows, **D)
    for k in ("du", "dx"):
        assert np.array_equal(r[k], base[k][:, rows]), k
    assert np.array_equal(r["status"], base["status"][rows])
    # NULL dw, NULL df0 and db0, NULL dx0: zeros
    zero = {k: np.zeros_like(a) for k, a in D["ddata"].items()}
    for a, b in ((dict(dx0=D["dx0"], dw=None, ddata=D["ddata"]), dict(dx0=D["dx0"], dw=np.zeros_like(D["dw"]), ddata=D["ddata"])),
                 (dict(dx0=D["dx0"], dw=D["dw"], ddata=None), dict(dx0=D["dx0"], dw=D["dw"], ddata=zero)),
                 (dict(dx0=None, dw=D["dw"], ddata=D["ddata"]), dict(dx0=np.zeros_like(D["dx0"]), dw=D["dw"], ddata=D["ddata"]))):
        ra, rb = tangent(name, log, **a), tangent(name, log, **b)
        for k in ra:
            assert np.array_equal(ra[k], rb[k]), k
    # a shared direction of data is the same direction in every row
    shared = {k: a[:1] for k, a in D["ddata"].items()}
    full = {k: np.repeat(a[:1], p.batch, axis=0) for k, a in D["ddata"].items()}
    ra, rb = tangent(name, log, D["dx0"], D["dw"], shared), tangent(name, log, D["dx0"], D["dw"], full)
    for k in ra:
        assert np.array_equal(ra[k], rb[k]), k
    # all-zero directions: all-zero outputs
    none = tangent(name, log)
    zeros = tangent(name, log, np.zeros_like(D["dx0"]), np.zeros_like(D["dw"]), zero)
    for r in (none, zeros):
        assert (r["du"] == 0).all() and (r["dx"] == 0).all() and (r["status"] == 0).all()


def test_shared_model_with_one_image_equals_per_trajectory_images(hip):
    """A batch that shares its matrices: ONE M, H_c, A_c (stride 0, M staged into LDS) gives the bits of
    per-trajectory images."""
    import torch
    name = "small"
    p, A, B, w = csh.setup(name)
    cm = solver(p.sizes())
    arrays = {k: (np.repeat(a[:1], p.batch, axis=0) if k in ch.MATRIX_NAMES else a) for k, a in p.arrays.items()}
    Aq, Bq = np.repeat(A[:1], p.batch, axis=0), np.repeat(B[:1], p.batch, axis=0)
    point = [torch.zeros((p.batch, n), dtype=torch.float64, device="cuda") for n in (p.nz, p.nl, p.nv, p.nv)]
    r = cm.RecedingSweep({k: _dev(a) for k, a in arrays.items()}, *point, _dev(Aq), _dev(Bq), SIX, log=("x", "U", "v"))
    log = {k: r[k] for k in ("x", "U", "v", "eflag")}
    D = directions(p)
    res = []
    for shared in (False, True):
        d = {k: _dev(a[:1] if (shared and k in ch.MATRIX_NAMES) else a) for k, a in arrays.items()}
        g = cm.RecedingSweepTangent(d, _dev(Aq[0] if shared else Aq), _dev(Bq[0] if shared else Bq), SIX, log,
                                    dx0=_dev(D["dx0"]), dw=_dev(D["dw"]), ddata={k: _dev(a) for k, a in D["ddata"].items()})
        torch.cuda.synchronize()
        res.append({k: a.cpu().numpy() for k, a in g.items()})
    assert (res[0]["status"] == 0).all() and np.abs(res[0]["du"]).max() > 0
    for k in res[0]:
        assert np.array_equal(res[0][k], res[1][k]), k


def raw_call(hip, name, log, D, guard=0, drop_log=None, dir_stride=None, dir_step=None, null_map=False, handle=None,
             steps=None, batch=None, images=False, explicit_zero_images=False, no_outputs=False, traj_per_group=0,
             null_dir=False, spoil=None):
    """fbstab_hip_mpc_condensed_receding_sweep_tangent itself on ``csh.setup(name)`` with dx0 and dw of ``D``:
    (rc, du, dx as numpy arrays with ``guard`` rows of NaN in front of and behind the packed outputs, status).
    ``spoil(s)``: called on the namespace of the call's blocks (``dense, cmap, img, plant, lg, dr``: the ctypes
    structures; ``nzc, nv``) and of its plain arguments (``s.args``: nu, handle, dense, plant, log, dir, status, work -
    set one to None for a NULL pointer) before the call."""
    import types
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
    img = None
    if images:      # the map's f0, b0 at every step: a step of 0
        img = hip._CondensedRefImages(m["f0"].data_ptr(), m["b0"].data_ptr(), 0, 0, cm.nzc, cm.nv)
    dense = hip._DenseBatch()
    for k in ("H", "f", "A", "b"):
        a, i = cm._img[k], hip.DENSE_ARR.index(k)
        dense.base[i], dense.stride[i] = a.data_ptr(), cm._len[k]
    Ad, Bd = _dev(A.transpose(0, 2, 1)), _dev(B.transpose(0, 2, 1))
    plant = hip._Plant(Ad.data_ptr(), Bd.data_ptr(), nx * nx, nx * nu)
    dl = {k: torch.from_numpy(np.ascontiguousarray(log[k])).cuda() for k in ("x", "U", "v", "eflag")}
    at = lambda k: None if k == drop_log else dl[k].data_ptr()
    lg = hip._CondensedSweepLog(None, at("x"), at("U"), at("v"), at("eflag"), None)
    x0d, dwd = _dev(D["dx0"]), _dev(D["dw"])
    dr = hip._CondensedSweepDir()
    dr.dx0, dr.stride_dx0, dr.dw = x0d.data_ptr(), (nx if dir_stride is None else dir_stride), dwd.data_ptr()
    zf, zb = torch.zeros((Bn, cm.nzc), dtype=torch.float64, device="cuda"), torch.zeros((Bn, cm.nv), dtype=torch.float64, device="cuda")
    if explicit_zero_images:
        dr.df0, dr.db0, dr.stride_df0, dr.stride_db0 = zf.data_ptr(), zb.data_ptr(), cm.nzc, cm.nv
    if dir_step is not None:
        dr.df0, dr.db0, dr.stride_df0, dr.stride_db0, dr.step_df0 = zf.data_ptr(), zb.data_ptr(), cm.nzc, cm.nv, dir_step
    outs = {k: torch.full((max(steps, 0) + 2 * guard, Bn, n), np.nan, dtype=torch.float64, device="cuda")
            for k, n in (("du", nu), ("dx", nx))}
    sizes = condense.condensed_sweep_tangent_sizes(N, nx, nu, nc, max(traj_per_group, 0), False)
    work = torch.full((Bn + 1, sizes["work_doubles_per_traj"]), np.nan, dtype=torch.float64, device="cuda")
    status = torch.full((Bn,), 77, dtype=torch.int32, device="cuda")
    optr = lambda k: None if no_outputs else C.c_void_p(outs[k][guard:].data_ptr() if max(steps, 0) + guard > 0 else work.data_ptr())
    s = types.SimpleNamespace(dense=dense, cmap=cmap, img=img, plant=plant, lg=lg, dr=dr, nzc=cm.nzc, nv=cm.nv, zf=zf, zb=zb,
                              args=dict(nu=nu, handle=handle if handle is not None else cm.dense._h, dense=C.byref(dense),
                                        plant=C.byref(plant), log=C.byref(lg), dir=None if null_dir else C.byref(dr),
                                        status=C.c_void_p(status.data_ptr()), work=C.c_void_p(work.data_ptr())))
    if spoil is not None:
        spoil(s)
    g = s.args
    rc = lib.fbstab_hip_mpc_condensed_receding_sweep_tangent(
        g["handle"], N, nx, g["nu"], nc, Bn if batch is None else batch, g["dense"],
        None if null_map else C.byref(cmap), C.byref(img) if img is not None else None, g["plant"], steps,
        g["log"], g["dir"], C.c_double(0.0), optr("du"), optr("dx"), g["status"], traj_per_group, g["work"], None)
    torch.cuda.synchronize()
    tail = work[Bn].cpu().numpy()     # the row behind the documented size of the work array
    return rc, outs["du"].cpu().numpy(), outs["dx"].cpu().numpy(), status.cpu().numpy(), tail


def test_images_null_directions_and_the_room_around_the_outputs(hip):
    """images = NULL against images that hold map->f0, map->b0 at every step, NULL df0 / db0 against explicit zeros:
    no bit changes.  The rows in front of and behind the packed outputs and behind the work array are untouched."""
    name = "small"
    p, A, B, w = csh.setup(name)
    log = forward(name)
    D = directions(p)
    base = tangent(name, log, D["dx0"], D["dw"])
    for kw in (dict(), dict(images=True), dict(explicit_zero_images=True), dict(images=True, explicit_zero_images=True)):
        rc, du, dx, status, tail = raw_call(hip, name, log, D, guard=2, **kw)
        assert rc == 0, hip.load_library().fbstab_hip_last_error()
        for got, want in ((du, base["du"]), (dx, base["dx"])):
            assert np.array_equal(got[2:-2], want), kw
            assert np.isnan(got[:2]).all() and np.isnan(got[-2:]).all(), kw
        assert np.array_equal(status, base["status"]) and np.isnan(tail).all(), kw


# ---- 6. argument checks ------------------------------------------------------------------------------------------------
def _null(which):
    return lambda s: s.args.__setitem__(which, None)


def _field_arg(which, value):
    return lambda s: s.args.__setitem__(which, value)


def _both(*fs):
    def spoil(s):
        for f in fs:
            f(s)
    return spoil


def _dense(slot, base=None, stride=None):
    def spoil(s):
        from fbstab_amd.hip_api import DENSE_ARR
        i = DENSE_ARR.index(slot)
        if base is not None:
            s.dense.base[i] = None
        if stride is not None:
            s.dense.stride[i] = stride
    return spoil


def _field(block, name, value):
    return lambda s: setattr(getattr(s, block), name, value)


def _dir_image(which, stride):
    """df0 or db0 given (zeros), with the trajectory stride ``stride``."""
    def spoil(s):
        s.dr.df0, s.dr.db0, s.dr.stride_df0, s.dr.stride_db0 = s.zf.data_ptr(), s.zb.data_ptr(), s.nzc, s.nv
        setattr(s.dr, "stride_" + which, stride)
    return spoil


def test_argument_checks(hip):
    """Every refusal of the entry point is FBSTAB_HIP_ERR_ARGUMENT with its text on the real runtime - each case also
    spoils the argument of a LATER check, so that the order is the documented one - and nothing is queued behind it:
    the outputs and status keep what they held."""
    from fbstab_amd.condense import CondensedMpc
    name = "small"
    p, A, B, w = csh.setup(name)
    nzc = (p.N + 1) * p.nu
    log = forward(name)
    D = directions(p)
    lib = hip.load_library()
    other = CondensedMpc(p.N + 1, p.nx, p.nu, p.nc, max_batch=2)     # another shape AND too small a max_batch
    small = CondensedMpc(*p.sizes(), max_batch=2)
    _LIVE.extend([other, small])
    null_handle = _null("handle")
    cases = [(dict(batch=-1, spoil=_field_arg("nu", 0)), b"problem sizes must be positive"),
             (dict(batch=-1, null_dir=True), b"negative batch")]
    cases += [(dict(no_outputs=True, spoil=_null(k)), b"null argument")
              for k in ("dense", "plant", "log", "dir", "status", "work")]
    cases += [(dict(no_outputs=True, spoil=_field("plant", "B", None)), b"both du and dx are null"),
              (dict(steps=-1, spoil=_field("plant", "B", None)), b"null plant matrix"),
              (dict(steps=-1, spoil=_field("plant", "A", None)), b"null plant matrix"),
              (dict(steps=-1, traj_per_group=-1), b"negative step count"),
              (dict(traj_per_group=-1, spoil=_dense("b", base=True)), b"negative traj_per_group"),
              # (the images are checked slot by slot, H, f, A, b: the later fault sits in a later slot or check)
              (dict(spoil=_both(_dense("H", base=True), _dense("f", stride=0))), b"null pointer in the condensed images"),
              (dict(spoil=_both(_dense("b", base=True), _field("plant", "stride_B", 1))),
               b"null pointer in the condensed images"),
              (dict(spoil=_both(_dense("f", stride=0), _field("plant", "stride_B", 1))),
               b"stride of a condensed image smaller than the array length"),
              (dict(spoil=_both(_dense("b", stride=1), _field("plant", "stride_A", 1))),
               b"stride of a condensed image smaller than the array length"),
              (dict(drop_log="x", spoil=_field("plant", "stride_B", 1)), b"plant stride smaller than the matrix"),
              (dict(drop_log="x", spoil=_field("plant", "stride_A", 1)), b"plant stride smaller than the matrix")]
    cases += [(dict(drop_log=k, dir_step=-1), b"logs are required") for k in ("x", "U", "v", "eflag")]
    cases += [(dict(dir_step=-1, dir_stride=1), b"negative step in the directions"),
              (dict(dir_stride=1, null_map=True), b"stride of a direction"),
              (dict(null_map=True, spoil=_dir_image("df0", nzc - 1)), b"stride of a direction"),
              (dict(null_map=True, spoil=_dir_image("db0", 1)), b"stride of a direction"),
              (dict(null_map=True, spoil=null_handle), b"needs the map"),
              (dict(spoil=_both(_field("cmap", "f0", None), null_handle)), b"null pointer in the map"),
              (dict(spoil=_both(_field("cmap", "M", None), null_handle)), b"null pointer in the map"),
              (dict(spoil=_both(_field("cmap", "stride_M", 1), null_handle)), b"stride of the map smaller"),
              (dict(spoil=_both(_field("cmap", "stride_b0", 1), null_handle)), b"stride of the map smaller"),
              # ... with images the map's M alone is looked at, then the images
              (dict(images=True, null_map=True, spoil=_field("img", "b0", None)), b"needs the map"),
              (dict(images=True, spoil=_both(_field("cmap", "M", None), _field("img", "b0", None))), b"needs the map"),
              (dict(images=True, spoil=_both(_field("cmap", "stride_M", 1), _field("img", "b0", None))),
               b"stride of the map smaller"),
              (dict(images=True, spoil=_both(_field("img", "b0", None), _field("img", "step_f0", -1))),
               b"null pointer in the reference images"),
              (dict(images=True, spoil=_both(_field("img", "step_f0", -1), _field("img", "stride_f0", 1))),
               b"negative step in the reference images"),
              (dict(images=True, spoil=_both(_field("img", "stride_f0", 1), null_handle)),
               b"trajectory stride of the reference images"),
              (dict(images=True, spoil=_both(_field("img", "stride_b0", 1), null_handle)),
               b"trajectory stride of the reference images"),
              # ... then the handle
              (dict(spoil=null_handle), b"null dense solver handle"),
              (dict(handle=other.dense._h), b"dense handle is not one of"),
              (dict(handle=small.dense._h), b"batch exceeds the max_batch")]
    for kw, text in cases:
        rc, du, dx, status, tail = raw_call(hip, name, log, D, **kw)
        assert rc == 1 and text in lib.fbstab_hip_last_error(), (kw, text, lib.fbstab_hip_last_error())
        assert np.isnan(du).all() and np.isnan(dx).all() and (status == 77).all() and np.isnan(tail).all(), (kw, text)
    # what the map's f0, b0 hold does not matter with images: NULL there is fine
    base = raw_call(hip, name, log, D, images=True)
    got = raw_call(hip, name, log, D, images=True, spoil=_both(_field("cmap", "f0", None), _field("cmap", "b0", None)))
    assert base[0] == 0 and got[0] == 0 and all(np.array_equal(a, b) for a, b in zip(base[1:4], got[1:4]))
    # batch == 0: OK, nothing queued; steps == 0: OK, status = 0 alone
    rc, du, dx, status, tail = raw_call(hip, name, log, D, batch=0)
    assert rc == 0 and np.isnan(du).all() and (status == 77).all()
    rc, du, dx, status, tail = raw_call(hip, name, log, D, steps=0, guard=1)
    assert rc == 0 and not status.any() and np.isnan(du).all() and np.isnan(dx).all()
    r = solver(p.sizes()).RecedingSweepTangent(_data(p), _dev(A), _dev(B), 0,
                                               {k: log[k][:0] for k in ("x", "U", "v", "eflag")}, dx0=D["dx0"])
    assert r["du"].shape == (0, p.batch, p.nu) and isinstance(r["dx"], np.ndarray) and not r["status"].any()
    with pytest.raises(NotImplementedError, match="matrix sequence 'Q'"):
        tangent(name, log, D["dx0"], None, dict(Q=np.zeros_like(p.arrays["Q"])))


# ---- 7. autograd -------------------------------------------------------------------------------------------------------
def test_forward_ad_is_the_method(hip):
    """``forward_ad`` through ``closed_loop_condensed_mpc``: the tangents of u and x are ``RecedingSweepTangent``'s
    output bit for bit - tangents on x0, w and one reference, the plant's A and B folded into dw and left out at
    retired steps - and a tangent on a matrix sequence raises."""
    import torch
    import torch.autograd.forward_ad as fwAD
    from fbstab_amd import autograd as ag
    name = "double_integrator"             # (one model for all trajectories; trajectory 2 retires at step 0)
    p, A, B, w = csh.setup(name)
    cm = solver(p.sizes())
    data = {k: _dev(a) for k, a in p.arrays.items()}
    At, Bt, wt = _dev(A[0]), _dev(B[0]), _dev(w[:SIX])
    rng = np.random.default_rng(71)
    qref = _dev(p.arrays["q"][None] + 0.05 * rng.standard_normal((SIX,) + p.arrays["q"].shape))
    tx0, tw, tq = _dev(rng.standard_normal(p.arrays["x0"].shape)), _dev(rng.standard_normal(w[:SIX].shape)), _dev(
        rng.standard_normal(tuple(qref.shape)))
    tA, tB = _dev(rng.standard_normal(A[0].shape)), _dev(rng.standard_normal(B[0].shape))
    with fwAD.dual_level():
        dual = dict(data)
        dual["x0"] = fwAD.make_dual(data["x0"], tx0)
        u, x, out = ag.closed_loop_condensed_mpc(cm, dual, fwAD.make_dual(At, tA), fwAD.make_dual(Bt, tB), SIX,
                                                 w=fwAD.make_dual(wt, tw), ref=dict(q=fwAD.make_dual(qref, tq)))
        du, dx = fwAD.unpack_dual(u).tangent, fwAD.unpack_dual(x).tangent
        up, xp = fwAD.unpack_dual(u).primal, fwAD.unpack_dual(x).primal
    torch.cuda.synchronize()
    # the same sweep and the method by hand
    point = [torch.zeros((p.batch, n), dtype=torch.float64, device="cuda") for n in (p.nz, p.nl, p.nv, p.nv)]
    d0 = {k: a.clone() for k, a in data.items()}
    r = cm.RecedingSweep(d0, *point, At, Bt, SIX, w=wt, log=("x", "U", "v"), ref=dict(q=qref))
    assert torch.equal(r["u"], up)
    gone = (r["eflag"] == -1)
    assert gone.any() and not gone.all()
    fold = torch.einsum("ij,kbj->kbi", tA, r["x"]) + torch.einsum("ij,kbj->kbi", tB, r["u"])
    dw = tw + torch.where(gone[:, :, None], torch.zeros_like(fold), fold)
    t = cm.RecedingSweepTangent(data, At, Bt, SIX, {k: r[k] for k in ("x", "U", "v", "eflag")}, dx0=tx0, dw=dw,
                                dref=dict(q=tq), ref=dict(q=qref))
    torch.cuda.synchronize()
    assert du is not None and torch.equal(du, t["du"]) and torch.equal(dx, t["dx"])
    assert du.abs().max() > 0 and not du[:, 2].any()
    # a plant of every trajectory's own: its tangent has that shape and folds row by row
    A3, B3 = _dev(A), _dev(B)
    tA3, tB3 = _dev(rng.standard_normal(A.shape)), _dev(rng.standard_normal(B.shape))
    with fwAD.dual_level():
        u3, x3, _ = ag.closed_loop_condensed_mpc(cm, data, fwAD.make_dual(A3, tA3), fwAD.make_dual(B3, tB3), SIX, w=wt)
        du3, dx3 = fwAD.unpack_dual(u3).tangent, fwAD.unpack_dual(x3).tangent
    r3 = cm.RecedingSweep({k: a.clone() for k, a in data.items()}, *[torch.zeros_like(a) for a in point], A3, B3, SIX,
                          w=wt, log=("x", "U", "v"))
    fold3 = torch.einsum("bij,kbj->kbi", tA3, r3["x"]) + torch.einsum("bij,kbj->kbi", tB3, r3["u"])
    fold3 = torch.where((r3["eflag"] == -1)[:, :, None], torch.zeros_like(fold3), fold3)
    t3 = cm.RecedingSweepTangent(data, A3, B3, SIX, {k: r3[k] for k in ("x", "U", "v", "eflag")}, dw=fold3)
    torch.cuda.synchronize()
    assert torch.equal(du3, t3["du"]) and torch.equal(dx3, t3["dx"]) and du3.abs().max() > 0
    with fwAD.dual_level():
        dual = dict(data)
        dual["Q"] = fwAD.make_dual(data["Q"], torch.zeros_like(data["Q"]))
        with pytest.raises(NotImplementedError, match="matrix sequence 'Q'"):
            ag.closed_loop_condensed_mpc(cm, dual, At, Bt, SIX)


def test_backward_with_a_loss_on_u_alone_or_on_x_alone_is_the_method(hip):
    """The function no longer materialises absent seeds (``jvp`` must tell an absent tangent from a zero one): a loss
    on ``u`` alone hands ``backward`` gx = None, one on ``x`` alone gu = None, and ``RecedingSweepAdjoint`` reads None
    as zeros - the gradients are that method's with explicit zeros, bit for bit."""
    import torch
    from fbstab_amd import autograd as ag
    name = "double_integrator"
    p, A, B, w = csh.setup(name)
    cm = solver(p.sizes())
    cu, cx = seeds(p, seed=33)
    At, Bt, wt = _dev(A[0]), _dev(B[0]), _dev(w[:SIX])
    for which in ("u", "x"):
        data = {k: _dev(a) for k, a in p.arrays.items()}
        for k in ("q", "x0"):
            data[k].requires_grad_(True)
        u, x, out = ag.closed_loop_condensed_mpc(cm, data, At, Bt, SIX, w=wt)
        ((_dev(cu) * u).sum() if which == "u" else (_dev(cx) * x).sum()).backward()
        point = [torch.zeros((p.batch, n), dtype=torch.float64, device="cuda") for n in (p.nz, p.nl, p.nv, p.nv)]
        r = cm.RecedingSweep({k: a.detach().clone() for k, a in data.items()}, *point, At, Bt, SIX, w=wt,
                             log=("x", "U", "v"))
        gu = _dev(cu) if which == "u" else torch.zeros_like(_dev(cu))
        gx = _dev(cx) if which == "x" else torch.zeros_like(_dev(cx))
        g = cm.RecedingSweepAdjoint({k: a.detach() for k, a in data.items()}, At, Bt, SIX,
                                    {k: r[k] for k in ("x", "U", "v", "eflag")}, gu=gu, gx=gx, want=("q",))
        torch.cuda.synchronize()
        assert g["q"].abs().max() > 0
        for k in ("q", "x0"):
            assert torch.equal(data[k].grad, g[k]), (which, k)


# ---- 8. central differences ----------------------------------------------------------------------------------------------
def test_central_differences_on_the_device(hip):
    """h = 1e-5 along x0, w and q on ``small`` with the forward run through ``CondensedMpc.RecedingSweep`` at
    abs_tol = 1e-11: |fd - ad| <= 1e-4 max(|ad|, 1e-2 sum of the magnitudes of ad's terms) for L = <cu, u> + <cx, x>,
    the step and the bound of the adjoint's central-difference test.  Trajectories whose exit flags or active sets
    differ between the two perturbed runs are left out, at most 1 in 5 - by the oracle's loop alone first."""
    import torch
    from oracle.oracle_py import default_options
    from fbstab_amd.condense import CondensedMpc
    p, A, B, w, cu, cx, dirs = sth.fd_setup()
    T = mah.FD_STEPS
    cap = p.batch // 5
    by_oracle = sth.fd_left_out(p, sth.fd_runs(sth.oracle_sweep(p, A, B), p, w, dirs))
    print("left out by the oracle's loop:", by_oracle)
    assert len(by_oracle) <= cap, by_oracle
    cm = CondensedMpc(*p.sizes(), max_batch=p.batch)
    _LIVE.append(cm)
    cm.dense.UpdateOptions(default_options(abs_tol=1e-11))

    def sweep(arr, ww):
        point = [torch.zeros((p.batch, n), dtype=torch.float64, device="cuda") for n in (p.nz, p.nl, p.nv, p.nv)]
        d = {k: _dev(a) for k, a in arr.items()}
        r = cm.RecedingSweep(d, *point, _dev(A), _dev(B), T, w=_dev(ww), log=("x", "U", "v"))
        torch.cuda.synchronize()
        lg = {k: r[k].cpu().numpy() for k in ("u", "x", "U", "v", "eflag")}
        lg["x_end"], lg["arrays"] = d["x0"].cpu().numpy(), arr
        return lg
    base = sweep(p.arrays, w)
    runs = sth.fd_runs(sweep, p, w, dirs)
    left = sth.fd_left_out(p, runs)
    print("left out on the device:", left)
    assert len(left) <= cap, left
    dlog = {k: torch.from_numpy(base[k]).cuda() for k in ("x", "U", "v", "eflag")}
    loss = lambda lg: (cu * lg["u"]).sum(axis=(0, 2)) + (cx * np.concatenate([lg["x"][1:], lg["x_end"][None]], 0)).sum(axis=(0, 2))
    for name, d in dirs.items():
        kw = dict(dx0=_dev(d)) if name == "x0" else dict(dw=_dev(d)) if name == "w" else dict(ddata=dict(q=_dev(d)))
        t = cm.RecedingSweepTangent({k: _dev(a) for k, a in p.arrays.items()}, _dev(A), _dev(B), T, dlog, **kw)
        torch.cuda.synchronize()
        du, dx = t["du"].cpu().numpy(), t["dx"].cpu().numpy()
        assert not t["status"].cpu().numpy().any()
        fd = (loss(runs[name][0]) - loss(runs[name][1])) / (2 * mah.FD_H)
        for q in range(p.batch):
            if q in left:
                continue
            ad = float((cu[:, q] * du[:, q]).sum() + (cx[:, q] * dx[:, q]).sum())
            bound = 1e-4 * max(abs(ad), 1e-2 * float(np.abs(cu[:, q] * du[:, q]).sum() + np.abs(cx[:, q] * dx[:, q]).sum()))
            print("%-2s traj %d: fd %+.6e ad %+.6e bound %.2e" % (name, q, fd[q], ad, bound))
            assert abs(fd[q] - ad) <= bound, (name, q, fd[q], ad, bound)
