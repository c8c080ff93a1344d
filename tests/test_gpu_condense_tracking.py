"""Per-step references on the condensed route on the device (fbstab_hip_mpc_condensed_reference_images_batch,
fbstab_hip_mpc_condensed_tracking_sweep, fbstab_hip_mpc_condensed_tracking_sweep_adjoint; ``CondensedMpc.ReferenceImages``,
``RecedingSweep(ref=...)``, ``RecedingSweepAdjoint(ref=...)``, ``autograd.closed_loop_condensed_mpc(ref=...)``): the
images against a loop over the VECTORS kernel bit for bit, RECONDENSE mode against a loop over the public calls bit for
bit, AFFINE mode against the reference loop of tests/condense_tracking_helpers.py, references equal to the data's
against the calls without references bit for bit (forward and reverse), the per-step gradients against the longdouble
recursion and against central differences, autograd, and asynchrony."""
import ctypes as C
import functools

import numpy as np
import pytest

from fbstab_amd.hip_api import MPC_SEQ
from tests import condense_helpers as ch
from tests import condense_sweep_adjoint_helpers as sah
from tests import condense_sweep_helpers as sh
from tests import condense_tracking_helpers as th
from tests import sweep_adjoint_helpers as mah

pytestmark = pytest.mark.gpu
LD = ch.LD
STEPS = th.STEPS
SIX = th.ADJOINT_STEPS
REF = th.REF_NAMES
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
def solver(sizes):
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
    sweep.cache_clear()
    forward.cache_clear()


def _data(p, qps=None):
    return {k: _dev(a if qps is None else a[qps]) for k, a in p.arrays.items()}


def _ref(name, steps=STEPS, qps=None, names=REF):
    r = th.references(name)
    return {k: _dev(r[k][:steps] if qps is None else r[k][:steps, qps]) for k in names}


# ---- 4. the images ----------------------------------------------------------------------------------------------------
def vectors_loop(cm, p, ref, steps, qps=None):
    """f0, b0 ``(steps, batch, n)`` from ``Condense(data_k with x0 = 0, "vectors")`` step by step."""
    import torch
    d = _data(p, qps)
    d["x0"] = torch.zeros_like(d["x0"])
    f0, b0 = [], []
    for k in range(steps):
        dk = dict(d)
        for n, a in ref.items():
            dk[n] = a[k].expand(d["x0"].shape[0], -1).contiguous()
        img = cm.Condense(dk, "vectors")
        f0.append(img["f"].clone()); b0.append(img["b"].clone())
    torch.cuda.synchronize()
    return torch.stack(f0).cpu().numpy(), torch.stack(b0).cpu().numpy()


@pytest.mark.parametrize("name", th.LOOP_FIXTURES)
def test_images_are_the_vectors_kernel_step_by_step(hip, name):
    import torch
    p = sh.setup(name)[0]
    cm = solver(p.sizes())
    ref = _ref(name)
    f0, b0 = vectors_loop(cm, p, ref, STEPS)
    for R in (1, 2, 0):
        im = cm.ReferenceImages(_data(p), ref, refs_per_group=R)
        torch.cuda.synchronize()
        assert im["f0"].cpu().numpy().tobytes() == f0.tobytes(), R
        assert im["b0"].cpu().numpy().tobytes() == b0.tobytes(), R
    # a trajectory alone gives the bits it has in the batch
    im = cm.ReferenceImages(_data(p, [3]), _ref(name, qps=[3]))
    assert im["f0"].cpu().numpy()[:, 0].tobytes() == np.ascontiguousarray(f0[:, 3]).tobytes()
    assert im["b0"].cpu().numpy()[:, 0].tobytes() == np.ascontiguousarray(b0[:, 3]).tobytes()
    # one (steps, 1, len) reference for the batch, and a sequence without a reference
    one = {"q": ref["q"][:, :1], "d": ref["d"]}
    im = cm.ReferenceImages(_data(p), one)
    fs, bs = vectors_loop(cm, p, one, STEPS)
    assert im["f0"].cpu().numpy().tobytes() == fs.tobytes() and im["b0"].cpu().numpy().tobytes() == bs.tobytes()
    assert fs.tobytes() != f0.tobytes()
    # padded output rows and strided reference rows: the same bits, and the pad survives
    lib = hip.load_library()
    d = cm._data(_data(p))
    nzc, nv, pad = cm.nzc, cm.nv, 3
    fo = torch.full((STEPS, p.batch, nzc + pad), np.nan, dtype=torch.float64, device="cuda")
    bo = torch.full((STEPS, p.batch, nv + pad), np.nan, dtype=torch.float64, device="cuda")
    wide = {}
    for k, a in ref.items():
        wide[k] = torch.full((STEPS, p.batch, a.shape[2] + 2), np.nan, dtype=torch.float64, device="cuda")
        wide[k][:, :, :a.shape[2]] = a
    blk, _ = cm._refs({k: a[:, :, :ref[k].shape[2]] for k, a in wide.items()}, STEPS, p.batch)
    im = hip._CondensedRefImages(fo.data_ptr(), bo.data_ptr(), p.batch * (nzc + pad), p.batch * (nv + pad), nzc + pad,
                                 nv + pad)
    mb = cm._mpc_block(d, p.batch)
    rc = lib.fbstab_hip_mpc_condensed_reference_images_batch(*p.sizes(), p.batch, STEPS, C.byref(mb), C.byref(blk),
                                                             C.byref(im), 0, 0, None)
    torch.cuda.synchronize()
    assert rc == 0, lib.fbstab_hip_last_error()
    fo, bo = fo.cpu().numpy(), bo.cpu().numpy()
    assert np.ascontiguousarray(fo[:, :, :nzc]).tobytes() == f0.tobytes() and np.isnan(fo[:, :, nzc:]).all()
    assert np.ascontiguousarray(bo[:, :, :nv]).tobytes() == b0.tobytes() and np.isnan(bo[:, :, nv:]).all()


# ---- the sweeps the tests share ------------------------------------------------------------------------------------
def run_sweep(name, mode, shift=False, T=0, ref="tracked", steps=STEPS):
    """``CondensedMpc.RecedingSweep`` on ``sh.setup(name)`` from a zero guess with the references of
    tests/condense_tracking_helpers.py (``ref``: "tracked", None, or a dict of device tensors): the returned dict as
    numpy arrays plus the point left in the caller's arrays and ``x_end``."""
    import torch
    from fbstab_amd import hip_api
    p, A, B, w = sh.setup(name)
    cm = solver(p.sizes())
    data = _data(p)
    point = [torch.zeros((p.batch, m), dtype=torch.float64, device="cuda") for m in (p.nz, p.nl, p.nv, p.nv)]
    rf = _ref(name, steps) if isinstance(ref, str) else ref
    r = cm.RecedingSweep(data, *point, _dev(A), _dev(B), steps, w=_dev(w[:steps]), shift=shift, mode=mode,
                         log=("x", "U", "v"), traj_per_group=T, ref=rf)
    torch.cuda.synchronize()
    res = {k: (hip_api.out_to_numpy(a) if k == "out" else a.cpu().numpy()) for k, a in r.items()}
    res.update(z_end=point[0].cpu().numpy(), l_end=point[1].cpu().numpy(), v_end=point[2].cpu().numpy(),
               y_end=point[3].cpu().numpy(), x_end=data["x0"].cpu().numpy())
    return res


@functools.lru_cache(maxsize=None)
def sweep(name, mode, shift=False):
    """Computed once, shared by the tests, left unchanged."""
    return run_sweep(name, mode, shift)


KEYS = ("u", "x", "U", "v", "eflag", "newton", "z_end", "l_end", "v_end", "y_end", "x_end")


def _same(a, b, keys=KEYS):
    return [k for k in keys if np.asarray(a[k]).tobytes() != np.asarray(b[k]).tobytes()]


def _check_plant(name, r):
    """x_log[k + 1] and x_end within the plant bound of (x_log[k], u_log[k], w_k); zero once gone."""
    p, A, B, w = sh.setup(name)
    steps = r["x"].shape[0]
    for k in range(steps):
        ref, S = sh.plant_reference(A, B, r["x"][k], r["u"][k], w[k])
        nxt = r["x"][k + 1] if k + 1 < steps else r["x_end"]
        live = r["eflag"][k] != -1
        assert (np.abs(nxt.astype(LD) - ref)[live] <= sh.plant_bound(p.nx, p.nu, S)[live]).all(), (name, k)
        assert (nxt[~live] == 0.0).all() and (r["u"][k][~live] == 0.0).all()


# ---- 5. RECONDENSE mode is the public calls with the step's sequences, bit for bit -----------------------------------
@pytest.mark.parametrize("name", th.LOOP_FIXTURES)
@pytest.mark.parametrize("shift", [False, True])
def test_tracked_recondense_sweep_is_a_loop_over_the_public_calls(hip, name, shift):
    import torch
    p, A, B, w = sh.setup(name)
    sizes = p.sizes()
    N, nx, nu, nc = sizes
    r = sweep(name, "recondense", shift)
    assert sh.retirement(r["eflag"]) == th.RETIRES[name]
    assert ((r["eflag"] == 0) | (r["eflag"] == -1)).all()
    _check_plant(name, r)
    assert (r["u"] == r["U"][:, :, :nu]).all()
    cm = solver(sizes)
    data = _data(p)
    ref = _ref(name)
    cm.Condense(data)
    U, v = np.zeros((p.batch, (N + 1) * nu)), np.zeros((p.batch, p.nv))
    for k in range(STEPS):
        if k > 0:
            U, v = r["U"][k - 1].copy(), r["v"][k - 1].copy()
            if shift:
                sh.shift_condensed(U, v, sizes)
        z = np.zeros((p.batch, N + 1, nx + nu))
        z[:, :, nx:] = U.reshape(p.batch, N + 1, nu)
        data["x0"] = _dev(r["x"][k])
        for n in REF:                                    # the swap: step k's sequences
            data[n] = ref[n][k]
        zd, ld, vd, yd = _dev(z.reshape(p.batch, -1)), _dev(np.zeros((p.batch, p.nl))), _dev(v), _dev(np.zeros_like(v))
        out = hip.out_to_numpy(cm.Solve(data, zd, ld, vd, yd, recondense="vectors"))
        torch.cuda.synchronize()
        gone = r["eflag"][k] == -1
        assert np.array_equal(out["newton_iters"], r["newton"][k]), k
        assert np.array_equal(out["eflag"][~gone], r["eflag"][k][~gone]), k
        first = gone & ((r["eflag"][k - 1] != -1) if k > 0 else True)
        assert (out["eflag"][first] != 0).all()
        Uk, vk = ch.u_of(p, zd.cpu().numpy()), vd.cpu().numpy()
        assert Uk[~gone].tobytes() == r["U"][k][~gone].tobytes() and vk[~gone].tobytes() == r["v"][k][~gone].tobytes(), k
        assert (r["U"][k][gone] == 0).all() and (r["v"][k][gone] == 0).all()
        if k + 1 == STEPS:
            # the point left in (z, l, v, y): the expansion of the last logged point with the LAST step's sequences
            ze, le, ve, ye = cm.Expand(data, _dev(r["U"][k]), _dev(r["v"][k]), _dev(r["y_end"]))
            for got, want in ((r["z_end"], ze), (r["l_end"], le), (r["v_end"], ve), (r["y_end"], ye)):
                assert got.tobytes() == want.cpu().numpy().tobytes()
            assert r["y_end"][~gone].tobytes() == yd.cpu().numpy()[~gone].tobytes()
            assert r["out"]["eflag"].tolist() == out["eflag"].tolist()


# ---- 6. AFFINE mode against the reference loop on the tracked problem -----------------------------------------------
@pytest.mark.parametrize("name", th.LOOP_FIXTURES)
@pytest.mark.parametrize("shift", [False, True])
def test_tracked_affine_sweep_against_the_reference_loop(name, shift):
    ref = th.oracle_loop(name, shift)
    assert sh.retirement(ref["eflag"]) == th.RETIRES[name]
    a, rcd = sweep(name, "affine", shift), sweep(name, "recondense", shift)
    assert np.array_equal(a["eflag"], ref["eflag"])
    _check_plant(name, a)
    g_a, g_r = sh.gap(a["u"], ref["u"]), sh.gap(rcd["u"], ref["u"])
    g_fma = sh.gap(th.oracle_loop(name, shift, "fma")["u"], ref["u"])
    g_aff_ref = sh.gap(th.oracle_loop(name, shift, "affine")["u"], ref["u"])
    floor = STEPS * 2.0 ** -52
    print(name, "shift" if shift else "unshifted", "g_a", g_a, "g_r", g_r, "g_fma", g_fma, "g_aff_ref", g_aff_ref,
          "floor", floor)
    assert g_a <= 10 * max(g_r, g_fma, g_aff_ref, floor)
    assert np.array_equal(rcd["eflag"], ref["eflag"])


# ---- 7. references equal to the data's: the sweep without references, bit for bit -------------------------------------
def _own(name, steps, names=REF):
    """The data's own sequences at every step, as a view with step 0 (nothing is copied)."""
    p = sh.setup(name)[0]
    return {k: _dev(p.arrays[k])[None].expand(steps, -1, -1) for k in names}


@pytest.mark.parametrize("name", th.LOOP_FIXTURES)
@pytest.mark.parametrize("mode", ["affine", "recondense"])
def test_references_equal_to_the_data_change_no_bit(name, mode):
    base = run_sweep(name, mode, ref=None)
    for T in (1, 2, 0):
        r = run_sweep(name, mode, T=T, ref=_own(name, STEPS))
        assert _same(r, base) == [], (T, _same(r, base))
        for k in ("eflag", "newton_iters", "prox_iters", "residual"):
            assert r["out"][k].tobytes() == base["out"][k].tobytes(), (T, k)
    # ... and the references of the tests do change the loop
    assert "u" in _same(sweep(name, mode), base)


# ---- the adjoint ------------------------------------------------------------------------------------------------------
def seeds(p, steps=SIX, seed=21):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((steps, p.batch, p.nu)), rng.standard_normal((steps, p.batch, p.nx))


@functools.lru_cache(maxsize=None)
def forward(name, mode="affine", shift=False, tracked=True):
    r = run_sweep(name, mode, shift, ref="tracked" if tracked else None, steps=SIX)
    return {k: r[k] for k in ("u", "x", "U", "v", "eflag")}


def adjoint(name, log, gu, gx, mode="affine", ref=None, **kw):
    """``CondensedMpc.RecedingSweepAdjoint`` on device tensors; numpy arrays back."""
    import torch
    p, A, B, w = sh.setup(name)
    cm = solver(p.sizes())
    dlog = {k: torch.from_numpy(np.ascontiguousarray(log[k])).cuda() for k in ("x", "U", "v", "eflag")}
    kw.setdefault("want", DATA_SEQ)
    kw.setdefault("mu", True)
    g = cm.RecedingSweepAdjoint(_data(p), _dev(A), _dev(B), log["eflag"].shape[0], dlog, gu=_dev(gu), gx=_dev(gx),
                                mode=mode, ref=ref, **kw)
    torch.cuda.synchronize()
    return {k: a.cpu().numpy() for k, a in g.items()}


# ---- 8. references equal to the data's: the adjoint without references ---------------------------------------------------
@pytest.mark.parametrize("name", th.LOOP_FIXTURES)
@pytest.mark.parametrize("mode", ["affine", "recondense"])
def test_adjoint_with_references_equal_to_the_data_sums_to_the_existing_adjoint(name, mode):
    p = sh.setup(name)[0]
    log = forward(name, mode, tracked=False)
    gu, gx = seeds(p)
    base = adjoint(name, log, gu, gx, mode=mode)
    g = adjoint(name, log, gu, gx, mode=mode, ref=_own(name, SIX))
    for k in ("x0", "mu", "status") + tuple(k for k in DATA_SEQ if k not in REF):
        assert g[k].tobytes() == base[k].tobytes(), k
    gone = log["eflag"] != 0
    for k in REF:
        assert g[k].shape == (SIX,) + base[k].shape
        total = np.zeros_like(base[k])
        for step in range(SIX - 1, -1, -1):              # the order of the device's sums: last step first
            total = total + g[k][step]
        assert total.tobytes() == base[k].tobytes(), k
        assert not g[k][gone].any(), k
    assert base["q"].any() and (gone.any() or name == "four_wave")
    # two of the four move, the others are summed as before
    g2 = adjoint(name, log, gu, gx, mode=mode, ref=_own(name, SIX, ("q", "d")))
    for k in ("r", "c", "x0"):
        assert g2[k].tobytes() == base[k].tobytes(), k
    for k in ("q", "d"):
        assert g2[k].tobytes() == g[k].tobytes(), k


# ---- 9. moving references against the longdouble recursion ---------------------------------------------------------------
def tracked_recursion(name, step_fns, maps, log, gu, gx):
    """sah.reference_condensed_sweep_adjoint with the problem of step k used at step k: (summed gradients,
    per-step gradients of q, r, c, d ``(steps, batch, len)``, status, mu)."""
    p, A, B, w = sh.setup(name)
    lens = p.seq_lengths()
    per = {k: np.zeros((SIX, p.batch, lens[k]), dtype=LD) for k in REF}

    def fn(k, q, xk, U, v, gU):
        st, dU, dv, tab = step_fns[k](k, q, xk, U, v, gU)
        if st == 0:
            for n in REF:
                per[n][k, q] = tab[n]
        return st, dU, dv, tab
    grads, status, mu = sah.reference_condensed_sweep_adjoint(fn, p, A, B, maps, log, gu, gx)
    return grads, per, status, mu


def device_step(p, cm):
    """The per-step adjoint from the device's own ``CondensedMpc.Adjoint`` at the expanded logged point."""
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
@pytest.mark.parametrize("name", th.LOOP_FIXTURES)
def test_moving_references_against_the_longdouble_recursion(hip, name, mode, shift):
    """The rule of test_six_steps_against_the_longdouble_recursion with the problem of step k used at step k: g_ref is
    the gap between two numpy recursions at the same logged points, one over the device's own per-step
    ``CondensedMpc.Adjoint``, one over ``chain_reference`` in longdouble; every gradient's gap - the per-step ones step
    by step - is at most 10 max(g_ref, steps 2^-52), relative to its largest entry."""
    p, A, B, w = sh.setup(name)
    cm = solver(p.sizes())
    log = forward(name, mode, shift)
    assert sh.retirement(log["eflag"]) == th.RETIRES[name]
    gu, gx = seeds(p)
    g = adjoint(name, log, gu, gx, mode=mode, ref=_ref(name, SIX))
    maps = [(a[1], a[3]) for a in sh.condenser(name).affine()]
    steps_p = [th.problem_at(name, k) for k in range(SIX)]
    ref, ref_per, rstatus, rmu = tracked_recursion(name, [sah.chain_step(pk) for pk in steps_p], maps, log, gu, gx)
    M = cm.X0Map(_data(p))["M"].cpu().numpy()
    dmaps = [sh.map_parts(p, M[q]) for q in range(p.batch)]
    dev, dev_per, dstatus, _ = tracked_recursion(name, [device_step(pk, cm) for pk in steps_p], dmaps, log, gu, gx)
    floor = SIX * 2.0 ** -52
    assert np.array_equal(g["status"], rstatus) and np.array_equal(dstatus, rstatus)
    for q, k in sh.retirement(log["eflag"]).items():
        assert np.array_equal(g["mu"][k:, q], gx[k:, q])
    summed = [k for k in MPC_SEQ if k not in REF]
    g_ref, gaps = sah.rel_gaps(dev, ref), sah.rel_gaps(g, ref)
    for k in summed:
        print("%-17s %-10s shift %d %-2s gap %.3g g_ref %.3g" % (name, mode, shift, k, gaps[k], g_ref[k]))
        assert gaps[k] <= 10 * max(g_ref[k], floor), (k, gaps[k], g_ref[k])
    for step in range(SIX):
        at = lambda d: {k: d[k][step] for k in REF}
        g_ref_k, gaps_k = sah.rel_gaps(at(dev_per), at(ref_per)), sah.rel_gaps(at(g), at(ref_per))
        for k in REF:
            print("%-17s %-10s shift %d %-2s step %d gap %.3g g_ref %.3g" % (name, mode, shift, k, step, gaps_k[k], g_ref_k[k]))
            assert gaps_k[k] <= 10 * max(g_ref_k[k], floor), (k, step, gaps_k[k], g_ref_k[k])
            assert not g[k][step][log["eflag"][step] != 0].any(), (k, step)
    top = float(np.abs(rmu).max())
    assert float(np.abs(g["mu"].astype(LD) - rmu).max()) <= 10 * max(g_ref["x0"], floor) * max(top, 1.0)


# ---- 10. central differences ------------------------------------------------------------------------------------------------
def test_central_differences_along_the_references(hip):
    """The problem, step size and bound of test_central_differences_on_the_device, along one direction of the whole
    ``(steps, batch, len)`` q reference and one of d (the references start from the data's own sequences, so the
    trajectory and its strictly complementary steps are that test's)."""
    import torch
    from oracle.oracle_py import default_options
    from fbstab_amd.condense import CondensedMpc
    p, A, B, cu, cx, _ = mah.fd_problem()
    T = mah.FD_STEPS
    cm = CondensedMpc(*p.sizes(), max_batch=p.batch)
    _LIVE.append(cm)
    cm.dense.UpdateOptions(default_options(abs_tol=1e-11))
    base = {k: np.repeat(p.arrays[k][None], T, axis=0) for k in ("q", "d")}
    rng = np.random.default_rng(77)
    dirs = {k: rng.standard_normal(base[k].shape) for k in ("q", "d")}

    def run(ref):
        point = [torch.zeros((p.batch, n), dtype=torch.float64, device="cuda") for n in (p.nz, p.nl, p.nv, p.nv)]
        d = {k: _dev(a) for k, a in p.arrays.items()}
        r = cm.RecedingSweep(d, *point, _dev(A), _dev(B), T, log=("x", "U", "v"), ref={k: _dev(a) for k, a in ref.items()})
        torch.cuda.synchronize()
        return r, d["x0"].cpu().numpy()
    r, x_end = run(base)
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
                                {k: r[k] for k in ("x", "U", "v", "eflag")}, gu=_dev(cu), gx=_dev(cx), want=("q", "d"),
                                ref={k: _dev(a) for k, a in base.items()})
    torch.cuda.synchronize()
    assert not g["status"].cpu().numpy().any()
    grads = {k: g[k].cpu().numpy() for k in ("q", "d")}
    for name in ("q", "d"):
        assert grads[name].shape == base[name].shape
        L = []
        for sg in (1.0, -1.0):
            ref = dict(base)
            ref[name] = base[name] + sg * mah.FD_H * dirs[name]
            rr, xe = run(ref)
            u = rr["u"].cpu().numpy()
            x = np.concatenate([rr["x"].cpu().numpy()[1:], xe[None]], 0)
            L.append((cu * u).sum(axis=(0, 2)) + (cx * x).sum(axis=(0, 2)))
        fd = (L[0] - L[1]) / (2 * mah.FD_H)
        for q in good:
            ad = float((grads[name][:, q] * dirs[name][:, q]).sum())
            bound = 1e-4 * max(abs(ad), 1e-2 * np.abs(grads[name][:, q]).sum())
            print("%-2s traj %d: fd %+.6e ad %+.6e bound %.2e" % (name, q, fd[q], ad, bound))
            assert abs(fd[q] - ad) <= bound, (name, q, fd[q], ad, bound)


# ---- 11. autograd -----------------------------------------------------------------------------------------------------------
def test_autograd_backward_is_the_method(hip):
    """``closed_loop_condensed_mpc(ref=...)``: backward is ``RecedingSweepAdjoint(ref=...)``'s output bit for bit, a
    ``(steps, 1, len)`` reference gets the batch sum, and a reference passed as a sliding window over a longer tensor
    receives the folded gradient."""
    import torch
    from fbstab_amd import autograd as ag
    name = "double_integrator"             # (one model for all trajectories; trajectory 2 retires at step 0)
    p, A, B, w = sh.setup(name)
    N, nx, nu, nc = p.sizes()
    cm = solver(p.sizes())
    data = _data(p)
    full = _ref(name, SIX)
    # q: per trajectory; r: one for the batch; d: per trajectory; c: not tracked.  x0 and E of the data want gradients too
    # ... and the reference of q is a window of (N + 1) nx doubles sliding by nx over (SIX + N) nx doubles per trajectory
    long_q = torch.cat([full["q"][0], full["q"][1:, :, -nx:].permute(1, 0, 2).reshape(p.batch, -1)], 1).contiguous()
    long_q.requires_grad_(True)
    win = lambda t: torch.as_strided(t, (SIX, p.batch, (N + 1) * nx), (nx, t.stride(0), 1))
    ref = dict(q=win(long_q), r=full["r"][:, :1].clone().requires_grad_(True), d=full["d"].clone().requires_grad_(True))
    for k in ("x0", "E"):
        data[k].requires_grad_(True)
    At, Bt, wt = _dev(A[0]), _dev(B[0]), _dev(w[:SIX])
    cu, cx = seeds(p, seed=31)
    u, x, out = ag.closed_loop_condensed_mpc(cm, data, At, Bt, SIX, w=wt, ref=ref)
    ((_dev(cu) * u).sum() + (_dev(cx) * x).sum()).backward()
    torch.cuda.synchronize()
    # the same sweep and the method by hand
    point = [torch.zeros((p.batch, n), dtype=torch.float64, device="cuda") for n in (p.nz, p.nl, p.nv, p.nv)]
    d0 = {k: a.detach().clone() for k, a in data.items()}
    rd = {k: a.detach() for k, a in ref.items()}
    r = cm.RecedingSweep(d0, *point, At, Bt, SIX, w=wt, log=("x", "U", "v"), ref=rd)
    assert np.array_equal(r["u"].cpu().numpy(), u.detach().cpu().numpy())
    g = cm.RecedingSweepAdjoint({k: a.detach() for k, a in data.items()}, At, Bt, SIX,
                                {k: r[k] for k in ("x", "U", "v", "eflag")}, gu=_dev(cu), gx=_dev(cx),
                                want=("q", "r", "d", "E"), ref=rd)
    torch.cuda.synchronize()
    assert g["q"].shape == (SIX, p.batch, (N + 1) * nx) and g["r"].shape == (SIX, p.batch, (N + 1) * nu)
    assert torch.equal(ref["d"].grad, g["d"])
    assert torch.equal(ref["r"].grad, g["r"].sum(1, keepdim=True))
    for k in ("x0", "E"):
        assert torch.equal(data[k].grad, g[k]), k
    # the gradient is added where the windows overlap: at most SIX terms per entry, in an order that is torch's (its
    # scatter-add is atomic on the device), so each sum is within SIX roundings of the sum of the magnitudes
    gq = g["q"].cpu().numpy()
    fold, mag = np.zeros(tuple(long_q.shape), dtype=LD), np.zeros(tuple(long_q.shape), dtype=LD)
    for k in range(SIX):
        fold[:, k * nx:k * nx + (N + 1) * nx] += gq[k]
        mag[:, k * nx:k * nx + (N + 1) * nx] += np.abs(gq[k])
    got = long_q.grad.cpu().numpy()
    assert (np.abs(got.astype(LD) - fold) <= SIX * LD(2.0) ** -52 * mag).all() and np.abs(got).sum() > 0
    assert got[:, :nx].tobytes() == np.ascontiguousarray(gq[0][:, :nx]).tobytes()      # (one window: no sum)
    assert (r["eflag"] == -1).any() and not (r["eflag"] == -1).all()
    # the call forms without references keep working
    u0, x0, _ = ag.closed_loop_condensed_mpc(cm, {k: a.detach() for k, a in data.items()}, At, Bt, SIX, w=wt)
    assert not torch.equal(u0, u.detach())


# ---- 12. asynchrony -----------------------------------------------------------------------------------------------------------
def test_tracked_calls_do_not_wait_for_the_device(hip):
    import torch
    name = "small"
    p, A, B, w = sh.setup(name)
    cm = solver(p.sizes())
    point = [torch.zeros((p.batch, m), dtype=torch.float64, device="cuda") for m in (p.nz, p.nl, p.nv, p.nv)]
    Ad, Bd, wd = _dev(A), _dev(B), _dev(w)
    ref = _ref(name)
    base = sweep(name, "affine")
    log = forward(name)
    dlog = {k: torch.from_numpy(np.ascontiguousarray(log[k])).cuda() for k in ("x", "U", "v", "eflag")}
    gu, gx = (_dev(a) for a in seeds(p))
    ref6 = _ref(name, SIX)
    d1, d2, d3 = _data(p), _data(p), _data(p)
    calls = (lambda: cm.ReferenceImages(d1, ref),
             lambda: cm.RecedingSweep(d2, *point, Ad, Bd, STEPS, w=wd, log=("x",), ref=ref),
             lambda: cm.RecedingSweepAdjoint(d3, Ad, Bd, SIX, dlog, gu=gu, gx=gx, want=("q", "Q"), ref=ref6))
    for i, call in enumerate(calls):
        torch.cuda.synchronize()
        # a spin of some tens of milliseconds queued first: were the call to wait for the device or copy a result to
        # the host, it would return behind the spin; an event recorded right behind the call is still pending when
        # it returns without
        torch.cuda._sleep(50_000_000)
        r = call()
        done = torch.cuda.Event()
        done.record()
        pending = not done.query()
        torch.cuda.synchronize()
        assert pending, "call %d waited for the device" % i
        assert all(a.is_cuda for a in r.values())
        if i == 1:
            assert r["u"].cpu().numpy().tobytes() == base["u"].tobytes()
