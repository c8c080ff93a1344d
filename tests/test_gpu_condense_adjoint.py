"""The adjoint of the condensed MPC route on the device (fbstab_hip_mpc_condensed_adjoint_batch,
``CondensedMpc.Adjoint``, ``autograd.solve_condensed_mpc``): the two kernels against the rounding rules of the
condensing maps on the pseudo-data problem, the dense step against the dense rule, the gradients against the table,
the placements of the C-ABI, a known answer, the distance to ``FBstabMpcBatch.Adjoint`` against the measured bias of
the regularisation, and torch's backward against the method.  Points come from ``CondensedMpc.Solve``."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import condense_adjoint_helpers as cah
from tests import condense_helpers as ch
from tests import helpers as H
from tests import linear_reference as lr
from tools import fixtures as fx

pytestmark = pytest.mark.gpu
MPC_NAMES = ch.MPC_NAMES
SHAPES = ("tiny", "small", "odd33", "flat", "four_wave")
ADJ = ("dz", "dl", "dv")
NAN = float("nan")


@pytest.fixture(scope="module")
def hip():
    from fbstab_amd import hip_api
    hip_api.load_library()
    return hip_api


def _shared_model(p):
    """A batch that shares its model: the matrices of QP 0 as ONE (1, len) image each, and QP 0's vectors for every
    QP with x0 moved a little (each QP of ``p`` is feasible for its own matrices only)."""
    B = p.batch
    arrays = {k: (np.ascontiguousarray(a[:1]) if k in ch.MATRIX_NAMES else np.ascontiguousarray(np.repeat(a[:1], B, axis=0)))
              for k, a in p.arrays.items()}
    arrays["x0"] = arrays["x0"] * (1.0 - 0.02 * np.arange(B))[:, None]
    return fx.MpcProblem(*p.sizes(), arrays)


def _per_qp(p):
    """... and with those images repeated for every QP."""
    B = p.arrays["x0"].shape[0]
    return fx.MpcProblem(*p.sizes(), {k: np.ascontiguousarray(np.repeat(a, B // a.shape[0], axis=0))
                                      for k, a in p.arrays.items()})


@functools.lru_cache(maxsize=None)
def solved(name, shared=False):
    """(problem, point (z, l, v), condensed images as the device left them, seeds) of the fixture: solved once by
    ``CondensedMpc.Solve``, shared by the tests, left unchanged."""
    from fbstab_amd.condense import CondensedMpc
    p = ch.problem(name)
    if shared:
        p = _shared_model(p)
    B = p.arrays["x0"].shape[0]
    cm = CondensedMpc(*p.sizes(), max_batch=B)
    z, l, v, y = (np.zeros((B, n)) for n in (cm.nz, cm.nl, cm.nv, cm.nv))
    out = cm.Solve({k: np.ascontiguousarray(a) for k, a in p.arrays.items()}, z, l, v, y)
    assert (out["eflag"] == 0).all(), out["eflag"]
    img = {k: cm._img[k].cpu().numpy() for k in ("H", "f", "A", "b")}
    cm.close()
    rng = np.random.default_rng(41)
    seeds = (rng.standard_normal((B, cm.nz)), rng.standard_normal((B, cm.nl)), rng.standard_normal((B, cm.nv)))
    return p, (z, l, v), img, seeds


def _padded(a, pad, fill=NAN):
    import torch
    a = np.asarray(a, dtype=np.float64)
    t = torch.full((a.shape[0], a.shape[1] + pad), fill, dtype=torch.float64, device="cuda")
    t[:, :a.shape[1]] = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t


def raw(hip, handle, p, img, x, seeds, qps=None, pad=0, want=MPC_NAMES, adj=True, sigma=0.0, batch=None):
    """One call of fbstab_hip_mpc_condensed_adjoint_batch on device copies (the QPs ``qps``): dict rc, the gradients,
    dz, dl, dv, status and the work arrays U, gU, dU, gvc, dvc, rU, eU, ev as the device left them; every output is pre-filled
    with NaN and carries ``pad`` more doubles per QP than its length.  A (1, len) array of ``p`` or ``img`` beside
    more QPs is passed with stride 0; a None seed is a NULL slot."""
    import torch
    lib = hip.load_library()
    Bp = p.arrays["x0"].shape[0]
    qps = list(range(Bp)) if qps is None else list(qps)
    B = len(qps)
    N, nx, nu, nc = p.sizes()
    nzc, nv = (N + 1) * nu, (N + 1) * nc
    lens = p.seq_lengths()
    keep = []

    def dev(a):
        t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()
        keep.append(t)
        return t

    data = hip._MpcBatch()
    for i, k in enumerate(MPC_NAMES):
        a = p.arrays[k]
        t = dev(a if a.shape[0] == 1 else a[qps])
        data.base[i], data.stride[i] = t.data_ptr(), (0 if (a.shape[0] == 1 and Bp > 1) else t.shape[1])
    dense = hip._DenseBatch()
    for k, i in (("H", 0), ("f", 1), ("A", 4), ("b", 5)):
        a = img[k]
        t = dev(a if a.shape[0] == 1 else a[qps])
        dense.base[i], dense.stride[i] = t.data_ptr(), (0 if (a.shape[0] == 1 and Bp > 1) else t.shape[1])
    xb, sb, ab = hip._VarBatch(), hip._VarBatch(), hip._VarBatch()
    for i, a in enumerate(x):
        t = _padded(a[qps], pad, 7.0)
        keep.append(t)
        xb.base[i], xb.stride[i] = t.data_ptr(), t.shape[1]
    for i, a in enumerate(seeds):
        if a is not None:
            t = _padded(a[qps], pad, 7.0)
            keep.append(t)
            sb.base[i], sb.stride[i] = t.data_ptr(), t.shape[1]
    out = {}
    grad = hip._MpcGradBatch()
    for i, k in enumerate(MPC_NAMES):
        if k in want:
            out[k] = torch.full((B, lens[k] + pad), NAN, dtype=torch.float64, device="cuda")
            grad.base[i], grad.stride[i] = out[k].data_ptr(), lens[k] + pad
    if adj:
        for i, (k, n) in enumerate(zip(ADJ, (p.nz, p.nl, p.nv))):
            out[k] = torch.full((B, n + pad), NAN, dtype=torch.float64, device="cuda")
            ab.base[i], ab.stride[i] = out[k].data_ptr(), n + pad
    per = 5 * nzc + 3 * nv
    work = torch.full((B * per + 4,), NAN, dtype=torch.float64, device="cuda")
    status = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    rc = lib.fbstab_hip_mpc_condensed_adjoint_batch(
        handle, N, nx, nu, nc, B if batch is None else batch, C.byref(data), C.byref(dense), C.byref(xb), C.byref(sb),
        C.c_double(sigma), C.byref(grad), C.byref(ab) if adj else None, C.c_void_p(work.data_ptr()),
        C.c_void_p(status.data_ptr()), None)
    torch.cuda.synchronize()
    res = {k: t.cpu().numpy() for k, t in out.items()}
    w = work.cpu().numpy()
    o = 0
    for k, n in (("U", nzc), ("gU", nzc), ("dU", nzc), ("gvc", nv), ("dvc", nv), ("rU", nzc), ("eU", nzc), ("ev", nv)):
        res[k] = w[o:o + B * n].reshape(B, n)
        o += B * n
    res["work_tail"] = w[o:]
    res["status"] = status.cpu().numpy()
    res["rc"] = rc
    res["msg"] = lib.fbstab_hip_last_error().decode()
    return res


def _handle(hip, p, max_batch=None):
    N, nx, nu, nc = p.sizes()
    B = p.arrays["x0"].shape[0]
    return hip.FBstabDenseBatch((N + 1) * nu, 0, (N + 1) * nc, max_batch=max_batch or B)


def _same_bits(a, b, names, rows_a=slice(None), rows_b=slice(None), lens=None):
    for k in names:
        n = a[k].shape[1] if lens is None else lens[k]
        assert a[k][rows_a, :n].tobytes() == b[k][rows_b, :n].tobytes(), k


# ---- 1. the rounding rules on the device ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", SHAPES)
def test_kernels_meet_the_rounding_rules(hip, oracle, name):
    """The seed kernel's outputs and the finish kernel's (dz, dl) within the rounding rules of the condensing maps on
    the pseudo-data problem, the gradients the table of the returned step, and the dense step (dU, dv) within the dense
    adjoint's rule: its residual at most 3 x the oracle's.
    (dU, dv) is the dense adjoint's step after its one refinement step; the step before it is (dU - eU, dv - ev) up
    to the rounding of the sum, and its residual is printed beside the refined one.  Ratios: LABNOTES.md."""
    p, x, img, seeds = solved(name)
    d = _handle(hip, p)
    res = raw(hip, d._h, p, img, x, seeds)
    d.close()
    assert res["rc"] == 0, res["msg"]
    assert (res["status"] == 0).all() and np.isnan(res["work_tail"]).all()
    pp = cah.pseudo_problem(p, *seeds)
    dense = ch.condensed_problem(p, img)
    e0 = np.zeros(0)
    dense_rule = []
    for q in range(p.batch):
        xq = tuple(t[q] for t in x)
        # the seed kernel: the condense rule on the pseudo-data problem (names f, b), and U
        assert res["U"][q].tobytes() == ch.u_of(p, x[0][q:q + 1])[0].tobytes()
        assert cah.seed_violations(res["gU"][q], res["gvc"][q], pp, q) == [], q
        # the dense step: the dense rule, residual within 3 x the oracle's
        xc, sc = (res["U"][q], e0, xq[2]), (res["gU"][q], e0, res["gvc"][q])
        r_dev = lr.adjoint_residual(dense, q, xc, (res["dU"][q], e0, res["dvc"][q]), sc)
        r_orc = lr.adjoint_residual(dense, q, xc, lr.oracle_adjoint(oracle, dense, q, xc, sc), sc)
        r_raw = lr.adjoint_residual(dense, q, xc, (res["dU"][q] - res["eU"][q], e0, res["dvc"][q] - res["ev"][q]), sc)
        print(name, q, "dense residual", r_dev, "oracle's", r_orc, "ratio", r_dev / r_orc, "unrefined", r_raw)
        dense_rule.append((q, r_dev, r_orc))
        # the finish kernel, fed the device's own (dU, dv): the expand rule on the pseudo-data problem
        assert cah.finish_violations(res["dz"][q], res["dl"][q], pp, q, res["dU"][q], res["dvc"][q]) == [], q
        assert res["dv"][q].tobytes() == res["dvc"][q].tobytes()
        assert ch.u_of(p, res["dz"][q:q + 1])[0].tobytes() == res["dU"][q].tobytes()
        # the gradients: the table of the returned step
        step = tuple(res[k][q] for k in ADJ)
        tab = lr.mpc_gradient_table(p, xq, step)
        scale = max(np.abs(np.concatenate(step)).max(), 1.0) * max(np.abs(np.concatenate(xq)).max(), 1.0)
        for k in MPC_NAMES:
            np.testing.assert_allclose(res[k][q], tab[k], rtol=1e-13, atol=1e-15 * scale, err_msg=k)
    assert all(r_dev <= 3 * r_orc for _, r_dev, r_orc in dense_rule), dense_rule


# ---- 2. placement and determinism -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "odd33", "four_wave"])
def test_placements_and_determinism(hip, name):
    p, x, img, seeds = solved(name)
    lens = dict(p.seq_lengths(), dz=p.nz, dl=p.nl, dv=p.nv)
    names = MPC_NAMES + ADJ
    d = _handle(hip, p)
    res = raw(hip, d._h, p, img, x, seeds)
    again = raw(hip, d._h, p, img, x, seeds)
    assert res["rc"] == 0 and again["rc"] == 0, res["msg"]
    _same_bits(res, again, names + ("U", "gU", "dU", "gvc", "dvc"))
    # a QP's bits do not depend on its batch
    for q in (0, p.batch - 1):
        alone = raw(hip, d._h, p, img, x, seeds, qps=[q])
        assert alone["rc"] == 0, alone["msg"]
        _same_bits(alone, res, names, rows_b=slice(q, q + 1))
    # strided x, seed, grad and adj: the same bits, and the doubles between two slots are untouched
    padded = raw(hip, d._h, p, img, x, seeds, pad=3)
    assert padded["rc"] == 0, padded["msg"]
    _same_bits(padded, res, names, lens=lens)
    for k in names:
        assert np.isnan(padded[k][:, lens[k]:]).all(), (k, "the doubles between two slots were written")
    # a subset of the slots, no adj, NULL gl and gv against zero arrays
    some = raw(hip, d._h, p, img, x, seeds, want=("Q", "B", "x0"), adj=False)
    assert some["rc"] == 0 and set(some) & set(names) == {"Q", "B", "x0"}
    _same_bits(some, res, ("Q", "B", "x0"))
    null = raw(hip, d._h, p, img, x, (seeds[0], None, None))
    zero = raw(hip, d._h, p, img, x, (seeds[0], np.zeros_like(seeds[1]), np.zeros_like(seeds[2])))
    assert null["rc"] == 0 and zero["rc"] == 0
    _same_bits(null, zero, names + ("gU", "gvc"))
    assert any(null[k].tobytes() != res[k].tobytes() for k in MPC_NAMES)
    d.close()


@pytest.mark.parametrize("name", ["small", "flat", "four_wave"])
def test_shared_model_with_one_image_equals_the_per_qp_images(hip, name):
    p, x, img, seeds = solved(name, shared=True)
    assert img["H"].shape[0] == 1 and img["A"].shape[0] == 1 and img["f"].shape[0] == p.batch
    d = _handle(hip, p)
    one = raw(hip, d._h, p, img, x, seeds)
    B = p.batch
    rep = {k: np.ascontiguousarray(np.repeat(a, B // a.shape[0], axis=0)) for k, a in img.items()}
    per = raw(hip, d._h, _per_qp(p), rep, x, seeds)
    d.close()
    assert one["rc"] == 0 and per["rc"] == 0, (one["msg"], per["msg"])
    assert (one["status"] == 0).all()
    _same_bits(one, per, MPC_NAMES + ADJ)


def test_handle_checks(hip):
    p, x, img, seeds = solved("small")
    d = _handle(hip, p)
    wrong = hip.FBstabDenseBatch(p.N * p.nu, 0, p.nv, max_batch=p.batch)
    with_l = hip.FBstabDenseBatch((p.N + 1) * p.nu, 1, p.nv, max_batch=p.batch)
    for h, word in ((wrong._h, "dense handle"), (with_l._h, "dense handle"), (None, "null dense solver handle")):
        r = raw(hip, h, p, img, x, seeds)
        assert r["rc"] == 1 and word in r["msg"], r["msg"]
        assert all(np.isnan(r[k]).all() for k in MPC_NAMES + ADJ)
    small = _handle(hip, p, max_batch=p.batch - 1)
    r = raw(hip, small._h, p, img, x, seeds)
    assert r["rc"] == 1 and "max_batch" in r["msg"], r["msg"]
    r = raw(hip, d._h, p, img, x, seeds, batch=0)          # OK, and queues nothing
    assert r["rc"] == 0 and all(np.isnan(r[k]).all() for k in MPC_NAMES + ADJ) and (r["status"] == -1).all()
    for s in (d, wrong, with_l, small):
        s.close()


# ---- 3. a known answer ------------------------------------------------------------------------------------------------
def test_lqr_gain_from_seeded_input_rows(hip):
    """All constraints inactive ((8, 4, 2, 1), seed 4401): with gz the unit vectors of u_0, the x0 gradients are the
    rows of du0/dx0 = -K_0 of the Riccati recursion (helpers.lqr_gain)."""
    from oracle.oracle_py import default_options
    from fbstab_amd.condense import CondensedMpc
    N, nx, nu, nc = 8, 4, 2, 1
    p = fx.random_ltv_mpc(np.random.default_rng(4401), 1, N, nx, nu, nc)
    for k in ("q", "r", "c"):
        p.arrays[k][:] = 0.0
    p.arrays["E"][:] = 0.0
    p.arrays["L"][:] = 0.0
    p.arrays["d"][:] = -1.0   # 0 <= 1 on every row: inactive, y = 1, v = 0
    K = H.lqr_gain(p)
    data = {k: np.ascontiguousarray(np.repeat(a, nu, axis=0)) for k, a in p.arrays.items()}
    cm = CondensedMpc(N, nx, nu, nc, max_batch=nu)
    cm.dense.UpdateOptions(default_options(abs_tol=1e-11))
    z, l, v, y = (np.zeros((nu, n)) for n in (cm.nz, cm.nl, cm.nv, cm.nv))
    out = cm.Solve(data, z, l, v, y)
    assert (out["eflag"] == 0).all()
    np.testing.assert_allclose(z[0][nx:nx + nu], K @ p.arrays["x0"][0], rtol=1e-6, atol=1e-9)
    gz = np.zeros((nu, cm.nz))
    gz[np.arange(nu), nx + np.arange(nu)] = 1.0
    g = cm.Adjoint(data, z, l, v, gz, want=("x0",))
    cm.close()
    assert set(g) == {"x0", "status"} and (g["status"] == 0).all()
    np.testing.assert_allclose(g["x0"], K, rtol=1e-6, atol=1e-9 * np.abs(K).max())


# ---- 4. agreement with the MPC adjoint ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "flat", "four_wave"])
def test_agrees_with_the_mpc_adjoint_up_to_the_sigma_bias(hip, name):
    """Same points and seeds on ``FBstabMpcBatch.Adjoint``.  The allowance: 10 x the largest gap between the chain and
    the solve of the MPC system V on these very points, both in longdouble on the CPU (the pure sigma bias: V is
    regularised in (z, l) there and in U here), plus the forward error 1e-5 max(|step|, 1) of check_step_and_table.
    Measured gaps: LABNOTES.md (condensed adjoint)."""
    from fbstab_amd.condense import CondensedMpc
    p, x, img, seeds = solved(name)
    data = {k: np.ascontiguousarray(a) for k, a in p.arrays.items()}
    cm = CondensedMpc(*p.sizes(), max_batch=p.batch)
    cm.Condense(data)
    got = cm.Adjoint(data, *x, *seeds, adj=True)
    cm.close()
    m = hip.FBstabMpcBatch(*p.sizes(), max_batch=p.batch)
    ref = m.Adjoint(data, *x, *seeds, adj=True)
    m.close()
    assert (got["status"] == 0).all() and (ref["status"] == 0).all()
    gaps = [cah.sigma_gap(p, q, tuple(t[q] for t in x), tuple(t[q] for t in seeds)) for q in range(p.batch)]
    bias = max(g for g, _ in gaps)
    for q in range(p.batch):
        a, b = (np.concatenate([r[k][q] for k in ADJ]) for r in (got, ref))
        smax = max(np.abs(b).max(), 1.0)
        dist = np.abs(a - b).max()
        print(name, q, "sigma gap (longdouble)", gaps[q][0], "max|step|", gaps[q][1], "device distance", dist,
              "allowed", 10 * bias + 1e-5 * smax)
        assert dist <= 10 * bias + 1e-5 * smax, (q, dist, bias, smax)


# ---- 5. autograd ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "four_wave"])
def test_autograd_backward_is_the_adjoint_bit_for_bit(hip, name):
    import torch
    from fbstab_amd.autograd import solve_condensed_mpc
    from fbstab_amd.condense import CondensedMpc
    p = ch.problem(name)
    B = p.batch
    cm = CondensedMpc(*p.sizes(), max_batch=B)
    no_grad = ("R", "d")
    data = {k: torch.from_numpy(np.ascontiguousarray(a)).cuda().requires_grad_(k not in no_grad)
            for k, a in p.arrays.items()}
    z, l, v, out = solve_condensed_mpc(cm, data)
    assert (hip.out_to_numpy(out)["eflag"] == 0).all()
    rng = np.random.default_rng(51)
    wz, wl, wv = (torch.from_numpy(rng.standard_normal(t.shape)).cuda() for t in (z, l, v))
    asked = []
    method = cm.Adjoint
    cm.Adjoint = lambda *a, **kw: (asked.append(tuple(kw["want"])), method(*a, **kw))[1]
    ((wz * z).sum() + (wl * l).sum() + (wv * v).sum()).backward()
    cm.Adjoint = method
    want = tuple(k for k in MPC_NAMES if k not in no_grad)
    assert asked == [want]                                   # ONE call, the gradients torch asks for
    det = {k: t.detach() for k, t in data.items()}
    g = cm.Adjoint(det, z.detach(), l.detach(), v.detach(), wz, wl, wv, want=want)
    assert (g["status"] == 0).all()
    for k in MPC_NAMES:
        if k in no_grad:
            assert data[k].grad is None, k
        else:
            assert data[k].grad.cpu().numpy().tobytes() == g[k].cpu().numpy().tobytes(), k
    # a loss of z alone: the other seeds travel as NULL
    x0 = det["x0"].clone().requires_grad_(True)
    z2, _, _, _ = solve_condensed_mpc(cm, dict(det, x0=x0))
    assert z2.detach().cpu().numpy().tobytes() == z.detach().cpu().numpy().tobytes()
    gx0, = torch.autograd.grad((wz * z2).sum(), [x0])
    g2 = cm.Adjoint(det, z2.detach(), l.detach(), v.detach(), wz, want=("x0",))
    assert gx0.cpu().numpy().tobytes() == g2["x0"].cpu().numpy().tobytes()
    cm.close()


def test_autograd_shared_inputs_get_the_batch_sum(hip):
    import torch
    from fbstab_amd.autograd import solve_condensed_mpc
    from fbstab_amd.condense import CondensedMpc
    p, _, _, _ = solved("small", shared=True)
    B = p.batch
    cm = CondensedMpc(*p.sizes(), max_batch=B)
    data = {k: torch.from_numpy(np.ascontiguousarray(a)).cuda() for k, a in p.arrays.items()}
    data["Q"] = data["Q"].reshape(-1)                          # (len,) and (1, len) are both shared
    for k in ("Q", "A", "E", "q", "x0"):
        data[k].requires_grad_(True)
    z, l, v, out = solve_condensed_mpc(cm, data)
    assert (hip.out_to_numpy(out)["eflag"] == 0).all()
    rng = np.random.default_rng(52)
    wz, wl, wv = (torch.from_numpy(rng.standard_normal(t.shape)).cuda() for t in (z, l, v))
    gQ, gA, gE, gq, gx0 = torch.autograd.grad((wz * z).sum() + (wl * l).sum() + (wv * v).sum(),
                                              [data[k] for k in ("Q", "A", "E", "q", "x0")])
    det = {k: t.detach().reshape(1, -1) if t.dim() == 1 else t.detach() for k, t in data.items()}
    g = cm.Adjoint(det, z.detach(), l.detach(), v.detach(), wz, wl, wv, want=("Q", "A", "E", "q", "x0"))
    assert gQ.shape == data["Q"].shape and gA.shape == (1, g["A"].shape[1]) and gq.shape == (B, g["q"].shape[1])
    for got, k in ((gQ, "Q"), (gA, "A"), (gE, "E")):
        assert got.cpu().numpy().tobytes() == g[k].sum(0).reshape(got.shape).cpu().numpy().tobytes(), k
    for got, k in ((gq, "q"), (gx0, "x0")):
        assert got.cpu().numpy().tobytes() == g[k].cpu().numpy().tobytes(), k
    cm.close()
