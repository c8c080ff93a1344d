"""Many right-hand sides on the condensed MPC route on the device (fbstab_hip_mpc_condensed_kkt_solve_batch,
fbstab_hip_mpc_condensed_x0_sensitivity_batch, ``CondensedMpc.KktSolve`` / ``.X0Sensitivity``,
``autograd.condensed_mpc_x0_sensitivity``): the kernels against the rounding rules of the condensing maps on each
right-hand side's pseudo-data problem, the dense step against the dense rule, slot and grouping independence bit for
bit, the x0 mode against its explicit seeds, the placements of the C-ABI, a known answer, and the distance to
``FBstabMpcBatch`` against the measured bias of the regularisation.  Points come from ``CondensedMpc.Solve`` (those
of tests/test_gpu_condense_adjoint.py, solved once)."""
import ctypes as C

import numpy as np
import pytest

from tests import condense_adjoint_helpers as cah
from tests import condense_helpers as ch
from tests import condense_multi_helpers as cmh
from tests import helpers as H
from tests import linear_reference as lr
from tests import test_gpu_condense_adjoint as tga
from tools import fixtures as fx

pytestmark = pytest.mark.gpu
MPC_NAMES = ch.MPC_NAMES
SHAPES = ("tiny", "small", "odd33", "flat", "four_wave")
ADJ = ("dz", "dl", "dv")
NAN = float("nan")
NRHS = 5
solved = tga.solved


@pytest.fixture(scope="module")
def hip():
    from fbstab_amd import hip_api
    hip_api.load_library()
    return hip_api


def _random_seeds(p, seed=71, nrhs=NRHS):
    rng = np.random.default_rng(seed)
    B = p.arrays["x0"].shape[0]
    return tuple(rng.standard_normal((B, nrhs, n)) for n in (p.nz, p.nl, p.nv))


def _multi_dev(a, rpad, pad, fill):
    """(B, K, n) on the device with ``rpad`` more doubles behind every vector and ``pad`` more behind every QP."""
    import torch
    B, K, n = a.shape
    t = torch.full((B, K * (n + rpad) + pad), fill, dtype=torch.float64, device="cuda")
    t[:, :K * (n + rpad)].view(B, K, n + rpad)[:, :, :n] = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t


def raw(hip, handle, p, img, x, seeds=None, qps=None, pad=0, rpad=0, want=ADJ, gain=None, sigma=0.0, batch=None,
        rpg=0):
    """One call of fbstab_hip_mpc_condensed_kkt_solve_batch (``seeds`` = (gz, gl, gv): (B, K, n) arrays, a (K, n) array
    is ONE block passed with stride 0, None a NULL slot) or of fbstab_hip_mpc_condensed_x0_sensitivity_batch (``seeds``
    None) on device copies of the QPs ``qps``.  Every output is pre-filled with NaN; a step vector carries ``rpad``
    more doubles than its length and a QP's block ``pad`` more.  Returns dict rc, msg, status, dz, dl, dv (B, K, n),
    gain (B, nu nx), ``gaps`` (every double of the outputs that no vector owns) and the work arrays."""
    import torch
    lib = hip.load_library()
    Bp = p.arrays["x0"].shape[0]
    qps = list(range(Bp)) if qps is None else list(qps)
    B = len(qps)
    N, nx, nu, nc = p.sizes()
    nzc, nv = (N + 1) * nu, (N + 1) * nc
    x0_mode = seeds is None
    K = nx if x0_mode else next(s for s in seeds if s is not None).shape[-2]
    gain = x0_mode if gain is None else gain
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
    xb = hip._VarBatch()
    for i, a in enumerate(x):
        t = tga._padded(a[qps], pad, 7.0)
        keep.append(t)
        xb.base[i], xb.stride[i] = t.data_ptr(), t.shape[1]
    lens = (p.nz, p.nl, p.nv)
    sb, ob = hip._MultiVarBatch(), hip._MultiVarBatch()
    if not x0_mode:
        for i, (a, n) in enumerate(zip(seeds, lens)):
            if a is None:
                continue
            if a.ndim == 2:                           # one block shared by the batch
                t = _multi_dev(a[None], rpad, 0, 7.0)
                sb.stride[i] = 0
            else:
                t = _multi_dev(a[qps], rpad, pad, 7.0)
                sb.stride[i] = t.shape[1]
            keep.append(t)
            sb.base[i], sb.rhs_stride[i] = t.data_ptr(), n + rpad
    out = {}
    for i, (k, n) in enumerate(zip(ADJ, lens)):
        if k in want:
            out[k] = torch.full((B, K * (n + rpad) + pad), NAN, dtype=torch.float64, device="cuda")
            ob.base[i], ob.stride[i], ob.rhs_stride[i] = out[k].data_ptr(), out[k].shape[1], n + rpad
    g = torch.full((B, nu * nx + pad), NAN, dtype=torch.float64, device="cuda") if gain else None
    per = nzc + K * (4 * nzc + 3 * nv)
    work = torch.full((B * per + 4,), NAN, dtype=torch.float64, device="cuda")
    status = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    head = (handle, N, nx, nu, nc, B if batch is None else batch, C.byref(data), C.byref(dense), C.byref(xb))
    tail = (rpg, C.c_void_p(work.data_ptr()), C.c_void_p(status.data_ptr()), None)
    if x0_mode:
        rc = lib.fbstab_hip_mpc_condensed_x0_sensitivity_batch(
            *head, C.c_double(sigma), C.byref(ob) if want else None, C.c_void_p(g.data_ptr()) if gain else None,
            nu * nx + pad, *tail)
    else:
        rc = lib.fbstab_hip_mpc_condensed_kkt_solve_batch(*head, K, C.byref(sb), C.c_double(sigma), C.byref(ob), *tail)
    torch.cuda.synchronize()
    res = dict(rc=rc, msg=lib.fbstab_hip_last_error().decode(), status=status.cpu().numpy(), K=K)
    gaps = []
    for k, n in zip(ADJ, lens):
        if k in out:
            a = out[k].cpu().numpy()
            body = a[:, :K * (n + rpad)].reshape(B, K, n + rpad)
            res[k] = np.ascontiguousarray(body[:, :, :n])
            gaps += [body[:, :, n:].reshape(-1), a[:, K * (n + rpad):].reshape(-1)]
    if gain:
        a = g.cpu().numpy()
        res["gain"] = np.ascontiguousarray(a[:, :nu * nx])
        gaps.append(a[:, nu * nx:].reshape(-1))
    res["gaps"] = np.concatenate(gaps) if gaps else np.zeros(0)
    w = work.cpu().numpy()
    o = 0
    for k, n in (("U", nzc), ("gU", K * nzc), ("dU", K * nzc), ("rU", K * nzc), ("eU", K * nzc), ("gvc", K * nv),
                 ("dvc", K * nv), ("ev", K * nv)):
        res[k] = w[o:o + B * n].reshape((B, n) if k == "U" else (B, K, n // K))
        o += B * n
    res["work_tail"] = w[o:]
    return res


def _same_bits(a, b, names, rows_a=slice(None), rows_b=slice(None)):
    for k in names:
        assert np.ascontiguousarray(a[k][rows_a]).tobytes() == np.ascontiguousarray(b[k][rows_b]).tobytes(), k


def _untouched(r, names=ADJ + ("gain",)):
    return all(np.isnan(r[k]).all() for k in names if k in r) and np.isnan(r["gaps"]).all()


# ---- 1. the rules in x0 mode ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SHAPES)
def test_x0_mode_meets_the_rounding_rules(hip, oracle, name):
    """Every column of every QP: the seed kernel's (gU, gv_c) and the finish kernel's (dz, dl) within the rounding
    rules of the condensing maps on the column's pseudo-data problem (x0 := e_j), dv and the u rows of dz the work
    array's bits; and on columns {0, a middle one, nx - 1} the dense step within the dense rule, its residual at most
    3 x the oracle's.  Ratios: LABNOTES.md (condensed multi)."""
    p, x, img, _ = solved(name)
    d = tga._handle(hip, p)
    res = raw(hip, d._h, p, img, x)
    d.close()
    assert res["rc"] == 0, res["msg"]
    assert (res["status"] == 0).all() and np.isnan(res["work_tail"]).all() and np.isnan(res["gaps"]).all()
    unit = cmh.x0_seeds(p)
    dense = ch.condensed_problem(p, img)
    e0 = np.zeros(0)
    nx, nu = p.nx, p.nu
    dense_rule = []
    for q in range(p.batch):
        assert res["U"][q].tobytes() == ch.u_of(p, x[0][q:q + 1])[0].tobytes()
        assert res["dv"][q].tobytes() == res["dvc"][q].tobytes()
        assert ch.u_of(p, res["dz"][q]).tobytes() == res["dU"][q].tobytes()
        for j in range(nx):
            pp = cmh.slot_problem(p, q, unit, j)
            assert cah.seed_violations(res["gU"][q, j], res["gvc"][q, j], pp, 0) == [], (q, j)
            assert cah.finish_violations(res["dz"][q, j], res["dl"][q, j], pp, 0, res["dU"][q, j],
                                         res["dvc"][q, j]) == [], (q, j)
        for j in sorted({0, nx // 2, nx - 1}):
            xc, sc = (res["U"][q], e0, x[2][q]), (res["gU"][q, j], e0, res["gvc"][q, j])
            r_dev = lr.adjoint_residual(dense, q, xc, (res["dU"][q, j], e0, res["dvc"][q, j]), sc)
            r_orc = lr.adjoint_residual(dense, q, xc, lr.oracle_adjoint(oracle, dense, q, xc, sc), sc)
            r_raw = lr.adjoint_residual(dense, q, xc, (res["dU"][q, j] - res["eU"][q, j], e0,
                                                       res["dvc"][q, j] - res["ev"][q, j]), sc)
            print(name, q, "column", j, "dense residual", r_dev, "oracle's", r_orc, "ratio", r_dev / r_orc,
                  "unrefined", r_raw)
            dense_rule.append((q, j, r_dev, r_orc))
    assert all(r_dev <= 3 * r_orc for _, _, r_dev, r_orc in dense_rule), dense_rule


# ---- 2. slots and groupings -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "odd33", "four_wave"])
def test_kkt_solve_slots_do_not_depend_on_position_company_or_grouping(hip, name):
    from fbstab_amd.condense import CondensedMpc
    p, x, img, _ = solved(name)
    seeds = _random_seeds(p)
    data = {k: np.ascontiguousarray(a) for k, a in p.arrays.items()}
    cm = CondensedMpc(*p.sizes(), max_batch=p.batch)
    cm.Condense(data)
    base = cm.KktSolve(data, *x, *seeds)
    assert (base["status"] == 0).all() and all(base[k].shape == (p.batch, NRHS, n)
                                               for k, n in zip(ADJ, (p.nz, p.nl, p.nv)))
    assert all(np.abs(base[k]).max() > 0 for k in ADJ)
    perm = np.array([3, 0, 4, 2, 1])
    moved = cm.KktSolve(data, *x, *(s[:, perm] for s in seeds))
    alone = cm.KktSolve(data, *x, *(s[:, 3:4] for s in seeds))
    for k in ADJ:
        assert moved[k].tobytes() == np.ascontiguousarray(base[k][:, perm]).tobytes(), k
        assert alone[k].tobytes() == np.ascontiguousarray(base[k][:, 3:4]).tobytes(), k
    for rpg in (1, 2, 0):
        r = cm.KktSolve(data, *x, *seeds, rhs_per_group=rpg)
        assert all(r[k].tobytes() == base[k].tobytes() for k in ADJ), rpg
    cm.close()


# ---- 3. the x0 mode against explicit seeds --------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "odd33", "four_wave"])
def test_x0_sensitivity_is_kkt_solve_with_the_unit_seeds(hip, name):
    from fbstab_amd.condense import CondensedMpc
    p, x, img, _ = solved(name)
    nx, nu = p.nx, p.nu
    data = {k: np.ascontiguousarray(a) for k, a in p.arrays.items()}
    cm = CondensedMpc(*p.sizes(), max_batch=p.batch)
    cm.Condense(data)
    full = cm.X0Sensitivity(data, *x, want=("dz", "dl", "dv", "gain"))
    assert (full["status"] == 0).all() and full["gain"].shape == (p.batch, nu, nx)
    explicit = cm.KktSolve(data, *x, *cmh.x0_seeds(p))          # (one (nx, n) block shared by the batch)
    for k in ADJ:
        assert full[k].tobytes() == explicit[k].tobytes(), k
    rows = np.ascontiguousarray(full["dz"][:, :, nx:nx + nu].transpose(0, 2, 1))
    assert np.ascontiguousarray(full["gain"]).tobytes() == rows.tobytes()
    only = cm.X0Sensitivity(data, *x, want=("gain",))
    assert set(only) == {"gain", "status"}                       # (no dz buffer exists)
    assert np.ascontiguousarray(only["gain"]).tobytes() == np.ascontiguousarray(full["gain"]).tobytes()
    default = cm.X0Sensitivity(data, *x)
    assert set(default) == {"dz", "gain", "status"} and default["dz"].tobytes() == full["dz"].tobytes()
    cm.close()
    # the C-ABI: step == NULL queues no finish launch and leaves nothing but gain written
    d = tga._handle(hip, p)
    r = raw(hip, d._h, p, img, x, want=())
    d.close()
    assert r["rc"] == 0 and (r["status"] == 0).all() and np.isnan(r["gaps"]).all()
    # (gain is nu x nx column-major per QP: entry (r, j) at r + j nu)
    assert r["gain"].reshape(p.batch, nx, nu).tobytes() == np.ascontiguousarray(full["dz"][:, :, nx:nx + nu]).tobytes()


# ---- 4. placements and determinism ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "odd33"])
def test_placements_and_determinism(hip, name):
    p, x, img, _ = solved(name)
    seeds = _random_seeds(p)
    d = tga._handle(hip, p)
    res = raw(hip, d._h, p, img, x, seeds)
    again = raw(hip, d._h, p, img, x, seeds)
    assert res["rc"] == 0 and again["rc"] == 0, res["msg"]
    assert (res["status"] == 0).all()
    _same_bits(res, again, ADJ + ("U", "gU", "dU", "gvc", "dvc"))
    x0 = raw(hip, d._h, p, img, x)
    # a QP's bits do not depend on its batch
    for q in (0, p.batch - 1):
        alone = raw(hip, d._h, p, img, x, seeds, qps=[q])
        assert alone["rc"] == 0, alone["msg"]
        _same_bits(alone, res, ADJ, rows_b=slice(q, q + 1))
        alone = raw(hip, d._h, p, img, x, qps=[q])
        _same_bits(alone, x0, ADJ + ("gain",), rows_b=slice(q, q + 1))
    # padded stride and rhs_stride: the same bits, and the doubles between vectors and between QPs are untouched
    for kw in (dict(pad=3), dict(rpad=2), dict(pad=3, rpad=2)):
        padded = raw(hip, d._h, p, img, x, seeds, **kw)
        assert padded["rc"] == 0, padded["msg"]
        _same_bits(padded, res, ADJ)
        assert padded["gaps"].size > 0 and np.isnan(padded["gaps"]).all(), kw
        padded = raw(hip, d._h, p, img, x, **kw)
        _same_bits(padded, x0, ADJ + ("gain",))
        assert np.isnan(padded["gaps"]).all(), kw
    # NULL step slots are skipped; NULL gl and gv against zero arrays
    for want in (("dz",), ("dl",), ("dv",), ("dz", "dv")):
        some = raw(hip, d._h, p, img, x, seeds, want=want)
        assert some["rc"] == 0 and set(some) & set(ADJ) == set(want)
        _same_bits(some, res, want)
    null = raw(hip, d._h, p, img, x, (seeds[0], None, None))
    zero = raw(hip, d._h, p, img, x, (seeds[0], np.zeros_like(seeds[1]), np.zeros_like(seeds[2])))
    assert null["rc"] == 0 and zero["rc"] == 0
    _same_bits(null, zero, ADJ + ("gU", "gvc"))
    assert any(null[k].tobytes() != res[k].tobytes() for k in ADJ)
    # a shared seed block (stride 0) equals its repetition
    block = tuple(s[2] for s in seeds)
    shared = raw(hip, d._h, p, img, x, block)
    rep = raw(hip, d._h, p, img, x, tuple(np.ascontiguousarray(np.repeat(b[None], p.batch, axis=0)) for b in block))
    assert shared["rc"] == 0 and rep["rc"] == 0, shared["msg"]
    _same_bits(shared, rep, ADJ)
    d.close()


@pytest.mark.parametrize("name", ["small", "odd33"])
def test_shared_model_with_one_image_equals_the_per_qp_images(hip, name):
    p, x, img, _ = solved(name, shared=True)
    assert img["H"].shape[0] == 1 and img["A"].shape[0] == 1 and img["f"].shape[0] == p.batch
    seeds = _random_seeds(p)
    d = tga._handle(hip, p)
    B = p.batch
    rep = {k: np.ascontiguousarray(np.repeat(a, B // a.shape[0], axis=0)) for k, a in img.items()}
    for s in (seeds, None):
        one = raw(hip, d._h, p, img, x, s)
        per = raw(hip, d._h, tga._per_qp(p), rep, x, s)
        assert one["rc"] == 0 and per["rc"] == 0, (one["msg"], per["msg"])
        assert (one["status"] == 0).all()
        _same_bits(one, per, ADJ + (("gain",) if s is None else ()))
    d.close()


# ---- 5. handle checks -------------------------------------------------------------------------------------------------
def test_handle_checks(hip):
    p, x, img, _ = solved("small")
    seeds = _random_seeds(p)
    d = tga._handle(hip, p)
    wrong = hip.FBstabDenseBatch(p.N * p.nu, 0, p.nv, max_batch=p.batch)
    with_l = hip.FBstabDenseBatch((p.N + 1) * p.nu, 1, p.nv, max_batch=p.batch)
    small = tga._handle(hip, p, max_batch=p.batch - 1)
    for s in (seeds, None):
        for h, word in ((wrong._h, "dense handle"), (with_l._h, "dense handle"), (None, "null dense solver handle"),
                        (small._h, "max_batch")):
            r = raw(hip, h, p, img, x, s)
            assert r["rc"] == 1 and word in r["msg"], r["msg"]
            assert _untouched(r) and (r["status"] == -1).all()
        r = raw(hip, d._h, p, img, x, s, batch=0)          # OK, and queues nothing
        assert r["rc"] == 0 and _untouched(r) and (r["status"] == -1).all() and np.isnan(r["U"]).all()
    r = raw(hip, d._h, p, img, x, seeds, rpg=-1)
    assert r["rc"] == 1 and "rhs_per_group" in r["msg"] and _untouched(r)
    for s in (d, wrong, with_l, small):
        s.close()


# ---- 6. a known answer --------------------------------------------------------------------------------------------------
def test_gain_is_the_lqr_gain(hip):
    """All constraints inactive ((8, 4, 2, 1), seed 4401, the construction of test_lqr_gain_from_seeded_input_rows):
    gain = du0/dx0 = -K_0 of the Riccati recursion (helpers.lqr_gain)."""
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
    data = {k: np.ascontiguousarray(a) for k, a in p.arrays.items()}
    cm = CondensedMpc(N, nx, nu, nc, max_batch=1)
    cm.dense.UpdateOptions(default_options(abs_tol=1e-11))
    z, l, v, y = (np.zeros((1, n)) for n in (cm.nz, cm.nl, cm.nv, cm.nv))
    out = cm.Solve(data, z, l, v, y)
    assert (out["eflag"] == 0).all()
    g = cm.X0Sensitivity(data, z, l, v, want=("gain",))
    cm.close()
    assert (g["status"] == 0).all() and g["gain"].shape == (1, nu, nx)
    np.testing.assert_allclose(g["gain"][0], K, rtol=1e-6, atol=1e-9 * np.abs(K).max())


# ---- 7. agreement with FBstabMpcBatch -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "flat", "four_wave"])
def test_agrees_with_the_mpc_calls_up_to_the_sigma_bias(hip, name):
    """The same points on ``FBstabMpcBatch.X0Sensitivity`` and ``.KktSolve``.  The allowance is that of
    test_agrees_with_the_mpc_adjoint_up_to_the_sigma_bias: 10 x the largest gap between the chain and the solve of the
    MPC system V on these very points, both in longdouble on the CPU, plus the forward error 1e-5 max(|step|, 1).  The
    gap is measured for every random seed and for the x0 columns {0, a middle one, nx - 1} of every QP; every column
    is compared.  Measured gaps: LABNOTES.md (condensed multi)."""
    from fbstab_amd.condense import CondensedMpc
    p, x, img, _ = solved(name)
    seeds = _random_seeds(p)
    unit = cmh.x0_seeds(p)
    data = {k: np.ascontiguousarray(a) for k, a in p.arrays.items()}
    cm = CondensedMpc(*p.sizes(), max_batch=p.batch)
    cm.Condense(data)
    got = (cm.X0Sensitivity(data, *x, want=ADJ), cm.KktSolve(data, *x, *seeds))
    cm.close()
    m = hip.FBstabMpcBatch(*p.sizes(), max_batch=p.batch)
    ref = (m.X0Sensitivity(data, *x, want=ADJ), m.KktSolve(data, *x, *seeds))
    m.close()
    cols = sorted({0, p.nx // 2, p.nx - 1})
    for mode, a, b in zip(("x0", "kkt"), got, ref):
        assert (a["status"] == 0).all() and (b["status"] == 0).all()
        gaps = []
        for q in range(p.batch):
            xq = tuple(t[q] for t in x)
            these = [tuple(s[j] for s in unit) for j in cols] if mode == "x0" else \
                [tuple(s[q, k] for s in seeds) for k in range(NRHS)]
            gaps.append(max(cah.sigma_gap(p, q, xq, s)[0] for s in these))
        bias = max(gaps)
        for q in range(p.batch):
            sa, sb = (np.concatenate([r[k][q] for k in ADJ], axis=1) for r in (a, b))
            smax = max(np.abs(sb).max(), 1.0)
            dist = np.abs(sa - sb).max()
            print(name, mode, q, "sigma gap (longdouble)", gaps[q], "max|step|", smax, "device distance", dist,
                  "allowed", 10 * bias + 1e-5 * smax)
            assert dist <= 10 * bias + 1e-5 * smax, (mode, q, dist, bias, smax)


# ---- 8. autograd ----------------------------------------------------------------------------------------------------
def test_autograd_x0_sensitivity_returns_the_methods_tensors_detached(hip):
    import torch
    from fbstab_amd.autograd import condensed_mpc_x0_sensitivity
    from fbstab_amd.condense import CondensedMpc
    p, x, img, _ = solved("small")
    cm = CondensedMpc(*p.sizes(), max_batch=p.batch)
    data = {k: torch.from_numpy(np.ascontiguousarray(a)).cuda().requires_grad_(True) for k, a in p.arrays.items()}
    z, l, v = (torch.from_numpy(np.ascontiguousarray(t)).cuda().requires_grad_(True) for t in x)
    cm.Condense({k: t.detach() for k, t in data.items()})
    for ctx in (torch.enable_grad(), torch.no_grad()):
        with ctx:
            res = condensed_mpc_x0_sensitivity(cm, data, z, l, v)
        assert set(res) == {"dz", "dl", "dv", "gain", "status"}
        assert all(not t.requires_grad and t.grad_fn is None for t in res.values())
        assert (res["status"] == 0).all()
        ref = cm.X0Sensitivity({k: t.detach() for k, t in data.items()}, z.detach(), l.detach(), v.detach(),
                               want=("dz", "dl", "dv", "gain"))
        for k in ("dz", "dl", "dv", "gain"):
            assert res[k].shape == ref[k].shape
            assert res[k].contiguous().cpu().numpy().tobytes() == ref[k].contiguous().cpu().numpy().tobytes(), k
    cm.close()
