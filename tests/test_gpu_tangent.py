"""GPU tests of the forward mode (fbstab_hip_mpc_tangent_batch, fbstab_hip_dense_tangent_batch): the direction
kernels against the numpy reference on one shape per solve kernel, the step bitwise against the adjoint entry
point fed the returned seeds, queue and batch invariance, duality with the adjoint's gradients, a known answer,
statuses, and torch.autograd.forward_ad."""
import numpy as np
import pytest

from fbstab_amd.hip_api import MPC_SEQ, DENSE_ARR
from tools import fixtures as fx
from oracle.oracle_py import default_options
from tests import helpers as H
from tests import linear_reference as LR
from tests import tangent_helpers as TH
from tests.shapes import MPC_SHAPES, DENSE_KERNEL_SHAPES, RELAX_FROM, RELAX

pytestmark = pytest.mark.gpu

CAP = "FBSTAB_HIP_MAX_WORKGROUPS"
FLAT = "FBSTAB_HIP_FLAT_ADJOINT"
STEP = ("dz", "dl", "dv")
RHS = ("gz", "gl", "gv")
GENERIC = "fbstab_mpc_kernel<64>"


@pytest.fixture(scope="module")
def hip():
    from fbstab_amd import hip_api
    assert hip_api.load_library().fbstab_hip_device_count() >= 1
    return hip_api


def _arrays(p):
    return {k: np.ascontiguousarray(a) for k, a in p.arrays.items()}


def _check_rhs_and_step(s, p, x, d, res):
    """``res`` = Tangent(..., rhs=True): status 0, the seeds within the bound of tangent_helpers.tangent_rhs for every
    QP, and (dz, dl, dv) bitwise what Adjoint(adj=True) returns for those seeds.  Returns the worst error / bound."""
    assert (res["status"] == 0).all()
    worst = 0.0
    for q in range(p.batch):
        worst = max(worst, TH.assert_rhs(p, q, tuple(t[q] for t in x), TH.one_direction(d, q),
                                         tuple(res[k][q] for k in RHS)))
    adj = s.Adjoint(_arrays(p), *x, *(res[k] for k in RHS), want=(), adj=True)
    assert (adj["status"] == 0).all()
    for k in STEP:
        assert np.array_equal(res[k], adj[k]), k
    assert np.abs(res["dz"]).max() > 0
    return worst


_FIRST = [next(i for i, (_, n) in enumerate(MPC_SHAPES) if n == name) for name in dict.fromkeys(n for _, n in MPC_SHAPES)]
_MPC_RUNS = [(i, f) for i in _FIRST for f in (("0", "1") if MPC_SHAPES[i][1] != GENERIC else (None,))]


@pytest.mark.parametrize("idx,flat", _MPC_RUNS, ids=["%s-%s" % (MPC_SHAPES[i][1], {"0": "record", "1": "flat", None: "flat"}[f])
                                                      for i, f in _MPC_RUNS])
def test_tangent_on_one_shape_per_mpc_solve_kernel(hip, monkeypatch, idx, flat):
    """Three random LTV QPs at the device's solutions, per-QP random directions on all twelve sequences; the record
    instances once on their record adjoint (FBSTAB_HIP_FLAT_ADJOINT=0) and once on the flat-vector one (=1)."""
    shape, kern = MPC_SHAPES[idx]
    monkeypatch.setenv("FBSTAB_HIP_GENERIC", "1" if kern == GENERIC else "0")
    if flat is not None:
        monkeypatch.setenv(FLAT, flat)
    p = fx.random_ltv_mpc(np.random.default_rng(7100 + idx), 3, *shape)
    s, x, out = H.cold_solve(hip, p)
    assert s.kernel_name() == kern
    assert s.adjoint_kernel_name().startswith("fbstab_mpc_r16_adjoint_kernel" if flat == "0" else "fbstab_mpc_adjoint_kernel")
    d = TH.random_directions(np.random.default_rng(100 + idx), p, p.batch)
    res = s.Tangent(_arrays(p), *x, d, rhs=True)
    print("worst error / bound %.3f" % _check_rhs_and_step(s, p, x, d, res))
    assert s.last_kernel_ms() > 0


@pytest.mark.parametrize("idx", range(len(DENSE_KERNEL_SHAPES)), ids=["x".join(map(str, s[0])) for s in DENSE_KERNEL_SHAPES])
def test_tangent_on_every_dense_kernel(hip, idx):
    """The same on one shape per dense kernel (the v_global shape with the relaxation of the adjoint's test)."""
    (nz, nl, nv), threads, (kg, vg), _ = DENSE_KERNEL_SHAPES[idx]
    p = fx.synthetic_dense_batch(3, nz, nl, nv, first_id=500 + 10 * idx)
    if vg:
        p.arrays["b"] = p.arrays["b"].copy()
        p.arrays["b"][:, RELAX_FROM:] += RELAX
    s, x, out = H.cold_solve(hip, p)
    assert s.query()["threads"] == threads and (out["eflag"] == 0).all()
    d = TH.random_directions(np.random.default_rng(200 + idx), p, p.batch)
    res = s.Tangent(_arrays(p), *x, d, rhs=True)
    print("worst error / bound %.3f" % _check_rhs_and_step(s, p, x, d, res))


@pytest.mark.parametrize("shape,flat", [((5, 6, 3, 8), None), ((4, 13, 2, 6), "0")], ids=["one_row", "row_pair_record"])
def test_bits_are_the_same_alone_packed_and_on_the_full_grid(hip, monkeypatch, shape, flat):
    """24 QPs on two workgroups (every wavefront row fetching and re-fetching), on the whole grid, and QPs 0, 7,
    23 alone: the seeds and (dz, dl, dv) are the same bits.  A direction shared by the batch (stride 0) gives seeds
    within the bound of the same direction copied per QP."""
    if flat is not None:
        monkeypatch.setenv(FLAT, flat)
    p = fx.random_ltv_mpc(np.random.default_rng(5150 + shape[1]), 24, *shape)
    s, x, out = H.cold_solve(hip, p)
    if flat == "0":
        assert s.kernel_name().startswith("fbstab_mpc_r32_kernel") and s.adjoint_kernel_name().startswith("fbstab_mpc_r16_adjoint_kernel")
    d = TH.random_directions(np.random.default_rng(11), p, p.batch)
    full = s.Tangent(_arrays(p), *x, d, rhs=True)
    monkeypatch.setenv(CAP, "2")
    packed_h = hip.FBstabMpcBatch(*p.sizes(), max_batch=p.batch)
    assert packed_h.query()["workgroups"] == 2 < p.batch
    packed = packed_h.Tangent(_arrays(p), *x, d, rhs=True)
    monkeypatch.delenv(CAP)
    alone_h = hip.FBstabMpcBatch(*p.sizes(), max_batch=1)
    for q in (0, 7, 23):
        one = {k: np.ascontiguousarray(a[q:q + 1]) for k, a in p.arrays.items()}
        alone = alone_h.Tangent(one, *(t[q:q + 1] for t in x), {k: np.ascontiguousarray(a[q:q + 1]) for k, a in d.items()},
                                rhs=True)
        for k in RHS + STEP:
            assert np.array_equal(alone[k][0], full[k][q]), (q, k)
    for k in RHS + STEP + ("status",):
        assert np.array_equal(packed[k], full[k]), k
    shared = {k: np.ascontiguousarray(a[3:4]) for k, a in d.items()}
    copied = {k: np.ascontiguousarray(np.repeat(a[3:4], p.batch, axis=0)) for k, a in d.items()}
    a, b = s.Tangent(_arrays(p), *x, shared, rhs=True), s.Tangent(_arrays(p), *x, copied, rhs=True)
    for q in range(p.batch):
        xq, dq = tuple(t[q] for t in x), TH.one_direction(copied, q)
        TH.assert_rhs(p, q, xq, dq, tuple(a[k][q] for k in RHS), "shared")
        TH.assert_rhs(p, q, xq, dq, tuple(b[k][q] for k in RHS), "copied")


def _duality(names, g, res, grads, d, q):
    LD = np.longdouble
    gg = np.concatenate([t[q] for t in g]).astype(LD)
    dx = np.concatenate([res[k][q] for k in STEP]).astype(LD)
    return float(abs(gg @ dx - TH.pairing(names, grads, d, q)) / np.abs(gg * dx).sum())


def test_duality_with_the_adjoint_on_the_device_mpc(hip):
    """<seeds, Tangent> against sum_k <Adjoint's gradient_k, direction_k> on the first three QPs of the batch of the
    CPU test (random_ltv_mpc(default_rng(8801), 8, 6, 4, 2, 6), abs_tol 1e-11), directions on all twelve sequences
    (dQ, dR not symmetric: the adjoint returns the gradient of the symmetric part): within DUALITY_BAR."""
    rng = np.random.default_rng(8801)
    p8 = fx.random_ltv_mpc(rng, 8, 6, 4, 2, 6)
    p = fx.MpcProblem(*p8.sizes(), {k: np.ascontiguousarray(a[:3]) for k, a in p8.arrays.items()})
    s, x, out = H.cold_solve(hip, p, default_options(abs_tol=1e-11))
    assert (out["eflag"] == 0).all()
    d = TH.random_directions(rng, p, p.batch)
    g = LR.random_seeds(rng, p)
    res = s.Tangent(_arrays(p), *x, d)
    grads = s.Adjoint(_arrays(p), *x, *g)
    assert (res["status"] == 0).all() and (grads["status"] == 0).all()
    for q in range(p.batch):
        gap = _duality(MPC_SEQ, g, res, grads, d, q)
        print("duality gap %.2e (bar %.1e)" % (gap, TH.DUALITY_BAR))
        assert gap <= TH.DUALITY_BAR, (q, gap)


def test_duality_with_the_adjoint_on_the_device_dense(hip):
    """The same for the dense QP, three (20, 5, 40) QPs."""
    p = fx.synthetic_dense_batch(3, 20, 5, 40, first_id=40)
    s, x, out = H.cold_solve(hip, p)
    assert (out["eflag"] == 0).all()
    rng = np.random.default_rng(2054)
    d = TH.random_directions(rng, p, p.batch)
    g = LR.random_seeds(rng, p)
    res = s.Tangent(_arrays(p), *x, d)
    grads = s.Adjoint(_arrays(p), *x, *g)
    assert (res["status"] == 0).all() and (grads["status"] == 0).all()
    for q in range(p.batch):
        gap = _duality(DENSE_ARR, g, res, grads, d, q)
        print("duality gap %.2e (bar %.1e)" % (gap, TH.DUALITY_BAR))
        assert gap <= TH.DUALITY_BAR, (q, gap)


def test_lqr_gain_from_unit_directions_of_the_initial_state(hip):
    """All constraints inactive: the nx unit directions dx0 give the columns of du0/dx0 = -K_0 of the Riccati
    recursion in the u0 rows of dz - one copy of the QP per column, the problem data not duplicated per input."""
    N, nx, nu, nc = 8, 4, 2, 1
    p = fx.random_ltv_mpc(np.random.default_rng(4401), 1, N, nx, nu, nc)
    for k in ("q", "r", "c"):
        p.arrays[k][:] = 0.0
    p.arrays["E"][:] = 0.0
    p.arrays["L"][:] = 0.0
    p.arrays["d"][:] = -1.0   # 0 <= 1 on every row: inactive, y = 1, v = 0
    K = H.lqr_gain(p)
    s, x, out = H.cold_solve(hip, p, default_options(abs_tol=1e-11))
    assert (out["eflag"] == 0).all()
    np.testing.assert_allclose(x[0][0][nx:nx + nu], K @ p.arrays["x0"][0], rtol=1e-6, atol=1e-9)
    wide = hip.FBstabMpcBatch(N, nx, nu, nc, max_batch=nx)
    rep = lambda a: np.ascontiguousarray(np.repeat(a, nx, axis=0))
    res = wide.Tangent(_arrays(p), *(rep(t) for t in x), {"x0": np.eye(nx)})   # (the data: one QP, stride 0)
    assert (res["status"] == 0).all()
    np.testing.assert_allclose(res["dz"][:, nx:nx + nu].T, K, rtol=1e-6, atol=1e-9 * np.abs(K).max())


def test_failed_factorisation_host_and_device_pointers_and_an_empty_batch(hip):
    """The failed-factorisation setup of the dense adjoint's test (a NaN in H[0] of QP 1): status [0, 1, 0], a zero
    dx for QP 1, the others untouched by it.  The host-pointer call returns the bits of the device-pointer call.
    batch == 0 returns OK."""
    import torch
    dev = torch.device("cuda:0")
    p = fx.synthetic_dense_batch(3, 50, 10, 100, first_id=70)
    ref = fx.synthetic_dense_batch(3, 50, 10, 100, first_id=70)
    p.arrays["H"] = p.arrays["H"].copy()
    p.arrays["H"][1, 0] = np.nan
    s = hip.FBstabDenseBatch(p.nz, p.nl, p.nv, max_batch=3)
    x = tuple(np.ascontiguousarray(ref.solution[k]) for k in ("z", "l", "v"))
    d = TH.random_directions(np.random.default_rng(1), p, p.batch)
    res = s.Tangent(_arrays(p), *x, d, rhs=True)
    good = s.Tangent(_arrays(ref), *x, d, rhs=True)
    assert res["status"].tolist() == [0, 1, 0] and good["status"].tolist() == [0, 0, 0]
    for k in STEP:
        assert np.array_equal(res[k][1], np.zeros_like(res[k][1])), k
        assert np.array_equal(res[k][[0, 2]], good[k][[0, 2]]) and np.abs(good[k][1]).max() > 0, k
    for k in RHS:   # (the seeds do not depend on the problem data)
        assert np.array_equal(res[k], good[k]), k
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    on_dev = s.Tangent({k: t(a) for k, a in ref.arrays.items()}, *(t(a) for a in x), {k: t(a) for k, a in d.items()},
                       rhs=True)
    no_rhs = s.Tangent({k: t(a) for k, a in ref.arrays.items()}, *(t(a) for a in x), {k: t(a) for k, a in d.items()})
    torch.cuda.synchronize()
    for k in STEP + RHS + ("status",):
        assert np.array_equal(good[k], on_dev[k].cpu().numpy()), k
    for k in STEP:
        assert np.array_equal(good[k], no_rhs[k].cpu().numpy()), k
    # the same on an MPC handle, with half of the slots null
    m = fx.random_ltv_mpc(np.random.default_rng(31), 3, 4, 5, 2, 6)
    ms, mx, _ = H.cold_solve(hip, m)
    md = TH.random_directions(np.random.default_rng(2), m, m.batch, names=("Q", "S", "A", "c", "L", "x0"))
    host = ms.Tangent(_arrays(m), *mx, md, rhs=True)
    mdev = ms.Tangent({k: t(a) for k, a in m.arrays.items()}, *(t(a) for a in mx), {k: t(a) for k, a in md.items()}, rhs=True)
    torch.cuda.synchronize()
    for k in STEP + RHS + ("status",):
        assert np.array_equal(host[k], mdev[k].cpu().numpy()), k
    empty = lambda arrs: {k: np.ascontiguousarray(a)[:0] for k, a in arrs.items()}   # (no rows, a row's strides)
    none = ms.Tangent(empty(m.arrays), *(a[:0] for a in mx), empty(md), rhs=True)
    assert none["dz"].shape == (0, m.nz) and none["status"].shape == (0,)
    none = s.Tangent(empty(ref.arrays), *(a[:0] for a in x), empty(d))
    assert none["dz"].shape == (0, p.nz)


def _dual_run(torch, fwAD, solve, solver, prim, tang, grad_names):
    """solve(solver, data) inside a dual level with the inputs of ``tang`` dual; returns the tangents of (z, l, v)
    and, after a backward of a fixed linear loss, the gradients of ``grad_names``."""
    leaves = {k: a.clone().requires_grad_(k in grad_names) for k, a in prim.items()}
    with fwAD.dual_level():
        data = {k: (fwAD.make_dual(a, tang[k]) if k in tang else a) for k, a in leaves.items()}
        z, l, v, out = solve(solver, data)
        tz, tl, tv = (fwAD.unpack_dual(t).tangent for t in (z, l, v))
        loss = (z * z.detach().cos()).sum() + (l * 0.5).sum() + (v * v.detach().sin()).sum()
        loss.backward()
    return (z, l, v, out), (tz, tl, tv), {k: leaves[k].grad.clone() for k in grad_names}


def test_forward_ad_through_solve_mpc(hip):
    """Under forward_ad.dual_level, tangents on a per-QP x0 and a Q shared by the batch equal the C-ABI call's
    (bitwise); the QP that runs into max_newton_iters gets zero tangents; and the backward's results are bitwise
    those of a run without any dual tensor."""
    import torch
    import torch.autograd.forward_ad as fwAD
    from fbstab_amd.autograd import solve_mpc
    dev = torch.device("cuda:0")
    N, nx, nu, nc = 6, 4, 2, 6
    p = fx.random_ltv_mpc(np.random.default_rng(6161), 3, N, nx, nu, nc)
    p.arrays["x0"][1] *= 5.0
    solver = hip.FBstabMpcBatch(N, nx, nu, nc, max_batch=3)
    solver.UpdateOptions(hip.DefaultOptions(max_newton_iters=10))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    prim = {k: t(a) for k, a in p.arrays.items()}
    prim["Q"] = prim["Q"][0:1].clone()   # one Q for the whole batch
    rng = np.random.default_rng(77)
    tang = {"x0": t(rng.standard_normal((3, nx))), "Q": t(rng.standard_normal((1, p.seq_lengths()["Q"])))}
    (z, l, v, out), tans, grads = _dual_run(torch, fwAD, solve_mpc, solver, prim, tang, ("Q", "x0", "d"))
    eflag = hip.out_to_numpy(out)["eflag"]
    assert eflag.tolist() == [0, 2, 0], eflag
    ref = solver.Tangent(prim, z.detach(), l.detach(), v.detach(), tang)
    torch.cuda.synchronize()
    for tn, k in zip(tans, STEP):
        a, b = tn.cpu().numpy(), ref[k].cpu().numpy()
        assert np.array_equal(a[[0, 2]], b[[0, 2]]) and np.abs(b[[0, 2]]).max() > 0, k
        assert not a[1].any(), k   # (whatever the library computed at that point)
    # the backward without any dual tensor
    plain = {k: a.clone().requires_grad_(k in grads) for k, a in prim.items()}
    z2, l2, v2, _ = solve_mpc(solver, plain)
    ((z2 * z2.detach().cos()).sum() + (l2 * 0.5).sum() + (v2 * v2.detach().sin()).sum()).backward()
    torch.cuda.synchronize()
    for k in grads:
        assert np.array_equal(grads[k].cpu().numpy(), plain[k].grad.cpu().numpy()), k
        assert grads[k].shape == prim[k].shape


def test_forward_ad_through_solve_dense(hip):
    """Tangents on f and on an H shared by the batch equal the C-ABI call's, and the backward is unchanged."""
    import torch
    import torch.autograd.forward_ad as fwAD
    from fbstab_amd.autograd import solve_dense
    dev = torch.device("cuda:0")
    nz, nl, nv = 20, 5, 40
    p = fx.synthetic_dense_batch(3, nz, nl, nv, first_id=60)
    solver = hip.FBstabDenseBatch(nz, nl, nv, max_batch=3)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    prim = {k: t(a) for k, a in p.arrays.items()}
    prim["H"] = prim["H"][0:1].clone()
    rng = np.random.default_rng(78)
    tang = {"f": t(rng.standard_normal((3, nz))), "H": t(rng.standard_normal((1, nz * nz)))}
    (z, l, v, out), tans, grads = _dual_run(torch, fwAD, solve_dense, solver, prim, tang, ("H", "f", "b"))
    assert (hip.out_to_numpy(out)["eflag"] == 0).all()
    ref = solver.Tangent(prim, z.detach(), l.detach(), v.detach(), tang)
    torch.cuda.synchronize()
    for tn, k in zip(tans, STEP):
        assert np.array_equal(tn.cpu().numpy(), ref[k].cpu().numpy()) and np.abs(ref[k].cpu().numpy()).max() > 0, k
    plain = {k: a.clone().requires_grad_(k in grads) for k, a in prim.items()}
    z2, l2, v2, _ = solve_dense(solver, plain)
    ((z2 * z2.detach().cos()).sum() + (l2 * 0.5).sum() + (v2 * v2.detach().sin()).sum()).backward()
    torch.cuda.synchronize()
    for k in grads:
        assert np.array_equal(grads[k].cpu().numpy(), plain[k].grad.cpu().numpy()), k
