"""GPU checks of the dense many-right-hand-side solves (fbstab_hip_dense_kkt_solve_batch,
fbstab_hip_dense_jacobian_batch, FBstabDenseBatch.KktSolve / Jacobian, fbstab_amd.autograd.dense_jacobian): every
right-hand side against the oracle's linear solver on one shape per dense kernel and, on the four-wavefront
kernels, bitwise against the adjoint; slot independence on the one-wavefront kernel; the Jacobian mode against the
seeded mode, the tangent, closed forms and central differences through the device solver; placement and statuses."""
import numpy as np
import pytest

from tools import fixtures as fx
from oracle.oracle_py import default_options
from tests import helpers as H
from tests import linear_reference as LR
from tests import dense_kkt_multi_helpers as KH
from tests.dense_kkt_multi_helpers import STEP
from tests.hostsim import HostAdjoint
from tests.shapes import DENSE_KERNEL_SHAPES, RELAX_FROM, RELAX
from tests.test_gpu_dense_adjoint import FWD_FACTOR, _spd

pytestmark = pytest.mark.gpu

CAP = "FBSTAB_HIP_MAX_WORKGROUPS"
THREADS = "FBSTAB_HIP_DENSE_THREADS"
B = 3


@pytest.fixture(scope="module")
def hip():
    from fbstab_amd import hip_api
    assert hip_api.load_library().fbstab_hip_device_count() >= 1
    return hip_api


def _arrays(p):
    return {k: np.ascontiguousarray(a) for k, a in p.arrays.items()}


def _forward_error(step, ref):
    smax = max(np.abs(np.concatenate(step)).max(), 1.0)
    return np.abs(np.concatenate(step) - np.concatenate(ref)).max() / smax


def _check(oracle, p, x, seeds, res, fwd_bar):
    """Per QP and right-hand side: status 0, the residual of V (dz, dl, dv) = (gz, -gl, -C.gv) within 3 x the
    oracle's (longdouble), and the step within ``fwd_bar`` of the oracle's.  Returns the worst residual ratio."""
    assert (res["status"] == 0).all()
    worst = 0.0
    for q in range(p.batch):
        xq = tuple(t[q] for t in x)
        for k in range(seeds[0].shape[1]):
            sk = tuple(t[q, k] for t in seeds)
            step = tuple(res[n][q, k] for n in STEP)
            ref = LR.oracle_adjoint(oracle, p, q, xq, sk)
            r_dev, r_orc = LR.adjoint_residual(p, q, xq, step, sk), LR.adjoint_residual(p, q, xq, ref, sk)
            err = _forward_error(step, ref)
            print("qp %d rhs %d residual %.3e oracle's %.3e forward error %.3e (bar %.3e)" % (q, k, r_dev, r_orc, err, fwd_bar))
            worst = max(worst, r_dev / r_orc)
            assert r_dev <= 3 * r_orc, (q, k, r_dev, r_orc)
            assert err <= fwd_bar, (q, k, err, fwd_bar)
    return worst


def _bitwise_the_adjoint(s, p, x, seeds, res):
    """Right-hand side k of ``res`` is bitwise Adjoint(..., adj=True) for seed k (the four-wavefront handles)."""
    for k in range(seeds[0].shape[1]):
        adj = s.Adjoint(_arrays(p), *x, *(np.ascontiguousarray(t[:, k]) for t in seeds), want=(), adj=True)
        assert (adj["status"] == 0).all()
        for n in STEP:
            assert np.array_equal(adj[n], res[n][:, k]), (k, n)


@pytest.mark.parametrize("idx", range(len(DENSE_KERNEL_SHAPES)), ids=["x".join(map(str, s[0])) for s in DENSE_KERNEL_SHAPES])
def test_every_right_hand_side_on_every_dense_kernel(hip, oracle, monkeypatch, idx):
    """At the device's solutions with three random seeds per QP, on one shape per dense kernel: status 0, every
    right-hand side's residual within 3 x the oracle's and its step within FWD_FACTOR x the shape's spread of the
    oracle's (the rule and the figures of test_gpu_dense_adjoint.py).  The one-wavefront shapes are also put through
    the four-wavefront policy (FBSTAB_HIP_DENSE_THREADS=256 and =64); on every four-wavefront handle each right-hand
    side is bitwise what Adjoint(..., adj=True) returns for its seed."""
    (nz, nl, nv), threads, (kg, vg), spread0 = DENSE_KERNEL_SHAPES[idx]
    p = fx.synthetic_dense_batch(B, nz, nl, nv, first_id=500 + 10 * idx)
    if vg:
        p.arrays["b"] = p.arrays["b"].copy()
        p.arrays["b"][:, RELAX_FROM:] += RELAX
    s, x, out = H.cold_solve(hip, p)
    assert s.query()["threads"] == threads and (out["eflag"] == 0).all()
    seeds = KH.random_seed_block(np.random.default_rng(6100 + idx), p, 3, B)
    res = s.KktSolve(_arrays(p), *x, *seeds)
    assert s.last_kernel_ms() > 0
    print("worst residual / oracle's %.3f" % _check(oracle, p, x, seeds, res, FWD_FACTOR * spread0))
    if threads != 64:
        _bitwise_the_adjoint(s, p, x, seeds, res)
        return
    for forced in ("256", "64"):
        monkeypatch.setenv(THREADS, forced)
        s4 = hip.FBstabDenseBatch(nz, nl, nv, max_batch=p.batch)
        a_lds = HostAdjoint("dense").layout(nz, nl, nv, nthreads=64)["a_lds"]
        assert s4.query()["threads"] == (256 if forced == "256" or not a_lds else 64)
        assert s4.query()["lds_bytes"] > s.query()["lds_bytes"]   # (the four-wavefront policy: K in LDS)
        res4 = s4.KktSolve(_arrays(p), *x, *seeds)
        _check(oracle, p, x, seeds, res4, FWD_FACTOR * spread0)
        _bitwise_the_adjoint(s4, p, x, seeds, res4)
        assert not all(np.array_equal(res[n], res4[n]) for n in STEP)   # (two kernels)


@pytest.mark.parametrize("shape", [(50, 10, 100), (30, 0, 40)], ids=["50x10x100", "30x0x40"])
def test_slot_independence_on_the_one_wavefront_kernel(hip, monkeypatch, shape):
    """Permuting the five seeds permutes the steps bitwise; a seed solved alone (nrhs = 1) equals its slot; and the
    same batch alone, packed behind other QPs, and on one workgroup gives the same bits."""
    K = 5
    p = fx.synthetic_dense_batch(B, *shape, first_id=640)
    s, x, out = H.cold_solve(hip, p)
    assert s.query()["threads"] == 64 and (out["eflag"] == 0).all()
    seeds = KH.random_seed_block(np.random.default_rng(12), p, K, B)
    base = s.KktSolve(_arrays(p), *x, *seeds)
    assert (base["status"] == 0).all() and np.abs(base["dz"]).max(axis=2).min() > 0
    perm = np.array([3, 0, 4, 2, 1])
    moved = s.KktSolve(_arrays(p), *x, *(np.ascontiguousarray(t[:, perm]) for t in seeds))
    for n in STEP:
        assert np.array_equal(moved[n], base[n][:, perm]), n
    for k in range(K):
        one = s.KktSolve(_arrays(p), *x, *(np.ascontiguousarray(t[:, k:k + 1]) for t in seeds))
        for n in STEP:
            assert np.array_equal(one[n][:, 0], base[n][:, k]), (k, n)
    # behind four other QPs in one batch
    other = fx.synthetic_dense_batch(4, *shape, first_id=700)
    both = fx.DenseProblem(*shape)
    both.arrays = {k: np.concatenate([other.arrays[k], p.arrays[k]]) for k in p.arrays}
    xo = tuple(np.concatenate([np.ascontiguousarray(other.solution[k]), t]) for k, t in zip(("z", "l", "v"), x))
    so = tuple(np.concatenate([t[[0, 1, 2, 0]], t]) for t in seeds)
    wide = hip.FBstabDenseBatch(*shape, max_batch=7)
    packed = wide.KktSolve(_arrays(both), *xo, *so)
    monkeypatch.setenv(CAP, "1")
    single = hip.FBstabDenseBatch(*shape, max_batch=B)
    assert single.query()["workgroups"] == 1
    queued = single.KktSolve(_arrays(p), *x, *seeds)
    for n in STEP:
        assert np.array_equal(packed[n][4:], base[n]), n
        assert np.array_equal(queued[n], base[n]), n


def _unit_spread(oracle, oracle_fma, p, q, xq, seeds):
    """Largest relative difference between the two roundings of the reference's step over the seeds ``seeds`` of one
    QP (rows of (gz, gl, gv)): the `spread` of test_gpu_dense_adjoint.py, for these right-hand sides."""
    spread = 0.0
    for k in range(seeds[0].shape[0]):
        sk = tuple(t[k] for t in seeds)
        spread = max(spread, _forward_error(LR.oracle_adjoint(oracle, p, q, xq, sk),
                                            LR.oracle_adjoint(oracle_fma, p, q, xq, sk)))
    return spread


@pytest.mark.parametrize("shape", [(20, 5, 40), (30, 0, 40)], ids=["20x5x40", "30x0x40"])
def test_jacobian_mode_against_the_seeded_mode_and_the_tangent(hip, oracle, oracle_fma, shape):
    """For wrt in f, h, b (h where nl > 0): the Jacobian is bitwise the seeded call on the unit seeds spelled out;
    row j agrees with Tangent for the perturbation e_j within the forward bar of test_gpu_dense_adjoint.py -
    FWD_FACTOR x the spread of the reference's two roundings on these right-hand sides at these points; and at
    nl == 0, dz/df is symmetric within the same bar (K is symmetric)."""
    nz, nl, nv = shape
    p = fx.synthetic_dense_batch(2, nz, nl, nv, first_id=660)
    s, x, out = H.cold_solve(hip, p)
    assert (out["eflag"] == 0).all()
    wide = hip.FBstabDenseBatch(nz, nl, nv, max_batch=max(shape))
    for wrt in ("f", "h", "b"):
        n = {"f": nz, "h": nl, "b": nv}[wrt]
        if n == 0:
            continue
        jac = s.Jacobian(_arrays(p), *x, wrt=wrt, want=STEP)
        unit = KH.unit_seed_block(p, wrt)
        seeded = s.KktSolve(_arrays(p), *x, *unit)
        assert (jac["status"] == 0).all() and jac["dz"].shape == (2, n, nz)
        for name in STEP:
            assert np.array_equal(jac[name], seeded[name]), (wrt, name)
        only = s.Jacobian(_arrays(p), *x, wrt=wrt)
        assert set(only) == {"dz", "status"} and np.array_equal(only["dz"], jac["dz"])
        for q in range(p.batch):
            xq = tuple(t[q] for t in x)
            bar = FWD_FACTOR * _unit_spread(oracle, oracle_fma, p, q, xq, unit)
            rep = lambda a: np.ascontiguousarray(np.repeat(a[q:q + 1], n, axis=0))
            tan = wide.Tangent(_arrays(LR.one_qp(p, q)), *(rep(t) for t in x), {wrt: np.eye(n)})
            assert (tan["status"] == 0).all()
            worst = max(_forward_error(tuple(jac[name][q, j] for name in STEP), tuple(tan[name][j] for name in STEP))
                        for j in range(n))
            print("wrt", wrt, "qp", q, "worst difference from Tangent %.3e (bar %.3e)" % (worst, bar))
            assert worst <= bar, (wrt, q, worst, bar)
            if wrt == "f" and nl == 0:
                J = jac["dz"][q]
                asym = np.abs(J - J.T).max() / max(np.abs(J).max(), 1.0)
                print("asymmetry of dz/df %.3e (bar %.3e)" % (asym, bar))
                assert asym <= bar, (q, asym, bar)


def _one_qp(hip, Hm, f, A, b):
    """One QP (nl = 0) solved at abs_tol = 1e-11: (solver, arrays, point)."""
    nz, nv = len(f), len(b)
    p = fx.DenseProblem(nz, 0, nv)
    row = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(1, -1))
    p.arrays = dict(H=row(Hm.T), f=row(f), G=np.zeros((1, 0)), h=np.zeros((1, 0)), A=row(A.T), b=row(b))
    s, x, out = H.cold_solve(hip, p, default_options(abs_tol=1e-11))
    assert (out["eflag"] == 0).all()
    return s, p, x


def test_known_answers_without_and_with_one_active_bound(hip):
    """The QPs of test_gpu_dense_adjoint.py's known answers.  No row active (A = 0, b = 1) and nl = 0: V's first block
    is H + sigma I alone, so dz/df = -(H + sigma I)^{-1} to the forward error of a backward-stable solve,
    100 nz eps cond(H + sigma I), and dz/db = 0.  With the one bound z_0 <= b_0 active: the Jacobians of the active-set
    solution map (linear_reference.active_set_solve on unit data), to 1e-6 relative - the sigma bias plus the solve
    tolerance, as there."""
    rng = np.random.default_rng(4402)
    nz, nv = 12, 4
    Hm, f = _spd(rng, nz), rng.standard_normal(nz)
    s, p, x = _one_qp(hip, Hm, f, np.zeros((nv, nz)), np.ones(nv))
    Hs = Hm + LR.SIGMA * np.eye(nz)
    inv = np.linalg.inv(Hs)
    bar = 100 * nz * np.finfo(float).eps * np.linalg.cond(Hs) * np.abs(inv).max()
    Jf = s.Jacobian(_arrays(p), *x, wrt="f")["dz"][0]
    Jb = s.Jacobian(_arrays(p), *x, wrt="b")["dz"][0]
    print("no active row: |dz/df + inv| %.3e (bar %.3e), |dz/db| %.3e" % (np.abs(Jf + inv).max(), bar, np.abs(Jb).max()))
    assert np.abs(Jf + inv).max() <= bar and np.abs(Jb).max() <= bar
    # z_0 bounded by half its unconstrained value (from above): row 0 of A is e_0', every other row inactive
    zu = -np.linalg.inv(Hm) @ f
    if zu[0] < 0:
        f, zu = -f, -zu
    A = np.zeros((nv, nz))
    A[0, 0] = 1.0
    b = np.ones(nv)
    b[0] = 0.5 * zu[0]
    s, p, x = _one_qp(hip, Hm, f, A, b)
    assert abs(x[0][0][0] - b[0]) <= 1e-8 * abs(b[0]) and x[2][0][0] > 1e-6
    act = np.zeros(nv, dtype=bool)
    act[0] = True
    arr = {k: p.arrays[k][0] for k in p.arrays}
    unit = lambda name, j: {**arr, "f": np.zeros(nz), "b": np.zeros(nv), name: np.eye(len(arr[name]))[j]}
    ref_f = np.stack([LR.active_set_solve(unit("f", j), nz, 0, nv, act)[0] for j in range(nz)])
    ref_b = np.stack([LR.active_set_solve(unit("b", j), nz, 0, nv, act)[0] for j in range(nv)])
    Jf = s.Jacobian(_arrays(p), *x, wrt="f")["dz"][0]
    Jb = s.Jacobian(_arrays(p), *x, wrt="b")["dz"][0]
    scale = max(np.abs(ref_f).max(), np.abs(ref_b).max())
    np.testing.assert_allclose(Jf, ref_f, rtol=1e-6, atol=1e-6 * scale)
    np.testing.assert_allclose(Jb, ref_b, rtol=1e-6, atol=1e-6 * scale)
    assert np.abs(ref_b[0]).max() > 0 and not ref_b[1:].any()


# synthetic_dense_batch(8, 20, 5, 40, first_id=FD_FIRST_ID): at the oracle's solutions linear_reference.strict_qps
# keeps 7 of the 8 QPs (all but QP 2; checked on the CPU before the first GPU run)
FD_FIRST_ID = 0


def test_central_differences_through_the_device_solver(hip):
    """One column of dz/db (an active row) and one of dz/df per strictly complementary QP against central differences
    through the device solver: the step size (h = 1e-5), the solve tolerance (abs_tol = 1e-11) and the bar (1e-4
    relative, against the column's largest entry or 1e-2 of its entries' sum) of test_gpu_dense_adjoint.py's
    test_central_differences_through_the_device_solver."""
    nz, nl, nv = 20, 5, 40
    base = fx.synthetic_dense_batch(8, nz, nl, nv, first_id=FD_FIRST_ID)
    o = default_options(abs_tol=1e-11)
    s, x, out = H.cold_solve(hip, base, o)
    assert (out["eflag"] == 0).all()
    strict = LR.strict_qps(base, x[0], x[2])
    assert 2 * len(strict) >= base.batch, [q for q, _ in strict]
    Jb = s.Jacobian(_arrays(base), *x, wrt="b")
    Jf = s.Jacobian(_arrays(base), *x, wrt="f")
    assert (Jb["status"] == 0).all() and (Jf["status"] == 0).all()
    h = 1e-5
    cases = []   # (QP, array, entry, sign)
    for q, act in strict:
        jb = int(np.nonzero(act)[0][0]) if act.any() else 0
        cases += [(q, "b", jb, 1.0), (q, "b", jb, -1.0), (q, "f", q % nz, 1.0), (q, "f", q % nz, -1.0)]
    pert = fx.DenseProblem(nz, nl, nv)
    pert.arrays = {k: np.stack([base.arrays[k][q] for q, _, _, _ in cases]) for k in base.arrays}
    for i, (q, k, j, sg) in enumerate(cases):
        pert.arrays[k][i, j] += sg * h
    _, xp, outp = H.cold_solve(hip, pert, o)
    assert (outp["eflag"] == 0).all()
    for i in range(0, len(cases), 2):
        q, k, j, _ = cases[i]
        fd = (xp[0][i] - xp[0][i + 1]) / (2 * h)
        col = (Jb if k == "b" else Jf)["dz"][q, j]
        bar = 1e-4 * max(np.abs(col).max(), 1e-2 * np.abs(col).sum())
        print("qp %d d z / d %s[%d]: |fd - column| %.3e (bar %.3e)" % (q, k, j, np.abs(fd - col).max(), bar))
        assert np.abs(fd - col).max() <= bar, (q, k, j)
        assert np.abs(col).max() > 0


@pytest.mark.parametrize("threads", [64, 256])
def test_failed_factorisation_is_reported_through_status(hip, monkeypatch, threads):
    """A NaN in H[0] of QP 1 (the construction of the dense adjoint's status test), on both policies: status
    [0, 1, 0], every right-hand side of QP 1 zero in both modes, QPs 0 and 2 the bits of the clean batch."""
    if threads == 256:
        monkeypatch.setenv(THREADS, "256")
    p = fx.synthetic_dense_batch(B, 50, 10, 100, first_id=70)
    ref = fx.synthetic_dense_batch(B, 50, 10, 100, first_id=70)
    p.arrays["H"] = p.arrays["H"].copy()
    p.arrays["H"][1, 0] = np.nan
    s = hip.FBstabDenseBatch(p.nz, p.nl, p.nv, max_batch=B)
    assert s.query()["threads"] == threads
    x = tuple(np.ascontiguousarray(ref.solution[k]) for k in ("z", "l", "v"))
    seeds = KH.random_seed_block(np.random.default_rng(1), p, 3, B)
    res, good = s.KktSolve(_arrays(p), *x, *seeds), s.KktSolve(_arrays(ref), *x, *seeds)
    jac, jgood = s.Jacobian(_arrays(p), *x, wrt="h", want=STEP), s.Jacobian(_arrays(ref), *x, wrt="h", want=STEP)
    assert res["status"].tolist() == jac["status"].tolist() == [0, 1, 0]
    assert good["status"].tolist() == jgood["status"].tolist() == [0, 0, 0]
    for n in STEP:
        for bad, ok in ((res, good), (jac, jgood)):
            assert np.array_equal(bad[n][1], np.zeros_like(bad[n][1])), n
            assert np.array_equal(bad[n][[0, 2]], ok[n][[0, 2]]) and np.abs(ok[n][1]).max(axis=1).min() > 0, n


def test_placement(hip):
    """A host-pointer call returns the bits of the device-pointer call, in both modes; a shared seed block (stride 0)
    those of its replicated form; rhs_stride = length + 3 leaves the NaN in the gaps; NULL l / v step slots are
    skipped; batch == 0 returns OK with nothing written; a matrix index or wrt = h at nl == 0 is refused; and
    autograd.dense_jacobian returns detached device tensors equal to the C-ABI's."""
    import torch
    from fbstab_amd.autograd import dense_jacobian
    dev = torch.device("cuda:0")
    K = 3
    p = fx.synthetic_dense_batch(B, 50, 10, 100, first_id=300)
    s, x, out = H.cold_solve(hip, p)
    seeds = KH.random_seed_block(np.random.default_rng(4), p, K, B)
    good = s.KktSolve(_arrays(p), *x, *seeds)
    jac = s.Jacobian(_arrays(p), *x, wrt="h", want=STEP)
    assert (good["status"] == 0).all() and (jac["status"] == 0).all()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    data = {k: t(a) for k, a in p.arrays.items()}
    on_dev = s.KktSolve(data, *(t(a) for a in x), *(t(a) for a in seeds))
    jac_dev = s.Jacobian(data, *(t(a) for a in x), wrt="h", want=STEP)
    torch.cuda.synchronize()
    for n in STEP + ("status",):
        assert np.array_equal(on_dev[n].cpu().numpy(), good[n]), n
        assert np.array_equal(jac_dev[n].cpu().numpy(), jac[n]), n
    assert s.last_kernel_ms() > 0
    # autograd.dense_jacobian
    J = dense_jacobian(s, {k: a.clone().requires_grad_(k == "b") for k, a in data.items()}, *(t(a) for a in x), wrt="h")
    torch.cuda.synchronize()
    for n in STEP + ("status",):
        assert J[n].is_cuda and not J[n].requires_grad and J[n].grad_fn is None, n
        assert np.array_equal(J[n].cpu().numpy(), jac[n]), n
    # one block of seeds for the whole batch
    shared = tuple(np.ascontiguousarray(g[1]) for g in seeds)
    copied = tuple(np.ascontiguousarray(np.repeat(g[None], B, axis=0)) for g in shared)
    a, b = s.KktSolve(_arrays(p), *x, *shared), s.KktSolve(_arrays(p), *x, *copied)
    a_dev = s.KktSolve(data, *(t(u) for u in x), *(t(u) for u in shared))
    torch.cuda.synchronize()
    for n in STEP:
        assert np.array_equal(a[n], b[n]) and np.array_equal(a_dev[n].cpu().numpy(), b[n]), n
    # vectors three doubles apart, QPs five: what lies between is not written
    lens = (p.nz, p.nl, p.nv)
    pads = [np.full((B, K * (n + 3) + 5), np.nan) for n in lens]
    views = [pd[:, :K * (n + 3)].reshape(B, K, n + 3)[:, :, :n] for pd, n in zip(pads, lens)]
    rc, status = KH.kkt_solve_into(s, _arrays(p), x, seeds, views)
    assert rc == 0 and status.tolist() == [0, 0, 0]
    for n, pd, vw, ln in zip(STEP, pads, views, lens):
        assert np.array_equal(vw, good[n]), n
        gaps = np.ones(pd.shape, dtype=bool)
        gaps[:, :K * (ln + 3)].reshape(B, K, ln + 3)[:, :, :ln] = False
        assert np.isnan(pd[gaps]).all() and gaps.sum() == B * (3 * K + 5), n
    # NULL l and v step slots are skipped, in both modes
    dz = np.full((B, K, p.nz), np.nan)
    rc, status = KH.kkt_solve_into(s, _arrays(p), x, seeds, (dz, None, None))
    assert rc == 0 and np.array_equal(dz, good["dz"])
    jz = np.full((B, p.nl, p.nz), np.nan)
    rc, status = KH.jacobian_into(s, _arrays(p), x, KH.WRT["h"], (jz, None, None))
    assert rc == 0 and status.tolist() == [0, 0, 0] and np.array_equal(jz, jac["dz"])
    # an empty batch: OK, nothing written
    dz[:] = np.nan
    rc, status = KH.kkt_solve_into(s, _arrays(p), x, seeds, (dz, None, None), batch=0)
    assert rc == 0 and status.size == 0 and np.isnan(dz).all()
    rc, status = KH.jacobian_into(s, _arrays(p), x, KH.WRT["h"], (jz, None, None), batch=0)
    assert rc == 0 and np.array_equal(jz, jac["dz"])
    # what takes the handle: a matrix index, and wrt = h without equalities
    rc, _ = KH.jacobian_into(s, _arrays(p), x, 4, (jz, None, None))
    assert rc == 1 and "wrt must be" in s._lib.fbstab_hip_last_error().decode()
    p0 = fx.synthetic_dense_batch(1, 30, 0, 40)
    s0 = hip.FBstabDenseBatch(30, 0, 40, max_batch=1)
    x0 = tuple(np.ascontiguousarray(p0.solution[k]) for k in ("z", "l", "v"))
    rc, _ = KH.jacobian_into(s0, _arrays(p0), x0, KH.WRT["h"], (np.zeros((1, 1, 30)), None, None))
    assert rc == 1 and "without equality constraints" in s0._lib.fbstab_hip_last_error().decode()
