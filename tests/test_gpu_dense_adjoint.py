"""GPU checks of the dense adjoint (fbstab_hip_dense_adjoint_batch, FBstabDenseBatch.Adjoint,
fbstab_amd.autograd.solve_dense): the adjoint system's residual against the oracle's linear solver and the gradient
table on one shape per dense kernel, the step's forward error, central differences through the device solver,
closed-form answers, independence of the factorisation option and of the queue, a failed factorisation reported
through `status`, torch autograd, and host against device pointers."""
import numpy as np
import pytest

from fbstab_amd.hip_api import DENSE_ARR
from tools import fixtures as fx
from oracle.oracle_py import default_options
from tests import helpers as H
from tests import linear_reference as LR
from tests.hostsim import HostAdjoint
from tests.shapes import DENSE_KERNEL_SHAPES, RELAX_FROM, RELAX

pytestmark = pytest.mark.gpu

CAP = "FBSTAB_HIP_MAX_WORKGROUPS"
THREADS = "FBSTAB_HIP_DENSE_THREADS"
KEYS = DENSE_ARR + ("dz", "dl", "dv")

# Forward error of the step against the oracle's: |step - oracle's step|_inf / max(|step|_inf, 1).  Two roundings
# of the reference's own solver - Oracle() and Oracle(fma=True) - differ by `spread` (last column of
# shapes.DENSE_KERNEL_SHAPES) on the three QPs of each shape at their solutions with this file's seeds (measured on
# the CPU at the oracle's solutions; the test prints the same figure at the device's).  The bar is FWD_FACTOR x
# that: the factor covers the device's different elimination arithmetic (right-looking updates, MFMA sums).
# cond(V) differs by shape, so each shape carries its own figure.  The residual rule is the binding check; this one
# catches a step that solves a neighbouring system.
FWD_FACTOR = 10


@pytest.fixture(scope="module")
def hip():
    from fbstab_amd import hip_api
    assert hip_api.load_library().fbstab_hip_device_count() >= 1
    return hip_api


def _arrays(p):
    return {k: np.ascontiguousarray(a) for k, a in p.arrays.items()}


def _check(oracle, oracle_fma, p, x, seeds, res, fwd_bar):
    """Per QP: status 0, the residual within 3 x the oracle's, the gradient table, and the forward error of the
    step.  Returns the largest relative difference between the two roundings of the oracle's step."""
    assert (res["status"] == 0).all()
    spread = 0.0
    for q in range(p.batch):
        xq = tuple(t[q] for t in x)
        sq = tuple(t[q] for t in seeds)
        step = tuple(res[k][q] for k in ("dz", "dl", "dv"))
        ref = LR.oracle_adjoint(oracle, p, q, xq, sq)
        ref_fma = LR.oracle_adjoint(oracle_fma, p, q, xq, sq)
        LR.check_step_and_table(p, q, xq, sq, step, {k: res[k][q] for k in DENSE_ARR}, ref)
        smax = max(np.abs(np.concatenate(step)).max(), 1.0)
        spread = max(spread, np.abs(np.concatenate(ref) - np.concatenate(ref_fma)).max() / smax)
        err = np.abs(np.concatenate(step) - np.concatenate(ref)).max() / smax
        print("forward error %.3e (bar %.3e)" % (err, fwd_bar))
        assert err <= fwd_bar, (q, err, fwd_bar)
    return spread


@pytest.mark.parametrize("idx", range(len(DENSE_KERNEL_SHAPES)), ids=["x".join(map(str, s[0])) for s in DENSE_KERNEL_SHAPES])
def test_adjoint_residual_table_and_forward_error_on_every_dense_kernel(hip, oracle, oracle_fma, monkeypatch, idx):
    """At the device's solutions with random seeds, on one shape per dense kernel: status 0, V (dz, dl, dv) =
    (gz, -gl, -C.gv) within 3 x the oracle's residual (longdouble), the gradients the table applied to the returned
    adjoint (rtol 1e-13), and the step within FWD_FACTOR x the shape's spread of the oracle's.  The one-wavefront
    shapes are also put through the four-wavefront kernel (FBSTAB_HIP_DENSE_THREADS=256): the same rule, and not
    the same bits - they are two kernels."""
    (nz, nl, nv), threads, (kg, vg), spread0 = DENSE_KERNEL_SHAPES[idx]
    lay = HostAdjoint("dense").layout(nz, nl, nv)
    assert (lay["k_global"], lay["v_global"]) == (kg, vg)
    if vg:
        assert not HostAdjoint("dense").layout(nz, nl, nv - 1)["v_global"]  # (the smallest such nv)
    p = fx.synthetic_dense_batch(3, nz, nl, nv, first_id=500 + 10 * idx)
    if vg:
        p.arrays["b"] = p.arrays["b"].copy()
        p.arrays["b"][:, RELAX_FROM:] += RELAX
    s, x, out = H.cold_solve(hip, p)
    assert s.query()["threads"] == threads
    assert (out["eflag"] == 0).all()
    seeds = LR.random_seeds(np.random.default_rng(idx), p)
    res = s.Adjoint(_arrays(p), *x, *seeds, adj=True)
    spread = _check(oracle, oracle_fma, p, x, seeds, res, FWD_FACTOR * spread0)
    print("oracle / oracle_fma step spread on", (nz, nl, nv), "%.3e" % spread)
    if threads == 64:
        monkeypatch.setenv(THREADS, "256")
        s4 = hip.FBstabDenseBatch(nz, nl, nv, max_batch=p.batch)
        assert s4.query()["threads"] == 256
        res4 = s4.Adjoint(_arrays(p), *x, *seeds, adj=True)
        _check(oracle, oracle_fma, p, x, seeds, res4, FWD_FACTOR * spread0)
        assert not all(np.array_equal(res[k], res4[k]) for k in ("dz", "dl", "dv"))
        # ... and through that policy's one-wavefront instance (fbstab_dense_adjoint_kernel<64>, K in LDS)
        monkeypatch.setenv(THREADS, "64")
        s1 = hip.FBstabDenseBatch(nz, nl, nv, max_batch=p.batch)
        # (where A does not fit the LDS beside K that instance is not offered: four wavefronts again)
        a_lds = HostAdjoint("dense").layout(nz, nl, nv, nthreads=64)["a_lds"]
        assert s1.query()["threads"] == (64 if a_lds else 256) and s1.query()["lds_bytes"] > s.query()["lds_bytes"]
        res1 = s1.Adjoint(_arrays(p), *x, *seeds, adj=True)
        _check(oracle, oracle_fma, p, x, seeds, res1, FWD_FACTOR * spread0)
        assert not all(np.array_equal(res[k], res1[k]) for k in ("dz", "dl", "dv"))


def test_central_differences_through_the_device_solver(hip):
    """synthetic_dense_batch(16, 20, 5, 40) solved at abs_tol = 1e-11; QPs strictly complementary at 1e-3 with
    fewer than nz active rows plus equalities (at least 8 of 16).  For a random linear loss L = a'z + b'l + c'v,
    central differences (h = 1e-5, all perturbed QPs in one batch) along a random direction of each of the six
    arrays (symmetric for H) match the adjoint's directional derivative to 1e-4."""
    nz, nl, nv = 20, 5, 40
    base = fx.synthetic_dense_batch(16, nz, nl, nv)
    o = default_options(abs_tol=1e-11)
    s, x, out = H.cold_solve(hip, base, o)
    assert (out["eflag"] == 0).all()
    strict = [q for q, _ in LR.strict_qps(base, x[0], x[2])]
    assert len(strict) >= 8, strict
    rng = np.random.default_rng(8802)
    seeds = LR.random_seeds(rng, base)
    grad = s.Adjoint(_arrays(base), *x, *seeds)
    assert (grad["status"] == 0).all()
    h = 1e-5
    dirs = LR.directions(rng, nz, nl, nv)
    cases = [(q, k, sg) for q in strict for k in DENSE_ARR for sg in (1.0, -1.0)]
    pert = fx.DenseProblem(nz, nl, nv)
    pert.arrays = {k: np.ascontiguousarray(np.stack([base.arrays[k][q] + (sg * h * dirs[k] if kk == k else 0.0)
                                                     for q, kk, sg in cases])) for k in DENSE_ARR}
    _, xp, outp = H.cold_solve(hip, pert, o)
    assert (outp["eflag"] == 0).all()
    loss = lambda j: sum(float(seeds[t][cases[j][0]] @ xp[t][j]) for t in range(3))
    for j in range(0, len(cases), 2):
        q, k, _ = cases[j]
        fd = (loss(j) - loss(j + 1)) / (2 * h)
        ad = float(grad[k][q] @ dirs[k])
        assert abs(fd - ad) <= 1e-4 * max(abs(ad), 1e-2 * np.abs(grad[k][q]).sum()), (q, k, fd, ad)


def _spd(rng, n):
    M = rng.standard_normal((n, n))
    return M @ M.T / n + 0.5 * np.eye(n)


def _rows(hip, Hm, f, A, b, gz):
    """One QP (nl = 0) repeated once per row of ``gz``, solved at abs_tol = 1e-11: (gradients, solutions)."""
    B, nz, nv = gz.shape[0], len(f), len(b)
    p = fx.DenseProblem(nz, 0, nv)
    rep = lambda a: np.ascontiguousarray(np.tile(np.asarray(a, dtype=np.float64).reshape(1, -1), (B, 1)))
    p.arrays = dict(H=rep(Hm.T), f=rep(f), G=np.zeros((B, 0)), h=np.zeros((B, 0)), A=rep(A.T), b=rep(b))
    s, x, out = H.cold_solve(hip, p, default_options(abs_tol=1e-11))
    assert (out["eflag"] == 0).all()
    g = s.Adjoint(_arrays(p), *x, gz, want=("f", "b"))
    assert (g["status"] == 0).all()
    return g, x


def test_known_answers_without_and_with_one_active_bound(hip):
    """No inequality active (A = 0, b = 1) and nl = 0: z = -inv(H) f, so seeds e_j on z give f_bar = -inv(H) e_j
    (to 1e-6 relative: the sigma bias plus the solve tolerance).  With the one bound z_0 <= b_0 active and the seed
    e_0 the loss is z_0 = b_0 locally: f_bar = 0 to 1e-6 max|inv(H)| and b_bar[0] = 1 to 1e-6."""
    rng = np.random.default_rng(4402)
    nz, nv = 12, 4
    Hm, f = _spd(rng, nz), rng.standard_normal(nz)
    Hinv = np.linalg.inv(Hm)
    g, x = _rows(hip, Hm, f, np.zeros((nv, nz)), np.ones(nv), np.eye(nz))
    np.testing.assert_allclose(x[0][0], -Hinv @ f, rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(g["f"], -Hinv, rtol=1e-6, atol=1e-6 * np.abs(Hinv).max())
    assert np.abs(g["b"]).max() <= 1e-6
    # z_0 bounded by half its unconstrained value (from above): row 0 of A is e_0', every other row inactive
    zu = -Hinv @ f
    if zu[0] < 0:
        f, zu = -f, -zu
    A = np.zeros((nv, nz))
    A[0, 0] = 1.0
    b = np.ones(nv)
    b[0] = 0.5 * zu[0]
    gz = np.zeros((1, nz))
    gz[0, 0] = 1.0
    g, x = _rows(hip, Hm, f, A, b, gz)
    assert abs(x[0][0][0] - b[0]) <= 1e-8 * abs(b[0]) and x[2][0][0] > 1e-6
    assert np.abs(g["f"][0]).max() <= 1e-6 * np.abs(Hinv).max()
    assert abs(g["b"][0][0] - 1.0) <= 1e-6 and np.abs(g["b"][0][1:]).max() <= 1e-6


def test_gradients_do_not_depend_on_the_factorisation_option(hip):
    """The one-wavefront adjoint always pivots: NATURAL and AUTO handles give the bits of a PIVOTED one, and the
    adjoint leaves pivoted_steps describing the last solve."""
    p = fx.synthetic_dense_batch(8, 50, 10, 100, first_id=40)
    seeds = LR.random_seeds(np.random.default_rng(5), p)
    res = {}
    for order in ("ORDER_PIVOTED", "ORDER_NATURAL", "ORDER_AUTO"):
        s = hip.FBstabDenseBatch(p.nz, p.nl, p.nv, max_batch=p.batch)
        assert s.query()["threads"] == 64
        s.SetFactorisation(getattr(s, order))
        z, l, v, y = (np.zeros((p.batch, n)) for n in (p.nz, p.nl, p.nv, p.nv))
        out = s.Solve(_arrays(p), z, l, v, y)
        assert (out["eflag"] == 0).all()
        before = s.Factorisation()
        assert before["order"] == getattr(s, order)
        if order == "ORDER_PIVOTED":
            x = (z, l, v)  # (every handle differentiates at the same points)
        res[order] = s.Adjoint(_arrays(p), *x, *seeds, adj=True)
        assert (res[order]["status"] == 0).all()
        assert s.Factorisation() == before
    for order in ("ORDER_NATURAL", "ORDER_AUTO"):
        for k in KEYS:
            assert np.array_equal(res[order][k], res["ORDER_PIVOTED"][k]), (order, k)
    assert np.abs(res["ORDER_PIVOTED"]["H"]).max() > 0


@pytest.mark.parametrize("shape,threads", [((50, 10, 100), 64), ((90, 12, 77), 256)])
def test_gradients_are_bitwise_the_same_alone_packed_and_queued(hip, monkeypatch, shape, threads):
    """QP gradients do not depend on where the queue puts them: alone, in a batch on two workgroups (every
    workgroup re-fetching), and in a batch on the whole grid - on the one-wavefront and the four-wavefront kernel."""
    p = fx.synthetic_dense_batch(24, *shape, first_id=900)
    s, x, out = H.cold_solve(hip, p)
    assert s.query()["threads"] == threads
    seeds = LR.random_seeds(np.random.default_rng(9), p)
    full = s.Adjoint(_arrays(p), *x, *seeds, adj=True)
    assert (full["status"] == 0).all()
    monkeypatch.setenv(CAP, "2")
    packed_h = hip.FBstabDenseBatch(*shape, max_batch=p.batch)
    assert packed_h.query()["workgroups"] == 2 < p.batch
    packed = packed_h.Adjoint(_arrays(p), *x, *seeds, adj=True)
    monkeypatch.delenv(CAP)
    alone_h = hip.FBstabDenseBatch(*shape, max_batch=1)
    for q in (0, 7, 23):
        one = {k: np.ascontiguousarray(a[q:q + 1]) for k, a in p.arrays.items()}
        alone = alone_h.Adjoint(one, *(t[q:q + 1] for t in x), *(t[q:q + 1] for t in seeds), adj=True)
        for k in KEYS:
            assert np.array_equal(alone[k][0], full[k][q]), (q, k)
    for k in KEYS:
        assert np.array_equal(packed[k], full[k]), k


@pytest.mark.parametrize("threads", [64, 256])
def test_failed_factorisation_is_reported_through_status(hip, monkeypatch, threads):
    """A NaN in H[0] of one QP is a NaN on the diagonal of K, which ends the factorisation by Eigen's rule - an
    arithmetic outcome: status 1, zero gradients and a zero adjoint for that QP, and the others untouched by it."""
    if threads == 256:
        monkeypatch.setenv(THREADS, "256")
    p = fx.synthetic_dense_batch(3, 50, 10, 100, first_id=70)
    ref = fx.synthetic_dense_batch(3, 50, 10, 100, first_id=70)
    p.arrays["H"] = p.arrays["H"].copy()
    p.arrays["H"][1, 0] = np.nan
    s = hip.FBstabDenseBatch(p.nz, p.nl, p.nv, max_batch=3)
    assert s.query()["threads"] == threads
    x = tuple(np.ascontiguousarray(ref.solution[k]) for k in ("z", "l", "v"))
    seeds = LR.random_seeds(np.random.default_rng(1), p)
    res = s.Adjoint(_arrays(p), *x, *seeds, adj=True)
    good = s.Adjoint(_arrays(ref), *x, *seeds, adj=True)
    assert res["status"].tolist() == [0, 1, 0] and good["status"].tolist() == [0, 0, 0]
    for k in KEYS:
        assert np.array_equal(res[k][1], np.zeros_like(res[k][1])), k
        assert np.array_equal(res[k][[0, 2]], good[k][[0, 2]]) and np.abs(good[k][1]).max() > 0, k


@pytest.mark.parametrize("shape", [(20, 5, 40), (30, 0, 40)])
def test_autograd_matches_the_c_abi_and_zeroes_unsolved_qps(hip, shape):
    """loss.backward() through fbstab_amd.autograd.solve_dense on device tensors: the gradients of the inputs that
    require grad equal the C-ABI call's at the returned points (bitwise), the others get none, and a QP that is
    not SUCCESS (here primal infeasible: two contradictory rows of A) gets zero gradients."""
    import torch
    from fbstab_amd.autograd import solve_dense
    dev = torch.device("cuda:0")
    nz, nl, nv = shape
    p = fx.synthetic_dense_batch(4, nz, nl, nv, first_id=60)
    # QP 1: z_0 <= -1 and -z_0 <= -1 on the first two rows
    A = p.arrays["A"].copy().reshape(4, nz, nv)   # [col][row]
    A[1, :, 0:2] = 0.0
    A[1, 0, 0], A[1, 0, 1] = 1.0, -1.0
    p.arrays["A"] = np.ascontiguousarray(A.reshape(4, -1))
    p.arrays["b"] = p.arrays["b"].copy()
    p.arrays["b"][1, 0:2] = -1.0
    solver = hip.FBstabDenseBatch(nz, nl, nv, max_batch=p.batch)
    want = ("H", "f", "A", "b") if nl == 0 else ("H", "G", "h", "b")
    data = {k: torch.from_numpy(np.ascontiguousarray(a)).to(dev).requires_grad_(k in want) for k, a in p.arrays.items()}
    z, l, v, out = solve_dense(solver, data)
    assert l.shape == (4, nl) and not out.requires_grad
    eflag = hip.out_to_numpy(out)["eflag"]
    assert eflag[1] != 0 and (np.delete(eflag, 1) == 0).all(), eflag
    a, b, c = (torch.from_numpy(t).to(dev) for t in LR.random_seeds(np.random.default_rng(12), p))
    loss = (a * z).sum() + (b * l).sum() + (c * v).sum()
    loss.backward()
    ref = solver.Adjoint({k: t.detach() for k, t in data.items()}, z.detach(), l.detach(), v.detach(), a, b, c)
    torch.cuda.synchronize()
    for k in DENSE_ARR:
        if k not in want:
            assert data[k].grad is None, k
            continue
        g = data[k].grad.cpu().numpy()
        r = ref[k].cpu().numpy()
        assert g.shape == p.arrays[k].shape
        assert np.array_equal(g[[0, 2, 3]], r[[0, 2, 3]]), k
        assert np.array_equal(g[1], np.zeros_like(g[1])), k
        assert np.abs(r[[0, 2, 3]]).max() > 0, k


def test_host_pointers_equal_device_pointers(hip):
    """The host-pointer call (staged through the handle's device buffers) returns the bits of the device-pointer
    call, the status included, also for a subset of the slots."""
    import torch
    dev = torch.device("cuda:0")
    p = fx.synthetic_dense_batch(5, 50, 10, 100, first_id=300)
    s, x, out = H.cold_solve(hip, p)
    seeds = LR.random_seeds(np.random.default_rng(4), p)
    host = s.Adjoint(_arrays(p), *x, *seeds, adj=True)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    on_dev = s.Adjoint({k: t(a) for k, a in p.arrays.items()}, *(t(a) for a in x), *(t(a) for a in seeds), adj=True)
    torch.cuda.synchronize()
    for k in KEYS + ("status",):
        assert np.array_equal(host[k], on_dev[k].cpu().numpy()), k
    assert s.last_kernel_ms() > 0
    part = s.Adjoint(_arrays(p), *x, seeds[0], want=("A",))
    part_dev = s.Adjoint({k: t(a) for k, a in p.arrays.items()}, *(t(a) for a in x), t(seeds[0]), want=("A",))
    assert set(part) == {"A", "status"} and np.array_equal(part["A"], part_dev["A"].cpu().numpy())
