"""GPU checks of the MPC adjoint (fbstab_hip_mpc_adjoint_batch, FBstabMpcBatch.Adjoint, fbstab_amd.autograd):
the adjoint system's residual against the oracle's linear solver on one shape per solve kernel (the one-row
record instances' own adjoint and the flat-vector one) and on the BASELINE batch, the gradient table, central differences of the solution map, the LQR gain, bitwise
invariance under the queue, and torch autograd."""
import numpy as np
import pytest

from tools import fixtures as fx
from oracle.oracle_py import default_options
from tests import helpers as H
from tests import adjoint_helpers as AH
from tests.test_gpu_components import _MPC_SHAPES

pytestmark = pytest.mark.gpu

CAP = "FBSTAB_HIP_MAX_WORKGROUPS"


@pytest.fixture(scope="module")
def hip():
    from fbstab_amd import hip_api
    assert hip_api.load_library().fbstab_hip_device_count() >= 1
    return hip_api


def _solve(hip, p, o=None):
    s = hip.FBstabMpcBatch(*p.sizes(), max_batch=p.batch)
    if o is not None:
        s.UpdateOptions(H._opts(hip, o))
    z, l, v, y = (np.zeros((p.batch, n)) for n in (p.nz, p.nl, p.nv, p.nv))
    out = s.Solve(p.arrays, z, l, v, y)
    return s, (z, l, v), out


def _check_residual_and_table(oracle, p, x, seeds, res):
    """Per QP: the device's residual within 3 x the oracle's, its step within the forward error of the oracle's,
    the residual's own (C, mus) those of the oracle's RiccatiLinearSolver, and the gradient table."""
    assert (res["status"] == 0).all()
    for q in range(p.batch):
        xq = tuple(t[q] for t in x)
        sq = tuple(t[q] for t in seeds)
        step = tuple(res[k][q] for k in ("dz", "dl", "dv"))
        ref = AH.oracle_adjoint(oracle, p, q, xq, sq)
        z, l, v = xq
        pr = oracle.probe(AH.one_qp(p, q), z, l, v, z, l, v, AH.SIGMA, 0.95, r=np.zeros(p.nz + p.nl + p.nv), want_dx=True)
        C, mus = AH.fb_derivatives(p, q, xq)
        # (rows where both precisions take the same branch of the FB function: away from its switch at |(y, v)| =
        # 1e-13, and y of the same sign - on an active row y is zero to rounding, and the penalty term's kink at
        # y = 0 moves C by (1 - alpha) v with its sign)
        Am, bv = (m.astype(np.longdouble) for m in H.mpc_explicit(p, q)[4:])
        ys = bv - Am @ z.astype(np.longdouble)
        rr = np.hypot(pr["x_y"], v)
        far = ((rr >= 1e-12) | (rr < 1e-14)) & (np.sign(pr["x_y"]) == np.sign(ys.astype(np.float64)))
        assert far.sum() >= len(far) // 2
        np.testing.assert_allclose(C.astype(np.float64)[far], pr["gamma"][far], rtol=1e-12, atol=1e-13)
        np.testing.assert_allclose(mus.astype(np.float64)[far], pr["mus"][far], rtol=1e-12, atol=1e-13)
        r_dev = AH.adjoint_residual(p, q, xq, step, sq)
        r_orc = AH.adjoint_residual(p, q, xq, ref, sq)
        assert r_dev <= 3 * r_orc, (q, r_dev, r_orc)
        smax = max(np.abs(np.concatenate(step)).max(), 1.0)
        assert np.abs(np.concatenate(step) - np.concatenate(ref)).max() <= 1e-5 * smax, q  # (forward error, cond(V) ~ 1e11)
        scale = smax * max(np.abs(np.concatenate(xq)).max(), 1.0)
        tab = AH.gradient_table(AH.one_qp(p, q), xq, step)
        for k in AH.MPC_SEQ:
            np.testing.assert_allclose(res[k][q], tab[k], rtol=1e-13, atol=1e-15 * scale, err_msg=k)


_ONE_PER_KERNEL = [next(i for i, (_, n) in enumerate(_MPC_SHAPES) if n == name)
                   for name in dict.fromkeys(n for _, n in _MPC_SHAPES)]


ONE_ROW = ("fbstab_mpc_r16_kernel<12,4,20>", "fbstab_mpc_r16_kernel<12,4,32>")


@pytest.mark.parametrize("idx", _ONE_PER_KERNEL, ids=[_MPC_SHAPES[i][1] for i in _ONE_PER_KERNEL])
def test_adjoint_residual_against_the_oracle_on_one_shape_per_solve_kernel(hip, oracle, monkeypatch, idx):
    """At the device's solutions of random LTV QPs, on one shape per solve kernel: V (dz, dl, dv) = (gz, -gl, -C.gv)
    within 3 x the oracle's residual (longdouble), and the gradients are the table applied to the returned adjoint.
    The one-row record instances' handles run the RECORD adjoint (fbstab_mpc_r16_adjoint_kernel) - a kernel of
    its own: its bits are not the flat-vector adjoint's, which the same QPs are put through as well (FBSTAB_HIP_GENERIC)
    and checked by the same rule; the other handles run the flat-vector adjoint."""
    shape, kern = _MPC_SHAPES[idx]
    monkeypatch.setenv("FBSTAB_HIP_GENERIC", "1" if kern == "fbstab_mpc_kernel<64>" else "0")
    p = fx.random_ltv_mpc(np.random.default_rng(7100 + idx), 3, *shape)
    s, x, out = _solve(hip, p)
    assert s.kernel_name() == kern
    seeds = AH.random_seeds(np.random.default_rng(idx), p)
    res = s.Adjoint(p.arrays, *x, *seeds, adj=True)
    _check_residual_and_table(oracle, p, x, seeds, res)
    if kern in ONE_ROW:
        monkeypatch.setenv("FBSTAB_HIP_GENERIC", "1")
        flat = hip.FBstabMpcBatch(*p.sizes(), max_batch=p.batch).Adjoint(p.arrays, *x, *seeds, adj=True)
        _check_residual_and_table(oracle, p, x, seeds, flat)
        assert not all(np.array_equal(res[k], flat[k]) for k in ("dz", "dl", "dv"))


def test_adjoint_residual_against_the_oracle_on_the_baseline_batch(hip, oracle):
    p = fx.synthetic_mpc_batch(8)
    s, x, out = _solve(hip, p)
    assert (out["eflag"] == 0).all()
    seeds = AH.random_seeds(np.random.default_rng(3), p)
    res = s.Adjoint(p.arrays, *x, *seeds, adj=True)
    _check_residual_and_table(oracle, p, x, seeds, res)


def _sym_direction(rng, n, stages):
    M = rng.standard_normal((stages, n, n))
    return (M + np.transpose(M, (0, 2, 1))).reshape(stages, -1).reshape(-1) / 2


def test_central_differences_of_the_solution_map(hip):
    """Random LTV QPs solved at abs_tol = 1e-11; QPs strictly complementary at 1e-3 (every row: y or v at least
    1e-3).  For a random linear loss L = a'z + b'l + c'v, central differences along a random direction of each
    of the 12 sequences (symmetric stage blocks for Q and R) match the adjoint's directional derivative."""
    rng = np.random.default_rng(8801)
    shape = (6, 4, 2, 6)
    base = fx.random_ltv_mpc(rng, 8, *shape)
    o = default_options(abs_tol=1e-11)
    s, x, out = _solve(hip, base, o)
    assert (out["eflag"] == 0).all()
    y = np.stack([H.mpc_explicit(base, q)[5] - H.mpc_explicit(base, q)[4] @ x[0][q] for q in range(base.batch)])
    strict = [q for q in range(base.batch) if np.maximum(y[q], x[2][q]).min() >= 1e-3]
    assert len(strict) >= 3, strict
    seeds = AH.random_seeds(rng, base)
    grad = s.Adjoint(base.arrays, *x, *seeds)
    N, nx, nu, nc = shape
    h = 1e-5
    dirs = {}
    for k, n in base.seq_lengths().items():
        if k == "Q":
            dirs[k] = _sym_direction(rng, nx, N + 1)
        elif k == "R":
            dirs[k] = _sym_direction(rng, nu, N + 1)
        else:
            dirs[k] = rng.standard_normal(n)
    # one batch: QP q, sequence k, sign
    cases = [(q, k, sg) for q in strict for k in AH.MPC_SEQ for sg in (1.0, -1.0)]
    arr = {k: np.ascontiguousarray(np.stack([base.arrays[k][q] + (sg * h * dirs[k] if kk == k else 0.0)
                                             for q, kk, sg in cases])) for k in AH.MPC_SEQ}
    pert = fx.MpcProblem(N, nx, nu, nc, arr)
    _, xp, outp = _solve(hip, pert, o)
    assert (outp["eflag"] == 0).all()
    loss = lambda j: sum(float(seeds[t][cases[j][0]] @ xp[t][j]) for t in range(3))
    for j in range(0, len(cases), 2):
        q, k, _ = cases[j]
        fd = (loss(j) - loss(j + 1)) / (2 * h)
        ad = float(grad[k][q] @ dirs[k])
        assert abs(fd - ad) <= 1e-4 * max(abs(ad), 1e-2 * np.abs(grad[k][q]).sum()), (q, k, fd, ad)


def _lqr_gain(p):
    """-K_0 of the finite-horizon Riccati recursion of QP 0 (stage cost 1/2 [x;u]'[Q S';S R][x;u], the
    terminal stage's input eliminated)."""
    N, nx, nu, nc = p.sizes()
    a = {k: v[0] for k, v in p.arrays.items()}
    mat = lambda key, i, r, c: a[key][i * r * c:(i + 1) * r * c].reshape(c, r).T
    Q, R, S = (lambda i: mat("Q", i, nx, nx)), (lambda i: mat("R", i, nu, nu)), (lambda i: mat("S", i, nu, nx))
    P = Q(N) - S(N).T @ np.linalg.solve(R(N), S(N))
    K = None
    for i in range(N - 1, -1, -1):
        A, B = mat("A", i, nx, nx), mat("B", i, nx, nu)
        Quu, Qux, Qxx = R(i) + B.T @ P @ B, S(i) + B.T @ P @ A, Q(i) + A.T @ P @ A
        K = np.linalg.solve(Quu, Qux)
        P = Qxx - Qux.T @ K
    return -K


def test_lqr_gain_from_seeded_input_rows(hip):
    """All constraints inactive: du0/dx0 from nu QPs seeded with the unit vectors of u0 equals -K_0 of the
    Riccati recursion.  With an upper bound on input j active at stage 0, row j of du0/dx0 is zero."""
    N, nx, nu, nc = 8, 4, 2, 1
    p = fx.random_ltv_mpc(np.random.default_rng(4401), 1, N, nx, nu, nc)
    for k in ("q", "r", "c"):
        p.arrays[k][:] = 0.0
    p.arrays["E"][:] = 0.0
    p.arrays["L"][:] = 0.0
    p.arrays["d"][:] = -1.0   # 0 <= 1 on every row: inactive, y = 1, v = 0
    K = _lqr_gain(p)
    u0 = K @ p.arrays["x0"][0]
    if u0[0] < 0:
        p.arrays["x0"][:] *= -1.0
        u0 = -u0

    def rows(prob):
        rep = fx.MpcProblem(N, nx, nu, nc, {k: np.ascontiguousarray(np.repeat(v, nu, axis=0)) for k, v in prob.arrays.items()})
        o = default_options(abs_tol=1e-11)
        s, x, out = _solve(hip, rep, o)
        assert (out["eflag"] == 0).all()
        gz = np.zeros((nu, rep.nz))
        for j in range(nu):
            gz[j, nx + j] = 1.0
        g = s.Adjoint(rep.arrays, *x, gz, want=("x0",))
        return g["x0"], x

    J, x = rows(p)
    np.testing.assert_allclose(x[0][0][nx:nx + nu], u0, rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(J, K, rtol=1e-6, atol=1e-9 * np.abs(K).max())
    # input 0 bounded at stage 0 by half its unconstrained value: L = e_0, d = -u_max on stage 0's row
    b = fx.MpcProblem(N, nx, nu, nc, {k: v.copy() for k, v in p.arrays.items()})
    b.arrays["L"][0, 0] = 1.0
    b.arrays["d"][0, 0] = -0.5 * u0[0]
    Jb, xb = rows(b)
    assert abs(xb[0][0][nx] - 0.5 * u0[0]) <= 1e-8 * abs(u0[0]) and xb[2][0][0] > 1e-6
    assert np.abs(Jb[0]).max() <= 1e-6 * np.abs(K).max()


def test_gradients_are_bitwise_the_same_alone_packed_and_queued(hip, monkeypatch):
    """QP gradients do not depend on where the queue puts them: alone, in a batch on two workgroups (every
    workgroup re-fetching), and in a batch on the whole grid."""
    p = fx.random_ltv_mpc(np.random.default_rng(5150), 24, 5, 6, 3, 8)
    s, x, out = _solve(hip, p)
    seeds = AH.random_seeds(np.random.default_rng(9), p)
    full = s.Adjoint(p.arrays, *x, *seeds, adj=True)
    monkeypatch.setenv(CAP, "2")
    packed_h = hip.FBstabMpcBatch(*p.sizes(), max_batch=p.batch)
    assert packed_h.query()["workgroups"] == 2 < p.batch
    packed = packed_h.Adjoint(p.arrays, *x, *seeds, adj=True)
    monkeypatch.delenv(CAP)
    alone_h = hip.FBstabMpcBatch(*p.sizes(), max_batch=1)
    for q in (0, 7, 23):
        one = {k: np.ascontiguousarray(a[q:q + 1]) for k, a in p.arrays.items()}
        alone = alone_h.Adjoint(one, *(t[q:q + 1] for t in x), *(t[q:q + 1] for t in seeds), adj=True)
        for k in AH.MPC_SEQ + ("dz", "dl", "dv"):
            assert np.array_equal(alone[k][0], full[k][q]), (q, k)
    for k in AH.MPC_SEQ + ("dz", "dl", "dv"):
        assert np.array_equal(packed[k], full[k]), k


def test_autograd_matches_the_c_abi_and_zeroes_unsolved_qps(hip):
    """loss.backward() through fbstab_amd.autograd on device tensors: the gradients of the inputs that require
    grad equal the C-ABI call's at the returned points (bitwise), the others get none, and a QP that is not
    SUCCESS (here primal infeasible) gets zero gradients."""
    import torch
    from fbstab_amd.autograd import solve_mpc
    dev = torch.device("cuda:0")
    N, nx, nu, nc = 6, 4, 2, 6
    p = fx.random_ltv_mpc(np.random.default_rng(6060), 4, N, nx, nu, nc)
    # QP 1: u_0(0) <= -1 and u_0(0) >= 1 on stage 0's first two rows
    for r, sgn in ((0, 1.0), (1, -1.0)):
        p.arrays["E"][1, r:(N + 1) * nc * nx:nc][:nx] = 0.0
        for j in range(nu):
            p.arrays["L"][1, r + j * nc] = sgn if j == 0 else 0.0
        p.arrays["d"][1, r] = 1.0
    solver = hip.FBstabMpcBatch(N, nx, nu, nc, max_batch=p.batch)
    want = ("Q", "q", "A", "E", "d", "x0")
    data = {k: torch.from_numpy(v.copy()).to(dev).requires_grad_(k in want) for k, v in p.arrays.items()}
    z, l, v, out = solve_mpc(solver, data)
    eflag = hip.out_to_numpy(out)["eflag"]
    assert eflag[1] != 0 and (np.delete(eflag, 1) == 0).all(), eflag
    rng = np.random.default_rng(12)
    a, b, c = (torch.from_numpy(t).to(dev) for t in AH.random_seeds(rng, p))
    loss = (a * z).sum() + (b * l).sum() + (c * v).sum()
    loss.backward()
    ref = solver.Adjoint({k: t.detach() for k, t in data.items()}, z.detach(), l.detach(), v.detach(), a, b, c)
    torch.cuda.synchronize()
    for k in AH.MPC_SEQ:
        if k not in want:
            assert data[k].grad is None, k
            continue
        g = data[k].grad.cpu().numpy()
        r = ref[k].cpu().numpy()
        assert np.array_equal(g[[0, 2, 3]], r[[0, 2, 3]]), k
        assert np.array_equal(g[1], np.zeros_like(g[1])), k
        assert np.abs(r[[0, 2, 3]]).max() > 0, k
