"""GPU checks of the MPC adjoint (fbstab_hip_mpc_adjoint_batch, FBstabMpcBatch.Adjoint, fbstab_amd.autograd):
the adjoint system's residual against the oracle's linear solver on one shape per solve kernel (the one-row
record instances' own adjoint and the flat-vector one) and on the BASELINE batch, the gradient table, central differences of the solution map, the LQR gain, bitwise
invariance under the queue, and torch autograd."""
import numpy as np
import pytest

from fbstab_amd.hip_api import MPC_SEQ
from tools import fixtures as fx
from oracle.oracle_py import default_options
from tests import helpers as H
from tests import linear_reference as LR
from tests.shapes import MPC_SHAPES

pytestmark = pytest.mark.gpu

CAP = "FBSTAB_HIP_MAX_WORKGROUPS"


@pytest.fixture(scope="module")
def hip():
    from fbstab_amd import hip_api
    assert hip_api.load_library().fbstab_hip_device_count() >= 1
    return hip_api


_ONE_PER_KERNEL = [next(i for i, (_, n) in enumerate(MPC_SHAPES) if n == name)
                   for name in dict.fromkeys(n for _, n in MPC_SHAPES)]


ONE_ROW = ("fbstab_mpc_r16_kernel<12,4,20>", "fbstab_mpc_r16_kernel<12,4,32>")


@pytest.mark.parametrize("idx", _ONE_PER_KERNEL, ids=[MPC_SHAPES[i][1] for i in _ONE_PER_KERNEL])
def test_adjoint_residual_against_the_oracle_on_one_shape_per_solve_kernel(hip, oracle, monkeypatch, idx):
    """At the device's solutions of random LTV QPs, on one shape per solve kernel: V (dz, dl, dv) = (gz, -gl, -C.gv)
    within 3 x the oracle's residual (longdouble), and the gradients are the table applied to the returned adjoint.
    The one-row record instances' handles run the RECORD adjoint (fbstab_mpc_r16_adjoint_kernel) - a kernel of
    its own: its bits are not the flat-vector adjoint's, which the same QPs are put through as well (FBSTAB_HIP_GENERIC)
    and checked by the same rule; the other handles run the flat-vector adjoint."""
    shape, kern = MPC_SHAPES[idx]
    monkeypatch.setenv("FBSTAB_HIP_GENERIC", "1" if kern == "fbstab_mpc_kernel<64>" else "0")
    p = fx.random_ltv_mpc(np.random.default_rng(7100 + idx), 3, *shape)
    s, x, out = H.cold_solve(hip, p)
    assert s.kernel_name() == kern
    seeds = LR.random_seeds(np.random.default_rng(idx), p)
    res = s.Adjoint(p.arrays, *x, *seeds, adj=True)
    LR.check_mpc_batch(oracle, p, x, seeds, res)
    if kern in ONE_ROW:
        monkeypatch.setenv("FBSTAB_HIP_GENERIC", "1")
        flat = hip.FBstabMpcBatch(*p.sizes(), max_batch=p.batch).Adjoint(p.arrays, *x, *seeds, adj=True)
        LR.check_mpc_batch(oracle, p, x, seeds, flat)
        assert not all(np.array_equal(res[k], flat[k]) for k in ("dz", "dl", "dv"))


def test_adjoint_residual_against_the_oracle_on_the_baseline_batch(hip, oracle):
    p = fx.synthetic_mpc_batch(8)
    s, x, out = H.cold_solve(hip, p)
    assert (out["eflag"] == 0).all()
    seeds = LR.random_seeds(np.random.default_rng(3), p)
    res = s.Adjoint(p.arrays, *x, *seeds, adj=True)
    LR.check_mpc_batch(oracle, p, x, seeds, res)


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
    s, x, out = H.cold_solve(hip, base, o)
    assert (out["eflag"] == 0).all()
    y = np.stack([H.mpc_explicit(base, q)[5] - H.mpc_explicit(base, q)[4] @ x[0][q] for q in range(base.batch)])
    strict = [q for q in range(base.batch) if np.maximum(y[q], x[2][q]).min() >= 1e-3]
    assert len(strict) >= 3, strict
    seeds = LR.random_seeds(rng, base)
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
    cases = [(q, k, sg) for q in strict for k in MPC_SEQ for sg in (1.0, -1.0)]
    arr = {k: np.ascontiguousarray(np.stack([base.arrays[k][q] + (sg * h * dirs[k] if kk == k else 0.0)
                                             for q, kk, sg in cases])) for k in MPC_SEQ}
    pert = fx.MpcProblem(N, nx, nu, nc, arr)
    _, xp, outp = H.cold_solve(hip, pert, o)
    assert (outp["eflag"] == 0).all()
    loss = lambda j: sum(float(seeds[t][cases[j][0]] @ xp[t][j]) for t in range(3))
    for j in range(0, len(cases), 2):
        q, k, _ = cases[j]
        fd = (loss(j) - loss(j + 1)) / (2 * h)
        ad = float(grad[k][q] @ dirs[k])
        assert abs(fd - ad) <= 1e-4 * max(abs(ad), 1e-2 * np.abs(grad[k][q]).sum()), (q, k, fd, ad)


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
    K = H.lqr_gain(p)
    u0 = K @ p.arrays["x0"][0]
    if u0[0] < 0:
        p.arrays["x0"][:] *= -1.0
        u0 = -u0

    def rows(prob):
        rep = fx.MpcProblem(N, nx, nu, nc, {k: np.ascontiguousarray(np.repeat(v, nu, axis=0)) for k, v in prob.arrays.items()})
        o = default_options(abs_tol=1e-11)
        s, x, out = H.cold_solve(hip, rep, o)
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
    s, x, out = H.cold_solve(hip, p)
    seeds = LR.random_seeds(np.random.default_rng(9), p)
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
        for k in MPC_SEQ + ("dz", "dl", "dv"):
            assert np.array_equal(alone[k][0], full[k][q]), (q, k)
    for k in MPC_SEQ + ("dz", "dl", "dv"):
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
    a, b, c = (torch.from_numpy(t).to(dev) for t in LR.random_seeds(rng, p))
    loss = (a * z).sum() + (b * l).sum() + (c * v).sum()
    loss.backward()
    ref = solver.Adjoint({k: t.detach() for k, t in data.items()}, z.detach(), l.detach(), v.detach(), a, b, c)
    torch.cuda.synchronize()
    for k in MPC_SEQ:
        if k not in want:
            assert data[k].grad is None, k
            continue
        g = data[k].grad.cpu().numpy()
        r = ref[k].cpu().numpy()
        assert np.array_equal(g[[0, 2, 3]], r[[0, 2, 3]]), k
        assert np.array_equal(g[1], np.zeros_like(g[1])), k
        assert np.abs(r[[0, 2, 3]]).max() > 0, k
