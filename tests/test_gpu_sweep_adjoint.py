"""GPU checks of the closed loop's derivative: the logged sweep (fbstab_hip_mpc_receding_sweep_logged), its
adjoint through time (fbstab_hip_mpc_receding_sweep_adjoint: fbstab_mpc_r16_sweep_adjoint_kernel in one launch,
or the per-step form) and fbstab_amd.autograd.closed_loop_mpc."""
import numpy as np
import pytest

from oracle.oracle_py import default_options
from fbstab_amd.hip_api import MPC_SEQ
from tests import helpers as H
from tests import sweep_adjoint_helpers as SH
from tools import fixtures as fx

pytestmark = pytest.mark.gpu

CAP = "FBSTAB_HIP_MAX_WORKGROUPS"
PER_STEP = "fbstab_sweep_costate_kernel"

# (shape, environment, what RecedingSweepAdjoint launches): one per adjoint kernel, and the per-step form
CASES = [
    ((3, 5, 2, 7), {}, "fbstab_mpc_r16_sweep_adjoint_kernel<12,4,20>"),      # padded
    ((3, 12, 4, 20), {}, "fbstab_mpc_r16_sweep_adjoint_kernel<12,4,20>"),    # exact
    ((3, 12, 4, 32), {}, "fbstab_mpc_r16_sweep_adjoint_kernel<12,4,32>"),
    ((4, 18, 5, 10), {"FBSTAB_HIP_FLAT_ADJOINT": "0"}, "fbstab_mpc_r16_sweep_adjoint_kernel<18,5,10>"),
    ((3, 5, 2, 7), {"FBSTAB_HIP_GENERIC": "1"}, PER_STEP),
]
IDS = ["5-2-7-padded", "12-4-20-exact", "12-4-32", "18-5-10-row-pair", "5-2-7-generic"]


@pytest.fixture(scope="module")
def hip():
    from fbstab_amd import hip_api
    assert hip_api.load_library().fbstab_hip_device_count() >= 1
    return hip_api


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda:0"))


def _sweep(hip, solver, p, A, B, steps, retire=True, log=True, opts=None):
    """One sweep from a zero guess on device copies of ``p``: the result dict in numpy (``x0``: the final states)."""
    import torch
    if opts is not None:
        solver.UpdateOptions(H._opts(hip, opts))
    data = {k: _dev(a) for k, a in p.arrays.items()}
    mk = lambda n: torch.zeros((p.batch, n), dtype=torch.float64, device=data["Q"].device)
    z, l, v, y = mk(p.nz), mk(p.nl), mk(p.nv), mk(p.nv)
    r = solver.RecedingSweep(data, z, l, v, y, A, B, steps, retire=retire, log_inputs=True, log=log)
    res = dict(u=r["u"].cpu().numpy(), x0=data["x0"].cpu().numpy(), z=z.cpu().numpy(), l=l.cpu().numpy(),
               v=v.cpu().numpy(), out=hip.out_to_numpy(r["out"]), stats=r["stats"])
    for k in ("z_log", "l_log", "v_log", "x_log", "eflag_log"):
        if k in r:
            res[k] = r[k].cpu().numpy()
    return res


def _np_log(r):
    return dict(z=r["z_log"], l=r["l_log"], v=r["v_log"], eflag=r["eflag_log"], x=r["x_log"])


def _adjoint(solver, p, A, B, r, gu, gx, retire=True, want=None, mu=False):
    data = {k: _dev(a) for k, a in p.arrays.items()}
    log = {k: _dev(r[k]) for k in ("z_log", "l_log", "v_log", "eflag_log")}
    g = solver.RecedingSweepAdjoint(data, A, B, r["eflag_log"].shape[0], log, gu=None if gu is None else _dev(gu),
                                    gx=None if gx is None else _dev(gx), retire=retire, want=want, mu=mu)
    return {k: t.cpu().numpy() for k, t in g.items()}


def _plant(rng, nx, nu):
    """A random plant near the identity with a small input gain: the states stay near the x0 the random QPs were
    made feasible for, so that most steps end in SUCCESS."""
    return np.eye(nx) + 0.03 * rng.standard_normal((nx, nx)), 0.1 * rng.standard_normal((nx, nu))


def test_logged_sweep_is_the_sweep_and_logs_what_it_returned(hip, monkeypatch):
    """(8, 6, 3, 5), 5 trajectories x 4 steps, one pushed infeasible and retired: the logged sweep's results are
    bitwise the unlogged sweep's, z_log holds every u, x_log the states (x_log[k+1] = A x_log[k] + B u[k] as the
    kernel forms it), a retired trajectory logs eflag -1 and zero points, and the per-step form logs the same
    bits."""
    shape, T, S = (8, 6, 3, 5), 5, 4
    N, nx, nu, nc = shape
    rng = np.random.default_rng(4242)
    p = fx.random_ltv_mpc(rng, T, *shape)
    A, B = _plant(rng, nx, nu)
    # trajectory 2: u_0(0) <= -1 and u_0(0) >= 1 on stage 0's first two rows
    for r_, sgn in ((0, 1.0), (1, -1.0)):
        p.arrays["E"][2, r_:(N + 1) * nc * nx:nc][:nx] = 0.0
        for j in range(nu):
            p.arrays["L"][2, r_ + j * nc] = sgn if j == 0 else 0.0
        p.arrays["d"][2, r_] = 1.0
    mks = lambda: hip.FBstabMpcBatch(*shape, max_batch=T)
    plain = _sweep(hip, mks(), p, A, B, S, log=False)
    logged = _sweep(hip, mks(), p, A, B, S)
    assert mks().kernel_name().startswith("fbstab_mpc_r16_kernel")
    for k in ("u", "x0", "z", "l", "v"):
        assert np.array_equal(plain[k], logged[k]), k
    for k in ("eflag", "newton_iters", "prox_iters", "residual"):
        assert np.array_equal(plain["out"][k], logged["out"][k]), k
    e = logged["eflag_log"]
    assert (e[:, 2] == -1).all() and (np.delete(e, 2, axis=1) == 0).all(), e
    for k in range(S):
        assert np.array_equal(logged["z_log"][k][:, nx:nx + nu], logged["u"][k]), k
    assert not logged["z_log"][:, 2].any() and not logged["l_log"][:, 2].any() and not logged["v_log"][:, 2].any()
    assert np.array_equal(logged["x_log"][0], p.arrays["x0"])
    live = [0, 1, 3, 4]
    from fractions import Fraction
    fma = lambda a, b, c: float(Fraction(a) * Fraction(b) + Fraction(c))   # one rounding
    for k in range(S):
        nxt = logged["x_log"][k + 1] if k + 1 < S else logged["x0"]
        for q in live:
            for t in range(nx):  # the kernel's order: A's columns, then B's, fused multiply-adds
                acc = 0.0
                for c in range(nx):
                    acc = fma(float(A[t, c]), float(logged["x_log"][k][q, c]), acc)
                for j in range(nu):
                    acc = fma(float(B[t, j]), float(logged["u"][k][q, j]), acc)
                assert acc == nxt[q, t], (k, q, t)
    assert not logged["x_log"][1:, 2].any() and not logged["x0"][2].any()
    monkeypatch.setenv("FBSTAB_HIP_SWEEP_PER_STEP", "1")
    per = _sweep(hip, mks(), p, A, B, S)
    for k in ("u", "x0", "z", "z_log", "l_log", "v_log", "x_log", "eflag_log"):
        assert np.array_equal(per[k], logged[k]), k


def _case(hip, monkeypatch, idx, batch, seed):
    shape, env, name = CASES[idx]
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    rng = np.random.default_rng(seed + idx)
    p = fx.random_ltv_mpc(rng, batch, *shape)
    A, B = _plant(rng, shape[1], shape[2])
    return shape, name, rng, p, A, B


@pytest.mark.parametrize("idx", range(len(CASES)), ids=IDS)
def test_one_step_is_the_adjoint(hip, monkeypatch, idx):
    """T = 1, gx = 0: gradients and status are bitwise those of ``Adjoint`` with gz = gu on the u0 entries, the x0
    slot included."""
    shape, name, rng, p, A, B = _case(hip, monkeypatch, idx, 3, 9100)
    N, nx, nu, nc = shape
    s = hip.FBstabMpcBatch(*shape, max_batch=p.batch)
    assert s.sweep_adjoint_kernel_name() == name
    assert (name == PER_STEP) == (not s.adjoint_kernel_name().startswith("fbstab_mpc_r16_adjoint_kernel"))
    r = _sweep(hip, s, p, A, B, 1)
    assert (r["eflag_log"] == 0).all()
    gu = rng.standard_normal((1, p.batch, nu))
    g = _adjoint(s, p, A, B, r, gu, np.zeros((1, p.batch, nx)))
    gz = np.zeros((p.batch, p.nz))
    gz[:, nx:nx + nu] = gu[0]
    ref = s.Adjoint(p.arrays, r["z_log"][0], r["l_log"][0], r["v_log"][0], gz)
    assert np.array_equal(g["status"], ref["status"]) and (ref["status"] == 0).all()
    for k in MPC_SEQ:
        assert np.abs(ref[k]).max() > 0, k
        assert np.array_equal(g[k], ref[k]), k


@pytest.mark.parametrize("idx", range(len(CASES)), ids=IDS)
def test_several_steps_against_the_composed_reference(hip, oracle, oracle_fma, monkeypatch, idx):
    """T = 4, 9 trajectories on ONE workgroup (rows take more than one trajectory): against the recursion in numpy
    over the device's own per-step ``Adjoint`` at the logged points, within ten times the spread between the two
    roundings of the reference; the per-step form is held to the same bar, and the same call twice gives the same
    bits."""
    monkeypatch.setenv(CAP, "1")
    shape, name, rng, p, A, B = _case(hip, monkeypatch, idx, 9, 9200)
    N, nx, nu, nc = shape
    T = 4
    s = hip.FBstabMpcBatch(*shape, max_batch=p.batch)
    assert s.sweep_adjoint_kernel_name() == name and s.query()["workgroups"] == 1
    r = _sweep(hip, s, p, A, B, T)
    assert (r["eflag_log"] == 0).sum() >= 3 * T
    gu, gx = rng.standard_normal((T, p.batch, nu)), rng.standard_normal((T, p.batch, nx))
    log = _np_log(r)
    bars, spread = SH.spread_bars(oracle, oracle_fma, p, A, B, log, gu, gx)
    print("spread", shape, {k: "%.1e" % v for k, v in spread.items()})
    ref, rst, rmu = SH.reference_sweep_adjoint(SH.device_step_adjoint(s, p), p, A, B, log, gu, gx)
    g = _adjoint(s, p, A, B, r, gu, gx, mu=True)
    again = _adjoint(s, p, A, B, r, gu, gx, mu=True)
    for k in MPC_SEQ + ("status", "mu"):
        assert np.array_equal(g[k], again[k]), k
    assert np.array_equal(g["status"], rst)
    SH.assert_within(g, ref, bars, name)
    np.testing.assert_allclose(g["mu"], rmu, rtol=0, atol=max(bars["x0"], 1e-12) * np.abs(rmu).max())
    if name != PER_STEP:
        monkeypatch.setenv("FBSTAB_HIP_SWEEP_ADJOINT_PER_STEP", "1")
        assert s.sweep_adjoint_kernel_name() == PER_STEP
        per = _adjoint(s, p, A, B, r, gu, gx)
        assert np.array_equal(per["status"], rst)
        SH.assert_within(per, ref, bars, PER_STEP)


@pytest.mark.parametrize("retire", [True, False], ids=["retire", "keep"])
def test_retirement_and_failed_steps(hip, oracle, oracle_fma, retire):
    """6 trajectories x 5 steps at the BASELINE shape with N = 6, two pushed infeasible: the gradients match the
    reference recursion (eflag -1 cuts the costate, a step that is no solution passes it through the plant), and
    a retired trajectory's gradients from seeds at or after its retirement step are exactly zero."""
    T, S = 6, 5
    p = fx.synthetic_mpc_batch(T, first_id=7000, N=6)
    p.arrays["x0"][1, 6:9] = [2.5, -2.5, 2.5]
    p.arrays["x0"][4, 3:6] = [40.0, -40.0, 40.0]
    N, nx, nu, nc = p.sizes()
    A, B = fx.quadrotor_model()
    s = hip.FBstabMpcBatch(N, nx, nu, nc, max_batch=T)
    r = _sweep(hip, s, p, A, B, S, retire=retire)
    e = r["eflag_log"]
    bad = sorted(set(np.flatnonzero((e != 0).any(axis=0)).tolist()))
    assert bad and len(bad) < T, e
    if retire:
        assert (e[:, bad] == -1).any() and not ((e != 0) & (e != -1)).any(), e
    else:
        assert not (e == -1).any() and (e[:, bad] > 0).any(), e
    rng = np.random.default_rng(77)
    gu, gx = rng.standard_normal((S, T, nu)), rng.standard_normal((S, T, nx))
    log = _np_log(r)
    bars, spread = SH.spread_bars(oracle, oracle_fma, p, A, B, log, gu, gx)
    print("spread", p.sizes(), retire, {k: "%.1e" % v for k, v in spread.items()})
    ref, rst, _ = SH.reference_sweep_adjoint(SH.device_step_adjoint(s, p), p, A, B, log, gu, gx, retire)
    g = _adjoint(s, p, A, B, r, gu, gx, retire=retire)
    assert np.array_equal(g["status"], rst)
    SH.assert_within(g, ref, bars, "retire" if retire else "keep")
    if retire:
        for q in bad:
            k0 = int(np.flatnonzero(e[:, q] == -1)[0])   # retirement step
            gu0, gx0 = gu.copy(), gx.copy()
            gu0[:k0], gx0[:k0] = 0.0, 0.0
            late = _adjoint(s, p, A, B, r, gu0, gx0)
            for k in MPC_SEQ:
                assert not late[k][q].any(), (q, k)


def test_known_answer_without_active_constraints(hip):
    """All constraints inactive ((8, 4, 2, 1), the plant = the QP's stage-0 model, T = 5): the closed loop is
    x+ = (A + B K_0) x with K_0 of the Riccati recursion, so dL/dx_0 = lambda_0 of
    lambda_k = (A + B K_0)'(gx_k + lambda_(k+1)) + K_0'gu_k."""
    N, nx, nu, nc = 8, 4, 2, 1
    T = 5
    p = fx.random_ltv_mpc(np.random.default_rng(4401), 1, N, nx, nu, nc)
    for k in ("q", "r", "c"):
        p.arrays[k][:] = 0.0
    p.arrays["E"][:] = 0.0
    p.arrays["L"][:] = 0.0
    p.arrays["d"][:] = -1.0
    K = H.lqr_gain(p)
    A = p.arrays["A"][0][:nx * nx].reshape(nx, nx).T.copy()
    B = p.arrays["B"][0][:nx * nu].reshape(nu, nx).T.copy()
    s = hip.FBstabMpcBatch(N, nx, nu, nc, max_batch=1)
    r = _sweep(hip, s, p, A, B, T, opts=default_options(abs_tol=1e-11))
    assert (r["eflag_log"] == 0).all()
    np.testing.assert_allclose(r["u"][0][0], K @ p.arrays["x0"][0], rtol=1e-6, atol=1e-9)
    rng = np.random.default_rng(5)
    gu, gx = rng.standard_normal((T, 1, nu)), rng.standard_normal((T, 1, nx))
    g = _adjoint(s, p, A, B, r, gu, gx, want=("x0",))
    lam = np.zeros(nx)
    for k in range(T - 1, -1, -1):
        lam = (A + B @ K).T @ (gx[k, 0] + lam) + K.T @ gu[k, 0]
    np.testing.assert_allclose(g["x0"][0], lam, rtol=1e-6, atol=1e-9 * np.abs(lam).max())


def test_central_differences_of_the_closed_loop_on_the_device(hip):
    """The CPU test's problem and rule (tests/test_sweep_adjoint_cpu.py) with the forward run through
    ``RecedingSweep`` at abs_tol = 1e-11 and the gradients from ``RecedingSweepAdjoint``."""
    p, A, B, cu, cx, dirs = SH.fd_problem()
    o = default_options(abs_tol=1e-11)
    s = hip.FBstabMpcBatch(*p.sizes(), max_batch=p.batch)
    r = _sweep(hip, s, p, A, B, SH.FD_STEPS, opts=o)
    good = SH.strictly_complementary(p, _np_log(r))
    assert len(good) >= 3, good
    g = _adjoint(s, p, A, B, r, cu, cx)

    def run(prob):
        rr = _sweep(hip, s, prob, A, B, SH.FD_STEPS, log=True)
        return rr["u"], np.concatenate([rr["x_log"][1:], rr["x0"][None]], 0)

    figures = SH.fd_check(run, g, good, p, cu, cx, dirs)
    for name, q, fd, ad, bound in figures:
        print(f"{name:3s} q {q} fd {fd:+.9e} ad {ad:+.9e} |fd-ad| {abs(fd - ad):.2e} bound {bound:.2e}")
    for name, q, fd, ad, bound in figures:
        assert abs(fd - ad) <= bound, (name, q, fd, ad, bound)


def test_closed_loop_autograd(hip, monkeypatch):
    """closed_loop_mpc on (6, 4, 2, 6), 4 trajectories x 3 steps, a loss quadratic in u and x: backward() fills
    q, Q (per trajectory), a shared R, x0 and the plant's A and B with what RecedingSweepAdjoint gives for the
    autograd seeds, and asks the library for nothing else."""
    import torch
    from fbstab_amd.autograd import closed_loop_mpc
    shape, Bn, T = (6, 4, 2, 6), 4, 3
    N, nx, nu, nc = shape
    rng = np.random.default_rng(6161)
    p = fx.random_ltv_mpc(rng, Bn, *shape)
    p.arrays["R"][:] = p.arrays["R"][0]
    An, Bm = _plant(rng, nx, nu)
    solver = hip.FBstabMpcBatch(*shape, max_batch=Bn)
    want = ("Q", "R", "q", "x0")
    data = {k: _dev(a[0] if k == "R" else a).requires_grad_(k in want) for k, a in p.arrays.items()}
    assert data["R"].dim() == 1
    A, B = _dev(An).requires_grad_(True), _dev(Bm).requires_grad_(True)
    asked = []
    real = solver.RecedingSweepAdjoint
    monkeypatch.setattr(solver, "RecedingSweepAdjoint",
                        lambda *a, **kw: (asked.append(tuple(kw["want"])), real(*a, **kw))[1])
    u, x, out = closed_loop_mpc(solver, data, A, B, T)
    assert u.shape == (T, Bn, nu) and x.shape == (T, Bn, nx)
    assert (hip.out_to_numpy(out)["eflag"] == 0).all()
    wu, wx = _dev(rng.standard_normal((T, Bn, nu))), _dev(rng.standard_normal((T, Bn, nx)))
    loss = 0.5 * (wu * u * u).sum() + 0.5 * (wx * x * x).sum()
    loss.backward()
    assert asked == [want]
    monkeypatch.undo()
    # by hand: the same sweep, the autograd seeds
    r = _sweep(hip, solver, p, An, Bm, T)
    assert np.array_equal(r["u"], u.detach().cpu().numpy())
    xs = np.concatenate([r["x_log"][1:], r["x0"][None]], 0)
    assert np.array_equal(xs, x.detach().cpu().numpy())
    gu, gx = wu.cpu().numpy() * r["u"], wx.cpu().numpy() * xs
    g = _adjoint(solver, p, An, Bm, r, gu, gx, want=want, mu=True)
    assert (g["status"] == 0).all()
    for k in MPC_SEQ:
        if k not in want:
            assert data[k].grad is None, k
            continue
        got = data[k].grad.cpu().numpy()
        assert got.shape == data[k].shape
        exp = g[k].sum(0) if k == "R" else g[k]
        assert np.abs(exp).max() > 0, k
        if k == "R":
            np.testing.assert_allclose(got, exp, rtol=1e-13, atol=1e-15 * np.abs(g[k]).max() * Bn)
        else:
            assert np.array_equal(got, exp), k
    gA = np.einsum("kbi,kbj->ij", g["mu"], r["x_log"])
    gB = np.einsum("kbi,kbj->ij", g["mu"], r["u"])
    np.testing.assert_allclose(A.grad.cpu().numpy(), gA, rtol=1e-12, atol=1e-14 * np.abs(gA).max())
    np.testing.assert_allclose(B.grad.cpu().numpy(), gB, rtol=1e-12, atol=1e-14 * np.abs(gB).max())
