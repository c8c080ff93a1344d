"""GPU checks of the scenario sweep (fbstab_hip_mpc_receding_sweep_scenario): the disturbed plant
x_(k+1) = A x_k + B u_k + w_k and the shifted warm start, in the one-launch form (receding_plant_step) and in the
per-step form (fbstab_receding_plant_kernel), and ``closed_loop_mpc(..., w=, shift=)``.  The problems P1 .. P6 are
tests/scenario_helpers.problem's; every one of them ends every solve in SUCCESS on the oracle's loop, shifted or
not, unless a test pushes a trajectory infeasible itself."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle.oracle_py import default_options
from tests import helpers as H
from tests import closed_loop as CL
from tests import scenario_helpers as SC
from tests import sweep_adjoint_helpers as SH
from tools import fixtures as fx

pytestmark = pytest.mark.gpu

PER_STEP_ENV = "FBSTAB_HIP_SWEEP_PER_STEP"
OUT_FIELDS = ("eflag", "newton_iters", "prox_iters", "residual")
LOGS = ("z_log", "l_log", "v_log", "x_log", "eflag_log")


@pytest.fixture(scope="module")
def hip():
    from fbstab_amd import hip_api
    assert hip_api.load_library().fbstab_hip_device_count() >= 1
    return hip_api


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda:0"))


def _solver(hip, p, kernel, opts=None):
    s = hip.FBstabMpcBatch(*p.sizes(), max_batch=p.batch)
    assert s.kernel_name() == kernel, s.kernel_name()
    if opts is not None:
        s.UpdateOptions(H._opts(hip, opts))
    return s


def _state(p):
    """Device copies of the data and a zero point."""
    import torch
    data = {k: _dev(a) for k, a in p.arrays.items()}
    mk = lambda n: torch.zeros((p.batch, n), dtype=torch.float64, device=data["Q"].device)
    return data, [mk(p.nz), mk(p.nl), mk(p.nv), mk(p.nv)]


def _numpy(hip, r, data, X):
    res = dict(u=r["u"].cpu().numpy(), x0=data["x0"].cpu().numpy(), z=X[0].cpu().numpy(), l=X[1].cpu().numpy(),
               v=X[2].cpu().numpy(), stats=r["stats"].copy())
    o = hip.out_to_numpy(r["out"])
    res.update({f: o[f].copy() for f in OUT_FIELDS})
    res.update({k: r[k].cpu().numpy() for k in LOGS})
    return res


def _sweep(hip, s, p, A, B, steps, retire=True, w=None, shift=False):
    """One logged sweep from a zero point on device copies of ``p``, through ``RecedingSweep``."""
    data, X = _state(p)
    r = s.RecedingSweep(data, *X, A, B, steps, retire=retire, log_inputs=True, log=True,
                        w=None if w is None else _dev(w), shift=shift)
    return _numpy(hip, r, data, X)


def _raw_scenario(hip, s, p, A, B, steps, retire, scenario):
    """The entry point itself with a log and ``scenario`` as given (a ctypes pointer or None)."""
    import torch
    data, X = _state(p)
    dev = X[0].device
    blk, flags = hip._MpcBatch(), []
    T = hip._fill_block(blk, hip.MPC_SEQ, s.seq_len, data, None, flags, shared=False)
    vb = hip._fill_vars(tuple(X), (s.nz, s.nl, s.nv, s.nv), T, flags)
    assert all(flags) and T == p.batch
    plant, keep = s._plant(A, B, dev)
    out = torch.zeros((T, 40), dtype=torch.uint8, device=dev)
    mk = lambda n: torch.zeros((steps, T, n), dtype=torch.float64, device=dev)
    r = dict(out=out, u=mk(s.nu), z_log=mk(s.nz), l_log=mk(s.nl), v_log=mk(s.nv), x_log=mk(s.nx),
             eflag_log=torch.zeros((steps, T), dtype=torch.int32, device=dev))
    lg = hip._SweepLog(*[r[k].data_ptr() for k in LOGS])
    stats = np.zeros((steps, 4), dtype=np.uint64)
    rc = s._lib.fbstab_hip_mpc_receding_sweep_scenario(
        s._h, T, C.byref(blk), C.byref(vb), out.data_ptr(), C.byref(plant), steps, 1 if retire else 0,
        r["u"].data_ptr(), stats.ctypes.data, None, None, C.byref(lg), scenario)
    assert rc == 0, s._lib.fbstab_hip_last_error()
    st = np.zeros(steps, dtype=[("newton_sum", np.int64), ("success", np.int64), ("retired_total", np.int64),
                                ("newton_max", np.int64)])
    for j, n in enumerate(st.dtype.names):
        st[n] = stats[:, j].astype(np.int64)
    r["stats"] = st
    return _numpy(hip, r, data, X)


def _same(a, b, what, keys=("u", "x0", "z", "l", "v") + LOGS + OUT_FIELDS, bitwise=True):
    for k in keys:
        if bitwise:
            assert a[k].tobytes() == b[k].tobytes(), (what, k)
        else:
            assert (a[k] == b[k]).all(), (what, k)
    for k in a["stats"].dtype.names:
        assert np.array_equal(a["stats"][k], b["stats"][k]), (what, "stats", k)


def _infeasible_p1():
    p, A, B, w, S, kernel = SC.problem("P1")
    p.arrays["x0"][5, 6:9] = [2.5, -2.5, 2.5]     # attitude far beyond its bound
    return p, A, B, w, S, kernel


# ---- G1 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["one_launch", "per_step"])
def test_nothing_moves_by_default(hip, monkeypatch, form):
    """P1 with trajectory 5 pushed infeasible and retired: the logged sweep against the new entry point with
    scenario = NULL, bitwise on the inputs, the final state, the point, all five logs, the statistics and the
    SolverOut fields; and against an all-zero ``w`` under ``==`` (the one addition may turn a -0 into +0)."""
    if form == "per_step":
        monkeypatch.setenv(PER_STEP_ENV, "1")
    p, A, B, w, S, kernel = _infeasible_p1()
    s = _solver(hip, p, kernel)
    ref = _sweep(hip, s, p, A, B, S)
    assert (ref["eflag_log"][:, 5] == -1).any() and ref["stats"]["retired_total"][-1] == 1
    assert ref["stats"]["newton_sum"].sum() > 0 and np.abs(ref["u"]).max() > 0
    _same(ref, _raw_scenario(hip, s, p, A, B, S, True, None), "scenario = NULL")
    off = hip._SweepScenario(None, 0)
    _same(ref, _raw_scenario(hip, s, p, A, B, S, True, C.byref(off)), "w = NULL, shift = 0")
    _same(ref, _sweep(hip, s, p, A, B, S, w=np.zeros_like(w)), "w = 0", bitwise=False)
    s.close()


def test_shift_outside_zero_and_one_is_refused(hip):
    p, A, B, w, S, kernel = SC.problem("P1")
    s = _solver(hip, p, kernel)
    data, X = _state(p)
    blk, flags = hip._MpcBatch(), []
    T = hip._fill_block(blk, hip.MPC_SEQ, s.seq_len, data, None, flags, shared=False)
    vb = hip._fill_vars(tuple(X), (s.nz, s.nl, s.nv, s.nv), T, flags)
    plant, keep = s._plant(A, B, X[0].device)
    import torch
    out = torch.zeros((T, 40), dtype=torch.uint8, device=X[0].device)
    for bad in (2, -1):
        sc = hip._SweepScenario(None, bad)
        rc = s._lib.fbstab_hip_mpc_receding_sweep_scenario(
            s._h, T, C.byref(blk), C.byref(vb), out.data_ptr(), C.byref(plant), S, 1, None, None, None, None, None,
            C.byref(sc))
        assert rc == 1 and b"shift is 0 or 1" in s._lib.fbstab_hip_last_error(), bad
    assert not X[0].any() and np.array_equal(data["x0"].cpu().numpy(), p.arrays["x0"])   # nothing ran
    s.close()


# ---- G2, G4, G5: one call against a step at a time --------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _stepwise(pid, rows):
    """Problem ``pid`` (its first ``rows`` trajectories), retire off, shift on: ONE call of S steps, and S calls of
    one step each given w[k:k+1] and shift = 0, the point moved by torch slice copies between the calls.  Returns
    (problem pieces, the one call's results, the step-at-a-time results in the same layout, and per step what the
    device was about to solve: x0 and the shifted guess)."""
    import torch
    from fbstab_amd import hip_api as hip
    p, A, B, w, S, kernel = SC.problem(pid)
    p, w = SC.take(p, np.arange(rows)), np.ascontiguousarray(w[:, :rows])
    s = _solver(hip, p, kernel)
    one = _sweep(hip, s, p, A, B, S, retire=False, w=w, shift=True)
    s.close()
    s = _solver(hip, p, kernel)
    data, X = _state(p)
    wd = _dev(w)
    parts, before = [], []
    for k in range(S):
        before.append(dict(x0=data["x0"].cpu().numpy().copy(), guess=tuple(t.cpu().numpy().copy() for t in X[:3])))
        r = s.RecedingSweep(data, *X, A, B, 1, retire=False, log_inputs=True, log=True, w=wd[k:k + 1], shift=False)
        parts.append(_numpy(hip, r, data, X))
        if k + 1 < S:
            CL.shift_point(X[0], X[1], X[2], p.sizes())
    s.close()
    per = {k: np.concatenate([q[k] for q in parts], 0) for k in ("u",) + LOGS}
    per.update({k: parts[-1][k] for k in ("x0", "z", "l", "v") + OUT_FIELDS})
    per["stats"] = np.concatenate([q["stats"] for q in parts])
    per["steps"] = parts
    return (p, A, B, w, S), one, per, before


@pytest.mark.parametrize("pid,rows", [("P1", 11), ("P2", 12), ("P3", 12), ("P4", 12), ("P5", 6), ("P6", 6)])
def test_one_call_equals_a_step_at_a_time(hip, pid, rows):
    """The shift and the disturbance of the kernels against the same loop driven from outside: bitwise on the
    inputs, the logs, the final state, the final point and the SolverOut fields (P1 on 11 trajectories: its third
    wavefront is partly filled)."""
    (p, A, B, w, S), one, per, before = _stepwise(pid, rows)
    assert (one["eflag_log"] == 0).all(), one["eflag_log"]
    assert np.abs(one["u"]).max() > 0 and np.abs(w).max() > 0
    _same(one, per, pid)
    # the log holds returned points, unshifted: the last step's is the point left in x
    assert np.array_equal(one["z_log"][-1], one["z"]) and np.array_equal(one["v_log"][-1], one["v"])
    # ... and the shift was exercised: the guess of step 1 is step 0's point moved by one stage
    N, nx, nu, nc = p.sizes()
    assert np.array_equal(before[1]["guess"][0][:, :N * (nx + nu)], one["z_log"][0][:, nx + nu:])
    assert np.array_equal(before[1]["guess"][0][:, N * (nx + nu):], one["z_log"][0][:, N * (nx + nu):])


@pytest.mark.parametrize("pid,rows", [("P1", 11), ("P4", 12)])
def test_the_plant_adds_the_disturbance(hip, pid, rows):
    """x_log[k + 1] (and the final x0) against A x_log[k] + B u[k] + w[k] in numpy, per entry within
    (nx + nu + 2) 2^-52 (|A||x| + |B||u| + |w|): the bound for a sum of that many rounded terms."""
    (p, A, B, w, S), one, per, before = _stepwise(pid, rows)
    N, nx, nu, nc = p.sizes()
    for k in range(S):
        x, u = one["x_log"][k], one["u"][k]
        nxt = one["x_log"][k + 1] if k + 1 < S else one["x0"]
        ref = x @ A.T + u @ B.T + w[k]
        bound = (nx + nu + 2) * 2.0 ** -52 * (np.abs(x) @ np.abs(A).T + np.abs(u) @ np.abs(B).T + np.abs(w[k]))
        assert (np.abs(nxt - ref) <= bound).all(), (pid, k, np.abs(nxt - ref).max())
        assert np.abs(w[k]).max() > 100 * bound.max()   # (the disturbance is far above what the bound lets pass)


@pytest.mark.parametrize("pid", ["P1", "P4"])
def test_teacher_forced_parity_with_the_reference_loop(hip, oracle, oracle_fma, pid):
    """A step at a time with the shift on; at every step the oracle solves what the device is about to solve - the
    device's x0, the device's shifted previous point as the guess.  Every exit flag equal; proximal and Newton
    counts equal to the oracle's or to its fused-multiply-add build's, at most (T S) // 50 = 1 solve left out of
    the count comparison (the project's cap for warm-started loops); u_0 to 2e-5."""
    (p, A, B, w, S), one, per, before = _stepwise(pid, 12)
    N, nx, nu, nc = p.sizes()
    T = p.batch
    flips = 0
    for k in range(S):
        q = fx.MpcProblem(N, nx, nu, nc, dict(p.arrays))
        q.arrays["x0"] = np.ascontiguousarray(before[k]["x0"])
        zc, lc, vc, yc, oc = oracle.solve_mpc(q, before[k]["guess"], nthreads=oracle.num_threads())
        assert (oc["eflag"] == 0).all(), (pid, k, oc["eflag"])
        g = per["steps"][k]
        assert np.array_equal(g["eflag"], oc["eflag"]), (pid, k)
        same = (g["prox_iters"] == oc["prox_iters"]) & (g["newton_iters"] == oc["newton_iters"])
        if not same.all():
            of = oracle_fma.solve_mpc(q, before[k]["guess"], nthreads=oracle_fma.num_threads())[4]
            same = same | ((g["prox_iters"] == of["prox_iters"]) & (g["newton_iters"] == of["newton_iters"]))
        print(pid, "step", k, "newton", g["newton_iters"].tolist(), "oracle", oc["newton_iters"].tolist())
        flips += int((~same).sum())
        np.testing.assert_allclose(g["u"][0], zc[:, nx:nx + nu], rtol=0, atol=2e-5)
    assert flips <= (T * S) // 50, flips


# ---- G3 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pid", ["P1", "P4", "P5"])
def test_scenario_in_one_launch_equals_a_launch_per_step(hip, monkeypatch, pid):
    """w, shift = 1 and retirement on the one-row, the row-pair and the widest instance family (P1 with the
    infeasible trajectory): receding_plant_step against fbstab_receding_plant_kernel, bitwise."""
    p, A, B, w, S, kernel = _infeasible_p1() if pid == "P1" else SC.problem(pid)

    def run():
        s = _solver(hip, p, kernel)
        r = _sweep(hip, s, p, A, B, S, retire=True, w=w, shift=True)
        s.close()
        return r

    one = run()
    monkeypatch.setenv(PER_STEP_ENV, "1")
    per = run()
    monkeypatch.delenv(PER_STEP_ENV)
    if pid == "P1":
        assert one["stats"]["retired_total"][-1] == 1 and (one["eflag_log"][-1, 5] == -1)
        assert not one["x0"][5].any() and not one["z"][5].any()   # parked: w is not added
    assert (one["eflag_log"] <= 0).all(), one["eflag_log"]
    _same(one, per, pid)
    s = _solver(hip, p, kernel)
    plain = _sweep(hip, s, p, A, B, S, retire=True)
    s.close()
    assert not np.array_equal(plain["u"], one["u"]) and not np.array_equal(plain["x0"], one["x0"])


# ---- G6 ---------------------------------------------------------------------------------------------------------
def test_the_shift_pays_on_a_time_invariant_horizon_and_costs_on_a_random_one(hip):
    """The headline shape, 48 trajectories x 12 steps under position noise of sd 1e-2: the shifted sweep needs at
    most half the Newton steps of the unshifted one (the oracle's loop: 2184 against 8375, a ratio of 0.26; the
    factor of two left over covers count differences on the few QPs near infeasibility) and retires nobody (the
    oracle's retires none).  On P5, a random time-varying horizon, steps 2-4 cost MORE shifted (the oracle's loop
    on scenario_helpers.problem("P5"): 184 against 93): the sign is the problem's."""
    T, S = 48, 12
    p = fx.synthetic_mpc_batch(T, first_id=7000)
    A, B = fx.quadrotor_model()
    w = SC.position_noise(5, S, T, p.sizes()[1])
    s = _solver(hip, p, "fbstab_mpc_r16_kernel<12,4,20>")
    plain = _sweep(hip, s, p, A, B, S, w=w, shift=False)
    moved = _sweep(hip, s, p, A, B, S, w=w, shift=True)
    s.close()
    a, b = int(plain["stats"]["newton_sum"].sum()), int(moved["stats"]["newton_sum"].sum())
    print("newton steps unshifted", a, plain["stats"]["newton_sum"].tolist(), "shifted", b,
          moved["stats"]["newton_sum"].tolist())
    assert 2 * b <= a, (a, b)
    assert moved["stats"]["retired_total"][-1] == 0
    p, A, B, w, S, kernel = SC.problem("P5")
    s = _solver(hip, p, kernel)
    plain = _sweep(hip, s, p, A, B, S, w=w, shift=False)
    moved = _sweep(hip, s, p, A, B, S, w=w, shift=True)
    s.close()
    a, b = int(plain["stats"]["newton_sum"][1:].sum()), int(moved["stats"]["newton_sum"][1:].sum())
    print("P5 steps 2-4 unshifted", a, "shifted", b)
    assert b > a, (a, b)


# ---- G7 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [False, True], ids=["unshifted", "shifted"])
def test_autograd_gives_the_costate_to_w(hip, shift):
    """fd_problem() on the device at abs_tol = 1e-11, w = 1e-2 N(0, 1) from seed 77, L = <cu, u> + <cx, x>:
    ``w.grad`` is bitwise the ``mu`` of a direct RecedingSweepAdjoint on the same log with retired rows zeroed, it
    passes the sweep adjoint's central-difference rule along one random direction on the device's own closed loop
    (the trajectories strictly complementary at every step), and asking for it changes no other gradient."""
    import torch
    from fbstab_amd.autograd import closed_loop_mpc
    p, A, B, cu, cx, dirs = SH.fd_problem()
    N, nx, nu, nc = p.sizes()
    S = SH.FD_STEPS
    rng = np.random.default_rng(77)
    w = 1e-2 * rng.standard_normal((S, p.batch, nx))
    dw = rng.standard_normal(w.shape)
    s = hip.FBstabMpcBatch(*p.sizes(), max_batch=p.batch)
    s.UpdateOptions(H._opts(hip, default_options(abs_tol=1e-11)))
    want = ("q", "r", "d", "x0")
    grads = {}
    for noise in (True, False):
        data = {k: _dev(a).requires_grad_(k in want) for k, a in p.arrays.items()}
        wt = _dev(w).requires_grad_(noise)
        u, x, out = closed_loop_mpc(s, data, _dev(A), _dev(B), S, w=wt, shift=shift)
        ((_dev(cu) * u).sum() + (_dev(cx) * x).sum()).backward()
        grads[noise] = {k: data[k].grad.cpu().numpy() for k in want}
        if noise:
            gw, un, xn = wt.grad.cpu().numpy(), u.detach().cpu().numpy(), x.detach().cpu().numpy()
        else:
            assert wt.grad is None
    for k in want:
        assert np.abs(grads[True][k]).max() > 0 and np.array_equal(grads[True][k], grads[False][k]), k
    r = _sweep(hip, s, p, A, B, S, w=w, shift=shift)
    assert np.array_equal(r["u"], un) and np.array_equal(np.concatenate([r["x_log"][1:], r["x0"][None]], 0), xn)
    data = {k: _dev(a) for k, a in p.arrays.items()}
    g = s.RecedingSweepAdjoint(data, A, B, S, {k: _dev(r[k]) for k in ("z_log", "l_log", "v_log", "eflag_log")},
                               gu=_dev(cu), gx=_dev(cx), mu=True)
    mu = np.where((r["eflag_log"] == -1)[:, :, None], 0.0, g["mu"].cpu().numpy())
    assert np.abs(mu).max() > 0 and gw.tobytes() == mu.tobytes()
    good = SH.strictly_complementary(p, dict(z=r["z_log"], l=r["l_log"], v=r["v_log"], eflag=r["eflag_log"],
                                             x=r["x_log"]))
    assert len(good) >= 3, good

    def loss(wk):
        rr = _sweep(hip, s, p, A, B, S, w=wk, shift=shift)
        xs = np.concatenate([rr["x_log"][1:], rr["x0"][None]], 0)
        return (cu * rr["u"]).sum(axis=(0, 2)) + (cx * xs).sum(axis=(0, 2))

    fd = (loss(w + SH.FD_H * dw) - loss(w - SH.FD_H * dw)) / (2 * SH.FD_H)
    s.close()
    figures = []
    for q in good:
        ad = float((gw[:, q] * dw[:, q]).sum())
        figures.append((q, fd[q], ad, 1e-4 * max(abs(ad), 1e-2 * np.abs(gw[:, q]).sum())))
    for q, f, ad, bound in figures:
        print(f"w   q {q} shift {int(shift)} fd {f:+.9e} ad {ad:+.9e} |fd-ad| {abs(f - ad):.2e} bound {bound:.2e}")
    for q, f, ad, bound in figures:
        assert abs(f - ad) <= bound, (q, f, ad, bound)
