"""Shared helpers of the scenario-sweep tests (fbstab_hip_mpc_receding_sweep_scenario): the closed loop with a
disturbed plant and a shifted warm start in numpy, around any batched ``solve`` (the oracle, or the device a step
at a time), and the problems of tests/test_gpu_sweep_scenario.py.

The loop (include/fbstab_hip.h): step k solves for x_k from the previous point, retirement parks a trajectory at
the origin with a zero point, the returned point is logged, x_(k+1) = A x_k + B u_k + w_k (not for a parked
trajectory), and with ``shift`` the point is moved one stage towards the present - z_i <- z_(i+1), l_i <- l_(i+1),
v_i <- v_(i+1) for i < N, stage N keeping its values - before it is the next guess, except behind the last step."""
import numpy as np

from tools import fixtures as fx


def shift_point(z, l, v, sizes):
    """(z, l, v) ``(batch, n)`` moved one stage towards the present, in place (numpy arrays or torch tensors: slice
    copies from a clone of the source, so that no copy reads what it has written)."""
    N, nx, nu, nc = sizes
    for a, b in ((z, nx + nu), (l, nx), (v, nc)):
        src = a[:, b:].clone() if hasattr(a, "clone") else a[:, b:].copy()
        a[:, :N * b] = src
    return z, l, v


def closed_loop(solve, p, A, B, steps, w=None, shift=False, retire=True, guess=None):
    """``solve(x0, z, l, v) -> (z, l, v, y, out)`` on ``(batch, n)`` numpy arrays, ``out`` a record array with
    eflag, newton_iters, prox_iters.  ``p``: the fixtures.MpcProblem whose x0 starts the loop; ``A``/``B`` row-major;
    ``w`` ``(steps, batch, nx)`` or None.  Returns the log of tests/sweep_adjoint_helpers.oracle_closed_loop -
    ``z, l, v`` (returned points, unshifted; zeros once retired), ``eflag`` (-1 once retired), ``x`` (the states the
    steps were solved for), ``u``, ``x_end`` - plus ``newton`` and ``prox`` ``(steps, batch)``, ``raw_eflag`` and
    ``point``: the (z, l, v) left behind the last step (unshifted)."""
    sizes = p.sizes()
    N, nx, nu, nc = sizes
    Bn = p.batch
    x0 = p.arrays["x0"].copy()
    z, l, v = ((np.zeros((Bn, p.nz)), np.zeros((Bn, p.nl)), np.zeros((Bn, p.nv))) if guess is None
               else tuple(a.copy() for a in guess))
    gone = np.zeros(Bn, dtype=bool)
    log = dict(z=[], l=[], v=[], eflag=[], x=[], u=[], newton=[], prox=[], raw_eflag=[])
    for k in range(steps):
        z, l, v, y, out = solve(x0, z, l, v)
        z, l, v = z.copy(), l.copy(), v.copy()
        if retire:
            gone = gone | (out["eflag"] != 0)
        z[gone] = 0.0; l[gone] = 0.0; v[gone] = 0.0
        u = z[:, nx:nx + nu].copy()
        log["z"].append(z.copy()); log["l"].append(l.copy()); log["v"].append(v.copy())
        log["eflag"].append(np.where(gone, -1, out["eflag"]).astype(np.int32))
        log["raw_eflag"].append(np.asarray(out["eflag"]).astype(np.int32))
        log["newton"].append(np.asarray(out["newton_iters"]).astype(np.int64))
        log["prox"].append(np.asarray(out["prox_iters"]).astype(np.int64))
        log["x"].append(x0.copy()); log["u"].append(u)
        x0 = x0 @ A.T + u @ B.T
        if w is not None:
            x0 = x0 + w[k]
        x0[gone] = 0.0
        if shift and k + 1 < steps:
            shift_point(z, l, v, sizes)
    res = {k: np.stack(a) for k, a in log.items()}
    res["x_end"] = x0
    res["point"] = (z, l, v)
    return res


def oracle_solve(oracle, p, opts=None):
    """``solve`` of ``closed_loop`` with the oracle on ``p``'s data."""
    N, nx, nu, nc = p.sizes()

    def solve(x0, z, l, v):
        arr = dict(p.arrays)
        arr["x0"] = np.ascontiguousarray(x0)
        return oracle.solve_mpc(fx.MpcProblem(N, nx, nu, nc, arr), x0guess=(z, l, v), opts=opts,
                                nthreads=oracle.num_threads())
    return solve


def position_noise(seed, steps, batch, nx, sd=1e-2):
    """w[:, :, 0:3] = sd N(0, 1), the other states undisturbed."""
    w = np.zeros((steps, batch, nx))
    w[:, :, 0:3] = sd * np.random.default_rng(seed).standard_normal((steps, batch, 3))
    return w


def _generator_problem(name, N, T, S):
    gen = fx.OcpGenerator()
    getattr(gen, name)(N)
    one = gen.GetFBstabInput()
    sim = gen.GetSimulationInputs()
    A, B = np.asarray(sim["A"], dtype=np.float64), np.asarray(sim["B"], dtype=np.float64)
    Nn, nx, nu, nc = one.sizes()
    p = fx.MpcProblem(Nn, nx, nu, nc)
    p.arrays = {k: np.repeat(a, T, axis=0) for k, a in one.arrays.items()}
    p.arrays["x0"] = np.ascontiguousarray(p.arrays["x0"] * (1.0 + 0.02 * np.arange(T)[:, None]))
    # (per state: the largest initial value of that state over the batch sets the scale of its disturbance)
    w = 1e-2 * np.abs(p.arrays["x0"]).max(axis=0) * np.random.default_rng(5).standard_normal((S, T, nx))
    return p, A, B, w


def _ltv_problem(N, nx, nu, nc, T=6, S=4):
    rng = np.random.default_rng(5)
    p = fx.random_ltv_mpc(rng, T, N, nx, nu, nc)
    A = np.eye(nx)
    B = 0.02 * rng.standard_normal((nx, nu))
    w = 1e-2 * rng.standard_normal((S, T, nx))
    return p, A, B, w


def problem(pid):
    """The problems P1 .. P6 of the GPU tests: ``(p, A, B, w, steps, kernel name)``."""
    if pid in ("P1", "P2"):
        T, S = 12, 5
        make = fx.synthetic_mpc_batch if pid == "P1" else fx.boxed_mpc_batch
        p = make(T, first_id=7000, N=6)
        A, B = fx.quadrotor_model()
        w = position_noise(5, S, T, p.sizes()[1])
        return p, A, B, w, S, "fbstab_mpc_r16_kernel<12,4,20>" if pid == "P1" else "fbstab_mpc_r16_kernel<12,4,32>"
    if pid == "P3":
        return _generator_problem("SpacecraftRelativeMotion", 12, 12, 5) + (5, "fbstab_mpc_r16_kernel<12,4,20>")
    if pid == "P4":
        return _generator_problem("CopolymerizationReactor", 16, 12, 5) + (5, "fbstab_mpc_r32_kernel<18,5,10>")
    if pid == "P5":
        return _ltv_problem(4, 20, 6, 16) + (4, "fbstab_mpc_r32_kernel<24,8,16>")
    if pid == "P6":
        return _ltv_problem(4, 24, 8, 32) + (4, "fbstab_mpc_r32_kernel<24,8,32>")
    raise KeyError(pid)


def take(p, rows):
    """The trajectories ``rows`` of ``p`` as a problem of their own."""
    N, nx, nu, nc = p.sizes()
    q = fx.MpcProblem(N, nx, nu, nc)
    q.arrays = {k: np.ascontiguousarray(a[rows]) for k, a in p.arrays.items()}
    return q
