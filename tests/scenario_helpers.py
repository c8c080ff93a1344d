"""Shared helpers of the scenario-sweep tests (fbstab_hip_mpc_receding_sweep_scenario): the disturbances and the
problems of tests/test_gpu_sweep_scenario.py (the loop itself: tests/closed_loop.logged_closed_loop)."""
import numpy as np

from tools import fixtures as fx


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
