"""TEST INFRASTRUCTURE ONLY: what tests/test_condense_sweep_cpu.py and tests/test_gpu_condense_sweep.py share - the
closed-loop set-ups, the reference loop through the condensed QP (the oracle's dense solver on the extended-precision
condensing of tests/condense_helpers.py), the acceptance rule for the affine map of x0 and the host build of
fbstab_amd/csrc/fb_condense_sweep.h (tests/hostsim/condense_sweep.cc)."""
import ctypes as C
import functools

import numpy as np

from tests import condense_helpers as ch
from tests import hostsim
from tools import fixtures as fx

LD = ch.LD
STEPS = 12
LOOP_FIXTURES = ("double_integrator", "small", "tiny", "four_wave")
# which trajectory retires at which step (unshifted and shifted alike), by the oracle: the table of the tests
RETIRES = {"double_integrator": {2: 0}, "small": {2: 3, 4: 4}, "tiny": {1: 4}, "four_wave": {}}


def with_x0(p, x0):
    """``p`` with the initial states ``x0`` ``(batch, nx)``; the other arrays are shared, not copied."""
    m = fx.MpcProblem(*p.sizes())
    m.arrays = dict(p.arrays)
    m.arrays["x0"] = np.ascontiguousarray(x0, dtype=np.float64)
    return m


# ---- the closed-loop set-ups ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def setup(name):
    """(problem, A, B, w): the fixture of tests/condense_helpers.py, its plant - row-major ``(batch, nx, nx)`` /
    ``(batch, nx, nu)``: each QP's own stage-0 matrices, or for double_integrator the generator's simulation model
    - and the disturbances ``(STEPS, batch, nx)``.  double_integrator: rows 4 and 5 of d of every stage of trajectory
    2 are +1, so that u >= 1 and u <= -1 contradict."""
    p = ch.problem(name)
    N, nx, nu, nc = p.sizes()
    if name == "double_integrator":
        g = fx.OcpGenerator()
        g.DoubleIntegrator()
        sim = g.GetSimulationInputs()
        A = np.repeat(np.asarray(sim["A"], dtype=np.float64).reshape(1, nx, nx), p.batch, axis=0)
        B = np.repeat(np.asarray(sim["B"], dtype=np.float64).reshape(1, nx, nu), p.batch, axis=0)
        m = fx.MpcProblem(N, nx, nu, nc)
        m.arrays = {k: a.copy() for k, a in p.arrays.items()}
        d = m.arrays["d"].reshape(p.batch, N + 1, nc)
        d[2, :, 4:6] = 1.0
        p = m
    else:
        A = np.ascontiguousarray(p.arrays["A"][:, :nx * nx].reshape(p.batch, nx, nx).transpose(0, 2, 1))
        B = np.ascontiguousarray(p.arrays["B"][:, :nx * nu].reshape(p.batch, nu, nx).transpose(0, 2, 1))
    w = 0.01 * np.random.default_rng(5).standard_normal((STEPS, p.batch, nx))
    return p, A, B, w


def plant_step(A, B, x, u, w=None):
    """x+ = A x + B u (+ w) per trajectory in float64."""
    xn = np.einsum("qrc,qc->qr", A, x) + np.einsum("qrj,qj->qr", B, u)
    return xn if w is None else xn + w


def plant_reference(A, B, x, u, w=None):
    """(x+ in longdouble, S = the sum of the magnitudes of its terms), per trajectory."""
    Al, Bl, xl, ul = (np.asarray(a, dtype=LD) for a in (A, B, x, u))
    xn = np.einsum("qrc,qc->qr", Al, xl) + np.einsum("qrj,qj->qr", Bl, ul)
    S = np.einsum("qrc,qc->qr", np.abs(Al), np.abs(xl)) + np.einsum("qrj,qj->qr", np.abs(Bl), np.abs(ul))
    if w is not None:
        xn = xn + np.asarray(w, dtype=LD)
        S = S + np.abs(np.asarray(w, dtype=LD))
    return xn, S


def plant_bound(nx, nu, S):
    """(nx + nu + 3) 2^-53 S: one rounding per term of the chain, the disturbance's addition and a spare."""
    return LD(nx + nu + 3) * LD(2.0) ** -53 * S


def shift_condensed(U, v, sizes):
    """(U, v) ``(batch, n)`` moved one stage towards the present, in place; stage N keeps its values."""
    N, nx, nu, nc = sizes
    U[:, :N * nu] = U[:, nu:].copy()
    v[:, :N * nc] = v[:, nc:].copy()


def condensed_closed_loop(solve, p, A, B, steps, w=None, shift=False, retire=True):
    """tests/closed_loop.logged_closed_loop on the condensed point: ``solve(x, U, v) -> (U, v, out)`` on
    ``(batch, n)`` numpy arrays.  Returns the log: ``u, x, U, v`` (returned points, unshifted; zeros once retired),
    ``eflag`` (-1 once retired), ``newton``, and ``x_end``."""
    sizes = p.sizes()
    N, nx, nu, nc = sizes
    x = p.arrays["x0"].copy()
    U, v = np.zeros((p.batch, (N + 1) * nu)), np.zeros((p.batch, p.nv))
    gone = np.zeros(p.batch, dtype=bool)
    log = dict(u=[], x=[], U=[], v=[], eflag=[], newton=[])
    for k in range(steps):
        U, v, out = solve(x, U, v)
        U, v = U.copy(), v.copy()
        if retire:
            gone = gone | (out["eflag"] != 0)
        U[gone] = 0.0; v[gone] = 0.0
        log["u"].append(U[:, :nu].copy()); log["x"].append(x.copy())
        log["U"].append(U.copy()); log["v"].append(v.copy())
        log["eflag"].append(np.where(gone, -1, out["eflag"]).astype(np.int32))
        log["newton"].append(np.asarray(out["newton_iters"]).astype(np.int32))
        x = plant_step(A, B, x, U[:, :nu], None if w is None else w[k])
        x[gone] = 0.0
        if shift and k + 1 < steps:
            shift_condensed(U, v, sizes)
    res = {k: np.stack(a) for k, a in log.items()}
    res["x_end"] = x
    return res


# ---- the reference's condensed QP as a function of x0 -------------------------------------------------------------
class ReferenceCondenser:
    """ch.condense_reference for many initial states of one problem: H_c and A_c (which x0 does not enter) are
    formed once per QP, f_c and b_c by the same longdouble formulas per state."""

    def __init__(self, p):
        self.p = p
        self.parts = []
        for q in range(p.batch):
            H, f, G, h, A, b = ch._explicit(p, q, False)
            T, _ = ch._rollout(p, G, h, False)
            r = ch.condense_reference(p, q)
            self.parts.append((H, f, G, h, A, b, T, r["H"].astype(np.float64).T.reshape(-1),
                               r["A"].astype(np.float64).T.reshape(-1)))

    def vectors(self, q, x):
        """(f_c, b_c) of QP ``q`` at the initial state ``x`` in longdouble."""
        H, f, G, h, A, b, T, _, _ = self.parts[q]
        h = h.copy()
        h[:self.p.nx] = -np.asarray(x, dtype=LD)      # (mpc_explicit: the rows of stage 0 read -x_0 = -x0)
        _, t = ch._rollout(self.p, G, h, False)
        return T.T @ (H @ t + f), b - A @ t

    def problem(self, X):
        """The dense problem of every QP at the states ``X`` ``(batch, nx)``, rounded to double."""
        fb = [self.vectors(q, X[q]) for q in range(self.p.batch)]
        return ch.condensed_problem(self.p, dict(
            H=np.stack([s[7] for s in self.parts]), A=np.stack([s[8] for s in self.parts]),
            f=np.stack([f.astype(np.float64) for f, _ in fb]), b=np.stack([b.astype(np.float64) for _, b in fb])))

    def affine(self):
        """The reference's own affine map in float64: (f0, F, b0, G) per QP from condensing x0 = 0 and the unit
        states."""
        nx = self.p.nx
        res = []
        for q in range(self.p.batch):
            f0, b0 = (a.astype(np.float64) for a in self.vectors(q, np.zeros(nx)))
            cols = [tuple(a.astype(np.float64) for a in self.vectors(q, e)) for e in np.eye(nx)]
            res.append((f0, np.stack([f - f0 for f, _ in cols], axis=1), b0,
                        np.stack([b - b0 for _, b in cols], axis=1)))
        return res


@functools.lru_cache(maxsize=None)
def condenser(name):
    return ReferenceCondenser(setup(name)[0])


@functools.lru_cache(maxsize=None)
def oracle_loop(name, shift=False, variant="plain", retire=True):
    """The reference closed loop of ``setup(name)``: ``variant`` "plain" (Oracle()), "fma" (Oracle(fma=True)) or
    "affine" (Oracle() with f_c, b_c from the reference's float64 affine map)."""
    from oracle.oracle_py import Oracle
    p, A, B, w = setup(name)
    rc = condenser(name)
    orc = Oracle(fma=(variant == "fma"))
    aff = rc.affine() if variant == "affine" else None

    def solve(x, U, v):
        d = rc.problem(x)
        if aff is not None:
            d.arrays["f"] = np.stack([f0 + F @ x[q] for q, (f0, F, _, _) in enumerate(aff)])
            d.arrays["b"] = np.stack([b0 + G @ x[q] for q, (_, _, b0, G) in enumerate(aff)])
        z, _, vo, _, out = orc.solve_dense(d, x0guess=(U, np.zeros((p.batch, 0)), v), raise_on_error=False)
        return z, vo, out
    return condensed_closed_loop(solve, p, A, B, STEPS, w=w, shift=shift, retire=retire)


def gap(u, ur):
    """max|u - u'| / (1 + max|u|)."""
    return float(np.abs(np.asarray(u) - np.asarray(ur)).max() / (1.0 + np.abs(np.asarray(ur)).max()))


def retirement(eflag_log):
    """{trajectory: first step with a logged -1}."""
    e = np.asarray(eflag_log)
    return {int(q): int(np.argmax(e[:, q] == -1)) for q in range(e.shape[1]) if (e[:, q] == -1).any()}


# ---- the rule for the affine map ---------------------------------------------------------------------------------
def map_parts(p, M):
    """(F, G) as 2-D arrays from the flat column-major image [F; G]."""
    nzc, nv = (p.N + 1) * p.nu, p.nv
    W = np.asarray(M).reshape(p.nx, nzc + nv).T
    return W[:nzc], W[nzc:]


def affine_ratio(p, q, F, G, f0, b0, x):
    """The worst |base + M x - reference| / bound over f_c and b_c at the state ``x``: the reference and
    ch.condense_bound (factor 1) of the problem with x0 := x; base + M x formed in longdouble, so that the figure is
    the map's error and not that of forming the product."""
    X0 = p.arrays["x0"].copy()
    X0[q] = x
    m = with_x0(p, X0)
    ref, bound = ch.condense_reference(m, q), ch.condense_bound(m, q)
    xl = np.asarray(x, dtype=LD)
    got = dict(f=(np.asarray(f0, dtype=LD) + np.asarray(F, dtype=LD) @ xl),
               b=(np.asarray(b0, dtype=LD) + np.asarray(G, dtype=LD) @ xl))
    w = 0.0
    for k in ("f", "b"):
        err = np.abs(got[k] - ref[k])
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(bound[k] > 0, err / np.where(bound[k] > 0, bound[k], 1), np.where(err > 0, np.inf, 0))
        w = max(w, float(r.max()))
    return w


def test_states(p, q):
    """The states the rule is applied at: the fixture's own and two random ones."""
    rng = np.random.default_rng(100 + q)
    return [p.arrays["x0"][q].copy(), rng.standard_normal(p.nx), 3.0 * rng.standard_normal(p.nx)]


test_states.__test__ = False


# ---- the device logic on one host thread -----------------------------------------------------------------------
class HostSweep:
    """condense_x0_map / condense_sweep_step / condense_sweep_begin of fb_condense_sweep.h with Ctx<1>
    (hostsim/condense_sweep.cc)."""

    def __init__(self):
        self.lib = C.CDLL(hostsim.build("libhostsim_condense_sweep.so", "condense_sweep.cc",
                                        ("fb_common.h", "fb_batch.h", "fb_condense_plan.h", "fb_condense.h", "fb_condense_sweep.h")))
        self.lib.hostsim_x0_map.argtypes = [C.c_int] * 4 + [C.c_void_p] * 2
        self.lib.hostsim_sweep_sizes.argtypes = [C.c_int] * 6 + [C.c_void_p]
        self.lib.hostsim_sweep_step.argtypes = [C.c_void_p] * 8
        self.lib.hostsim_sweep_begin.argtypes = [C.c_int] * 4 + [C.c_void_p] * 5

    def x0_map(self, p, q):
        """The flat image [F; G] of QP ``q``."""
        M = np.full(((p.N + 1) * p.nu + p.nv) * p.nx, np.nan)
        keep, data = ch.HostCondense._data(p, q)
        self.lib.hostsim_x0_map(*p.sizes(), data, M.ctypes.data)
        return M

    def sizes(self, N, nx, nu, nc, T=0, stage_m=True):
        out = (C.c_longlong * 4)()
        self.lib.hostsim_sweep_sizes(N, nx, nu, nc, T, 1 if stage_m else 0, out)
        return dict(T=out[0], total=out[1], m_lds=out[2], ldm=out[3])

    def begin(self, sizes, z, v):
        N, nx, nu, nc = sizes
        U, vc, gone = np.full((N + 1) * nu, np.nan), np.full((N + 1) * nc, np.nan), np.full(1, 7, dtype=np.int32)
        self.lib.hostsim_sweep_begin(N, nx, nu, nc, z.ctypes.data, v.ctypes.data, U.ctypes.data, vc.ctypes.data,
                                     gone.ctypes.data)
        return U, vc, int(gone[0])

    def step(self, sizes, U, v, x, gone, eflag, newton, A, B, w=None, retire=True, shift=False, T=0, logs=True,
             affine=None, stage_m=False):
        """One step on ``(batch, n)`` arrays, IN PLACE on ``U, v, x, gone`` (int32).  ``A``/``B``: row-major
        per-trajectory plants.  ``affine``: None, or (M (rows, ne nx), f0, b0): ``f`` and ``b`` are returned.
        Returns a dict of the logs and ``xkeep``."""
        N, nx, nu, nc = sizes
        Bn = x.shape[0]
        nzc, nv = (N + 1) * nu, (N + 1) * nc
        Ac = np.ascontiguousarray(np.asarray(A).transpose(0, 2, 1))   # column-major images
        Bc = np.ascontiguousarray(np.asarray(B).transpose(0, 2, 1))
        res = dict(xkeep=np.full((Bn, nx), np.nan))
        if logs:
            res.update(u=np.full((Bn, nu), np.nan), x=np.full((Bn, nx), np.nan), U=np.full((Bn, nzc), np.nan),
                       v=np.full((Bn, nv), np.nan), eflag=np.full(Bn, 99, dtype=np.int32),
                       newton=np.full(Bn, 99, dtype=np.int32))
        sM = sf0 = sb0 = 0
        if affine is not None:
            M, f0, b0 = (np.ascontiguousarray(a, dtype=np.float64) for a in affine)
            sM = 0 if M.shape[0] == 1 else M.shape[1]
            sf0, sb0 = nzc, nv
            res["f"], res["b"] = np.full((Bn, nzc), np.nan), np.full((Bn, nv), np.nan)
        ptr = lambda a: None if a is None else a.ctypes.data
        wk = None if w is None else np.ascontiguousarray(w, dtype=np.float64)
        dp = (C.c_void_p * 16)(ptr(U), ptr(v), ptr(x), ptr(res["xkeep"]), ptr(Ac), ptr(Bc), ptr(wk),
                               ptr(res.get("u")), ptr(res.get("x")), ptr(res.get("U")), ptr(res.get("v")),
                               ptr(M) if affine is not None else None, ptr(f0) if affine is not None else None,
                               ptr(b0) if affine is not None else None, ptr(res.get("f")), ptr(res.get("b")))
        ip = (C.c_int * 10)(N, nx, nu, nc, Bn, int(retire), int(shift), int(affine is not None), T, int(stage_m))
        sp = (C.c_longlong * 8)(nx, nx * nx, nx * nu, sM, sf0, sb0, nzc, nv)
        ef = np.ascontiguousarray(eflag, dtype=np.int32)
        nw = np.ascontiguousarray(newton, dtype=np.int32)
        self.lib.hostsim_sweep_step(ip, sp, dp, ef.ctypes.data, nw.ctypes.data, gone.ctypes.data,
                                    ptr(res.get("eflag")), ptr(res.get("newton")))
        return res
