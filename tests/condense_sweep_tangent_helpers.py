"""TEST INFRASTRUCTURE ONLY: what tests/test_condense_sweep_tangent_cpu.py and
tests/test_gpu_condense_sweep_tangent.py share - the host build of fbstab_amd/csrc/fb_condense_sweep_tangent.h
(tests/hostsim/condense_sweep_tangent.cc), the step function's numpy reference with its rounding rules, and the
forward recursion through a logged sweep of the condensed route in numpy with a pluggable per-step solve.

The recursion (include/fbstab_hip.h): dx = dx0 and for k = 0 .. T-1: eflag -1: du_k = 0, dx <- 0; eflag != 0: du_k = 0,
dx <- A_p dx + dw_k; otherwise one dense adjoint at the logged (U_k, v_k) with the seeds gU = -(df0_k + F dx),
gv_c = db0_k + G dx: a failed factorisation counts in ``status`` and is the plant alone, a good one gives
du_k = dU[0:nu], dx <- A_p dx + B_p du_k + dw_k."""
import ctypes as C

import numpy as np

from tests import condense_adjoint_helpers as cah
from tests import condense_helpers as ch
from tests import condense_sweep_adjoint_helpers as sah
from tests import condense_sweep_helpers as csh
from tests import hostsim
from tests import sweep_adjoint_helpers as mah
from tests import tangent_helpers as TH

LD = ch.LD
SIX = sah.SIX
U2 = sah.U2
ptr = sah.ptr


class HostSweepTangent:
    """condense_sweep_tangent_step of fb_condense_sweep_tangent.h with Ctx<1> (hostsim/condense_sweep_tangent.cc)."""

    def __init__(self):
        self.lib = C.CDLL(hostsim.build("libhostsim_condense_sweep_tangent.so", "condense_sweep_tangent.cc",
                                        ("fb_common.h", "fb_batch.h", "fb_condense_plan.h", "fb_condense.h",
                                         "fb_condense_sweep_tangent.h")))
        self.lib.hostsim_sweep_tangent_step.argtypes = [C.c_void_p] * 4
        self.lib.hostsim_sweep_tangent_step.restype = None

    def step(self, sizes, A, B, affine, close=None, open_=None, dx0=None, T=0, stage_m=False, status=None,
             outputs=True):
        """One launch on ``(batch, n)`` arrays.  ``A``/``B``: row-major per-trajectory plants.
        ``affine``: (M (rows, ne nx), f0, b0).
        ``close``: None, or dict(eflag, st1, st2, dU, dx[, dw]) of the closed step (``dx``: the carried direction).
        ``open_``: None, or dict(eflag, x[, df0, db0]) of the opened step.
        ``dx0``: read by a launch that does not close (None: NULL).  ``status`` (int32): updated IN PLACE where given.
        Returns dict(dx - the carried direction behind the launch -, status, du, dx_out - of the closed step -, f, b,
        gU, gv - of the opened step)."""
        N, nx, nu, nc = sizes
        nzc, nv = (N + 1) * nu, (N + 1) * nc
        src = close if close is not None else open_
        Bn = len(src["eflag"]) if src is not None else len(dx0)
        f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)
        i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
        keep = []
        hold = lambda a: (keep.append(a), a)[1]
        Ac, Bc = hold(f64(np.asarray(A).transpose(0, 2, 1))), hold(f64(np.asarray(B).transpose(0, 2, 1)))
        M, f0, b0 = (hold(f64(a)) for a in affine)
        sM = 0 if M.shape[0] == 1 else M.shape[1]
        dx = f64(close["dx"]).copy() if close is not None else np.full((Bn, nx), np.nan)
        res = dict(dx=dx)
        dU = ec = s1 = s2 = dw = None
        if close is not None:
            dU, ec, s1, s2 = hold(f64(close["dU"])), hold(i32(close["eflag"])), hold(i32(close["st1"])), hold(i32(close["st2"]))
            dw = hold(f64(close["dw"])) if close.get("dw") is not None else None
            if outputs:
                res["du"], res["dx_out"] = np.full((Bn, nu), np.nan), np.full((Bn, nx), np.nan)
        st = status if status is not None else np.full(Bn, 55, dtype=np.int32)
        eo = xl = df0 = db0 = None
        if open_ is not None:
            eo, xl = hold(i32(open_["eflag"])), hold(f64(open_["x"]))
            df0 = hold(f64(open_["df0"])) if open_.get("df0") is not None else None
            db0 = hold(f64(open_["db0"])) if open_.get("db0") is not None else None
            for k, n in (("f", nzc), ("b", nv), ("gU", nzc), ("gv", nv)):
                res[k] = np.full((Bn, n), np.nan)
        x0 = hold(f64(dx0)) if dx0 is not None else None
        dp = (C.c_void_p * 18)(ptr(dU), ptr(dx), ptr(x0), ptr(Ac), ptr(Bc), ptr(dw), ptr(res.get("du")),
                               ptr(res.get("dx_out")), ptr(xl), ptr(M), ptr(f0), ptr(b0), ptr(res.get("f")),
                               ptr(res.get("b")), ptr(df0), ptr(db0), ptr(res.get("gU")), ptr(res.get("gv")))
        ip = (C.c_int * 9)(N, nx, nu, nc, Bn, int(close is not None), int(open_ is not None), T, int(stage_m))
        sp = (C.c_longlong * 10)(nx, nx * nx, nx * nu, sM, nzc, nv, nzc, nv, nzc, nv)
        npp = (C.c_void_p * 5)(ptr(ec), ptr(eo), ptr(s1), ptr(s2), ptr(st))
        self.lib.hostsim_sweep_tangent_step(ip, sp, dp, npp)
        res["status"] = st
        return res


# ---- the step function in numpy -----------------------------------------------------------------------------------
case_of = sah.case_of


def dx_reference(A, B, dx, dU, dw, cs):
    """(dx+ in longdouble, S = the sum of the magnitudes of its terms) of one trajectory: A, B row-major."""
    nu = np.asarray(B).shape[1]
    Al, Bl, d, u = (np.asarray(a, dtype=LD) for a in (A, B, dx, np.asarray(dU)[:nu]))
    if cs == 0:
        return np.zeros(Al.shape[0], dtype=LD), np.zeros(Al.shape[0], dtype=LD)
    out, S = Al @ d, np.abs(Al) @ np.abs(d)
    if cs == 2:
        out, S = out + Bl @ u, S + np.abs(Bl) @ np.abs(u)
    if dw is not None:
        out, S = out + np.asarray(dw, dtype=LD), S + np.abs(np.asarray(dw, dtype=LD))
    return out, S


def dx_bound(nx, nu, S):
    """The adjoint helpers' lambda rule on the nx + nu terms of the plant's chain: (nx + nu + 3) 2^-53 S."""
    return sah.lambda_bound(nu, nx, S)


def seeds_reference(F, G, dx, df0, db0, good):
    """((gU, gv_c) in longdouble, (S_U, S_v)) of one trajectory: F (nzc, nx), G (nv, nx); zero where not ``good``."""
    Fl, Gl, d = (np.asarray(a, dtype=LD) for a in (F, G, dx))
    f = np.zeros(Fl.shape[0], dtype=LD) if df0 is None else np.asarray(df0, dtype=LD)
    b = np.zeros(Gl.shape[0], dtype=LD) if db0 is None else np.asarray(db0, dtype=LD)
    if not good:
        return (np.zeros_like(f), np.zeros_like(b)), (np.zeros_like(f), np.zeros_like(b))
    return (-(f + Fl @ d), b + Gl @ d), (np.abs(f) + np.abs(Fl) @ np.abs(d), np.abs(b) + np.abs(Gl) @ np.abs(d))


def seed_bound(nx, S):
    """The adjoint helpers' seed rule on a chain of nx products and the base: (nx + 2) 2^-53 S."""
    return sah.seed_bound(nx, S)


# ---- the recursion in numpy -----------------------------------------------------------------------------------------
def reference_condensed_sweep_tangent(step_fn, p, A, B, maps, log, dx0=None, dw=None, df0=None, db0=None):
    """``step_fn(k, q, xk, U, v, gU, gv) -> (status, dU)``: the dense step of trajectory ``q`` at step k for the seeds
    (gU, gv_c).  ``maps``: per trajectory (F, G).  ``df0``/``db0``: None, ``(batch, n)`` (one direction for all steps)
    or ``(steps, batch, n)``.  Everything is carried in longdouble.  Returns (du, dx, status)."""
    N, nx, nu, nc = p.sizes()
    T, Bn = log["eflag"].shape
    du, dxs = np.zeros((T, Bn, nu), dtype=LD), np.zeros((T, Bn, nx), dtype=LD)
    status = np.zeros(Bn, dtype=np.int32)
    at = lambda a, k, q: None if a is None else (a[k][q] if np.ndim(a) == 3 else a[q])
    for q in range(Bn):
        d = np.zeros(nx, dtype=LD) if dx0 is None else np.asarray(dx0[q], dtype=LD)
        Aq, Bq = np.asarray(A[q], dtype=LD), np.asarray(B[q], dtype=LD)
        F, G = maps[q]
        for k in range(T):
            e = log["eflag"][k][q]
            if e == -1:
                d = np.zeros(nx, dtype=LD)
                dxs[k, q] = d
                continue
            nxt = Aq @ d + (LD(0) if dw is None else np.asarray(dw[k][q], dtype=LD))
            if e == 0:
                (gU, gv), _ = seeds_reference(F, G, d, at(df0, k, q), at(db0, k, q), True)
                st, dU = step_fn(k, q, log["x"][k][q], log["U"][k][q], log["v"][k][q], gU, gv)
                if st != 0:
                    status[q] += 1
                else:
                    du[k, q] = np.asarray(dU, dtype=LD)[:nu]
                    nxt = nxt + Bq @ du[k, q]
            d = nxt
            dxs[k, q] = d
    return du, dxs, status


def recursion_error_bound(op, p, A, B, maps, log, du, dx, dx0, dw, df0, db0):
    """Entry by entry, how far a float64 evaluation of the recursion that meets the step rules may lie from the
    longdouble recursion (du, dx) when both apply the same operator ``op`` (a DenseOperator): to first order the
    error e of the carried direction obeys
        e_seed = |M| e + seed_bound(S_seed)           the seeds are M dx + base, each within its rule
        e_du   = |W[0:nu]| e_seed + 2^-53 |du|        the dense step is linear; dU is rounded to double once
        e+     = |A_p| e + |B_p| e_du + dx_bound(S)   the plant's chain within its rule
    with the magnitudes S taken at the reference; a retired step resets e to zero, a step without a solution drops
    the middle line.  Returns (bound on du, bound on dx), TWICE the first-order figure: the spare covers the
    second-order terms and the magnitudes being the reference's, not the evaluation's."""
    N, nx, nu, nc = p.sizes()
    T, Bn = log["eflag"].shape
    bdu, bdx = np.zeros((T, Bn, nu), dtype=LD), np.zeros((T, Bn, nx), dtype=LD)
    at = lambda a, k, q: None if a is None else (a[k][q] if np.ndim(a) == 3 else a[q])
    for q in range(Bn):
        e = np.zeros(nx, dtype=LD)
        d = np.zeros(nx, dtype=LD) if dx0 is None else np.asarray(dx0[q], dtype=LD)
        Aq, Bq = np.abs(np.asarray(A[q], dtype=LD)), np.abs(np.asarray(B[q], dtype=LD))
        F, G = (np.asarray(a, dtype=LD) for a in maps[q])
        for k in range(T):
            flag = log["eflag"][k][q]
            if flag == -1:
                e, d = np.zeros(nx, dtype=LD), np.zeros(nx, dtype=LD)
                continue
            S = Aq @ np.abs(d) + (0 if dw is None else np.abs(np.asarray(dw[k][q], dtype=LD)))
            nxt = Aq @ e
            if flag == 0:
                _, (SU, Sv) = seeds_reference(F, G, d, at(df0, k, q), at(db0, k, q), True)
                es = np.concatenate([np.abs(F) @ e + seed_bound(nx, SU), np.abs(G) @ e + seed_bound(nx, Sv)])
                W = op.at(k, q, log["x"][k][q], log["U"][k][q], log["v"][k][q])
                bdu[k, q] = np.abs(W[:nu]) @ es + U2 * np.abs(du[k, q])
                nxt = nxt + Bq @ bdu[k, q]
                S = S + Bq @ np.abs(du[k, q])
            e = nxt + dx_bound(nx, nu, S)
            bdx[k, q] = e
            d = np.asarray(dx[k, q], dtype=LD)
    return 2 * bdu, 2 * bdx


class DenseOperator:
    """The dense step of both recursions as ONE matrix per (step, trajectory): W = V_c^-1 diag(I, -C) in longdouble
    at the expanded logged point, so that (dU, dv) = W (gU, gv_c).  The forward recursion applies W, the backward one
    its transpose - V_c = [H_c + sigma I, A_c'; -C A_c, mus] gives W11 = W11' and W21 = W12' in exact arithmetic, so
    W'(gU, 0) IS the adjoint's step, and with the transpose taken literally the two recursions are dual to the
    rounding of their matrix-vector products whatever the accuracy of the inverse."""

    def __init__(self, p, sigma=cah.SIGMA):
        self.p, self.sigma, self.W = p, sigma, {}

    def at(self, k, q, xk, U, v):
        if (k, q) not in self.W:
            m, x = sah.expanded_point(self.p, q, xk, U, v)
            img = ch.condense_reference(m, 0)
            V, Cg = cah.dense_system(m, 0, x, img["H"], img["A"], self.sigma)
            nzc = img["H"].shape[0]
            R = np.eye(V.shape[0], dtype=LD)
            R[nzc:, nzc:] = np.diag(-Cg)
            self.W[(k, q)] = cah.solve_refined(V, R)
        return self.W[(k, q)]

    def forward(self):
        def fn(k, q, xk, U, v, gU, gv):
            W = self.at(k, q, xk, U, v)
            return 0, (W @ np.concatenate([gU, gv]))[:len(gU)]
        return fn

    def backward(self):
        def fn(k, q, xk, U, v, gU):
            W = self.at(k, q, xk, U, v)
            s = W.T @ np.concatenate([gU, np.zeros(W.shape[0] - len(gU), dtype=LD)])
            return 0, s[:len(gU)], s[len(gU):], None
        return fn


def mpc_form_recursion(step_fn, p, A, B, log, dx0=None, dw=None):
    """The forward recursion with the per-step solve in the MPC form: ``step_fn(k, q, xk, U, v, dx) -> (status,
    du_k)`` sees the direction of the state itself (and knows the step's directions of q, r, c, d).  Carried in
    longdouble.  Returns (du, dx, status)."""
    N, nx, nu, nc = p.sizes()
    T, Bn = log["eflag"].shape
    du, dxs = np.zeros((T, Bn, nu), dtype=LD), np.zeros((T, Bn, nx), dtype=LD)
    status = np.zeros(Bn, dtype=np.int32)
    for q in range(Bn):
        d = np.zeros(nx, dtype=LD) if dx0 is None else np.asarray(dx0[q], dtype=LD)
        Aq, Bq = np.asarray(A[q], dtype=LD), np.asarray(B[q], dtype=LD)
        for k in range(T):
            e = log["eflag"][k][q]
            if e == -1:
                d = np.zeros(nx, dtype=LD)
                dxs[k, q] = d
                continue
            nxt = Aq @ d + (LD(0) if dw is None else np.asarray(dw[k][q], dtype=LD))
            if e == 0:
                st, duk = step_fn(k, q, log["x"][k][q], log["U"][k][q], log["v"][k][q], d)
                if st != 0:
                    status[q] += 1
                else:
                    du[k, q] = np.asarray(duk, dtype=LD)[:nu]
                    nxt = nxt + Bq @ du[k, q]
            d = nxt
            dxs[k, q] = d
    return du, dxs, status


def chain_mpc_step(p, directions, sigma=cah.SIGMA):
    """``mpc_form_recursion``'s step from cah.chain_reference in longdouble: the directions of step k
    (``directions(k, q) -> name -> flat array`` for q, r, c, d) and x0 := dx through tangent_helpers.tangent_rhs."""
    nu = p.nu

    def fn(k, q, xk, U, v, dx):
        m, x = sah.expanded_point(p, q, xk, U, v)
        d = dict(directions(k, q))
        d["x0"] = np.asarray(dx, dtype=np.float64)
        (gz, gl, gv), _ = TH.tangent_rhs(m, 0, x, d)
        c = cah.chain_reference(m, 0, x, (gz.astype(np.float64), gl.astype(np.float64), gv.astype(np.float64)), sigma)
        return 0, c["dU"][:nu]
    return fn


def rel_gap(got, ref):
    """max|got - ref| / max|ref| (1 where the reference is zero)."""
    top = float(np.abs(ref).max()) if np.size(ref) else 0.0
    return float(np.abs(np.asarray(got, dtype=LD) - ref).max()) / (top if top > 0 else 1.0) if np.size(ref) else 0.0


def duality_sides(gu, gx, du, dx, lam0, mu, eflag, dx0=None, dw=None, gf0=None, gb0=None, df0=None, db0=None,
                  extra=()):
    """Both sides of sum_k <gu_k, du_k> + <gx_k, dx_(k+1)> = <lambda_0, dx0> + sum_k <mu_k, dw_k> [not retired] +
    <gf0, df0> + <gb0, db0> (+ ``extra``: pairs (gradient, direction) of per-step sequences) per trajectory in
    longdouble, and the sum of the magnitudes of all their products.  Returns (lhs, rhs, S), ``(batch,)`` each."""
    f = lambda a: np.asarray(a, dtype=LD)
    Bn = f(du).shape[1]
    lhs, rhs, S = np.zeros(Bn, dtype=LD), np.zeros(Bn, dtype=LD), np.zeros(Bn, dtype=LD)
    for g, d in ((gu, du), (gx, dx)):
        if g is not None:
            t = f(g) * f(d)
            lhs, S = lhs + t.sum(axis=(0, 2)), S + np.abs(t).sum(axis=(0, 2))
    if dx0 is not None:
        t = f(lam0) * f(dx0)
        rhs, S = rhs + t.sum(axis=1), S + np.abs(t).sum(axis=1)
    if dw is not None:
        t = np.where((np.asarray(eflag) == -1)[:, :, None], LD(0), f(mu) * f(dw))
        rhs, S = rhs + t.sum(axis=(0, 2)), S + np.abs(t).sum(axis=(0, 2))
    for g, d in ((gf0, df0), (gb0, db0)) + tuple(extra):
        if g is not None and d is not None:
            t = f(g) * f(d)
            ax = tuple(i for i in range(t.ndim) if i != t.ndim - 2)
            rhs, S = rhs + t.sum(axis=ax), S + np.abs(t).sum(axis=ax)
    return lhs, rhs, S


# ---- central differences -------------------------------------------------------------------------------------------
FD_STEPS, FD_H = mah.FD_STEPS, mah.FD_H    # (the adjoint's central-difference tests differentiate the same map)
FD_NAME, FD_SEED = "small", 81


def fd_setup():
    """The fixture, a random linear loss in (u, x) and one direction each of x0, w and q."""
    p, A, B, w = csh.setup(FD_NAME)
    rng = np.random.default_rng(FD_SEED)
    T = FD_STEPS
    cu, cx = rng.standard_normal((T, p.batch, p.nu)), rng.standard_normal((T, p.batch, p.nx))
    dirs = dict(x0=rng.standard_normal(p.arrays["x0"].shape), w=rng.standard_normal((T, p.batch, p.nx)),
                q=rng.standard_normal(p.arrays["q"].shape))
    return p, A, B, w[:T], cu, cx, dirs


def fd_runs(sweep, p, w, dirs):
    """The loop at +h and -h along each direction: name -> (log+, log-); ``sweep(arrays, w) -> log`` with ``x_end``."""
    runs = {}
    for name, d in dirs.items():
        pair = []
        for sg in (1.0, -1.0):
            arr = {k: a.copy() for k, a in p.arrays.items()}
            ww = w
            if name == "w":
                ww = w + sg * FD_H * d
            else:
                arr[name] = arr[name] + sg * FD_H * d
            pair.append(sweep(arr, ww))
        runs[name] = pair
    return runs


def fd_left_out(p, runs):
    """Trajectories whose exit flags or active sets (v > y row by row at the expanded logged points) differ between the
    two perturbed runs of any direction."""
    from tests import helpers as H
    from tools import fixtures as fx
    N, nx, nu, nc = p.sizes()
    out = set()

    def active(arr, lg, k, q):
        one = {n: a[q:q + 1] for n, a in arr.items()}
        one["x0"] = lg["x"][k][q:q + 1]
        m = fx.MpcProblem(N, nx, nu, nc, one)
        _, (z, l, v) = sah.expanded_point(m, 0, lg["x"][k][q], lg["U"][k][q], lg["v"][k][q])
        Am, bv = H.mpc_explicit(m, 0)[4:]
        return lg["v"][k][q] > bv - Am @ z
    for name, (lp, lm) in runs.items():
        for q in range(p.batch):
            if not np.array_equal(lp["eflag"][:, q], lm["eflag"][:, q]):
                out.add(q)
                continue
            for k in range(lp["eflag"].shape[0]):
                if lp["eflag"][k, q] == 0 and not np.array_equal(active(lp["arrays"], lp, k, q), active(lm["arrays"], lm, k, q)):
                    out.add(q)
    return sorted(out)


def oracle_sweep(p, A, B):
    from oracle.oracle_py import Oracle, default_options
    from tools import fixtures as fx
    orc, opts = Oracle(), default_options(abs_tol=1e-11)

    def sweep(arr, w):
        m = fx.MpcProblem(*p.sizes(), arr)
        rc = csh.ReferenceCondenser(m)

        def solve(x, U, v):
            z, _, vo, _, out = orc.solve_dense(rc.problem(x), x0guess=(U, np.zeros((m.batch, 0)), v), opts=opts,
                                               raise_on_error=False)
            return z, vo, out
        lg = csh.condensed_closed_loop(solve, m, A, B, FD_STEPS, w=w)
        lg["arrays"] = arr
        return lg
    return sweep
