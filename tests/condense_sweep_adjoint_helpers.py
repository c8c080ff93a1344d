"""TEST INFRASTRUCTURE ONLY: what tests/test_condense_sweep_adjoint_cpu.py and
tests/test_gpu_condense_sweep_adjoint.py share - the host build of fbstab_amd/csrc/fb_condense_sweep_adjoint.h
(tests/hostsim/condense_sweep_adjoint.cc), the step function's numpy reference with its rounding rule, and the
backward recursion through a logged sweep of the condensed route in numpy with a pluggable per-step adjoint.

The recursion (include/fbstab_hip.h): lambda = 0 and for k = T-1 .. 0: mu = gx[k] + lambda; eflag -1: lambda <- 0;
eflag != 0: lambda <- A_p'mu; otherwise one dense adjoint at the logged (U_k, v_k) with the seed
(gu[k] + B_p'mu, 0, .., 0): a failed factorisation counts in ``status`` and gives lambda <- A_p'mu, a good one gives
lambda <- A_p'mu + F'(-dU) + G'dv and adds the finish's gradients at the expanded point to the sums."""
import ctypes as C

import numpy as np

from fbstab_amd.hip_api import MPC_SEQ
from tests import condense_adjoint_helpers as cah
from tests import condense_helpers as ch
from tests import condense_sweep_helpers as csh
from tests import hostsim
from tests import linear_reference as lr

LD = ch.LD
SIX = 6  # the steps of the recursion tests
U2 = LD(2.0) ** -53


def ptr(a):
    return None if a is None else a.ctypes.data


class HostSweepAdjoint:
    """condense_sweep_adjoint_step / _finish / _begin of fb_condense_sweep_adjoint.h and both instantiations of
    condense_adjoint_finish with Ctx<1> (hostsim/condense_sweep_adjoint.cc)."""

    def __init__(self):
        self.lib = C.CDLL(hostsim.build("libhostsim_condense_sweep_adjoint.so", "condense_sweep_adjoint.cc",
                                        ("fb_common.h", "fb_batch.h", "fb_condense_plan.h", "fb_adjoint.h", "fb_condense.h",
                                         "fb_condense_adjoint.h", "fb_condense_sweep.h", "fb_condense_sweep_adjoint.h")))
        self.lib.hostsim_sweep_adjoint_step.argtypes = [C.c_void_p] * 4
        self.lib.hostsim_sweep_adjoint_step.restype = None
        self.lib.hostsim_sweep_adjoint_plain_finish.argtypes = [C.c_int] * 5 + [C.c_void_p] * 9 + [C.c_int] + [
            C.c_void_p] * 3
        self.lib.hostsim_sweep_adjoint_finish.argtypes = [C.c_int] * 4 + [C.c_void_p] * 7 + [C.c_int] + [C.c_void_p] * 2
        self.lib.hostsim_sweep_adjoint_finish.restype = None
        self.lib.hostsim_sweep_adjoint_begin.argtypes = [C.c_int] * 4 + [C.c_void_p] * 5
        self.lib.hostsim_sweep_adjoint_begin.restype = None

    def step(self, sizes, A, B, close=None, open_=None, affine=None, T=0, stage_m=False, status=None, gf0=None,
             gb0=None, want_x0=False):
        """One launch on ``(batch, n)`` arrays.  ``A``/``B``: row-major per-trajectory plants.
        ``close``: None, or dict(eflag, st1, st2, dU, dv, mu[, dl0]) of the closed step.
        ``open_``: None, or dict(eflag, x[, gu, gx]) of the opened step.
        ``affine``: None (lambda from ``dl0``, no f_c, b_c), or (M (rows, ne nx), f0, b0).
        ``status`` (int32), ``gf0``, ``gb0``: updated IN PLACE where given.
        Returns dict(mu, mu_log, gU, f, b, dl0 - of the opened step -, x0 - the lambda of a launch that does not
        open)."""
        N, nx, nu, nc = sizes
        nzc, nv = (N + 1) * nu, (N + 1) * nc
        src = close if close is not None else open_
        Bn = len(src["eflag"])
        f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)
        i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
        Ac, Bc = f64(np.asarray(A).transpose(0, 2, 1)), f64(np.asarray(B).transpose(0, 2, 1))
        mu = f64(close["mu"]).copy() if close is not None else np.full((Bn, nx), np.nan)
        dl0 = None
        if affine is None:
            dl0 = f64(close["dl0"]).copy() if close is not None else np.full((Bn, nx), np.nan)
        res = dict(mu=mu, dl0=dl0)
        keep = []
        hold = lambda a: (keep.append(a), a)[1]
        dU = hold(f64(close["dU"])) if close is not None else None
        dv = hold(f64(close["dv"])) if close is not None else None
        ec = hold(i32(close["eflag"])) if close is not None else None
        s1 = hold(i32(close["st1"])) if close is not None else None
        s2 = hold(i32(close["st2"])) if close is not None else None
        st = status if status is not None else np.zeros(Bn, dtype=np.int32)
        eo = gu = gx = xl = None
        if open_ is not None:
            eo, xl = hold(i32(open_["eflag"])), hold(f64(open_["x"]))
            gu = hold(f64(open_["gu"])) if open_.get("gu") is not None else None
            gx = hold(f64(open_["gx"])) if open_.get("gx") is not None else None
            res["mu_log"] = np.full((Bn, nx), np.nan)
            res["gU"] = np.full((Bn, nzc), np.nan)
        M = f0 = b0 = None
        sM = 0
        if affine is not None:
            M, f0, b0 = (hold(f64(a)) for a in affine)
            sM = 0 if M.shape[0] == 1 else M.shape[1]
            if open_ is not None:
                res["f"], res["b"] = np.full((Bn, nzc), np.nan), np.full((Bn, nv), np.nan)
        if open_ is None and want_x0:
            res["x0"] = np.full((Bn, nx), np.nan)
        dp = (C.c_void_p * 19)(ptr(dU), ptr(dv), ptr(dl0), ptr(mu), ptr(Ac), ptr(Bc), ptr(gu), ptr(gx),
                               ptr(res.get("mu_log")), ptr(res.get("gU")), ptr(xl), ptr(M), ptr(f0), ptr(b0),
                               ptr(res.get("f")), ptr(res.get("b")), ptr(gf0), ptr(gb0), ptr(res.get("x0")))
        ip = (C.c_int * 10)(N, nx, nu, nc, Bn, int(close is not None), int(open_ is not None),
                            int(affine is not None), T, int(stage_m))
        sp = (C.c_longlong * 8)(nx * nx, nx * nu, sM, nzc, nv, nzc, nv, nx)
        npp = (C.c_void_p * 5)(ptr(ec), ptr(eo), ptr(s1), ptr(s2), ptr(st))
        self.lib.hostsim_sweep_adjoint_step(ip, sp, dp, npp)
        res["status"] = st
        return res

    def plain_finish(self, acc, p, q, x, gz, gl, dU, dv, grads, ok=True):
        """condense_adjoint_finish<acc> of QP ``q`` into the dict ``grads`` (name -> array, IN PLACE)."""
        keep, data = ch.HostCondense._data(p, q)
        f64 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
        z, l, v = (f64(a) for a in x)
        gz, gl, dU, dv = (f64(a) for a in (gz, gl, dU, dv))
        gptr = (C.c_void_p * 12)(*[ptr(grads.get(k)) for k in ch.MPC_NAMES])
        self.lib.hostsim_sweep_adjoint_plain_finish(int(acc), *p.sizes(), data, ptr(z), ptr(l), ptr(v), ptr(gz), ptr(gl),
                                                    ptr(dU), ptr(dv), gptr, 1 if ok else 0, None, None, None)

    def finish(self, p, q, xk, U, v, dU, dv, grads, ok=True):
        """The finish kernel's work on trajectory ``q`` at the state ``xk``: adds to ``grads`` IN PLACE (its "x0"
        entry, where present, receives -dl[0:nx])."""
        X0 = p.arrays["x0"].copy()
        X0[q] = xk
        m = csh.with_x0(p, X0)
        keep, data = ch.HostCondense._data(m, q)
        f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)
        U, v, dU, dv = (f64(a) for a in (U, v, dU, dv))
        z, l, gz = np.full(p.nz, np.nan), np.full(p.nl, np.nan), np.zeros(p.nz)
        gptr = (C.c_void_p * 12)(*[ptr(grads.get(k)) for k in ch.MPC_NAMES])
        self.lib.hostsim_sweep_adjoint_finish(*p.sizes(), data, ptr(U), ptr(v), ptr(dU), ptr(dv), ptr(gz), gptr,
                                              1 if ok else 0, ptr(z), ptr(l))
        return z, l


# ---- the step function in numpy -----------------------------------------------------------------------------------
def case_of(eflag, st1, st2):
    """0: retired, 1: the plant alone (no solution, or a failed factorisation), 2: the adjoint contributes."""
    e = np.asarray(eflag)
    bad = (np.asarray(st1) != 0) | (np.asarray(st2) != 0)
    return np.where(e == -1, 0, np.where((e != 0) | bad, 1, 2))


def lambda_reference(A, F, G, mu, dU, dv, cs):
    """(lambda in longdouble, S = the sum of the magnitudes of its terms) of one trajectory: A row-major (nx, nx),
    F (nzc, nx), G (nv, nx)."""
    Al, Fl, Gl, m, du, dvl = (np.asarray(a, dtype=LD) for a in (A, F, G, mu, dU, dv))
    if cs == 0:
        return np.zeros(Al.shape[0], dtype=LD), np.zeros(Al.shape[0], dtype=LD)
    lam, S = Al.T @ m, np.abs(Al).T @ np.abs(m)
    if cs == 2:
        lam = lam + Fl.T @ (-du) + Gl.T @ dvl
        S = S + np.abs(Fl).T @ np.abs(du) + np.abs(Gl).T @ np.abs(dvl)
    return lam, S


def lambda_bound(ne, nx, S):
    """(ne + nx + 3) 2^-53 S: one rounding per term of the chain and spares."""
    return LD(ne + nx + 3) * U2 * S


def seed_reference(B, mu, gu):
    """(gU[0:nu] in longdouble, S) of one trajectory: B row-major (nx, nu)."""
    Bl, m, g = (np.asarray(a, dtype=LD) for a in (B, mu, gu))
    return g + Bl.T @ m, np.abs(g) + np.abs(Bl).T @ np.abs(m)


def seed_bound(nu, S):
    return LD(nu + 2) * U2 * S


# ---- the recursion in numpy -----------------------------------------------------------------------------------------
def reference_condensed_sweep_adjoint(step_fn, p, A, B, maps, log, gu, gx):
    """``step_fn(k, q, xk, U, v, gU) -> (status, dU, dv, table)``: the dense adjoint of trajectory ``q`` at step k
    (``table``: name -> gradient of the 11 data sequences at that step, or None).  ``maps``: per trajectory (F, G).
    Everything is carried in longdouble.  Returns (grads, status, mu_log); grads["x0"] is the final lambda."""
    N, nx, nu, nc = p.sizes()
    T, Bn = log["eflag"].shape
    lens = p.seq_lengths()
    grads = {k: np.zeros((Bn, lens[k]), dtype=LD) for k in MPC_SEQ}
    status = np.zeros(Bn, dtype=np.int32)
    mu_log = np.zeros((T, Bn, nx), dtype=LD)
    lam = np.zeros((Bn, nx), dtype=LD)
    for k in range(T - 1, -1, -1):
        for q in range(Bn):
            mu = (LD(0) if gx is None else np.asarray(gx[k][q], dtype=LD)) + lam[q]
            mu_log[k, q] = mu
            e = log["eflag"][k][q]
            Aq, Bq = np.asarray(A[q], dtype=LD), np.asarray(B[q], dtype=LD)
            if e == -1:
                lam[q] = 0
                continue
            atm = Aq.T @ mu
            if e != 0:
                lam[q] = atm
                continue
            gU = np.zeros((N + 1) * nu, dtype=LD)
            gU[:nu] = (LD(0) if gu is None else np.asarray(gu[k][q], dtype=LD)) + Bq.T @ mu
            st, dU, dv, tab = step_fn(k, q, log["x"][k][q], log["U"][k][q], log["v"][k][q], gU)
            if st != 0:
                status[q] += 1
                lam[q] = atm
                continue
            F, G = maps[q]
            lam[q] = atm + np.asarray(F, dtype=LD).T @ (-np.asarray(dU, dtype=LD)) + np.asarray(G, dtype=LD).T @ np.asarray(dv, dtype=LD)
            if tab is not None:
                for name in MPC_SEQ:
                    if name != "x0":
                        grads[name][q] += tab[name]
    grads["x0"] = lam.copy()
    return grads, status, mu_log


def expanded_point(p, q, xk, U, v):
    """(problem of one QP with x0 := xk, (z, l, v)) in float64 from the longdouble expand of the logged point."""
    one = lr.one_qp(p, q)
    m = csh.with_x0(one, np.asarray(xk, dtype=np.float64)[None])
    z, l, _, _ = ch.expand_reference(m, 0, np.asarray(U, dtype=LD), np.asarray(v, dtype=LD), np.asarray(v, dtype=LD))
    return m, (z.astype(np.float64), l.astype(np.float64), np.asarray(v, dtype=np.float64))


def chain_step(p, sigma=cah.SIGMA):
    """The per-step adjoint from cah.chain_reference in longdouble at the expanded logged point, with the gradient
    table of lr.mpc_gradient_table."""
    N, nx, nu, nc = p.sizes()

    def fn(k, q, xk, U, v, gU):
        m, x = expanded_point(p, q, xk, U, v)
        gz = np.zeros((N + 1, nx + nu), dtype=LD)
        gz[0, nx:] = gU[:nu]
        gz = gz.reshape(-1)
        c = cah.chain_reference(m, 0, x, (gz.astype(np.float64), None, None), sigma)
        tab = lr.mpc_gradient_table(m, x, (c["dz"], c["dl"], c["dv"]))
        return 0, c["dU"], c["dv"], tab
    return fn


def rel_gaps(got, ref, rows=None):
    """Per sequence: max over the trajectories of max|got - ref| / max|ref| (1 where the reference is zero)."""
    out = {}
    for k in MPC_SEQ:
        if k not in got:
            continue
        w = 0.0
        for q in (range(ref[k].shape[0]) if rows is None else rows):
            top = float(np.abs(ref[k][q]).max())
            w = max(w, float(np.abs(np.asarray(got[k][q], dtype=LD) - ref[k][q]).max()) / (top if top > 0 else 1.0))
        out[k] = w
    return out
