"""CPU tests of forward mode through the closed-loop sweep of the condensed route
(fbstab_hip_mpc_condensed_receding_sweep_tangent; fbstab_amd/csrc/fb_condense_sweep_tangent.h compiled for the host):
the step function's bookkeeping and rounding, the rules' power against seeded defects, duality of the recursion with
the backward recursion of tests/condense_sweep_adjoint_helpers.py, and the host stage
(condensed_sweep_tangent_run of fb_condense_stage.h) in a stand-alone driver, plain and under the sanitizers."""
import functools
import os
import subprocess

import numpy as np
import pytest

from fbstab_amd import hip_api
from tests import condense_sweep_adjoint_helpers as sah
from tests import condense_sweep_helpers as csh
from tests import condense_sweep_tangent_helpers as sth
from tests.test_host_stage import CSRC, HOSTSIM

LD = sth.LD
SIZES = (3, 5, 2, 3)        # ne = 20, nx = 5: odd sizes, nothing a multiple of anything
BN = 7                      # cases: retired, not SUCCESS, status 1 set, status 2 set, good x 3


@functools.lru_cache(maxsize=None)
def host():
    return sth.HostSweepTangent()


@functools.lru_cache(maxsize=None)
def host_adjoint():
    return sah.HostSweepAdjoint()


def step_case(seed=0):
    rng = np.random.default_rng(seed)
    N, nx, nu, nc = SIZES
    nzc, nv = (N + 1) * nu, (N + 1) * nc
    ne = nzc + nv
    d = dict(A=rng.standard_normal((BN, nx, nx)), B=rng.standard_normal((BN, nx, nu)),
             M=rng.standard_normal((BN, ne * nx)), f0=rng.standard_normal((BN, nzc)), b0=rng.standard_normal((BN, nv)),
             dx=rng.standard_normal((BN, nx)), dU=rng.standard_normal((BN, nzc)), dw=rng.standard_normal((BN, nx)),
             eflag=np.array([-1, 3, 0, 0, 0, 0, 0], dtype=np.int32), st1=np.array([0, 0, 1, 0, 0, 0, 0], dtype=np.int32),
             st2=np.array([0, 1, 0, 1, 0, 0, 0], dtype=np.int32), x=rng.standard_normal((BN, nx)),
             df0=rng.standard_normal((BN, nzc)), db0=rng.standard_normal((BN, nv)),
             eflag_open=np.array([0, 0, -1, 0, 5, 0, 0], dtype=np.int32))
    return d, ne


def parts(d, q):
    N, nx, nu, nc = SIZES
    nzc = (N + 1) * nu
    W = d["M"][q].reshape(nx, -1).T
    return W[:nzc], W[nzc:]


def close_args(d, dw=True):
    return dict(eflag=d["eflag"], st1=d["st1"], st2=d["st2"], dU=d["dU"], dx=d["dx"], dw=d["dw"] if dw else None)


def open_args(d, dirs=True):
    return dict(eflag=d["eflag_open"], x=d["x"], df0=d["df0"] if dirs else None, db0=d["db0"] if dirs else None)


OUT = ("dx", "du", "dx_out", "gU", "gv", "f", "b")


# ---- 1. bookkeeping ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("staged", [False, True])
@pytest.mark.parametrize("T", [1, 2, 5])
def test_step_bookkeeping_is_exact(T, staged):
    """All four cases in one batch, T = 1, 2, 5 trajectories per workgroup, M per trajectory or one staged image: the
    case rule, status, du exactly zero where the step does not contribute, dx+ exactly zero once retired (dw is not
    added), zero seeds where the opened step does not contribute, f_c and b_c the bits of the adjoint kernel's open."""
    d, ne = step_case()
    N, nx, nu, nc = SIZES
    if staged:
        d["M"] = d["M"][:1]
    Mfull = np.repeat(d["M"], BN, axis=0) if staged else d["M"]
    cs = sth.case_of(d["eflag"], d["st1"], d["st2"])
    assert list(cs) == [0, 1, 1, 1, 2, 2, 2]
    status = np.full(BN, 3, dtype=np.int32)
    r = host().step(SIZES, d["A"], d["B"], (d["M"], d["f0"], d["b0"]), close=close_args(d), open_=open_args(d), T=T,
                    stage_m=staged, status=status)
    assert list(status) == [3, 3, 4, 4, 3, 3, 3]      # += 1 where a factorisation failed on a SUCCESS step only
    assert not r["du"][cs != 2].any() and np.array_equal(r["du"][cs == 2], d["dU"][cs == 2, :nu])
    assert not r["dx"][0].any() and d["dw"][0].all()                       # retired: the constant 0, dw not added
    assert np.array_equal(r["dx"], r["dx_out"]) and r["dx"][1:].all()
    good = d["eflag_open"] == 0
    assert not r["gU"][~good].any() and not r["gv"][~good].any()
    assert r["gU"][good].all() and r["gv"][good].all()
    # f_c, b_c: bitwise those of the adjoint kernel's open at the same state
    ra = host_adjoint().step(SIZES, d["A"], d["B"], affine=(d["M"], d["f0"], d["b0"]), T=T, stage_m=staged,
                             open_=dict(eflag=d["eflag_open"], x=d["x"]))
    assert np.array_equal(r["f"], ra["f"]) and np.array_equal(r["b"], ra["b"])
    # T and a shared staged image change nothing
    r1 = host().step(SIZES, d["A"], d["B"], (Mfull, d["f0"], d["b0"]), close=close_args(d), open_=open_args(d), T=1)
    for k in OUT:
        assert np.array_equal(r[k], r1[k]), k
    # the launch that does not close: dx = dx0 (NULL: zero), status = 0; the one that does not open writes no seed
    first = host().step(SIZES, d["A"], d["B"], (d["M"], d["f0"], d["b0"]), open_=open_args(d), dx0=d["dx"], T=T,
                        stage_m=staged)
    assert np.array_equal(first["dx"], d["dx"]) and not first["status"].any()
    null = host().step(SIZES, d["A"], d["B"], (d["M"], d["f0"], d["b0"]), open_=open_args(d, dirs=False), T=T,
                       stage_m=staged)
    assert not null["dx"].any() and not null["gU"].any() and not null["gv"].any()
    assert np.array_equal(null["f"], r["f"]) and np.array_equal(null["b"], r["b"])
    last = host().step(SIZES, d["A"], d["B"], (d["M"], d["f0"], d["b0"]), close=close_args(d), T=T, stage_m=staged)
    assert np.array_equal(last["dx"], r["dx"]) and np.array_equal(last["du"], r["du"])
    # NULL dw and NULL df0, db0 are zeros, bit for bit
    z = dict(d, dw=np.zeros_like(d["dw"]), df0=np.zeros_like(d["df0"]), db0=np.zeros_like(d["db0"]))
    ra = host().step(SIZES, d["A"], d["B"], (d["M"], d["f0"], d["b0"]), close=close_args(d, dw=False),
                     open_=open_args(d, dirs=False), T=T, stage_m=staged)
    rb = host().step(SIZES, d["A"], d["B"], (d["M"], d["f0"], d["b0"]), close=close_args(z), open_=open_args(z), T=T,
                     stage_m=staged)
    for k in OUT:
        assert np.array_equal(ra[k], rb[k]) and not (np.signbit(ra[k]) != np.signbit(rb[k])).any(), k


# ---- 2. rounding -------------------------------------------------------------------------------------------------------
def launch(d, T=2):
    return host().step(SIZES, d["A"], d["B"], (d["M"], d["f0"], d["b0"]), close=close_args(d), open_=open_args(d), T=T)


def test_step_rounding_rules():
    """dx+ within (nx + nu + 3) 2^-53, the seeds within (nx + 2) 2^-53 of the sum of the magnitudes of their terms,
    against longdouble (the rules of the adjoint helpers, lambda_bound and seed_bound, on the forward chains)."""
    d, ne = step_case(1)
    N, nx, nu, nc = SIZES
    cs = sth.case_of(d["eflag"], d["st1"], d["st2"])
    r = launch(d)
    worst = [0.0, 0.0]
    for q in range(BN):
        ref, S = sth.dx_reference(d["A"][q], d["B"][q], d["dx"][q], d["dU"][q], d["dw"][q], cs[q])
        bound = sth.dx_bound(nx, nu, S)
        err = np.abs(r["dx"][q].astype(LD) - ref)
        assert (err <= bound).all(), (q, cs[q])
        if cs[q]:
            worst[0] = max(worst[0], float((err / bound).max()))
        F, G = parts(d, q)
        (gU, gv), (SU, Sv) = sth.seeds_reference(F, G, r["dx"][q], d["df0"][q], d["db0"][q], d["eflag_open"][q] == 0)
        for got, want, S in ((r["gU"][q], gU, SU), (r["gv"][q], gv, Sv)):
            err = np.abs(got.astype(LD) - want)
            assert (err <= sth.seed_bound(nx, S)).all(), q
            if S.any():
                worst[1] = max(worst[1], float((err / sth.seed_bound(nx, S)).max()))
    print("dx+: worst |error| / bound = %.3g; seeds: %.3g" % tuple(worst))


def test_rules_catch_seeded_defects():
    """The rules must refuse a dropped dw, B_p' for B_p (a square input block), G dx with the wrong sign, and
    dU[nu:2nu] taken for du."""
    d, ne = step_case(2)
    N, nx, nu, nc = SIZES
    cs = sth.case_of(d["eflag"], d["st1"], d["st2"])
    r = launch(d)
    good = [q for q in range(BN) if cs[q] == 2]

    def dx_violations(dx_of):
        bad = 0
        for q in range(BN):
            ref, S = sth.dx_reference(d["A"][q], d["B"][q], d["dx"][q], d["dU"][q], d["dw"][q], cs[q])
            bad += int((np.abs(dx_of(q).astype(LD) - ref) > sth.dx_bound(nx, nu, S)).any())
        return bad

    def defect(q, drop_dw=False, wrong_du=False):
        if cs[q] == 0:
            return np.zeros(nx)
        out = d["A"][q] @ d["dx"][q]
        if cs[q] == 2:
            out = out + d["B"][q] @ (d["dU"][q, nu:2 * nu] if wrong_du else d["dU"][q, :nu])
        return out if drop_dw else out + d["dw"][q]
    assert dx_violations(lambda q: r["dx"][q]) == 0
    assert dx_violations(lambda q: defect(q)) == 0                         # (the numpy form itself passes)
    assert dx_violations(lambda q: defect(q, drop_dw=True)) == BN - 1      # every trajectory that is not retired
    assert dx_violations(lambda q: defect(q, wrong_du=True)) == len(good)
    # B_p' for B_p: on a plant with nu = nx inputs the two differ by the transpose alone
    rng = np.random.default_rng(3)
    Asq, Bsq, dx, dU = (rng.standard_normal(s) for s in ((nx, nx), (nx, nx), nx, nx))
    ref, S = sth.dx_reference(Asq, Bsq, dx, dU, None, 2)
    assert (np.abs((Asq @ dx + Bsq @ dU).astype(LD) - ref) <= sth.dx_bound(nx, nx, S)).all()
    assert (np.abs((Asq @ dx + Bsq.T @ dU).astype(LD) - ref) > sth.dx_bound(nx, nx, S)).any()
    # the seeds: G dx with the wrong sign
    opened = [q for q in range(BN) if d["eflag_open"][q] == 0]

    def seed_violations(gv_of):
        bad = 0
        for q in range(BN):
            F, G = parts(d, q)
            (_, gv), (_, Sv) = sth.seeds_reference(F, G, r["dx"][q], d["df0"][q], d["db0"][q], d["eflag_open"][q] == 0)
            bad += int((np.abs(gv_of(q).astype(LD) - gv) > sth.seed_bound(nx, Sv)).any())
        return bad
    assert seed_violations(lambda q: r["gv"][q]) == 0
    flipped = lambda q: (d["db0"][q] - parts(d, q)[1] @ r["dx"][q]) if d["eflag_open"][q] == 0 else np.zeros_like(d["db0"][q])
    assert seed_violations(flipped) == len([q for q in opened if r["dx"][q].any()])


# ---- 3. duality of the recursion ---------------------------------------------------------------------------------------
def host_recursion(p, A, B, M, f0, b0, log, step_fn, dx0, dw, df0, db0, T=2):
    """The forward recursion through the HOST BUILD of the step kernel: launch, the dense step of ``step_fn`` on the
    seeds the launch wrote (in longdouble, rounded to double where the kernel reads it), launch ...  Returns (du, dx,
    status) as the kernel wrote them."""
    sizes = p.sizes()
    N, nx, nu, nc = sizes
    steps, Bn = log["eflag"].shape
    nzc = (N + 1) * nu
    du, dx = np.zeros((steps, Bn, nu)), np.zeros((steps, Bn, nx))
    status = np.full(Bn, 9, dtype=np.int32)
    opened = lambda k: dict(eflag=log["eflag"][k], x=log["x"][k], df0=df0, db0=db0)
    r = host().step(sizes, A, B, (M, f0, b0), open_=opened(0), dx0=dx0, T=T, status=status)
    for k in range(steps):
        dU = np.zeros((Bn, nzc))
        for q in range(Bn):
            if log["eflag"][k][q] == 0:
                dU[q] = step_fn(k, q, log["x"][k][q], log["U"][k][q], log["v"][k][q], r["gU"][q].astype(LD),
                                r["gv"][q].astype(LD))[1].astype(np.float64)
        zero = np.zeros(Bn, dtype=np.int32)
        r = host().step(sizes, A, B, (M, f0, b0), T=T, status=status,
                        close=dict(eflag=log["eflag"][k], st1=zero, st2=zero, dU=dU, dx=r["dx"], dw=dw[k]),
                        open_=opened(k + 1) if k + 1 < steps else None)
        du[k], dx[k] = r["du"], r["dx_out"]
    return du, dx, status


@pytest.mark.parametrize("name", csh.LOOP_FIXTURES)
def test_recursion_is_dual_to_the_backward_recursion(name):
    """Six steps over the oracle's logs (RETIRES puts the retired case inside them).  One DenseOperator W per (step,
    trajectory) serves both recursions - the forward one applies W, the backward one W' - so
    sum_k <gu_k, du_k> + <gx_k, dx_(k+1)> = <lambda_0, dx0> + sum_k <mu_k, dw_k> [not retired] + <gf0, df0> + <gb0, db0>
    holds to 50 steps 2^-64 of the sum of the magnitudes of the terms when both are carried in longdouble; and the
    host build of the step kernel, fed the same W, lies within the step rules carried through the recursion
    (condense_sweep_tangent_helpers.recursion_error_bound) of the longdouble forward recursion, entry by entry."""
    p, A, B, w = csh.setup(name)
    full = csh.oracle_loop(name)
    assert csh.retirement(full["eflag"]) == csh.RETIRES[name]
    assert all(k < sah.SIX for k in csh.RETIRES[name].values())   # the retired case lies inside the six steps
    log = {k: full[k][:sah.SIX] for k in ("u", "x", "U", "v", "eflag")}
    N, nx, nu, nc = p.sizes()
    nzc, nv = (N + 1) * nu, p.nv
    aff = csh.condenser(name).affine()
    maps = [(a[1], a[3]) for a in aff]
    rng = np.random.default_rng(12)
    gu, gx = rng.standard_normal((sah.SIX, p.batch, nu)), rng.standard_normal((sah.SIX, p.batch, nx))
    dx0, dw = rng.standard_normal((p.batch, nx)), rng.standard_normal((sah.SIX, p.batch, nx))
    df0, db0 = rng.standard_normal((p.batch, nzc)), rng.standard_normal((p.batch, nv))
    op = sth.DenseOperator(p)
    du, dx, tstatus = sth.reference_condensed_sweep_tangent(op.forward(), p, A, B, maps, log, dx0, dw, df0, db0)
    # the backward recursion with gf0, gb0 summed beside it: its step is W'(gU, 0), f_bar = -dU, b_bar = dv
    gf0, gb0 = np.zeros((p.batch, nzc), dtype=LD), np.zeros((p.batch, nv), dtype=LD)
    back = op.backward()

    def backward_step(k, q, xk, U, v, gU):
        st, dU, dv, tab = back(k, q, xk, U, v, gU)
        gf0[q] += -dU
        gb0[q] += dv
        return st, dU, dv, tab
    grads, astatus, mu = sah.reference_condensed_sweep_adjoint(backward_step, p, A, B, maps, log, gu, gx)
    assert not tstatus.any() and not astatus.any()
    lhs, rhs, S = sth.duality_sides(gu, gx, du, dx, grads["x0"], mu, log["eflag"], dx0, dw, gf0, gb0, df0, db0)
    bar = LD(50 * sah.SIX) * LD(2.0) ** -64
    live = S > 0            # (a trajectory retired at step 0 has no term at all)
    print(name, "duality: worst |lhs - rhs| / S = %.3g (bar %.3g)" % (float((np.abs(lhs - rhs)[live] / S[live]).max()), float(bar)))
    assert live.sum() >= p.batch - 1 and (np.abs(lhs - rhs) <= bar * S).all(), (lhs, rhs, S)
    for q, k in csh.RETIRES[name].items():
        assert not du[k:, q].any() and not dx[k:, q].any()
    # the kernel's host build on the same operator: per entry, the step rules carried through the recursion
    M = np.stack([np.concatenate([F, G], axis=0).T.reshape(-1) for F, G in maps])
    f0, b0 = np.stack([a[0] for a in aff]), np.stack([a[2] for a in aff])
    hdu, hdx, hstatus = host_recursion(p, A, B, M, f0, b0, log, op.forward(), dx0, dw, df0, db0)
    assert not hstatus.any()
    bdu, bdx = sth.recursion_error_bound(op, p, A, B, maps, log, du, dx, dx0, dw, df0, db0)
    worst = 0.0
    for got, ref, bound in ((hdu, du, bdu), (hdx, dx, bdx)):
        err = np.abs(got.astype(LD) - ref)
        assert (err <= bound).all(), (name, float((err / np.where(bound > 0, bound, 1)).max()))
        worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
        # (where the dense operator is ill conditioned - four_wave, double_integrator - the entrywise bound is wide:
        # the sanity figure of the adjoint's test stays beside it)
        assert sth.rel_gap(got, ref) <= 1e-9, (name, sth.rel_gap(got, ref))
    print(name, "host build against the longdouble recursion: worst |error| / bound = %.3g, largest bound %.3g of the "
          "largest entry, gaps du %.3g dx %.3g" % (worst, float(bdx.max() / np.abs(dx).max()), sth.rel_gap(hdu, du),
                                                    sth.rel_gap(hdx, dx)))
    for q, k in csh.RETIRES[name].items():
        assert not hdu[k:, q].any() and not hdx[k:, q].any()


@pytest.mark.parametrize("name", ["small", "double_integrator"])
def test_recursion_m_form_against_the_mpc_form(name):
    """The recursion on the condensed seeds gU = -(df0 + F dx), gv_c = db0 + G dx (df0, db0: the condensed images of
    the directions of q, r, c, d at x0 = 0) lands where the recursion that hands every step the MPC-form directions
    (x0 := dx, q, r, c, d; tangent_helpers.tangent_rhs, chain_reference) does: the sign and layout conventions of the
    new call are those of the single-point forward mode.  That comparison is between two test helpers; the same
    recursion through the HOST BUILD of the step kernel (the images rounded to double) must land there too.  A sanity
    figure at 1e-9 of the largest entry, as the adjoint's M-form test has it."""
    from tests import condense_adjoint_helpers as cah
    from tests import condense_helpers as ch
    from tests import linear_reference as lr
    p, A, B, w = csh.setup(name)
    full = csh.oracle_loop(name)
    log = {k: full[k][:sah.SIX] for k in ("u", "x", "U", "v", "eflag")}
    N, nx, nu, nc = p.sizes()
    rng = np.random.default_rng(13)
    lens = p.seq_lengths()
    dd = {k: rng.standard_normal((p.batch, lens[k])) for k in ("q", "r", "c", "d")}
    dx0, dw = rng.standard_normal((p.batch, nx)), rng.standard_normal((sah.SIX, p.batch, nx))
    # the images of the directions: condensing is linear in q, r, c, d, and at x0 = 0 it is the images' own base
    arrays = {k: a.copy() for k, a in p.arrays.items()}
    arrays.update(dd)
    arrays["x0"] = np.zeros_like(arrays["x0"])
    zero = {k: np.zeros_like(a) for k, a in dd.items()}
    base = dict(arrays)
    base.update(zero)
    from tools import fixtures as fx
    pd, p0 = fx.MpcProblem(N, nx, nu, nc, arrays), fx.MpcProblem(N, nx, nu, nc, base)
    img = [(ch.condense_reference(pd, q), ch.condense_reference(p0, q)) for q in range(p.batch)]
    df0 = np.stack([a["f"] - b["f"] for a, b in img])
    db0 = np.stack([a["b"] - b["b"] for a, b in img])
    maps = [(a[1], a[3]) for a in csh.condenser(name).affine()]
    op = sth.DenseOperator(p)
    du, dx, st = sth.reference_condensed_sweep_tangent(op.forward(), p, A, B, maps, log, dx0, dw, df0, db0)
    one = lambda k, q: {n: a[q] for n, a in dd.items()}
    mu_, mx, ms = sth.mpc_form_recursion(sth.chain_mpc_step(p, one), p, A, B, log, dx0, dw)
    assert np.array_equal(st, ms)
    print(name, "M form against MPC form: du %.3g dx %.3g" % (sth.rel_gap(du, mu_), sth.rel_gap(dx, mx)))
    assert np.abs(mu_).max() > 0 and sth.rel_gap(du, mu_) <= 1e-9 and sth.rel_gap(dx, mx) <= 1e-9
    # ... and so does the host build of the step kernel on the images rounded to double: the shipped step function
    # has the conventions of the single-point forward mode (the comparison above is between two helpers alone)
    aff = csh.condenser(name).affine()
    M = np.stack([np.concatenate([F, G], axis=0).T.reshape(-1) for F, G in maps])
    f0, b0 = np.stack([a[0] for a in aff]), np.stack([a[2] for a in aff])
    hdu, hdx, hs = host_recursion(p, A, B, M, f0, b0, log, op.forward(), dx0, dw, df0.astype(np.float64),
                                  db0.astype(np.float64))
    assert np.array_equal(hs, ms)
    print(name, "host build against MPC form: du %.3g dx %.3g" % (sth.rel_gap(hdu, mu_), sth.rel_gap(hdx, mx)))
    assert sth.rel_gap(hdu, mu_) <= 1e-9 and sth.rel_gap(hdx, mx) <= 1e-9


def test_the_central_difference_seed_stays_inside_the_cap_by_the_oracle_alone():
    """The GPU test's central differences leave out trajectories whose exit flags or active sets differ between the
    two perturbed runs, at most 1 in 5: with the chosen seed the oracle's own loop stays inside that cap."""
    p, A, B, w, cu, cx, dirs = sth.fd_setup()
    left = sth.fd_left_out(p, sth.fd_runs(sth.oracle_sweep(p, A, B), p, w, dirs))
    print("left out by the oracle's loop:", left)
    assert len(left) <= p.batch // 5, left


# ---- 4. the host stage -------------------------------------------------------------------------------------------------
GROUPS = ("placement", "carve", "sequence", "refusals")


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def driver(request, tmp_path_factory):
    """-> run(group) -> (exit status, output).  `sanitized`: the same driver built with
    -fsanitize=address,undefined; a finding ends it with a non-zero status."""
    d = tmp_path_factory.mktemp("condense_sweep_tangent_" + request.param)
    exe = str(d / "condense_sweep_tangent_driver")
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", *extra,
                           "-I" + os.path.join(HOSTSIM, "runtime_shim"), "-I" + CSRC, "-o", exe,
                           os.path.join(HOSTSIM, "condense_sweep_tangent_driver.cc")])

    def run(group):
        r = subprocess.run([exe, group], capture_output=True, text=True)
        return r.returncode, r.stdout + r.stderr
    return run


@pytest.mark.parametrize("group", GROUPS)
def test_the_sweep_tangent_stage_places_carves_queues_and_refuses_as_the_header_says(driver, group):
    status, output = driver(group)
    assert status == 0 and output == "", output[-4000:]


def test_the_driver_knows_its_groups(driver):
    assert driver("no such group")[0] == 2


def test_symbols_and_sizes_without_gpu():
    lib = hip_api.load_library()
    for name in ("fbstab_hip_mpc_condensed_receding_sweep_tangent", "fbstab_hip_mpc_condensed_sweep_tangent_sizes"):
        assert name in hip_api.EXPORTED_SYMBOLS and getattr(lib, name).argtypes is not None
    from fbstab_amd import condense
    s = condense.condensed_sweep_tangent_sizes(10, 40, 3, 6)
    f = condense.condensed_sweep_sizes(10, 40, 3, 6)
    assert s["traj_per_group"] == f["traj_per_group"] and s["lds_bytes"] == f["lds_bytes"]
    assert s["work_doubles_per_traj"] == 4 * 33 + 3 * 66 + 40 + 1
    with pytest.raises(Exception):
        condense.condensed_sweep_tangent_sizes(10, 40, 3, 6, traj_per_group=-1)
    assert hasattr(condense.CondensedMpc, "RecedingSweepTangent")
