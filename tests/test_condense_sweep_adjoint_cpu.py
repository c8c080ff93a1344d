"""CPU tests of the adjoint through the closed-loop sweep of the condensed route
(fbstab_hip_mpc_condensed_receding_sweep_adjoint; fbstab_amd/csrc/fb_condense_sweep_adjoint.h compiled for the host):
the step function's bookkeeping and rounding, the rule's power against seeded defects, the accumulating finish, the
recursion against the MPC-form recursion of tests/sweep_adjoint_helpers.py, and central differences of the oracle's
condensed closed loop."""
import functools

import numpy as np
import pytest

from fbstab_amd import hip_api
from fbstab_amd.hip_api import MPC_SEQ
from tests import condense_adjoint_helpers as cah
from tests import condense_helpers as ch
from tests import condense_sweep_adjoint_helpers as sah
from tests import condense_sweep_helpers as csh
from tests import linear_reference as lr
from tests import sweep_adjoint_helpers as mah

LD = sah.LD
SIZES = (3, 5, 2, 3)        # ne = 20, nx = 5: odd sizes, nothing a multiple of anything
BN = 7                      # cases: retired, not SUCCESS, status 1 set, status 2 set, good x 3


@functools.lru_cache(maxsize=None)
def host():
    return sah.HostSweepAdjoint()


def step_case(seed=0):
    rng = np.random.default_rng(seed)
    N, nx, nu, nc = SIZES
    nzc, nv = (N + 1) * nu, (N + 1) * nc
    ne = nzc + nv
    d = dict(A=rng.standard_normal((BN, nx, nx)), B=rng.standard_normal((BN, nx, nu)),
             M=rng.standard_normal((BN, ne * nx)), f0=rng.standard_normal((BN, nzc)), b0=rng.standard_normal((BN, nv)),
             mu=rng.standard_normal((BN, nx)), dU=rng.standard_normal((BN, nzc)), dv=rng.standard_normal((BN, nv)),
             eflag=np.array([-1, 3, 0, 0, 0, 0, 0], dtype=np.int32), st1=np.array([0, 0, 1, 0, 0, 0, 0], dtype=np.int32),
             st2=np.array([0, 1, 0, 1, 0, 0, 0], dtype=np.int32), gu=rng.standard_normal((BN, nu)),
             gx=rng.standard_normal((BN, nx)), x=rng.standard_normal((BN, nx)),
             eflag_open=np.array([0, 0, -1, 0, 5, 0, 0], dtype=np.int32))
    return d, ne


def parts(d, q):
    N, nx, nu, nc = SIZES
    nzc = (N + 1) * nu
    W = d["M"][q].reshape(nx, -1).T
    return W[:nzc], W[nzc:]


def close_args(d):
    return dict(eflag=d["eflag"], st1=d["st1"], st2=d["st2"], dU=d["dU"], dv=d["dv"], mu=d["mu"])


@pytest.mark.parametrize("T", [1, 2, 5])
def test_step_bookkeeping_is_exact(T):
    """All four cases in one batch, T = 1, 2, 5 trajectories per workgroup: the case rule, status, gf0 / gb0, mu and
    mu_log, the zero seed of a step that does not contribute, f_c and b_c in the forward kernel's order."""
    d, ne = step_case()
    N, nx, nu, nc = SIZES
    nzc, nv = (N + 1) * nu, (N + 1) * nc
    cs = sah.case_of(d["eflag"], d["st1"], d["st2"])
    assert list(cs) == [0, 1, 1, 1, 2, 2, 2]
    status = np.full(BN, 3, dtype=np.int32)
    gf0, gb0 = np.ones((BN, nzc)), np.ones((BN, nv))
    r = host().step(SIZES, d["A"], d["B"], close=close_args(d), affine=(d["M"], d["f0"], d["b0"]), T=T,
                    open_=dict(eflag=d["eflag_open"], x=d["x"], gu=d["gu"], gx=d["gx"]), status=status, gf0=gf0, gb0=gb0)
    assert list(status) == [3, 3, 4, 4, 3, 3, 3]      # += 1 where a factorisation failed on a SUCCESS step only
    good = cs == 2
    assert np.array_equal(gf0, np.where(good[:, None], 1.0 + (0.0 - d["dU"]), 1.0))
    assert np.array_equal(gb0, np.where(good[:, None], 1.0 + d["dv"], 1.0))
    # lambda, as the kernel sums it (float64, ascending, FMA or not: compared through the rule in the next test);
    # here: exactly zero where retired, and mu = gx + lambda bit for bit
    lam = r["mu"] - d["gx"]
    assert np.array_equal(r["mu"][0], d["gx"][0])      # retired: lambda = 0
    assert np.array_equal(r["mu"], r["mu_log"])
    for q in range(BN):
        want = d["eflag_open"][q] == 0
        assert np.array_equal(r["gU"][q, nu:], np.zeros(nzc - nu))
        assert (r["gU"][q, :nu] != 0).all() == want and (want or not r["gU"][q].any())
    # f_c, b_c = base + M x with j ascending: the forward kernel's order is one FMA chain from 0
    for q in range(BN):
        F, G = parts(d, q)
        for e in range(ne):
            row = (F if e < nzc else G)[e if e < nzc else e - nzc]
            acc = LD(0)
            for j in range(nx):
                acc = acc + LD(row[j]) * LD(d["x"][q, j])
            got = r["f"][q, e] if e < nzc else r["b"][q, e - nzc]
            base = d["f0"][q, e] if e < nzc else d["b0"][q, e - nzc]
            S = np.abs(row) @ np.abs(d["x"][q]) + abs(base)
            assert abs(LD(got) - (LD(base) + acc)) <= LD(nx + 2) * sah.U2 * S
    assert np.isfinite(lam).all()
    # T and a shared staged image change nothing
    r1 = host().step(SIZES, d["A"], d["B"], close=close_args(d), affine=(d["M"], d["f0"], d["b0"]), T=1,
                     open_=dict(eflag=d["eflag_open"], x=d["x"], gu=d["gu"], gx=d["gx"]))
    for k in ("mu", "gU", "f", "b"):
        assert np.array_equal(r[k], r1[k]), k
    M1 = np.repeat(d["M"][:1], BN, axis=0)
    ra = host().step(SIZES, d["A"], d["B"], close=close_args(d), affine=(M1, d["f0"], d["b0"]), T=T,
                     open_=dict(eflag=d["eflag_open"], x=d["x"], gu=d["gu"], gx=d["gx"]))
    rb = host().step(SIZES, d["A"], d["B"], close=close_args(d), affine=(d["M"][:1], d["f0"], d["b0"]), T=T, stage_m=True,
                     open_=dict(eflag=d["eflag_open"], x=d["x"], gu=d["gu"], gx=d["gx"]))
    for k in ("mu", "gU", "f", "b"):
        assert np.array_equal(ra[k], rb[k]), k


def lambda_of(d, T=2, **kw):
    """The lambda of the closing launch (no open part: it lands in the x0 slot)."""
    return host().step(SIZES, d["A"], d["B"], close=close_args(d), affine=(d["M"], d["f0"], d["b0"]), T=T,
                       want_x0=True, **kw)["x0"]


def test_step_rounding_rule():
    """lambda within (ne + nx + 3) 2^-53 of the sum of the magnitudes of its terms, the seed within (nu + 2) 2^-53,
    against longdouble; the first launch (no close) opens with lambda = 0."""
    d, ne = step_case(1)
    N, nx, nu, nc = SIZES
    cs = sah.case_of(d["eflag"], d["st1"], d["st2"])
    lam = lambda_of(d)
    worst = 0.0
    for q in range(BN):
        F, G = parts(d, q)
        ref, S = sah.lambda_reference(d["A"][q], F, G, d["mu"][q], d["dU"][q], d["dv"][q], cs[q])
        bound = sah.lambda_bound(ne, nx, S)
        assert (np.abs(lam[q].astype(LD) - ref) <= bound).all(), (q, cs[q])
        if cs[q]:
            worst = max(worst, float((np.abs(lam[q].astype(LD) - ref) / bound).max()))
    print("lambda: worst |error| / bound = %.3g" % worst)
    r = host().step(SIZES, d["A"], d["B"], affine=(d["M"], d["f0"], d["b0"]), T=2,
                    open_=dict(eflag=np.zeros(BN, dtype=np.int32), x=d["x"], gu=d["gu"], gx=d["gx"]))
    assert np.array_equal(r["mu"], d["gx"])
    for q in range(BN):
        ref, S = sah.seed_reference(d["B"][q], r["mu"][q], d["gu"][q])
        assert (np.abs(r["gU"][q, :nu].astype(LD) - ref) <= sah.seed_bound(nu, S)).all(), q
    # NULL seeds are zeros
    r0 = host().step(SIZES, d["A"], d["B"], affine=(d["M"], d["f0"], d["b0"]), T=2,
                     open_=dict(eflag=np.zeros(BN, dtype=np.int32), x=d["x"]))
    assert not r0["mu"].any() and not r0["gU"].any()


def test_rule_catches_seeded_defects():
    """The rule must refuse a dropped G'dv, +dU for -dU, B_p for B_p' (a square input block), lambda kept on
    retirement, and one entry of M moved by 1e-9."""
    d, ne = step_case(2)
    N, nx, nu, nc = SIZES
    nzc = (N + 1) * nu
    cs = sah.case_of(d["eflag"], d["st1"], d["st2"])

    def violations(lam_of):
        bad = 0
        for q in range(BN):
            F, G = parts(d, q)
            ref, S = sah.lambda_reference(d["A"][q], F, G, d["mu"][q], d["dU"][q], d["dv"][q], cs[q])
            bad += int((np.abs(lam_of(q).astype(LD) - ref) > sah.lambda_bound(ne, nx, S)).any())
        return bad
    lam = lambda_of(d)
    assert violations(lambda q: lam[q]) == 0
    good = [q for q in range(BN) if cs[q] == 2]

    def defect(q, drop_G=False, plus_dU=False, keep_retired=False, bump=False):
        F, G = parts(d, q)
        F, G = F.copy(), G.copy()
        if bump:
            F[1, 2] += 1e-9
        if cs[q] == 0:
            return d["A"][q].T @ d["mu"][q] if keep_retired else np.zeros(nx)
        out = d["A"][q].T @ d["mu"][q]
        if cs[q] == 2:
            out = out + F.T @ (d["dU"][q] if plus_dU else -d["dU"][q]) + (0 if drop_G else G.T @ d["dv"][q])
        return out
    assert violations(lambda q: defect(q)) == 0                      # (the numpy form itself passes)
    assert violations(lambda q: defect(q, drop_G=True)) == len(good)
    assert violations(lambda q: defect(q, plus_dU=True)) == len(good)
    assert violations(lambda q: defect(q, keep_retired=True)) == 1
    assert violations(lambda q: defect(q, bump=True)) == len(good)
    # B_p for B_p' in the seed: on a plant with nu = nx inputs the two differ by the transpose alone
    rng = np.random.default_rng(3)
    Bsq, mu, gu = rng.standard_normal((nx, nx)), rng.standard_normal(nx), rng.standard_normal(nx)
    ref, S = sah.seed_reference(Bsq, mu, gu)
    assert (np.abs((gu + Bsq.T @ mu).astype(LD) - ref) <= sah.seed_bound(nx, S)).all()
    assert (np.abs((gu + Bsq @ mu).astype(LD) - ref) > sah.seed_bound(nx, S)).any()


def test_accumulating_finish():
    """Twice the accumulating finish from zeroed slots is exactly twice the storing finish; the storing
    instantiation is bitwise today's HostCondenseAdjoint.finish; ok = false adds nothing; the sweep's finish at the
    expanded point equals the storing finish there, and its x0 slot receives -dl[0:nx]."""
    p = ch.problem("small")
    rng = np.random.default_rng(4)
    N, nx, nu, nc = p.sizes()
    lens = p.seq_lengths()
    q = 1
    x = (rng.standard_normal(p.nz), rng.standard_normal(p.nl), rng.standard_normal(p.nv))
    gz = rng.standard_normal(p.nz)
    dU, dv = rng.standard_normal((N + 1) * nu), rng.standard_normal(p.nv)
    old, _ = cah.HostCondenseAdjoint().finish(p, q, x, gz, None, dU, dv)
    store = {k: np.full(lens[k], np.nan) for k in MPC_SEQ}
    host().plain_finish(0, p, q, x, gz, None, dU, dv, store)
    acc = {k: np.zeros(lens[k]) for k in MPC_SEQ}
    for _ in range(2):
        host().plain_finish(1, p, q, x, gz, None, dU, dv, acc)
    for k in MPC_SEQ:
        assert np.array_equal(store[k], old[k]), k
        assert np.array_equal(acc[k], 2.0 * store[k]), k
    before = {k: a.copy() for k, a in acc.items()}
    host().plain_finish(1, p, q, x, gz, None, dU, dv, acc, ok=False)
    for k in MPC_SEQ:
        assert np.array_equal(np.abs(acc[k]), np.abs(before[k])), k
    # the sweep's finish: expand of (U, v) at xk, then the accumulating finish with gz = 0
    U, v, xk = rng.standard_normal((N + 1) * nu), np.abs(rng.standard_normal(p.nv)), rng.standard_normal(nx)
    got = {k: np.zeros(lens[k]) for k in MPC_SEQ}
    z, l = host().finish(p, q, xk, U, v, dU, dv, got)
    X0 = p.arrays["x0"].copy()
    X0[q] = xk
    m = csh.with_x0(p, X0)
    ze, le, _, _ = ch.HostCondense().expand(m, q, U, v, v)
    assert np.array_equal(z, ze) and np.array_equal(l, le)
    ref, (dz, dl, _) = cah.HostCondenseAdjoint().finish(m, q, (z, l, v), np.zeros(p.nz), None, dU, dv)
    for k in MPC_SEQ:
        assert np.array_equal(got[k], ref[k] + 0.0), k
    assert np.array_equal(got["x0"], 0.0 - dl[:nx])
    untouched = {k: np.full(lens[k], 7.0) for k in MPC_SEQ}
    host().finish(p, q, xk, U, v, dU, dv, untouched, ok=False)
    assert all((a == 7.0).all() for a in untouched.values())


def test_symbols_and_sizes_without_gpu():
    lib = hip_api.load_library()
    for name in ("fbstab_hip_mpc_condensed_receding_sweep_adjoint", "fbstab_hip_mpc_condensed_sweep_adjoint_sizes"):
        assert name in hip_api.EXPORTED_SYMBOLS and getattr(lib, name).argtypes is not None
    from fbstab_amd import condense
    s = condense.condensed_sweep_adjoint_sizes(10, 40, 3, 6)
    f = condense.condensed_sweep_sizes(10, 40, 3, 6)
    assert s["traj_per_group"] == f["traj_per_group"] and s["lds_bytes"] == f["lds_bytes"]
    assert s["work_doubles_per_traj"] == 4 * 33 + 2 * 66 + 2 * 40 + 1
    assert s["work_doubles_per_traj_grad"] == s["work_doubles_per_traj"] + 2 * 11 * 43 + 11 * 40
    with pytest.raises(Exception):
        condense.condensed_sweep_adjoint_sizes(10, 40, 3, 6, traj_per_group=-1)


# ---- the recursion ----------------------------------------------------------------------------------------------------
def fixture_log(name):
    p, A, B, w = csh.setup(name)
    full = csh.oracle_loop(name)
    log = {k: full[k][:sah.SIX] for k in ("u", "x", "U", "v", "eflag")}
    return p, A, B, log


@pytest.mark.parametrize("name", csh.LOOP_FIXTURES)
def test_recursion_m_form_against_the_mpc_form(name):
    """Six steps over the oracle's logs (trajectories retire at steps 0, 3, 4, 4: RETIRES).  At every contributing
    step the chain in longdouble gives (dU, dv, dl) for the seed the MPC-form recursion
    (sweep_adjoint_helpers.reference_sweep_adjoint, table through lr.mpc_gradient_table: x0 entry -dl[0:nx]) hands it;
    the M' form F'(-dU) + G'dv of the same step must agree with -dl[0:nx].
    The bound: both are sums of the same products in exact arithmetic (the identity is linear algebra and holds for
    any (dU, dv)); the M' form reads F and G of ReferenceCondenser.affine(), whose entries are differences of two
    float64 roundings of longdouble images, |dF[e][j]| <= 2^-53 (2 |f0[e]| + 2 |F[e][j]|) and likewise G, so
    |difference[j]| <= 2^-52 sum_e (|f0 b0[e]| + |M[e][j]|) |g[e]|, plus the longdouble sums' own 2^-63 per term
    (taken as another 2^-53 of the same sum: a spare)."""
    p, A, B, log = fixture_log(name)
    assert csh.retirement(csh.oracle_loop(name)["eflag"]) == csh.RETIRES[name]
    N, nx, nu, nc = p.sizes()
    aff = csh.condenser(name).affine()
    rng = np.random.default_rng(11)
    gu, gx = rng.standard_normal((sah.SIX, p.batch, nu)), rng.standard_normal((sah.SIX, p.batch, nx))
    zs, ls = np.zeros((sah.SIX, p.batch, p.nz)), np.zeros((sah.SIX, p.batch, p.nl))
    for k in range(sah.SIX):
        for q in range(p.batch):
            if log["eflag"][k][q] == 0:
                _, (z, l, _) = sah.expanded_point(p, q, log["x"][k][q], log["U"][k][q], log["v"][k][q])
                zs[k, q], ls[k, q] = z, l
    worst = [0.0]
    lens = p.seq_lengths()

    def adjoint_for(q):
        def adjoint_fn(k, x, gz, active):     # (one trajectory: the plants of these fixtures are per trajectory)
            m, xq = sah.expanded_point(p, q, log["x"][k][q], log["U"][k][q], log["v"][k][q])
            c = cah.chain_reference(m, 0, xq, (gz[0], None, None))
            tab = lr.mpc_gradient_table(m, xq, (c["dz"], c["dl"], c["dv"]))
            f0, F, b0, G = (np.asarray(a, dtype=LD) for a in aff[q])
            t = F.T @ (-c["dU"]) + G.T @ c["dv"]
            bound = 3 * sah.U2 * ((np.abs(f0)[:, None] + np.abs(F)).T @ np.abs(c["dU"])
                                  + (np.abs(b0)[:, None] + np.abs(G)).T @ np.abs(c["dv"]))
            err = np.abs(t - (-c["dl"][:nx]))
            assert (err <= bound).all(), (name, k, q, float(err.max()), float(bound.min()))
            worst[0] = max(worst[0], float((err / np.where(bound > 0, bound, 1)).max()))
            return np.zeros(1, dtype=np.int32), {n: tab[n][None] for n in MPC_SEQ}
        return adjoint_fn
    ref = {n: np.zeros((p.batch, lens[n])) for n in MPC_SEQ}
    rstatus, rmu = np.zeros(p.batch, dtype=np.int32), np.zeros((sah.SIX, p.batch, nx))
    for q in range(p.batch):
        mlog = dict(z=zs[:, q:q + 1], l=ls[:, q:q + 1], v=log["v"][:, q:q + 1], eflag=log["eflag"][:, q:q + 1])
        g1, s1, m1 = mah.reference_sweep_adjoint(adjoint_for(q), lr.one_qp(p, q), A[q], B[q], mlog, gu[:, q:q + 1],
                                                 gx[:, q:q + 1])
        for n in MPC_SEQ:
            ref[n][q] = g1[n][0]
        rstatus[q], rmu[:, q] = s1[0], m1[:, 0]
    print("%s: worst per-step |M' form - (-dl0)| / bound = %.3g" % (name, worst[0]))
    # ... and the whole recursion in the M' form lands where the MPC form does (the same bound through six steps of a
    # stable loop: a sanity figure at 1e-9 of the largest entry, not a rounding bound)
    got, gstatus, gmu = sah.reference_condensed_sweep_adjoint(sah.chain_step(p), p, A, B, [(a[1], a[3]) for a in aff],
                                                              log, gu, gx)
    assert np.array_equal(gstatus, rstatus)
    gaps = sah.rel_gaps(got, {k: np.asarray(a, dtype=LD) for k, a in ref.items()})
    print(name, {k: "%.2g" % g for k, g in gaps.items()})
    assert max(gaps.values()) <= 1e-9, gaps
    assert float(np.abs(gmu - rmu).max()) <= 1e-9 * (1 + float(np.abs(rmu).max()))
    for q, k in csh.RETIRES[name].items():
        if k < sah.SIX:
            assert np.array_equal(gmu[k:, q].astype(np.float64), gx[k:, q])   # retired: lambda = 0 behind it


# ---- central differences -------------------------------------------------------------------------------------------
def oracle_condensed_loop(p, A, B, steps, w=None):
    """The oracle's closed loop through the condensed QP of ``p`` (tests/condense_sweep_helpers.py)."""
    from oracle.oracle_py import Oracle, default_options
    orc = Oracle()
    opts = default_options(abs_tol=1e-11)
    rc = csh.ReferenceCondenser(p)
    Ab, Bb = (np.repeat(np.asarray(a)[None], p.batch, axis=0) for a in (A, B))

    def solve(x, U, v):
        z, _, vo, _, out = orc.solve_dense(rc.problem(x), x0guess=(U, np.zeros((p.batch, 0)), v), opts=opts,
                                           raise_on_error=False)
        return z, vo, out
    return csh.condensed_closed_loop(solve, p, Ab, Bb, steps, w=w), rc, Ab, Bb


def test_central_differences_of_the_oracle_loop():
    """h = 1e-5 along q, r, d, x0, a symmetric Q direction and one random direction of w, under
    |fd - ad| <= 1e-4 max(|ad|, 1e-2 sum|grad|) on the strictly complementary trajectories of fd_problem() (seed
    2025): at least 5 of the 8 qualify."""
    p, A, B, cu, cx, dirs = mah.fd_problem()
    N, nx, nu, nc = p.sizes()
    T = mah.FD_STEPS
    log, rc, Ab, Bb = oracle_condensed_loop(p, A, B, T)
    zs = np.zeros((T, p.batch, p.nz))
    for k in range(T):
        for q in range(p.batch):
            zs[k, q] = sah.expanded_point(p, q, log["x"][k][q], log["U"][k][q], log["v"][k][q])[1][0]
    good = mah.strictly_complementary(p, dict(eflag=log["eflag"], x=log["x"], z=zs, v=log["v"]))
    print("strictly complementary:", good)
    assert len(good) >= 5, good
    aff = rc.affine()
    grads, status, mu = sah.reference_condensed_sweep_adjoint(sah.chain_step(p), p, Ab, Bb,
                                                              [(a[1], a[3]) for a in aff], log, cu, cx)
    assert not status.any()
    g64 = {k: a.astype(np.float64) for k, a in grads.items()}

    def run(problem):
        lg = oracle_condensed_loop(problem, A, B, T)[0]
        return lg["u"], np.concatenate([lg["x"][1:], lg["x_end"][None]], 0)
    figures = mah.fd_check(run, g64, good, p, cu, cx, dirs)
    for name, q, fd, ad, bound in figures:
        print("%-2s traj %d: fd %+.6e ad %+.6e bound %.2e" % (name, q, fd, ad, bound))
    for name, q, fd, ad, bound in figures:
        assert abs(fd - ad) <= bound, (name, q, fd, ad, bound)
    # one random direction of w: dL/dw_k = mu_k
    rng = np.random.default_rng(77)
    dw = rng.standard_normal((T, p.batch, nx))
    L = []
    for sg in (1.0, -1.0):
        lg = oracle_condensed_loop(p, A, B, T, w=sg * mah.FD_H * dw)[0]
        x = np.concatenate([lg["x"][1:], lg["x_end"][None]], 0)
        L.append((cu * lg["u"]).sum(axis=(0, 2)) + (cx * x).sum(axis=(0, 2)))
    fd = (L[0] - L[1]) / (2 * mah.FD_H)
    mu64 = mu.astype(np.float64)
    for q in good:
        ad = float((mu64[:, q] * dw[:, q]).sum())
        bound = 1e-4 * max(abs(ad), 1e-2 * np.abs(mu64[:, q]).sum())
        print("w  traj %d: fd %+.6e ad %+.6e bound %.2e" % (q, fd[q], ad, bound))
        assert abs(fd[q] - ad) <= bound, (q, fd[q], ad, bound)
