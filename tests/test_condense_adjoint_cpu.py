"""The adjoint of the condensed MPC route (fbstab_hip_mpc_condensed_adjoint_batch, fb_condense_adjoint.h) without a
GPU: the chain seed -> dense solve -> finish in extended precision against the documented MPC system, the device
logic compiled for one host thread against the rounding rules of tests/condense_helpers.py on the pseudo-data
problem, seeded defects against those rules, and the argument checks of the C-ABI, which run before any device
call."""
import ctypes as C

import numpy as np
import pytest

from tests import condense_adjoint_helpers as cah
from tests import condense_helpers as ch
from tests import linear_reference as lr
from tools import fixtures as fx

LD = ch.LD
SHAPES = ("tiny", "small", "odd33", "flat", "four_wave")


@pytest.fixture(scope="module")
def host():
    return cah.HostCondenseAdjoint()


def _point_and_seeds(p, seed):
    """A point with v >= 0 and random seeds for every QP of ``p`` (the maps are linear: any point serves)."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((p.batch, p.nz)), rng.standard_normal((p.batch, p.nl)),
         np.abs(rng.standard_normal((p.batch, p.nv))))
    return x, lr.random_seeds(rng, p)


# ---- 1. the identity: the chain solves the MPC system up to where sigma sits -------------------------------------
@pytest.mark.parametrize("name", ["tiny", "small", "four_wave", "flat"])
def test_chain_residual_is_sigma_times_the_norm_of_dx_and_dl(name):
    p = ch.problem(name)
    x, seeds = _point_and_seeds(p, 21)
    N, nx, nu, nc = p.sizes()
    sigma = 1e-8
    for q in range(p.batch):
        xq, sq = tuple(t[q] for t in x), tuple(t[q] for t in seeds)
        assert all(np.abs(s).max() > 0 for s in sq)
        c = cah.chain_reference(p, q, xq, sq, sigma)
        res = lr.adjoint_residual(p, q, xq, (c["dz"], c["dl"], c["dv"]), sq, sigma=sigma)
        dx = c["dz"].reshape(N + 1, nx + nu)[:, :nx]
        pred = float(LD(sigma) * np.sqrt((dx * dx).sum() + (c["dl"] * c["dl"]).sum()))
        print(name, q, "residual", res, "sigma ||(dx, dl)||", pred, "ratio", res / pred)
        assert abs(res / pred - 1.0) <= 1e-6, (q, res, pred)


# ---- 2, 3, 4, 5. the device logic on the host --------------------------------------------------------------------
@pytest.mark.parametrize("name", SHAPES)
def test_host_build_of_the_seed_map_meets_the_condense_rule(host, name):
    p = ch.problem(name)
    x, (gz, gl, gv) = _point_and_seeds(p, 22)
    pp = cah.pseudo_problem(p, gz, gl, gv)
    for q in range(p.batch):
        ch.assert_condition(pp, q)
        U, gU, gvc = host.seed(p, q, x[0][q], gz[q], gl[q], gv[q])
        assert U.tobytes() == ch.u_of(p, x[0][q:q + 1])[0].tobytes()
        assert cah.seed_violations(gU, gvc, pp, q) == []


@pytest.mark.parametrize("name", SHAPES)
def test_host_build_of_the_finish_sweeps_meets_the_expand_rule_and_the_table(host, name):
    p = ch.problem(name)
    x, (gz, gl, gv) = _point_and_seeds(p, 23)
    pp = cah.pseudo_problem(p, gz, gl, gv)
    rng = np.random.default_rng(24)
    for q in range(p.batch):
        dU, dv = rng.standard_normal((p.N + 1) * p.nu), rng.standard_normal(p.nv)
        xq = tuple(t[q] for t in x)
        grads, (dz, dl, dvo) = host.finish(p, q, xq, gz[q], gl[q], dU, dv)
        assert cah.finish_violations(dz, dl, pp, q, dU, dv) == []
        assert dvo.tobytes() == dv.tobytes()
        assert ch.u_of(p, dz[None])[0].tobytes() == dU.tobytes()
        # the gradients: the table of the returned step, the existing rule
        tab = lr.mpc_gradient_table(p, xq, (dz, dl, dvo))
        scale = max(np.abs(np.concatenate((dz, dl, dvo))).max(), 1.0) * max(np.abs(np.concatenate(xq)).max(), 1.0)
        for k in cah.MPC_NAMES:
            np.testing.assert_allclose(grads[k], tab[k], rtol=1e-13, atol=1e-15 * scale, err_msg=k)
        # a subset of the slots: the same bits, the others untouched; a failed factorisation: zeros everywhere
        some, _ = host.finish(p, q, xq, gz[q], gl[q], dU, dv, want=("A", "x0", "E"))
        assert all(some[k].tobytes() == grads[k].tobytes() for k in some)
        zero, adj0 = host.finish(p, q, xq, gz[q], gl[q], dU, dv, ok=False)
        assert all((g == 0).all() for g in zero.values()) and all((a == 0).all() for a in adj0)


@pytest.mark.parametrize("name", ["small", "odd33"])
def test_null_seeds_are_zero_seeds_bit_for_bit(host, name):
    p = ch.problem(name)
    x, (gz, gl, gv) = _point_and_seeds(p, 25)
    rng = np.random.default_rng(26)
    q = 1
    xq = tuple(t[q] for t in x)
    zl, zv = np.zeros(p.nl), np.zeros(p.nv)
    for a, b in (((None, gv[q]), (zl, gv[q])), ((gl[q], None), (gl[q], zv)), ((None, None), (zl, zv))):
        got, want = host.seed(p, q, xq[0], gz[q], *a), host.seed(p, q, xq[0], gz[q], *b)
        assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want))
    dU, dv = rng.standard_normal((p.N + 1) * p.nu), rng.standard_normal(p.nv)
    g0, a0 = host.finish(p, q, xq, gz[q], None, dU, dv)
    g1, a1 = host.finish(p, q, xq, gz[q], zl, dU, dv)
    assert all(g0[k].tobytes() == g1[k].tobytes() for k in g0)
    assert all(s.tobytes() == t.tobytes() for s, t in zip(a0, a1))


# ---- 6. the rules catch seeded defects -----------------------------------------------------------------------------
def _s_transposed(p):
    """``p`` with the nu x nx column-major images of S read as nx x nu ones."""
    N, nx, nu, nc = p.sizes()
    S = p.arrays["S"].reshape(p.batch, N + 1, nx, nu)
    arrays = {k: a.copy() for k, a in p.arrays.items()}
    arrays["S"] = np.ascontiguousarray(S.reshape(p.batch, N + 1, nu, nx).transpose(0, 1, 3, 2)).reshape(p.batch, -1)
    return fx.MpcProblem(N, nx, nu, nc, arrays)


@pytest.mark.parametrize("defect", ["gl_dropped", "gvc_sign_flipped", "S_transposed_in_dl", "gl0_not_in_dx0"])
def test_rules_catch_seeded_defects(host, defect):
    caught = []
    names = [n for n in SHAPES if not (defect == "S_transposed_in_dl" and n == "tiny")]   # (a 1 x 1 S is its transpose)
    for name in names:
        p = ch.problem(name)
        x, (gz, gl, gv) = _point_and_seeds(p, 27)
        pp = cah.pseudo_problem(p, gz, gl, gv)
        q = 0
        rng = np.random.default_rng(28)
        dU, dv = rng.standard_normal((p.N + 1) * p.nu), rng.standard_normal(p.nv)
        # the correct maps pass
        _, gU, gvc = host.seed(p, q, x[0][q], gz[q], gl[q], gv[q])
        assert cah.seed_violations(gU, gvc, pp, q) == []
        _, (dz, dl, _) = host.finish(p, q, tuple(t[q] for t in x), gz[q], gl[q], dU, dv)
        assert cah.finish_violations(dz, dl, pp, q, dU, dv) == []
        if defect == "gl_dropped":
            _, bU, bvc = host.seed(p, q, x[0][q], gz[q], None, gv[q])
            bad = cah.seed_violations(bU, bvc, pp, q)
        elif defect == "gvc_sign_flipped":
            bad = cah.seed_violations(gU, -gvc, pp, q)
        elif defect == "S_transposed_in_dl":
            _, (bz, bl, _) = host.finish(_s_transposed(p), q, tuple(t[q] for t in x), gz[q], gl[q], dU, dv)
            bad = cah.finish_violations(bz, bl, pp, q, dU, dv)
            assert "dz" not in bad       # (S enters the dl recursion alone)
        else:
            gl0 = gl[q].copy()
            gl0[:p.nx] = 0.0
            _, (bz, bl, _) = host.finish(p, q, tuple(t[q] for t in x), gz[q], gl0, dU, dv)
            bad = cah.finish_violations(bz, bl, pp, q, dU, dv)
        if bad:
            caught.append(name)
    print(defect, "caught on", caught)
    assert caught == names, (defect, caught)


# ---- 7. the C-ABI without a GPU -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from fbstab_amd import hip_api
    return hip_api.load_library()


class _Call:
    """fbstab_hip_mpc_condensed_adjoint_batch on valid arguments for (2, 3, 2, 2), batch 2, but for the handle (there is
    none without a device); the pointers are never followed before the device check."""
    N, nx, nu, nc = 2, 3, 2, 2

    def __init__(self):
        from fbstab_amd import hip_api
        self.buf = np.zeros(4096)
        self.st = np.zeros(8, dtype=np.int32)
        n1, N, nx, nu, nc = self.N + 1, self.N, self.nx, self.nu, self.nc
        at = self.buf.ctypes.data
        self.len = [n1 * nx * nx, n1 * nu * nu, n1 * nu * nx, n1 * nx, n1 * nu, N * nx * nx, N * nx * nu, N * nx,
                    n1 * nc * nx, n1 * nc * nu, n1 * nc, nx]
        self.data, self.grad = hip_api._MpcBatch(), hip_api._MpcGradBatch()
        for i, n in enumerate(self.len):
            self.data.base[i], self.data.stride[i] = at, n
            self.grad.base[i], self.grad.stride[i] = at, n
        nz, nv = n1 * nu, n1 * nc
        self.dlen = [nz * nz, nz, 0, 0, nv * nz, nv]
        self.dense = hip_api._DenseBatch()
        for i, n in enumerate(self.dlen):
            if n:
                self.dense.base[i], self.dense.stride[i] = at, n
        self.xlen = [n1 * (nx + nu), n1 * nx, nv]
        self.x, self.seed, self.adj = hip_api._VarBatch(), hip_api._VarBatch(), hip_api._VarBatch()
        for blk in (self.x, self.seed, self.adj):
            for i, n in enumerate(self.xlen):
                blk.base[i], blk.stride[i] = at, n
        self.sizes = [self.N, self.nx, self.nu, self.nc]
        self.batch, self.handle = 2, None
        self.work, self.status = at, self.st.ctypes.data
        self.null = ()

    def _ref(self, name):
        return None if name in self.null else C.byref(getattr(self, name))

    def __call__(self, lib):
        rc = lib.fbstab_hip_mpc_condensed_adjoint_batch(
            self.handle, *self.sizes, self.batch, self._ref("data"), self._ref("dense"), self._ref("x"),
            self._ref("seed"), C.c_double(0.0), self._ref("grad"), self._ref("adj"),
            None if "work" in self.null else C.c_void_p(self.work),
            None if "status" in self.null else C.c_void_p(self.status), None)
        return rc, lib.fbstab_hip_last_error().decode()


def _bad_cases():
    """name -> (what to break, a word of the message that names the check)."""
    def size(i):
        def f(c): c.sizes[i] = 0
        return f
    cases = {f"{n}_zero": (size(i), "sizes") for i, n in enumerate(("N", "nx", "nu", "nc"))}
    cases["negative_batch"] = (lambda c: setattr(c, "batch", -1), "negative batch")
    for blk in ("data", "dense", "x", "seed", "grad", "work", "status"):
        cases[f"null_{blk}"] = (lambda c, b=blk: setattr(c, "null", (b,)), "null")
    cases["null_data_pointer"] = (lambda c: c.data.base.__setitem__(5, None), "null problem data pointer")
    cases["short_data_stride"] = (lambda c: c.data.stride.__setitem__(0, c.len[0] - 1), "problem data stride")
    cases["negative_data_stride"] = (lambda c: c.data.stride.__setitem__(11, -3), "problem data stride")
    cases["null_H"] = (lambda c: c.dense.base.__setitem__(0, None), "condensed images")
    cases["null_b"] = (lambda c: c.dense.base.__setitem__(5, None), "condensed images")
    cases["short_H_stride"] = (lambda c: c.dense.stride.__setitem__(0, c.dlen[0] - 1), "condensed image")
    cases["f_stride_0"] = (lambda c: c.dense.stride.__setitem__(1, 0), "condensed image")
    cases["b_stride_short"] = (lambda c: c.dense.stride.__setitem__(5, c.dlen[5] - 1), "condensed image")
    cases["null_z"] = (lambda c: c.x.base.__setitem__(0, None), "null variable pointer")
    cases["null_l"] = (lambda c: c.x.base.__setitem__(1, None), "null variable pointer")
    cases["null_v"] = (lambda c: c.x.base.__setitem__(2, None), "null variable pointer")
    cases["null_gz"] = (lambda c: c.seed.base.__setitem__(0, None), "null seed pointer")
    cases["short_z_stride"] = (lambda c: c.x.stride.__setitem__(0, c.xlen[0] - 1), "variable stride")
    cases["short_gl_stride"] = (lambda c: c.seed.stride.__setitem__(1, 0), "seed stride")
    cases["short_dv_stride"] = (lambda c: c.adj.stride.__setitem__(2, c.xlen[2] - 1), "adjoint stride")
    cases["short_grad_stride"] = (lambda c: c.grad.stride.__setitem__(5, c.len[5] - 1), "gradient stride")
    cases["grad_stride_0"] = (lambda c: c.grad.stride.__setitem__(0, 0), "gradient stride")
    return cases


def test_entry_point_is_exported_and_bound(lib):
    from fbstab_amd import hip_api
    assert "fbstab_hip_mpc_condensed_adjoint_batch" in hip_api.EXPORTED_SYMBOLS
    assert len(lib.fbstab_hip_mpc_condensed_adjoint_batch.argtypes) == 16


@pytest.mark.parametrize("case", sorted(_bad_cases()))
def test_bad_arguments_are_refused_before_any_device_call(lib, case):
    breaker, word = _bad_cases()[case]
    c = _Call()
    breaker(c)
    rc, msg = c(lib)
    assert rc == 1 and word in msg, (rc, msg)


def test_valid_arguments_reach_the_handle_check(lib):
    # what needs no handle is checked first: valid blocks are stopped by the missing handle, and by nothing before
    for breaker in (lambda c: None,
                    lambda c: setattr(c, "batch", 0),
                    lambda c: setattr(c, "null", ("adj",)),                                   # adj is optional
                    lambda c: (c.seed.base.__setitem__(1, None), c.seed.base.__setitem__(2, None)),   # and so are gl, gv
                    lambda c: [c.grad.base.__setitem__(i, None) for i in range(12)],
                    lambda c: (c.dense.stride.__setitem__(0, 0), c.dense.stride.__setitem__(4, 0)),   # one H_c, A_c image
                    lambda c: [c.data.stride.__setitem__(i, 0) for i in range(12)],
                    lambda c: (setattr(c, "batch", 1), c.x.stride.__setitem__(0, 0))):         # batch 1: strides unread
        c = _Call()
        breaker(c)
        rc, msg = c(lib)
        assert rc == 1 and "null dense solver handle" in msg, (rc, msg)


# ---- the refinement step of the dense adjoint ------------------------------------------------------------------------
def _reduced_solve(Hc, Ac, Cg, mus, sigma, gU, gvc):
    """V_c (dU, dv) = (gU, -C gv_c) the way the dense adjoint solves it, in double: dv eliminated, K = H_c + sigma I +
    A_c' Gamma A_c factored, dv recovered from dU."""
    gam = Cg / mus
    K = Hc + sigma * np.eye(len(gU)) + Ac.T @ (gam[:, None] * Ac)
    dU = np.linalg.solve(K, gU + Ac.T @ (gam * gvc))
    return dU, gam * (Ac @ dU - gvc)


@pytest.mark.parametrize("nzc,nv", [(2, 2), (9, 66), (72, 36)])
def test_host_build_of_the_refinement_step(host, nzc, nv):
    """condense_adjoint_residual within the rounding of its nzc + nv + 1 terms of the longdouble z rows' residual, and
    one step (residual, the same reduced solve, condense_adjoint_correct) takes the residual of a system with active
    rows (mus = sigma C: Gamma = 1 / sigma) from eps / sigma down by 1e3 at the least: what is left is eps / sigma of
    a correction that is 1e-6 of the step or less."""
    rng = np.random.default_rng(31 + nzc)
    sigma = 1e-8
    M = rng.standard_normal((nzc, nzc))
    Hc = M @ M.T / nzc + 0.1 * np.eye(nzc)
    Ac = rng.standard_normal((nv, nzc))
    act = np.arange(nv) < min(nzc - 1, nv // 2)
    Cg = np.where(act, 0.95, 1e-3) * (1 + 0.01 * rng.random(nv))
    mus = np.where(act, sigma * Cg, 1.0)
    gU, gvc = 100 * rng.standard_normal(nzc), rng.standard_normal(nv)

    def residual_norm(dU, dv):
        e1 = Hc.astype(LD) @ dU.astype(LD) + LD(sigma) * dU + Ac.T.astype(LD) @ dv.astype(LD) - gU
        e3 = -Cg.astype(LD) * (Ac.astype(LD) @ dU.astype(LD)) + mus.astype(LD) * dv + Cg.astype(LD) * gvc
        return e1, float(np.sqrt((e1 * e1).sum() + (e3 * e3).sum()))

    dU, dv = _reduced_solve(Hc, Ac, Cg, mus, sigma, gU, gvc)
    e1, before = residual_norm(dU, dv)
    rU = host.residual(Hc, Ac, sigma, gU, dU, dv)
    mag = np.abs(gU) + np.abs(Hc) @ np.abs(dU) + sigma * np.abs(dU) + np.abs(Ac.T) @ np.abs(dv)
    assert (np.abs(rU.astype(LD) + e1) <= (nzc + nv + 2) * 2.0 ** -53 * mag).all()
    eU, ev = _reduced_solve(Hc, Ac, Cg, mus, sigma, rU, np.zeros(nv))
    dU2, dv2 = host.correct(eU, ev, dU, dv)
    assert dU2.tobytes() == (dU + eU).tobytes() and dv2.tobytes() == (dv + ev).tobytes()
    _, after = residual_norm(dU2, dv2)
    print(nzc, nv, "residual before", before, "after", after)
    assert before > 0 and after <= 1e-3 * before, (before, after)
