"""Many right-hand sides on the condensed MPC route (fbstab_hip_mpc_condensed_kkt_solve_batch,
fbstab_hip_mpc_condensed_x0_sensitivity_batch, fb_condense_multi.h) without a GPU: the symbols and the argument
checks of the C-ABI, which run before any device call, the size query against its documented formulas, the device
logic compiled for one host thread against the rounding rules of tests/condense_helpers.py on each right-hand
side's own pseudo-data problem and bit for bit across groupings, seeded defects against those rules, and the x0
chain in extended precision against a known answer and the MPC system."""
import ctypes as C

import numpy as np
import pytest

from tests import condense_adjoint_helpers as cah
from tests import condense_helpers as ch
from tests import condense_multi_helpers as cmh
from tests import helpers as H
from tests import linear_reference as lr
from tools import fixtures as fx

LD = ch.LD
HOST_SHAPES = ("small", "odd33", "flat")
NRHS = 5


@pytest.fixture(scope="module")
def lib():
    from fbstab_amd import hip_api
    return hip_api.load_library()


@pytest.fixture(scope="module")
def host():
    return cmh.HostCondenseMulti()


# ---- 1. the C-ABI without a GPU ------------------------------------------------------------------------------------
class _Call:
    """The two entries on valid arguments for (2, 3, 2, 2), batch 2, nrhs 3 (x0 mode: nx = 3), but for the handle
    (there is none without a device); the pointers are never followed before the device check."""
    N, nx, nu, nc = 2, 3, 2, 2

    def __init__(self, x0=False):
        from fbstab_amd import hip_api
        self.x0 = x0
        self.buf = np.zeros(4096)
        self.st = np.zeros(8, dtype=np.int32)
        n1, N, nx, nu, nc = self.N + 1, self.N, self.nx, self.nu, self.nc
        at = self.buf.ctypes.data
        self.len = [n1 * nx * nx, n1 * nu * nu, n1 * nu * nx, n1 * nx, n1 * nu, N * nx * nx, N * nx * nu, N * nx,
                    n1 * nc * nx, n1 * nc * nu, n1 * nc, nx]
        self.data = hip_api._MpcBatch()
        for i, n in enumerate(self.len):
            self.data.base[i], self.data.stride[i] = at, n
        nz, nv = n1 * nu, n1 * nc
        self.dlen = [nz * nz, nz, 0, 0, nv * nz, nv]
        self.dense = hip_api._DenseBatch()
        for i, n in enumerate(self.dlen):
            if n:
                self.dense.base[i], self.dense.stride[i] = at, n
        self.xlen = [n1 * (nx + nu), n1 * nx, nv]
        self.x = hip_api._VarBatch()
        self.nrhs = 3
        self.seed, self.step = hip_api._MultiVarBatch(), hip_api._MultiVarBatch()
        for i, n in enumerate(self.xlen):
            self.x.base[i], self.x.stride[i] = at, n
            for blk in (self.seed, self.step):
                blk.base[i], blk.rhs_stride[i], blk.stride[i] = at, n, self.nrhs * n
        self.sizes = [self.N, self.nx, self.nu, self.nc]
        self.batch, self.handle = 2, None
        self.work, self.status, self.gain = at, self.st.ctypes.data, at
        self.gain_stride, self.rpg = nu * nx, 0
        self.null = ()

    def _ref(self, name):
        return None if name in self.null else C.byref(getattr(self, name))

    def _ptr(self, name):
        return None if name in self.null else C.c_void_p(getattr(self, name))

    def __call__(self, lib):
        head = (self.handle, *self.sizes, self.batch, self._ref("data"), self._ref("dense"), self._ref("x"))
        tail = (self.rpg, self._ptr("work"), self._ptr("status"), None)
        if self.x0:
            rc = lib.fbstab_hip_mpc_condensed_x0_sensitivity_batch(*head, C.c_double(0.0), self._ref("step"),
                                                                   self._ptr("gain"), self.gain_stride, *tail)
        else:
            rc = lib.fbstab_hip_mpc_condensed_kkt_solve_batch(*head, self.nrhs, self._ref("seed"), C.c_double(0.0),
                                                              self._ref("step"), *tail)
        return rc, lib.fbstab_hip_last_error().decode()


def _bad_cases():
    """name -> (x0 mode?, what to break, a word of the message that names the check): one case per rule."""
    cases = {}
    cases["nrhs_zero"] = (False, lambda c: setattr(c, "nrhs", 0), "fewer than one right-hand side")
    cases["null_z_seed"] = (False, lambda c: c.seed.base.__setitem__(0, None), "null seed pointer")
    cases["short_seed_rhs_stride"] = (False, lambda c: c.seed.rhs_stride.__setitem__(1, c.xlen[1] - 1), "seed rhs_stride")
    cases["short_step_rhs_stride"] = (False, lambda c: c.step.rhs_stride.__setitem__(0, c.xlen[0] - 1), "step rhs_stride")
    cases["short_seed_stride"] = (False, lambda c: c.seed.stride.__setitem__(2, 3 * c.xlen[2] - 1), "seed stride")
    cases["short_step_stride"] = (False, lambda c: c.step.stride.__setitem__(0, 3 * c.xlen[0] - 1), "step stride")
    cases["step_stride_0"] = (False, lambda c: c.step.stride.__setitem__(1, 0), "step stride")
    cases["null_work"] = (False, lambda c: setattr(c, "null", ("work",)), "null")
    cases["null_status"] = (False, lambda c: setattr(c, "null", ("status",)), "null")
    cases["null_work_x0"] = (True, lambda c: setattr(c, "null", ("work",)), "null")
    cases["null_step_block"] = (False, lambda c: setattr(c, "null", ("step",)), "null seed or step block")
    cases["null_seed_block"] = (False, lambda c: setattr(c, "null", ("seed",)), "null seed or step block")
    cases["short_gain_stride"] = (True, lambda c: setattr(c, "gain_stride", c.nu * c.nx - 1), "gain stride")
    cases["negative_rhs_per_group"] = (False, lambda c: setattr(c, "rpg", -1), "negative rhs_per_group")
    cases["negative_rhs_per_group_x0"] = (True, lambda c: setattr(c, "rpg", -2), "negative rhs_per_group")
    cases["step_and_gain_null_x0"] = (True, lambda c: setattr(c, "null", ("step", "gain")), "both step and gain")
    cases["short_step_stride_x0"] = (True, lambda c: c.step.stride.__setitem__(0, 3 * c.xlen[0] - 1), "step stride")
    cases["nx_zero"] = (True, lambda c: c.sizes.__setitem__(1, 0), "sizes")
    cases["null_H"] = (False, lambda c: c.dense.base.__setitem__(0, None), "condensed images")
    cases["short_z_stride"] = (True, lambda c: c.x.stride.__setitem__(0, c.xlen[0] - 1), "variable stride")
    return cases


def test_entry_points_are_exported_and_bound(lib):
    from fbstab_amd import hip_api
    for name, nargs in (("fbstab_hip_mpc_condensed_multi_sizes", 9), ("fbstab_hip_mpc_condensed_kkt_solve_batch", 17),
                        ("fbstab_hip_mpc_condensed_x0_sensitivity_batch", 17)):
        assert name in hip_api.EXPORTED_SYMBOLS
        assert len(getattr(lib, name).argtypes) == nargs


@pytest.mark.parametrize("case", sorted(_bad_cases()))
def test_bad_arguments_are_refused_before_any_device_call(lib, case):
    x0, breaker, word = _bad_cases()[case]
    c = _Call(x0)
    breaker(c)
    rc, msg = c(lib)
    assert rc == 1 and word in msg, (rc, msg)


def test_valid_arguments_reach_the_handle_check(lib):
    # what needs no handle is checked first: valid blocks are stopped by the missing handle, and by nothing before
    def shared_seed(c):
        c.seed.stride[0] = 0

    def batch_one(c):
        c.batch = 1
        c.seed.stride[0] = c.step.stride[1] = 0

    def one_rhs(c):
        c.nrhs = 1
        for i in range(3):
            c.seed.rhs_stride[i] = c.step.rhs_stride[i] = 0
            c.seed.stride[i] = c.step.stride[i] = c.xlen[i]

    for x0, breaker in ((False, lambda c: None), (True, lambda c: None),
                        (False, lambda c: setattr(c, "batch", 0)),
                        (False, lambda c: (c.seed.base.__setitem__(1, None), c.seed.base.__setitem__(2, None))),
                        (False, lambda c: [c.step.base.__setitem__(i, None) for i in range(3)]),
                        (False, shared_seed), (False, batch_one), (False, one_rhs),
                        (False, lambda c: setattr(c, "rpg", 7)),
                        (True, lambda c: setattr(c, "null", ("step",))),           # gain alone
                        (True, lambda c: setattr(c, "null", ("gain",))),           # the step alone
                        (True, lambda c: (setattr(c, "batch", 1), setattr(c, "gain_stride", 0))),
                        (False, lambda c: (c.dense.stride.__setitem__(0, 0), c.dense.stride.__setitem__(4, 0)))):
        c = _Call(x0)
        breaker(c)
        rc, msg = c(lib)
        assert rc == 1 and "null dense solver handle" in msg, (rc, msg)


# ---- 2. the size query ---------------------------------------------------------------------------------------------
def _shapes():
    return [next(s[1] for s in ch.SHAPES if s[0] == n) for n in ("tiny", "small", "odd33", "flat", "four_wave")] + [
        (10, 40, 3, 6), (15, 12, 4, 20)]


@pytest.mark.parametrize("shape", _shapes())
def test_sizes_follow_the_documented_formulas(lib, host, shape):
    from fbstab_amd.condense import condensed_multi_sizes, condensed_sizes
    N, nx, nu, nc = shape
    for nrhs in (1, 5, nx, 300):
        for R in (0, 1, 2, 7):
            got = condensed_multi_sizes(N, nx, nu, nc, nrhs, R)
            want = cmh.sizes_formula(N, nx, nu, nc, nrhs, R)
            assert got == {k: want[k] for k in got}, (nrhs, R, got, want)
            assert 1 <= got["rhs_per_group"] <= nrhs
            if R == 0:
                assert got["lds_bytes"] <= 80 * 1024 or got["rhs_per_group"] == 1
        hs = host.sizes(N, nx, nu, nc, nrhs)     # the header's own functions
        want = cmh.sizes_formula(N, nx, nu, nc, nrhs)
        assert (hs["per"], hs["window"], hs["rule"]) == (want["per"], want["window"], want["rhs_per_group"])
    # the stage window is that of fbstab_hip_mpc_condensed_sizes: its lds_bytes less its carry
    carry = max((N + 2) * cmh._e((nx | 1) * nu), (N + 1) * (nx + nu + nc) + 2 * nx + 8)
    assert condensed_sizes(N, nx, nu, nc)["lds_bytes"] == 8 * (want["window"] + cmh._e(carry))


def test_the_rule_on_the_headline_shape(lib):
    from fbstab_amd.condense import condensed_multi_sizes
    got = condensed_multi_sizes(10, 40, 3, 6, 40)
    assert got["rhs_per_group"] == 6 and got["lds_bytes"] == 8 * (3836 + 6 * 620)
    assert condensed_multi_sizes(2, 33, 3, 1, 33)["rhs_per_group"] == 7    # odd33: groups of 7, a last one of 5


def test_sizes_refuse_bad_arguments_and_lds_above_160_kb(lib):
    used, lds, work = C.c_int(-1), C.c_longlong(-1), C.c_longlong(-1)
    out = (C.byref(used), C.byref(lds), C.byref(work))
    f = lib.fbstab_hip_mpc_condensed_multi_sizes
    for args in ((0, 3, 2, 2, 3, 0), (2, 3, 2, 0, 3, 0), (2, 3, 2, 2, 0, 0), (2, 3, 2, 2, 3, -1)):
        assert f(*args, *out) == 1, args
        assert (used.value, lds.value, work.value) == (0, 0, 0)
    # (10, 40, 3, 6): 620 doubles per right-hand side behind a window of 3836: 26 of them fit 20480 doubles, 27 do not
    want = cmh.sizes_formula(10, 40, 3, 6, 40, 27)
    assert want["lds_bytes"] > 160 * 1024 >= cmh.sizes_formula(10, 40, 3, 6, 40, 26)["lds_bytes"]
    assert f(10, 40, 3, 6, 40, 27, *out) == 3 and "LDS" in lib.fbstab_hip_last_error().decode()
    assert (used.value, lds.value, work.value) == (0, 0, 0)
    assert f(10, 40, 3, 6, 40, 26, *out) == 0 and used.value == 26
    assert f(10, 40, 3, 6, 40, 26, None, None, None) == 0          # output pointers may be NULL
    assert f(10, 40, 3, 6, 5, 27, *out) == 0 and used.value == 5   # (a value above nrhs is nrhs)


# ---- 3. the device logic on the host -------------------------------------------------------------------------------
def _point_and_seeds(p, seed, nrhs=NRHS):
    """A point with v >= 0 for every QP of ``p`` and ``nrhs`` random seeds per QP, all three parts non-zero."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((p.batch, p.nz)), rng.standard_normal((p.batch, p.nl)),
         np.abs(rng.standard_normal((p.batch, p.nv))))
    seeds = tuple(rng.standard_normal((p.batch, nrhs, n)) for n in (p.nz, p.nl, p.nv))
    return x, seeds


def _dense_steps(p, nrhs, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((nrhs, (p.N + 1) * p.nu)), rng.standard_normal((nrhs, p.nv))


@pytest.mark.parametrize("name", HOST_SHAPES)
def test_host_build_of_the_multi_seed_map(host, name):
    p = ch.problem(name)
    x, seeds = _point_and_seeds(p, 61)
    for q in (0, p.batch - 1):
        sq = tuple(s[q] for s in seeds)
        runs = {R: host.seed(p, q, x[0][q], sq, NRHS, R) for R in (1, 2, 5)}
        U, gU, gvc = runs[5]
        assert U.tobytes() == ch.u_of(p, x[0][q:q + 1])[0].tobytes()
        for k in range(NRHS):
            pp = cmh.slot_problem(p, q, sq, k)
            ch.assert_condition(pp, 0)
            assert cah.seed_violations(gU[k], gvc[k], pp, 0) == [], (q, k)
        # a slot's bits: the same for every R (R = 2 leaves a partial last group) ...
        for R in (1, 2):
            assert all(a.tobytes() == b.tobytes() for a, b in zip(runs[R], runs[5])), R
        # ... in any slot position and beside any other seeds
        perm = np.array([3, 0, 4, 2, 1])
        _, pU, pv = host.seed(p, q, x[0][q], tuple(s[perm] for s in sq), NRHS, 2)
        assert pU.tobytes() == gU[perm].tobytes() and pv.tobytes() == gvc[perm].tobytes()
        _, aU, av = host.seed(p, q, x[0][q], tuple(s[3:4] for s in sq), 1, 1)
        assert aU.tobytes() == gU[3:4].tobytes() and av.tobytes() == gvc[3:4].tobytes()
        # NULL gl / gv are bitwise zero arrays
        zl, zv = np.zeros_like(sq[1]), np.zeros_like(sq[2])
        for a, b in (((None, sq[2]), (zl, sq[2])), ((sq[1], None), (sq[1], zv)), ((None, None), (zl, zv))):
            got, want = host.seed(p, q, x[0][q], (sq[0],) + a, NRHS, 2), host.seed(p, q, x[0][q], (sq[0],) + b, NRHS, 2)
            assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want))


@pytest.mark.parametrize("name", HOST_SHAPES)
def test_host_build_of_the_multi_finish_map(host, name):
    p = ch.problem(name)
    x, seeds = _point_and_seeds(p, 62)
    for q in (0, p.batch - 1):
        sq = tuple(s[q] for s in seeds)
        dU, dv = _dense_steps(p, NRHS, 63 + q)
        runs = {R: host.finish(p, q, sq, dU, dv, R) for R in (1, 2, 5)}
        r5 = runs[5]
        for k in range(NRHS):
            pp = cmh.slot_problem(p, q, sq, k)
            assert cah.finish_violations(r5["dz"][k], r5["dl"][k], pp, 0, dU[k], dv[k]) == [], (q, k)
            assert ch.u_of(p, r5["dz"][k][None])[0].tobytes() == dU[k].tobytes()
        assert r5["dv"].tobytes() == dv.tobytes()
        for R in (1, 2):
            assert all(runs[R][n].tobytes() == r5[n].tobytes() for n in r5), R
        perm = np.array([3, 0, 4, 2, 1])
        pr = host.finish(p, q, tuple(s[perm] for s in sq), dU[perm], dv[perm], 2)
        assert all(pr[n].tobytes() == r5[n][perm].tobytes() for n in r5)
        al = host.finish(p, q, tuple(s[3:4] for s in sq), dU[3:4], dv[3:4], 1)
        assert all(al[n].tobytes() == r5[n][3:4].tobytes() for n in r5)
        # a NULL gl is a zero array (gv is not read); NULL step slots are skipped; a failed factorisation: zeros
        n0 = host.finish(p, q, (sq[0], None, None), dU, dv, 2)
        z0 = host.finish(p, q, (sq[0], np.zeros_like(sq[1]), sq[2]), dU, dv, 2)
        assert all(n0[n].tobytes() == z0[n].tobytes() for n in n0)
        some = host.finish(p, q, sq, dU, dv, 2, want=("dz",))
        assert set(some) == {"dz"} and some["dz"].tobytes() == r5["dz"].tobytes()
        some = host.finish(p, q, sq, dU, dv, 2, want=("dl",))
        assert set(some) == {"dl"} and some["dl"].tobytes() == r5["dl"].tobytes()
        zero = host.finish(p, q, sq, dU, dv, 2, ok=False)
        assert all((zero[n] == 0).all() for n in zero)


@pytest.mark.parametrize("name", HOST_SHAPES)
def test_x0_mode_is_the_explicit_unit_seeds_bit_for_bit(host, name):
    p = ch.problem(name)
    x, _ = _point_and_seeds(p, 64)
    unit = cmh.x0_seeds(p)
    q = 1
    dU, dv = _dense_steps(p, p.nx, 65)
    for R in (1, 2, p.nx):
        a, b = host.seed(p, q, x[0][q], None, p.nx, R), host.seed(p, q, x[0][q], unit, p.nx, R)
        assert all(s.tobytes() == t.tobytes() for s, t in zip(a, b)), R
        fa, fb = host.finish(p, q, None, dU, dv, R), host.finish(p, q, unit, dU, dv, R)
        assert all(fa[n].tobytes() == fb[n].tobytes() for n in fa), R
    # ... and they meet the rules on the pseudo-data problem x0 := e_j (columns 0, a middle one, nx - 1)
    for j in (0, p.nx // 2, p.nx - 1):
        pp = cmh.slot_problem(p, q, unit, j)
        assert cah.seed_violations(a[1][j], a[2][j], pp, 0) == [], j
        assert cah.finish_violations(fa["dz"][j], fa["dl"][j], pp, 0, dU[j], dv[j]) == [], j


@pytest.mark.parametrize("nzc,nv", [(2, 2), (9, 66), (72, 36)])
def test_host_build_of_the_multi_refinement_step(host, nzc, nv):
    """condense_multi_residual within the rounding of its nzc + nv + 1 terms of the longdouble residual for every
    right-hand side, the same bits for every grouping; condense_multi_correct is the sum, and the gain its first nu
    rows."""
    rng = np.random.default_rng(66 + nzc)
    sigma, nu = 1e-8, 2
    Hc, Ac = rng.standard_normal((nzc, nzc)), rng.standard_normal((nv, nzc))
    gU, dU, dv = (rng.standard_normal((NRHS, n)) for n in (nzc, nzc, nv))
    runs = {R: host.residual(Hc, Ac, sigma, gU, dU, dv, R) for R in (1, 2, 5)}
    assert runs[1].tobytes() == runs[5].tobytes() and runs[2].tobytes() == runs[5].tobytes()
    for k in range(NRHS):
        ref = gU[k] - (Hc.astype(LD) @ dU[k].astype(LD) + LD(sigma) * dU[k] + Ac.T.astype(LD) @ dv[k].astype(LD))
        mag = np.abs(gU[k]) + np.abs(Hc) @ np.abs(dU[k]) + sigma * np.abs(dU[k]) + np.abs(Ac.T) @ np.abs(dv[k])
        assert (np.abs(runs[5][k].astype(LD) - ref) <= (nzc + nv + 2) * 2.0 ** -53 * mag).all(), k
    eU, ev = rng.standard_normal((NRHS, nzc)), rng.standard_normal((NRHS, nv))
    for R in (1, 2, 5):
        sU, sv, g = host.correct(eU, ev, dU, dv, R, nu, gain=True)
        assert sU.tobytes() == (dU + eU).tobytes() and sv.tobytes() == (dv + ev).tobytes()
        assert g.tobytes() == np.ascontiguousarray(sU[:, :nu]).tobytes()
    _, _, g = host.correct(eU, ev, dU, dv, 2, nu, gain=True, ok=False)
    assert (g == 0).all()


# ---- 4. the rules catch seeded defects -----------------------------------------------------------------------------
@pytest.mark.parametrize("defect", ["rhs_stride_ignored", "unit_direction_sign_flipped", "partial_last_group_not_written",
                                    "B_du_dropped_from_the_forward_sweep"])
def test_rules_catch_seeded_defects(host, defect):
    caught = []
    for name in HOST_SHAPES:
        p = ch.problem(name)
        x, seeds = _point_and_seeds(p, 67)
        q = 0
        sq = tuple(s[q] for s in seeds)
        dU, dv = _dense_steps(p, NRHS, 68)
        k = NRHS - 1
        pp = cmh.slot_problem(p, q, sq, k)
        # the correct maps pass on the slot that the defect will hit
        _, gU, gvc = host.seed(p, q, x[0][q], sq, NRHS, 2)
        assert cah.seed_violations(gU[k], gvc[k], pp, 0) == []
        fin = host.finish(p, q, sq, dU, dv, 2)
        assert cah.finish_violations(fin["dz"][k], fin["dl"][k], pp, 0, dU[k], dv[k]) == []
        if defect == "rhs_stride_ignored":
            # every slot reads the seed at the base: slot k computes slot 0's vectors
            _, bU, bv = host.seed(p, q, x[0][q], sq, NRHS, 2, rhs_stride=0)
            bad = cah.seed_violations(bU[k], bv[k], pp, 0)
        elif defect == "unit_direction_sign_flipped":
            unit = cmh.x0_seeds(p)
            j = p.nx - 1
            ppj = cmh.slot_problem(p, q, unit, j)
            _, gx, vx = host.seed(p, q, x[0][q], None, p.nx, 2)
            assert cah.seed_violations(gx[j], vx[j], ppj, 0) == []
            _, bU, bv = host.seed(p, q, x[0][q], (unit[0], -unit[1], unit[2]), p.nx, 2)
            bad = cah.seed_violations(bU[j], bv[j], ppj, 0)
        elif defect == "partial_last_group_not_written":
            _, bU, bv = host.seed(p, q, x[0][q], sq, NRHS, 2, groups=NRHS // 2)
            bf = host.finish(p, q, sq, dU, dv, 2, groups=NRHS // 2)
            bad = cah.seed_violations(bU[k], bv[k], pp, 0) + cah.finish_violations(bf["dz"][k], bf["dl"][k], pp, 0,
                                                                                   dU[k], dv[k])
            assert len(bad) == 4      # (every output of the slot)
        else:
            arrays = {n: a.copy() for n, a in p.arrays.items()}
            arrays["B"][:] = 0.0
            bf = host.finish(fx.MpcProblem(*p.sizes(), arrays), q, sq, dU, dv, 2)
            bad = cah.finish_violations(bf["dz"][k], bf["dl"][k], pp, 0, dU[k], dv[k])
            assert "dz" in bad
        if bad:
            caught.append(name)
    print(defect, "caught on", caught)
    assert caught == list(HOST_SHAPES), (defect, caught)


# ---- 5. the x0 chain in longdouble ---------------------------------------------------------------------------------
def test_x0_chain_gives_the_lqr_gain():
    """All constraints inactive ((8, 4, 2, 1), seed 4401, the construction of test_lqr_gain_from_seeded_input_rows):
    the u_0 rows of the chain's dz over the unit seeds of x0 are du0/dx0 = -K_0 of the Riccati recursion."""
    N, nx, nu, nc = 8, 4, 2, 1
    p = fx.random_ltv_mpc(np.random.default_rng(4401), 1, N, nx, nu, nc)
    for k in ("q", "r", "c"):
        p.arrays[k][:] = 0.0
    p.arrays["E"][:] = 0.0
    p.arrays["L"][:] = 0.0
    p.arrays["d"][:] = -1.0   # 0 <= 1 on every row: inactive, y = 1, v = 0 at every z
    K = H.lqr_gain(p)
    x = (np.zeros(p.nz), np.zeros(p.nl), np.zeros(p.nv))
    unit = cmh.x0_seeds(p)
    G = np.stack([cah.chain_reference(p, 0, x, tuple(s[j] for s in unit), 1e-8)["dz"][nx:nx + nu] for j in range(nx)])
    np.testing.assert_allclose(G.T.astype(np.float64), K, rtol=1e-6)


@pytest.mark.parametrize("name", ["small", "flat"])
def test_x0_chain_is_the_mpc_system_up_to_the_sigma_bias(name):
    """The chain with the unit seeds against cah.mpc_solve_reference: the gap the helper measures (cah.sigma_gap) is
    V^-1 applied to the chain's residual in the MPC system, so at most ||V^-1||_2 times its 2-norm, and that residual
    is sigma (dx, dl) on the x and equality rows (test_condense_adjoint_cpu.py, the identity)."""
    p = ch.problem(name)
    x, _ = _point_and_seeds(p, 69)
    unit = cmh.x0_seeds(p)
    N, nx, nu, nc = p.sizes()
    sigma = 1e-8
    q = 2
    xq = tuple(t[q] for t in x)
    V, Cg = cmh.mpc_system(p, q, xq, sigma)
    inv_norm = float(np.linalg.norm(np.linalg.inv(V.astype(np.float64)), 2))
    for j in (0, nx // 2, nx - 1):
        sj = tuple(s[j] for s in unit)
        gap, smax = cah.sigma_gap(p, q, xq, sj, sigma)
        c = cah.chain_reference(p, q, xq, sj, sigma)
        dx = c["dz"].reshape(N + 1, nx + nu)[:, :nx]
        res = float(LD(sigma) * np.sqrt((dx * dx).sum() + (c["dl"] * c["dl"]).sum()))
        print(name, "column", j, "sigma gap", gap, "max|step|", smax, "||V^-1|| sigma ||(dx, dl)||", inv_norm * res)
        assert gap <= 1.01 * inv_norm * res + 1e-15 * smax, (j, gap, inv_norm, res)
