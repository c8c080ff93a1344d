"""Condensing an MPC QP (fbstab_hip_mpc_condense_batch / _expand_batch, fb_condense.h) without a GPU: the
extended-precision reference of tests/condense_helpers.py against the oracle, the device logic compiled for one
host thread against that reference, the acceptance rule against seeded defects, and the argument checks of the
C-ABI, which run before any device call."""
import ctypes as C

import numpy as np
import pytest

from oracle.oracle_py import Oracle, default_options
from tests import condense_helpers as ch
from tests.helpers import mpc_explicit, natural_residual_norm
from tools import fixtures as fx

LD = ch.LD


@pytest.fixture(scope="module")
def host():
    return ch.HostCondense()


# ---- 1. the reference is right ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "flat", "servo_motor"])
def test_reference_condensed_qp_solves_the_mpc_qp(name):
    p = ch.problem(name)
    orc = Oracle()
    o = default_options(abs_tol=1e-6)
    zc, _, vc, yc, outc = orc.solve_dense(ch.condensed_problem(p), opts=o)
    zm, lm, vm, ym, outm = orc.solve_mpc(p, opts=o)
    assert (outc["eflag"] == 0).all() and (outm["eflag"] == 0).all(), (outc["eflag"], outm["eflag"])
    f = ch.rule_factor(p)
    for q in range(p.batch):
        z, l, v, y = ch.expand_reference(p, q, zc[q], vc[q], yc[q])
        H, ff, G, h, A, b = mpc_explicit(p, q)
        nr = natural_residual_norm(H, ff, G, h, A, b, z.astype(np.float64), l.astype(np.float64), v)
        assert nr <= 2e-6, (q, nr)
        # the states satisfy the dynamics and the costates the x rows of stationarity, to rounding
        Hl, fl, Gl, hl, Al = (np.asarray(a, dtype=LD) for a in (H, ff, G, h, A))
        vl = np.asarray(v, dtype=LD)
        rz = Hl @ z + fl + Gl.T @ l + Al.T @ vl
        bz = (np.abs(Hl) @ np.abs(z) + np.abs(fl) + np.abs(Gl).T @ np.abs(l) + np.abs(Al).T @ np.abs(vl)) * f
        xrows = (np.arange(p.nz) % (p.nx + p.nu)) < p.nx
        assert (np.abs(rz)[xrows] <= bz[xrows]).all()
        rl = hl - Gl @ z
        assert (np.abs(rl) <= (np.abs(hl) + np.abs(Gl) @ np.abs(z)) * f).all()


# ---- 2. the device logic on the host ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ch.SHAPE_NAMES)
def test_host_build_of_the_kernels_meets_the_rule(host, name):
    p = ch.problem(name)
    rng = np.random.default_rng(3)
    for q in range(p.batch):
        ref, bound = ch.assert_condition(p, q)
        res = host.condense(p, q, host.ALL)
        got = ch.images(res, p)
        print(name, q, "worst error / bound:", ch.worst_ratio(got, ref, bound))
        assert ch.rule_violations(got, ref, bound) == []
        assert np.array_equal(got["H"], got["H"].T)          # bit for bit
        vec = host.condense(p, q, host.VECTORS)
        assert vec["f"].tobytes() == res["f"].tobytes() and vec["b"].tobytes() == res["b"].tobytes()
        assert np.isnan(vec["H"]).all() and np.isnan(vec["A"]).all()
        mat = host.condense(p, q, host.MATRICES)
        assert mat["H"].tobytes() == res["H"].tobytes() and mat["A"].tobytes() == res["A"].tobytes()
        assert np.isnan(mat["f"]).all() and np.isnan(mat["b"]).all()
        U, v, y = rng.standard_normal((p.N + 1) * p.nu), np.abs(rng.standard_normal(p.nv)), rng.standard_normal(p.nv)
        z, l, vo, yo = host.expand(p, q, U, v, y)
        zr, lr, _, _ = ch.expand_reference(p, q, U, v, y)
        zb, lb = ch.expand_bound(p, q, U, v, y)
        assert (np.abs(z - zr) <= zb).all() and (np.abs(l - lr) <= lb).all()
        assert vo.tobytes() == v.tobytes() and yo.tobytes() == y.tobytes()


# ---- 3. the rule catches seeded defects --------------------------------------------------------------------------
def _mutated(p, name):
    """``p`` with one term of the data changed: what a kernel that mishandles that term would condense."""
    N, nx, nu, nc = p.sizes()
    m = fx.MpcProblem(N, nx, nu, nc)
    m.arrays = {k: a.copy() for k, a in p.arrays.items()}
    if name == "S_dropped":
        m.arrays["S"][:] = 0.0
    elif name == "S_transposed":   # the nu x nx column-major images read as nx x nu ones
        S = p.arrays["S"].reshape(p.batch, N + 1, nx, nu)                      # [.., col, row] of the true image
        m.arrays["S"] = np.ascontiguousarray(S.reshape(p.batch, N + 1, nu, nx).transpose(0, 1, 3, 2)).reshape(p.batch, -1)
    elif name == "c_omitted":
        m.arrays["c"][:] = 0.0
    return m


@pytest.mark.parametrize("defect", ["S_dropped", "S_transposed", "c_omitted", "L_diagonal_missing", "one_entry_1e-9"])
def test_rule_catches_seeded_defects(host, defect):
    caught = []
    for name in ch.SHAPE_NAMES:
        p = ch.problem(name)
        ref, bound = ch.assert_condition(p, 0)
        good = ch.images(host.condense(p, 0), p)
        assert ch.rule_violations(good, ref, bound) == []
        if defect == "L_diagonal_missing":
            bad = {k: a.copy() for k, a in good.items()}
            for k in range(p.N + 1):
                bad["A"][k * p.nc:(k + 1) * p.nc, k * p.nu:(k + 1) * p.nu] = 0.0
        elif defect == "one_entry_1e-9":
            bad = {k: a.copy() for k, a in good.items()}
            for k in bad:
                i = np.unravel_index(np.argmax(np.abs(bad[k])), bad[k].shape)
                bad[k][i] *= 1.0 + 1e-9
        else:
            bad = {k: a.astype(np.float64) for k, a in ch.condense_reference(_mutated(p, defect), 0).items()}
        if ch.rule_violations(bad, ref, bound):
            caught.append(name)
    print(defect, "caught on", caught)
    assert caught, defect
    if defect == "one_entry_1e-9":
        assert caught == list(ch.SHAPE_NAMES)


# ---- 4. the C-ABI without a GPU ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from fbstab_amd import hip_api
    return hip_api.load_library()


def _lds_bytes(N, nx, nu, nc):
    """The formula include/fbstab_hip.h states."""
    e = lambda n: n + (n & 1)
    ldx, ldc, ldu = nx | 1, nc | 1, nu | 1
    carry = max((N + 2) * e(ldx * nu), (N + 1) * (nx + nu + nc) + 2 * nx + 8)
    return 8 * (2 * e(ldx * nx) + e(ldx * nu) + e(ldc * nx) + e(ldu * nx) + e(ldc * nu) + e(ldu * nu) + e(carry))


def test_condensed_sizes(lib):
    for N, nx, nu, nc in [(1, 1, 1, 1), (3, 5, 2, 3), (2, 33, 3, 1), (6, 30, 3, 5), (8, 6, 8, 4), (10, 40, 3, 6),
                          (15, 12, 4, 20), (10, 60, 4, 6)]:
        nz, nv, lds = C.c_int(-1), C.c_int(-1), C.c_longlong(-1)
        assert lib.fbstab_hip_mpc_condensed_sizes(N, nx, nu, nc, C.byref(nz), C.byref(nv), C.byref(lds)) == 0
        assert (nz.value, nv.value, lds.value) == ((N + 1) * nu, (N + 1) * nc, _lds_bytes(N, nx, nu, nc))
        assert lds.value <= 160 * 1024
    lds = C.c_longlong(-1)
    assert _lds_bytes(10, 120, 4, 6) > 160 * 1024
    assert lib.fbstab_hip_mpc_condensed_sizes(10, 120, 4, 6, None, None, C.byref(lds)) == 3 and lds.value == 0
    assert b"LDS" in lib.fbstab_hip_last_error()
    assert lib.fbstab_hip_mpc_condensed_sizes(0, 2, 1, 1, None, None, None) == 1
    assert lib.fbstab_hip_mpc_condensed_sizes(2, 2, 1, 1, None, None, None) == 0   # (null outputs are allowed)


class _Call:
    """fbstab_hip_mpc_condense_batch / _expand_batch on valid arguments for (2, 3, 2, 2), batch 2; the pointers
    are never followed before the device check."""
    N, nx, nu, nc = 2, 3, 2, 2

    def __init__(self):
        from fbstab_amd import hip_api
        self.buf = np.zeros(4096)
        n1, N, nx, nu, nc = self.N + 1, self.N, self.nx, self.nu, self.nc
        self.len = [n1 * nx * nx, n1 * nu * nu, n1 * nu * nx, n1 * nx, n1 * nu, N * nx * nx, N * nx * nu, N * nx,
                    n1 * nc * nx, n1 * nc * nu, n1 * nc, nx]
        self.data = hip_api._MpcBatch()
        for i, n in enumerate(self.len):
            self.data.base[i], self.data.stride[i] = self.buf.ctypes.data, n
        nz, nv = n1 * nu, n1 * nc
        self.olen = [nz * nz, nz, 0, 0, nv * nz, nv]
        self.dense = hip_api._DenseOutBatch()
        for i, n in enumerate(self.olen):
            if n:
                self.dense.base[i], self.dense.stride[i] = self.buf.ctypes.data, n
        self.xc, self.x = hip_api._VarBatch(), hip_api._VarBatch()
        for i, n in enumerate([nz, 0, nv, nv]):
            if n:
                self.xc.base[i], self.xc.stride[i] = self.buf.ctypes.data, n
        for i, n in enumerate([n1 * (nx + nu), n1 * nx, nv, nv]):
            self.x.base[i], self.x.stride[i] = self.buf.ctypes.data, n
        self.sizes = [self.N, self.nx, self.nu, self.nc]
        self.batch, self.what = 2, 3
        self.null = ()

    def _ref(self, name):
        return None if name in self.null else C.byref(getattr(self, name))

    def condense(self, lib):
        rc = lib.fbstab_hip_mpc_condense_batch(*self.sizes, self.batch, self._ref("data"), self.what,
                                               self._ref("dense"), 0, None)
        return rc, lib.fbstab_hip_last_error().decode()

    def expand(self, lib):
        rc = lib.fbstab_hip_mpc_expand_batch(*self.sizes, self.batch, self._ref("data"), self._ref("xc"),
                                             self._ref("x"), 0, None)
        return rc, lib.fbstab_hip_last_error().decode()


def _bad_cases():
    """name -> (entry, what to break)."""
    def size(i):
        def f(c): c.sizes[i] = 0
        return f
    cases = {}
    for e in ("condense", "expand"):
        for i, n in enumerate(("N", "nx", "nu", "nc")):
            cases[f"{e}_{n}_zero"] = (e, size(i))
        cases[f"{e}_negative_batch"] = (e, lambda c: setattr(c, "batch", -1))
        cases[f"{e}_null_data_block"] = (e, lambda c: setattr(c, "null", ("data",)))
        cases[f"{e}_null_data_pointer"] = (e, lambda c: c.data.base.__setitem__(5, None))
        cases[f"{e}_short_data_stride"] = (e, lambda c: c.data.stride.__setitem__(0, c.len[0] - 1))
        cases[f"{e}_negative_data_stride"] = (e, lambda c: c.data.stride.__setitem__(11, -3))
    cases["condense_what_0"] = ("condense", lambda c: setattr(c, "what", 0))
    cases["condense_what_4"] = ("condense", lambda c: setattr(c, "what", 4))
    cases["condense_null_out_block"] = ("condense", lambda c: setattr(c, "null", ("dense",)))
    cases["condense_null_H"] = ("condense", lambda c: c.dense.base.__setitem__(0, None))
    cases["condense_null_b"] = ("condense", lambda c: c.dense.base.__setitem__(5, None))
    cases["condense_short_H_stride"] = ("condense", lambda c: c.dense.stride.__setitem__(0, c.olen[0] - 1))
    cases["condense_f_stride_0"] = ("condense", lambda c: c.dense.stride.__setitem__(1, 0))
    cases["condense_H_stride_0_per_qp_model"] = ("condense", lambda c: c.dense.stride.__setitem__(0, 0))

    def mixed(c):   # every matrix sequence shared but one
        for i in (0, 1, 2, 5, 6, 8):
            c.data.stride[i] = 0
        c.dense.stride[4] = 0
    cases["condense_A_stride_0_one_sequence_per_qp"] = ("condense", mixed)
    cases["expand_null_xc_block"] = ("expand", lambda c: setattr(c, "null", ("xc",)))
    cases["expand_null_x_block"] = ("expand", lambda c: setattr(c, "null", ("x",)))
    cases["expand_null_U"] = ("expand", lambda c: c.xc.base.__setitem__(0, None))
    cases["expand_null_v"] = ("expand", lambda c: c.xc.base.__setitem__(2, None))
    cases["expand_null_yc_with_y"] = ("expand", lambda c: c.xc.base.__setitem__(3, None))
    cases["expand_short_U_stride"] = ("expand", lambda c: c.xc.stride.__setitem__(0, 1))
    cases["expand_short_z_stride"] = ("expand", lambda c: c.x.stride.__setitem__(0, 0))
    cases["expand_short_l_stride"] = ("expand", lambda c: c.x.stride.__setitem__(1, 2))
    return cases


@pytest.mark.parametrize("case", sorted(_bad_cases()))
def test_bad_arguments_are_refused_before_any_device_call(lib, case):
    entry, breaker = _bad_cases()[case]
    c = _Call()
    breaker(c)
    rc, msg = getattr(c, entry)(lib)
    assert rc == 1 and msg, (rc, msg)


def test_valid_arguments_reach_the_device_check(lib):
    for entry in ("condense", "expand"):
        c = _Call()
        c.batch = 0                                  # OK, and queues nothing - with or without a device
        assert getattr(c, entry)(lib)[0] == 0
        # slots `what` does not select may be NULL; shared model with one image of H and A
        c = _Call()
        c.batch = 0
        c.what = 2
        c.dense.base[0] = c.dense.base[4] = None
        assert c.condense(lib)[0] == 0
        c = _Call()
        c.batch = 0
        for i in (0, 1, 2, 5, 6, 8, 9):
            c.data.stride[i] = 0
        c.dense.stride[0] = c.dense.stride[4] = 0
        assert c.condense(lib)[0] == 0
    if lib.fbstab_hip_device_count() == 0:
        for entry in ("condense", "expand"):
            rc, msg = getattr(_Call(), entry)(lib)
            assert rc == 2 and "device" in msg, (rc, msg)
            # the device is checked before the LDS rule
            c = _Call()
            c.sizes[1] = 200
            for i, n in enumerate(c.len):
                c.data.stride[i] = 0
            c.batch = 1
            assert getattr(c, entry)(lib)[0] == 2
