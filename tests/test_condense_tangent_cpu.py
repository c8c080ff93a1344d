"""The forward mode of the condensed MPC route (fbstab_hip_mpc_condensed_tangent_batch) without a GPU: the export and
every refusal of the C-ABI in its documented order, the host stage condensed_tangent_run of fb_condense_stage.h under
tests/hostsim/condense_tangent_stage_driver.cc (plain, and under the address and undefined-behaviour sanitizers), and
the whole tangent as a chain of the host builds of the device logic - direction, seed, the condensed solve, finish -
against the longdouble chain, central differences of the oracle's solves and the adjoint's gradient table."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle.oracle_py import default_options
from tests import condense_adjoint_helpers as cah
from tests import condense_helpers as ch
from tests import condense_tangent_helpers as cth
from tests import linear_reference as lr
from tests import tangent_helpers as TH
from tests.hostsim import HostTangent
from tests.test_host_stage import CSRC, HOSTSIM
from tools import fixtures as fx

GROUPS = ("carve", "sequence", "refusals")


# ---- 1. the C-ABI without a GPU -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from fbstab_amd import hip_api
    return hip_api.load_library()


class _Call:
    """fbstab_hip_mpc_condensed_tangent_batch on valid arguments for (2, 3, 2, 2), batch 2, but for the handle (there is
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
        self.data, self.ddata = hip_api._MpcBatch(), hip_api._MpcBatch()
        for i, n in enumerate(self.len):
            self.data.base[i], self.data.stride[i] = at, n
            self.ddata.base[i], self.ddata.stride[i] = at, n
        nz, nv = n1 * nu, n1 * nc
        self.dlen = [nz * nz, nz, 0, 0, nv * nz, nv]
        self.dense = hip_api._DenseBatch()
        for i, n in enumerate(self.dlen):
            if n:
                self.dense.base[i], self.dense.stride[i] = at, n
        self.xlen = [n1 * (nx + nu), n1 * nx, nv]
        self.x, self.dx, self.rhs = hip_api._VarBatch(), hip_api._VarBatch(), hip_api._VarBatch()
        for blk in (self.x, self.dx, self.rhs):
            for i, n in enumerate(self.xlen):
                blk.base[i], blk.stride[i] = at, n
        self.sizes = [self.N, self.nx, self.nu, self.nc]
        self.batch, self.handle = 2, None
        self.work, self.status = at, self.st.ctypes.data
        self.null = ()

    def _ref(self, name):
        return None if name in self.null else C.byref(getattr(self, name))

    def __call__(self, lib):
        rc = lib.fbstab_hip_mpc_condensed_tangent_batch(
            self.handle, *self.sizes, self.batch, self._ref("data"), self._ref("dense"), self._ref("x"),
            self._ref("ddata"), C.c_double(0.0), self._ref("dx"), self._ref("rhs"),
            None if "work" in self.null else C.c_void_p(self.work),
            None if "status" in self.null else C.c_void_p(self.status), None)
        return rc, lib.fbstab_hip_last_error().decode()


def _set(block, field, i, value):
    return lambda c: getattr(getattr(c, block), field).__setitem__(i, value)


# (what to break, the message) in the documented order: every case also breaks what the NEXT case breaks, so a refusal
# that comes back with its own message shows that its check runs before the next one
_ORDER = [
    (lambda c: c.sizes.__setitem__(2, 0), "condense: problem sizes must be positive"),
    (lambda c: setattr(c, "batch", -1), "condense: negative batch"),
    (lambda c: setattr(c, "null", c.null + ("data",)), "condense: null problem data block"),
    (_set("data", "base", 5, None), "condense: null problem data pointer"),
    (_set("data", "stride", 11, 2), "condense: problem data stride smaller than the array length"),
    (lambda c: setattr(c, "null", c.null + ("ddata",)), "condensed tangent: null argument"),
    (_set("dense", "base", 0, None), "condensed tangent: null pointer in the condensed images"),
    (_set("dense", "stride", 1, 0), "condensed tangent: stride of a condensed image smaller than the array length"),
    (_set("x", "base", 0, None), "condensed tangent: null variable pointer"),
    (_set("x", "stride", 0, 1), "condensed tangent: variable stride smaller than the vector length"),
    (_set("dx", "base", 0, None), "condensed tangent: null tangent pointer (dx)"),
    (_set("dx", "stride", 0, 1), "condensed tangent: tangent stride smaller than the vector length"),
    (_set("rhs", "base", 0, None), "condensed tangent: null right-hand side pointer (rhs)"),
    (_set("rhs", "stride", 0, 0), "condensed tangent: right-hand side stride smaller than the vector length"),
    (_set("ddata", "stride", 3, 1), "condensed tangent: perturbation stride is neither 0 nor at least the array length"),
    (lambda c: None, "condensed tangent: null dense solver handle"),
]


def test_entry_point_is_exported_and_refuses_in_the_documented_order_without_gpu(lib):
    """The symbol is in the library and in EXPORTED_SYMBOLS, and every refusal that needs no handle comes back as
    FBSTAB_HIP_ERR_ARGUMENT with its message, each before the checks behind it; valid arguments are stopped by the
    missing handle (there is none without a device) and by nothing before."""
    from fbstab_amd import hip_api
    assert "fbstab_hip_mpc_condensed_tangent_batch" in hip_api.EXPORTED_SYMBOLS
    assert len(lib.fbstab_hip_mpc_condensed_tangent_batch.argtypes) == 16
    for i, (breaker, message) in enumerate(_ORDER):
        c = _Call()
        for later, _ in reversed(_ORDER[i:i + 2]):   # (the next check's argument first, then this one's)
            later(c)
        assert c(lib) == (1, message), (i, message)
    for k in ("dense", "x", "dx", "work", "status"):
        c = _Call()
        c.null = (k,)
        assert c(lib) == (1, "condensed tangent: null argument"), k
    # what is allowed reaches the handle check: rhs NULL, NULL perturbation slots whatever their stride, stride 0 on
    # a perturbation and on H_c, A_c, batch 0, and with batch 1 strides that nobody reads
    for breaker in (lambda c: setattr(c, "null", ("rhs",)),
                    lambda c: [(c.ddata.base.__setitem__(i, None), c.ddata.stride.__setitem__(i, -3)) for i in range(12)],
                    lambda c: [c.ddata.stride.__setitem__(i, 0) for i in range(12)],
                    lambda c: (c.dense.stride.__setitem__(0, 0), c.dense.stride.__setitem__(4, 0)),
                    lambda c: setattr(c, "batch", 0),
                    lambda c: (setattr(c, "batch", 1), c.x.stride.__setitem__(0, 0), c.dx.stride.__setitem__(1, -1),
                               c.rhs.stride.__setitem__(2, 0), c.ddata.stride.__setitem__(0, 1))):
        c = _Call()
        breaker(c)
        assert c(lib) == (1, "condensed tangent: null dense solver handle")


# ---- 2. the host stage ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["plain", "sanitized"])
def driver(request, tmp_path_factory):
    """-> run(group) -> (exit status, output): tests/hostsim/condense_tangent_stage_driver.cc, a program of its own;
    `sanitized`: built with -fsanitize=address,undefined, where a finding ends it with a non-zero status."""
    d = tmp_path_factory.mktemp("condense_tangent_stage_" + request.param)
    exe = str(d / "condense_tangent_stage_driver")
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", *extra,
                           "-I" + os.path.join(HOSTSIM, "runtime_shim"), "-I" + CSRC, "-o", exe,
                           os.path.join(HOSTSIM, "condense_tangent_stage_driver.cc")])

    def run(group):
        r = subprocess.run([exe, group], capture_output=True, text=True)
        return r.returncode, r.stdout + r.stderr
    return run


@pytest.mark.parametrize("group", GROUPS)
def test_the_tangent_stage_checks_carves_and_queues_as_the_header_says(driver, group):
    """carve: the seed tail begins where the adjoint's work ends and ends with the documented size, and with rhs the
    work array (allocated without the tail) is never addressed beyond the adjoint's part; sequence: the direction first,
    then the adjoint's six, the blocks each launch receives, batch 1 reads no stride, batch 0 queues nothing;
    refusals: every one of include/fbstab_hip.h in its order, before any device call."""
    status, output = driver(group)
    assert status == 0 and output == "", output[-4000:]


def test_the_driver_knows_its_groups(driver):
    assert driver("no such group")[0] == 2


# ---- 3. end to end on the host ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hosts():
    return HostTangent(), cah.HostCondenseAdjoint()


@pytest.mark.parametrize("name", ["small", "odd33", "four_wave", "flat"])
def test_tangent_end_to_end_on_the_host(hosts, oracle, name):
    """HostTangent.rhs, HostCondenseAdjoint.seed, the double solve of cah.dense_system refined once,
    HostCondenseAdjoint.finish(want=()), at the oracle's solutions (abs_tol 1e-11) of the fixture, all 12 sequences
    perturbed, dQ and dR symmetrised.  Every QP is strictly complementary at 1e-3 (asserted first).  Then
      - the seeds meet the rounding bound of tangent_helpers.assert_rhs;
      - the step is the longdouble chain's (cah.chain_reference on the same seeds) within the forward error
        1e-5 max(|step|, 1) that linear_reference.check_step_and_table allows a step at cond(V) ~ 1e11;
      - it is within 1e-4 of its largest entry of the central differences (h = 1e-5) of the oracle's solves (the
        project's bar for this comparison; measured 4.2e-6 at worst, flat QP 0, 1e-7 or below elsewhere);
      - <g, J dtheta> agrees with sum_k <gradient_table_k, dtheta_k>, both steps from this chain, relative to the
        sum of the magnitudes of the terms of <g, J dtheta>, within tangent_helpers.DUALITY_BAR (measured 2.4e-15:
        the chain keeps the duality with the adjoint's table).  The number is printed."""
    host_t, host_ca = hosts
    p = ch.problem(name)
    opts = default_options(abs_tol=1e-11)
    z, l, v, _, out = oracle.solve_mpc(p, opts=opts)
    assert (out["eflag"] == 0).all()
    margins = [cth.strictness(p, q, z, v) for q in range(p.batch)]
    assert min(margins) >= 1e-3, margins
    rng = np.random.default_rng(9100 + len(name))
    d = cth.symmetrised(p, TH.random_directions(rng, p, p.batch))
    g = lr.random_seeds(rng, p)
    h = 1e-5
    plus = fx.MpcProblem(*p.sizes(), {k: p.arrays[k] + h * d[k] for k in ch.MPC_NAMES})
    minus = fx.MpcProblem(*p.sizes(), {k: p.arrays[k] - h * d[k] for k in ch.MPC_NAMES})
    sp, sm = oracle.solve_mpc(plus, opts=opts), oracle.solve_mpc(minus, opts=opts)
    assert (sp[4]["eflag"] == 0).all() and (sm[4]["eflag"] == 0).all()
    worst_fd = worst_dual = worst_chain = 0.0
    for q in range(p.batch):
        x = (z[q], l[q], v[q])
        dq = TH.one_direction(d, q)
        rhs = host_t.rhs(p, x, dq)
        TH.assert_rhs(p, q, x, dq, rhs)
        chain = cth.HostChain(p, q, x, host_ca)
        step = chain.step(rhs)
        ref = cah.chain_reference(p, q, x, rhs)
        dx = np.concatenate(step)
        dref = np.concatenate([ref[k] for k in cth.STEP]).astype(np.float64)
        err = np.abs(dx - dref).max() / max(np.abs(dref).max(), 1.0)
        worst_chain = max(worst_chain, err)
        assert err <= 1e-5, (q, err)
        fd = np.concatenate([(sp[i][q] - sm[i][q]) / (2 * h) for i in range(3)])
        err = np.abs(dx - fd).max() / np.abs(dx).max()
        worst_fd = max(worst_fd, err)
        assert err <= 1e-4, (q, err)
        gq = tuple(t[q] for t in g)
        table = lr.mpc_gradient_table(lr.one_qp(p, q), x, chain.step(gq))
        dual = cth.duality_number(gq, step, table, dq)
        worst_dual = max(worst_dual, dual)
    print("condensed tangent on the host, %s: strictness %.2e, chain %.2e, central differences %.2e, duality %.2e"
          % (name, min(margins), worst_chain, worst_fd, worst_dual))
    assert worst_dual <= TH.DUALITY_BAR, worst_dual
