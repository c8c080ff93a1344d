"""GPU tests: the reference's hand-calculated COMPONENT goldens through the HIP
Newton-step probes (fbstab_hip_mpc_debug_newton / fbstab_hip_dense_debug_newton),
and seeded random-shape subsets of tools/fuzz_shapes.py / tools/fuzz_dense.py that
reach every MPC kernel instance and every dense kernel.

The goldens are the reference's own (tests/golden/reference_kats.json, transcribed
from fbstab/components/test/mpc_component_unit_tests.h:99-461 and
dense_unit_tests.h:100-213); tests/test_oracle.py pins the oracle with them on the
CPU, this file puts the same numbers to the device path."""
import numpy as np
import pytest

from tools import fixtures as fx
from oracle.oracle_py import default_options
from tests import helpers as H
from tests.shapes import MPC_SHAPES, DEGENERATE_SHAPES, fuzz_dense_instances

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from fbstab_amd import hip_api
    assert hip_api.load_library().fbstab_hip_device_count() >= 1
    return hip_api


def _opts(hip, o):
    h = hip.Options()
    for name, _ in h._fields_:
        setattr(h, name, getattr(o, name))
    return h


@pytest.mark.parametrize("kernel", ["r16", "generic"])
def test_mpc_component_goldens_through_the_hip_probe(hip, kats, monkeypatch, kernel):
    """mpc_component_unit_tests.h:99-461 on the record kernel (padded <12,4,20>
    instance) and on the flat-vector kernel: the products gemvH/GT/AT/G and the
    constants f, h behind the natural residual, A z, the InnerResidual golden
    (1e-14 in the reference; 1e-12 here for rv, which is recovered from the step),
    and the Newton system's residual, block by block."""
    monkeypatch.setenv("FBSTAB_HIP_GENERIC", "1" if kernel == "generic" else "0")
    c = kats["mpc_components"]
    p = H.mpc_component_fixture(c)
    data = {k: a[0] for k, a in p.arrays.items()}
    s = hip.FBstabMpcBatch(*p.sizes(), max_batch=1)
    if kernel == "r16":
        assert s.kernel_name() == "fbstab_mpc_r16_kernel<12,4,20>"
    Hm, f, G, h, A, b = H.mpc_explicit(p)
    ramp = lambda n: np.arange(1, n + 1, dtype=np.float64)
    exp = lambda op: np.asarray(c[op]["expected"], dtype=np.float64)
    alpha = 0.95

    # ---- gemvH + f + gemvGT + gemvAT and h - gemvG at the ramp vectors (:99-192)
    s.UpdateOptions(hip.DefaultOptions(sigma0=1.0, sigma_max=100.0, alpha=alpha))
    z, l, v = ramp(p.nz), ramp(p.nl), ramp(p.nv)
    g = s.debug_newton(data, z, l, v, z, l, v)
    assert g["ok"]
    np.testing.assert_allclose(g["rz"], exp("gemvH") + f + exp("gemvGT") + exp("gemvAT"), rtol=0, atol=1e-12)
    np.testing.assert_allclose(g["rl"], h - exp("gemvG"), rtol=0, atol=1e-12)
    # gemvA golden through the step: adz = A dz, and y = b - A z enters dv
    np.testing.assert_allclose(exp("gemvA"), A @ z, rtol=0, atol=0)
    np.testing.assert_allclose(g["adz"], A @ g["dz"], rtol=0, atol=1e-12 * (1 + np.abs(g["dz"]).max()))

    # ---- InnerResidual golden: x.Fill(2), xbar.Fill(-2), sigma = 1 (:316-355)
    gi = c["inner_residual"]
    fill = lambda n, a: np.full(n, float(a))
    z, l, v = fill(p.nz, 2), fill(p.nl, 2), fill(p.nv, 2)
    zb, lb, vb = fill(p.nz, -2), fill(p.nl, -2), fill(p.nv, -2)
    g = s.debug_newton(data, z, l, v, zb, lb, vb)
    assert g["ok"]
    np.testing.assert_allclose(g["rz"] + 1.0 * (z - zb), gi["rz"], rtol=0, atol=1e-13)
    np.testing.assert_allclose(g["rl"] + 1.0 * (l - lb), gi["rl"], rtol=0, atol=1e-13)
    # rv = phi(y + sigma (v - vbar), v): the third block row of the Newton system,
    # -gamma (A dz) + mus dv = -rv, gives it back from the device's step
    y = b - A @ z
    gam, mus = H.pfb_gradient(y + 1.0 * (v - vb), v, alpha, 1.0)
    np.testing.assert_allclose(gam * g["adz"] - mus * g["dv"], gi["rv"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(H.pfb(y + (v - vb), v, alpha), gi["rv"], rtol=0, atol=1e-13)

    # ---- the Riccati golden's point: x = (1,2,4), xbar = (2,1,3), sigma = 1 (:386-461):
    # every block of V dx - r vanishes (r = -inner residual here), W = (H dz + G'dl + A'dv, -G dz)
    z, l, v = fill(p.nz, 1), fill(p.nl, 2), fill(p.nv, 4)
    zb, lb, vb = fill(p.nz, 2), fill(p.nl, 1), fill(p.nv, 3)
    g = s.debug_newton(data, z, l, v, zb, lb, vb)
    assert g["ok"]
    y = b - A @ z
    gam, mus = H.pfb_gradient(y + (v - vb), v, alpha, 1.0)
    rz = -(g["rz"] + (z - zb))
    rl = -(g["rl"] + (l - lb))
    rv = -H.pfb(y + (v - vb), v, alpha)
    e1 = Hm @ g["dz"] + g["dz"] + G.T @ g["dl"] + A.T @ g["dv"] - rz
    e2 = -G @ g["dz"] + g["dl"] - rl
    e3 = -gam * (A @ g["dz"]) + mus * g["dv"] - rv
    for e in (e1, e2, e3):
        assert np.abs(e).max() <= 1e-12, np.abs(e).max()
    np.testing.assert_allclose(g["wz"], Hm @ g["dz"] + G.T @ g["dl"] + A.T @ g["dv"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(g["wl"], -G @ g["dz"], rtol=0, atol=1e-12)
    s.close()


@pytest.mark.parametrize("threads", ["64", "256"])
def test_dense_component_goldens_through_the_hip_probe(hip, kats, monkeypatch, threads):
    """dense_unit_tests.h:100-213 on the one-wavefront and the four-wavefront dense
    kernels: NaturalResidual and InnerResidual goldens, rv through the step, and the
    linear solver's residual (1e-12 in the reference)."""
    monkeypatch.setenv("FBSTAB_HIP_DENSE_THREADS", threads)
    c = kats["dense_components"]
    p = H.dense_from_kat(dict(H=c["H"], f=c["f"], A=c["A"], b=c["b"]))
    data = {k: a[0] for k, a in p.arrays.items()}
    Hm, f, G, h, A, b = H.dense_explicit(p)
    gi, gn, gl = c["inner_residual"], c["natural_residual"], c["linear_solver"]
    sigma, alpha = gi["sigma"], 0.95
    s = hip.FBstabDenseBatch(p.nz, p.nl, p.nv, max_batch=1)
    assert s.query()["threads"] == int(threads)
    s.UpdateOptions(hip.DefaultOptions(sigma0=sigma, sigma_max=100.0, alpha=alpha))
    e = np.zeros(0)
    z, v = np.asarray(gi["x_z"], float), np.asarray(gi["x_v"], float)
    zb, vb = np.asarray(gi["xbar_z"], float), np.asarray(gi["xbar_v"], float)
    g = s.debug_newton(data, z, e, v, zb, e, vb)
    assert g["ok"]
    np.testing.assert_allclose(g["rz"], gn["rz"], rtol=0, atol=1e-13)
    np.testing.assert_allclose(g["rz"] + sigma * (z - zb), gi["rz"], rtol=0, atol=1e-13)
    y = b - A @ z
    np.testing.assert_allclose(np.minimum(y, v), gn["rv"], rtol=0, atol=1e-14)
    gam, mus = H.pfb_gradient(y + sigma * (v - vb), v, alpha, sigma)
    np.testing.assert_allclose(gam * (A @ g["dz"]) - mus * g["dv"], gi["rv"], rtol=0, atol=1e-12)
    # linear solver (:169-208): both block rows of the eliminated-free system vanish
    rz = -(g["rz"] + sigma * (z - zb))
    rv = -H.pfb(y + sigma * (v - vb), v, alpha)
    e1 = Hm @ g["dz"] + sigma * g["dz"] + A.T @ g["dv"] - rz
    e3 = -gam * (A @ g["dz"]) + mus * g["dv"] - rv
    assert np.sqrt(e1 @ e1 + e3 @ e3) <= gl["tol"]
    s.close()


@pytest.mark.parametrize("idx", range(len(MPC_SHAPES)))
def test_random_shapes_on_every_mpc_instance(hip, oracle, idx):
    """tools/fuzz_shapes.py, a fixed subset: random time-varying problems (dense
    constraint rows, S != 0) of shapes chosen to land on each of the five record
    instances and on the flat-vector kernel, a third of them with a restricted line
    search.  Exit flags and proximal counts equal the oracle's; Newton counts differ
    by at most 2; solutions within the parity tolerance."""
    (N, nx, nu, nc), kern = MPC_SHAPES[idx]
    rng = np.random.default_rng(7000 + idx)
    B = int(rng.integers(2, 12))
    o = default_options()
    if idx % 3 == 2:
        o = default_options(max_linesearch_iters=int(rng.integers(1, 12)), nonmonotone_linesearch=int(rng.random() < 0.5))
    p = fx.random_ltv_mpc(rng, B, N, nx, nu, nc)
    s = hip.FBstabMpcBatch(N, nx, nu, nc, max_batch=B)
    assert s.kernel_name() == kern, s.kernel_name()
    s.UpdateOptions(_opts(hip, o))
    z = np.zeros((B, p.nz)); l = np.zeros((B, p.nl)); v = np.zeros((B, p.nv)); y = np.zeros((B, p.nv))
    out = s.Solve({k: np.ascontiguousarray(a) for k, a in p.arrays.items()}, z, l, v, y)
    s.close()
    c = oracle.solve_mpc(p, opts=o, nthreads=oracle.num_threads())
    oc = c[4]
    assert np.array_equal(out["eflag"], oc["eflag"])
    assert np.array_equal(out["prox_iters"], oc["prox_iters"])
    dn = np.abs(out["newton_iters"].astype(int) - oc["newton_iters"].astype(int))
    assert dn.max() == 0, dn  # (strict since round 5: 20 fuzz seeds with every count equal, profiles/r05_a_*)
    good = oc["eflag"] == 0
    if good.any():
        scale = 1.0 + np.abs(c[0]).max(axis=1, keepdims=True)
        assert (np.abs(z - c[0])[good] <= 10 * o.abs_tol * scale[good]).all()


@pytest.mark.parametrize("idx", range(0, len(MPC_SHAPES), 2))
def test_random_shapes_with_bound_constraints_on_every_mpc_instance(hip, oracle, idx):
    """The same with BOUND constraints (fixtures.random_ltv_mpc_bounds: one +-1 entry per row) - the
    constraints that take the record kernels' row form of the costate step, on the one-row instances
    (explicit inverse of Lc) and the row-pair ones (substitution) alike: every count equal to the oracle's."""
    (N, nx, nu, nc), kern = MPC_SHAPES[idx]
    rng = np.random.default_rng(7500 + idx)
    B = int(rng.integers(2, 10))
    o = default_options()
    p = fx.random_ltv_mpc_bounds(rng, B, N, nx, nu, nc)
    s = hip.FBstabMpcBatch(N, nx, nu, nc, max_batch=B)
    assert s.kernel_name() == kern, s.kernel_name()
    s.UpdateOptions(_opts(hip, o))
    z = np.zeros((B, p.nz)); l = np.zeros((B, p.nl)); v = np.zeros((B, p.nv)); y = np.zeros((B, p.nv))
    out = s.Solve({k: np.ascontiguousarray(a) for k, a in p.arrays.items()}, z, l, v, y)
    s.close()
    c = oracle.solve_mpc(p, opts=o, nthreads=oracle.num_threads())
    oc = c[4]
    assert np.array_equal(out["eflag"], oc["eflag"])
    assert np.array_equal(out["prox_iters"], oc["prox_iters"])
    assert np.array_equal(out["newton_iters"], oc["newton_iters"]), (out["newton_iters"], oc["newton_iters"])
    good = oc["eflag"] == 0
    if good.any():
        scale = 1.0 + np.abs(c[0]).max(axis=1, keepdims=True)
        assert (np.abs(z - c[0])[good] <= 10 * o.abs_tol * scale[good]).all()


@pytest.mark.parametrize("idx", range(1, len(MPC_SHAPES), 2))
def test_random_shapes_with_sparse_constraint_rows_on_every_mpc_instance(hip, oracle, idx):
    """The same with SPARSE rows (fixtures.random_ltv_mpc_sparse_rows: two or three entries of 0.3 .. 0.8 per
    row) - rows that take the row form of the costate step without being bounds (choose_costate_form:
    nonzeros per row x column sums of C'C <= 8), like the bench line's time-varying workload."""
    (N, nx, nu, nc), kern = MPC_SHAPES[idx]
    rng = np.random.default_rng(7700 + idx)
    B = int(rng.integers(2, 10))
    o = default_options()
    p = fx.random_ltv_mpc_sparse_rows(rng, B, N, nx, nu, nc)
    s = hip.FBstabMpcBatch(N, nx, nu, nc, max_batch=B)
    assert s.kernel_name() == kern, s.kernel_name()
    s.UpdateOptions(_opts(hip, o))
    z = np.zeros((B, p.nz)); l = np.zeros((B, p.nl)); v = np.zeros((B, p.nv)); y = np.zeros((B, p.nv))
    out = s.Solve({k: np.ascontiguousarray(a) for k, a in p.arrays.items()}, z, l, v, y)
    s.close()
    c = oracle.solve_mpc(p, opts=o, nthreads=oracle.num_threads())
    oc = c[4]
    assert np.array_equal(out["eflag"], oc["eflag"])
    assert np.array_equal(out["prox_iters"], oc["prox_iters"])
    assert np.array_equal(out["newton_iters"], oc["newton_iters"]), (out["newton_iters"], oc["newton_iters"])
    good = oc["eflag"] == 0
    if good.any():
        scale = 1.0 + np.abs(c[0]).max(axis=1, keepdims=True)
        assert (np.abs(z - c[0])[good] <= 10 * o.abs_tol * scale[good]).all()


@pytest.mark.parametrize("idx", range(0, len(MPC_SHAPES), 2))
def test_warm_started_second_solve_on_every_mpc_instance(hip, oracle, oracle_fma, idx):
    """tools/fuzz_shapes.py ... warm, a fixed subset (the tool's twelve seeds:
    profiles/r06_*_fuzz_warm_start_family_12_seeds.txt): every shape is solved, then solved AGAIN with x0 moved
    by a few per cent, warm-started from the device's first solution - device and oracle get the same guess, so
    the second solve is an independent comparison on identical inputs.  QPs with a solution: flag, proximal and
    Newton count equal to the oracle's, or to the oracle's FMA build where the two builds of the oracle part
    (the one-step kind of test_the_one_count_the_references_rounding_decides).  QPs that end without one (the
    moved x0 makes some infeasible): flag and proximal count; their Newton counts are the tool's to report, not
    a test's to bound (iterates at norms of 1e8: the carried residual and a freshly evaluated one part by more
    than a tolerance).
    Shape 2 of the list ((3, 12, 1, 17): nx > N nu, stages whose Pi keeps eigenvalues of order sigma) is the
    one that FAILED this test when it was written: the one-row instances multiplied with an explicitly inverted
    factor in the reference form of the costate step too, a warm-started one-step solve left 1.4e-6 of its
    Newton system behind (the oracle's substitution: 2e-8) and took a second proximal iteration.  That form
    substitutes since (fb_mpc_r16.h: newton_core; LABNOTES R6.5) and the shape passes as it is, with
    no step refined."""
    (N, nx, nu, nc), kern = MPC_SHAPES[idx]
    rng = np.random.default_rng(9000 + idx)
    B = int(rng.integers(3, 12))
    o = default_options()
    p = fx.random_ltv_mpc(rng, B, N, nx, nu, nc)
    s = hip.FBstabMpcBatch(N, nx, nu, nc, max_batch=B)
    assert s.kernel_name() == kern, s.kernel_name()
    s.UpdateOptions(_opts(hip, o))
    z = np.zeros((B, p.nz)); l = np.zeros((B, p.nl)); v = np.zeros((B, p.nv)); y = np.zeros((B, p.nv))
    s.Solve({k: np.ascontiguousarray(a) for k, a in p.arrays.items()}, z, l, v, y)
    p2 = fx.MpcProblem(N, nx, nu, nc)
    p2.arrays = dict(p.arrays)
    x0 = p.arrays["x0"]
    p2.arrays["x0"] = np.ascontiguousarray(x0 * (1.0 + 0.05 * rng.standard_normal(x0.shape)) + 0.01 * rng.standard_normal(x0.shape))
    guess = (z.copy(), l.copy(), v.copy())
    y2 = np.zeros((B, p.nv))
    out = s.Solve({k: np.ascontiguousarray(a) for k, a in p2.arrays.items()}, z, l, v, y2)
    assert s.refined_steps() == 0
    s.close()
    oc = oracle.solve_mpc(p2, guess, opts=o, nthreads=oracle.num_threads())[4]
    assert np.array_equal(out["eflag"], oc["eflag"])
    assert np.array_equal(out["prox_iters"][oc["eflag"] != 0], oc["prox_iters"][oc["eflag"] != 0])
    conv = oc["eflag"] == 0
    same = (out["prox_iters"] == oc["prox_iters"]) & (out["newton_iters"] == oc["newton_iters"])
    if not same[conv].all():
        of = oracle_fma.solve_mpc(p2, guess, opts=o, nthreads=oracle_fma.num_threads())[4]
        same = same | ((out["prox_iters"] == of["prox_iters"]) & (out["newton_iters"] == of["newton_iters"]))
    assert same[conv].all(), (out[conv], oc[conv])


def test_the_one_count_the_references_rounding_decides(hip, oracle, oracle_fma):
    """The one deviation 12 fuzz seeds of the sparse-row family hold (~8,400 QPs; profiles/r05_a_*): seed 301,
    shape 144, QP 4 - a one-step QP whose exact Newton step ends at 2e-7.  The ORACLE's own step leaves
    1.2e-6 of the Newton system behind, over abs_tol by itself, and it runs a second iteration; the oracle
    compiled with fused multiply-adds allowed (oracle/liboracle_fma.so: same algorithm, same order of
    operations) stops after one.  No literal counts here: on EVERY QP of the shape the
    device's (flag, proximal, Newton) triple must be the triple of one of the two builds of the oracle, and
    wherever the two builds agree with each other - the count is not the compiler's to decide - it is
    theirs.  The solutions agree to a third of the tolerance either way."""
    p, o = H.fuzz_stream_shape(301, 143, "sparse")
    N, nx, nu, nc = p.sizes()
    B = p.batch
    s = hip.FBstabMpcBatch(N, nx, nu, nc, max_batch=B)
    assert s.kernel_name() == "fbstab_mpc_r16_kernel<12,4,20>"
    s.UpdateOptions(_opts(hip, o))
    z = np.zeros((B, p.nz)); l = np.zeros((B, p.nl)); v = np.zeros((B, p.nv)); y = np.zeros((B, p.nv))
    out = s.Solve({k: np.ascontiguousarray(a) for k, a in p.arrays.items()}, z, l, v, y)
    s.close()
    c = oracle.solve_mpc(p, opts=o, nthreads=oracle.num_threads())
    f = oracle_fma.solve_mpc(p, opts=o, nthreads=oracle_fma.num_threads())
    triple = lambda r: np.stack([r["eflag"], r["prox_iters"], r["newton_iters"]], axis=1).astype(int)
    td, tc, tf = triple(out), triple(c[4]), triple(f[4])
    as_plain, as_fma = (td == tc).all(axis=1), (td == tf).all(axis=1)
    assert (as_plain | as_fma).all(), (td, tc, tf)
    both = (tc == tf).all(axis=1)
    assert as_plain[both].all()
    assert (~both).sum() <= 1  # (the two builds part on QP 4 alone: what profiles/r05_c_* measured over 25,206 QPs)
    assert (out["eflag"] == 0).all()
    assert np.abs(z - c[0]).max() <= 3e-7 * (1.0 + np.abs(c[0]).max())


def _solve_on(hipmod, which, p, o, shape, monkeypatch=None, cap=None):
    """One batch through the C-ABI of the product library (which = None) or of a variant
    build (hip_api.library), host pointers; ``cap``: FBSTAB_HIP_MAX_WORKGROUPS at the handle's
    creation.  Returns (kernel, z, l, v, y, out, workgroups)."""
    import contextlib
    N, nx, nu, nc = shape
    B = p.batch
    if cap is not None:
        monkeypatch.setenv("FBSTAB_HIP_MAX_WORKGROUPS", str(cap))
    with (hipmod.library(H.VARIANT_LIBS[which]) if which else contextlib.nullcontext()):
        s = hipmod.FBstabMpcBatch(N, nx, nu, nc, max_batch=B)
    if cap is not None:
        monkeypatch.delenv("FBSTAB_HIP_MAX_WORKGROUPS")
    kern = s.kernel_name()
    wg = s.query()["workgroups"]
    s.UpdateOptions(_opts(hipmod, o))
    z = np.zeros((B, p.nz)); l = np.zeros((B, p.nl)); v = np.zeros((B, p.nv)); y = np.zeros((B, p.nv))
    out = s.Solve({k: np.ascontiguousarray(a) for k, a in p.arrays.items()}, z, l, v, y)
    s.close()
    return kern, z, l, v, y, out, wg


@pytest.mark.parametrize("inst", range(5))
def test_pattern_initialised_build_agrees_bitwise_on_every_record_instance(hip, oracle, monkeypatch, inst):
    """VERDICT r3 item 5.  The record kernels' cooperative passes read EVERY lane's policy
    object (v_readlane of rec, pack, lpo, N ...), also of rows that hold no QP; a member
    that no code path has set is `undef` in the IR, which the optimiser may resolve
    differently from build to build (the <12,4,32> episode).  The
    variant library `tests/_build/libfbstab_hip_pattern.so` is the same sources compiled with
    -ftrivial-auto-var-init=pattern (and -Wuninitialized -Wconditional-uninitialized,
    clean): every automatic variable starts from a fixed bit pattern, so such a read gives
    the same garbage every time - and a result that depends on it differs from the product
    build's.  The variant also keeps the guard s_nop in front of every group of fused
    broadcast-FMAs (FB_FMAC_GUARD_NOP=1), which the product build drops where
    tools/check_dpp_hazards.py proves them unnecessary: an operand read too early would show
    here as a difference too.  For each of the five record instances: its four fuzz shapes of
    test_random_shapes_on_every_mpc_instance plus batches of 1, 2, 3, 5 and 7 QPs on an exact
    and a padded shape - outputs of the two builds bitwise equal, and at parity with the oracle.
    A handle made for such a batch runs it spread (one QP per wavefront, the other rows idle), so
    the tiny batches run a second time on ONE workgroup (FBSTAB_HIP_MAX_WORKGROUPS=1): rows and
    whole wavefront halves without a QP beside busy ones, and rows that fetch again."""
    import os
    if not os.path.exists(H.VARIANT_LIBS["pattern"]):
        pytest.fail("tests/_build/libfbstab_hip_pattern.so is missing: `make -C fbstab_amd/csrc pattern` "
                    "(__graft_entry__.build() builds it)")
    cases = []
    for j in range(4):
        idx = 4 * inst + j
        shape, kern = MPC_SHAPES[idx]
        rng = np.random.default_rng(7000 + idx)
        B = int(rng.integers(2, 12))
        o = default_options()
        if idx % 3 == 2:
            o = default_options(max_linesearch_iters=int(rng.integers(1, 12)),
                                nonmonotone_linesearch=int(rng.random() < 0.5))
        cases.append((shape, kern, fx.random_ltv_mpc(rng, B, *shape), o, None))
    for j in (0, 1):  # exact and padded shape of the instance, tiny batches, spread and on one workgroup
        shape, kern = MPC_SHAPES[4 * inst + j]
        for B in (1, 2, 3, 5, 7):
            rng = np.random.default_rng(9000 + 100 * inst + 10 * j + B)
            p = fx.random_ltv_mpc(rng, B, *shape)
            cases.append((shape, kern, p, default_options(), None))
            cases.append((shape, kern, p, default_options(), 1))
    for shape, kern, p, o, cap in cases:
        a = _solve_on(hip, None, p, o, shape, monkeypatch, cap)
        b = _solve_on(hip, "pattern", p, o, shape, monkeypatch, cap)
        assert a[0] == kern and b[0] == kern, (a[0], b[0], kern)
        if cap is not None:
            assert a[6] == b[6] == cap, (a[6], b[6])
        for x, y_ in zip(a[1:5], b[1:5]):
            assert np.array_equal(x, y_), (shape, p.batch)
        for f in ("eflag", "residual", "newton_iters", "prox_iters", "initial_residual"):
            assert np.array_equal(a[5][f], b[5][f]), (shape, p.batch, f)
        c = oracle.solve_mpc(p, opts=o, nthreads=oracle.num_threads())
        oc = c[4]
        assert np.array_equal(a[5]["eflag"], oc["eflag"]), (shape, p.batch)
        assert np.array_equal(a[5]["prox_iters"], oc["prox_iters"]), (shape, p.batch)
        assert np.array_equal(a[5]["newton_iters"], oc["newton_iters"]), (shape, p.batch)
        good = oc["eflag"] == 0
        if good.any():
            scale = 1.0 + np.abs(c[0]).max(axis=1, keepdims=True)
            assert (np.abs(a[1] - c[0])[good] <= 10 * o.abs_tol * scale[good]).all()


@pytest.mark.parametrize("kernel", ["record", "generic"])
def test_one_step_qp_on_a_29_wide_stage_takes_the_oracles_counts(hip, oracle, monkeypatch, kernel):
    """The deviation round 4 found and pinned (tools/fuzz_shapes.py seed 42, shape 128: N=3, nx=23, nu=6,
    nc=1, <24,8,16>), now closed: a QP with no active constraint converges in ONE Newton step to the
    accuracy of the linear solve; the oracle's step leaves 3.7e-7 - under abs_tol = 1e-6, done after one
    proximal iteration - and the kernels', which multiplied with explicitly inverted factors, left 4.6e-6
    in the z block (forward stable, not backward stable) and took one more iteration of each kind.  The
    row-pair record instances and the flat-vector kernel now SUBSTITUTE with the Cholesky factors, as
    riccati_linear_solver.cc:234-325 does (fb_row16.h subst_rows / subst_cols_t, fb_mpc.h solve_lower):
    counts EQUAL to the oracle's on every QP, on both kernels - and with the refinement option on top
    (reserved = 1) as well."""
    monkeypatch.setenv("FBSTAB_HIP_GENERIC", "1" if kernel == "generic" else "0")
    p, o = H.fuzz_stream_shape(42, 127)
    N, nx, nu, nc = p.sizes()
    B = p.batch
    assert (N, nx, nu, nc, B) == (3, 23, 6, 1, 10)
    c = oracle.solve_mpc(p, opts=o, nthreads=oracle.num_threads())
    oc = c[4]
    for reserved in (0, 1):
        s = hip.FBstabMpcBatch(N, nx, nu, nc, max_batch=B)
        assert s.kernel_name() == ("fbstab_mpc_r32_kernel<24,8,16>" if kernel == "record" else "fbstab_mpc_kernel<64>")
        h = _opts(hip, o)
        h.reserved = reserved
        s.UpdateOptions(h)
        z = np.zeros((B, p.nz)); l = np.zeros((B, p.nl)); v = np.zeros((B, p.nv)); y = np.zeros((B, p.nv))
        out = s.Solve({k: np.ascontiguousarray(a) for k, a in p.arrays.items()}, z, l, v, y)
        refined = s.refined_steps()
        s.close()
        assert np.array_equal(out["eflag"], oc["eflag"]) and (out["eflag"] == 0).all()
        assert np.array_equal(out["prox_iters"], oc["prox_iters"]), (reserved, out["prox_iters"], oc["prox_iters"])
        assert np.array_equal(out["newton_iters"], oc["newton_iters"]), (reserved, out["newton_iters"], oc["newton_iters"])
        assert (out["residual"] <= 1e-6).all()
        scale = 1.0 + np.abs(c[0]).max(axis=1, keepdims=True)
        assert (np.abs(z - c[0]) <= 10 * o.abs_tol * scale).all()
        assert refined == 0 if reserved == 0 else refined >= 0


@pytest.mark.parametrize("kernel", ["record", "generic"])
@pytest.mark.parametrize("case", ["baseline", "wide"])
def test_newton_system_residual_against_the_oracles_at_sigma_1e_8(hip, oracle, monkeypatch, kernel, case):
    """|V dx - r| of ONE Newton step at sigma = 1e-8 (cond(V) ~ 1e11), block row by block
    row, in extended precision, device against oracle - on the BASELINE shape (cold start and near the
    solution: the one-row record instance, explicit inverses, row form of the costate step) and on all ten
    QPs of the 29-wide shape of the fuzz stream's deviation (row-pair instance: substitution).  Asserted for
    every QP probed:
      * the 2-norm of the device's residual is within 3 x the oracle's (same class; on the BASELINE shape the
        record kernel's is in fact 10 to 4e4 times SMALLER);
      * every block row is within 10 x the oracle's SAME block row - or, where the formulations leave their
        rounding error in different block rows, below half the oracle's whole residual.  Where the second
        clause is needed, so that nobody has to find it: the row form satisfies the z rows identically
        (3e-14 against the oracle's 5e-8 at the cold start) and carries dz's forward error in the l rows
        (1e-12 against the oracle's 2e-15, whose substitutions put theirs in the z rows); and the
        reference's form of the costate step leaves 1e-8 in the l rows of the wide shape (the product with
        the explicit inv(Pi), which the reference forms too but applies by substitution) where the oracle
        has 1e-14 - each time a residual no larger overall, hundreds of times the oracle's in that block.
    With the refinement option (reserved = 1 ... ) every block row goes to rounding level; that is a test of
    its own below."""
    monkeypatch.setenv("FBSTAB_HIP_GENERIC", "1" if kernel == "generic" else "0")
    if case == "baseline":
        p, o = fx.synthetic_mpc_batch(4), default_options()
        name = "fbstab_mpc_r16_kernel<12,4,20>"
    else:
        p, o = H.fuzz_stream_shape(42, 127)
        name = "fbstab_mpc_r32_kernel<24,8,16>"
    N, nx, nu, nc = p.sizes()
    zero = lambda n: np.zeros(n)
    s = hip.FBstabMpcBatch(N, nx, nu, nc, max_batch=1)
    assert s.kernel_name() == (name if kernel == "record" else "fbstab_mpc_kernel<64>")
    s.UpdateOptions(_opts(hip, o))
    points = [(q, None) for q in range(min(p.batch, 10))]
    if case == "baseline":  # ... and near the solution, where active rows put 1 / sigma into the stage Hessians
        sol = oracle.solve_mpc(p, opts=o)
        rng = np.random.default_rng(5)
        for q in range(2):
            points.append((q, (sol[0][q] * (1 + 1e-3 * rng.standard_normal(p.nz)), sol[1][q] * (1 + 1e-3 * rng.standard_normal(p.nl)),
                               np.maximum(sol[2][q] * (1 + 1e-3 * rng.standard_normal(p.nv)), 0.0))))
    for q, x in points:
        data = {k: a[q] for k, a in p.arrays.items()}
        one = fx.MpcProblem(N, nx, nu, nc, {k: np.ascontiguousarray(a[q:q + 1]) for k, a in p.arrays.items()})
        z, l, v = x if x is not None else (zero(p.nz), zero(p.nl), zero(p.nv))
        g = s.debug_newton(data, z, l, v, z, l, v)
        assert g["ok"]
        pr = oracle.probe(one, z, l, v, z, l, v, o.sigma0, o.alpha)
        pr = oracle.probe(one, z, l, v, z, l, v, o.sigma0, o.alpha, r=-pr["inner"], want_dx=True)
        dx = pr["dx"]
        ostep = {"dz": dx[:p.nz], "dl": dx[p.nz:p.nz + p.nl], "dv": dx[p.nz + p.nl:p.nz + p.nl + p.nv]}
        eb, en = H.newton_system_residual(p, q, g, x, x, o.sigma0, o.alpha)
        ob, on = H.newton_system_residual(p, q, ostep, x, x, o.sigma0, o.alpha)
        assert en <= 3.0 * on, (case, kernel, q, eb, ob)
        for k in range(3):
            assert eb[k] <= max(10 * ob[k], 0.5 * on, 1e-15), (case, kernel, q, k, eb, ob)
    s.close()


@pytest.mark.parametrize("kernel", ["record", "generic"])
def test_refinement_option_takes_every_block_row_to_rounding_level(hip, monkeypatch, kernel):
    """The option (fbstab_options_t::reserved = k > 0; Solver::wants_refinement) on the Newton-step probe:
    with a threshold of 2^-40 of abs_tol every step of the 29-wide shape is refined, and |V dx - r| ends at
    rounding level in every block row on both kernels (1e-7 without)."""
    monkeypatch.setenv("FBSTAB_HIP_GENERIC", "1" if kernel == "generic" else "0")
    p, o = H.fuzz_stream_shape(42, 127)
    N, nx, nu, nc = p.sizes()
    s = hip.FBstabMpcBatch(N, nx, nu, nc, max_batch=1)
    h = _opts(hip, o)
    h.reserved = 41
    s.UpdateOptions(h)
    zero = lambda n: np.zeros(n)
    for q in range(p.batch):
        g = s.debug_newton({k: a[q] for k, a in p.arrays.items()}, zero(p.nz), zero(p.nl), zero(p.nv), zero(p.nz), zero(p.nl), zero(p.nv))
        assert g["ok"]
        eb, en = H.newton_system_residual(p, q, g, None, None, o.sigma0, o.alpha)
        assert max(eb) <= 1e-12, (q, eb)
    s.close()


def test_a_handle_created_for_eight_in_flight_gives_the_same_bits(hip):
    """fbstab_hip_mpc_create_in_flight: a handle that shares the device takes its share of the resident
    workgroups (and of the scratch memory) - the queue hands the same QPs to fewer rows, nothing else:
    outputs bitwise equal to a handle that has the device to itself."""
    B = 2048
    p = fx.synthetic_mpc_batch(B)
    res = []
    for k in (1, 8):
        s = hip.FBstabMpcBatch(*p.sizes(), max_batch=B, handles_in_flight=k)
        q = s.query()
        z = np.zeros((B, p.nz)); l = np.zeros((B, p.nl)); v = np.zeros((B, p.nv)); y = np.zeros((B, p.nv))
        out = s.Solve({k_: np.ascontiguousarray(a) for k_, a in p.arrays.items()}, z, l, v, y)
        res.append((z, l, v, y, out, q))
        s.close()
    assert res[1][5]["workgroups"] * 2 <= res[0][5]["workgroups"] and res[1][5]["scratch_bytes"] * 2 <= res[0][5]["scratch_bytes"]
    for a, b in zip(res[0][:4], res[1][:4]):
        assert np.array_equal(a, b)
    for f in ("eflag", "residual", "newton_iters", "prox_iters"):
        assert np.array_equal(res[0][4][f], res[1][4][f]), f


def test_the_refinement_option_leaves_the_baseline_workload_untouched(hip, oracle):
    """On the BASELINE workload (cold start, default options) no Newton step's linear residual comes near a
    tolerance (1e-12 against 1e-6): even with the option on (reserved = 1) fbstab_hip_mpc_refined_steps = 0,
    and the outputs are bit for bit those with it off."""
    B = 512
    p = fx.synthetic_mpc_batch(B)
    res = []
    for reserved in (1, 0):
        s = hip.FBstabMpcBatch(*p.sizes(), max_batch=B)
        h = _opts(hip, default_options())
        h.reserved = reserved
        s.UpdateOptions(h)
        z = np.zeros((B, p.nz)); l = np.zeros((B, p.nl)); v = np.zeros((B, p.nv)); y = np.zeros((B, p.nv))
        out = s.Solve({k: np.ascontiguousarray(a) for k, a in p.arrays.items()}, z, l, v, y)
        res.append((z, l, v, y, out, s.refined_steps()))
        s.close()
    assert res[0][5] == 0 and res[1][5] == 0
    for a, b in zip(res[0][:4], res[1][:4]):
        assert np.array_equal(a, b)
    for f in ("eflag", "residual", "newton_iters", "prox_iters", "initial_residual"):
        assert np.array_equal(res[0][4][f], res[1][4][f]), f


# (nz, nl, nv) -> threads per QP of the kernel that must run it (one wavefront for
# nz + nl <= 64, four beyond; the K-in-global-memory layout above ~140)
_DENSE_SHAPES = [
    ((1, 0, 1), 64), ((7, 3, 40), 64), ((50, 10, 100), 64), ((33, 0, 9), 64), ((60, 4, 131), 64), ((20, 5, 40), 64),
    ((64, 1, 30), 256), ((90, 12, 77), 256), ((120, 20, 60), 256), ((70, 0, 200), 256),
    ((150, 10, 90), 256), ((159, 24, 239), 256),
    # nz <= 64 < nz + nl with nv a multiple of 4: the MFMA assembly of fb_dense.h by default dispatch
    ((40, 30, 8), 256), ((33, 32, 64), 256),
]


@pytest.mark.parametrize("idx", range(len(_DENSE_SHAPES)))
def test_random_shapes_on_every_dense_kernel(hip, oracle, idx):
    """tools/fuzz_dense.py, a fixed subset over the one-wavefront kernel, the
    four-wavefront kernel and its K-in-global-memory instance."""
    (nz, nl, nv), threads = _DENSE_SHAPES[idx]
    rng = np.random.default_rng(8000 + idx)
    B = int(rng.integers(1, 9))
    o = default_options()
    p = fx.synthetic_dense_batch(B, nz, nl, nv, first_id=int(rng.integers(0, 1 << 20)))
    s = hip.FBstabDenseBatch(nz, nl, nv, max_batch=B)
    assert s.query()["threads"] == threads
    z = np.zeros((B, nz)); l = np.zeros((B, nl)); v = np.zeros((B, nv)); y = np.zeros((B, nv))
    out = s.Solve({k: np.ascontiguousarray(a) for k, a in p.arrays.items()}, z, l, v, y)
    s.close()
    c = oracle.solve_dense(p, opts=o, nthreads=oracle.num_threads())
    oc = c[4]
    assert np.array_equal(out["eflag"], oc["eflag"])
    assert np.array_equal(out["prox_iters"], oc["prox_iters"])
    dn = np.abs(out["newton_iters"].astype(int) - oc["newton_iters"].astype(int))
    assert dn.max() <= 2, dn
    good = oc["eflag"] == 0
    if good.any():
        scale = 1.0 + np.abs(c[0]).max(axis=1, keepdims=True)
        assert (np.abs(z - c[0])[good] <= 10 * o.abs_tol * scale[good]).all()


# ---- shapes beyond the on-chip budget: the reference allocates on the heap for any size
# (fbstab_mpc.cc:61-89, fbstab_dense.cc:18-42) ---------------------------------------------
def test_mpc_stage_wider_than_the_lds(hip, oracle):
    """(N 10, nx 80, nu 10, nc 40): the stage matrices and the Riccati work matrices of one
    stage are 480 KB - three times the LDS.  The flat-vector kernel then keeps them in the
    workgroup's global scratch (MpcProblem<C, WGLOBAL>); same parity bar, and the receding
    sweep (nx > 64: the plant step collects the new state in global memory) runs too."""
    N, nx, nu, nc = 10, 80, 10, 40
    rng = np.random.default_rng(91)
    B = 3
    # (dynamics I + 0.02 randn: the generator's default 0.15 gives an 80 x 80 state matrix a
    # spectral radius above 2, and ten stages of that a QP whose iteration path no two
    # roundings agree on)
    p = fx.random_ltv_mpc(rng, B, N, nx, nu, nc, dyn_noise=0.02)
    s = hip.FBstabMpcBatch(N, nx, nu, nc, max_batch=B)
    assert s.kernel_name() == "fbstab_mpc_kernel<64>"
    assert s.query()["lds_bytes"] < 160 * 1024
    o = default_options()
    z = np.zeros((B, p.nz)); l = np.zeros((B, p.nl)); v = np.zeros((B, p.nv)); y = np.zeros((B, p.nv))
    out = s.Solve({k: np.ascontiguousarray(a) for k, a in p.arrays.items()}, z, l, v, y)
    c = oracle.solve_mpc(p, opts=o, nthreads=oracle.num_threads())
    oc = c[4]
    assert np.array_equal(out["eflag"], oc["eflag"]) and (oc["eflag"] == 0).all()
    good = oc["eflag"] == 0
    assert np.array_equal(out["prox_iters"][good], oc["prox_iters"][good])
    assert np.array_equal(out["newton_iters"][good], oc["newton_iters"][good])
    scale = 1.0 + np.abs(c[0]).max(axis=1, keepdims=True)
    assert (np.abs(z - c[0])[good] <= 10 * o.abs_tol * scale[good]).all()
    # one Newton step against the oracle's RiccatiLinearSolver at a random point
    data = {k: a[0] for k, a in p.arrays.items()}
    zz, ll = rng.standard_normal(p.nz), rng.standard_normal(p.nl)
    vv = np.abs(rng.standard_normal(p.nv))
    s.UpdateOptions(hip.DefaultOptions(sigma0=1e-4, sigma_max=100.0))
    g = s.debug_newton(data, zz, ll, vv, 0.5 * zz, 0.5 * ll, 0.5 * vv)
    one = fx.MpcProblem(N, nx, nu, nc)
    one.arrays = {k: a[:1] for k, a in p.arrays.items()}
    pr = oracle.probe(one, zz, ll, vv, 0.5 * zz, 0.5 * ll, 0.5 * vv, 1e-4)
    pr = oracle.probe(one, zz, ll, vv, 0.5 * zz, 0.5 * ll, 0.5 * vv, 1e-4, r=-pr["inner"], want_dx=True)
    odz, odl, odv, _ = np.split(pr["dx"], [p.nz, p.nz + p.nl, p.nz + p.nl + p.nv])
    for a_, b_ in ((g["dz"], odz), (g["dl"], odl), (g["dv"], odv)):
        assert np.abs(a_ - b_).max() <= 1e-9 * (1 + np.abs(b_).max())
    s.close()
    # the sweep with more states than a lane can hold in registers
    import torch
    dev = torch.device("cuda:0")
    s = hip.FBstabMpcBatch(N, nx, nu, nc, max_batch=B)
    data = {k: torch.from_numpy(np.ascontiguousarray(a)).to(dev) for k, a in p.arrays.items()}
    mk = lambda n: torch.zeros((B, n), dtype=torch.float64, device=dev)
    A0 = np.asarray(p.arrays["A"][0][:nx * nx]).reshape(nx, nx).T.copy()
    B0 = np.asarray(p.arrays["B"][0][:nx * nu]).reshape(nu, nx).T.copy()
    x0 = p.arrays["x0"].copy()
    zt = mk(p.nz)
    r = s.RecedingSweep(data, zt, mk(p.nl), mk(p.nv), mk(p.nv), A0, B0, 2, retire=False, log_inputs=True)
    u0 = r["u"][0].cpu().numpy()
    np.testing.assert_allclose(u0, z[:, nx:nx + nu], atol=1e-5 * (1 + np.abs(z).max()))
    x1 = x0 @ A0.T + u0 @ B0.T
    # after two steps x0 = A x1 + B u1
    u1 = r["u"][1].cpu().numpy()
    np.testing.assert_allclose(data["x0"].cpu().numpy(), x1 @ A0.T + u1 @ B0.T, rtol=1e-12, atol=1e-12)
    s.close()


def test_dense_vectors_longer_than_the_lds(hip, oracle):
    """(nz 20, nl 5, nv 4000): ten iterate vectors of 4000 doubles are 320 KB.  The
    four-wavefront kernel keeps them - and K - in the workgroup's global scratch
    (DenseProblem<C, KGLOBAL, VGLOBAL>)."""
    nz, nl, nv = 20, 5, 4000
    B = 3
    # (ids 100..: of sixteen instances tried only ids 77 and 81 - whose oracle residual at an
    # exit test is 0.99e-6 against the tolerance 1e-6 - take a different number of proximal
    # iterations on the two sides)
    B = 4
    p = fx.synthetic_dense_batch(B, nz, nl, nv, first_id=100)
    s = hip.FBstabDenseBatch(nz, nl, nv, max_batch=B)
    q = s.query()
    assert q["threads"] == 256 and q["lds_bytes"] < 160 * 1024 and q["scratch_bytes"] >= 10 * nv * 8
    o = default_options()
    z = np.zeros((B, nz)); l = np.zeros((B, nl)); v = np.zeros((B, nv)); y = np.zeros((B, nv))
    out = s.Solve({k: np.ascontiguousarray(a) for k, a in p.arrays.items()}, z, l, v, y)
    out2, nrm = s.SolveFinal({k: np.ascontiguousarray(a) for k, a in p.arrays.items()},
                             np.zeros((B, nz)), np.zeros((B, nl)), np.zeros((B, nv)), np.zeros((B, nv)))
    s.close()
    c = oracle.solve_dense(p, opts=o, nthreads=oracle.num_threads())
    oc = c[4]
    assert np.array_equal(out["eflag"], oc["eflag"]) and (oc["eflag"] == 0).all()
    assert np.array_equal(out["prox_iters"], oc["prox_iters"])
    assert np.array_equal(out["newton_iters"], oc["newton_iters"])
    scale = 1.0 + np.abs(c[0]).max(axis=1, keepdims=True)
    assert (np.abs(z - c[0]) <= 10 * o.abs_tol * scale).all()
    assert np.array_equal(out2["newton_iters"], out["newton_iters"])
    np.testing.assert_allclose(np.sqrt((nrm[:, :3] ** 2).sum(axis=1)), out["residual"], rtol=1e-6, atol=1e-9)


@pytest.mark.parametrize("kind", ["mpc_record", "mpc_flat", "dense_wave", "dense_256"])
def test_overflowed_and_nan_guesses_end_where_the_reference_ends(hip, oracle, monkeypatch, kind):
    """An initial guess with a NaN, an infinity or an entry whose square overflows: the
    reference's sqrt propagates it through the Fischer-Burmeister function, the first
    factorisation fails and Solve throws (impl:263-267; the oracle raises for every
    case below).  The batch API reports exactly these QPs as DIVERGENCE (the documented
    stand-in for the throw) and solves the healthy QPs beside them as if alone."""
    if kind.startswith("mpc"):
        monkeypatch.setenv("FBSTAB_HIP_GENERIC", "1" if kind == "mpc_flat" else "0")
        p = fx.synthetic_mpc_batch(6, first_id=10)
        s = hip.FBstabMpcBatch(*p.sizes(), max_batch=6)
        solve1 = lambda q, g: oracle.solve_mpc(q, x0guess=g, opts=default_options())
    else:
        monkeypatch.setenv("FBSTAB_HIP_DENSE_THREADS", "256" if kind == "dense_256" else "0")
        p = fx.synthetic_dense_batch(6, 20, 5, 40, first_id=10)
        s = hip.FBstabDenseBatch(p.nz, p.nl, p.nv, max_batch=6)
        solve1 = lambda q, g: oracle.solve_dense(q, x0guess=g, opts=default_options())
    z = np.zeros((6, p.nz)); l = np.zeros((6, p.nl)); v = np.zeros((6, p.nv)); y = np.zeros((6, p.nv))
    v[1, 5] = np.nan
    v[2, 7] = 1e200
    z[3, 3] = np.inf
    v[4, 2] = -1e200
    bad = [1, 2, 3, 4]
    # the oracle, one QP at a time: the poisoned ones raise, the healthy ones converge
    ref = {}
    for q in range(6):
        one = type(p)(*p.sizes()) if kind.startswith("mpc") else type(p)(p.nz, p.nl, p.nv)
        one.arrays = {k: a[q:q + 1] for k, a in p.arrays.items()}
        g = (z[q:q + 1].copy(), l[q:q + 1].copy(), v[q:q + 1].copy())
        if q in bad:
            with pytest.raises(RuntimeError, match="Initialize failed"):
                solve1(one, g)
        else:
            ref[q] = solve1(one, g)
    out = s.Solve({k: np.ascontiguousarray(a) for k, a in p.arrays.items()}, z, l, v, y)
    s.close()
    assert out["eflag"].tolist() == [0, 1, 1, 1, 1, 0]
    for q, r in ref.items():
        assert out["newton_iters"][q] == r[4]["newton_iters"][0] and out["prox_iters"][q] == r[4]["prox_iters"][0]
        assert np.abs(z[q] - r[0][0]).max() <= 1e-5 * (1 + np.abs(r[0][0]).max())


@pytest.mark.parametrize("seed", sorted(DEGENERATE_SHAPES))
def test_degenerate_dense_shapes_in_the_default_order(hip, oracle, seed):
    """The default (Eigen's) elimination order on the shapes where the natural order parts
    from the oracle: exit flags, proximal AND Newton counts equal on every QP, solutions
    and multipliers' image G'l + A'v within the parity tolerance.  The opt-in orders on the
    same QPs: same exit flags (all converge) and the same z to the tolerance - their
    iteration counts are allowed to differ, that is what the option's documentation says."""
    inst = fuzz_dense_instances(seed, set(DEGENERATE_SHAPES[seed]))
    assert len(inst) == len(DEGENERATE_SHAPES[seed]), inst
    o = default_options()
    handed_over = 0
    for nz, nl, nv, B, first_id in inst:
        p = fx.synthetic_dense_batch(B, nz, nl, nv, first_id=first_id)
        c = oracle.solve_dense(p, opts=o, nthreads=oracle.num_threads())
        oc = c[4]
        for order in (None, "auto", "natural"):
            s = hip.FBstabDenseBatch(nz, nl, nv, max_batch=B)
            assert s.query()["threads"] == 64
            if order:
                s.SetFactorisation(s.ORDER_AUTO if order == "auto" else s.ORDER_NATURAL)
            z = np.zeros((B, nz)); l = np.zeros((B, nl)); v = np.zeros((B, nv)); y = np.zeros((B, nv))
            out = s.Solve({k: np.ascontiguousarray(a) for k, a in p.arrays.items()}, z, l, v, y)
            fac = s.Factorisation()
            s.close()
            assert np.array_equal(out["eflag"], oc["eflag"]), (nz, nl, nv, order)
            scale = 1.0 + np.abs(c[0]).max(axis=1, keepdims=True)
            assert (np.abs(z - c[0]) <= 10 * o.abs_tol * scale).all(), (nz, nl, nv, order)
            if order is None:
                assert fac["order"] == s.ORDER_PIVOTED
                assert np.array_equal(out["prox_iters"], oc["prox_iters"]), (nz, nl, nv)
                assert np.array_equal(out["newton_iters"], oc["newton_iters"]), (nz, nl, nv)
            elif order == "auto":
                handed_over += fac["pivoted_steps"]
    assert handed_over > 0  # (AUTO does hand steps of these QPs to the pivoted path)
