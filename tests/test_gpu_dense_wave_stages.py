"""The one-wavefront dense policy (fbstab_amd/csrc/fb_dense_wave.h) stage by stage on the device: each stage runs
alone in the probe library (tests/kernels/dense_wave_probe.hip through tests/dense_wave_probe.py) and is held to
an extended-precision reference by the first-order rounding bounds of tests/dense_wave_rules.py - the rules and
inputs that tests/test_dense_wave_rules_cpu.py shows to pass a plain float64 restatement and to catch seeded
defects.  The shapes sit on the edges of the code: nv = 1 (a branch of its own in the assembly's loads), odd nv at
the last row pair, the 16- and 32-row trips, nz at the 16-column tiles with nz + nl = 64, n = 1, the 16 / 32 / 48
block skips of the natural-order path, nv = 128 / 129 where the dv pass changes form, a denormal pivot in the
pseudo-inverse, tied diagonals.  Each test prints the worst |error| / bound it saw (LABNOTES keeps the baseline)."""
import numpy as np
import pytest

from tools import fixtures as fx
from tests import dense_wave_rules as dr
from tests import helpers as H
from tests.dense_wave_probe import DenseWaveProbe

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe():
    return DenseWaveProbe()


@pytest.fixture(scope="module")
def hip():
    from fbstab_amd import hip_api
    assert hip_api.load_library().fbstab_hip_device_count() >= 1
    return hip_api


def _assert_all(rules, where):
    print("%s: %s" % (where, "  ".join("%s %.3f" % kv for kv in rules.items())))
    for rule, worst in rules.items():
        assert worst <= 1.0, (where, rule, worst)


# ---- assemble ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", dr.ASSEMBLE_SHAPES)
def test_assemble(probe, shape):
    """K = [tril(H) mirrored + sigma I + A' Gamma A, G'; G, -sigma I] in the row registers and A' (rv / mu), sigma
    = 1 and 1e-8, Gamma from 1e-12 to 1e8 within a QP with the largest weights on the last rows; and again with
    the strict upper triangle of H set to NaN, which must not change a bit."""
    d = dr.problem(*shape)
    for sigma in dr.ASSEMBLE_SIGMAS:
        got = probe.assemble(d, sigma)
        _assert_all(dr.assemble_rules(d, sigma, *got), ("assemble", shape, sigma))
        poisoned = dict(d, H=dr.with_nan_upper(d["H"]))
        for a, b in zip(probe.assemble(poisoned, sigma), got):
            assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), (shape, sigma, "the upper triangle of H was read")


# ---- factor and substitute ---------------------------------------------------------------------------------------
def _factor_rules(probe, imgs, n, rhs, where, documented_order=False):
    verdict, ord_, dpiv, permv, Lg, x = probe.factor(imgs, n, rhs)
    assert (verdict == 1).all(), (where, verdict)
    for q in range(imgs.shape[0]):
        out = dr.factor_rules(imgs[q], n, ord_[q], dpiv[q], permv[q], Lg[q])
        if documented_order:
            want = dr.factor_restated(imgs[q], n, dr.DEVICE_AS_DOCUMENTED)[3]
            out["order as documented"] = 0.0 if np.array_equal(permv[q][:n], want[:n]) else np.inf
        if out["permutation"] == 0.0:
            perm, L, D = dr.factors_of(n, ord_[q], dpiv[q], permv[q], Lg[q])
            out["solve"] = dr.solve_rule(imgs[q], n, rhs[q], x[q], dr.abs_ldl(n, perm, L, D))
            assert not x[q, n:].any(), (where, q, "entries past n")
        _assert_all(out, where + (q,))


@pytest.mark.parametrize("n", dr.FACTOR_NS)
def test_factor_and_substitute_on_random_images(probe, n):
    """Pivoted LDL' and the substitutions on quasi-definite images: the elimination order is a permutation with its
    inverse, eliminated rows carry zero multipliers, the factors reproduce K and the solution's residual is within
    the solve rule.  (WHICH order is not asserted here: see test_factor_takes_ties_as_documented.)"""
    imgs, rhs = dr.random_images(n)
    _factor_rules(probe, imgs, n, rhs, ("factor", n))


def test_factor_takes_ties_as_documented(probe):
    """E diagonal with repeated entries and a larger one out of place, one and three coupling equality rows.  The
    order asserted is the one fb_dense_wave.h documents for `factor` - largest UPDATED |diagonal|, a tie to the
    lowest row index (tests/dense_wave_rules.DEVICE_AS_DOCUMENTED) - which is NOT Eigen's on these matrices
    (tests/test_dense_wave_rules_cpu.py holds the same restatement to Eigen's rule and shows it to fail there;
    LABNOTES: a kernel change to Eigen's rule was written, faulted on the GPU in another kernel that shares
    `factor`, and was taken out again).  The factors and the solution are held to the rules whatever the order."""
    for n, img, rhs, name in dr.tied_images():
        _factor_rules(probe, img, n, rhs, ("tied", name), documented_order=True)


def test_factor_verdicts_on_singular_matrices_are_as_documented(probe):
    """The zero matrix, diag(1, 0), [[0, 1], [1, 0]], zero pivots over a non-zero column, a NaN diagonal.  `factor`
    fails on a NaN diagonal and on a valid pivot behind an invalid one, as Eigen does; it does NOT look at the
    column under an invalid pivot, where Eigen fails if it is not zero (fb_dense_wave.h says so; sigma > 0 keeps
    every caller away from such a matrix).  Asserted: the documented verdict, and that it is Eigen's wherever the
    column test is not what decides."""
    for n, img, name in dr.singular_images():
        eigen = dr.eigen_ldlt(img[:n, :n])["ok"]
        documented = dr.factor_restated(img, n, dr.DEVICE_AS_DOCUMENTED)[0]
        verdict = bool(probe.factor(img[None], n, np.zeros((1, 64)))[0][0])
        print("singular '%s': Eigen %s, documented %s, device %s" % (name, eigen, documented, verdict))
        assert verdict == documented, name
        if dr.factor_restated(img, n)[0] == documented:  # (the column test does not decide)
            assert verdict == eigen, name


def test_substitute_takes_a_denormal_pivot_for_zero(probe):
    """A pivot of 1e-310 is valid for the factorisation and zero for the pseudo-inverse of D: its entry of the
    solution is 0, the rest solves the rest."""
    n, img, rhs, j = dr.denormal_pivot_image()
    verdict, ord_, dpiv, permv, Lg, x = probe.factor(img, n, rhs)
    assert verdict[0] == 1 and dpiv[0, j] == 1e-310 and ord_[0, j] == n - 1
    assert x[0, j] == 0.0 and not np.signbit(x[0, j])
    keep = [i for i in range(n) if i != j]
    perm, L, D = dr.factors_of(n, ord_[0], dpiv[0], permv[0], Lg[0])
    M = dr.abs_ldl(n, perm, L, D)
    worst = dr.solve_rule(dr.pad64(img[0][np.ix_(keep, keep)]), n - 1, rhs[0][keep], x[0][keep], M[np.ix_(keep, keep)])
    _assert_all({"solve": worst}, ("denormal pivot",))


# ---- the natural-order path ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", dr.STATIC_NS)
def test_factor_solve_static(probe, n):
    """The unrolled natural-order LDL' with both substitutions at every block skip (n <= 16, 32, 48 and above):
    the solution within the solve rule; a false verdict on a zero, denormal, infinite or NaN pivot; with the
    order chosen per step (order = 0) a false verdict on a pivot spread of spread_bits + 1 binades and a true one
    on spread_bits."""
    imgs, rhs = dr.static_images(n)
    for order in (2, 0):
        verdict, x = probe.static(imgs, n, rhs, order=order)
        assert (verdict == 1).all(), (n, order, verdict)
        for q in range(imgs.shape[0]):
            worst = dr.solve_rule(imgs[q], n, rhs[q], x[q], dr.natural_abs_ldl(imgs[q], n))
            _assert_all({"solve": worst}, ("static", n, order, q))
    imgs, rhs, names = dr.static_bad_pivots(n)
    verdict, _ = probe.static(imgs, n, rhs)
    assert not verdict.any(), (n, [nm for nm, v in zip(names, verdict) if v])
    for bits, order, expect in ((33, 0, False), (32, 0, True), (33, 2, True)):
        img, b = dr.static_spread_images(n, bits)
        verdict, _ = probe.static(img, n, b, order=order, spread_bits=32)
        assert bool(verdict[0]) == expect, (n, bits, order)


# ---- products and feasibility ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", dr.PRODUCT_SHAPES)
def test_products(probe, shape):
    """y = b - A z of load_guess and rz, rl of residual: row_dot, col_dot and A_col_dot with their remainders."""
    d = dr.problem(*shape)
    _assert_all(dr.product_rules(d, *probe.products(d)), ("products", shape))


@pytest.mark.parametrize("shape", [(17, 3, 33), (15, 0, 17)])
def test_feasibility_classes(probe, shape):
    """One constructed direction per class of full_feasibility.cc:25-88, and the w <= 1e-14 guard."""
    d, dz, dl, dv, expected, names = dr.feasibility_cases(*shape)
    got = probe.feasibility(d, dz, dl, dv, 1e-8)
    for q, name in enumerate(names):
        assert dr.feasibility_class(d, q, dz[q], dl[q], dv[q], 1e-8) == expected[q], (shape, name)
        assert got[q] == expected[q], (shape, name, got)


# ---- the whole step ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["default", "natural"])
@pytest.mark.parametrize("shape", dr.STEP_SHAPES)
def test_newton_step_residual_against_the_oracles(hip, oracle, shape, order):
    """One Newton step through fbstab_hip_dense_debug_newton at a random point, sigma = 1 and 1e-8, in the default
    and in the natural elimination order: |V dx - r| in extended precision (tests/helpers.newton_system_residual)
    within 3 x the oracle's own, the bar of the adjoint tests - a residual, not a forward error, so that the bar
    does not move with cond(K).  (1, 0, 1), (2, 1, 1): the smallest systems; (63, 1, 3): nz + nl = 64; nv = 128
    and 129: the two forms of the dv pass."""
    nz, nl, nv = shape
    p = fx.synthetic_dense_batch(1, nz, nl, nv, first_id=4100 + nv)
    s = hip.FBstabDenseBatch(nz, nl, nv, max_batch=1)
    if order == "natural":
        s.SetFactorisation(s.ORDER_NATURAL)
    rng = np.random.default_rng(11)
    z, l = rng.standard_normal(nz), rng.standard_normal(nl)
    v = np.abs(rng.standard_normal(nv))
    zb, lb, vb = 0.5 * z, 0.5 * l, 0.5 * v
    explicit = H.dense_explicit(p, 0)
    for sigma in (1.0, 1e-8):
        s.UpdateOptions(hip.DefaultOptions(sigma0=sigma, sigma_max=100.0))
        g = s.debug_newton({k: a[0] for k, a in p.arrays.items()}, z, l, v, zb, lb, vb)
        assert g["ok"]
        pr = oracle.probe(p, z, l, v, zb, lb, vb, sigma)
        dx = oracle.probe(p, z, l, v, zb, lb, vb, sigma, r=-pr["inner"], want_dx=True)["dx"]
        ostep = {"dz": dx[:nz], "dl": dx[nz:nz + nl], "dv": dx[nz + nl:nz + nl + nv]}
        eb, en = H.newton_system_residual(p, 0, g, (z, l, v), (zb, lb, vb), sigma, 0.95, explicit=explicit)
        ob, on = H.newton_system_residual(p, 0, ostep, (z, l, v), (zb, lb, vb), sigma, 0.95, explicit=explicit)
        print("step %s %s sigma %g: device %.3g (%s), oracle %.3g (%s)" % (shape, order, sigma, en, eb, on, ob))
        assert en <= 3.0 * on, (shape, order, sigma, eb, ob)
    s.close()
