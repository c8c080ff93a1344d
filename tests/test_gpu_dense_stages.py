"""The four-wavefront dense policy (fbstab_amd/csrc/fb_dense.h) stage by stage on the device, on every layout
DenseLayout::init can choose: each stage runs alone in the probe library (tests/kernels/dense_probe.hip through
tests/dense_probe.py) and is held to an extended-precision reference by the first-order rounding bounds of
tests/dense_rules.py - the rules, inputs and shapes that tests/test_dense_rules_cpu.py shows to pass a float64
restatement and the real header on one host thread, to catch seeded defects, and to sit on the paths their names
say (the path map from the compiled header; the probe reports the layout it runs and that is asserted here too).
Three QPs per shape, sigma = 1 and 1e-8, the step's own Gamma from 1e-12 up to min(1e8, ~ 1 / sigma) within a QP.
Each test prints the worst |error| / bound it saw (LABNOTES keeps the baseline)."""
import numpy as np
import pytest

from tests import dense_rules as dr
from tests import dense_wave_rules as wr
from tests.dense_probe import DenseProbe, SENTINEL

pytestmark = pytest.mark.gpu

PLACEMENT = {(0, 0): "lds", (1, 0): "kglobal", (1, 1): "vglobal"}


@pytest.fixture(scope="module")
def probe():
    assert SENTINEL == dr.SENTINEL_BITS
    return DenseProbe()


def _assert_all(rules, where):
    print("%s: %s" % (where, "  ".join("%s %.3f" % kv for kv in rules.items())))
    for rule, worst in rules.items():
        assert worst <= 1.0, (where, rule, worst)


def _path(probe, nz, nl, nv, want):
    """dense_rules.path_of on the layout the probe itself reports."""
    lay = probe.layout(nz, nl, nv, want)
    p = dr.path_of(lambda *a: lay, nz, nl, nv, lay["threads"])
    assert p["threads"] == lay["threads"]
    return p


def _key_of_case(shape, want):
    return next(k for k, shapes in dr.STEP_SHAPES.items() if k[0] == want and shape in shapes)


# ---- the step ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", dr.STEP_CASES, ids=str)
def test_newton_step(probe, case):
    """load_guess, residual, newton_step<false>: Gamma and rv / mu against their first-order bound, the assembly
    judged through the factors (|P K_ref P' - L D L'| within the assembly's plus the factorisation's bound), the
    solution's residual, adz, dv, wz, wl given the device's own dz, dl; what is exact by construction (nothing
    written above the diagonal on the ldlt_impl paths, the bookkeeping of ldlt_rows).  Once more with the strict upper
    triangle of the step's H set to NaN: no bit but wz's changes, on every assembly branch (wz = H dz + .. reads the
    full symmetric H, like the residual)."""
    shape, want = case
    path = _path(probe, *shape, want)
    assert dr.path_key(path) == _key_of_case(shape, want), path
    rows = path["factorisation"] == "rows"
    for sigma in dr.SIGMAS:
        d, xb = dr.step_inputs(*shape, sigma)
        got = probe.step(d, *xb, sigma, dr.ALPHA, want)
        _assert_all(dr.step_rules(d, xb, sigma, got, rows), ("step", shape, want, sigma))
        if shape[0] > 1:
            again = probe.step(d, *xb, sigma, dr.ALPHA, want, h_step=dr.with_nan_upper(d["H"]))
            for k in got:
                if k != "wz":
                    assert np.array_equal(dr._bits(got[k]), dr._bits(again[k])), (shape, sigma, k, "H's upper triangle was read")


@pytest.mark.parametrize("case", dr.STEP_CASES, ids=str)
def test_adjoint_step(probe, case):
    """dense_adjoint (newton_step<true>): rz, rl the seeds' bits, yb = -(g0 gv), rvm = yb / mu, and the third block
    row in the reference's order of operations, dv = (yb + g0 a) / mu; the rest as the plain step."""
    shape, want = case
    rows = _path(probe, *shape, want)["factorisation"] == "rows"
    for sigma in dr.SIGMAS:
        d, xb = dr.step_inputs(*shape, sigma, True)
        got = probe.step(d, *xb, sigma, dr.ALPHA, want, adjoint=True)
        _assert_all(dr.step_rules(d, xb, sigma, got, rows, adjoint=True), ("adjoint step", shape, want, sigma))


@pytest.mark.parametrize("case", dr.STEP_CASES, ids=str)
def test_products(probe, case):
    """y = b - A z of load_guess, rz and rl of residual, forcing_norm; and, where A is kept in LDS, that copy read
    back bit for bit through A_row_dot and A_col_dot on unit vectors (the odd leading dimension lda = nv | 1 and
    the e % nv, e / nv scatter of load_guess)."""
    shape, want = case
    path = _path(probe, *shape, want)
    d = dr.problem(*shape)
    got = probe.products(d, want)
    rules = dr.product_rules(d, got["y"], got["rz"], got["rl"])
    rules.update(dr.products_extra_rules(d, got, path["a_lds"]))
    assert ("A in LDS by rows" in rules) == (path["assembly"] != "global")
    _assert_all(rules, ("products", shape, want))


# ---- the factorisations on images ---------------------------------------------------------------------------------------
def _factor_cases():
    return [(name, n, nv, want) for name, cases in dr.FACTOR_CASES.items() for n, nv, want in cases]


def _check_images(probe, K, b, nv, want, rows, where, order=True):
    got = probe.factor(K, b, nv, want)
    assert (got["verdict"] == 1).all(), (where, got["verdict"])
    for q in range(K.shape[0]):
        rules = dr.image_rules(K[q], b[q], got, q, rows)
        if order:
            documented = dr.order_restated(K[q], rows, probe.layout(K.shape[1], 0, nv, want)["threads"])
            rules["order as documented"] = 0.0 if np.array_equal(got["perm"][q], documented) else np.inf
        _assert_all(rules, where + (q,))
    return got


@pytest.mark.parametrize("case", _factor_cases(), ids=str)
def test_factor_on_random_images(probe, case):
    """ldlt and ldlt_solve on quasi-definite images behind each variant: ldlt_rows (n <= 64), ldlt_impl at 256 threads
    (n = 129: the first step's search runs over more than one wavefront and hands over to the first half-way; 130:
    one more), at 64 threads, with K in global scratch (n = 257: more than one pivot candidate per thread), and with
    K in global scratch at n <= 64 (ldlt_solve_wave).  The factors reproduce K, the solution meets the solve rule,
    and the elimination order is bit for bit the float64 restatement's of the documented rule."""
    name, n, nv, want = case
    path = _path(probe, n, 0, nv, want)
    assert dr.path_key(path, False) == dr.FACTOR_PATHS[name], path
    K, b = dr.images(n)
    _check_images(probe, K, b, nv, want, path["factorisation"] == "rows", ("factor", name, n))


def test_the_search_hands_over_to_the_first_wavefront_at_64_candidates(probe):
    """n = 129 with the largest diagonal of step 64 at the LAST position, the 65th candidate: it is taken."""
    K, b = dr.handover_image()
    got = _check_images(probe, K, b, 4, 256, False, ("handover",))
    assert got["perm"][0][64] == 128


FAMILY_PATHS = dr.FAMILY_PATHS


@pytest.mark.parametrize("nv,want,rows", FAMILY_PATHS)
def test_factor_takes_ties_as_documented(probe, nv, want, rows):
    """The tied family.  The order asserted is the variant's documented one - ldlt_rows: largest UPDATED |diagonal|,
    a tie to the lowest row index; ldlt_impl: largest UPDATED |diagonal|, a tie to the first current position -
    neither of which is Eigen's on the whole family (printed per matrix)."""
    for n, img, rhs, name in dr.tied_images():
        K, b = img[:, :n, :n], rhs[:, :n]
        assert (_path(probe, n, 0, nv, want)["factorisation"] == "rows") == rows
        got = _check_images(probe, K, b, nv, want, rows, ("tied", name, nv, want))
        same = np.array_equal(dr.elimination_order(got["perm"][0], rows), dr.eigen_order(K[0]))
        print("tied '%s': the device's order %s Eigen's" % (name, "is" if same else "is NOT"))


@pytest.mark.parametrize("nv,want,rows", FAMILY_PATHS)
def test_factor_verdicts_on_singular_matrices_are_as_documented(probe, nv, want, rows):
    """The zero matrix, diag(1, 0), [[0, 1], [1, 0]], zero pivots over a non-zero column, a NaN diagonal (which the
    pre-check of `ldlt` reports false).  Neither variant looks at the column under an invalid pivot, where Eigen
    fails if it is not zero.  Asserted: the documented verdict, and that it is Eigen's wherever the column test is
    not what decides."""
    for n, img, name in dr.singular_images():
        K = img[None, :n, :n]
        eigen = dr.eigen_ldlt(img[:n, :n])["ok"]
        documented = bool(dr.factor_restated(K[0], np.zeros(n), rows)["verdict"][0])
        verdict = bool(probe.factor(K, np.zeros((1, n)), nv, want)["verdict"][0])
        print("singular '%s': Eigen %s, documented %s, device %s" % (name, eigen, documented, verdict))
        assert verdict == documented, name
        if wr.factor_restated(img, n)[0] == documented:  # (the column test does not decide)
            assert verdict == eigen, name


@pytest.mark.parametrize("nv,want,rows", FAMILY_PATHS)
def test_the_solve_takes_a_denormal_pivot_for_zero(probe, nv, want, rows):
    """A pivot of 1e-310 is valid for the factorisation and zero for the pseudo-inverse of D: its entry of the
    solution is exactly +0, the rest solves the rest."""
    n, img, rhs, j = dr.denormal_pivot_image()
    K, b = img[:, :n, :n], rhs[:, :n]
    got = probe.factor(K, b, nv, want)
    assert got["verdict"][0] == 1
    assert got["x"][0, j] == 0.0 and not np.signbit(got["x"][0, j])
    keep = [i for i in range(n) if i != j]
    order, L, D = dr.factors_of(got, 0, n, rows)
    assert D[list(order).index(j)] == 1e-310
    M = dr.abs_ldl(n, order, L, D)[np.ix_(keep, keep)]
    worst = wr.solve_rule(K[0][np.ix_(keep, keep)], n - 1, b[0][keep], got["x"][0][keep], M)
    _assert_all({"solve": worst}, ("denormal pivot", nv, want))


def test_ldlt_impl_on_larger_images_of_the_families(probe):
    """The same families inside n = 66 (ldlt_impl with ldlt_solve_impl, K in LDS): the image in the leading block,
    a graded positive diagonal smaller than its pivots behind it."""
    for n, img, rhs, name in dr.tied_images():
        K = dr.embed(img[0], n, 66)[None]
        b = np.concatenate([rhs[:, :n], np.ones((1, 66 - n))], axis=1)
        _check_images(probe, K, b, 4, 256, False, ("tied in 66", name))
    n, img, rhs, j = dr.denormal_pivot_image()
    base = np.array(img[0])
    base[j, j] = 1.0  # (so that the padding is graded below the image's normal pivots, not below the denormal one)
    K = dr.embed(base, n, 66)[None]
    K[0, j, j] = 1e-310
    b = np.concatenate([rhs[:, :n], np.ones((1, 66 - n))], axis=1)
    got = probe.factor(K, b, 4, 256)
    assert got["verdict"][0] == 1 and got["x"][0, j] == 0.0 and not np.signbit(got["x"][0, j])
    nan = dr.embed(dr.singular_images()[4][1], 5, 66)[None]
    assert probe.factor(nan, np.zeros((1, 66)), 4, 256)["verdict"][0] == 0


# ---- feasibility ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(zip(dr.FEASIBILITY_CASES, dr.FEASIBILITY_PLACEMENTS)), ids=str)
def test_feasibility_classes(probe, case):
    """One constructed direction per class of full_feasibility.cc:25-88, and the w <= 1e-14 guard, at one shape per
    placement: A in LDS, A in global memory, K in global scratch, the vectors there too, and 64 threads."""
    (shape, want), (placement, a_lds) = case
    lay = probe.layout(*shape, want)
    assert (PLACEMENT[(lay["k_global"], lay["v_global"])], lay["a_lds"], lay["threads"]) == (placement, a_lds, want)
    d, dz, dl, dv, expected, names = dr.feasibility_cases(*shape)
    got = probe.feasibility(d, dz, dl, dv, 1e-8, want)
    for q, name in enumerate(names):
        assert dr.feasibility_class(d, q, dz[q], dl[q], dv[q], 1e-8) == expected[q], (shape, name)
        assert got[q] == expected[q], (shape, name, got)
