"""The acceptance rules of tests/dense_wave_rules.py must have teeth.  A plain float64 numpy version of each
recurrence of fb_dense_wave.h (no lanes, no tiles, one rounding per operation) meets every rule on every input
the GPU tests use - if it did not, the DERIVATION of a bound would be wrong, not a kernel - and every seeded
defect breaks a rule.  The rules assert of themselves that they are not vacuous (bound <= 1e-5 of the largest
reference entry); the share of elimination steps that are only held to "close to the largest" is capped here.
Nothing in this file has seen a device."""
import numpy as np
import pytest

from tests import dense_wave_rules as dr


def _assert_all(rules, where):
    for rule, worst in rules.items():
        assert worst <= 1.0, (where, rule, worst)


# ---- assemble ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", dr.ASSEMBLE_SHAPES)
def test_assembly_restatement_meets_the_rules(shape):
    d = dr.problem(*shape)
    for sigma in dr.ASSEMBLE_SIGMAS:
        out = dr.assemble_rules(d, sigma, *dr.assemble_restated(d, sigma))
        print("assemble %s sigma %g: %s" % (shape, sigma, "  ".join("%s %.3f" % kv for kv in out.items())))
        _assert_all(out, (shape, sigma))
        # the strict upper triangle of H is never read
        got = dr.assemble_restated(d, sigma, H=dr.with_nan_upper(d["H"]))
        for a, b in zip(got, dr.assemble_restated(d, sigma)):
            assert np.array_equal(a, b)


def test_assembly_shapes_cover_every_pair_of_edges():
    shapes = set(dr.ASSEMBLE_SHAPES)
    for must in ((1, 0, 1), (64, 0, 1), (63, 1, 3), (16, 0, 16), (17, 3, 33)):
        assert must in shapes
    nzs = (1, 15, 16, 17, 33, 48, 49, 64)
    assert {s[0] for s in shapes} >= set(nzs) and {s[2] for s in shapes} >= set(dr.ASSEMBLE_NV)
    for nz in nzs:  # every nz with every nl class that exists for it
        kinds = {"0" if nl == 0 else ("1" if nl == 1 else "full") for z, nl, _ in shapes if z == nz and z + nl <= 64
                 and (nl in (0, 1) or z + nl == 64)}
        assert kinds >= ({"0"} if nz == 64 else ({"0", "1"} if nz == 63 else {"0", "1", "full"})), (nz, kinds)
    assert all(nz + nl <= 64 for nz, nl, _ in shapes)


@pytest.mark.parametrize("shape", [(63, 1, 3), (17, 3, 33), (16, 1, 49), (1, 0, 1), (64, 0, 131)])
def test_assembly_defects_break_a_rule(shape):
    d = dr.problem(*shape)
    for sigma in dr.ASSEMBLE_SIGMAS:
        got = dr.assemble_restated(d, sigma, defect=dr.Defect(drop_last_odd_row=True))
        assert max(dr.assemble_rules(d, sigma, *got).values()) > 1.0, (shape, sigma, "last odd row dropped")
        if shape[0] > 1:
            # (read from the wrong triangle of a symmetric H nothing changes: the input that tells is the one
            # whose upper triangle is not H's)
            got = dr.assemble_restated(d, sigma, H=dr.with_nan_upper(d["H"]), defect=dr.Defect(read_upper_h=True))
            assert max(dr.assemble_rules(d, sigma, *got).values()) > 1.0, (shape, sigma, "upper triangle read")


# ---- factor, substitute ----------------------------------------------------------------------------------------
def _factor_rules(img, n, b, defect=None):
    ok, ord_, dpiv, permv, Lg = dr.factor_restated(img, n, defect)
    assert ok
    out = dr.factor_rules(img, n, ord_, dpiv, permv, Lg)
    out["order"], share = dr.order_rule(img, n, permv)
    if out["permutation"] == 0.0:
        perm, L, D = dr.factors_of(n, ord_, dpiv, permv, Lg)
        x = dr.substitute_restated(n, b, ord_, dpiv, permv, Lg, defect)
        out["solve"] = dr.solve_rule(img, n, b, x, dr.abs_ldl(n, perm, L, D))
    return out, share


@pytest.mark.parametrize("n", dr.FACTOR_NS)
def test_factor_restatement_meets_the_rules_on_random_images(n):
    imgs, rhs = dr.random_images(n)
    for q in range(imgs.shape[0]):
        out, share = _factor_rules(imgs[q], n, rhs[q])
        print("factor n=%d qp %d: %s  close steps %.0f%%" % (n, q, "  ".join("%s %.3f" % kv for kv in out.items()), 100 * share))
        _assert_all(out, (n, q))
        assert share <= 0.10, (n, q, share)


def test_factor_restatement_meets_the_rules_on_the_tied_family():
    for n, img, rhs, name in dr.tied_images():
        out, share = _factor_rules(img[0], n, rhs[0])
        print("tied %s: %s" % (name, "  ".join("%s %.3f" % kv for kv in out.items())))
        _assert_all(out, name)
        assert share == 0.0, (name, share)
        klass = dr.eigen_ldlt(img[0][:n, :n])["klass"]
        assert klass.count("tie") >= 2, (name, klass)


def test_the_issue_example_eliminates_2_1_0_3():
    n, img, rhs, name = dr.tied_images()[0]
    assert name == "2 2 5 2 + 1"
    assert dr.eigen_ldlt(img[0][:n, :n])["order"][:4] == [2, 1, 0, 3]
    assert list(dr.factor_restated(img[0], n)[3][:4]) == [2, 1, 0, 3]
    assert list(dr.factor_restated(img[0], n, dr.Defect(lowest_index_tie=True))[3][:4]) == [2, 0, 1, 3]


def test_singular_verdicts_are_eigens():
    expect = {"zero matrix": True, "diag(1, 0)": True, "[[0, 1], [1, 0]]": False,
              "zero pivots over a non-zero column, behind valid pivots": False,
              "NaN on the diagonal of a full matrix": False}
    for n, img, name in dr.singular_images():
        e = dr.eigen_ldlt(img[:n, :n])["ok"]
        assert e == expect[name], (name, e)
        assert dr.factor_restated(img, n)[0] == e, name
    # the defect: an invalid pivot over a non-zero column passes
    passed = [name for n, img, name in dr.singular_images()
              if dr.factor_restated(img, n, dr.Defect(no_column_check=True))[0] and not expect[name]]
    assert "[[0, 1], [1, 0]]" in passed


def test_denormal_pivot_is_zero_for_the_pseudo_inverse():
    n, img, rhs, j = dr.denormal_pivot_image()
    ok, ord_, dpiv, permv, Lg = dr.factor_restated(img[0], n)
    assert ok and dpiv[j] == 1e-310 and ord_[j] == n - 1
    x = dr.substitute_restated(n, rhs[0], ord_, dpiv, permv, Lg)
    assert x[j] == 0.0
    keep = [i for i in range(n) if i != j]
    perm, L, D = dr.factors_of(n, ord_, dpiv, permv, Lg)
    M = dr.abs_ldl(n, perm, L, D)
    sub = dr.pad64(img[0][np.ix_(keep, keep)])
    assert dr.solve_rule(sub, n - 1, rhs[0][keep], x[keep], M[np.ix_(keep, keep)]) <= 1.0
    # the defect: threshold 0 instead of DBL_MIN divides by the denormal
    xd = dr.substitute_restated(n, rhs[0], ord_, dpiv, permv, Lg, dr.Defect(pinv_threshold_zero=True))
    assert xd[j] != 0.0


def test_factor_defects_break_a_rule():
    # the lowest-index tie break: on every member of the tied family
    for n, img, rhs, name in dr.tied_images():
        out, _ = _factor_rules(img[0], n, rhs[0], dr.Defect(lowest_index_tie=True))
        assert out["order"] > 1.0, name
    # the search on the updated diagonal (what a right-looking factorisation has at hand) instead of the original
    # one: on every random image of sixteen rows or more
    for n in (16, 17, 33, 63, 64):
        imgs, rhs = dr.random_images(n)
        for q in range(imgs.shape[0]):
            out, _ = _factor_rules(imgs[q], n, rhs[q], dr.Defect(updated_diagonal=True))
            assert out["order"] > 1.0, (n, q)
    # a multiplier left non-zero for an eliminated row
    for n in (2, 17, 64):
        imgs, rhs = dr.random_images(n)
        out, _ = _factor_rules(imgs[1], n, rhs[1], dr.Defect(stale_multiplier=True))
        assert out["multipliers of gone rows"] > 1.0, n


# ---- the natural-order path ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", dr.STATIC_NS)
def test_static_restatement_meets_the_rules(n):
    imgs, rhs = dr.static_images(n)
    for q in range(imgs.shape[0]):
        for order in (2, 0):
            ok, x = dr.static_restated(imgs[q], n, rhs[q], order=order)
            assert ok, (n, q, order)
            worst = dr.solve_rule(imgs[q], n, rhs[q], x, dr.natural_abs_ldl(imgs[q], n))
            print("static n=%d qp %d order %d: solve %.3f" % (n, q, order, worst))
            assert worst <= 1.0, (n, q, worst)
    imgs, rhs, names = dr.static_bad_pivots(n)
    for q, name in enumerate(names):
        assert not dr.static_restated(imgs[q], n, rhs[q])[0], (n, name)
    for bits, order, expect in ((33, 0, False), (32, 0, True), (33, 2, True)):
        img, b = dr.static_spread_images(n, bits)
        assert dr.static_restated(img[0], n, b[0], order=order, spread_bits=32)[0] == expect, (n, bits, order)


# ---- products, feasibility -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", dr.PRODUCT_SHAPES)
def test_products_restatement_meets_the_rules_and_the_defect_breaks_them(shape):
    d = dr.problem(*shape)
    out = dr.product_rules(d, *dr.products_restated(d))
    print("products %s: %s" % (shape, "  ".join("%s %.3f" % kv for kv in out.items())))
    _assert_all(out, shape)
    if shape[0] % 16:  # (a remainder exists)
        bad = dr.product_rules(d, *dr.products_restated(d, dr.Defect(remainder_weight_one=True)))
        assert max(bad.values()) > 1.0, shape


def test_product_shapes_cover_the_issue_sets():
    assert {s[0] for s in dr.PRODUCT_SHAPES} == {15, 16, 17, 31, 33}
    assert {s[2] for s in dr.PRODUCT_SHAPES} == {1, 15, 16, 17, 33}
    assert {s[1] for s in dr.PRODUCT_SHAPES} == {0, 3}


@pytest.mark.parametrize("shape", [(17, 3, 33), (15, 0, 17)])
def test_feasibility_cases_have_their_classes(shape):
    d, dz, dl, dv, expected, names = dr.feasibility_cases(*shape)
    for q, name in enumerate(names):
        assert dr.feasibility_class(d, q, dz[q], dl[q], dv[q], 1e-8) == expected[q], (shape, name)
    assert set(expected) == {0, 1, 2, 3}
