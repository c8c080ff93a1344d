"""The acceptance rules of tests/row_rules.py must have teeth: a plain float64 restatement of the row-held
Cholesky, inverse, right-solve and substitutions (reciprocal diagonal, one rounding per operation, no lanes)
passes them on F1-F4 - if it did not, the DERIVATION of a bound would be wrong, not a kernel - and every
seeded mutant of it fails at least one rule on every family it applies to.  The constants come from the
derivations in tests/row_rules.py; nothing here has seen a device."""
import numpy as np
import pytest

from tests import row_rules as rr


def _rules(A, dadd, B, b, mut=None):
    """Worst ratio of every rule over the QPs of one family, computed from the (mutated) restatement."""
    with np.errstate(invalid="ignore", over="ignore"):  # a mutant may drive a pivot negative: NaN fails the rules
        return _rules_of(A, dadd, B, b, mut)


def _rules_of(A, dadd, B, b, mut):
    rec, ok = rr.chol_restated(A, dadd, mut)
    X, W = rr.tri_inv_solve_restated(rec, B, mut)
    X1, _ = rr.tri_inv_solve_restated(rec, None, mut)
    assert np.array_equal(X, X1, equal_nan=True)
    out = {
        "chol": rr.chol_ratio(A, dadd, rec).max(),
        "inv": rr.inv_ratio(rec, X).max(),
        "right": rr.right_ratio(rec, B, W).max(),
        "subst_rows": rr.subst_ratio(rec, b, rr.subst_restated(rec, b, False, mut)).max(),
        "subst_cols_t": rr.subst_ratio(rec, b, rr.subst_restated(rec, b, True, mut), transposed=True).max(),
    }
    return out, ok


def _family_slices(N):
    A, dadd, _, fam = rr.healthy(N)
    B, b = rr.rhs(N)
    for f, name in enumerate(rr.FAMILIES):
        s = fam == f
        yield name, A[s], dadd[s], B[s], b[s]


@pytest.mark.parametrize("N,R", rr.PAIRS)
def test_restatement_passes_every_rule(N, R):
    for name, A, dadd, B, b in _family_slices(N):
        out, ok = _rules(A, dadd, B, b)
        print("N=%d %s restatement error/bound: %s" % (N, name, "  ".join("%s %.3f" % kv for kv in out.items())))
        assert ok.all()
        for rule, worst in out.items():
            assert worst <= 1.0, (N, name, rule, worst)


def test_restatement_reports_the_failures():
    for N, R in rr.PAIRS:
        A, dadd, what = rr.failures(N, R)
        with np.errstate(invalid="ignore", over="ignore"):
            _, ok = rr.chol_restated(A, dadd)
        assert not ok.any(), (N, [w for w, o in zip(what, ok) if o])


def _mutants(N, R):
    """(name, mutant, the families it applies to).  A dropped update or a lane served from the wrong row
    changes nothing where every off-diagonal entry is zero (F4: dropped update only - the wrong row's
    value there is the pivot's own square root); F3 has no diag_add to misapply."""
    m = [
        ("update dropped", rr.Mutant(drop_update=(N - 1, N // 2, 0)), ("F1", "F2", "F3")),
        ("diag_add twice", rr.Mutant(diag_twice=True), ("F1", "F2", "F4")),
        ("diag_add not on the last pivot", rr.Mutant(diag_skip_last=True), ("F1", "F2", "F4")),
        ("q off by 2^-30", rr.Mutant(q_rel_err=2.0 ** -30), rr.FAMILIES),
        ("right-solve entry scaled by the wrong pivot", rr.Mutant(wrong_pivot=(N - 1, N // 2, 0)), rr.FAMILIES),
    ]
    if R == 2 and N > 16:
        m.append(("lanes 16-31 served from the even row", rr.Mutant(hi_lanes_from_lo=True), rr.FAMILIES))
    return m


@pytest.mark.parametrize("N,R", rr.PRODUCT_PAIRS + [(17, 2)])
def test_every_mutant_fails_a_rule_on_every_family(N, R):
    for name, A, dadd, B, b in _family_slices(N):
        for what, mut, fams in _mutants(N, R):
            if name not in fams:
                continue
            out, _ = _rules(A, dadd, B, b, mut)
            worst = max(out.values())
            print("N=%d %s mutant '%s': worst error/bound %.3g" % (N, name, what, worst))
            assert worst > 1.0, (N, name, what, out)
