"""The row-held DPP linear algebra of fbstab_amd/csrc/fb_row16.h (and the scalar chains of fb_common.h),
primitive by primitive on the device, against extended-precision references: the probe library
tests/kernels/row_probe.hip wraps each primitive in a kernel of its own (tests/row_probe.py), the inputs and
the acceptance rules - derived from rounding analysis, with tests/test_row_rules_cpu.py showing they have
teeth - are tests/row_rules.py.  Every test prints its worst error-to-bound ratio (lines "ROWRATIO ...")
before it asserts.

Measured on an MI355X (worst error/bound over all instantiations): see LABNOTES, "Row primitives on the
device"."""
import functools

import numpy as np
import pytest

from tests import row_rules as rr
from tests.row_rules import LD, U
from tests.row_probe import Probe

pytestmark = pytest.mark.gpu

FUSED = [("cholinvsolve", 16, 1), ("cholinv", 12, 1), ("cholinv", 18, 2), ("cholinv", 24, 2),
         ("cholsolveright", 23, 2), ("cholsolveright", 32, 2)]
_FUSED_OF = {(N, R): name for name, N, R in FUSED}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _tril_bits_equal(a, b, diag=True):
    m = np.tril(np.ones(a.shape[-2:], dtype=bool), 0 if diag else -1)
    return np.array_equal(_bits(a)[..., m], _bits(b)[..., m])


@functools.lru_cache(maxsize=None)
def _probe(variant):
    return Probe(variant)


@functools.lru_cache(maxsize=None)
def _batch(N, R, arrangement):
    """The QPs of one run: 'healthy' = F1-F4; 'mixed' = the same QPs with an F5 failure after every third
    one, so that every wavefront holds several families and failing QPs beside healthy ones (F6)."""
    A, dadd, _, fam = rr.healthy(N)
    B, b = rr.rhs(N)
    n = A.shape[0]
    if arrangement == "healthy":
        return dict(A=A, dadd=dadd, B=B, b=b, fam=fam, h=np.arange(n), f=np.zeros(0, dtype=int), what=())
    FA, Fd, what = rr.failures(N, R)
    rng = np.random.default_rng(5)
    As, ds, Bs, bs, h, f, w = [], [], [], [], [], [], []
    for i in range(n):
        h.append(len(As)); As.append(A[i]); ds.append(dadd[i]); Bs.append(B[i]); bs.append(b[i])
        if i % 3 == 0:
            k = (i // 3) % FA.shape[0]
            f.append(len(As)); w.append(what[k])
            As.append(FA[k]); ds.append(Fd[k]); Bs.append(rng.standard_normal((N, N))); bs.append(rng.standard_normal(N))
    assert set(w) == set(what)
    return dict(A=np.stack(As), dadd=np.array(ds), B=np.stack(Bs), b=np.stack(bs), fam=fam,
                h=np.array(h), f=np.array(f), what=tuple(w))


@functools.lru_cache(maxsize=None)
def _run(variant, N, R, arrangement="healthy", fill="zero", wg=64):
    """chol_rows, then every triangular primitive on the factor the device itself produced, then the fused
    pass of this pair where the product has one.  Computed once per configuration and shared."""
    p, d, lpq = _probe(variant), _batch(N, R, arrangement), 16 * R
    img = lambda M: rr.lane_image(M, lpq, fill)
    o = dict(d)
    A_img, B_img, b_img = img(d["A"]), img(d["B"]), img(d["b"][:, :, None])
    o["rec"], o["flag"] = p.chol(N, R, A_img, d["dadd"], wg)
    L_img = img(o["rec"])
    o["X"] = p.tri_inv(N, R, L_img, wg)
    o["X2"], o["W2"] = p.tri_inv_solve(N, R, L_img, B_img, wg)
    o["W"] = p.tri_solve_right(N, R, L_img, B_img, wg)
    o["xs"] = p.subst(N, R, L_img, b_img, False, wg)
    # the factor by columns, as subst_cols_t wants it: lane r holds L[j][r] for j > r and 1 / L[r][r]
    o["xt"] = p.subst(N, R, img(np.tril(o["rec"]).transpose(0, 2, 1)), b_img, True, wg)
    if (N, R) in _FUSED_OF and variant != "nodpp":
        o["fa"], o["fx"], o["fw"], o["fflag"] = p.fused(_FUSED_OF[(N, R)], N, R, A_img, d["dadd"], B_img, wg)
    return o


TWO_PASS = ("rec", "X", "X2", "W2", "W", "xs", "xt")


def _equal_outputs(a, b, keys, idx_a=slice(None), idx_b=slice(None)):
    bad = []
    for k in keys:
        x, y = a[k][idx_a], b[k][idx_b]
        # (slots beyond the diagonal are not results; nor is the fused pass's diagonal slot - where it parks
        # the reciprocal there, the fused test compares it with chol_rows')
        same = _tril_bits_equal(x, y, diag=(k == "rec")) if k in ("rec", "fa") else _same_bits(x, y)
        if not same:
            bad.append(k)
    return bad


def _report(prim, N, R, fam, ratios):
    worst = {}
    for f, name in enumerate(rr.FAMILIES):
        worst[name] = float(ratios[fam == f].max())
        print("ROWRATIO %-22s N=%-2d R=%d %s %.4f" % (prim, N, R, name, worst[name]))
    return worst


# ---- lane maps and reductions ----------------------------------------------------------------------------
@pytest.mark.parametrize("R,wg", [(1, 64), (2, 64), (1, 256), (2, 256)])
def test_lane_maps_are_exact(R, wg):
    lpq, n = 16 * R, 32 // R  # two 256-thread workgroups: rows 0-15 of a workgroup, both pairs of every wavefront
    q, l = np.meshgrid(np.arange(n), np.arange(lpq), indexing="ij")
    v = 1000.0 * q + l + 0.5  # lane-identifying payloads
    vi = (100000 * q + l + 1).astype(np.int32)
    od, oi = _probe("default").lane_map(R, v, vi, wg)
    J = np.arange(lpq)
    own_row = 16 * (l // 16)  # bc / bci reach the lanes of the lane's own 16-lane row
    assert np.array_equal(od[:, :, 0, :], v[q[:, :, None], own_row[:, :, None] + (J & 15)[None, None, :]])
    assert np.array_equal(oi[:, :, 0, :], vi[q[:, :, None], own_row[:, :, None] + (J & 15)[None, None, :]])
    want = np.broadcast_to(v[:, None, :], (n, lpq, lpq))
    assert np.array_equal(od[:, :, 1, :], want), "bcs"
    assert np.array_equal(od[:, :, 2, :], want), "bcr"
    assert np.array_equal(oi[:, :, 1, :], np.broadcast_to(vi[:, None, :], (n, lpq, lpq))), "bcri"
    assert np.array_equal(_probe("default").bc_all(R, v, wg), want), "bc_all"
    for variant in ("guard", "nodpp"):
        od2, oi2 = _probe(variant).lane_map(R, v, vi, wg)
        assert _same_bits(od, od2) and np.array_equal(oi, oi2), variant


@pytest.mark.parametrize("R,wg", [(1, 64), (2, 64), (2, 256)])
def test_reductions(R, wg):
    lpq, n = 16 * R, 32 // R
    rng = np.random.default_rng(11)
    scale = 2.0 ** (8 * np.arange(n))[:, None]  # QPs of very different magnitude: a neighbour's value would show
    ints = rng.integers(-1000, 1000, (n, lpq)).astype(np.float64) * scale
    rnd = rng.standard_normal((n, lpq)) * 10.0 ** rng.integers(-6, 6, (n, lpq))
    neg = -np.abs(rng.standard_normal((n, lpq))) - 1e-3
    neg[np.arange(n), rng.integers(0, lpq, n)] = -0.0  # the maximum of each QP is -0.0 (no +0.0 among them)
    p = _probe("default")
    for name, v in (("ints", ints), ("random", rnd), ("negative", neg)):
        out = p.reduce(R, v, wg)
        rows = v.reshape(n, R, 16)
        # every lane of a row / of a QP holds the same bits
        assert (_bits(out[:, :, :2]).reshape(n, R, 16, 2) == _bits(out[:, :, :2]).reshape(n, R, 16, 2)[:, :, :1]).all(), name
        assert (_bits(out[:, :, 2:]) == _bits(out[:, :1, 2:])).all(), name
        row_max = np.repeat(rows.max(axis=2), 16, axis=1)
        assert _same_bits(out[:, :, 1], row_max), (name, "row max")
        assert _same_bits(out[:, :, 3], np.broadcast_to(v.max(axis=1)[:, None], (n, lpq))), (name, "qp max")
        row_sum = np.repeat(rows.astype(LD).sum(axis=2), 16, axis=1)
        qp_sum = np.broadcast_to(v.astype(LD).sum(axis=1)[:, None], (n, lpq))
        if name == "ints":
            assert np.array_equal(out[:, :, 0].astype(LD), row_sum) and np.array_equal(out[:, :, 2].astype(LD), qp_sum)
        else:
            row_abs = np.repeat(np.abs(rows).astype(LD).sum(axis=2), 16, axis=1)
            qp_abs = np.broadcast_to(np.abs(v).astype(LD).sum(axis=1)[:, None], (n, lpq))
            r_row = float((np.abs(out[:, :, 0].astype(LD) - row_sum) / (15 * U * row_abs)).max())
            r_qp = float((np.abs(out[:, :, 2].astype(LD) - qp_sum) / ((lpq - 1) * U * qp_abs)).max())
            print("ROWRATIO row_reduce sum R=%d %s %.4f\nROWRATIO qp_reduce sum R=%d %s %.4f" % (R, name, r_row, R, name, r_qp))
            assert r_row <= 1.0 and r_qp <= 1.0, (name, r_row, r_qp)
        if name == "negative":
            assert np.signbit(out[:, :, 3]).all() and (out[:, :, 3] == 0).all()
        assert _same_bits(out, _probe("guard").reduce(R, v, wg)) and _same_bits(out, _probe("nodpp").reduce(R, v, wg))


# ---- scalar chains on the chip's seeds ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mantissas():
    rng = np.random.default_rng(3)
    m = np.concatenate([[1.0, 1.0 + 2.0 ** -52, 2.0 - 2.0 ** -52], 1.0 + rng.random(512)])
    m.setflags(write=False)
    return m


def _grid(k_lo, k_hi):
    """m 2^k for every tenth k of [k_lo, k_hi]"""
    k = np.arange(k_lo, k_hi + 1, 10)
    return np.ldexp(_mantissas()[None, :], k[:, None]).ravel()


def _ulps(got, ref):
    """|got - ref| in ulps of the reference value"""
    with np.errstate(invalid="ignore"):
        return np.abs(got.astype(LD) - ref) / np.spacing(np.abs(ref.astype(np.float64))).astype(LD)


def _worst(x, err):
    i = int(np.argmax(err))
    return "worst %.3f ulp at x = %r (%s)" % (float(err[i]), float(x[i]), float(x[i]).hex())


@pytest.mark.parametrize("wg", [64, 256])
def test_scalar_chains(wg):
    p = _probe("default")
    # fsqrt: +normal inputs within 1 ulp, the header's claim.  The header claimed it for +denormal inputs too;
    # the device gives up to 6.887 ulp there (x = 0x0.000007eb61e73p-1022; 2.56 ulp at 2^-1073): the residual
    # x - g^2 is about x 2^-48 and underflows, so the last correction is lost.  False but harmless (fb_common.h
    # says why, and what restoring the ulp costs), so the header is corrected and what is asserted on +denormal
    # inputs is what its analysis leaves: the coupled step's 3/2 eps^2 for a seed within eps = 2^-23 (the
    # 2^29 ulp of v_rsq_f64), = 192 ulp, + 2 for the roundings - a bound from the instruction's precision, not
    # from the measurement, and far under what a missing step would leave (2^30 ulp).
    x = _grid(-1074, 1023)
    x = x[(x > 0) & np.isfinite(x)]
    err = _ulps(p.scalar(x, wg)[:, 1], np.sqrt(x.astype(LD)))
    den = x < np.finfo(np.float64).tiny
    print("ROWRATIO fsqrt ulp %.4f (%s)" % (float(err[~den].max()), _worst(x[~den], err[~den])))
    print("ROWRATIO fsqrt +denormal ulp %.4f (%s)" % (float(err[den].max()), _worst(x[den], err[den])))
    e_sqrt = (x[~den], err[~den])
    e_sqrt_den = (x[den], err[den])
    # ... and everything else comes back as it went in
    sp = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -1.0, -2.5e-310, -1e300])
    back = p.scalar(sp, wg)[:, 1]
    ok_special = np.array_equal(_bits(back)[~np.isnan(sp)], _bits(sp)[~np.isnan(sp)]) and np.isnan(back[np.isnan(sp)]).all()
    # rsqrt_full on [2^-1000, 2^1000]: 2 ulp
    xr = _grid(-1000, 999)
    xr = np.concatenate([xr, [2.0 ** 1000]])
    er = _ulps(p.scalar(xr, wg)[:, 0], LD(1) / np.sqrt(xr.astype(LD)))
    print("ROWRATIO rsqrt_full ulp %.4f (%s)" % (float(er.max()), _worst(xr, er)))
    # rcp_fast on [1e-13, 2^1000]: 1 ulp
    xc = _grid(-44, 999)
    xc = np.concatenate([xc[(xc >= 1e-13) & (xc <= 2.0 ** 1000)], [1e-13, 2.0 ** 1000]])
    ec = _ulps(p.scalar(xc, wg)[:, 2], LD(1) / xc.astype(LD))
    print("ROWRATIO rcp_fast ulp %.4f (%s)" % (float(ec.max()), _worst(xc, ec)))
    assert e_sqrt[1].max() <= 1.0, _worst(*e_sqrt)
    assert e_sqrt_den[1].max() <= 1.5 * (2.0 ** -23) ** 2 / U + 2.0, _worst(*e_sqrt_den)
    assert ok_special, (sp, back)
    assert er.max() <= 2.0, _worst(xr, er)
    assert ec.max() <= 1.0, _worst(xc, ec)
    for variant in ("guard", "nodpp"):
        assert _same_bits(p.scalar(xr, wg), _probe(variant).scalar(xr, wg)), variant


@pytest.mark.parametrize("wg", [64, 256])
def test_pfb_all_against_pfb_and_its_gradient(wg):
    rng = np.random.default_rng(17)
    n = 4096
    mag = lambda: rng.standard_normal(n) * 10.0 ** rng.integers(-20, 7, n)
    a, b = mag(), mag()
    a[::7] = np.abs(a[::7]); b[::7] = np.abs(b[::7])     # both positive
    a[1::11] = 0.0; b[2::11] = 0.0; a[3::13] = -0.0      # exactly on the a > 0, b > 0 boundary
    # both sides of r = 1e-13: r = 1e-13 (1 +- 2^-k) in every quadrant
    th = rng.uniform(0, 2 * np.pi, 512)
    rr_ = 1e-13 * (1.0 + np.concatenate([2.0 ** -np.arange(1, 53, 0.203125)[:256], -2.0 ** -np.arange(1, 53, 0.203125)[:256]]))
    a[:512], b[:512] = rr_ * np.cos(th), rr_ * np.sin(th)
    alpha = rng.choice([0.95, 0.5, 1.0, 0.05], n)
    out = _probe("default").pfb(a, b, alpha, wg)
    phi_ok = _same_bits(out[:, 0], out[:, 3])
    scale = np.maximum(alpha, (1.0 - alpha) * np.maximum(np.abs(a), np.abs(b)))
    tol = 4.0 * np.spacing(scale)
    e0, e1 = np.abs(out[:, 1] - out[:, 4]) / tol, np.abs(out[:, 2] - out[:, 5]) / tol
    i = int(np.argmax(np.maximum(e0, e1)))
    print("ROWRATIO pfb_all gradient %.4f of 4 ulp (a = %r, b = %r, alpha = %r)" % (max(e0[i], e1[i]), a[i], b[i], alpha[i]))
    # the same branch on both sides: below 1e-13 both give the constant, and only there
    r = np.sqrt(a.astype(LD) ** 2 + b.astype(LD) ** 2)
    const = alpha * (1.0 - 0.70710678118654752440)
    is_const_all = (out[:, 1] == const) & (out[:, 2] == const)
    is_const_ref = (out[:, 4] == const) & (out[:, 5] == const)
    clear = np.abs(r / LD(1e-13) - 1) > 16 * U  # (the device's r carries ~3 u of rounding: not judged that close to 1e-13)
    assert phi_ok, "phi of pfb_all is not bitwise pfb's"
    assert np.array_equal(is_const_all, is_const_ref), "pfb_all and pfb_gradient part at r = 1e-13"
    assert np.array_equal(is_const_all[clear], (r < LD(1e-13))[clear])
    assert np.isfinite(out).all()
    assert max(e0.max(), e1.max()) <= 1.0, (a[i], b[i], alpha[i], out[i])
    # a > 0 and b > 0 against either one <= 0: the (1 - alpha) term is present in the one case only
    both = (a > 0) & (b > 0) & ~is_const_all
    with np.errstate(invalid="ignore"):  # (r = 0: the constant branch, masked out below)
        g0_plain = alpha * (1.0 - (a.astype(LD) / r).astype(np.float64))
    far = np.abs(out[:, 1] - g0_plain) > 8 * tol
    big = (1.0 - alpha) * np.abs(b) > 32 * tol
    assert (far[both & big]).all() and not far[~both & ~is_const_all & (r > 0)].any()


# ---- chol_rows ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,R", rr.PAIRS)
def test_chol_rows_meets_the_componentwise_rule(N, R):
    o = _run("default", N, R)
    ratios = rr.chol_ratio(o["A"], o["dadd"], o["rec"])
    worst = _report("chol_rows", N, R, o["fam"], ratios)
    assert (o["flag"] == 1).all()
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("N,R", rr.PAIRS)
def test_failures_are_reported_and_neighbours_untouched(N, R):
    """F5 and F6: a failing QP reports false on every one of its lanes and true nowhere else; the QPs beside
    it are bitwise what they are beside healthy neighbours; and nothing a lane r < N computes depends on what
    the lanes r >= N of its QP held (zeros in one run, finite garbage and NaN in the other)."""
    ref = _run("default", N, R)
    for fill in ("zero", "garbage"):
        o = _run("default", N, R, "mixed", fill)
        assert (o["flag"][o["h"]] == 1).all(), fill
        bad = [w for w, fl in zip(o["what"], o["flag"][o["f"]]) if fl.any()]
        assert not bad, (fill, bad)
        if "fflag" in o:
            assert np.array_equal(o["fflag"], o["flag"]), fill
        keys = TWO_PASS + (("fa", "fx", "fw") if "fa" in o else ())
        assert not _equal_outputs(o, ref, keys, o["h"]), (fill, _equal_outputs(o, ref, keys, o["h"]))
    z, g = _run("default", N, R, "mixed", "zero"), _run("default", N, R, "mixed", "garbage")
    assert _tril_bits_equal(z["rec"], g["rec"])  # the failing QPs' own rows too
    g2 = _run("default", N, R, "healthy", "garbage")
    assert not _equal_outputs(g2, ref, TWO_PASS)


# ---- triangular work on the device's own factor ---------------------------------------------------------------
@pytest.mark.parametrize("N,R", rr.PAIRS)
def test_triangular_primitives_meet_their_rules(N, R):
    o = _run("default", N, R)
    rec, fam = o["rec"], o["fam"]
    worst = {}
    for prim, ratios in (("tri_inv_cols", rr.inv_ratio(rec, o["X"])),
                         ("tri_inv_cols_solve x", rr.inv_ratio(rec, o["X2"])),
                         ("tri_inv_cols_solve w", rr.right_ratio(rec, o["B"], o["W2"])),
                         ("tri_solve_right", rr.right_ratio(rec, o["B"], o["W"])),
                         ("subst_rows", rr.subst_ratio(rec, o["b"], o["xs"])),
                         ("subst_cols_t", rr.subst_ratio(rec, o["b"], o["xt"], transposed=True))):
        worst[prim] = max(_report(prim, N, R, fam, ratios).values())
    assert max(worst.values()) <= 1.0, worst


# ---- the fused pass ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,N,R", FUSED)
def test_fused_pass_meets_the_rules_and_is_bitwise_the_two_passes(name, N, R):
    o = _run("default", N, R)
    park = name == "cholsolveright"
    # The factor the fused pass describes.  With PARK its a is chol_rows' record.  Without, a keeps the
    # UNSCALED columns (fb_row16.h: the scaled ones live in the streams' source register only; the header's
    # earlier "a[k] = L[r][k]" did not hold - found by this test, harmless, nothing reads a): the entry times
    # the reciprocal pivot, rounded once, is the factor's entry - the multiplication level 6 does - and the
    # reciprocals, not a result of this form, are chol_rows'.
    i = np.arange(N)
    q = o["rec"][:, i, i]
    rec = np.tril(o["fa"] if park else o["fa"] * q[:, None, :], -1)
    rec[:, i, i] = o["fa"][:, i, i] if park else q
    worst = {"chol": max(_report(name + " a", N, R, o["fam"], rr.chol_ratio(o["A"], o["dadd"], rec)).values())}
    if name in ("cholinvsolve", "cholinv"):
        worst["x"] = max(_report(name + " x", N, R, o["fam"], rr.inv_ratio(rec, o["fx"])).values())
    if name in ("cholinvsolve", "cholsolveright"):
        worst["w"] = max(_report(name + " w", N, R, o["fam"], rr.right_ratio(rec, o["B"], o["fw"])).values())
    assert (o["fflag"] == 1).all()
    assert max(worst.values()) <= 1.0, worst
    # bitwise chol_rows + tri_inv_cols_solve / tri_inv_cols / tri_solve_right
    assert _tril_bits_equal(rec, o["rec"], diag=park), "the factor"
    if name == "cholinvsolve":
        assert _same_bits(o["fx"], o["X2"]) and _same_bits(o["fw"], o["W2"])
    elif name == "cholinv":
        assert _same_bits(o["fx"], o["X"])
    else:
        assert _same_bits(o["fw"], o["W"])
    # the flags on F5 (test_failures_... compares them lane by lane in both fills too)
    m = _run("default", N, R, "mixed", "garbage")
    assert np.array_equal(m["fflag"], m["flag"]) and not m["fflag"][m["f"]].any()


# ---- across builds -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,R", rr.PAIRS)
def test_builds_agree_bitwise(N, R):
    """The build without the guard s_nop (the product's) against the one that keeps them all - every output -
    and the two-pass forms with the fused broadcast-FMA against the mov + fma pairs of FB_FMAC_DPP=0."""
    for arrangement, fill in (("healthy", "zero"), ("mixed", "garbage")):
        d, g, nd = (_run(v, N, R, arrangement, fill) for v in ("default", "guard", "nodpp"))
        keys = TWO_PASS + (("fa", "fx", "fw") if "fa" in d else ())
        h = d["h"]
        assert not _equal_outputs(d, g, keys, h, h), ("guard", arrangement, _equal_outputs(d, g, keys, h, h))
        assert not _equal_outputs(d, nd, TWO_PASS, h, h), ("nodpp", arrangement, _equal_outputs(d, nd, TWO_PASS, h, h))
        assert np.array_equal(d["flag"], g["flag"]) and np.array_equal(d["flag"], nd["flag"])
        if "fflag" in d:
            assert np.array_equal(d["fflag"], g["fflag"])


@pytest.mark.parametrize("N,R", [(16, 1), (23, 2)])
def test_rows_4_to_15_of_a_workgroup(N, R):
    """One case of the factorisation, the triangular work and the fused pass from a 256-thread workgroup."""
    a, b = _run("default", N, R), _run("default", N, R, wg=256)
    keys = TWO_PASS + ("fa", "fx", "fw")
    assert not _equal_outputs(a, b, keys), _equal_outputs(a, b, keys)
    assert np.array_equal(a["flag"], b["flag"]) and np.array_equal(a["fflag"], b["fflag"])


# ---- dot products ------------------------------------------------------------------------------------------
def _wide(rng, shape):
    return rng.standard_normal(shape) * 10.0 ** rng.integers(-4, 5, shape)


BC_DOTS = [(0, N, R) for N, R in rr.PRODUCT_PAIRS] + [(3, 11, 1), (14, 19, 2)]


@pytest.mark.parametrize("B,E,R", BC_DOTS)
def test_bc_dot(B, E, R):
    lpq, n = 16 * R, 16 // R
    rng = np.random.default_rng([B, E, R])
    M, v, init = _wide(rng, (n, lpq, E)), _wide(rng, (n, lpq)), _wide(rng, (n, lpq))
    terms = M[:, :, B:E].astype(LD) * v[:, None, B:E].astype(LD)
    for wg in ((64, 256) if (B, E, R) in ((0, 16, 1), (14, 19, 2)) else (64,)):
        got = _probe("default").bc_dot(B, E, R, M, v, init, wg)
        ratio = rr.dot_ratio(got, terms, init)
        print("ROWRATIO bc_dot<%d,%d,%d> wg %d %.4f" % (B, E, R, wg, ratio))
        assert ratio <= 1.0
        assert _same_bits(got, _probe("guard").bc_dot(B, E, R, M, v, init, wg))
        # (FB_FMAC_DPP=0 sums the same products in the same order into the same four partial sums)
        assert _same_bits(got, _probe("nodpp").bc_dot(B, E, R, M, v, init, wg))


@pytest.mark.parametrize("NC,R", [(20, 1), (32, 1), (10, 2), (16, 2), (32, 2)])
@pytest.mark.parametrize("neg", [False, True])
def test_bc_cols_dot(NC, R, neg):
    lpq, n = 16 * R, 16 // R
    nsrc = (NC + lpq - 1) // lpq
    rng = np.random.default_rng([NC, R, int(neg)])
    C, src, p0 = _wide(rng, (n, lpq, NC)), _wide(rng, (n, lpq, nsrc)), _wide(rng, (n, lpq, 4))  # p[] non-zero on entry
    k = np.arange(NC)
    served = src[:, k % lpq, k // lpq]  # [n, NC]: lane k % lpq of src[k / lpq]
    prod = (-1 if neg else 1) * C.astype(LD) * served[:, None, :].astype(LD)
    for wg in ((64, 256) if (NC, R) == (32, 2) else (64,)):
        got = _probe("default").bc_cols_dot(NC, R, neg, C, src, p0, wg)
        worst = 0.0
        for i in range(4):
            if (k % 4 == i).any():
                worst = max(worst, rr.dot_ratio(got[:, :, i], prod[:, :, k % 4 == i], p0[:, :, i]))
            else:
                assert _same_bits(got[:, :, i], p0[:, :, i])
        print("ROWRATIO bc_cols_dot<%d,%d,%d> wg %d %.4f" % (NC, R, neg, wg, worst))
        assert worst <= 1.0
        assert _same_bits(got, _probe("guard").bc_cols_dot(NC, R, neg, C, src, p0, wg))


@pytest.mark.parametrize("N", [16, 12, 23, 32, 18, 24])
def test_dot4(N):
    n = 16
    rng = np.random.default_rng(N)
    M, b, init = _wide(rng, (n, 16, N)), _wide(rng, (n, 16, N)), _wide(rng, (n, 16))
    for wg in ((64, 256) if N == 23 else (64,)):
        got = _probe("default").dot4(N, M, b, init, wg)
        ratio = rr.dot_ratio(got, M.astype(LD) * b.astype(LD), init)
        print("ROWRATIO dot4<%d> wg %d %.4f" % (N, wg, ratio))
        assert ratio <= 1.0
