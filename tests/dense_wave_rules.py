"""Inputs, references, acceptance rules and plain float64 restatements for the stages of the one-wavefront dense
policy, fbstab_amd/csrc/fb_dense_wave.h.  Shared by tests/test_gpu_dense_wave_stages.py (the device, through
tests/dense_wave_probe.py) and tests/test_dense_wave_rules_cpu.py (the restatements and their seeded defects
through the SAME rules).  Nothing in here has seen a device.

Conventions.  Matrices are in mathematical shape, [count, rows, cols]; the probe wrapper lays them out by
columns.  A "64 x 64 image" is K zero-padded: image[q, t, c] = K[t][c], rows and columns n .. 63 zero.  The
factors of DenseWave::factor come as the device leaves them: permv[k] = the row eliminated at step k (lanes
k < n), ord[t] = the step at which row t went, dpiv[t] = its pivot, Lg[k][t] = the multiplier row t received
at step k (zero for rows that were gone).

References are evaluated in numpy.longdouble (64-bit mantissa) from the doubles under test.

The rules are componentwise first-order rounding bounds on absolute values, u = 2^-53; the constants come from
counting roundings, none was fitted to a measurement:

  inner product, m accumulated terms:   |got - exact| <= 2 (m + 2) u S,  S = the sum of the terms' magnitudes.
      A term accumulated into a running sum of m terms, in whatever order and however the sum is split into
      partial sums, passes through at most m - 1 roundings of additions (an fma counts as its addition); the
      term itself carries at most two more (the product Gamma_k A_kj of the assembly, or H_ij + sigma, and a
      product not fused into its addition); one more for the final combination of partial sums with an outside
      term would make m + 2 - which is taken as is -, and the factor 2 covers the second-order terms
      (1 + u)^(m + 2) - 1 <= 2 (m + 2) u for every m used here (m u < 1e-13).
        E = tril(H) mirrored + sigma I + A' Gamma A:  m = nv + 1 (the seed H_ij + sigma [i = j] is a term)
        A' (rv / mu):                                 m = nv
        y = b - A z, rl = h - G z:                    m = nz + 1
        rz = f + H z + G' l + A' v:                   m = nz + nl + nv + 1
  factorisation:  |P K P' - L D L'| <= 2 (n + 2) u |L| |D| |L'|, L, D and P rebuilt from the device's own
      ord, dpiv, Lg.  An entry of the Schur complement is updated by at most n - 1 fmas, one rounding each;
      the multiplier is col * (1 / d): two roundings; (n + 1) u in all, one more for the representation of the
      product L D L' itself, doubled for second order.
  solve:  |K x - b| <= 2 (n + 2) u (|L| |D| |L'| |x| + |b|), with |L| |D| |L'| mapped back to the original
      order.  This is the factorisation's bound carried to the solution; each substitution adds up to n u
      |L| |D| |L'| |x| of its own in the worst case (roundings all of one sign), which the rule does NOT
      grant: it is the bar a solve has to meet whose substitution errors are, as rounding errors are, not
      aligned.  tests/test_dense_wave_rules_cpu.py shows that a float64 restatement meets it on every input
      used on the device.
  Exact by construction (bitwise): Kr symmetric; dg = Kr[t][t]; the G blocks and the -sigma diagonal are the
      inputs' bits; everything from row / column n on is +0; permv is a permutation of 0 .. n - 1 and ord its
      inverse; multipliers of rows that are gone are zero.

Every bound is applied only where it can fail: the largest bound of a QP is at most 1e-5 of its largest
reference entry (`_ratio` asserts it).

The elimination ORDER is held to eigen_ldlt(), a float64 restatement of Eigen's LDLT as oracle/oracle_linalg.h
states it: at step k the largest |diagonal| among positions k .. n - 1 of the matrix AS STORED at that moment,
the first position winning a tie, then a symmetric swap of positions k and the winner.  Two things follow from
the storage and are easy to miss.  The factorisation is left-looking: when step k searches, the diagonal entries
behind position k have NOT been updated by the steps before - the search runs on the ORIGINAL diagonal - while
the pivot itself, taken after the search, is the updated entry.  And "first" is first by POSITION, which the
swaps have shuffled: the row that sat at position k when another won goes to the winner's old place.  A step is
compared strictly where the best and the second-best remaining |diagonal| are bitwise equal (a tie) or more than
1e-10 apart (relative); elsewhere ("close") it only has to have taken a diagonal within that margin of the best.
The float64 restatement of the factorisation follows that rule and is held to it on the CPU; DenseWave::factor as
it stands does not (DEVICE_AS_DOCUMENTED below, LABNOTES), and the device tests assert its documented order.
"""
import functools

import numpy as np

from tests.tangent_helpers import U

LD = np.longdouble
DBL_MIN = float(np.finfo(np.float64).tiny)
CLOSE = 1e-10
VACUITY = 1e-5
K_FEASIBLE, K_PRIMAL_INFEASIBLE, K_DUAL_INFEASIBLE, K_BOTH_INFEASIBLE = 0, 1, 2, 3  # fb_common.h: Feasibility

# (nz, nl, nv): nz in {1, 15, 16, 17, 33, 48, 49, 64} x nl in {0, 1, 64 - nz} x the nv below, every pair of
# values of two of the three at least once where the shape exists, and the five shapes named by hand
ASSEMBLE_NV = (1, 2, 3, 15, 16, 17, 31, 32, 33, 48, 49, 65, 131)
ASSEMBLE_SHAPES = [
    (1, 0, 1), (64, 0, 1), (63, 1, 3), (16, 0, 16), (17, 3, 33),
    (1, 1, 2), (1, 63, 15), (1, 0, 131),
    (15, 0, 17), (15, 1, 31), (15, 49, 32),
    (16, 1, 48), (16, 48, 49), (16, 0, 3),
    (17, 0, 65), (17, 1, 131), (17, 47, 2),
    (33, 0, 3), (33, 1, 15), (33, 31, 16),
    (48, 0, 31), (48, 1, 32), (48, 16, 33),
    (49, 0, 48), (49, 1, 49), (49, 15, 65),
    (64, 0, 131), (64, 0, 2), (64, 0, 17),
]
ASSEMBLE_SIGMAS = (1.0, 1e-8)
FACTOR_NS = (1, 2, 16, 17, 33, 63, 64)
STATIC_NS = (1, 16, 17, 32, 33, 48, 49, 63, 64)
PRODUCT_SHAPES = [(15, 0, 1), (16, 3, 15), (17, 0, 16), (31, 3, 17), (33, 0, 33), (15, 3, 33), (16, 0, 17),
                  (17, 3, 1), (31, 0, 15), (33, 3, 16)]
STEP_SHAPES = [(1, 0, 1), (2, 1, 1), (63, 1, 3), (20, 5, 128), (20, 5, 129)]
PER_CASE = 3  # QPs per shape


def _rng(tag, *ints):
    return np.random.default_rng([20250117] + [int(i) for i in ints] + [ord(c) for c in tag])


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ---- inputs: problems --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def problem(nz, nl, nv, count=PER_CASE):
    """A batch of dense QP data and a point: dict of H [count, nz, nz] (symmetric), f, G [count, nl, nz], h,
    A [count, nv, nz], b, z, l, v, and of the assembly's gam, rvm [count, nv].  Gamma spans 1e-12 .. 1e8 within
    each QP (nv = 1: over the QPs)."""
    rng = _rng("problem", nz, nl, nv)
    M = rng.standard_normal((count, nz, nz))
    H = M @ M.transpose(0, 2, 1) / nz
    H = np.tril(H) + np.tril(H, -1).transpose(0, 2, 1)
    d = dict(H=H, f=rng.standard_normal((count, nz)), G=rng.standard_normal((count, nl, nz)),
             h=rng.standard_normal((count, nl)), A=rng.standard_normal((count, nv, nz)),
             b=rng.standard_normal((count, nv)), z=rng.standard_normal((count, nz)),
             l=rng.standard_normal((count, nl)), v=np.abs(rng.standard_normal((count, nv))))
    gam = 10.0 ** rng.uniform(-12.0, 8.0, (count, nv))
    if nv >= 2:
        # (the largest weight sits on the LAST row, and on the one before it in every other QP: a tail row that
        #  is dropped or taken twice must not hide behind the rounding of a heavier row)
        for q in range(count):
            gam[q, nv - 1] = 1e8
            if q % 2 == 1 and nv >= 3:
                gam[q, nv - 2] = 1e8
            gam[q, rng.integers(0, max(1, nv - 2))] = 1e-12
    else:
        gam[:, 0] = np.array([1e-12, 1.0, 1e8] * count)[:count]
    d["gam"] = gam
    d["rvm"] = rng.standard_normal((count, nv)) * 10.0 ** rng.uniform(-3.0, 3.0, (count, nv))
    _freeze(*d.values())
    return d


def with_nan_upper(H):
    """H with its strict upper triangle set to NaN: what the assembly must never read."""
    out = np.array(H)
    iu = np.triu_indices(H.shape[-1], 1)
    out[:, iu[0], iu[1]] = np.nan
    return out


# ---- inputs: images ------------------------------------------------------------------------------------------
def pad64(K):
    K = np.asarray(K, dtype=np.float64)
    img = np.zeros(K.shape[:-2] + (64, 64))
    img[..., : K.shape[-2], : K.shape[-1]] = K
    return img


def _quasi_definite(rng, n, ne, sigma):
    """[[E, G'], [G, -sigma I]], E = D (M M' / ne + I) D with D = diag(2^k): exact scaling, graded diagonal."""
    M = rng.standard_normal((ne, ne))
    D = 2.0 ** rng.integers(-3, 4, ne).astype(np.float64)
    E = D[:, None] * (M @ M.T / ne + np.eye(ne)) * D[None, :]
    E = np.tril(E) + np.tril(E, -1).T
    K = np.zeros((n, n))
    K[:ne, :ne] = E
    G = rng.standard_normal((n - ne, ne))
    K[ne:, :ne] = G
    K[:ne, ne:] = G.T
    K[ne:, ne:] = -sigma * np.eye(n - ne)
    return K


@functools.lru_cache(maxsize=None)
def random_images(n, count=4):
    """(images [count, 64, 64], rhs [count, 64]): quasi-definite, a quarter of the rows equality rows (none for
    the first QP), sigma = 1 and 1e-4 in turn."""
    rng = _rng("images", n)
    Ks = []
    for q in range(count):
        ne = n if (q == 0 or n == 1) else max(1, n - max(1, n // 4))
        Ks.append(_quasi_definite(rng, n, ne, 1.0 if q % 2 == 0 else 1e-4))
    b = np.zeros((count, 64))
    b[:, :n] = rng.standard_normal((count, n))
    return _freeze(pad64(np.stack(Ks)), b)


def _tied(diag, G, sigma):
    diag = np.asarray(diag, dtype=np.float64)
    ne, nl = diag.size, G.shape[0]
    K = np.zeros((ne + nl, ne + nl))
    K[:ne, :ne] = np.diag(diag)
    K[ne:, :ne] = G
    K[:ne, ne:] = G.T
    K[ne:, ne:] = -sigma * np.eye(nl)
    return K


@functools.lru_cache(maxsize=None)
def tied_images():
    """The tied family: E diagonal with repeated entries and a larger one out of place, one and three coupling
    equality rows.  [(n, images [1, 64, 64], rhs [1, 64], name)].  The ties are exact and stay exact (E is
    diagonal: no elimination inside it touches another of its diagonal entries)."""
    rng = _rng("tied")
    out = []
    diags = {"2 2 5 2": [2, 2, 5, 2], "3 3 2 7 3 2 3": [3, 3, 2, 7, 3, 2, 3],
             "twenty": [4, 4, 1, 4, 9, 1, 4, 4, 9, 1, 4, 2, 2, 4, 16, 4, 1, 9, 4, 4],
             "sixty": list(np.tile([2.0, 8.0, 2.0, 0.5, 8.0, 2.0], 10))}
    for name, dg in diags.items():
        for nl in (1, 3):
            ne = len(dg)
            G = rng.standard_normal((nl, ne))
            if name == "2 2 5 2" and nl == 1:
                G = np.array([[1.0, 0.75, -0.5, 1.25]])  # one equality row coupling all four
            K = _tied(dg, G, 1e-4)
            b = np.zeros((1, 64))
            b[0, : ne + nl] = rng.standard_normal(ne + nl)
            out.append((ne + nl, pad64(K)[None], b, "%s + %d" % (name, nl)))
    return out


@functools.lru_cache(maxsize=None)
def singular_images():
    """The singular family: [(n, image [64, 64], name)]; the verdict is eigen_ldlt()'s."""
    rng = _rng("singular")
    M = rng.standard_normal((5, 5))
    nan5 = M @ M.T + np.eye(5)
    nan5[2, 2] = np.nan
    return [(3, pad64(np.zeros((3, 3))), "zero matrix"),
            (2, pad64(np.diag([1.0, 0.0])), "diag(1, 0)"),
            (2, pad64(np.array([[0.0, 1.0], [1.0, 0.0]])), "[[0, 1], [1, 0]]"),
            (4, pad64(np.array([[2.0, 0, 0, 0], [0, 0.0, 0, 1.0], [0, 0, 3.0, 0], [0, 1.0, 0, 0.0]])),
             "zero pivots over a non-zero column, behind valid pivots"),
            (5, pad64(nan5), "NaN on the diagonal of a full matrix")]


@functools.lru_cache(maxsize=None)
def denormal_pivot_image():
    """(n, image [1, 64, 64], rhs [1, 64], index): a quasi-definite matrix with one uncoupled row whose diagonal
    is 1e-310: a valid pivot for the factorisation, zero for the pseudo-inverse of D (|d| <= DBL_MIN)."""
    rng = _rng("denormal")
    n, j = 6, 2
    K5 = _quasi_definite(rng, 5, 4, 1e-4)
    keep = [i for i in range(n) if i != j]
    K = np.zeros((n, n))
    K[np.ix_(keep, keep)] = K5
    K[j, j] = 1e-310
    b = np.zeros((1, 64))
    b[0, :n] = rng.standard_normal(n)
    return n, pad64(K)[None], b, j


@functools.lru_cache(maxsize=None)
def static_images(n, count=3):
    """Healthy inputs of the natural-order path: quasi-definite images as random_images, sigma = 1 and 1e-4."""
    rng = _rng("static", n)
    Ks = []
    for q in range(count):
        ne = n if (q == 0 or n == 1) else max(1, n - max(1, n // 4))
        Ks.append(_quasi_definite(rng, n, ne, 1.0 if q % 2 == 0 else 1e-4))
    b = np.zeros((count, 64))
    b[:, :n] = rng.standard_normal((count, n))
    return _freeze(pad64(np.stack(Ks)), b)


@functools.lru_cache(maxsize=None)
def static_bad_pivots(n):
    """(images, rhs, names): a positive definite matrix with one uncoupled row whose diagonal is zero, denormal,
    infinite or NaN, at the first and at the last row."""
    rng = _rng("badpivot", n)
    Ks, names = [], []
    for j in sorted({0, n - 1}):
        for name, val in (("zero", 0.0), ("denormal", 1e-310), ("infinite", np.inf), ("NaN", np.nan)):
            M = rng.standard_normal((n, n))
            K = M @ M.T / n + np.eye(n)
            K[j, :] = 0.0
            K[:, j] = 0.0
            K[j, j] = val
            Ks.append(K)
            names.append("%s pivot at %d" % (name, j))
    b = np.zeros((len(Ks), 64))
    b[:, :n] = rng.standard_normal((len(Ks), n))
    return pad64(np.stack(Ks)), b, tuple(names)


def static_spread_images(n, bits):
    """Diagonal images (pivots are the entries themselves) whose binary exponents span exactly `bits`:
    1 and 1.5 * 2^-bits.  (Identity padding counts as a pivot of one: the spread is the same for every n.)"""
    K = np.eye(n)
    K[n // 2, n // 2] = 1.5 * 2.0 ** -bits
    if n > 1:
        K[0, 0] = 1.0
    b = np.zeros((1, 64))
    b[0, :n] = 1.0
    return pad64(K)[None], b


# ---- rules -------------------------------------------------------------------------------------------------
def _ratio(res, bnd, ref, what):
    """Worst residual-to-bound ratio over everything; a non-finite residual, or a residual where the bound is
    zero, is inf.  Asserts the rule is not vacuous: the largest bound <= 1e-5 of the largest reference entry."""
    res, bnd, ref = (np.asarray(a, dtype=LD) for a in (res, bnd, ref))
    if res.size == 0:
        return 0.0
    top = np.abs(ref[np.isfinite(ref)]).max() if np.isfinite(ref).any() else LD(0)
    assert np.isfinite(bnd).all() and bnd.max() <= VACUITY * top, (what, float(bnd.max()), float(top))
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(bnd > 0, res / bnd, np.where(res == 0, LD(0), LD(np.inf)))
    q = np.where(np.isfinite(res), q, LD(np.inf))
    return float(q.max())


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _same_bits(a, b):
    return 0.0 if np.array_equal(_bits(a), _bits(b)) else np.inf


def k_reference(d, q, sigma):
    """(K, S, A' rvm, |A|' |rvm|) of QP q in longdouble: K = [tril(H) mirrored + sigma I + A' Gamma A, G';
    G, -sigma I] (n x n) and S, the sum of the magnitudes of the terms of each E entry."""
    H, G, A = d["H"][q].astype(LD), d["G"][q].astype(LD), d["A"][q].astype(LD)
    gam, rvm = d["gam"][q].astype(LD), d["rvm"][q].astype(LD)
    nz, nl = H.shape[0], G.shape[0]
    Hl = np.tril(H) + np.tril(H, -1).T
    sI = LD(sigma) * np.eye(nz, dtype=LD)
    K = np.zeros((nz + nl, nz + nl), dtype=LD)
    K[:nz, :nz] = Hl + sI + A.T @ (gam[:, None] * A)
    K[nz:, :nz] = G
    K[:nz, nz:] = G.T
    K[nz:, nz:] = -LD(sigma) * np.eye(nl, dtype=LD)
    S = np.abs(Hl) + sI + np.abs(A).T @ (gam[:, None] * np.abs(A))
    return K, S, A.T @ rvm, np.abs(A).T @ np.abs(rvm)


def assemble_rules(d, sigma, Kr, dg, atr):
    """{rule: worst ratio over the batch} for what assemble() left: Kr [count, 64, 64], dg, atr [count, 64]."""
    count, nz, nl, nv = d["H"].shape[0], d["H"].shape[1], d["G"].shape[1], d["A"].shape[1]
    n = nz + nl
    Kr, dg, atr = (np.asarray(a, dtype=np.float64) for a in (Kr, dg, atr))
    out = {"E": 0.0, "atr": 0.0}
    out["symmetric"] = _same_bits(Kr, Kr.transpose(0, 2, 1))
    out["dg"] = _same_bits(dg, Kr[:, np.arange(64), np.arange(64)])
    out["G blocks"] = max(_same_bits(Kr[:, nz:n, :nz], d["G"]), _same_bits(Kr[:, :nz, nz:n], d["G"].transpose(0, 2, 1)))
    minus_sigma = np.broadcast_to(-sigma * np.eye(nl), (count, nl, nl)) + 0.0  # (+ 0.0: off-diagonal +0, not -0)
    out["-sigma block"] = _same_bits(Kr[:, nz:n, nz:n], minus_sigma)
    pad = np.ones((64, 64), dtype=bool)
    pad[:n, :n] = False
    out["padding +0"] = 0.0 if not _bits(Kr[:, pad]).any() else np.inf
    for q in range(count):
        K, S, at, ats = k_reference(d, q, sigma)
        e = Kr[q, :nz, :nz].astype(LD)
        out["E"] = max(out["E"], _ratio(np.abs(e - K[:nz, :nz]), LD(2 * (nv + 1 + 2) * U) * S, K[:nz, :nz], "E"))
        out["atr"] = max(out["atr"], _ratio(np.abs(atr[q, :nz].astype(LD) - at), LD(2 * (nv + 2) * U) * ats, at, "atr"))
    return out


def factors_of(n, ord_, dpiv, permv, Lg):
    """(perm, L, D) in elimination order, longdouble, from one QP's device factors."""
    perm = np.asarray(permv[:n], dtype=np.int64)
    L = np.eye(n, dtype=LD)
    for k in range(n):
        L[k + 1:, k] = np.asarray(Lg[k], dtype=np.float64)[perm[k + 1:]].astype(LD)
    D = np.asarray(dpiv, dtype=np.float64)[perm].astype(LD)
    return perm, L, D


def abs_ldl(n, perm, L, D):
    """|L| |D| |L'| in the ORIGINAL order of rows and columns."""
    Mp = (np.abs(L) * np.abs(D)[None, :]) @ np.abs(L).T
    M = np.zeros((n, n), dtype=LD)
    M[np.ix_(perm, perm)] = Mp
    return M


def factor_rules(img, n, ord_, dpiv, permv, Lg):
    """{rule: worst ratio} for one QP's factors: img [64, 64], ord / dpiv / permv [64], Lg [64, 64] (Lg[k][t])."""
    out = {}
    permv, ord_ = np.asarray(permv), np.asarray(ord_)
    Lg = np.asarray(Lg, dtype=np.float64)
    is_perm = np.array_equal(np.sort(permv[:n]), np.arange(n))
    out["permutation"] = 0.0 if is_perm else np.inf
    if not is_perm:
        return out
    out["ord inverse"] = 0.0 if np.array_equal(ord_[permv[:n]], np.arange(n)) else np.inf
    gone = np.zeros((64, 64), dtype=bool)  # gone[k][t]: row t is no longer (or never was) part of step k
    gone[:, n:] = True
    gone[n:, :] = True
    for k in range(n):
        gone[k, permv[: k + 1]] = True
    out["multipliers of gone rows"] = 0.0 if not (Lg[gone] != 0.0).any() else np.inf
    perm, L, D = factors_of(n, ord_, dpiv, permv, Lg)
    K = np.asarray(img, dtype=np.float64)[:n, :n].astype(LD)
    Kp = K[np.ix_(perm, perm)]
    res = np.abs(Kp - (L * D[None, :]) @ L.T)
    bnd = LD(2 * (n + 2) * U) * ((np.abs(L) * np.abs(D)[None, :]) @ np.abs(L).T)
    out["K = L D L'"] = _ratio(res, bnd, K, "factor")
    return out


def solve_rule(img, n, b, x, M):
    """|K x - b| against 2 (n + 2) u (M |x| + |b|), M = |L| |D| |L'| in the original order."""
    K = np.asarray(img, dtype=np.float64)[:n, :n].astype(LD)
    xl, bl = np.asarray(x, dtype=np.float64)[:n].astype(LD), np.asarray(b, dtype=np.float64)[:n].astype(LD)
    res = np.abs(K @ xl - bl)
    bnd = LD(2 * (n + 2) * U) * (M @ np.abs(xl) + np.abs(bl))
    return _ratio(res, bnd, bl, "solve")


def natural_abs_ldl(img, n):
    """|L| |D| |L'| of the natural-order LDL' (float64) of an image: the scale of the static path's bound."""
    K = np.asarray(img, dtype=np.float64)[:n, :n].copy()
    L = np.eye(n)
    D = np.zeros(n)
    for k in range(n):
        D[k] = K[k, k]
        L[k + 1:, k] = K[k + 1:, k] / D[k]
        K[k + 1:, k + 1:] -= np.outer(L[k + 1:, k], K[k, k + 1:])
    return ((np.abs(L) * np.abs(D)[None, :]) @ np.abs(L).T).astype(LD)


def product_rules(d, y, rz, rl):
    """{rule: worst ratio} for y = b - A z (load_guess) and rz, rl (residual) of a problem batch."""
    H, G, A = (d[k].astype(LD) for k in ("H", "G", "A"))
    f, h, b, z, l, v = (d[k].astype(LD)[:, :, None] for k in ("f", "h", "b", "z", "l", "v"))
    nz, nl, nv = H.shape[1], G.shape[1], A.shape[1]
    Gt, At = G.transpose(0, 2, 1), A.transpose(0, 2, 1)
    out = {}
    ref = b - A @ z
    S = np.abs(b) + np.abs(A) @ np.abs(z)
    out["y"] = _ratio(np.abs(np.asarray(y)[:, :, None].astype(LD) - ref), LD(2 * (nz + 1 + 2) * U) * S, ref, "y")
    ref = f + H @ z + Gt @ l + At @ v
    S = np.abs(f) + np.abs(H) @ np.abs(z) + np.abs(Gt) @ np.abs(l) + np.abs(At) @ np.abs(v)
    out["rz"] = _ratio(np.abs(np.asarray(rz)[:, :, None].astype(LD) - ref), LD(2 * (nz + nl + nv + 1 + 2) * U) * S, ref, "rz")
    if nl:
        ref = h - G @ z
        S = np.abs(h) + np.abs(G) @ np.abs(z)
        out["rl"] = _ratio(np.abs(np.asarray(rl)[:, :, None].astype(LD) - ref), LD(2 * (nz + 1 + 2) * U) * S, ref, "rl")
    return out


# ---- Eigen's rule, restated from oracle/oracle_linalg.h (float64) ----------------------------------------------
def eigen_ldlt(K):
    """Eigen::LDLT on the lower triangle of K [n, n].  Returns dict(ok, order, klass): order[k] = the ORIGINAL
    index eliminated at step k, klass[k] in 'tie' / 'clear' / 'close' / 'last' (module docstring), and
    diag0[k] / best[k]: |original diagonal| of the row taken and the largest one on offer."""
    m = np.array(K, dtype=np.float64)
    n = m.shape[0]
    where = np.arange(n)  # where[pos] = original index of the row now stored at pos
    out = dict(ok=True, order=[], klass=[], best=[])
    if n <= 1:
        out["order"], out["klass"], out["best"] = list(range(n)), ["last"] * n, [abs(m[0, 0])] * n
        return out
    found_zero, ret = False, True
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for k in range(n):
            big, best = k, abs(m[k, k])
            for i in range(k + 1, n):
                if abs(m[i, i]) > best:
                    best, big = abs(m[i, i]), i
            rest = sorted((abs(m[i, i]) for i in range(k, n) if i != big), reverse=True)
            if not rest:
                klass = "last"
            elif rest[0] == best:
                klass = "tie"
            elif best - rest[0] > CLOSE * best:
                klass = "clear"
            else:
                klass = "close"  # (NaNs compare false: a NaN in play makes the step 'close')
            out["klass"].append(klass)
            out["best"].append(best)
            if big != k:
                m[[k, big], :k] = m[[big, k], :k]
                m[big + 1:, [k, big]] = m[big + 1:, [big, k]]
                m[k, k], m[big, big] = m[big, big], m[k, k]
                tmp = m[k + 1:big, k].copy()
                m[k + 1:big, k] = m[big, k + 1:big]
                m[big, k + 1:big] = tmp
                where[[k, big]] = where[[big, k]]
            out["order"].append(int(where[k]))
            if k > 0:
                temp = np.diag(m)[:k] * m[k, :k]
                m[k, k] -= m[k, :k] @ temp
                m[k + 1:, k] -= m[k + 1:, :k] @ temp
            akk = m[k, k]
            valid = abs(akk) > 0.0
            if k == 0 and not valid:
                out["ok"] = bool((np.tril(m, -1) == 0.0).all())
                out["order"], out["klass"], out["best"] = list(range(n)), ["zero first pivot"] * n, [best] * n
                return out
            if valid:
                m[k + 1:, k] /= akk
            else:
                ret = ret and bool((m[k + 1:, k] == 0.0).all())
            if found_zero and valid:
                ret = False
            elif not valid:
                found_zero = True
    out["ok"] = ret
    return out


def order_rule(img, n, permv):
    """(worst, share): 0 / inf for one QP's elimination order against eigen_ldlt(), and the share of its steps
    that are only 'close' (the caller caps it)."""
    K = np.asarray(img, dtype=np.float64)[:n, :n]
    e = eigen_ldlt(K)
    d0 = np.abs(np.diag(K))
    worst, close = 0.0, 0
    for k in range(n):
        p = int(permv[k])
        if e["klass"][k] == "close":
            close += 1
            ok = 0 <= p < n and d0[p] >= e["best"][k] * (1.0 - CLOSE)
        else:
            ok = p == e["order"][k]
        if not ok:
            worst = np.inf
    return worst, close / float(n)


# ---- the reference's feasibility test (full_feasibility.cc:25-88), restated ------------------------------------
def feasibility_class(d, q, dz, dl, dv, tol):
    H, G, A = d["H"][q], d["G"][q], d["A"][q]
    f, h, b = d["f"][q], d["h"][q], d["b"][q]
    d1 = (A @ dz).max()
    d2 = np.abs(G @ dz).max() if G.shape[0] else 0.0
    d3 = np.abs(H @ dz).max()
    d4 = f @ dz
    w = np.abs(dz).max()
    dual_feasible = not (d1 <= w * tol and d2 <= tol * w and d3 <= tol * w and d4 < 0 and w > 1e-14)
    p1 = np.abs(G.T @ dl + A.T @ dv).max()
    p2 = h @ dl + b @ dv
    u = max(np.abs(dv).max(), np.abs(dl).max() if dl.size else 0.0)
    primal_feasible = not (p1 <= tol * u and p2 < 0)
    if primal_feasible and dual_feasible:
        return K_FEASIBLE
    if primal_feasible:
        return K_DUAL_INFEASIBLE
    if dual_feasible:
        return K_PRIMAL_INFEASIBLE
    return K_BOTH_INFEASIBLE


@functools.lru_cache(maxsize=None)
def feasibility_cases(nz, nl, nv):
    """(problem dict, dz, dl, dv [5, .], expected classes, names): one constructed direction per class and the
    w <= 1e-14 guard.  Coordinate 0 of z is a free direction of the cost (row and column 0 of H zero, column 0 of
    G zero) along which every inequality loosens (column 0 of A positive) and f decreases; row 0 of A is zero
    with b_0 < 0: that constraint alone is unsatisfiable.  Every product that decides a class is exact."""
    rng = _rng("feasibility", nz, nl, nv)
    base = problem(nz, nl, nv, 1)
    d = {k: np.repeat(np.array(a), 5, axis=0) for k, a in base.items()}
    d["H"][:, 0, :] = 0.0
    d["H"][:, :, 0] = 0.0
    d["G"][:, :, 0] = 0.0
    d["A"][:, :, 0] = np.abs(d["A"][:, :, 0]) + 0.125
    d["A"][:, 0, :] = 0.0
    d["f"][:, 0] = 1.0
    d["b"][:, 0] = -1.0
    dz, dl, dv = np.zeros((5, nz)), np.zeros((5, nl)), np.zeros((5, nv))
    dz[0] = rng.standard_normal(nz)
    dl[0] = rng.standard_normal(nl)
    dv[0] = rng.standard_normal(nv)
    dz[1, 0] = -1.0                 # dual infeasible
    dv[2, 0] = 1.0                  # primal infeasible
    dz[3, 0], dv[3, 0] = -1.0, 1.0  # both
    dz[4, 0] = -1e-15               # the guard: a dual ray too short to count
    expected = (K_FEASIBLE, K_DUAL_INFEASIBLE, K_PRIMAL_INFEASIBLE, K_BOTH_INFEASIBLE, K_FEASIBLE)
    names = ("feasible", "dual infeasible", "primal infeasible", "both", "w <= 1e-14")
    return d, dz, dl, dv, expected, names


# ---- the restatements: float64, one rounding per operation, no lanes, no tiles ---------------------------------
class Defect:
    """Seeded defects of the restatements (tests/test_dense_wave_rules_cpu.py); none set = the restatement."""
    def __init__(self, drop_last_odd_row=False, read_upper_h=False, lowest_index_tie=False, updated_diagonal=False,
                 stale_multiplier=False, pinv_threshold_zero=False, remainder_weight_one=False,
                 no_column_check=False):
        self.drop_last_odd_row = drop_last_odd_row      # the last row of an odd nv is left out of A' Gamma A
        self.read_upper_h = read_upper_h                # E mirrored from the upper triangle of H
        self.lowest_index_tie = lowest_index_tie        # a tie goes to the lowest ORIGINAL index
        self.updated_diagonal = updated_diagonal        # the search runs on the updated (Schur) diagonal
        self.stale_multiplier = stale_multiplier        # an eliminated row keeps a non-zero multiplier
        self.pinv_threshold_zero = pinv_threshold_zero  # pseudo-inverse of D: |d| > 0 instead of |d| > DBL_MIN
        self.remainder_weight_one = remainder_weight_one  # row_dot: one clamped remainder term weighted 1
        self.no_column_check = no_column_check          # an invalid pivot over a non-zero column passes


# What fb_dense_wave.h documents for DenseWave::factor today, as a combination of the defects above: the search on the
# updated diagonal, a tie to the lowest row index, no look at the column under an invalid pivot.
DEVICE_AS_DOCUMENTED = Defect(updated_diagonal=True, lowest_index_tie=True, no_column_check=True)


def assemble_restated(d, sigma, H=None, defect=None):
    """(Kr [count, 64, 64], dg, atr [count, 64]) in float64: products and sums rounded one by one."""
    H = np.asarray(d["H"] if H is None else H)
    G, A, gam, rvm = d["G"], d["A"], d["gam"], d["rvm"]
    count, nz, nl, nv = H.shape[0], H.shape[1], G.shape[1], A.shape[1]
    n = nz + nl
    Kr = np.zeros((count, 64, 64))
    if defect is not None and defect.read_upper_h:
        E = np.triu(H) + np.triu(H, 1).transpose(0, 2, 1)
    else:
        E = np.tril(H) + np.tril(H, -1).transpose(0, 2, 1)
    E = E + sigma * np.eye(nz)
    rows = nv - 1 if (defect is not None and defect.drop_last_odd_row and nv % 2 == 1) else nv
    for k in range(rows):
        E = E + A[:, k, :, None] * (gam[:, k, None, None] * A[:, k, None, :])
    E = np.tril(E) + np.tril(E, -1).transpose(0, 2, 1)
    Kr[:, :nz, :nz] = E
    Kr[:, nz:n, :nz] = G
    Kr[:, :nz, nz:n] = G.transpose(0, 2, 1)
    Kr[:, nz:n, nz:n] = -sigma * np.eye(nl) + 0.0
    atr = np.zeros((count, 64))
    for k in range(nv):
        atr[:, :nz] = atr[:, :nz] + A[:, k, :] * rvm[:, k, None]
    return Kr, Kr[:, np.arange(64), np.arange(64)].copy(), atr


def factor_restated(img, n, defect=None):
    """DenseWave::factor on one image, float64: right-looking, nothing swapped, Eigen's rule by positions.
    Returns (ok, ord, dpiv, permv, Lg) as the device leaves them (None factors on a false verdict)."""
    Kr = np.array(img, dtype=np.float64)
    dg = np.diag(Kr).copy()
    dg0 = dg.copy()
    alive = np.arange(64) < n
    pos = np.arange(64)
    ord_, permv = np.full(64, 64), np.zeros(64, dtype=np.int64)
    dpiv, Lg = np.zeros(64), np.zeros((64, 64))
    found_zero = False
    if np.isnan(dg[:n]).any():
        return False, None, None, None, None
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for k in range(n):
            look = dg if (defect is not None and defect.updated_diagonal) else dg0
            mag = np.where(alive, np.abs(look), -1.0)
            hit = np.flatnonzero(mag == mag.max())
            if defect is not None and defect.lowest_index_tie:
                p = int(hit[0])
            else:
                p = int(hit[np.argmin(pos[hit])])
            pos[pos == k] = pos[p]
            pos[p] = k
            d = dg[p]
            permv[k] = p
            valid = abs(d) > 0.0
            colp = Kr[:, p].copy()
            alive[p] = False
            ord_[p], dpiv[p] = k, d
            if not valid and not (defect is not None and defect.no_column_check):
                if (colp[alive] != 0.0).any():
                    return False, None, None, None, None
                if k == 0 and (np.tril(Kr[:n, :n], -1) != 0.0).any():
                    return False, None, None, None, None
            if found_zero and valid:
                return False, None, None, None, None
            if not valid:
                found_zero = True
            lm = np.where(alive & valid, colp * (1.0 / d), 0.0) if valid else np.zeros(64)
            if defect is not None and defect.stale_multiplier and k > 0:
                lm[permv[0]] = 0.5
            Lg[k] = lm
            if valid:
                Kr = Kr - lm[:, None] * colp[None, :]
                dg = dg - lm * colp
    return True, ord_, dpiv, permv, Lg


def substitute_restated(n, b, ord_, dpiv, permv, Lg, defect=None):
    """DenseWave::substitute, float64: forward sweep by steps, pseudo-inverse of D, backward sweep by rows."""
    x = np.array(b, dtype=np.float64)
    thr = 0.0 if (defect is not None and defect.pinv_threshold_zero) else DBL_MIN
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for k in range(63):
            x = x - Lg[k] * x[permv[k]]
        x = np.where((np.arange(64) < n) & (np.abs(dpiv) > thr), x / np.where(dpiv == 0, 1.0, dpiv), 0.0)
        for j in range(62, -1, -1):
            x[permv[j]] = x[permv[j]] - np.sum(Lg[j] * x)
    return x


def static_restated(img, n, b, order=2, spread_bits=32):
    """DenseWave::factor_solve_static, float64: natural-order elimination of the augmented column, the verdict on
    the pivots' exponents (identity padding counts as a pivot of one up to the end of the last block of sixteen
    steps taken), backward sweep.  Returns (ok, x)."""
    K = np.array(img, dtype=np.float64)
    x = np.array(b, dtype=np.float64)
    last = 63 if n > 48 else 16 * ((n + 15) // 16)  # the last pivot looked at
    piv = np.ones(last + 1)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for k in range(last):
            piv[k] = K[k, k] if k < n else 1.0
            lm = np.zeros(64)
            lm[k + 1:] = K[k + 1:, k] * (1.0 / piv[k])
            x = x - lm * x[k]
            K[:, k + 1:] = K[:, k + 1:] - lm[:, None] * K[k, k + 1:][None, :]
        piv[last] = K[last, last] if last < n else 1.0
        e = (piv.view(np.uint64) >> np.uint64(52)) & np.uint64(0x7ff)
        emin, emax = int(e.min()), int(e.max())
        if emin == 0 or emax == 0x7ff or (order == 0 and emax - emin > spread_bits):
            return False, None
        dfull = np.ones(64)
        dfull[: last + 1] = piv
        x = x / dfull
        for j in range(last, 0, -1):
            u = np.zeros(64)
            u[:j] = K[:j, j] / dfull[:j]
            x = x - u * x[j]
    return True, x


def _row_dot(M, x, defect=None, U16=16):
    """row_dot of fb_dense_wave.h for every row of M [rows, n]: full blocks of sixteen, then the remainder with
    clamped loads and zero weights."""
    n = M.shape[1]
    s = M[:, : n - n % U16] @ x[: n - n % U16]
    if n % U16:
        k0 = n - n % U16
        for u in range(U16):
            kk = min(k0 + u, n - 1)
            w = x[kk] if k0 + u < n else 0.0
            if defect is not None and defect.remainder_weight_one and k0 + u == n:
                w = 1.0
            s = s + M[:, kk] * w
    return s


def products_restated(d, defect=None):
    count = d["H"].shape[0]
    y = np.stack([d["b"][q] - _row_dot(d["A"][q], d["z"][q], defect) for q in range(count)])
    rz = np.stack([d["f"][q] + _row_dot(d["H"][q], d["z"][q], defect) + d["G"][q].T @ d["l"][q]
                   + d["A"][q].T @ d["v"][q] for q in range(count)])
    rl = np.stack([d["h"][q] - _row_dot(d["G"][q], d["z"][q], defect) for q in range(count)])
    return y, rz, rl
