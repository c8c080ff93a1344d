"""Inputs, references, acceptance rules and plain float64 restatements for the stages of the four-wavefront dense
policy, fbstab_amd/csrc/fb_dense.h (DenseProblem<C, KGLOBAL, VGLOBAL>).  Shared by tests/test_gpu_dense_stages.py
(the device, through tests/dense_probe.py) and tests/test_dense_rules_cpu.py (the path map, the restatements with
their seeded defects, and the real header on one host thread, all through the SAME rules).  Nothing in here has
seen a device.  Problems, images, the longdouble K, Eigen's rule and the product rules come from
tests/dense_wave_rules.py, whose conventions hold here too (matrices [count, rows, cols]; u = 2^-53; a rule is a
componentwise first-order rounding bound and passes at a ratio |error| / bound <= 1; `_ratio` refuses a vacuous one).

THE PATHS.  `path_of` restates the run-time choices of fbstab_hip_dense_create, newton_step, ldlt and ldlt_solve on
the fields of DenseLayout::init, which the CPU tests take from the compiled header (tests/hostsim/dense_stage.cc).

THE FACTORS, two storage forms, both brought to (order, L, D) with P K P' = L D L', P x = x[order]:
  ldlt_impl (and ldlt_fused): L below the diagonal of the K region in its FINAL, swapped position, D on the
      diagonal, perm[k] = the position (>= k) that was swapped with k at step k - a sequence of transpositions;
      order = the transpositions applied in turn to 0 .. n - 1.  Nothing above the diagonal is ever written.
  ldlt_rows: nothing is swapped; the K region holds the multipliers, Lm[n k + t] = what row t received at step k,
      with dpiv[t], ord[t] per row and perm[k] = the row eliminated at step k (an elimination ORDER).

THE RULES that are new here (the others are those of tests/dense_wave_rules.py):
  Gamma and rv / mu.  gam = g0 / mu, rvm = -phi / mu, mu = g1 + sigma g0, with (g0, g1) the generalised gradient
      of phi at (ys, v), ys = y + sigma (v - vb), y the device's own (it is held to its rule as a product).  A
      "few ulps" cannot be the bar: g1 = alpha (1 - v / r) cancels where Gamma is large - Gamma <= 1 / sigma, and
      close to it only where g1 << sigma g0, that is 1 - v / r ~ sigma - so an ABSOLUTE error of a few u in g1 is a
      RELATIVE one of u / sigma in mu and in Gamma, whatever the code does.  The rule is the first-order bound
      that says so.  With a = ys, b = v, r = sqrt(a^2 + b^2), Ea = 2 u (|y| + sigma (|v| + |vb|)) the rounding of
      ys (two operations on terms of that size, doubled), c = 8 u (a / r carries <= 4.5 u: two squares, their sum,
      a root within an ulp, the quotient; the difference from 1, the scaling by alpha and the second term with its
      product add 3.5 u more):
        E0 = c (alpha (|a / r| + |1 - a / r|) + [a, b > 0] (1 - alpha) |b|) + alpha Ea b^2 / r^3
        E1 = c (alpha (|b / r| + |1 - b / r|) + [a, b > 0] (1 - alpha) |a|) + alpha Ea |a| b / r^3
             + [a, b > 0] (1 - alpha) Ea
        Emu = E1 + sigma E0 + 2 u |mu|
        |gam - ref| <= E0 / |mu| + |g0| Emu / mu^2 + u |gam|
        Ephi = c (alpha (|a| + |b| + r) + (1 - alpha) a+ b+) + Ea (alpha |1 - a / r| + alpha + (1 - alpha) b+)
        |rvm - ref| <= Ephi / |mu| + |phi| Emu / mu^2 + u |rvm|
      The inputs keep (ys, v) away from the kinks of the gradient (r < 1e-13, a = 0, b = 0) by far more than Ea.
  The composite assembly rule of `step`: K cannot be seen between the assembly and the factorisation, so the
      assembly is judged through the factors:
        |P K_ref P' - L D L'| <= 2 (nv + 3) u P S P' + 2 (n + 2) u |L| |D| |L'|     entrywise,
      K_ref and S (the sum of the magnitudes of the terms of each E entry; zero outside E, where K is a copy of
      the inputs' bits) from k_reference in longdouble with the DEVICE'S OWN Gamma: the assembly's inner-product
      bound (m = nv + 1 terms) plus the factorisation's.  A dropped tile, a wrong Gamma, a column read from the
      wrong slot or a missing sigma breaks it by orders of magnitude; a changed summation order does not.
  The solution of `step`: with x = [dz; dl] and rhs_ref = (-(rz + sigma (z - zb)) - A' rvm, rl + sigma (l - lb))
      in longdouble from the device's own rz, rl, rvm,
        |K_ref x - rhs_ref| <= 2 (n + 2) u (M |x| + B) + 2 (nv + 3) u S |x| + 2 (nv + 4) u B,
      M = |L| |D| |L'| in the original order, B = |rz| + sigma (|z| + |zb|) + |A|' |rvm| (and |rl| + sigma (|l| +
      |lb|)): the solve rule, the assembly's error carried to the residual, and the formation of the right-hand
      side itself (nv + 2 accumulated terms).
  adz = A dz, dv = rvm + gam adz, wz = H dz + G' dl + A' dv, wl = -G dz, given the device's own dz, dl (and its adz
      inside dv, its dv inside wz): inner-product bounds 2 (m + 2) u S with m = nz, 2, nz + nl + nv, nz.
  The ADJ form (dense_adjoint): yb = -(g0 gv), rvm = yb / mu, and the third block row in the reference's order of
      operations, dv = (yb + g0 a) / mu with a = adz: |dv - ref| <= (3 u (|yb| + |g0 a|) + E0 |a|) / |mu|
      + |dv| Emu / |mu| + u |dv|, and |yb - ref| <= u |yb| + E0 |gv|.
  The elimination ORDER of each variant is asserted bit for bit against a float64 restatement of what the code
      does - ldlt_rows: tests/dense_wave_rules.DEVICE_AS_DOCUMENTED (largest UPDATED |diagonal|, a tie to the lowest
      row index, no look at the column under an invalid pivot); ldlt_impl: largest UPDATED |diagonal|, a tie to the
      first CURRENT position after the swaps, no column check - on inputs whose longdouble run of the same rule has
      no `close` step (best and second best |diagonal| neither bitwise equal nor more than CLOSE apart):
      `close_share`, which the CPU tests assert to be zero.  A condition on the inputs, not a tolerance.
  Vacuity.  `_ratio` refuses a bound above 1e-5 of the largest entry of what it is given as the reference.  Three
      results here are what cancellation leaves of much larger terms once Gamma reaches 1e8 - the residual
      K x - rhs, dv of the ADJ form (dv_as_the_reference in fb_dense.h says why) and wz = .. + A' dv - and are
      weighed against the magnitude of those terms (|K| |x| + |rhs|, (|yb| + |g0 a|) / |mu|, S) instead; and gam, rvm,
      yb and dv are judged over the whole batch at once, because nv = 1 spreads its Gammas over the QPs.
  Exact by construction: on the ldlt_impl path everything above the diagonal of the K region keeps the probe's
      sentinel; k <= perm[k] < n there; on the ldlt_rows path perm is a permutation, ord its inverse, and rows that
      are gone carry zero multipliers; an H whose strict upper triangle is NaN changes no bit of the step but wz
      (the residual and wz = H dz + .. read the full symmetric H by design).
"""
import functools

import numpy as np

from tests.tangent_helpers import U
from tests import dense_wave_rules as wr
from tests.dense_wave_rules import (CLOSE, DBL_MIN, LD, PER_CASE, _bits, _quasi_definite, _ratio, _rng,  # noqa: F401
                                    abs_ldl, denormal_pivot_image, eigen_ldlt, feasibility_cases,
                                    feasibility_class, k_reference, problem, product_rules, singular_images,
                                    tied_images, with_nan_upper)

SENTINEL_BITS = np.uint64(0x7ff80000dead0000)
SENTINEL = np.array([SENTINEL_BITS], dtype=np.uint64).view(np.float64)[0]
SIGMAS = (1.0, 1e-8)
ALPHA = 0.95

# ---- the shapes of the device tests: ((nz, nl, nv), threads asked for) by the path they name -------------------
# (threads, assembly, factorisation, substitution, placement)
STEP_SHAPES = {
    (256, "lds", "rows", "rows", "lds"): [(1, 0, 1), (2, 1, 1), (63, 1, 3), (64, 0, 5)],
    (256, "mfma", "rows", "rows", "lds"): [(1, 0, 4), (15, 0, 4), (16, 3, 8), (17, 0, 12), (33, 3, 16), (48, 16, 4),
                                           (49, 0, 124), (64, 0, 8)],
    (256, "mfma", "impl", "impl", "lds"): [(33, 32, 4), (40, 30, 8), (64, 1, 4), (64, 6, 64)],
    (256, "lds", "impl", "impl", "lds"): [(64, 1, 30), (65, 0, 4), (64, 6, 65), (90, 5, 3)],
    (256, "global", "impl", "impl", "lds"): [(96, 0, 4), (64, 6, 68), (120, 19, 7)],
    (256, "global", "rows", "rows", "lds"): [(20, 5, 330)],
    (256, "global", "impl", "impl", "kglobal"): [(140, 0, 4), (129, 12, 5), (257, 0, 2)],
    (256, "global", "impl", "wave", "kglobal"): [(20, 5, 2435)],
    (256, "global", "impl", "wave", "vglobal"): [(20, 5, 2534)],
    (256, "global", "impl", "impl", "vglobal"): [(64, 6, 2497)],
    (64, "mfma", "rows", "rows", "lds"): [(20, 5, 40)],
    (64, "lds", "rows", "rows", "lds"): [(20, 5, 41)],  # (found by the path map, not by reading)
    (64, "mfma", "impl", "impl", "lds"): [(40, 30, 8)],
    (64, "lds", "impl", "impl", "lds"): [(64, 6, 65)],
}
STEP_CASES = [(shape, path[0]) for path, shapes in STEP_SHAPES.items() for shape in shapes]
# images: (n, nv, threads asked for) -> (factorisation, substitution, placement); nv only selects the placement
FACTOR_CASES = {
    "rows": [(1, 4, 256), (2, 4, 256), (63, 4, 256), (64, 4, 256)],
    "impl": [(65, 4, 256), (66, 4, 256), (128, 4, 256), (129, 4, 256), (130, 4, 256)],
    "impl 64": [(65, 4, 64)],
    "impl kglobal": [(257, 4, 256)],
    "impl kglobal, solve_wave": [(25, 2435, 256)],
}
FACTOR_PATHS = {"rows": (256, "rows", "rows", "lds"), "impl": (256, "impl", "impl", "lds"),
                "impl 64": (64, "impl", "impl", "lds"), "impl kglobal": (256, "impl", "impl", "kglobal"),
                "impl kglobal, solve_wave": (256, "impl", "wave", "kglobal")}
# the tied, singular and denormal families run at their natural n <= 64, (nv, threads asked for, ldlt_rows?): ldlt_rows
# with K in LDS at 256 and 64 threads, and ldlt_impl with ldlt_solve_wave (nv = 4000 puts K and the vectors into
# global scratch whatever n is)
FAMILY_PATHS = [(4, 256, True), (4, 64, True), (4000, 256, False)]
# one shape per placement for `feasibility`: ((nz, nl, nv), threads)
FEASIBILITY_CASES = [((17, 3, 33), 256), ((96, 3, 5), 256), ((140, 3, 5), 256), ((20, 5, 2534), 256), ((17, 3, 33), 64)]
FEASIBILITY_PLACEMENTS = [("lds", 1), ("lds", 0), ("kglobal", 0), ("vglobal", 0), ("lds", 1)]  # (placement, a_lds)


def path_of(layout, nz, nl, nv, want):
    """The path (dict) the product takes for a shape and a workgroup width asked for.  `layout(nz, nl, nv, nt)`
    returns DenseLayout::init's wave, k_global, v_global, a_lds.  Restated: fbstab_hip_dense_create's fall-back
    from 64 threads, and the branches of newton_step, ldlt and ldlt_solve."""
    nt = want
    lay = layout(nz, nl, nv, nt)
    if nt == 64 and (lay["k_global"] or not lay["a_lds"]):
        nt = 256
        lay = layout(nz, nl, nv, nt)
    kg, nk = bool(lay["k_global"]), nz + nl
    if lay["a_lds"] and nt % 64 == 0 and nz <= 64 and nv % 4 == 0:
        assembly = "mfma"
    else:
        assembly = "lds" if lay["a_lds"] else "global"
    if not kg and nt >= 64 and lay["wave"]:
        factorisation = substitution = "rows"
    else:
        factorisation = "fused" if (not kg and nt > 64 and nk <= 64) else "impl"
        substitution = "wave" if nk <= 64 else "impl"
    placement = "vglobal" if lay["v_global"] else "kglobal" if kg else "lds"
    return dict(threads=nt, assembly=assembly, factorisation=factorisation, substitution=substitution,
                placement=placement, a_lds=int(lay["a_lds"]))


def path_key(p, with_assembly=True):
    return (p["threads"],) + ((p["assembly"],) if with_assembly else ()) + (p["factorisation"], p["substitution"],
                                                                          p["placement"])


# ---- inputs ----------------------------------------------------------------------------------------------------
def _gamma_targets(rng, count, nv):
    g = 10.0 ** rng.uniform(-12.0, 8.0, (count, nv))
    if nv >= 2:  # (as dense_wave_rules.problem: the heaviest weights on the last rows, the lightest somewhere before)
        for q in range(count):
            g[q, nv - 1] = 1e8
            if q % 2 == 1 and nv >= 3:
                g[q, nv - 2] = 1e8
            g[q, rng.integers(0, max(1, nv - 2))] = 1e-12
    else:
        g[:, 0] = np.array([1e-12, 1.0, 1e8] * count)[:count]
    return g


@functools.lru_cache(maxsize=None)
def step_inputs(nz, nl, nv, sigma, adjoint=False, count=PER_CASE):
    """(d, xb): the problem batch of dense_wave_rules.problem with a point (ys, v) per constraint that makes the
    step's own Gamma span 1e-12 .. min(1e8, ~ 1 / sigma) within a QP (Gamma < 1 / sigma whatever the point is), and
    xb = (zb, lb, vb) - or, adjoint, the seeds (gz, gl, gv), with b moved so that y = b - A z is the wanted ys
    (dense_adjoint sets xbar = x).  Targets g < 1e-2: ys = 1, v = 20 g (g0 ~ (1 - alpha) v); g >= 1e-2: v = 1,
    ys = -sqrt(2 / g) (g1 ~ alpha ys^2 / 2), the topmost ys = -1e-6."""
    base = problem(nz, nl, nv, count)
    rng = _rng("step", nz, nl, nv, int(adjoint))
    g = _gamma_targets(rng, count, nv)
    small = g < 1e-2
    v = np.where(small, 20.0 * g, 1.0)
    ys = np.where(small, 1.0, -np.sqrt(2.0 / np.maximum(g, 1e-2)))
    ys = np.where(g >= 1e8, -1e-6, ys)
    d = dict(base, v=v)
    Az = np.einsum("qij,qj->qi", base["A"], base["z"])
    if adjoint:
        d["b"] = ys + Az
        xb = (rng.standard_normal((count, nz)), rng.standard_normal((count, nl)),
              rng.standard_normal((count, nv)) * 10.0 ** rng.uniform(-3.0, 3.0, (count, nv)))
    else:
        xb = (0.5 * base["z"], 0.5 * base["l"], v - (ys - (base["b"] - Az)) / sigma)
    for a in list(d.values()) + list(xb):
        a.setflags(write=False)
    return d, xb


@functools.lru_cache(maxsize=None)
def images(n, count=PER_CASE):
    """(images [count, n, n], rhs [count, n]): quasi-definite, a quarter of the rows equality rows (none for the
    first QP), sigma = 1 and 1e-4 in turn - dense_wave_rules.random_images without the padding, any n."""
    rng = _rng("dense images", n)
    Ks = []
    for q in range(count):
        ne = n if (q == 0 or n == 1) else max(1, n - max(1, n // 4))
        Ks.append(_quasi_definite(rng, n, ne, 1.0 if q % 2 == 0 else 1e-4))
    K, b = np.stack(Ks), rng.standard_normal((count, n))
    K.setflags(write=False)
    b.setflags(write=False)
    return K, b


def embed(K64, n, m):
    """An n x n image of the 64-padded families inside an m x m one (m >= n): the rest is a graded positive
    diagonal, smaller than every |diagonal| of the image that is not zero, so that it is eliminated behind it."""
    K = np.zeros((m, m))
    K[:n, :n] = np.asarray(K64)[:n, :n]
    dg = np.abs(np.diag(K)[:n])
    floor = dg[dg > 0].min() if (dg > 0).any() else 1.0
    for i in range(n, m):
        K[i, i] = floor * 0.5 ** (1 + (i - n) % 40) * (1.0 + (i - n) / (4.0 * m))
    return K


@functools.lru_cache(maxsize=None)
def handover_image(n=129):
    """(image [1, n, n], rhs [1, n]): at step k = n - 65 - where 65 candidates are left, one more than a wavefront
    holds - the largest diagonal sits at the LAST position; before it the pivots come in natural order.  A search
    that hands over to the first wavefront one step early never sees that candidate."""
    rng = _rng("handover", n)
    k0 = n - 65
    dg = np.concatenate([1000.0 - np.arange(k0), 100.0 - 0.25 * np.arange(64), [500.0]])
    C = 1e-3 * rng.standard_normal((n, n))
    K = np.diag(dg) + np.tril(C, -1) + np.tril(C, -1).T
    return K[None], rng.standard_normal((1, n))


# ---- the factors, from both storage forms ------------------------------------------------------------------------
def factors_of_impl(n, perm, Kf):
    """(order, L, D) from ldlt_impl's K region (Kf[i, j] = K[i + j n]) and its transpositions."""
    order = np.arange(n)
    for k in range(n):
        p = int(perm[k])
        order[[k, p]] = order[[p, k]]
    Kf = np.asarray(Kf, dtype=np.float64)
    return order, np.tril(Kf, -1).astype(LD) + np.eye(n, dtype=LD), np.diag(Kf).astype(LD)


def factors_of_rows(n, perm, flat, dpiv, ord_):
    """(order, L, D) from ldlt_rows' multipliers (flat[n k + t]), pivots and elimination order."""
    return wr.factors_of(n, ord_, dpiv, perm, np.asarray(flat, dtype=np.float64)[: n * n].reshape(n, n))


def factors_of(got, q, n, rows):
    if rows:
        return factors_of_rows(n, got["perm"][q], got["flat"][q], got["dpiv"][q], got["ord"][q])
    return factors_of_impl(n, got["perm"][q], got["K"][q])


def structure_rules(got, q, n, rows, sentinel):
    """{rule: 0 / inf}: what is exact by construction in the factors of QP q."""
    out = {}
    perm = np.asarray(got["perm"][q][:n], dtype=np.int64)
    if rows:
        ok = np.array_equal(np.sort(perm), np.arange(n))
        out["permutation"] = 0.0 if ok else np.inf
        if ok:
            ord_ = np.asarray(got["ord"][q])
            out["ord inverse"] = 0.0 if np.array_equal(ord_[perm], np.arange(n)) else np.inf
            Lg = np.asarray(got["flat"][q])[: n * n].reshape(n, n)
            gone = np.zeros((n, n), dtype=bool)
            for k in range(n):
                gone[k, perm[: k + 1]] = True
            out["multipliers of gone rows"] = 0.0 if not (Lg[gone] != 0.0).any() else np.inf
    else:
        ok = bool(((perm >= np.arange(n)) & (perm < n)).all())
        out["transpositions"] = 0.0 if ok else np.inf
        if sentinel:
            up = _bits(np.asarray(got["K"][q]))[np.triu_indices(n, 1)]
            out["nothing written above the diagonal"] = 0.0 if (up == SENTINEL_BITS).all() else np.inf
    out["structure"] = 0.0 if ok else np.inf
    return out


def factor_rule(K, order, L, D, m, S=None):
    """|P K P' - L D L'| against 2 (m + 2) u |L| |D| |L'| (+ 2 (nv + 3) u P S P' where S is given as that term)."""
    K = np.asarray(K, dtype=LD)
    Kp = K[np.ix_(order, order)]
    res = np.abs(Kp - (L * D[None, :]) @ L.T)
    bnd = LD(2 * (m + 2) * U) * ((np.abs(L) * np.abs(D)[None, :]) @ np.abs(L).T)
    if S is not None:
        bnd = bnd + S[np.ix_(order, order)]
    return _ratio(res, bnd, K, "factor")


def mirrored(K):
    """The symmetric matrix whose lower triangle is K's."""
    K = np.asarray(K)
    return np.tril(K) + np.tril(K, -1).T


def image_rules(K, b, got, q, rows):
    """{rule: ratio} for `factor` on image K [n, n] with right-hand side b: structure, K = L D L', the solve."""
    n = K.shape[0]
    out = structure_rules(got, q, n, rows, sentinel=False)
    if out.pop("structure") != 0.0:
        return out
    order, L, D = factors_of(got, q, n, rows)
    Ks = mirrored(K)
    out["K = L D L'"] = factor_rule(Ks, order, L, D, n)
    out["solve"] = wr.solve_rule(Ks, n, b, got["x"][q], abs_ldl(n, order, L, D))
    return out


# ---- the pieces of the step in longdouble --------------------------------------------------------------------------
def pfb_terms(ys, v, alpha, sigma, Ea):
    """dict of g0, g1, mu, phi and their error bounds E0, Emu, Ephi (module docstring), longdouble."""
    a, b, Ea = np.asarray(ys, dtype=LD), np.asarray(v, dtype=LD), np.asarray(Ea, dtype=LD)
    al, sg, c = LD(alpha), LD(sigma), LD(8 * U)
    r = np.sqrt(a * a + b * b)
    rs = np.where(r > 0, r, LD(1))
    ar, br = a / rs, b / rs
    both = ((a > 0) & (b > 0)).astype(LD)
    g0 = al * (1 - ar) + both * (1 - al) * b
    g1 = al * (1 - br) + both * (1 - al) * a
    flat = r < LD(1e-13)
    kink = al * (1 - LD(0.70710678118654752440))
    g0, g1 = np.where(flat, kink, g0), np.where(flat, kink, g1)
    E0 = c * (al * (np.abs(ar) + np.abs(1 - ar)) + both * (1 - al) * np.abs(b)) + al * Ea * b * b / rs ** 3
    E1 = (c * (al * (np.abs(br) + np.abs(1 - br)) + both * (1 - al) * np.abs(a)) + al * Ea * np.abs(a) * b / rs ** 3
          + both * (1 - al) * Ea)
    mu = g1 + sg * g0
    Emu = E1 + sg * E0 + LD(2 * U) * np.abs(mu)
    ap, bp = np.maximum(a, 0), np.maximum(b, 0)
    phi = al * (a + b - r) + (1 - al) * ap * bp
    Ephi = c * (al * (np.abs(a) + np.abs(b) + r) + (1 - al) * ap * bp) + Ea * (al * np.abs(1 - ar) + al + (1 - al) * bp)
    return dict(g0=g0, g1=g1, mu=mu, phi=phi, E0=E0, Emu=Emu, Ephi=Ephi)


def _vec(a, q):
    return np.asarray(a[q], dtype=np.float64).astype(LD)


def step_rules(d, xb, sigma, got, rows, alpha=ALPHA, adjoint=False, sentinel=True):
    """{rule: worst ratio over the batch} for what `step` left (tests/dense_probe.DenseProbe.step's dict)."""
    count, nz, nl, nv = d["H"].shape[0], d["H"].shape[1], d["G"].shape[1], d["A"].shape[1]
    n = nz + nl
    out = {"verdict": 0.0 if (np.asarray(got["verdict"]) == 1).all() else np.inf}
    if out["verdict"] != 0.0:
        return out

    def worst(name, r):
        out[name] = max(out.get(name, 0.0), r)

    if not adjoint:
        for k, r in product_rules(d, got["y"], got["rz"], got["rl"]).items():
            worst(k, r)
    # Gamma and rv / mu, over the whole batch at once (nv = 1 spreads its Gammas over the QPs: `_ratio` weighs the
    # largest bound against the largest reference entry of what it is given)
    f64 = lambda a: np.asarray(a, dtype=np.float64).astype(LD)
    y, v, gam, rvm = f64(got["y"]), f64(d["v"]), f64(got["gam"]), f64(got["rvm"])
    vb = v if adjoint else f64(xb[2])
    Ea = LD(2 * U) * (np.abs(y) + LD(sigma) * (np.abs(v) + np.abs(vb)))
    t = pfb_terms(y + LD(sigma) * (v - vb), v, alpha, sigma, Ea)
    mu, amu = t["mu"], np.abs(t["mu"])
    ref = t["g0"] / mu
    worst("gam", _ratio(np.abs(gam - ref), t["E0"] / amu + np.abs(t["g0"]) * t["Emu"] / mu ** 2 + LD(U) * np.abs(ref),
                        ref, "gam"))
    if adjoint:
        gv = f64(xb[2])
        ref = -(t["g0"] * gv)
        Eyb = LD(U) * np.abs(ref) + t["E0"] * np.abs(gv)
        worst("yb", _ratio(np.abs(f64(got["yb"]) - ref), Eyb, ref, "yb"))
        ref = ref / mu
        worst("rvm", _ratio(np.abs(rvm - ref), Eyb / amu + np.abs(ref) * t["Emu"] / amu + LD(U) * np.abs(ref), ref,
                            "rvm"))
    else:
        ref = -t["phi"] / mu
        worst("rvm", _ratio(np.abs(rvm - ref), t["Ephi"] / amu + np.abs(t["phi"]) * t["Emu"] / mu ** 2
                            + LD(U) * np.abs(ref), ref, "rvm"))
    dv_parts = []
    for q in range(count):
        H, G, A = (d[k][q].astype(LD) for k in ("H", "G", "A"))
        z, l, v = _vec(d["z"], q), _vec(d["l"], q), _vec(d["v"], q)
        y, gam, rvm = _vec(got["y"], q), _vec(got["gam"], q), _vec(got["rvm"], q)
        sg = LD(sigma)
        if adjoint:
            zb, lb, vb = z, l, v
            rz, rl = -_vec(xb[0], q), _vec(xb[1], q)
            worst("rz, rl are the seeds", wr._same_bits(got["rz"][q], -np.asarray(xb[0][q])))
        else:
            zb, lb, vb = (_vec(t, q) for t in xb)
            rz, rl = _vec(got["rz"], q), _vec(got["rl"], q)
        Ea = LD(2 * U) * (np.abs(y) + sg * (np.abs(v) + np.abs(vb)))
        t = pfb_terms(y + sg * (v - vb), v, alpha, sigma, Ea)
        mu, amu = t["mu"], np.abs(t["mu"])
        if adjoint:
            yb = _vec(got["yb"], q)
        # the factors against K_ref built with the device's own Gamma
        for k, r in structure_rules(got, q, n, rows, sentinel).items():
            worst(k, r)
        if out["structure"] != 0.0:
            continue
        dd = {"H": d["H"], "G": d["G"], "A": d["A"], "gam": got["gam"], "rvm": got["rvm"]}
        K, S, _, _ = k_reference(dd, q, sigma)
        Sn = np.zeros((n, n), dtype=LD)
        Sn[:nz, :nz] = S
        order, L, D = factors_of(got, q, n, rows)
        worst("P K P' = L D L'", factor_rule(K, order, L, D, n, LD(2 * (nv + 3) * U) * Sn))
        # the solution
        x = np.concatenate([_vec(got["dz"], q), _vec(got["dl"], q)])
        dz, dl = x[:nz], x[nz:]
        rhs = np.concatenate([-(rz + sg * (z - zb)) - A.T @ rvm, rl + sg * (l - lb)])
        B = np.concatenate([np.abs(rz) + sg * (np.abs(z) + np.abs(zb)) + np.abs(A).T @ np.abs(rvm),
                            np.abs(rl) + sg * (np.abs(l) + np.abs(lb))])
        M = abs_ldl(n, order, L, D)
        bnd = (LD(2 * (n + 2) * U) * (M @ np.abs(x) + B) + LD(2 * (nv + 3) * U) * (Sn @ np.abs(x))
               + LD(2 * (nv + 4) * U) * B)
        # (the scale of the vacuity check is that of the residual's own terms, |K| |x|: with Gamma at 1e8 the
        #  right-hand side is what is left of them after cancellation)
        worst("solve", _ratio(np.abs(K @ x - rhs), bnd, np.abs(K) @ np.abs(x) + np.abs(rhs), "solve"))
        # what follows the solve
        adz, dv = _vec(got["adz"], q), _vec(got["dv"], q)
        ref = A @ dz
        worst("adz", _ratio(np.abs(adz - ref), LD(2 * (nz + 2) * U) * (np.abs(A) @ np.abs(dz)), ref, "adz"))
        if adjoint:
            ref = (yb + t["g0"] * adz) / mu
            bnd = ((LD(3 * U) * (np.abs(yb) + np.abs(t["g0"] * adz)) + t["E0"] * np.abs(adz)) / amu
                   + np.abs(ref) * t["Emu"] / amu + LD(U) * np.abs(ref))
            scale = (np.abs(yb) + np.abs(t["g0"] * adz)) / amu
        else:
            ref = rvm + gam * adz
            bnd = LD(2 * 4 * U) * (np.abs(rvm) + np.abs(gam * adz))
            scale = np.abs(rvm) + np.abs(gam * adz)
        # (judged over the batch, like Gamma, whose error dv inherits; the vacuity check on the scale of the two
        #  terms of dv, which cancel on active rows - fb_dense.h: dv_as_the_reference)
        dv_parts.append((np.abs(dv - ref), bnd, scale))
        ref = H @ dz + G.T @ dl + A.T @ dv
        Sw = np.abs(H) @ np.abs(dz) + np.abs(G).T @ np.abs(dl) + np.abs(A).T @ np.abs(dv)
        # (vacuity on the scale of the terms: A' dv cancels against the rest where dv is large)
        worst("wz", _ratio(np.abs(_vec(got["wz"], q) - ref), LD(2 * (nz + nl + nv + 2) * U) * Sw, Sw, "wz"))
        if nl:
            ref = -(G @ dz)
            worst("wl", _ratio(np.abs(_vec(got["wl"], q) - ref), LD(2 * (nz + 2) * U) * (np.abs(G) @ np.abs(dz)), ref,
                               "wl"))
    if dv_parts:
        worst("dv", _ratio(*(np.concatenate(a) for a in zip(*dv_parts)), "dv"))
    out.pop("structure", None)
    return out


def products_extra_rules(d, got, a_lds):
    """forcing_norm (a root of nz + nl + nv squares: (m + 3) u relative, doubled) and the LDS copy of A (bitwise)."""
    out = {}
    terms = np.concatenate([d["f"], d["h"], d["b"]], axis=1).astype(LD)
    ref = np.sqrt((terms * terms).sum(axis=1))
    out["forcing_norm"] = _ratio(np.abs(np.asarray(got["nrm"]).astype(LD) - ref), LD(2 * (terms.shape[1] + 3) * U) * ref,
                                 ref, "norm")
    if a_lds:
        out["A in LDS by rows"] = wr._same_bits(got["a_rows"], d["A"] + 0.0)
        out["A in LDS by columns"] = wr._same_bits(got["a_cols"], d["A"] + 0.0)
    return out


# ---- the elimination order -----------------------------------------------------------------------------------------
def close_share(K, rows):
    """The share of steps of the longdouble run of a variant's pivot rule (rows: ldlt_rows; else ldlt_impl) on the
    lower triangle of K that are `close`: best and second best |diagonal| on offer not equal and within CLOSE."""
    m = mirrored(K).astype(LD)
    n = m.shape[0]
    alive = np.ones(n, dtype=bool)
    pos = np.arange(n)
    close = 0
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for k in range(n):
            mag = np.where(alive, np.abs(np.diag(m)), LD(-1))
            best = mag.max()
            hit = np.flatnonzero(mag == best)
            p = int(hit[0]) if rows else int(hit[np.argmin(pos[hit])])
            rest = mag[alive & (np.arange(n) != p)]
            if rest.size and rest.max() != best and best - rest.max() <= LD(CLOSE) * best:
                close += 1
            pos[pos == k] = pos[p]
            pos[p] = k
            alive[p] = False
            dd = m[p, p]
            if abs(dd) > 0:
                lm = np.where(alive, m[:, p] / dd, LD(0))
                m = m - lm[:, None] * m[p, :][None, :]
    return close / float(n)


def order_restated(K, rows, nt=256):
    """perm as the variant's float64 restatement leaves it on image K (None on a false verdict)."""
    n = K.shape[0]
    if rows:
        r = wr.factor_restated(wr.pad64(mirrored(K)), n, wr.DEVICE_AS_DOCUMENTED)
        return None if not r[0] else np.asarray(r[3][:n])
    r = ldlt_impl_restated(K, nt)
    return r[1] if r[0] else None


def eigen_order(K):
    return np.asarray(eigen_ldlt(mirrored(K))["order"])


def elimination_order(perm, rows):
    """The original index eliminated at each step, from either form of perm."""
    if rows:
        return np.asarray(perm)
    order = np.arange(len(perm))
    for k in range(len(perm)):
        p = int(perm[k])
        order[[k, p]] = order[[p, k]]
    return order


# ---- the restatements: float64, one rounding per operation, the tile, chunk and swap structure explicit --------------
class Defect:
    """Seeded defects of the restatements (tests/test_dense_rules_cpu.py); none set = the restatement."""
    NAMES = ("skip_last_row_tile", "pad_from_column_0", "chunk_writes_all", "gamma_missing", "skip_middle_segment",
             "handover_off_by_one", "forward_undo", "pinv_threshold_zero", "lda_read_nv")

    def __init__(self, **kw):
        for name in self.NAMES:
            setattr(self, name, bool(kw.pop(name, False)))
        assert not kw, kw
    # skip_last_row_tile:  the MFMA assembly skips the last tile of the last block row
    # pad_from_column_0:   a padded column of an MFMA operand is re-read from column 0 instead of nz - 1
    # chunk_writes_all:    the LDS-scalar assembly writes every column of a JC chunk (j > i, j >= nz)
    # gamma_missing:       Gamma is missing from the second operand of A' Gamma A
    # skip_middle_segment: ldlt_impl's swap leaves out the segment k + 1 .. p - 1
    # handover_off_by_one: ldlt_impl's search goes to the first wavefront at n - k <= 65
    # forward_undo:        ldlt_solve_impl undoes the transpositions in forward order
    # pinv_threshold_zero: pseudo-inverse of D: |d| > 0 instead of |d| > DBL_MIN
    # lda_read_nv:         the LDS copy of A is read with lda = nv where it was written with nv | 1


NONE = Defect()


def pfb_gradient64(a, b, alpha):
    r = np.sqrt(a * a + b * b)
    rs = np.where(r > 0, r, 1.0)
    both = (a > 0) & (b > 0)
    g0 = alpha * (1.0 - a / rs) + np.where(both, (1.0 - alpha) * b, 0.0)
    g1 = alpha * (1.0 - b / rs) + np.where(both, (1.0 - alpha) * a, 0.0)
    kink = alpha * (1.0 - 0.70710678118654752440)
    return np.where(r < 1e-13, kink, g0), np.where(r < 1e-13, kink, g1)


def pfb64(a, b, alpha):
    return alpha * (a + b - np.sqrt(a * a + b * b)) + (1.0 - alpha) * np.maximum(a, 0.0) * np.maximum(b, 0.0)


def assemble_restated(H, G, A, gam, rhs_in, sigma, branch, defect=NONE):
    """(K [n, n] with K[i, j] = what the K region holds at i + j n - the sentinel where nothing was written -, rhs)
    for one QP: newton_step's three assemblies.  rhs_in = (rz, rl, z, zb, l, lb, rvm).  `branch`: mfma / lds /
    global."""
    nz, nl, nv = H.shape[0], G.shape[0], A.shape[0]
    n = nz + nl
    mem = np.full(n * n + n, SENTINEL)  # the K region by columns; what follows it takes writes past its end
    Kv = mem[: n * n].reshape(n, n).T   # (a view: Kv[i, j] is mem[i + j n])
    lda = nv | 1
    Al = np.full(lda * nz, np.nan)
    Al.reshape(nz, lda)[:, :nv] = A.T   # load_guess: Al[(e % nv) + (e / nv) lda] = A[e]
    lda_r = nv if defect.lda_read_nv else lda
    col = lambda c: Al[c * lda_r: c * lda_r + nv]
    gw = np.ones(nv) if defect.gamma_missing else gam
    if branch == "mfma":
        nt16 = (nz + 15) // 16
        for I in range(nt16):
            for J in range(I + 1):
                if defect.skip_last_row_tile and I == nt16 - 1 and J == I:
                    continue
                ij = np.arange(16)
                pad = 0 if defect.pad_from_column_0 else nz - 1
                ci = np.where(16 * I + ij < nz, 16 * I + ij, pad)
                cj = np.where(16 * J + ij < nz, 16 * J + ij, pad)
                Ai = np.stack([col(c) for c in ci])
                Bj = np.stack([gw * col(c) for c in cj])
                acc = np.zeros((16, 16))
                for k0 in range(0, nv, 4):  # one v_mfma_f64_16x16x4 per four rows of A
                    acc = acc + Ai[:, k0:k0 + 4] @ Bj[:, k0:k0 + 4].T
                for r in range(16):
                    for c in range(16):
                        i, j = 16 * I + r, 16 * J + c
                        if i < nz and j <= i:
                            Kv[i, j] = H[i, j] + (sigma if i == j else 0.0) + acc[r, c]
    elif branch == "lds":
        JC = 6
        for i in range(nz):
            g = gw * col(i)
            for j0 in range(0, i + 1, JC):
                for m in range(JC):
                    j = j0 + m
                    off = m * lda_r if j < nz else 0  # columns past nz re-read column j0
                    acc = Al[j0 * lda_r + off: j0 * lda_r + off + nv] @ g
                    if (j <= i and j < nz) or defect.chunk_writes_all:
                        h = H[i, j] if j < nz else 0.0
                        if i + j * n < mem.size:
                            mem[i + j * n] = h + (sigma if i == j else 0.0) + acc
    else:
        for i in range(nz):
            for j in range(i + 1):
                Kv[i, j] = H[i, j] + (sigma if i == j else 0.0) + np.sum(gw * A[:, i] * A[:, j])
    Kv[nz:, :nz] = G
    for i in range(nz, n):
        for j in range(nz, i + 1):
            Kv[i, j] = -sigma if i == j else 0.0
    rz, rl, z, zb, l, lb, rvm = rhs_in
    atr = np.array([col(j) @ rvm for j in range(nz)]) if branch != "global" else A.T @ rvm
    rhs = np.concatenate([-(rz + sigma * (z - zb)) - atr, rl + sigma * (l - lb)])
    return Kv.copy(), rhs


def ldlt_impl_restated(K, nt=256, defect=NONE):
    """ldlt_impl on the lower triangle of K: (ok, perm, Kf); the part above the diagonal is not touched."""
    m = np.array(K, dtype=np.float64)
    n = m.shape[0]
    perm = np.zeros(n, dtype=np.int64)
    if np.isnan(np.diag(m)).any():  # (the pre-check of `ldlt`)
        return False, None, None
    found_zero = False
    hand = 65 if defect.handover_off_by_one else 64
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for k in range(n):
            look = np.abs(np.diag(m)[k:])
            if nt > 64 and n - k <= hand:
                look = look[:64]  # the first wavefront decides alone: the candidates of its 64 lanes
            p = k + int(np.argmax(look))  # the first maximum by current position
            perm[k] = p
            if p != k:
                m[[k, p], :k] = m[[p, k], :k]
                m[p + 1:, [k, p]] = m[p + 1:, [p, k]]
                if not defect.skip_middle_segment:
                    tmp = m[k + 1:p, k].copy()
                    m[k + 1:p, k] = m[p, k + 1:p]
                    m[p, k + 1:p] = tmp
                m[k, k], m[p, p] = m[p, p], m[k, k]
            dd = m[k, k]
            valid = abs(dd) > 0.0
            if found_zero and valid:
                return False, None, None
            if not valid:
                found_zero = True
            if n - k - 1 > 0 and valid:
                idd = 1.0 / dd
                c = m[k + 1:, k].copy()
                upd = np.tril(np.outer(c, c * idd))  # K(i, j) -= K(i, k) (K(j, k) / d), i >= j
                low = np.tril_indices(n - k - 1)
                sub = m[k + 1:, k + 1:]
                sub[low] = sub[low] - upd[low]
                m[k + 1:, k] = c * idd
    return True, perm, m


def ldlt_solve_impl_restated(Kf, perm, b, defect=NONE):
    """ldlt_solve_impl (and ldlt_solve_wave, the same formulas on one wavefront)."""
    x = np.array(b, dtype=np.float64)
    n = x.size
    thr = 0.0 if defect.pinv_threshold_zero else DBL_MIN
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for k in range(n):
            p = perm[k]
            x[k], x[p] = x[p], x[k]
        for k in range(n - 1):
            x[k + 1:] = x[k + 1:] - Kf[k + 1:, k] * x[k]
        dg = np.diag(Kf)
        x = np.where(np.abs(dg) > thr, x / np.where(dg == 0, 1.0, dg), 0.0)
        for k in range(n - 1, 0, -1):
            x[:k] = x[:k] - Kf[k, :k] * x[k]
        for k in (range(n) if defect.forward_undo else range(n - 1, -1, -1)):
            p = perm[k]
            x[k], x[p] = x[p], x[k]
    return x


def factor_restated(K, b, rows, nt=256, defect=NONE):
    """`factor` of the probe on one image: dict as one QP of DenseProbe.factor (leading axis of one)."""
    n = K.shape[0]
    out = dict(verdict=np.zeros(1, dtype=np.int32), perm=np.full((1, n), -1), K=np.full((1, n, n), np.nan),
               flat=np.full((1, n * n), np.nan), dpiv=np.full((1, 64), np.nan), ord=np.full((1, 64), -1),
               x=np.full((1, n), np.nan))
    if rows:
        ok, ord_, dpiv, permv, Lg = wr.factor_restated(wr.pad64(mirrored(K)), n, wr.DEVICE_AS_DOCUMENTED)
        if not ok:
            return out
        b64 = np.zeros(64)
        b64[:n] = b
        thr = wr.Defect(pinv_threshold_zero=defect.pinv_threshold_zero)
        out.update(perm=permv[None, :n], flat=Lg[:n, :n].reshape(1, -1), dpiv=dpiv[None], ord=ord_[None],
                   x=wr.substitute_restated(n, b64, ord_, dpiv, permv, Lg, thr)[None, :n])
    else:
        ok, perm, Kf = ldlt_impl_restated(K, nt, defect)
        if not ok:
            return out
        out.update(perm=perm[None], K=Kf[None], x=ldlt_solve_impl_restated(Kf, perm, b, defect)[None])
    out["verdict"][0] = 1
    return out


def step_restated(d, xb, sigma, path, alpha=ALPHA, adjoint=False, defect=NONE, h_step=None):
    """`step` of the probe in float64 along `path` (path_of's dict): the dict of DenseProbe.step."""
    count, nz, nl, nv = d["H"].shape[0], d["H"].shape[1], d["G"].shape[1], d["A"].shape[1]
    n = nz + nl
    rows = path["factorisation"] == "rows"
    keys = ("verdict", "perm", "K", "flat", "dpiv", "ord", "y", "rz", "rl", "dz", "dl", "dv", "adz", "wz", "wl", "gam",
            "rvm", "yb")
    res = {k: [] for k in keys}
    for q in range(count):
        Hs = np.asarray(d["H"] if h_step is None else h_step)[q]
        H, G, A = d["H"][q], d["G"][q], d["A"][q]
        z, l, v = d["z"][q], d["l"][q], d["v"][q]
        y = d["b"][q] - A @ z
        if adjoint:
            zb, lb, vb = z, l, v
            rz, rl = -xb[0][q], xb[1][q] + 0.0
        else:
            zb, lb, vb = (t[q] for t in xb)
            rz = d["f"][q] + H @ z + G.T @ l + A.T @ v
            rl = d["h"][q] - G @ z
        ys = y + sigma * (v - vb)
        g0, g1 = pfb_gradient64(ys, v, alpha)
        mu = g1 + sigma * g0
        gam = g0 / mu
        if adjoint:
            yb = -(g0 * xb[2][q])
            rvm = yb / mu
        else:
            yb = np.full(nv, np.nan)
            rvm = -pfb64(ys, v, alpha) / mu
        K, rhs = assemble_restated(Hs, G, A, gam, (rz, rl, z, zb, l, lb, rvm), sigma, path["assembly"], defect)
        with np.errstate(invalid="ignore"):
            f = factor_restated(K, rhs, rows, path["threads"], defect)
        for k in ("verdict", "perm", "K", "flat", "dpiv", "ord"):
            res[k].append(f[k][0])
        x = f["x"][0]
        dz, dl = x[:nz], x[nz:]
        adz = A @ dz
        dv = (yb + g0 * adz) / mu if adjoint else rvm + gam * adz
        wz = Hs @ dz + G.T @ dl + A.T @ dv
        for k, a in (("y", y), ("rz", rz), ("rl", rl), ("dz", dz), ("dl", dl), ("dv", dv), ("adz", adz), ("wz", wz),
                     ("wl", -(G @ dz)), ("gam", gam), ("rvm", rvm), ("yb", yb)):
            res[k].append(a)
    return {k: np.stack(a) for k, a in res.items()}
