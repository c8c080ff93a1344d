"""Inputs, acceptance rules and a plain float64 restatement for the row-held linear algebra of
fbstab_amd/csrc/fb_row16.h.  Shared by tests/test_gpu_row_primitives.py (the device, through the probe
library) and tests/test_row_rules_cpu.py (the restatement and its seeded mutants through the SAME rules).

Storage convention of the factor, as chol_rows leaves it: rec[q, r, k] = L[r][k] for k < r, rec[q, r, r] =
1 / L[r][r]; slots k > r are not part of the result.  Every residual is evaluated in numpy.longdouble from
the doubles under test; a diagonal enters as L_jj = 1 / q formed in longdouble.

The bounds (u = 2^-53), from rounding analysis and not from any measurement:
  factor:      |A + diag_add I - L L'|_ij <= 2 (N + 8) u (|L| |L'|)_ij
               entry ij takes j fma roundings and one multiply by q; q is within 2 ulp = 4 u of the exact
               reciprocal square root, so 1 / q^2 is within 8 u of the pivot; 2 is the margin for second order.
  triangular:  |L x - b|_i <= 2 (N + 2) u (|L| |x|)_i   (inverse columns: b = e_r; right-solve: rows of
               W L' = B; substitutions): at most N - 1 fma roundings and one multiply by q per entry.
  dot:         |got - exact| <= (T + 4) u S, T products, S the sum of their magnitudes (tests/tangent_helpers).
"""
import functools

import numpy as np

from tests.tangent_helpers import U

LD = np.longdouble

PRODUCT_PAIRS = [(16, 1), (12, 1), (23, 2), (32, 2), (18, 2), (24, 2)]
EDGE_PAIRS = [(1, 1), (2, 1), (17, 2)]
PAIRS = PRODUCT_PAIRS + EDGE_PAIRS
FAMILIES = ("F1", "F2", "F3", "F4")
PER_FAMILY = 12  # QPs per family and pair


# ---- inputs --------------------------------------------------------------------------------------------
def _rng(tag, N):
    return np.random.default_rng([20240611, N] + [ord(c) for c in tag])


def _spd(rng, n, N):
    G = rng.standard_normal((n, N, N))
    return G @ G.transpose(0, 2, 1) + np.eye(N)


@functools.lru_cache(maxsize=None)
def family(name, N, n=PER_FAMILY):
    """(A [n, N, N] symmetric, diag_add [n], vmin [n, N]): vmin is the eigenvector of the smallest
    eigenvalue for F2 (a right-hand side of the triangular tests), zeros otherwise."""
    rng = _rng(name, N)
    vmin = np.zeros((n, N))
    if name == "F1":  # well conditioned
        A = _spd(rng, n, N)
        dadd = rng.choice([1e-6, 0.25], n)
    elif name == "F2":  # stage-like: Q diag(lambda) Q', lambda log-uniform in [1e-8, 1e3], sigma = 1e-8
        A = np.empty((n, N, N))
        for i in range(n):
            Q, _ = np.linalg.qr(rng.standard_normal((N, N)))
            lam = 10.0 ** rng.uniform(-8.0, 3.0, N)
            if i % 2 == 1 and N > 2:  # several eigenvalues of A + sigma I equal to sigma (nx > N nu, R6.5)
                lam[rng.permutation(N)[: max(2, N // 3)]] = 0.0
            M = (Q * lam) @ Q.T
            A[i] = 0.5 * (M + M.T)
            vmin[i] = Q[:, int(np.argmin(lam))]
        dadd = np.full(n, 1e-8)
    elif name == "F3":  # graded: D A D, D = diag(2^k), exact scaling; no diag_add (it would vanish beside 2^40)
        A0 = _spd(rng, n, N)
        D = 2.0 ** rng.integers(-20, 21, (n, N)).astype(np.float64)
        A = D[:, :, None] * A0 * D[:, None, :]
        dadd = np.zeros(n)
    elif name == "F4":  # exact shapes: identity and diagonal matrices
        A = np.zeros((n, N, N))
        for i in range(n):
            A[i] = np.eye(N) if i % 3 == 0 else np.diag(rng.uniform(0.5, 4.0, N))
        dadd = np.where(np.arange(n) % 4 == 0, 0.0, 1e-8)
        dadd[1:3] = 1e-8
    else:
        raise KeyError(name)
    for a in (A, dadd, vmin):
        a.setflags(write=False)
    return A, dadd, vmin


@functools.lru_cache(maxsize=None)
def healthy(N):
    """F1-F4 as one batch: A, diag_add, vmin, family index per QP."""
    parts = [family(f, N) for f in FAMILIES]
    fam = np.repeat(np.arange(len(FAMILIES)), PER_FAMILY)
    out = tuple(np.concatenate([p[i] for p in parts]) for i in range(3)) + (fam,)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def rhs(N):
    """Right-hand sides for healthy(N): B [n, N, N] (rows of the right-solve) and b [n, N].  QPs take turns:
    random, unit vectors, and - for F2 - the eigenvector of the smallest eigenvalue."""
    A, _, vmin, fam = healthy(N)
    n = A.shape[0]
    rng = _rng("rhs", N)
    B = rng.standard_normal((n, N, N))
    b = rng.standard_normal((n, N))
    for i in range(n):
        if i % 3 == 1:
            B[i] = np.eye(N)
            b[i] = np.eye(N)[i % N]
        elif i % 3 == 2 and FAMILIES[fam[i]] == "F2":
            B[i] = np.outer(rng.standard_normal(N), vmin[i])
            b[i] = vmin[i]
    B.setflags(write=False)
    b.setflags(write=False)
    return B, b


@functools.lru_cache(maxsize=None)
def failures(N, R):
    """F5: (A, diag_add, what) of QPs whose factorisation must report failure."""
    rng = _rng("F5", N)
    pos = sorted({0, N // 2, N - 1} | ({16} if (R == 2 and N > 16) else set()))
    As, ds, what = [], [], []
    for p in pos:
        # a pivot that turns negative at p: A_pp = |l|^2 - 1 - diag_add with l the row of the leading factor
        A = _spd(rng, 1, N)[0]
        d = 0.25
        if p > 0:
            L0 = np.linalg.cholesky(A[:p, :p] + d * np.eye(p))
            l = np.linalg.solve(L0, A[:p, p])
            A[p, p] = l @ l - 1.0 - d
        else:
            A[0, 0] = -1.0 - d
        As.append(A); ds.append(d); what.append("negative pivot at %d" % p)
        # diag_add = 0 on a singular matrix: row and column p are zero, the pivot is exactly 0
        A = _spd(rng, 1, N)[0]
        A[p, :] = 0.0
        A[:, p] = 0.0
        As.append(A); ds.append(0.0); what.append("zero pivot at %d, diag_add = 0" % p)
    A = _spd(rng, 1, N)[0]
    A[N - 1, 0] = A[0, N - 1] = np.nan  # reaches the last pivot through L[N-1][0]
    As.append(A); ds.append(1e-8); what.append("NaN entry")
    A = _spd(rng, 1, N)[0]
    A[N // 2, N // 2] = np.nan
    As.append(A); ds.append(1e-8); what.append("NaN on the diagonal")
    return np.stack(As), np.array(ds), tuple(what)


def lane_image(M, lpq, fill, seed=7):
    """[n, N, K] -> [n, lpq, K]: rows r >= N are zeros (fill = 'zero') or finite garbage with NaNs among it."""
    n, N, K = M.shape
    img = np.zeros((n, lpq, K))
    img[:, :N] = M
    if fill == "garbage" and lpq > N:
        rng = np.random.default_rng(seed)
        g = rng.standard_normal((n, lpq - N, K)) * 10.0 ** rng.integers(-30, 30, (n, lpq - N, K))
        g[rng.random(g.shape) < 0.2] = np.nan
        img[:, N:] = g
    elif fill not in ("zero", "garbage"):
        raise KeyError(fill)
    return img


# ---- rules ---------------------------------------------------------------------------------------------
def _ratio(res, bnd):
    """Worst residual-to-bound ratio per QP; a non-finite residual or a residual where the bound is zero is inf."""
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(bnd > 0, res / bnd, np.where(res == 0, LD(0), LD(np.inf)))
    q = np.where(np.isfinite(res) & np.isfinite(bnd), q, LD(np.inf))
    return q.reshape(q.shape[0], -1).max(axis=1).astype(np.float64)


def factor_ld(rec):
    """The factor a record describes, in longdouble: strict lower triangle as stored, L_jj = 1 / q."""
    rec = np.asarray(rec)
    L = np.tril(rec.astype(LD), -1)
    i = np.arange(rec.shape[-1])
    L[:, i, i] = LD(1) / rec[:, i, i].astype(LD)
    return L


def chol_ratio(A, dadd, rec):
    N = A.shape[-1]
    L = factor_ld(rec)
    M = A.astype(LD) + np.asarray(dadd, dtype=LD)[:, None, None] * np.eye(N, dtype=LD)
    res = np.abs(M - L @ L.transpose(0, 2, 1))
    bnd = LD(2 * (N + 8) * U) * (np.abs(L) @ np.abs(L).transpose(0, 2, 1))
    low = np.tril(np.ones((N, N), dtype=bool))  # the lower triangle is what the factorisation reads
    return _ratio(np.where(low, res, 0), np.where(low, bnd, 1))


def inv_ratio(rec, X):
    """X[q, r, k] = entry k of column r of inv(L), as tri_inv_cols leaves it in lane r."""
    N = rec.shape[-1]
    L = factor_ld(rec)
    Xm = np.asarray(X).astype(LD).transpose(0, 2, 1)
    res = np.abs(L @ Xm - np.eye(N, dtype=LD))
    return _ratio(res, LD(2 * (N + 2) * U) * (np.abs(L) @ np.abs(Xm)))


def right_ratio(rec, B, W):
    """W L' = B, W[q, r, c] the row r of the solution."""
    N = rec.shape[-1]
    L = factor_ld(rec)
    Wl = np.asarray(W).astype(LD)
    Lt = L.transpose(0, 2, 1)
    res = np.abs(Wl @ Lt - np.asarray(B).astype(LD))
    return _ratio(res, LD(2 * (N + 2) * U) * (np.abs(Wl) @ np.abs(Lt)))


def subst_ratio(rec, b, x, transposed=False):
    """L x = b (subst_rows) or L' x = b (subst_cols_t)."""
    N = rec.shape[-1]
    L = factor_ld(rec)
    if transposed:
        L = L.transpose(0, 2, 1)
    xl = np.asarray(x).astype(LD)[:, :, None]
    res = np.abs(L @ xl - np.asarray(b).astype(LD)[:, :, None])
    return _ratio(res, LD(2 * (N + 2) * U) * (np.abs(L) @ np.abs(xl)))


def dot_ratio(got, terms, init=None):
    """got [...] against the sum over the last axis of terms [..., T] (+ init): (T + 4) u S."""
    t = np.asarray(terms).astype(LD)
    T = t.shape[-1]
    ref = t.sum(axis=-1)
    S = np.abs(t).sum(axis=-1)
    if init is not None:
        ref = ref + np.asarray(init).astype(LD)
        S = S + np.abs(np.asarray(init).astype(LD))
    res = np.abs(np.asarray(got).astype(LD) - ref)
    return float(_ratio(res.reshape(1, -1), (LD((T + 4) * U) * S).reshape(1, -1))[0])


# ---- the restatement: float64, reciprocal diagonal, one rounding per operation, no lanes -----------
def _fma(a, b, c):
    # a * b + c with (all but) one rounding: the product and the sum carried in longdouble's 64 bits
    return (np.asarray(a).astype(LD) * np.asarray(b).astype(LD) + np.asarray(c).astype(LD)).astype(np.float64)


def _rsqrt(d):
    with np.errstate(invalid="ignore", divide="ignore"):
        return (LD(1) / np.sqrt(d.astype(LD))).astype(np.float64)


class Mutant:
    """Seeded defects of the restatement (tests/test_row_rules_cpu.py); None of them set = the restatement."""
    def __init__(self, drop_update=None, diag_twice=False, diag_skip_last=False, q_rel_err=0.0,
                 hi_lanes_from_lo=False, wrong_pivot=None):
        self.drop_update = drop_update        # (r, m, j): the update of entry (r, m) by pivot j is lost
        self.diag_twice = diag_twice
        self.diag_skip_last = diag_skip_last
        self.q_rel_err = q_rel_err
        self.hi_lanes_from_lo = hi_lanes_from_lo  # a broadcast of lane m >= 16 delivers lane m - 16's value
        self.wrong_pivot = wrong_pivot        # (r, c, c'): right-solve entry (r, c) scaled by pivot c'


def _served(v, mut):
    """What the broadcasts of the per-row values v[q, m] deliver."""
    if mut is not None and mut.hi_lanes_from_lo and v.shape[1] > 16:
        v = v.copy()
        v[:, 16:] = v[:, : v.shape[1] - 16]
    return v


def _lane(j, mut):
    return j - 16 if (mut is not None and mut.hi_lanes_from_lo and j >= 16) else j


def chol_restated(A, dadd, mut=None):
    a = np.array(A, dtype=np.float64)
    n, N, _ = a.shape
    ok = np.ones(n, dtype=bool)
    for j in range(N):
        add = np.array(dadd, dtype=np.float64)
        if mut is not None and mut.diag_twice:
            add = add + add
        if mut is not None and mut.diag_skip_last and j == N - 1:
            add = np.zeros(n)
        d = a[:, _lane(j, mut), j] + add  # the pivot is a broadcast of lane j's a[j]
        ok &= d > 0
        q = _rsqrt(d)
        if mut is not None and mut.q_rel_err:
            q = q * (1.0 + mut.q_rel_err)
        lj = a[:, :, j] * q[:, None]  # every row's, row j's own (sqrt(d)) included
        if j + 1 < N:
            src = _served(lj, mut)
            new = _fma(-lj[:, :, None], src[:, None, j + 1:], a[:, :, j + 1:])
            if mut is not None and mut.drop_update is not None and mut.drop_update[2] == j:
                r0, m0, _ = mut.drop_update
                new[:, r0, m0 - j - 1] = a[:, r0, m0]
            a[:, :, j + 1:] = new
        a[:, :, j] = lj
        a[:, j, j] = q
    return a, ok


def tri_inv_solve_restated(rec, B=None, mut=None):
    """(X, W) of tri_inv_cols_solve: X[q, r, :] column r of inv(L), W = B inv(L)'.  B = None: X alone."""
    n, N, _ = rec.shape
    x = np.broadcast_to(np.eye(N), (n, N, N)).copy()
    w = None if B is None else np.array(B, dtype=np.float64)
    for k in range(N):
        q = rec[:, _lane(k, mut), k]  # a broadcast of lane k's diagonal slot
        x[:, :, k] = x[:, :, k] * q[:, None]
        if w is not None:
            qw = np.broadcast_to(q[:, None], (n, N)).copy()
            if mut is not None and mut.wrong_pivot is not None and mut.wrong_pivot[1] == k:
                qw[:, mut.wrong_pivot[0]] = rec[:, mut.wrong_pivot[2], mut.wrong_pivot[2]]
            w[:, :, k] = w[:, :, k] * qw
        if k + 1 < N:
            col = _served(np.concatenate([np.zeros((n, k + 1)), rec[:, k + 1:, k]], axis=1), mut)[:, None, k + 1:]
            x[:, :, k + 1:] = _fma(col, -x[:, :, k, None], x[:, :, k + 1:])
            if w is not None:
                w[:, :, k + 1:] = _fma(col, -w[:, :, k, None], w[:, :, k + 1:])
    return x, w


def subst_restated(rec, b, transposed=False, mut=None):
    n, N, _ = rec.shape
    i = np.arange(N)
    dinv = rec[:, i, i]
    Ls = np.tril(rec, -1)
    acc = np.array(b, dtype=np.float64)
    order = range(N - 1, 0, -1) if transposed else range(N - 1)
    for k in order:
        xk = _served(acc * dinv, mut)[:, k]
        m = Ls[:, k, :] if transposed else Ls[:, :, k]  # L[k][r] on rows r < k / L[r][k] on rows r > k
        acc = _fma(-m, xk[:, None], acc)
    return acc * dinv
