"""Shared helpers of the tests (and of the developer tools under tools/)."""
import os

import numpy as np

from tools import fixtures as fx


def dense_from_kat(k):
    nz = len(k["f"])
    G = np.asarray(k.get("G", []), dtype=np.float64).reshape(-1, nz)
    return fx.dense_problem(k["H"], k["f"], G, k.get("h", []), k["A"], k["b"])


def mpc_from_kat(k):
    g = fx.OcpGenerator()
    getattr(g, k["name"])(k["N"])
    return g.GetFBstabInput()


def mpc_component_fixture(c):
    """N=2 double integrator with the FULL E at every stage
    (mpc_component_unit_tests.h:37-93)."""
    N = c["N"]
    col = lambda v: np.asarray(v, dtype=np.float64).reshape(-1, 1)
    m = lambda v: np.atleast_2d(np.asarray(v, dtype=np.float64))
    p = fx.MpcProblem(N, 2, 1, 6)
    seq = dict(Q=[m(c["Q"])] * (N + 1), R=[m(c["R"])] * (N + 1),
               S=[m(c["S"])] * (N + 1), q=[col(c["q"])] * (N + 1),
               r=[col(c["r"])] * (N + 1), A=[m(c["A"])] * N, B=[m(c["B"])] * N,
               c=[col(c["c"])] * N, E=[m(c["E"])] * (N + 1),
               L=[m(c["L"])] * (N + 1), d=[col(c["d"])] * (N + 1))
    p.arrays = {k: fx._colmajor(v).reshape(1, -1) for k, v in seq.items()}
    p.arrays["x0"] = np.asarray(c["x0"], dtype=np.float64).reshape(1, -1)
    return p


# -- the parity bar of the GPU tests (test_gpu_parity.py, test_gpu_queue.py) ------------------
def _opts(hip, o):
    """oracle Options -> hip_api Options (same POD)."""
    h = hip.Options()
    for name, _ in h._fields_:
        setattr(h, name, getattr(o, name))
    return h


def _unique_duals(dense, vc, act_tol=1e-7):
    """Dense QPs of the batch whose multipliers are pinned by the KKT conditions: the
    gradients of the equalities and of the active inequalities (oracle's v > 0) are
    linearly independent.  Elsewhere (l, v) is any point of a face - FBstab returns the
    one its proximal path runs into, which depends on the rounding of every Newton solve
    in the directions where K's eigenvalues are of the size of sigma (cond(K) ~ 1e16):
    the one-wavefront kernel in its opt-in NATURAL / AUTO elimination orders
    (fbstab_hip_dense_set_factorisation) and the oracle, which pivots like Eigen, then
    agree in z, y and G'l + A'v but not in l and v.  (The default order is Eigen's and is
    compared entry by entry.)"""
    nz, nl, nv = dense.nz, dense.nl, dense.nv
    B = vc.shape[0]
    uniq = np.zeros(B, dtype=bool)
    for i in range(B):
        A = dense.arrays["A"][i].reshape(nz, nv).T
        rows = [A[vc[i] > act_tol]]
        if nl:
            rows.append(dense.arrays["G"][i].reshape(nz, nl).T)
        M = np.vstack(rows)
        uniq[i] = M.shape[0] == 0 or np.linalg.matrix_rank(M, tol=1e-8) == M.shape[0]
    return uniq


def _assert_parity(gpu, cpu, abs_tol, exact_frac=1.0, max_dn=0, dense=None):
    """The parity bar.  STRICT by default: exit flag, proximal and Newton count of
    EVERY instance equal to the oracle's.  Only the opt-in dense elimination orders (NATURAL / AUTO: a
    different pivot order than Eigen's, by the caller's choice) pass a looser `exact_frac` / `max_dn`."""
    zg, lg, vg, yg, og = gpu
    zc, lc, vc, yc, oc = cpu
    assert np.array_equal(og["eflag"], oc["eflag"])
    assert np.array_equal(og["prox_iters"], oc["prox_iters"])
    dn = np.abs(og["newton_iters"].astype(int) - oc["newton_iters"].astype(int))
    assert dn.max() <= max_dn, (dn.max(), np.nonzero(dn)[0][:10])
    assert (dn == 0).mean() >= exact_frac, ((dn != 0).sum(), np.nonzero(dn)[0][:10])
    if max_dn == 0:
        assert int(og["newton_iters"].sum()) == int(oc["newton_iters"].sum())
    pinned = np.ones(zc.shape[0], dtype=bool)
    if dense is not None:
        # multipliers: entry by entry where they are unique, through G'l + A'v everywhere
        pinned = _unique_duals(dense, vc)
        nz, nl, nv = dense.nz, dense.nl, dense.nv
        A = dense.arrays["A"].reshape(-1, nz, nv)   # A[b, k, i] = A_b[i][k]
        img = lambda l, v: (np.einsum("bki,bi->bk", A, v) +
                            (np.einsum("bkq,bq->bk", dense.arrays["G"].reshape(-1, nz, nl), l) if nl else 0.0))
        ig, ic = img(lg, vg), img(lc, vc)
        scale = 1.0 + np.abs(ic).max(axis=1, keepdims=True)
        assert (np.abs(ig - ic) <= 10 * abs_tol * scale).all(), np.abs(ig - ic).max()
    for g, c, sel in ((zg, zc, None), (lg, lc, pinned), (vg, vc, pinned), (yg, yc, None)):
        if c.size:
            scale = 1.0 + np.abs(c).max(axis=1, keepdims=True)
            close = np.abs(g - c) <= 10 * abs_tol * scale
            if sel is not None:
                close = close[sel]
            assert close.all(), np.abs(g - c).max()
    ok = oc["eflag"] == 0
    np.testing.assert_allclose(og["initial_residual"], oc["initial_residual"], rtol=1e-10)
    # residuals agree where they are well above the rounding floor of a
    # cancellation-dominated quantity (terms are O(1..100), eps*100 ~ 1e-14,
    # amplified by the Newton step's conditioning, cond(K) up to 1e11: a few 1e-8)
    big = ok & (oc["residual"] > 1e-7)
    # (a different elimination order - `dense` - rounds the last step differently:
    # a tenth of the tolerance the solve stops at)
    if big.any():
        np.testing.assert_allclose(og["residual"][big], oc["residual"][big], rtol=2e-2,
                                   atol=3e-8 if dense is None else max(3e-8, 0.1 * abs_tol))


# Variant builds of the product sources the tests load beside the product library (`with
# hip_api.library(VARIANT_LIBS[name])`); built by `make -C fbstab_amd/csrc <name>` into tests/_build/:
#   "pattern"  every automatic variable initialised to a bit pattern (-ftrivial-auto-var-init=pattern)
#              and the guard s_nop of every fused broadcast-FMA kept: a read of a value the code never
#              set gives the same garbage in every build instead of whatever the optimiser made of it
VARIANT_LIBS = {"pattern": os.path.join(os.path.dirname(os.path.abspath(__file__)), "_build", "libfbstab_hip_pattern.so")}


def mpc_explicit(p, b=0):
    """Explicit (H, f, G, h, A, b) of QP ``b`` of an MpcProblem, built from the
    definitions in fbstab_mpc.h:22-49 / mpc_data.cc (G=[-I; A B -I; ...],
    h=-(x0,c), b=-d)."""
    N, nx, nu, nc = p.sizes()
    ns = nx + nu
    a = {k: v[b] for k, v in p.arrays.items()}
    mat = lambda key, k, r, c: a[key][k * r * c:(k + 1) * r * c].reshape(c, r).T
    H = np.zeros((p.nz, p.nz))
    A = np.zeros((p.nv, p.nz))
    G = np.zeros((p.nl, p.nz))
    f = np.zeros(p.nz)
    h = np.zeros(p.nl)
    bb = np.zeros(p.nv)
    for i in range(N + 1):
        o = i * ns
        H[o:o + nx, o:o + nx] = mat("Q", i, nx, nx)
        H[o + nx:o + ns, o:o + nx] = mat("S", i, nu, nx)
        H[o:o + nx, o + nx:o + ns] = mat("S", i, nu, nx).T
        H[o + nx:o + ns, o + nx:o + ns] = mat("R", i, nu, nu)
        f[o:o + nx] = a["q"][i * nx:(i + 1) * nx]
        f[o + nx:o + ns] = a["r"][i * nu:(i + 1) * nu]
        A[i * nc:(i + 1) * nc, o:o + nx] = mat("E", i, nc, nx)
        A[i * nc:(i + 1) * nc, o + nx:o + ns] = mat("L", i, nc, nu)
        bb[i * nc:(i + 1) * nc] = -a["d"][i * nc:(i + 1) * nc]
        G[i * nx:(i + 1) * nx, o:o + nx] = -np.eye(nx)
        if i == 0:
            h[:nx] = -a["x0"]
        else:
            G[i * nx:(i + 1) * nx, o - ns:o - ns + nx] = mat("A", i - 1, nx, nx)
            G[i * nx:(i + 1) * nx, o - ns + nx:o] = mat("B", i - 1, nx, nu)
            h[i * nx:(i + 1) * nx] = -a["c"][(i - 1) * nx:i * nx]
    return H, f, G, h, A, bb


def newton_system_residual(p, q, step, x=None, xbar=None, sigma=1e-8, alpha=0.95, explicit=None):
    """|V dx - r| of the Newton system V(x, xbar, sigma) dx = -R(x, xbar, sigma) (abstract_components.h:276-288,
    full_residual.cc:49-74) for QP ``q`` of the MpcProblem ``p`` at x = (z, l, v) (default: zeros), evaluated in
    numpy longdouble (64-bit mantissa).  step: dict with dz, dl, dv.  Returns ([max |.| of the z, l, v block
    rows], 2-norm over all rows).  ``explicit``: the QP's (H, f, G, h, A, b) where ``p`` is not an MpcProblem
    (``dense_explicit(p, q)`` for a dense one)."""
    LD = np.longdouble
    Hm, f, G, hh, A, b = (m.astype(LD) for m in (explicit if explicit is not None else mpc_explicit(p, q)))
    zero = lambda n: np.zeros(n, LD)
    z, l, v = (t.astype(LD) for t in x) if x is not None else (zero(p.nz), zero(p.nl), zero(p.nv))
    zb, lb, vb = (t.astype(LD) for t in xbar) if xbar is not None else (z, l, v)
    sig, al = LD(sigma), LD(alpha)
    ys = (b - A @ z) + sig * (v - vb)
    rr = np.sqrt(ys * ys + v * v)
    c0 = al * (1 - 1 / np.sqrt(LD(2)))
    safe = np.where(rr > 0, rr, 1)
    gam = np.where(rr < 1e-13, c0, al * (1 - ys / safe))
    mu = np.where(rr < 1e-13, c0, al * (1 - v / safe))
    pos = (rr >= 1e-13) & (ys > 0) & (v > 0)
    gam = np.where(pos, gam + (1 - al) * v, gam)
    mu = np.where(pos, mu + (1 - al) * ys, mu)
    mus = mu + sig * gam
    phi = al * (ys + v - rr) + (1 - al) * np.maximum(ys, 0) * np.maximum(v, 0)
    rz = -(Hm @ z + f + G.T @ l + A.T @ v + sig * (z - zb))
    rl = -(hh - G @ z + sig * (l - lb))
    dz, dl, dv = (np.asarray(step[k]).astype(LD) for k in ("dz", "dl", "dv"))
    e1 = Hm @ dz + sig * dz + G.T @ dl + A.T @ dv - rz
    e2 = -G @ dz + sig * dl - rl
    e3 = -gam * (A @ dz) + mus * dv + phi
    blocks = [float(np.abs(e).max()) if e.size else 0.0 for e in (e1, e2, e3)]  # (a dense QP may have no l rows)
    return blocks, float(np.sqrt((e1 * e1).sum() + (e2 * e2).sum() + (e3 * e3).sum()))


def fuzz_stream_shape(seed, index, family="random"):
    """Shape number ``index`` (from 0) of tools/fuzz_shapes.py's stream for ``seed``: (problem, options).
    ``family``: "random" (the default stream), "bounds" or "sparse" (the tool's options of those names)."""
    from oracle.oracle_py import default_options
    gen = {"random": fx.random_ltv_mpc, "bounds": fx.random_ltv_mpc_bounds, "sparse": fx.random_ltv_mpc_sparse_rows}[family]
    rng = np.random.default_rng(seed)
    for it in range(index + 1):
        nx = int(rng.integers(1, 27)); nu = int(rng.integers(1, 10)); nc = int(rng.integers(1, 34)); N = int(rng.integers(1, 13))
        B = int(rng.integers(1, 14))
        o = default_options()
        if rng.random() < 0.3:
            o = default_options(max_linesearch_iters=int(rng.integers(1, 12)), nonmonotone_linesearch=int(rng.random() < 0.5))
        p = gen(rng, B, N, nx, nu, nc)
    return p, o


def dense_explicit(p, b=0):
    a = {k: v[b] for k, v in p.arrays.items()}
    H = a["H"].reshape(p.nz, p.nz).T
    G = a["G"].reshape(p.nz, p.nl).T
    A = a["A"].reshape(p.nz, p.nv).T
    return H, a["f"], G, a["h"], A, a["b"]


def natural_residual_norm(H, f, G, h, A, b, z, l, v):
    """||(Hz+f+G'l+A'v, h-Gz, min(b-Az, v))||, the KKT measure the reference's
    tests use (fbstab_dense_unit_tests.cc:172-176)."""
    rz = H @ z + f + G.T @ l + A.T @ v
    rl = h - G @ z
    rv = np.minimum(b - A @ z, v)
    return np.sqrt(rz @ rz + rl @ rl + rv @ rv)


# -- the reference's per-iteration display (fbstab_algorithm-impl.h:411-541) ----
EXIT_MESSAGES = {0: " Success\n", 1: " Divergence\n", 2: " Iteration limit exceeded\n",
                 3: " Primal Infeasibility\n", 4: " Dual Infeasibility\n",
                 5: " Primal-Dual Infeasibility\n"}


def format_display(records, level, out, opts):
    """Text of display level ``level`` (2 = ITER, 3 = ITER_DETAILED) from trace
    records ``(n, 8)`` = kind, i0, i1, v0..v4 (fbstab_trace_record_t) and the
    SolverOut record ``out``; the wall time is written as ``<t>``."""
    s = ""
    if level == 2:
        s += "%12s  %12s  %12s  %12s  %12s  %12s  %12s\n" % (
            "prox iter", "newton iters", "|rz|", "|rl|", "|rv|", "Inner res", "Inner tol")
    for r in records:
        kind, i0, i1, v = int(r[0]), int(r[1]), int(r[2]), r[3:]
        if kind == 1 and level == 2:
            s += "%12d  %12d  %12.4e  %12.4e  %12.4e  %12.4e  %12.4e\n" % (i0, i1, *v[:5])
        elif kind == 2 and level == 3:
            s += "Begin Prox Iter: %d, Total Newton Iters: %d, Residual: %6.4e\n" % (i0, i1, v[0])
            s += "%10s  %10s  %10s  %10s  %10s\n" % ("Iter", "Step Size", "|rz|", "|rl|", "|rv|")
        elif kind == 3 and level == 3:
            s += "%10d  %10e  %10e  %10e  %10e\n" % (i0, *v[:4])
        elif kind == 4 and level == 3:
            s += "Exiting inner loop. Inner residual: %6.4e, Inner tolerance: %6.4e\n" % (v[0], v[1])
        elif kind == 5:
            s += "\nOptimization completed!  Exit code:" + EXIT_MESSAGES[int(out["eflag"])]
            s += "Time elapsed: <t> ms (-1.0 indicates timing disabled)\n"
            s += "Proximal iterations: %d out of %d\n" % (out["prox_iters"], opts.max_prox_iters)
            s += "Newton iterations: %d out of %d\n" % (out["newton_iters"], opts.max_newton_iters)
            s += "%10s  %10s  %10s  %10s\n" % ("|rz|", "|rl|", "|rv|", "Tolerance")
            s += "%10.4e  %10.4e  %10.4e  %10.4e\n\n" % tuple(v[:4])
    return s


def normalise_time(text):
    import re
    return re.sub(r"Time elapsed: \S+ ms", "Time elapsed: <t> ms", text)


def display_texts_agree(a, b, rtol=5e-4, atol=1e-7):
    """Token-wise comparison of two display texts: words must be equal, numbers
    agree to ``atol + rtol*|b|`` (the display prints 5 significant digits; atol
    is 1e-7 of the largest residual of the solve), and numbers below 1e4*atol -
    residuals left behind by a converged Newton iteration, which squares the
    rounding differences of the step before - within a factor of two."""
    import re
    ta, tb = re.split(r"[\s,]+", a.strip()), re.split(r"[\s,]+", b.strip())
    if len(ta) != len(tb):
        return False, "token count %d vs %d" % (len(ta), len(tb))
    for x, y in zip(ta, tb):
        try:
            fx_, fy = float(x), float(y)
        except ValueError:
            if x != y:
                return False, "%r vs %r" % (x, y)
            continue
        err = abs(fx_ - fy)
        if err > atol + rtol * abs(fy) and not (abs(fy) < 1e4 * atol and err <= 0.5 * max(abs(fx_), abs(fy))):
            return False, "%r vs %r" % (x, y)
    return True, ""


LOOP_FIELDS = ("eflag", "newton_iters", "prox_iters", "residual", "initial_residual")


def reference_loop_cases(kats):
    """The problems the restated loop is pinned on against the reference's own FBstabAlgorithm<> loop:
    (kind, problem, options).  tests/golden/reference_loop.npz holds what the reference loop returned for
    them (tests/golden/make_loop_golden.py)."""
    from oracle.oracle_py import default_options, reliable_options
    cases = []
    for k in kats["dense_end_to_end"]:
        cases.append(("dense", dense_from_kat(k), default_options(abs_tol=1e-8)))
    for k in kats["mpc_end_to_end"][:4]:
        cases.append(("mpc", mpc_from_kat(k), default_options(abs_tol=1e-8)))
    cases.append(("mpc", fx.synthetic_mpc_batch(6), default_options()))
    cases.append(("mpc", fx.synthetic_mpc_batch(3, first_id=11), reliable_options(display_level=0)))
    cases.append(("dense", fx.synthetic_dense_batch(6, 20, 5, 40), default_options()))
    cases.append(("dense", fx.synthetic_dense_batch(3, 50, 10, 100), default_options(max_newton_iters=7)))
    return cases


def solve_case(orc, kind, p, opts):
    """(z, l, v, y, out) of `orc` on one of reference_loop_cases."""
    return orc.solve_dense(p, opts=opts) if kind == "dense" else orc.solve_mpc(p, opts=opts)


# Every bad-argument call of fbstab_hip_<kind>_adjoint_batch / _solve_batch that a machine without a GPU can make:
# no handle exists there, so the handle is NULL in all of them - alone ("valid": everything else in order) and
# together with each other fault.  `null`: argument blocks passed as NULL; `zero`: blocks whose strides are 0.
HANDLE_FREE_CASES = {
    "valid": dict(),
    "valid_batch2": dict(batch=2),
    "null_data": dict(null=("data",)),
    "null_x": dict(null=("x",)),
    "null_seed": dict(null=("seed",)),
    "null_grad": dict(null=("grad",)),
    "null_out": dict(null=("out",)),
    "null_all": dict(null=("data", "x", "seed", "grad", "out")),
    "null_seed_z": dict(seed_z=False),
    "null_seed_z_batch2": dict(batch=2, seed_z=False),
    "zero_data_stride": dict(batch=2, zero=("data",)),
    "zero_x_stride": dict(batch=2, zero=("x",)),
    "zero_seed_stride": dict(batch=2, zero=("seed",)),
    "zero_grad_stride": dict(batch=2, zero=("grad",)),
    "zero_adj_stride": dict(batch=2, zero=("adj",)),
    "zero_strides": dict(batch=2, zero=("data", "x", "seed", "grad", "adj")),
    "zero_strides_batch1": dict(batch=1, zero=("data", "x", "seed", "grad", "adj")),
}
_ADJOINT_ONLY = ("seed", "grad", "adj")


def handle_free_cases(entry):
    """Names of the HANDLE_FREE_CASES that apply to ``entry`` ("adjoint_batch" or "solve_batch": no seeds,
    gradients or adjoints there)."""
    if entry == "adjoint_batch":
        return list(HANDLE_FREE_CASES)
    return [k for k in HANDLE_FREE_CASES if not any(t in k for t in _ADJOINT_ONLY)]


def handle_free_call(lib, kind, entry, batch=1, null=(), zero=(), seed_z=True):
    """``(rc, message)`` of fbstab_hip_<kind>_<entry> with a NULL handle and otherwise valid host arguments (every
    slot of every block a buffer with stride 8, an ``adj`` block included) except as the case says."""
    import ctypes as C
    from fbstab_amd import hip_api
    buf = np.zeros(64)
    out = np.zeros(2 * 40, dtype=np.uint8)   # two SolverOut records, or two status words
    data_t, grad_t = ((hip_api._MpcBatch, hip_api._MpcGradBatch) if kind == "mpc"
                      else (hip_api._DenseBatch, hip_api._DenseGradBatch))

    def block(cls, name, slots):
        b = cls()
        for i in range(slots):
            b.base[i], b.stride[i] = buf.ctypes.data, (0 if name in zero else 8)
        return b

    n = len(data_t().base)
    blocks = dict(data=block(data_t, "data", n), x=block(hip_api._VarBatch, "x", 4),
                  seed=block(hip_api._VarBatch, "seed", 3), grad=block(grad_t, "grad", n),
                  adj=block(hip_api._VarBatch, "adj", 3))
    if not seed_z:
        blocks["seed"].base[0] = None
    ref = lambda name: None if name in null else C.byref(blocks[name])
    outp = None if "out" in null else out.ctypes.data
    fn = getattr(lib, f"fbstab_hip_{kind}_{entry}")
    if entry == "adjoint_batch":
        rc = fn(None, batch, ref("data"), ref("x"), ref("seed"), 0.0, ref("grad"), ref("adj"), outp, 0, None)
    else:
        rc = fn(None, batch, ref("data"), ref("x"), outp, 0, None)
    return rc, lib.fbstab_hip_last_error().decode()


# -- what more than one GPU test module (and tools/) uses -------------------------------------------------------
OUT_FIELDS = ("eflag", "residual", "initial_residual", "newton_iters", "prox_iters")


def is_mpc(p):
    return hasattr(p, "N")


def cold_solve(hip, p, o=None):
    """``p`` solved on the device from a zero guess with host arrays: (solver handle, (z, l, v), out)."""
    s = hip.FBstabMpcBatch(*p.sizes(), max_batch=p.batch) if is_mpc(p) else hip.FBstabDenseBatch(p.nz, p.nl, p.nv, max_batch=p.batch)
    if o is not None:
        s.UpdateOptions(_opts(hip, o))
    z, l, v, y = (np.zeros((p.batch, n)) for n in (p.nz, p.nl, p.nv, p.nv))
    out = s.Solve({k: np.ascontiguousarray(a) for k, a in p.arrays.items()}, z, l, v, y)
    return s, (z, l, v), out


def solve_dense_host(hip, p, opts, guess=None, order=None):
    s = hip.FBstabDenseBatch(p.nz, p.nl, p.nv, max_batch=p.batch)
    if order is not None:  # fbstab_hip_dense_set_factorisation (default: the reference's order)
        s.SetFactorisation({"pivoted": s.ORDER_PIVOTED, "auto": s.ORDER_AUTO, "natural": s.ORDER_NATURAL}[order])
    s.UpdateOptions(_opts(hip, opts))
    B = p.batch
    z = np.zeros((B, p.nz)); l = np.zeros((B, p.nl)); v = np.zeros((B, p.nv)); y = np.full((B, p.nv), 7.0)
    if guess is not None:
        z[:], l[:], v[:] = guess
    data = {k: np.ascontiguousarray(a) for k, a in p.arrays.items()}
    out = s.Solve(data, z, l, v, y)
    s.close()
    return z, l, v, y, out


def lqr_gain(p):
    """-K_0 of the finite-horizon Riccati recursion of QP 0 (stage cost 1/2 [x;u]'[Q S';S R][x;u], the
    terminal stage's input eliminated)."""
    N, nx, nu, nc = p.sizes()
    a = {k: v[0] for k, v in p.arrays.items()}
    mat = lambda key, i, r, c: a[key][i * r * c:(i + 1) * r * c].reshape(c, r).T
    Q, R, S = (lambda i: mat("Q", i, nx, nx)), (lambda i: mat("R", i, nu, nu)), (lambda i: mat("S", i, nu, nx))
    P = Q(N) - S(N).T @ np.linalg.solve(R(N), S(N))
    K = None
    for i in range(N - 1, -1, -1):
        A, B = mat("A", i, nx, nx), mat("B", i, nx, nu)
        Quu, Qux, Qxx = R(i) + B.T @ P @ B, S(i) + B.T @ P @ A, Q(i) + A.T @ P @ A
        K = np.linalg.solve(Quu, Qux)
        P = Qxx - Qux.T @ K
    return -K


def pfb_gradient(ys, v, alpha, sigma):
    """(gamma, mus) of riccati_linear_solver.cc:346-365 / :91-99, in numpy."""
    r = np.sqrt(ys * ys + v * v)
    d = alpha * (1.0 - 1.0 / np.sqrt(2.0))
    with np.errstate(divide="ignore", invalid="ignore"):
        g = np.where(r < 1e-13, d, alpha * (1.0 - ys / r))
        m = np.where(r < 1e-13, d, alpha * (1.0 - v / r))
    both = (r >= 1e-13) & (ys > 0) & (v > 0)
    g = g + np.where(both, (1.0 - alpha) * v, 0.0)
    m = m + np.where(both, (1.0 - alpha) * ys, 0.0)
    return g, m + sigma * g


def pfb(a, b, alpha):
    return alpha * (a + b - np.sqrt(a * a + b * b)) + (1.0 - alpha) * np.maximum(a, 0) * np.maximum(b, 0)


def records_agree(dev, ref, what):
    assert len(dev) == len(ref), (what, len(dev), len(ref))
    assert np.array_equal(dev[:, :3], ref[:, :3]), what  # kinds, iteration numbers
    # FP tolerance: the device evaluates the same formulas in a different order
    # (DESIGN.md 3): 1e-6 relative, 1e-7 of the largest residual of the solve
    # absolute (the linear blocks of the inner residual are rounding noise of
    # that size after every Newton step).  Residuals below 1e-3 of that scale
    # are what a converged Newton iteration leaves behind - quadratic convergence
    # squares the rounding difference of the step before - and only have to
    # agree within a factor of two.
    d, r = dev[:, 3:], ref[:, 3:]
    scale = records_scale(ref)
    err = np.abs(d - r)
    tight = err <= 1e-7 * scale + 1e-6 * np.abs(r)
    loose = (np.abs(r) < 1e-3 * scale) & (err <= 0.5 * np.maximum(np.abs(d), np.abs(r)))
    bad = ~(tight | loose).all(axis=1)
    assert not bad.any(), (what, dev[bad], ref[bad])


def records_scale(rec):
    return max(1.0, float(np.abs(rec[:, 3:]).max()))
