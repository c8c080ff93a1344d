"""GPU tests of the persistent grid's work queue: every solve kernel pulls QP indices from a device counter, so
one QP must give the same bits whichever row, wavefront or workgroup solves it, whatever QPs share its wavefront,
and whether it is its slot's first QP or its fifth.

A handle made for a batch of B <= 256 QPs runs SPREAD: one QP per wavefront (record kernels: row 0 only,
fb_record_kernel.h R16Queue::fetch) or per workgroup (flat-vector and dense kernels).  The test knob
FBSTAB_HIP_MAX_WORKGROUPS caps the grid of a handle at creation, so that a few dozen QPs PACK every row of a
wavefront (four 16-lane rows on the r16 instances, two 32-lane rows on r32) and make every slot re-fetch -
its scratch slot, its LDS region and, on the dense kernels, the workgroup's factorisation scratch reused for the
next QP.  Each test asserts the geometry it relies on (kernel, capped grid, batch >= 4 x slots); the outputs are
compared with the oracle at the strict bar and BITWISE with the spread solve of the same QPs (DESIGN.md
section 4.1: every cooperative pass runs on all rows whatever they hold)."""
import numpy as np
import pytest

from tools import fixtures as fx
from oracle.oracle_py import default_options
from tests.helpers import _opts, _assert_parity, OUT_FIELDS
from tests.shapes import MPC_SHAPES, DEGENERATE_SHAPES, fuzz_dense_instances

pytestmark = pytest.mark.gpu

CAP = "FBSTAB_HIP_MAX_WORKGROUPS"
HEADLINE = "fbstab_mpc_r16_kernel<12,4,20>"
FLAT = "fbstab_mpc_kernel<64>"


@pytest.fixture(scope="module")
def hip():
    from fbstab_amd import hip_api
    assert hip_api.load_library().fbstab_hip_device_count() >= 1
    return hip_api


def _rows(kernel):
    """QPs one workgroup holds at a time: 4 rows (r16), 2 rows (r32), 1 (flat-vector and dense kernels)."""
    return 4 if "r16" in kernel else 2 if "r32" in kernel else 1


def _concat(ps):
    q = type(ps[0])(*ps[0].sizes()) if isinstance(ps[0], fx.MpcProblem) else type(ps[0])(ps[0].nz, ps[0].nl, ps[0].nv)
    q.arrays = {k: np.ascontiguousarray(np.concatenate([p.arrays[k] for p in ps])) for k in ps[0].arrays}
    return q


def _take(p, idx):
    q = _concat([p])
    q.arrays = {k: np.ascontiguousarray(a[idx]) for k, a in p.arrays.items()}
    return q


def _solve(hip, monkeypatch, p, o, cap=None, guess=None, order=None, reserved=0):
    """One host-pointer batch on a fresh handle; ``cap``: FBSTAB_HIP_MAX_WORKGROUPS at its creation (None: unset).
    Returns dict(x=(z, l, v, y, out), kernel, workgroups, refined, pivoted)."""
    if cap is None:
        monkeypatch.delenv(CAP, raising=False)
    else:
        monkeypatch.setenv(CAP, str(cap))
    B = p.batch
    mpc = isinstance(p, fx.MpcProblem)
    s = hip.FBstabMpcBatch(*p.sizes(), max_batch=B) if mpc else hip.FBstabDenseBatch(p.nz, p.nl, p.nv, max_batch=B)
    monkeypatch.delenv(CAP, raising=False)
    if order is not None:
        s.SetFactorisation(order)
    h = _opts(hip, o)
    h.reserved = reserved
    s.UpdateOptions(h)
    z = np.zeros((B, p.nz)); l = np.zeros((B, p.nl)); v = np.zeros((B, p.nv)); y = np.zeros((B, p.nv))
    if guess is not None:
        z[:], l[:], v[:] = guess
    out = s.Solve({k: np.ascontiguousarray(a) for k, a in p.arrays.items()}, z, l, v, y)
    q = s.query()
    r = dict(x=(z, l, v, y, out), kernel=s.kernel_name() if mpc else "dense%d" % q["threads"],
             workgroups=q["workgroups"],
             refined=s.refined_steps() if mpc else None, pivoted=None if mpc else s.Factorisation()["pivoted_steps"])
    s.close()
    return r


def _assert_packed(r, kernel, B, cap):
    """The regime reached: the intended kernel, the capped grid, at least four QPs per slot."""
    assert r["kernel"] == kernel, (r["kernel"], kernel)
    assert r["workgroups"] == cap, r["workgroups"]
    assert B >= 4 * cap * _rows(kernel), (B, cap, kernel)


def _assert_spread(r, kernel, B):
    """Uncapped handle made for B <= 256 QPs: one QP per wavefront (record kernels) or workgroup."""
    assert r["kernel"] == kernel, (r["kernel"], kernel)
    assert r["workgroups"] == B, (r["workgroups"], B)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _assert_same_bits(a, b, what=""):
    """z, l, v, y and the out fields of two solves bitwise equal (NaN payloads and signed zeros included)."""
    for name, x, y_ in zip("zlvy", a[:4], b[:4]):
        assert np.array_equal(_bits(x), _bits(y_)), (what, name, np.nonzero((_bits(x) != _bits(y_)).any(axis=1))[0])
    for f in OUT_FIELDS:
        assert np.array_equal(_bits(a[4][f]), _bits(b[4][f])), (what, f, a[4][f], b[4][f])


def _pick(x, idx):
    return tuple(t[idx] for t in x)


def _mixed_mpc(shape, seed, per_family, dyn_noise=0.15):
    """random_ltv_mpc, _bounds and _sparse_rows QPs of one shape in one batch, interleaved."""
    rng = np.random.default_rng(seed)
    ps = [g(rng, per_family, *shape, dyn_noise=dyn_noise)
          for g in (fx.random_ltv_mpc, fx.random_ltv_mpc_bounds, fx.random_ltv_mpc_sparse_rows)]
    p = _concat(ps)
    order = np.arange(p.batch).reshape(3, per_family).T.reshape(-1)
    return _take(p, order)


# ---- packed parity on every kernel ----------------------------------------------------------------------------
_PACKED_MPC = [(i, None) for i in (0, 1, 4, 5, 8, 9, 12, 13, 16, 17)] + [("flat", (3, 10, 9, 12)), ("flat", (10, 80, 10, 40))]


@pytest.mark.parametrize("case", _PACKED_MPC, ids=lambda c: ("%s-%s" % (MPC_SHAPES[c[0]][1], "exact" if c[0] % 4 == 0 else "padded")
                                                              if c[1] is None else "flat-%s" % "x".join(map(str, c[1]))))
def test_packed_rows_match_the_spread_solve_and_the_oracle_on_every_mpc_kernel(hip, oracle, monkeypatch, case):
    """Two workgroups solve a batch of the three random families (dense, bound and sparse constraint rows): every
    row of every wavefront busy, every slot on its fourth QP or later.  Strict parity with the oracle; outputs
    bitwise equal to the spread solve and to the packed solve of the same batch in reverse order (other
    neighbours, another place in the slot's sequence).  The flat-vector kernel on an LDS shape and on the stage
    of test_mpc_stage_wider_than_the_lds (its matrices in the workgroup's global scratch)."""
    idx, shape = case
    if shape is None:
        shape, kern = MPC_SHAPES[idx]
        monkeypatch.setenv("FBSTAB_HIP_GENERIC", "0")
        seed = 12000 + idx
    else:
        kern = FLAT
        monkeypatch.setenv("FBSTAB_HIP_GENERIC", "1")
        seed = 12100 + shape[1]
    cap = 2
    per_family = {4: 11, 2: 6, 1: 3}[_rows(kern)]
    wide = shape[1] > 64
    p = _mixed_mpc(shape, seed, per_family, dyn_noise=0.02 if wide else 0.15)
    B = p.batch
    o = default_options()
    packed = _solve(hip, monkeypatch, p, o, cap=cap)
    _assert_packed(packed, kern, B, cap)
    spread = _solve(hip, monkeypatch, p, o)
    _assert_spread(spread, kern, B)
    rev = np.arange(B)[::-1].copy()
    back = _solve(hip, monkeypatch, _take(p, rev), o, cap=cap)
    _assert_packed(back, kern, B, cap)
    cpu = oracle.solve_mpc(p, opts=o, nthreads=oracle.num_threads())
    _assert_parity(packed["x"], cpu, o.abs_tol)
    _assert_same_bits(packed["x"], spread["x"], "spread")
    _assert_same_bits(_pick(back["x"], rev), packed["x"], "reversed")


def _degenerate_mix():
    """The first instance of the degenerate dense family (seed 11) beside synthetic QPs of its shape."""
    nz, nl, nv, B, first_id = fuzz_dense_instances(11, {DEGENERATE_SHAPES[11][0]})[0]
    deg = fx.synthetic_dense_batch(B, nz, nl, nv, first_id=first_id)
    syn = fx.synthetic_dense_batch(max(12 - B, 4), nz, nl, nv, first_id=41000)
    return _concat([syn, deg])


_PACKED_DENSE = [("wave", "default"), ("wave", "auto"), ("wave", "natural"), ("256", (50, 10, 100)), ("256", (150, 20, 220))]


@pytest.mark.parametrize("case", _PACKED_DENSE, ids=lambda c: "dense%s-%s" % (64 if c[0] == "wave" else 256,
                                                                             c[1] if c[0] == "wave" else "x".join(map(str, c[1]))))
def test_packed_workgroups_match_the_spread_solve_and_the_oracle_on_every_dense_kernel(hip, oracle, monkeypatch, case):
    """Two workgroups of a dense kernel solve every QP of the batch in turn, each reusing its workgroup's
    factorisation scratch (Lg/Hd/Gt and the went_pivoted flag of fb_dense_wave.h; K and the vectors of the
    KGLOBAL instance).  The one-wavefront kernel in its three elimination orders on synthetic QPs plus an
    instance of the degenerate family; the 256-thread kernel with K in LDS and in global memory.  Oracle bar:
    strict in the default order; the opt-in orders keep the bar of test_degenerate_dense_shapes_in_the_default_order
    (flag and z).  Bitwise equal to the spread solve and to the reversed packed solve, pivoted_steps too."""
    kind, arg = case
    cap = 2
    o = default_options()
    order = None
    if kind == "wave":
        monkeypatch.setenv("FBSTAB_HIP_DENSE_THREADS", "0")
        p = _degenerate_mix()
        D = hip.FBstabDenseBatch
        order = {"default": None, "auto": D.ORDER_AUTO, "natural": D.ORDER_NATURAL}[arg]
        kern = "dense64"
    else:
        monkeypatch.setenv("FBSTAB_HIP_DENSE_THREADS", "256")
        p = fx.synthetic_dense_batch(8, *arg, first_id=42000 + arg[0])
        kern = "dense256"
    B = p.batch
    packed = _solve(hip, monkeypatch, p, o, cap=cap, order=order)
    _assert_packed(packed, kern, B, cap)
    spread = _solve(hip, monkeypatch, p, o, order=order)
    _assert_spread(spread, kern, B)
    rev = np.arange(B)[::-1].copy()
    back = _solve(hip, monkeypatch, _take(p, rev), o, cap=cap, order=order)
    _assert_packed(back, kern, B, cap)
    cpu = oracle.solve_dense(p, opts=o, nthreads=oracle.num_threads())
    if order is None:
        _assert_parity(packed["x"], cpu, o.abs_tol, dense=p if kind == "wave" else None)
    else:
        zg, zc = packed["x"][0], cpu[0]
        assert np.array_equal(packed["x"][4]["eflag"], cpu[4]["eflag"])
        assert (np.abs(zg - zc) <= 10 * o.abs_tol * (1.0 + np.abs(zc).max(axis=1, keepdims=True))).all()
    _assert_same_bits(packed["x"], spread["x"], "spread")
    _assert_same_bits(_pick(back["x"], rev), packed["x"], "reversed")
    assert packed["pivoted"] == spread["pivoted"] == back["pivoted"], (packed["pivoted"], spread["pivoted"], back["pivoted"])


# ---- neighbour isolation in a shared wavefront --------------------------------------------------------------
_ISOLATION_MPC = [("headline", HEADLINE), ("r32", "fbstab_mpc_r32_kernel<18,5,10>"), ("flat", FLAT)]


def _isolation_batch(which):
    if which == "r32":
        return fx.random_ltv_mpc(np.random.default_rng(12300), 16, 7, 18, 5, 10)
    return fx.synthetic_mpc_batch(16, first_id=4242)


@pytest.mark.parametrize("which,kern", _ISOLATION_MPC, ids=[c[0] for c in _ISOLATION_MPC])
def test_failed_and_infeasible_qps_leave_their_wavefront_neighbours_alone(hip, oracle, monkeypatch, which, kern):
    """The batch of test_mpc_mixed_outcome_batch, sixteen QPs on ONE workgroup: two whose factorisation fails
    (negative stage costs) and two with contradictory constraint rows (primal infeasible: iterates run away
    along the certificate's ray) share the wavefront with healthy QPs.  The failed ones report DIVERGENCE, the
    infeasible ones the oracle's flag and proximal count, and every healthy QP the bits of the spread solve of
    the healthy QPs alone and the oracle's counts."""
    monkeypatch.setenv("FBSTAB_HIP_GENERIC", "1" if kern == FLAT else "0")
    p = _isolation_batch(which)
    N, nx, nu, nc = p.sizes()
    B = p.batch
    fail, infeasible = [1, 9], [3, 12]
    a = {k: v.copy() for k, v in p.arrays.items()}
    E = a["E"].reshape(B, N + 1, nx, nc)    # column-major nc x nx blocks: [stage, column, row]
    L = a["L"].reshape(B, N + 1, nu, nc)
    d = a["d"].reshape(B, N + 1, nc)
    for q in fail:
        a["R"][q] = -5.0 * a["R"][q]
        a["Q"][q] = -5.0 * a["Q"][q]
    for q in infeasible:                    # rows 0 and 1: w'e + 1 <= 0 and -w'e + 1 <= 0
        E[q, :, :, 1] = -E[q, :, :, 0]
        L[q, :, :, 1] = -L[q, :, :, 0]
        d[q, :, 0] = d[q, :, 1] = 1.0
    p.arrays = a
    healthy = [q for q in range(B) if q not in fail + infeasible]
    keep = [q for q in range(B) if q not in fail]
    o = default_options()
    packed = _solve(hip, monkeypatch, p, o, cap=1)
    _assert_packed(packed, kern, B, 1)
    out = packed["x"][4]
    assert (out["eflag"][fail] == 1).all(), out["eflag"]
    cpu = oracle.solve_mpc(_take(p, keep), opts=o, nthreads=oracle.num_threads())
    oc = cpu[4]
    inf_in_keep = [keep.index(q) for q in infeasible]
    assert np.array_equal(out["eflag"][infeasible], oc["eflag"][inf_in_keep]) and (oc["eflag"][inf_in_keep] != 0).all()
    assert np.array_equal(out["prox_iters"][infeasible], oc["prox_iters"][inf_in_keep])
    h_in_keep = [keep.index(q) for q in healthy]
    _assert_parity(_pick(packed["x"], healthy), _pick(cpu, h_in_keep), o.abs_tol)
    alone = _solve(hip, monkeypatch, _take(p, healthy), o)
    _assert_spread(alone, kern, len(healthy))
    _assert_same_bits(_pick(packed["x"], healthy), alone["x"], "healthy")


_POISON_KINDS = [("headline", HEADLINE), ("r32", "fbstab_mpc_r32_kernel<18,5,10>"), ("flat", FLAT),
                 ("dense_wave", "dense64"), ("dense_256", "dense256")]


@pytest.mark.parametrize("which,kern", _POISON_KINDS, ids=[c[0] for c in _POISON_KINDS])
def test_poisoned_guesses_leave_their_wavefront_neighbours_alone(hip, oracle, monkeypatch, which, kern):
    """The guesses of test_overflowed_and_nan_guesses_end_where_the_reference_ends (a NaN, an infinity, +-1e200)
    on QPs that share ONE workgroup with healthy QPs: the line search, open_prox, close_subproblem and load_guess
    passes run for one owner row on all 64 lanes, where a lane mask or a 0 * NaN would leak.  The poisoned QPs
    report DIVERGENCE; every healthy QP has the bits of the spread solve of the healthy QPs alone and the
    oracle's counts."""
    if which.startswith("dense"):
        monkeypatch.setenv("FBSTAB_HIP_DENSE_THREADS", "256" if which == "dense_256" else "0")
        p = fx.synthetic_dense_batch(8, 20, 5, 40, first_id=10)
        bad = [1, 3, 4, 6]
    else:
        monkeypatch.setenv("FBSTAB_HIP_GENERIC", "1" if kern == FLAT else "0")
        p = _isolation_batch(which) if which == "r32" else fx.synthetic_mpc_batch(16, first_id=10)
        bad = [1, 4, 9, 14]
    B = p.batch
    z = np.zeros((B, p.nz)); l = np.zeros((B, p.nl)); v = np.zeros((B, p.nv))
    v[bad[0], 5] = np.nan
    v[bad[1], 7] = 1e200
    z[bad[2], 3] = np.inf
    v[bad[3], 2] = -1e200
    healthy = [q for q in range(B) if q not in bad]
    o = default_options()
    packed = _solve(hip, monkeypatch, p, o, cap=1, guess=(z, l, v))
    _assert_packed(packed, kern, B, 1)
    out = packed["x"][4]
    assert (out["eflag"][bad] == 1).all() and (out["eflag"][healthy] == 0).all(), out["eflag"]
    sub = _take(p, healthy)
    cpu = oracle.solve_mpc(sub, opts=o, nthreads=oracle.num_threads()) if isinstance(p, fx.MpcProblem) \
        else oracle.solve_dense(sub, opts=o, nthreads=oracle.num_threads())
    _assert_parity(_pick(packed["x"], healthy), cpu, o.abs_tol)
    alone = _solve(hip, monkeypatch, sub, o)
    _assert_spread(alone, kern, len(healthy))
    _assert_same_bits(_pick(packed["x"], healthy), alone["x"], "healthy")


# ---- early and late finishers, warm starts, refinement --------------------------------------------------------
_EXACT = [0, 4, 8, 12, 16]


@pytest.mark.parametrize("idx", _EXACT, ids=[MPC_SHAPES[i][1] for i in _EXACT])
def test_iteration_limits_and_warm_starts_on_packed_rows(hip, oracle, oracle_fma, monkeypatch, idx):
    """On the exact shape of each record instance, two workgroups: (1) max_newton_iters at the median count of
    the batch, so that half of each wavefront stops at the limit while its neighbours go on, (2) a second solve
    warm-started from the first one's solution with x0 moved (load_guess_coop for a packed owner).  The oracle
    rules of test_warm_start_and_iteration_limits and test_warm_started_second_solve_on_every_mpc_instance;
    every capped run bitwise equal to the uncapped one."""
    shape, kern = MPC_SHAPES[idx]
    monkeypatch.setenv("FBSTAB_HIP_GENERIC", "0")
    rng = np.random.default_rng(12500 + idx)
    cap = 2
    B = 4 * cap * _rows(kern)
    p = fx.random_ltv_mpc(rng, B, *shape)
    # (1) iteration limit
    full = oracle.solve_mpc(p, opts=default_options(), nthreads=oracle.num_threads())[4]["newton_iters"]
    o = default_options(max_newton_iters=int(np.median(full)))
    packed = _solve(hip, monkeypatch, p, o, cap=cap)
    _assert_packed(packed, kern, B, cap)
    spread = _solve(hip, monkeypatch, p, o)
    cpu = oracle.solve_mpc(p, opts=o, nthreads=oracle.num_threads())
    stopped = cpu[4]["eflag"] == 2
    assert 0 < stopped.sum() < B, cpu[4]["eflag"]
    _assert_parity(packed["x"], cpu, o.abs_tol)
    _assert_same_bits(packed["x"], spread["x"], "iteration limit")
    # (2) warm start from the first solve of the default options
    o = default_options()
    first = _solve(hip, monkeypatch, p, o, cap=cap)
    first_spread = _solve(hip, monkeypatch, p, o)
    _assert_same_bits(first["x"], first_spread["x"], "cold")
    p2 = _concat([p])
    x0 = p.arrays["x0"]
    p2.arrays["x0"] = np.ascontiguousarray(x0 * (1.0 + 0.05 * rng.standard_normal(x0.shape)) + 0.01 * rng.standard_normal(x0.shape))
    guess = tuple(t.copy() for t in first["x"][:3])
    warm = _solve(hip, monkeypatch, p2, o, cap=cap, guess=guess)
    _assert_packed(warm, kern, B, cap)
    warm_spread = _solve(hip, monkeypatch, p2, o, guess=guess)
    _assert_same_bits(warm["x"], warm_spread["x"], "warm")
    assert warm["refined"] == warm_spread["refined"] == 0
    out = warm["x"][4]
    oc = oracle.solve_mpc(p2, guess, opts=o, nthreads=oracle.num_threads())[4]
    assert np.array_equal(out["eflag"], oc["eflag"])
    assert np.array_equal(out["prox_iters"][oc["eflag"] != 0], oc["prox_iters"][oc["eflag"] != 0])
    conv = oc["eflag"] == 0
    same = (out["prox_iters"] == oc["prox_iters"]) & (out["newton_iters"] == oc["newton_iters"])
    if not same[conv].all():
        of = oracle_fma.solve_mpc(p2, guess, opts=o, nthreads=oracle_fma.num_threads())[4]
        same = same | ((out["prox_iters"] == of["prox_iters"]) & (out["newton_iters"] == of["newton_iters"]))
    assert same[conv].all(), (out[conv], oc[conv])


@pytest.mark.parametrize("case", ["wide-fuzz", "r16"])
def test_refinement_on_packed_rows(hip, oracle, monkeypatch, case):
    """The refinement option (reserved = 1) with packed rows: on the 29-wide shape of the fuzz stream's
    deviation (<24,8,16>, ten QPs on one workgroup of two rows) and on random QPs of the exact <12,4,32> shape
    (two workgroups of four rows).  Flags and counts equal to the oracle's, z within the parity tolerance;
    outputs and refined_steps() equal to the uncapped run."""
    from tests import helpers as H
    monkeypatch.setenv("FBSTAB_HIP_GENERIC", "0")
    if case == "wide-fuzz":
        p, o = H.fuzz_stream_shape(42, 127)
        kern, cap = "fbstab_mpc_r32_kernel<24,8,16>", 1
    else:
        shape, kern = MPC_SHAPES[4]
        cap = 2
        p, o = fx.random_ltv_mpc(np.random.default_rng(12600), 32, *shape), default_options()
    B = p.batch
    packed = _solve(hip, monkeypatch, p, o, cap=cap, reserved=1)
    _assert_packed(packed, kern, B, cap)
    spread = _solve(hip, monkeypatch, p, o, reserved=1)
    _assert_spread(spread, kern, B)
    _assert_same_bits(packed["x"], spread["x"], "refinement")
    assert packed["refined"] == spread["refined"] >= 0
    # (the bar of test_one_step_qp_on_a_29_wide_stage_takes_the_oracles_counts: a refined step ends nearer the
    # solution than the oracle's unrefined one, so the final residuals are not compared with the oracle's)
    z, out = packed["x"][0], packed["x"][4]
    zc, oc = oracle.solve_mpc(p, opts=o, nthreads=oracle.num_threads())[0::4]
    assert np.array_equal(out["eflag"], oc["eflag"]) and (out["eflag"] == 0).all()
    assert np.array_equal(out["prox_iters"], oc["prox_iters"]), (out["prox_iters"], oc["prox_iters"])
    assert np.array_equal(out["newton_iters"], oc["newton_iters"]), (out["newton_iters"], oc["newton_iters"])
    assert (out["residual"] <= o.abs_tol).all()
    assert (np.abs(z - zc) <= 10 * o.abs_tol * (1.0 + np.abs(zc).max(axis=1, keepdims=True))).all()


# ---- the real spread boundary, no knob ------------------------------------------------------------------------
_BOUNDARY = [((2,) + MPC_SHAPES[i][0][1:], MPC_SHAPES[i][1]) for i in _EXACT] + [((30, 12, 4, 20), HEADLINE)]


@pytest.mark.parametrize("shape,kern", _BOUNDARY, ids=["%s-N%d" % (k, s[0]) for s, k in _BOUNDARY])
def test_one_qp_past_the_grid_switches_from_spread_to_packed_with_the_same_bits(hip, oracle, monkeypatch, shape, kern):
    """The switch users cross: a handle whose grid W is its natural one (max_batch above it) solves batch W
    spread (one QP per wavefront) and batch W + 1 packed (a quarter or half as many workgroups, rows 1-3 busy)
    from the same QP list.  QPs 0..W-1 bitwise equal; the W + 1 run strict against the oracle.  On the headline
    shape also W x 4 (every slot one QP) against W x 4 + 1 (the first re-fetch)."""
    monkeypatch.setenv("FBSTAB_HIP_GENERIC", "0")
    monkeypatch.delenv(CAP, raising=False)
    head = shape[0] == 30
    s = hip.FBstabMpcBatch(*shape, max_batch=1 << 16)   # (the staging buffers follow max_batch at the first solve)
    assert s.kernel_name() == kern
    W = s.query()["workgroups"]
    s.close()
    rows = _rows(kern)
    sizes = [W, W + 1] + ([W * rows, W * rows + 1] if head else [])
    n = max(sizes)
    s = hip.FBstabMpcBatch(*shape, max_batch=n)
    assert s.query()["workgroups"] == W
    p = fx.synthetic_mpc_batch(n, first_id=60000) if head else fx.random_ltv_mpc(np.random.default_rng(12700 + shape[1]), n, *shape)
    o = default_options()
    s.UpdateOptions(_opts(hip, o))
    res = {}
    for b in sizes:
        z = np.zeros((b, p.nz)); l = np.zeros((b, p.nl)); v = np.zeros((b, p.nv)); y = np.zeros((b, p.nv))
        out = s.Solve({k: np.ascontiguousarray(a[:b]) for k, a in p.arrays.items()}, z, l, v, y)
        res[b] = (z, l, v, y, out)
    s.close()
    cpu = oracle.solve_mpc(p, opts=o, nthreads=oracle.num_threads())
    for lo, hi in zip(sizes[::2], sizes[1::2]):
        _assert_same_bits(_pick(res[hi], slice(0, lo)), res[lo], "%d vs %d" % (lo, hi))
        _assert_parity(res[hi], _pick(cpu, slice(0, hi)), o.abs_tol)


# ---- keep-flag fallback --------------------------------------------------------------------------------------
def test_keep_flag_on_a_capped_handle_runs_the_plain_path(hip, monkeypatch):
    """FBSTAB_HIP_KEEP_MATRICES solves QP q in slot q; a batch above the slots of a capped headline handle
    falls back to the plain queue (fbstab_hip.hip: keep needs batch <= workgroups x QPs per workgroup): two
    flagged calls in a row give the bits of an unflagged call."""
    import torch
    dev = torch.device("cuda:0")
    B = 32
    p = fx.synthetic_mpc_batch(B, first_id=61000)
    monkeypatch.setenv(CAP, "2")
    s = hip.FBstabMpcBatch(*p.sizes(), max_batch=B)
    monkeypatch.delenv(CAP)
    assert s.kernel_name() == HEADLINE and s.query()["workgroups"] == 2 and B >= 4 * 2 * 4
    data = {k: torch.from_numpy(np.ascontiguousarray(a)).to(dev) for k, a in p.arrays.items()}
    mk = lambda n: torch.zeros((B, n), dtype=torch.float64, device=dev)
    res = []
    for keep in (False, True, True):
        z, l, v, y = mk(p.nz), mk(p.nl), mk(p.nv), mk(p.nv)
        out = hip.out_to_numpy(s.Solve(data, z, l, v, y, keep_matrices=keep))
        res.append(tuple(t.cpu().numpy() for t in (z, l, v, y)) + (out,))
    s.close()
    assert (res[0][4]["eflag"] == 0).all()
    for r in res[1:]:
        _assert_same_bits(r, res[0], "keep")
