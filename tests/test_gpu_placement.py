"""GPU tests of the C-ABI's addressing promise (include/fbstab_hip.h): QP b of every array lives at base + b *
stride, records and separate arrays both work, stride 0 shares an array - on every entry point, input and OUTPUT
blocks alike, host and device pointers.

The rule of every case: the packed call (stride = length) and the placed call (tests/placement_helpers.py: records
or spread rows with canaries in between, or one shared row) run on fresh handles with the same options; every output
slot, the SolverOut fields, ``norms`` and ``status`` are bitwise equal, and every canary is intact.  Bitwise is the
bar because a QP's arithmetic does not depend on its address.  The gaps of the INPUT blocks hold NaN, so a read past
a slot that reaches arithmetic changes bits.  Each case asserts the kernel it means to run, and per kernel family one
placed result is also held to the reference (the oracle, or the fp64 tables of the adjoint / tangent / sweep helpers)
at the bar the neighbouring tests use.

Batches: B = 7 (MPC) / 5 (dense) on ONE workgroup (FBSTAB_HIP_MAX_WORKGROUPS=1: rows and workgroups re-fetch, the last
round of a wavefront partly empty), B = 1, and on one shape the uncapped grid's spread limit + 1.  QP 1 of a batch does
not end in SUCCESS (MPC: an initial state far outside what the constraints allow; dense: contradictory rows); in the
derivative cases its data holds a NaN, so its factorisation fails and its slots must be exactly zero."""
import ctypes as C
import functools

import numpy as np
import pytest

from fbstab_amd.hip_api import MPC_SEQ, DENSE_ARR
from tools import fixtures as fx
from oracle.oracle_py import default_options
from tests import helpers as H
from tests import placement_helpers as P
from tests import linear_reference as LR
from tests import tangent_helpers as TH
from tests import reduced_helpers as R
from tests import sweep_adjoint_helpers as SH
from tests.helpers import OUT_FIELDS
from tests.hostsim import HostAdjoint

pytestmark = pytest.mark.gpu

CAP, GENERIC, THREADS, FLAT = ("FBSTAB_HIP_MAX_WORKGROUPS", "FBSTAB_HIP_GENERIC", "FBSTAB_HIP_DENSE_THREADS",
                               "FBSTAB_HIP_FLAT_ADJOINT")
SWEEP_STEP, SWEEP_ADJ_STEP = "FBSTAB_HIP_SWEEP_PER_STEP", "FBSTAB_HIP_SWEEP_ADJOINT_PER_STEP"
ERR_ARGUMENT = 1
STEP, RHS = ("dz", "dl", "dv"), ("gz", "gl", "gv")
R16, R32, FLAT_KERNEL = "fbstab_mpc_r16_kernel", "fbstab_mpc_r32_kernel", "fbstab_mpc_kernel<64>"
REC_ADJ, FLAT_ADJ = "fbstab_mpc_r16_adjoint_kernel", "fbstab_mpc_adjoint_kernel<64>"
PER_STEP = "fbstab_sweep_costate_kernel"

# id -> (kind, shape, environment at handle creation, solve kernel, adjoint kernel or None: solve only).  MPC shapes
# (N, nx, nu, nc), dense (nz, nl, nv): the smallest that reach each kernel.  Dense kernels are told by threads per QP
# and by where K lives: "dense256k" is the four-wavefront kernel with the KKT matrix in global memory - (116, 20, 150)
# is the smallest nz at (nl, nv) = (20, 150) for which DenseLayout::init says so ((110, 20, 150) keeps K in the LDS).
KERNELS = {
    "r16-12-4-20-exact": ("mpc", (3, 12, 4, 20), {}, R16 + "<12,4,20>", REC_ADJ + "<12,4,20>"),
    "r16-12-4-20-padded": ("mpc", (5, 6, 3, 8), {}, R16 + "<12,4,20>", REC_ADJ + "<12,4,20>"),
    "r16-12-4-32": ("mpc", (3, 6, 2, 27), {}, R16 + "<12,4,32>", REC_ADJ + "<12,4,32>"),
    "r32-18-5-10": ("mpc", (5, 16, 5, 9), {FLAT: "0"}, R32 + "<18,5,10>", REC_ADJ + "<18,5,10>"),
    "r32-24-8-16": ("mpc", (4, 20, 6, 16), {FLAT: "0"}, R32 + "<24,8,16>", REC_ADJ + "<24,8,16>"),
    "r32-24-8-32": ("mpc", (3, 14, 7, 21), {FLAT: "0"}, R32 + "<24,8,32>", REC_ADJ + "<24,8,32>"),
    "flat": ("mpc", (5, 6, 3, 8), {GENERIC: "1"}, FLAT_KERNEL, FLAT_ADJ),
    "dense-wave": ("dense", (20, 5, 40), {}, "dense64", "dense64"),
    "dense-wave-nl0": ("dense", (30, 0, 40), {}, "dense64", "dense64"),
    "dense-four": ("dense", (90, 12, 77), {THREADS: "256"}, "dense256", "dense256"),
    "dense-kkt-in-memory": ("dense", (116, 20, 150), {}, "dense256k", None),
}
SOLVE_IDS = list(KERNELS)
DERIV_IDS = [k for k, c in KERNELS.items() if c[4] is not None]
LAYOUTS = ["records", "spread"]
WHERE = ["host", "device"]


@pytest.fixture(scope="module")
def hip():
    from fbstab_amd import hip_api
    assert hip_api.load_library().fbstab_hip_device_count() >= 1
    return hip_api


def _device(where):
    if where == "host":
        return None
    import torch
    return torch.device("cuda:0")


# ---- problems ------------------------------------------------------------------------------------------------
def _mpc_problem(shape, B, shared=()):
    """Random LTV QPs; QP 1 starts 30 away from the origin in every state and ends PRIMAL_INFEASIBLE (the oracle
    says so, and every anchored case asserts it; 1e6 away where the constraints are shared: not SUCCESS either).  ``shared``: the batch is QP 0 repeated, with its own q, r and x0
    (small perturbations) where those are not shared - every QP then meets the one set of constraints."""
    p = fx.random_ltv_mpc(np.random.default_rng(8800 + shape[1]), B, *shape)
    a = {k: v.copy() for k, v in p.arrays.items()}
    if shared:
        rng = np.random.default_rng(8900 + shape[1])
        a = {k: np.repeat(v[:1], B, axis=0) for k, v in a.items()}
        for k in ("q", "r", "x0"):
            if k not in shared:
                a[k] = a[k] + 0.02 * rng.standard_normal(a[k].shape)
    if B > 1:
        # (the shared constraints of the (5, 16, 5, 9) batch still admit 1e4: there the solve runs into its iteration limit)
        a["x0"][1] = (1e6 if shared else 30.0) * np.where(a["x0"][1] < 0, -1.0, 1.0)
    return fx.MpcProblem(*shape, {k: np.ascontiguousarray(v) for k, v in a.items()})


def _dense_problem(shape, B, shared=()):
    """Synthetic dense QPs whose first two inequality rows are z_0 <= b_0 and -z_0 <= b_1 in every QP (so that A
    can be shared): b = (50, 50) but for QP 1, where (-1, -1) contradicts itself."""
    nz, nl, nv = shape
    p = fx.synthetic_dense_batch(B, nz, nl, nv, first_id=8800)
    a = {k: v.copy() for k, v in p.arrays.items()}
    if shared:
        a = {k: (np.repeat(v[:1], B, axis=0) if k in shared else v) for k, v in a.items()}
    A = a["A"].reshape(B, nz, nv).copy()   # [col][row]
    A[:, :, 0:2] = 0.0
    A[:, 0, 0], A[:, 0, 1] = 1.0, -1.0
    a["A"] = A.reshape(B, -1)
    a["b"] = a["b"].copy()
    a["b"][:, 0:2] = 50.0
    if B > 1:
        a["b"][1, 0:2] = -1.0
    q = fx.DenseProblem(nz, nl, nv)
    q.arrays = {k: np.ascontiguousarray(v) for k, v in a.items()}
    return q


def _problem(kind, shape, B, shared=()):
    return (_mpc_problem if kind == "mpc" else _dense_problem)(shape, B, tuple(shared))


def _names(kind):
    return MPC_SEQ if kind == "mpc" else DENSE_ARR


def _with_nan(p, kind):
    """The data of the derivative calls: a NaN in Q[0] / H[0] of QP 1, whose factorisation then fails (status 1)."""
    a = {k: v.copy() for k, v in p.arrays.items()}
    if p.batch > 1:
        a["Q" if kind == "mpc" else "H"][1, 0] = np.nan
    return a


# ---- handles ---------------------------------------------------------------------------------------------------
def _setenv(monkeypatch, env, cap=None):
    for k in (CAP, GENERIC, THREADS, FLAT, SWEEP_STEP, SWEEP_ADJ_STEP):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if cap is not None:
        monkeypatch.setenv(CAP, str(cap))


@functools.lru_cache(maxsize=None)
def _dense_layout(shape):
    return HostAdjoint("dense").layout(*shape)


def _handle(hip, case, B, cap=None):
    """A fresh handle of the case's kernel (the environment is the caller's: _setenv) with the default options; the
    kernels it will run are asserted here."""
    kind, shape, env, kern, adj = KERNELS[case]
    if kind == "mpc":
        s = hip.FBstabMpcBatch(*shape, max_batch=B)
        assert s.kernel_name() == kern, (s.kernel_name(), kern)
        if adj is not None:
            assert s.adjoint_kernel_name() == adj, (s.adjoint_kernel_name(), adj)
    else:
        s = hip.FBstabDenseBatch(*shape, max_batch=B)
        q = s.query()
        lay = _dense_layout(shape)
        name = "dense%d%s" % (q["threads"], "k" if q["threads"] == 256 and lay["k_global"] and q["scratch_bytes"] > 0 else "")
        assert name == kern, (name, kern, lay)
    if cap is not None:
        assert s.query()["workgroups"] == cap
    s.UpdateOptions(H._opts(hip, default_options()))
    return s


def _blocks(hip, s):
    if s._kind == "mpc":
        return hip._MpcBatch, hip._MpcGradBatch, MPC_SEQ, s.seq_len
    return hip._DenseBatch, hip._DenseGradBatch, DENSE_ARR, s.arr_len


def _restride(block, stride):
    """Case h: every slot of a block that is not NULL gets the one stride."""
    if stride is not None and block is not None:
        for i in range(len(block.base)):
            if block.base[i]:
                block.stride[i] = stride


def _stream(stream):
    return C.c_void_p(stream) if stream else None


def _np(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _assert_same(got, ref, what):
    assert set(got) == set(ref), (what, sorted(got), sorted(ref))
    for k in ref:
        a, b = _bits(got[k]), _bits(ref[k])
        assert a.shape == b.shape, (what, k, a.shape, b.shape)
        assert np.array_equal(a, b), (what, k, np.argwhere(a != b)[:4])


# ---- the entry points, called through the library with the blocks as the placements give them ---------------
def _lay(layout, arrays, canary=(), dev=None):
    return {"records": P.records, "spread": P.spread, "packed": P.packed}[layout](arrays, canary).on(dev)


def _vars(layout, p, B, dev, guess=None):
    """(z, l, v, y): the guess (zeros) placed, y canary (it is output only)."""
    z, l, v = guess if guess is not None else (np.zeros((B, n)) for n in (p.nz, p.nl, p.nv))
    return _lay(layout, dict(z=z, l=l, v=v, y=np.zeros((B, p.nv))), ("y",), dev)


def _solve(hip, s, D, X, B, final=False, keep=False, stride=None):
    """fbstab_hip_*_solve_batch[_final] on the data placement D and the variables X.  Returns (rc, results): z, l, v,
    y as they stand in X's slots, the SolverOut fields and, with ``final``, norms - out and norms packed by
    definition."""
    data_t, _, names, lens = _blocks(hip, s)
    blk, flags = data_t(), []
    P.fill_block(blk, names, lens, D, B, flags)
    vb = hip._fill_vars(tuple(X[k] for k in "zlvy"), (s.nz, s.nl, s.nv, s.nv), B, flags)
    _restride(blk, stride), _restride(vb, stride)
    where, fl, stream = hip._placement(flags, X["z"], keep_matrices=keep)
    out = where.out(X["z"], B)
    nrm = where.zeros(X["z"], (B, 4)) if final else None
    fn = getattr(s._lib, "fbstab_hip_%s_solve_batch%s" % (s._kind, "_final" if final else ""))
    args = [s._h, B, C.byref(blk), C.byref(vb), where.ptr(out)] + ([C.c_void_p(where.ptr(nrm))] if final else [])
    rc = fn(*args, fl, _stream(stream))
    res = {k: X.read(k) for k in "zlvy"}
    o = hip.out_to_numpy(out)
    res.update({f: o[f].copy() for f in OUT_FIELDS})
    if final:
        res["norms"] = _np(nrm)
    return rc, res


def _adjoint(hip, s, D, X, S, G, A, B, want=None, reduced=False, out=None, stride=None):
    """fbstab_hip_*_adjoint_batch[_reduced]: S the seeds (gz[, gl, gv]: absent slots NULL), G the gradient slots (of
    which ``want`` go into the block; slots G holds as one row are summed over the batch), A the adjoint slots or
    None.  Returns (rc, results): the wanted gradients, (dz, dl, dv) and status."""
    data_t, grad_t, names, lens = _blocks(hip, s)
    blk, gb, flags = data_t(), grad_t(), []
    var = (s.nz, s.nl, s.nv)
    P.fill_block(blk, names, lens, D, B, flags)
    xb = hip._fill_vars(tuple(X[k] for k in "zlv"), var, B, flags)
    sb = hip._fill_vars(tuple(S.views.get(k) for k in RHS), var, B, flags, optional=True)
    want = tuple(G.views) if want is None else want
    P.fill_block(gb, names, lens, G, B, [], optional=True, only=want)
    ab = hip._fill_vars(tuple(A[k] for k in STEP), var, B, []) if A is not None else None
    for b in (blk, xb, sb, gb, ab):
        _restride(b, stride)
    where, fl, stream = hip._placement(flags, X["z"])
    status = where.zeros(X["z"], B, "i4")
    args = [s._h, B, C.byref(blk), C.byref(xb), C.byref(sb), C.c_double(0.0), C.byref(gb),
            C.byref(ab) if ab is not None else None, C.c_void_p(where.ptr(status))]
    if reduced:
        args.append(C.c_void_p(where.ptr(out)) if out is not None else None)
    fn = getattr(s._lib, "fbstab_hip_%s_adjoint_batch%s" % (s._kind, "_reduced" if reduced else ""))
    rc = fn(*args, fl, _stream(stream))
    res = {k: G.read(k) for k in want}
    if A is not None:
        res.update({k: A.read(k) for k in STEP})
    res["status"] = _np(status)
    return rc, res


def _tangent(hip, s, D, X, DD, DX, RH, B, stride=None):
    """fbstab_hip_*_tangent_batch: DD the perturbations (absent names NULL, one-row names stride 0), DX the tangent
    slots, RH the right-hand side's or None."""
    data_t, _, names, lens = _blocks(hip, s)
    blk, db, flags = data_t(), data_t(), []
    var = (s.nz, s.nl, s.nv)
    P.fill_block(blk, names, lens, D, B, flags)
    P.fill_block(db, names, lens, DD, B, flags, optional=True)
    xb = hip._fill_vars(tuple(X[k] for k in "zlv"), var, B, flags)
    dxb = hip._fill_vars(tuple(DX[k] for k in STEP), var, B, [])
    rb = hip._fill_vars(tuple(RH[k] for k in RHS), var, B, []) if RH is not None else None
    for b in (blk, db, xb, dxb, rb):
        _restride(b, stride)
    where, fl, stream = hip._placement(flags, X["z"])
    status = where.zeros(X["z"], B, "i4")
    fn = getattr(s._lib, "fbstab_hip_%s_tangent_batch" % s._kind)
    rc = fn(s._h, B, C.byref(blk), C.byref(xb), C.byref(db), C.c_double(0.0), C.byref(dxb),
            C.byref(rb) if rb is not None else None, C.c_void_p(where.ptr(status)), fl, _stream(stream))
    res = {k: DX.read(k) for k in STEP}
    if RH is not None:
        res.update({k: RH.read(k) for k in RHS})
    res["status"] = _np(status)
    return rc, res


def _intact(*placed):
    for i, p in enumerate(placed):
        if p is not None:
            p.assert_intact("block %d" % i)


# ---- a. solves ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_solution(case, B):
    from oracle.oracle_py import Oracle
    kind, shape = KERNELS[case][:2]
    p = _problem(kind, shape, B)
    orc = Oracle(False)
    return orc.solve_mpc(p, opts=default_options()) if kind == "mpc" else orc.solve_dense(p, opts=default_options())


def _anchor_solve(case, p, res):
    """One placed solve per kernel against the oracle: the bar of the queue tests (tests/helpers._assert_parity:
    flags, proximal and Newton counts, the solution) on the QPs that end in SUCCESS, flag and proximal count on QP 1."""
    cpu = _oracle_solution(case, p.batch)
    oc = cpu[4]
    assert oc["eflag"][1] != 0 and (np.delete(oc["eflag"], 1) == 0).all(), oc["eflag"]
    assert res["eflag"][1] == oc["eflag"][1] and res["prox_iters"][1] == oc["prox_iters"][1]
    ok = np.flatnonzero(oc["eflag"] == 0)
    out = np.zeros(len(ok), dtype=[(f, res[f].dtype) for f in OUT_FIELDS])
    for f in OUT_FIELDS:
        out[f] = res[f][ok]
    gpu = tuple(res[k][ok] for k in "zlvy") + (out,)
    dense = None
    if KERNELS[case][3] == "dense64":   # (the one-wavefront kernel's bar in the queue tests: multipliers where unique)
        dense = fx.DenseProblem(p.nz, p.nl, p.nv)
        dense.arrays = {k: np.ascontiguousarray(a[ok]) for k, a in p.arrays.items()}
    H._assert_parity(gpu, tuple(t[ok] for t in cpu), default_options().abs_tol, dense=dense)


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case", SOLVE_IDS)
def test_placed_solves_are_the_packed_solves(hip, monkeypatch, case, layout, where):
    """fbstab_hip_*_solve_batch and _solve_batch_final with the data AND (z, l, v, y) placed, on ONE workgroup (B =
    7 / 5) and for one QP: z, l, v, y, the SolverOut fields and the norms bitwise those of the packed call, every
    gap intact.  The device-pointer records run of each kernel is also held to the oracle."""
    kind, shape, env = KERNELS[case][:3]
    dev = _device(where)
    for B, cap in ((7 if kind == "mpc" else 5, 1), (1, None)):
        _setenv(monkeypatch, env, cap)
        p = _problem(kind, shape, B)
        for final in (False, True):
            ref = _solve(hip, _handle(hip, case, B, cap), _lay("packed", p.arrays, dev=dev), _vars("packed", p, B, dev),
                         B, final)
            D, X = _lay(layout, p.arrays, dev=dev), _vars(layout, p, B, dev)
            got = _solve(hip, _handle(hip, case, B, cap), D, X, B, final)
            assert ref[0] == 0 and got[0] == 0
            _assert_same(got[1], ref[1], "%s B=%d final=%s" % (case, B, final))
            _intact(D, X)
            if B > 1:
                assert got[1]["eflag"][1] != 0 and (np.delete(got[1]["eflag"], 1) == 0).all(), got[1]["eflag"]
                if final and layout == "records" and where == "device":
                    _anchor_solve(case, p, got[1])


@pytest.mark.parametrize("layout", LAYOUTS)
def test_placed_solve_one_qp_past_the_spread_limit(hip, monkeypatch, layout):
    """The uncapped handle of the headline instance solves W QPs spread, one per wavefront, and W + 1 packed (rows
    1 to 3 busy: tests/test_gpu_queue.py computes the same boundary): W + 1 placed QPs on device pointers are
    bitwise the packed call's."""
    case = "r16-12-4-20-exact"
    kind, shape, env = KERNELS[case][:3]
    _setenv(monkeypatch, env)
    s = hip.FBstabMpcBatch(*shape, max_batch=1 << 16)
    W = s.query()["workgroups"]
    s.close()
    B = W + 1
    dev = _device("device")
    p = _problem(kind, shape, B)
    res = []
    for lay in ("packed", layout):
        h = _handle(hip, case, B)
        assert h.query()["workgroups"] == W < B
        D, X = _lay(lay, p.arrays, dev=dev), _vars(lay, p, B, dev)
        res.append(_solve(hip, h, D, X, B, final=True))
        _intact(D, X)
        h.close()
    assert res[0][0] == 0 and res[1][0] == 0
    _assert_same(res[1][1], res[0][1], "W + 1 = %d" % B)
    assert res[1][1]["eflag"][1] != 0 and (res[1][1]["eflag"] == 0).mean() > 0.9


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case", ["r16-12-4-20-padded", "r32-18-5-10"])
def test_placed_solves_with_kept_matrices(hip, monkeypatch, case, layout):
    """FBSTAB_HIP_KEEP_MATRICES on a one-row and a row-pair instance (QP q in slot q: the grid is not capped): two
    flagged calls, the second warm-started from the first with every x0 moved; the second call's results are
    bitwise the packed twin's."""
    kind, shape, env = KERNELS[case][:3]
    dev = _device("device")
    B = 7
    _setenv(monkeypatch, env)
    p = _problem(kind, shape, B)
    x0 = p.arrays["x0"] * 1.03 + 0.01
    res = {}
    for lay, keep in (("packed", True), (layout, True)):
        h = _handle(hip, case, B)
        assert B <= h.query()["workgroups"] * 2
        D, X = _lay(lay, p.arrays, dev=dev), _vars(lay, p, B, dev)
        assert _solve(hip, h, D, X, B, keep=keep)[0] == 0
        D.write("x0", x0)
        rc, res[lay, keep] = _solve(hip, h, D, X, B, keep=keep)
        assert rc == 0
        _intact(D, X)
        h.close()
    _assert_same(res[layout, True], res["packed", True], "kept")


# ---- b. shared data on the solve -------------------------------------------------------------------------------
_SHARED = [(c, n) for c in ("r16-12-4-20-padded", "r32-18-5-10", "flat")
           for n in (R.MPC_MATRICES, MPC_SEQ[:-1])] + \
          [(c, ("H", "G", "A")) for c in ("dense-wave", "dense-four")]


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("case,names", _SHARED, ids=["%s-%s" % (c, "".join(n)) for c, n in _SHARED])
def test_shared_data_solves_are_the_replicated_packed_solves(hip, monkeypatch, case, names, where):
    """The named arrays given ONCE (stride 0; one row and a gap), the others spread, against the packed batch in
    which the row is repeated for every QP: bitwise, on one workgroup, with the norms."""
    kind, shape, env = KERNELS[case][:3]
    dev = _device(where)
    B = 7 if kind == "mpc" else 5
    _setenv(monkeypatch, env, 1)
    p = _problem(kind, shape, B, shared=names)
    placed, twin = P.shared(p.arrays, names)
    assert all(np.array_equal(twin[k], p.arrays[k]) for k in twin)   # (the problem IS the replicated batch)
    D, X = placed.on(dev), _vars("spread", p, B, dev)
    got = _solve(hip, _handle(hip, case, B, 1), D, X, B, final=True)
    ref = _solve(hip, _handle(hip, case, B, 1), _lay("packed", twin, dev=dev), _vars("packed", p, B, dev), B, final=True)
    assert got[0] == 0 and ref[0] == 0
    _assert_same(got[1], ref[1], case)
    _intact(D, X)
    assert got[1]["eflag"][1] != 0 and (got[1]["eflag"] == 0).any(), got[1]["eflag"]


# ---- c. adjoints ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _points(case, B):
    """The points the derivative cases are taken at: the oracle's solutions of the case's problem (QP 1's is the end
    of a diverging run; its data gets a NaN anyway) and random seeds."""
    kind, shape = KERNELS[case][:2]
    p = _problem(kind, shape, B)
    z, l, v = _oracle_solution(case, B)[:3]
    x = tuple(np.where(np.isfinite(t), t, 0.0) for t in (z, l, v))
    seeds = LR.random_seeds(np.random.default_rng(31 + B), p)
    return p, x, seeds


def _grad_lens(kind, shape):
    return R.mpc_lens(*shape) if kind == "mpc" else R.dense_lens(*shape)


def _deriv_blocks(layout, kind, shape, p, x, seeds, B, dev, seed_names=RHS):
    """(D, X, S, G, A): the data with the NaN, the points, the seeds, and the gradient and adjoint slots, all
    canary."""
    D = _lay(layout, _with_nan(p, kind), dev=dev)
    X = _lay(layout, dict(zip("zlv", x)), dev=dev)
    S = _lay(layout, {k: a for k, a in zip(RHS, seeds) if k in seed_names}, dev=dev)
    lens = _grad_lens(kind, shape)
    G = _lay(layout, {k: np.zeros((B, lens[k])) for k in _names(kind)}, _names(kind), dev)
    A = _lay(layout, {k: np.zeros((B, n)) for k, n in zip(STEP, (p.nz, p.nl, p.nv))}, STEP, dev)
    return D, X, S, G, A


def _anchor_adjoint(kind, p, x, seeds, res, oracle):
    """The bar of the adjoint tests for the QPs of status 0: residual within 3 x the oracle's, the gradient table."""
    ok = [q for q in range(p.batch) if res["status"][q] == 0 and q != 1]
    if kind == "mpc":
        sub = fx.MpcProblem(p.N, p.nx, p.nu, p.nc, {k: np.ascontiguousarray(a[ok]) for k, a in p.arrays.items()})
        LR.check_mpc_batch(oracle, sub, tuple(t[ok] for t in x), tuple(t[ok] for t in seeds),
                           {k: a[ok] for k, a in res.items()})
        return
    for q in ok:
        xq, sq = tuple(t[q] for t in x), tuple(t[q] for t in seeds)
        LR.check_step_and_table(p, q, xq, sq, tuple(res[k][q] for k in STEP), {k: res[k][q] for k in DENSE_ARR},
                                LR.oracle_adjoint(oracle, p, q, xq, sq))


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("seeding", ["all_seeds", "gz_only"])
@pytest.mark.parametrize("case", DERIV_IDS)
def test_placed_adjoints_are_the_packed_adjoints(hip, oracle, monkeypatch, case, seeding, layout, where):
    """fbstab_hip_*_adjoint_batch with x, the seeds (gl and gv present, or NULL), all gradient slots and adj placed,
    on one workgroup and for one QP: bitwise the packed call, gaps intact, QP 1 (a NaN in its data: status 1)
    exactly zero in every slot.  The device-pointer records run with all seeds is held to the oracle's adjoint and
    the gradient table."""
    kind, shape, env = KERNELS[case][:3]
    dev = _device(where)
    seed_names = RHS if seeding == "all_seeds" else ("gz",)
    for B, cap in ((7 if kind == "mpc" else 5, 1), (1, None)):
        _setenv(monkeypatch, env, cap)
        p, x, seeds = _points(case, B)
        ref = _adjoint(hip, _handle(hip, case, B, cap), *_deriv_blocks("packed", kind, shape, p, x, seeds, B, dev, seed_names), B)
        blocks = _deriv_blocks(layout, kind, shape, p, x, seeds, B, dev, seed_names)
        got = _adjoint(hip, _handle(hip, case, B, cap), *blocks, B)
        assert ref[0] == 0 and got[0] == 0
        _assert_same(got[1], ref[1], "%s B=%d" % (case, B))
        _intact(*blocks)
        if B > 1:
            res = got[1]
            assert res["status"].tolist() == [0, 1] + [0] * (B - 2)
            for k in _names(kind) + STEP:
                assert not _bits(res[k][1]).any(), k   # (+0.0 in every entry)
                assert res[k].size == 0 or np.abs(np.delete(res[k], 1, axis=0)).max() > 0, k
            if seeding == "all_seeds" and layout == "records" and where == "device":
                _anchor_adjoint(kind, p, x, seeds, res, oracle)


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case", ["r16-12-4-20-padded", "r32-18-5-10", "flat", "dense-wave-nl0", "dense-four"])
def test_unwanted_gradient_slots_stay_untouched(hip, monkeypatch, case, layout, where):
    """Only {q, x0, A} (MPC) / {f, G} (dense; G is empty where nl == 0) wanted and no adj: the wanted slots are
    bitwise the packed call's, the buffers that would have held the others still hold their canaries."""
    kind, shape, env = KERNELS[case][:3]
    dev = _device(where)
    want = ("q", "x0", "A") if kind == "mpc" else ("f", "G")
    B = 7 if kind == "mpc" else 5
    _setenv(monkeypatch, env, 1)
    p, x, seeds = _points(case, B)
    res = []
    for lay in ("packed", layout):
        D, X, S, G, A = _deriv_blocks(lay, kind, shape, p, x, seeds, B, dev)
        res.append(_adjoint(hip, _handle(hip, case, B, 1), D, X, S, G, None, B, want=want))
        _intact(D, X, S, G, A)
        for k in _names(kind):
            if k not in want:
                assert (_bits(G.read(k)) == P.CANARY).all(), k
        for k in STEP:
            assert (_bits(A.read(k)) == P.CANARY).all(), k
    assert res[0][0] == 0 and res[1][0] == 0
    _assert_same(res[1][1], res[0][1], case)
    assert set(res[1][1]) == set(want) | {"status"}


# ---- d. reduced adjoints -------------------------------------------------------------------------------------------
_REDUCED = [(c, B) for c in ("r16-12-4-20-padded", "dense-wave") for B in (3, R.chunk() + 1)]


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case,B", _REDUCED, ids=["%s-B%d" % c for c in _REDUCED])
def test_reduced_adjoints_mix_one_row_sums_with_placed_slots(hip, monkeypatch, case, B, layout, where):
    """fbstab_hip_*_adjoint_batch_reduced with the matrices' gradients summed (stride 0: ONE row followed by a gap)
    and the vectors' per QP in placed slots: the per-QP slots, adj and status bitwise those of the placed
    fbstab_hip_*_adjoint_batch (case c), the sums bitwise the packed reduced call's and within the bound of the
    fp64 table (tests/reduced_helpers.check_sum), the canary behind each single row intact."""
    kind, shape, env = KERNELS[case][:3]
    dev = _device(where)
    matrices = R.MPC_MATRICES if kind == "mpc" else R.DENSE_MATRICES
    names = _names(kind)
    _setenv(monkeypatch, env)
    p, x, seeds = _points(case, B)
    lens = _grad_lens(kind, shape)
    grads = {k: np.zeros((B, lens[k])) for k in names}

    def run(lay):
        D, X, S, _, A = _deriv_blocks(lay, kind, shape, p, x, seeds, B, dev)
        G = P.shared(grads, matrices, canary=names, rest={"records": P.records, "spread": P.spread, "packed": P.packed}[lay])[0].on(dev)
        r = _adjoint(hip, _handle(hip, case, B), D, X, S, G, A, B, reduced=True)
        _intact(D, X, S, G, A)
        for k in matrices:
            assert G.views[k].shape[0] == 1 and G.slots[k][0].gap.sum() == P.GAP
        return r

    got, ref = run(layout), run("packed")
    blocks = _deriv_blocks(layout, kind, shape, p, x, seeds, B, dev)
    per_qp = _adjoint(hip, _handle(hip, case, B), *blocks, B)
    assert got[0] == 0 and ref[0] == 0 and per_qp[0] == 0
    _assert_same(got[1], ref[1], case)
    for k in tuple(k for k in names if k not in matrices) + STEP + ("status",):
        assert np.array_equal(_bits(got[1][k]), _bits(per_qp[1][k])), k
    keep = got[1]["status"] == 0
    assert keep.tolist() == [True, False] + [True] * (B - 2)
    step = tuple(got[1][k] for k in STEP)
    tab = (R.mpc_sum_table if kind == "mpc" else R.dense_sum_table)(*shape, x, step, keep)
    for k in matrices:
        R.check_sum(k, got[1][k], tab[k], B)


# ---- e. tangents ---------------------------------------------------------------------------------------------------
def _directions(kind, p, B):
    """Per-QP directions, two names shared by the batch (one row), two left out (NULL)."""
    shared, absent = (("R", "c"), ("S", "L")) if kind == "mpc" else (("f",), ("h",))
    names = tuple(k for k in _names(kind) if k not in absent)
    return TH.random_directions(np.random.default_rng(61), p, B, names=names), shared


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("rhs", ["rhs", "no_rhs"])
@pytest.mark.parametrize("case", DERIV_IDS)
def test_placed_tangents_are_the_packed_tangents(hip, monkeypatch, case, rhs, layout, where):
    """fbstab_hip_*_tangent_batch with ddata placed per QP, two slots NULL and two of stride 0, dx placed, rhs placed
    or NULL, on one workgroup and for one QP: bitwise the packed call with the same one-row directions, gaps
    intact, QP 1 (status 1) zero in dx.  The device-pointer records run with rhs: its seeds within the bound of
    tests/tangent_helpers.tangent_rhs for every QP."""
    kind, shape, env = KERNELS[case][:3]
    dev = _device(where)
    for B, cap in ((7 if kind == "mpc" else 5, 1), (1, None)):
        _setenv(monkeypatch, env, cap)
        p, x, _ = _points(case, B)
        d, shared = _directions(kind, p, B)
        res = []
        for lay in ("packed", layout):
            D = _lay(lay, _with_nan(p, kind), dev=dev)
            X = _lay(lay, dict(zip("zlv", x)), dev=dev)
            rest = {"records": P.records, "spread": P.spread, "packed": P.packed}[lay]
            DD = (P.shared(d, shared, rest=rest)[0] if B > 1 else rest(d)).on(dev)
            DX = _lay(lay, {k: np.zeros((B, n)) for k, n in zip(STEP, (p.nz, p.nl, p.nv))}, STEP, dev)
            RH = _lay(lay, {k: np.zeros((B, n)) for k, n in zip(RHS, (p.nz, p.nl, p.nv))}, RHS, dev) if rhs == "rhs" else None
            res.append(_tangent(hip, _handle(hip, case, B, cap), D, X, DD, DX, RH, B))
            _intact(D, X, DD, DX, RH)
        assert res[0][0] == 0 and res[1][0] == 0
        _assert_same(res[1][1], res[0][1], "%s B=%d" % (case, B))
        got = res[1][1]
        if B > 1:
            assert got["status"].tolist() == [0, 1] + [0] * (B - 2)
            assert not any(_bits(got[k][1]).any() for k in STEP)
            assert np.abs(np.delete(got["dz"], 1, axis=0)).max() > 0
            if rhs == "rhs" and layout == "records" and where == "device":
                for q in (q for q in range(B) if got["status"][q] == 0):
                    TH.assert_rhs(p, q, tuple(t[q] for t in x), TH.one_direction({k: (a[:1] if k in shared else a) for k, a in d.items()}, q),
                                  tuple(got[k][q] for k in RHS), case)


# ---- f. sweeps -----------------------------------------------------------------------------------------------------
def _tail(n, dev, rows=1):
    """``n`` doubles in one row followed by a canary tail in the same allocation: a packed array of the call."""
    return P.spread({"a": np.zeros((1, n))}, ("a",), first_pad=P.GAP).on(dev)


def _sweep_and_adjoint(hip, s, shape, data, x0, X, plant, B, steps, G, gu, gx, dev, stride=None):
    """fbstab_hip_mpc_receding_sweep_logged, then fbstab_hip_mpc_receding_sweep_adjoint on its log.  ``data``: the
    eleven arrays but x0, ``x0`` its own placement (stride nx + 3), ``plant``: a placement of A and B (one row:
    stride 0).  u_log and the log are packed, each with a canary tail.  Returns (rcs, results)."""
    import torch
    N, nx, nu, nc = shape
    D = P.merge(data, x0, order=MPC_SEQ)
    blk, flags = hip._MpcBatch(), []
    P.fill_block(blk, MPC_SEQ, s.seq_len, D, B, flags)
    vb = hip._fill_vars(tuple(X[k] for k in "zlvy"), (s.nz, s.nl, s.nv, s.nv), B, flags)
    assert all(flags)
    pa, pb = plant.slots["A"], plant.slots["B"]
    pl = hip._Plant(plant["A"].data_ptr(), plant["B"].data_ptr(), 0 if pa[3] == 1 else pa[2], 0 if pb[3] == 1 else pb[2])
    _restride(blk, stride), _restride(vb, stride)
    if stride is not None:
        pl.stride_A = pl.stride_B = stride
    out = torch.zeros((B, 40), dtype=torch.uint8, device=dev)
    u_log = _tail(steps * B * nu, dev)
    logs = {k: _tail(steps * B * n, dev) for k, n in (("z", s.nz), ("l", s.nl), ("v", s.nv), ("x0", nx))}
    eflag = torch.full((steps * B + 4,), 0x5EED5EED, dtype=torch.int32, device=dev)
    lg = hip._SweepLog(*[logs[k]["a"].data_ptr() for k in ("z", "l", "v", "x0")], eflag.data_ptr())
    stats = np.zeros((steps, 4), dtype=np.uint64)
    rc1 = s._lib.fbstab_hip_mpc_receding_sweep_logged(
        s._h, B, C.byref(blk), C.byref(vb), out.data_ptr(), C.byref(pl), steps, 1, u_log["a"].data_ptr(),
        stats.ctypes.data, None, None, C.byref(lg))
    res = {k: X.read(k) for k in "zlvy"}
    res["x0"] = x0.read("x0")
    res["u_log"] = u_log.read("a")
    res.update({k + "_log": t.read("a") for k, t in logs.items()})
    e = eflag.cpu().numpy()
    assert (e[-4:] == 0x5EED5EED).all()
    res["eflag_log"] = e[:-4].reshape(steps, B)
    o = hip.out_to_numpy(out)
    res.update({f: o[f].copy() for f in OUT_FIELDS})
    res["stats"] = stats
    _intact(D, X, plant, u_log, *logs.values())
    if rc1 != 0:
        return (rc1, None), res
    gb = hip._MpcGradBatch()
    P.fill_block(gb, MPC_SEQ, s.seq_len, G, B, [], optional=True)
    _restride(gb, stride)
    mu = _tail(steps * B * nx, dev)
    status = torch.zeros(B, dtype=torch.int32, device=dev)
    rc2 = s._lib.fbstab_hip_mpc_receding_sweep_adjoint(
        s._h, B, C.byref(blk), C.byref(pl), steps, 1, C.byref(lg), gu.data_ptr(), gx.data_ptr(), C.c_double(0.0),
        C.byref(gb), mu["a"].data_ptr(), status.data_ptr(), None)
    res.update({"grad_" + k: G.read(k) for k in MPC_SEQ})
    res["mu"] = mu.read("a")
    res["status"] = status.cpu().numpy()
    _intact(D, plant, G, mu, *logs.values())
    return (rc1, rc2), res


def _sweep_problem(shape, B, shared):
    p = _mpc_problem(shape, B, shared=MPC_SEQ[:-1] if shared else ())
    N, nx, nu, nc = shape
    rng = np.random.default_rng(9300 + nx)
    A = np.eye(nx) + 0.03 * rng.standard_normal((nx, nx))
    Bm = 0.1 * rng.standard_normal((nx, nu))
    return p, A, Bm, rng.standard_normal((3, B, nu)), rng.standard_normal((3, B, nx))


def _sweep_blocks(layout, p, A, Bm, B, shared, dev):
    """Placed run: the data by ``layout`` (x0 on its own at stride nx + 3) with ONE plant; shared run: everything but
    x0 given once, and a plant per trajectory (the same matrices, slightly different per trajectory) with gaps."""
    rest = {"records": P.records, "spread": P.spread, "packed": P.packed}[layout]
    eleven = {k: p.arrays[k] for k in MPC_SEQ[:-1]}
    x0 = (P.packed if layout == "packed" else functools.partial(P.spread, first_pad=3))({"x0": p.arrays["x0"]}).on(dev)
    X = _vars(layout, p, B, dev)
    col = lambda M: np.ascontiguousarray(M.T).reshape(1, -1)   # column-major image
    if shared:
        # (the problem IS QP 0's data repeated: the packed twin holds all B copies)
        data = (P.packed(eleven) if layout == "packed" else P.shared(eleven, MPC_SEQ[:-1])[0]).on(dev)
        scale = 1.0 + 1e-3 * np.arange(B)[:, None]
        plant = rest(dict(A=col(A) * scale, B=col(Bm) * scale)).on(dev)
    else:
        data = rest(eleven).on(dev)
        plant = P.shared(dict(A=col(A), B=col(Bm)), ("A", "B"))[0].on(dev)
    lens = p.seq_lengths()
    G = rest({k: np.zeros((B, lens[k])) for k in MPC_SEQ}, MPC_SEQ).on(dev)
    return data, x0, X, plant, G


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("data_mode", ["placed", "shared"])
@pytest.mark.parametrize("form", ["one_launch", "per_step"])
@pytest.mark.parametrize("case", ["r16-12-4-20-padded", "r32-18-5-10"])
def test_placed_sweeps_and_their_adjoints(hip, oracle, oracle_fma, monkeypatch, case, form, data_mode, layout):
    """Three steps of fbstab_hip_mpc_receding_sweep_logged and fbstab_hip_mpc_receding_sweep_adjoint on its log, in the
    one-launch forms and in the per-step forms: the data placed (x0 at stride nx + 3) with one plant, or everything
    but x0 shared with a plant per trajectory; x and the gradient slots placed; u_log, the log and mu_log packed
    with a canary tail.  Bitwise the packed twin, gaps and tails intact.  The per-step adjoint adds its packed
    temporary image into the caller's strided slots (fbstab_sweep_costate_kernel).  The records run on placed data
    is held to the recursion in numpy over the device's per-step adjoints, at ten times the spread of the
    reference's two roundings (tests/test_gpu_sweep_adjoint.py's bar)."""
    import torch
    kind, shape, env = KERNELS[case][:3]
    N, nx, nu, nc = shape
    dev = _device("device")
    B, steps, shared = 7, 3, data_mode == "shared"
    _setenv(monkeypatch, env)
    if form == "per_step":
        monkeypatch.setenv(SWEEP_STEP, "1")
        monkeypatch.setenv(SWEEP_ADJ_STEP, "1")
    p, A, Bm, gu, gx = _sweep_problem(shape, B, shared)
    gud, gxd = (torch.from_numpy(t).to(dev) for t in (gu, gx))
    res = []
    for lay in ("packed", layout):
        s = _handle(hip, case, B)
        assert s.sweep_adjoint_kernel_name() == (PER_STEP if form == "per_step" else KERNELS[case][4].replace("adjoint", "sweep_adjoint"))
        assert B <= s.query()["workgroups"] * 2   # (the one-launch sweep needs a slot per trajectory)
        data, x0, X, plant, G = _sweep_blocks(lay, p, A, Bm, B, shared, dev)
        res.append(_sweep_and_adjoint(hip, s, shape, data, x0, X, plant, B, steps, G, gud, gxd, dev))
        if lay == layout and layout == "records" and not shared:
            got = res[-1][1]
            log = dict(z=got["z_log"].reshape(steps, B, -1), l=got["l_log"].reshape(steps, B, -1),
                       v=got["v_log"].reshape(steps, B, -1), eflag=got["eflag_log"])
            bars, _ = SH.spread_bars(oracle, oracle_fma, p, A, Bm, log, gu, gx)
            ref, rst, _ = SH.reference_sweep_adjoint(SH.device_step_adjoint(s, p), p, A, Bm, log, gu, gx)
            assert np.array_equal(got["status"], rst)
            SH.assert_within({k: got["grad_" + k] for k in MPC_SEQ}, ref, bars, case)
        s.close()
    assert res[0][0] == (0, 0) and res[1][0] == (0, 0), (res[0][0], res[1][0])
    _assert_same(res[1][1], res[0][1], case)
    e = res[1][1]["eflag_log"]
    assert (e[:, 1] != 0).all() and (e == 0).any(), e


# ---- g. refusals ---------------------------------------------------------------------------------------------------
def _refusal_blocks(hip, s, p, B, dev):
    """Full-size packed blocks of a solve, and the snapshot that proves a refused call left them alone."""
    D, X = _lay("packed", p.arrays, dev=dev), _vars("packed", p, B, dev)
    data_t, _, names, lens = _blocks(hip, s)
    blk, flags = data_t(), []
    P.fill_block(blk, names, lens, D, B, flags)
    vb = hip._fill_vars(tuple(X[k] for k in "zlvy"), (s.nz, s.nl, s.nv, s.nv), B, flags)
    where, fl, stream = hip._placement(flags, X["z"])
    out = where.out(X["z"], B)
    return D, X, blk, vb, where, fl, stream, out


def _refused(hip, s, rc, text):
    assert rc == ERR_ARGUMENT, "no error returned (rc %d)" % rc
    assert text in s._lib.fbstab_hip_last_error().decode()
    assert s.last_kernel_ms() < 0   # (no launch was bracketed: nothing queued)


_BAD = [("variable_stride_below_the_length", "x", 0, lambda n: n - 1, "variable stride smaller than the vector length"),
        ("data_stride_below_the_length", "data", 3, lambda n: n - 1, "problem data stride smaller than the array length"),
        ("negative_data_stride", "data", 1, lambda n: -n, "problem data stride smaller than the array length")]


# (the sweeps take device pointers only: include/fbstab_hip.h)
_ENTRIES = [(e, w) for e in ("mpc_solve_batch", "mpc_solve_batch_final", "dense_solve_batch", "dense_solve_batch_final")
            for w in WHERE] + [("mpc_receding_sweep", "device"), ("mpc_receding_sweep_logged", "device")]


@pytest.mark.parametrize("bad", _BAD, ids=[b[0] for b in _BAD])
@pytest.mark.parametrize("entry,where", _ENTRIES, ids=["%s-%s" % e for e in _ENTRIES])
def test_solves_and_sweeps_refuse_strides_that_overlap(hip, monkeypatch, entry, where, bad):
    """batch = 3, every buffer of full packed size: a variable stride of len - 1, a data stride of len - 1 and a data
    stride of -len are FBSTAB_HIP_ERR_ARGUMENT on host AND device pointers (the sweeps take device pointers only),
    with the existing texts, before anything is queued, and no buffer changes."""
    _, block, slot, f, text = bad
    case = "dense-wave" if entry.startswith("dense") else "r16-12-4-20-padded"
    kind, shape, env = KERNELS[case][:3]
    dev = _device(where)
    B = 3
    _setenv(monkeypatch, env)
    p = _problem(kind, shape, B)
    s = _handle(hip, case, B)
    D, X, blk, vb, wh, fl, stream, out = _refusal_blocks(hip, s, p, B, dev)
    b = vb if block == "x" else blk
    b.stride[slot] = f(b.stride[slot])
    before = [bf.host_bits().copy() for pl in (D, X) for bf in pl.buffers] + [_np(out).copy()]
    fn = getattr(s._lib, "fbstab_hip_" + entry)
    if "sweep" in entry:
        import torch
        nx, nu = shape[1], shape[2]
        Ad, Bd = torch.eye(nx, dtype=torch.float64, device=dev).reshape(-1), torch.zeros(nx * nu, dtype=torch.float64, device=dev)
        pl = hip._Plant(Ad.data_ptr(), Bd.data_ptr(), 0, 0)
        u = torch.zeros(2 * B * nu, dtype=torch.float64, device=dev)
        args = [s._h, B, C.byref(blk), C.byref(vb), wh.ptr(out), C.byref(pl), 2, 1, u.data_ptr(), None, None, None]
        if entry.endswith("logged"):
            args.append(None)
        rc = fn(*args)
        assert not u.any()
    elif entry.endswith("final"):
        nrm = wh.zeros(X["z"], (B, 4))
        rc = fn(s._h, B, C.byref(blk), C.byref(vb), wh.ptr(out), C.c_void_p(wh.ptr(nrm)), fl, _stream(stream))
        assert not _np(nrm).any()
    else:
        rc = fn(s._h, B, C.byref(blk), C.byref(vb), wh.ptr(out), fl, _stream(stream))
    _refused(hip, s, rc, text)
    after = [bf.host_bits() for pl in (D, X) for bf in pl.buffers] + [_np(out)]
    assert all(np.array_equal(a, b_) for a, b_ in zip(before, after))


@pytest.mark.parametrize("kind", ["mpc", "dense"])
@pytest.mark.parametrize("entry", ["adjoint", "tangent"])
def test_adjoints_and_tangents_refuse_short_strides_on_device_pointers(hip, monkeypatch, kind, entry):
    """The refusals the adjoints and tangents already make, once each on the device path (batch = 3, full-size
    buffers): a gradient stride of len - 1, a perturbation stride of len - 1; and, like the solves now, a data
    stride of len - 1.  Nothing is written."""
    case = "r16-12-4-20-padded" if kind == "mpc" else "dense-wave"
    _, shape, env = KERNELS[case][:3]
    dev = _device("device")
    B = 3
    _setenv(monkeypatch, env)
    p, x, seeds = _points(case, B)
    s = _handle(hip, case, B)
    for which, text in (("own", None), ("data", "problem data stride smaller than the array length")):
        D, X, S, G, A = _deriv_blocks("packed", kind, shape, p, x, seeds, B, dev)
        data_t, grad_t, names, lens = _blocks(hip, s)
        blk, gb, db, flags = data_t(), grad_t(), data_t(), []
        P.fill_block(blk, names, lens, D, B, flags)
        xb = hip._fill_vars(tuple(X[k] for k in "zlv"), (s.nz, s.nl, s.nv), B, flags)
        sb = hip._fill_vars(tuple(S[k] for k in RHS), (s.nz, s.nl, s.nv), B, flags, optional=True)
        ab = hip._fill_vars(tuple(A[k] for k in STEP), (s.nz, s.nl, s.nv), B, [])
        P.fill_block(gb, names, lens, G, B, [])
        DD = _lay("packed", TH.random_directions(np.random.default_rng(5), p, B), dev=dev)
        P.fill_block(db, names, lens, DD, B, [])
        if which == "data":
            blk.stride[1] -= 1
        elif entry == "adjoint":
            gb.stride[1] -= 1
            text = "gradient stride smaller than the array length"
        else:
            db.stride[1] -= 1
            text = "perturbation stride is neither 0 nor at least the array length"
        where, fl, stream = hip._placement(flags, X["z"])
        status = where.zeros(X["z"], B, "i4")
        if entry == "adjoint":
            rc = getattr(s._lib, "fbstab_hip_%s_adjoint_batch" % kind)(
                s._h, B, C.byref(blk), C.byref(xb), C.byref(sb), C.c_double(0.0), C.byref(gb), C.byref(ab),
                C.c_void_p(status.data_ptr()), fl, _stream(stream))
        else:
            rc = getattr(s._lib, "fbstab_hip_%s_tangent_batch" % kind)(
                s._h, B, C.byref(blk), C.byref(xb), C.byref(db), C.c_double(0.0), C.byref(ab), None,
                C.c_void_p(status.data_ptr()), fl, _stream(stream))
        _refused(hip, s, rc, text)
        for k in names:
            assert (_bits(G.read(k)) == P.CANARY).all(), k
        for k in STEP:
            assert (_bits(A.read(k)) == P.CANARY).all(), k


# ---- h. one QP -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("stride", [0, 1])
@pytest.mark.parametrize("case", ["r16-12-4-20-padded", "flat", "dense-wave"])
def test_one_qp_lives_at_the_base_whatever_the_strides_say(hip, monkeypatch, case, stride, where):
    """batch == 1 with EVERY stride of every block set to 0, and to 1: solve, solve_final, adjoint, reduced adjoint
    (stride 1 only: a gradient stride of 0 asks for the sum there at every batch size), tangent and - device
    pointers, record handle - the logged sweep with its adjoint are bitwise the packed call.  On host pointers a
    stride of 1 used to reach hipMemcpy2DAsync as a pitch below the width."""
    kind, shape, env = KERNELS[case][:3]
    dev = _device(where)
    B = 1
    _setenv(monkeypatch, env)
    p = _problem(kind, shape, B)
    _, x, seeds = _points(case, B)
    d = TH.random_directions(np.random.default_rng(62), p, B)
    zeros = lambda names, lens: {k: np.zeros((B, n)) for k, n in zip(names, lens)}
    var = (p.nz, p.nl, p.nv)
    results = []
    for st in (None, stride):
        r = {}
        for final in (False, True):
            rc, r["solve%d" % final] = _solve(hip, _handle(hip, case, B), _lay("packed", p.arrays, dev=dev),
                                              _vars("packed", p, B, dev), B, final, stride=st)
            assert rc == 0
        for reduced in (False, True):
            if reduced and stride == 0:
                continue
            blocks = _deriv_blocks("packed", kind, shape, p, x, seeds, B, dev)
            rc, r["adjoint%d" % reduced] = _adjoint(hip, _handle(hip, case, B), *blocks, B, reduced=reduced, stride=st)
            assert rc == 0
        D, X = _lay("packed", p.arrays, dev=dev), _lay("packed", dict(zip("zlv", x)), dev=dev)
        rc, r["tangent"] = _tangent(hip, _handle(hip, case, B), D, X, _lay("packed", d, dev=dev),
                                    _lay("packed", zeros(STEP, var), STEP, dev), _lay("packed", zeros(RHS, var), RHS, dev), B,
                                    stride=st)
        assert rc == 0
        if where == "device" and kind == "mpc":
            import torch
            _, A, Bm, gu, gx = _sweep_problem(shape, B, False)
            data, x0, X, plant, G = _sweep_blocks("packed", p, A, Bm, B, False, dev)
            rcs, r["sweep"] = _sweep_and_adjoint(hip, _handle(hip, case, B), shape, data, x0, X, plant, B, 3, G,
                                                 torch.from_numpy(gu).to(dev), torch.from_numpy(gx).to(dev), dev, stride=st)
            assert rcs == (0, 0), rcs
        results.append(r)
    for k in results[0]:
        _assert_same(results[1][k], results[0][k], "%s stride %d" % (k, stride))
    assert results[0]["solve0"]["eflag"][0] == 0 and results[0]["adjoint0"]["status"][0] == 0
