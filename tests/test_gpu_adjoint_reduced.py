"""GPU checks of the batch-summed gradients (fbstab_hip_mpc_adjoint_batch_reduced,
fbstab_hip_dense_adjoint_batch_reduced, ``Adjoint(..., reduce=...)``, shared parameters in fbstab_amd.autograd):
the sums against the gradient table in extended precision within the worst-case bound of a sum of 2 B rounded
products in any order, per-QP slots and the adjoint bitwise those of fbstab_hip_*_adjoint_batch, determinism
(the same bits twice, and from a handle on two workgroups), QPs left out for their eflag or their adjoint status,
autograd, and host against device pointers.

Shapes: tests/reduced_helpers.py (one per solve kernel that feeds the reducer).  Batch sizes, with C the chunk
constant of fb_grad_reduce_plan.h: 1, 3, C, C + 1, 2 C + 3 on the smallest shape of each kind - one short chunk, a
full one, a full and a short one, two full and a short one - and C + 1 elsewhere."""
import gc

import numpy as np
import pytest

from tools import fixtures as fx
from tests import linear_reference as LR
from tests import reduced_helpers as R

pytestmark = pytest.mark.gpu

CAP = "FBSTAB_HIP_MAX_WORKGROUPS"
STEP = ("dz", "dl", "dv")
C = R.chunk()
SMALL = {"dense": (5, 2, 9), "mpc": (4, 5, 2, 7)}
CASES = [(kind, shape, B) for kind, shapes in (("dense", R.DENSE_SHAPES), ("mpc", R.MPC_SHAPES)) for shape in shapes
         for B in ((1, 3, C, C + 1, 2 * C + 3) if shape == SMALL[kind] else (C + 1,))]
IDS = ["%s-%s-B%d" % (k, "x".join(map(str, s)), B) for k, s, B in CASES]


@pytest.fixture(scope="module")
def hip():
    from fbstab_amd import hip_api
    assert hip_api.load_library().fbstab_hip_device_count() >= 1
    return hip_api


class Case:
    """A solved batch of one kind and shape: handle, data, points, seeds, and the calls the tests share."""

    def __init__(self, hip, kind, shape, B, problem=None):
        self.kind, self.shape, self.B = kind, shape, B
        if kind == "dense":
            self.names, self.matrices = R.DENSE_ARR, R.DENSE_MATRICES
            self.p = problem or fx.synthetic_dense_batch(B, *shape, first_id=1000)
            self.make = lambda mb=B: hip.FBstabDenseBatch(*shape, max_batch=mb)
            self.seeds = LR.random_seeds(np.random.default_rng(B), self.p)
        else:
            self.names, self.matrices = R.MPC_SEQ, R.MPC_MATRICES
            self.p = problem or fx.random_ltv_mpc(np.random.default_rng(9000 + shape[1]), B, *shape)
            self.make = lambda mb=B: hip.FBstabMpcBatch(*shape, max_batch=mb)
            self.seeds = LR.random_seeds(np.random.default_rng(B), self.p)
        self.vectors = tuple(k for k in self.names if k not in self.matrices)
        self.data = {k: np.ascontiguousarray(a) for k, a in self.p.arrays.items()}
        self.s = self.make()
        p = self.p
        z, l, v, y = (np.zeros((B, n)) for n in (p.nz, p.nl, p.nv, p.nv))
        self.out = self.s.Solve(self.data, z, l, v, y)
        self.x = (z, l, v)
        self._memo = {}

    def adjoint(self, s=None, x=None, data=None, **kw):
        return (s or self.s).Adjoint(data or self.data, *(x or self.x), *self.seeds, adj=True, **kw)

    def old(self):
        """fbstab_hip_*_adjoint_batch: every slot per QP."""
        if "old" not in self._memo:
            self._memo["old"] = self.adjoint()
        return self._memo["old"]

    def all_reduced(self):
        if "red" not in self._memo:
            self._memo["red"] = self.adjoint(reduce=self.names)
        return self._memo["red"]

    def table(self, x, step, keep=None):
        if self.kind == "dense":
            return R.dense_sum_table(*self.shape, x, step, keep)
        return R.mpc_sum_table(*self.shape, x, step, keep)

    def check(self, res, keep=None, x=None, names=None, batch=None):
        """Every reduced array of ``res`` against the table of the RETURNED (x, adj), within the bound."""
        tab = self.table(x or self.x, tuple(res[k] for k in STEP), keep)
        worst = 0.0
        for k in names or self.names:
            assert res[k].shape[0] == 1, (k, res[k].shape)
            worst = max(worst, R.check_sum(k, res[k], tab[k], batch or self.B))
        print("%s %s B=%d: largest difference / bound %.3f" % (self.kind, self.shape, self.B, worst))


_cases = {}


@pytest.fixture(scope="module", autouse=True)
def _release_the_shared_cases():
    """The solved batches are shared by the tests of this module and released with it: a handle owns device
    memory and a stream, and none of them outlives the module."""
    yield
    for c in _cases.values():
        c.s.close()
    _cases.clear()
    gc.collect()  # (handles that autograd graphs of this module still hold)


@pytest.fixture
def case(hip, request):
    key = request.param
    if key not in _cases:
        _cases[key] = Case(hip, *key)
    return _cases[key]


@pytest.mark.parametrize("case", CASES, ids=IDS, indirect=True)
def test_sums_against_the_table_and_the_rest_bitwise_the_old_call(case):
    """One call with ``adj`` and every slot reduced: |difference| <= (2 B + 4) 2^-53 S entry by entry against the
    table in longdouble from the returned (x, adj) (S: the magnitudes of the entry's products summed over the
    batch - the worst case of any order of summation, derived, not tuned); adj and status bitwise those of
    fbstab_hip_*_adjoint_batch on the same handle."""
    old, red = case.old(), case.all_reduced()
    for k in STEP + ("status",):
        assert np.array_equal(red[k], old[k]), k
    assert (old["status"] == 0).all()
    case.check(red)
    assert all(np.abs(red[k]).sum() > 0 for k in case.matrices if red[k].size)


@pytest.mark.parametrize("case", CASES, ids=IDS, indirect=True)
def test_mixed_slots(case):
    """The matrices reduced and the vectors per QP in one call: the per-QP slots, adj and status bitwise the old
    call's, the reduced ones bitwise those of the call that reduces everything (hence within its bound)."""
    old, red = case.old(), case.all_reduced()
    mix = case.adjoint(reduce=case.matrices)
    for k in case.vectors + STEP + ("status",):
        assert mix[k].shape == old[k].shape and np.array_equal(mix[k], old[k]), k
    for k in case.matrices:
        assert mix[k].shape == red[k].shape and np.array_equal(mix[k], red[k]), k
    case.check(mix, names=case.matrices)
    # ... and without `adj`: the sums are formed from the handle's own copy of the adjoint steps
    quiet = case.s.Adjoint(case.data, *case.x, *case.seeds, reduce=case.matrices, want=case.matrices)
    assert set(quiet) == set(case.matrices) | {"status"}
    for k in case.matrices:
        assert np.array_equal(quiet[k], red[k]), k


@pytest.mark.parametrize("case", [c for c in CASES if c[2] == 2 * C + 3], ids=lambda c: c[0], indirect=True)
def test_the_same_bits_twice_and_from_a_handle_on_two_workgroups(case, monkeypatch):
    """The order of every sum is fixed by the shape and the batch size: the same call twice gives identical bits,
    and so does a handle created under FBSTAB_HIP_MAX_WORKGROUPS=2, whose adjoint packs and re-fetches."""
    red = case.all_reduced()
    again = case.adjoint(reduce=case.names)
    monkeypatch.setenv(CAP, "2")
    packed_h = case.make()
    monkeypatch.delenv(CAP)
    assert packed_h.query()["workgroups"] == 2 < case.B
    packed = case.adjoint(s=packed_h, reduce=case.names)
    for k in case.names + STEP + ("status",):
        assert np.array_equal(again[k], red[k]), k
        assert np.array_equal(packed[k], red[k]), k


def _infeasible_dense(B, shape, q):
    """tests/test_gpu_dense_adjoint.py's mixed-outcome batch: QP q has z_0 <= -1 and -z_0 <= -1."""
    nz, nl, nv = shape
    p = fx.synthetic_dense_batch(B, nz, nl, nv, first_id=60)
    A = p.arrays["A"].copy().reshape(B, nz, nv)   # [col][row]
    A[q, :, 0:2] = 0.0
    A[q, 0, 0], A[q, 0, 1] = 1.0, -1.0
    p.arrays["A"] = np.ascontiguousarray(A.reshape(B, -1))
    p.arrays["b"] = p.arrays["b"].copy()
    p.arrays["b"][q, 0:2] = -1.0
    return p


def _infeasible_mpc(B, shape, q):
    """tests/test_gpu_adjoint.py's mixed-outcome batch: QP q has u_0(0) <= -1 and u_0(0) >= 1."""
    N, nx, nu, nc = shape
    p = fx.random_ltv_mpc(np.random.default_rng(6060), B, N, nx, nu, nc)
    for r, sgn in ((0, 1.0), (1, -1.0)):
        p.arrays["E"][q, r:(N + 1) * nc * nx:nc][:nx] = 0.0
        for j in range(nu):
            p.arrays["L"][q, r + j * nc] = sgn if j == 0 else 0.0
        p.arrays["d"][q, r] = 1.0
    return p


@pytest.mark.parametrize("kind,shape", [("dense", (20, 5, 40)), ("mpc", (6, 4, 2, 6))], ids=["dense", "mpc"])
def test_a_qp_that_is_not_success_is_left_out_with_out(hip, kind, shape):
    """One QP of the batch is infeasible (eflag != SUCCESS); its point is overwritten with NaN before the adjoint
    call.  With ``out`` every reduced slot is finite and is the reduction of the batch without that QP: within the
    bound of the table over the other QPs, and of the call on the batch with the QP removed."""
    B, q = 6, 1
    c = Case(hip, kind, shape, B, problem=(_infeasible_dense if kind == "dense" else _infeasible_mpc)(B, shape, q))
    eflag = c.out["eflag"]
    assert eflag[q] != 0 and (np.delete(eflag, q) == 0).all(), eflag
    x = tuple(t.copy() for t in c.x)
    for t in x:
        t[q] = np.nan
    red = c.adjoint(x=x, reduce=c.names, out=c.out)
    keep = np.arange(B) != q
    for k in c.names:
        assert np.isfinite(red[k]).all(), k
    c.check(red, keep=keep, x=x)
    # the batch with the QP removed: the same per-QP terms (a QP's adjoint does not depend on its neighbours)
    sub = c.s.Adjoint({k: np.ascontiguousarray(a[keep]) for k, a in c.data.items()}, *(t[keep] for t in c.x),
                      *(t[keep] for t in c.seeds), adj=True, reduce=c.names)
    for k in STEP:
        assert np.array_equal(sub[k], red[k][keep]), k
    tab = c.table(tuple(t[keep] for t in c.x), tuple(sub[k] for k in STEP))
    for k in c.names:
        R.check_sum(k, red[k], tab[k], B)
        R.check_sum(k, sub[k], tab[k], B - 1)
    # per-QP slots do not depend on `out`
    mix = c.adjoint(x=c.x, reduce=c.matrices, out=c.out)
    old = c.old()
    for k in c.vectors + STEP + ("status",):
        assert np.array_equal(mix[k], old[k]), k


@pytest.mark.parametrize("kind,shape", [("dense", (50, 10, 100)), ("mpc", (3, 12, 4, 20))], ids=["dense", "mpc"])
def test_a_qp_whose_factorisation_failed_is_left_out_without_out(hip, kind, shape):
    """The set-up of the failed-factorisation tests: a NaN in H[0] / Q[0] of QP 1 is a NaN on the diagonal of K -
    status 1.  Without ``out`` that QP is left out of every reduced slot, its NaN point included."""
    B, q = 3, 1
    c = Case(hip, kind, shape, B)
    assert (c.out["eflag"] == 0).all()
    bad = {k: a.copy() for k, a in c.data.items()}
    bad[c.names[0]][q, 0] = np.nan
    x = tuple(t.copy() for t in c.x)
    x[2][q] = np.nan
    red = c.adjoint(x=x, data=bad, reduce=c.names)
    assert red["status"].tolist() == [0, 1, 0]
    keep = np.arange(B) != q
    for k in c.names:
        assert np.isfinite(red[k]).all() and np.abs(red[k]).max() > 0, k
    c.check(red, keep=keep, x=x)


def _shared_dense(B, nz, nl, nv, q):
    """One (H, G, A) for the whole batch (column-major images of length len) and per-QP f, h, b that make every QP
    feasible - h = G z*, b = A z* + slack at a random z* of its own, a quarter of the rows without slack - but QP
    q: rows 0 and 1 of A are opposite, and its b asks for a'z <= -1 and -a'z <= -1.  Returns (the batch with the
    matrices repeated, the arrays as the autograd test passes them)."""
    rng = np.random.default_rng(7700)
    M = rng.standard_normal((nz, nz))
    Hm = M @ M.T / nz + 0.5 * np.eye(nz)
    G, A = rng.standard_normal((nl, nz)), rng.standard_normal((nv, nz))
    A[1] = -A[0]
    zs = rng.standard_normal((B, nz))
    slack = np.where(rng.random((B, nv)) < 0.25, 0.0, rng.random((B, nv)) + 0.1)
    slack[:, 0:2] = 0.5
    b = zs @ A.T + slack
    b[q, 0:2] = -1.0
    arrays = dict(H=np.ascontiguousarray(Hm.T.reshape(-1)), f=rng.standard_normal((B, nz)),
                  G=np.ascontiguousarray(G.T.reshape(-1)), h=zs @ G.T, A=np.ascontiguousarray(A.T.reshape(-1)), b=b)
    p = fx.DenseProblem(nz, nl, nv)
    p.arrays = {k: np.ascontiguousarray(a if a.ndim == 2 else np.tile(a, (B, 1))) for k, a in arrays.items()}
    return p, arrays


def test_autograd_dense_shared_matrices(hip):
    """solve_dense with H, G, A of shape (len,) requiring grad beside per-QP f, h, b (QP 1 infeasible): the forward
    (z, l, v) bitwise those of the expanded solve, .grad of the parameter's shape and, within the bound, the batch
    sum of the gradients of the existing per-QP path on the expanded and cloned inputs (which zeroes the unsolved
    QP: it contributes nothing); the per-QP inputs' gradients bitwise that path's."""
    import torch
    from fbstab_amd.autograd import solve_dense
    dev = torch.device("cuda:0")
    nz, nl, nv = 20, 5, 40
    B, q = 5, 1
    shared = ("H", "G", "A")
    p, arrays = _shared_dense(B, nz, nl, nv, q)
    solver = hip.FBstabDenseBatch(nz, nl, nv, max_batch=B)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    data = {k: t(a).requires_grad_(True) for k, a in arrays.items()}
    assert all(data[k].shape == (solver.arr_len[i],) for i, k in enumerate(R.DENSE_ARR) if k in shared)
    z, l, v, out = solve_dense(solver, data)
    eflag = hip.out_to_numpy(out)["eflag"]
    assert eflag[q] != 0 and (np.delete(eflag, q) == 0).all(), eflag
    seeds = [t(s) for s in LR.random_seeds(np.random.default_rng(12), p)]
    (sum((a * w).sum() for a, w in zip(seeds, (z, l, v)))).backward()
    # the existing per-QP path on expanded and cloned inputs
    wide = {k: (a.detach().expand(B, -1).clone() if k in shared else a.detach().clone()).requires_grad_(True)
            for k, a in data.items()}
    z2, l2, v2, out2 = solve_dense(hip.FBstabDenseBatch(nz, nl, nv, max_batch=B), wide)
    (sum((a * w).sum() for a, w in zip(seeds, (z2, l2, v2)))).backward()
    torch.cuda.synchronize()
    for a, w in ((z, z2), (l, l2), (v, v2)):
        assert torch.equal(a, w)
    _compare_shared_grads(hip, solver, data, wide, shared, R.DENSE_ARR, (z, l, v), seeds, eflag, B,
                          lambda x, step, keep: R.dense_sum_table(nz, nl, nv, x, step, keep))


def _compare_shared_grads(hip, solver, data, wide, shared, names, x, seeds, eflag, B, table):
    import torch
    keep = eflag == 0
    ref = solver.Adjoint({k: a.detach() for k, a in wide.items()}, *(t.detach() for t in x), *seeds, adj=True)
    torch.cuda.synchronize()
    keep &= ref["status"].cpu().numpy() == 0
    xs = tuple(t.detach().cpu().numpy() for t in x)
    tab = table(xs, tuple(ref[k].cpu().numpy() for k in STEP), keep)
    for k in names:
        g, w = data[k].grad, wide[k].grad
        assert g is not None and g.shape == data[k].shape, k
        if k in shared:
            assert g.dim() == 1
            R.check_sum(k, g.cpu().numpy(), tab[k], B)
            # ... and against the per-QP path's own gradients, summed over the batch in longdouble
            R.check_sum(k, g.cpu().numpy(), (w.cpu().numpy().astype(np.longdouble).sum(axis=0), tab[k][1]), B)
            assert np.abs(g.cpu().numpy()).max() > 0, k
        else:
            assert torch.equal(g, w), k
            assert not g[~torch.from_numpy(keep).to(g.device)].any(), k


def test_autograd_mpc_shared_matrices(hip):
    """solve_mpc with shared Q, R, A, B (shape (len,) and (1, len)) requiring grad, the other sequences per QP (QP 1
    infeasible): as the dense test."""
    import torch
    from fbstab_amd.autograd import solve_mpc
    dev = torch.device("cuda:0")
    shape = (6, 4, 2, 6)
    N, nx, nu, nc = shape
    B, q = 5, 1
    p = _infeasible_mpc(B, shape, q)
    shared = ("Q", "R", "A", "B")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    data = {}
    for k, a in p.arrays.items():
        if k in shared:
            data[k] = t(a[0:1].copy() if k in ("R", "B") else a[0].copy()).requires_grad_(True)  # (1, len) and (len,)
        elif k == "S":  # (shared as well, so that the stage Hessians stay QP 0's: a shared input that wants no gradient)
            data[k] = t(a[0:1].copy())
        else:
            data[k] = t(a.copy()).requires_grad_(k in ("q", "E", "d", "x0"))
    solver = hip.FBstabMpcBatch(*shape, max_batch=B)
    z, l, v, out = solve_mpc(solver, data)
    eflag = hip.out_to_numpy(out)["eflag"]
    assert eflag[q] != 0 and (np.delete(eflag, q) == 0).all(), eflag
    seeds = [t(s) for s in LR.random_seeds(np.random.default_rng(12), p)]
    (sum((a * w).sum() for a, w in zip(seeds, (z, l, v)))).backward()
    wide = {k: (a.detach().reshape(1, -1).expand(B, -1).clone() if k in shared + ("S",) else a.detach().clone())
            .requires_grad_(a.requires_grad) for k, a in data.items()}
    z2, l2, v2, out2 = solve_mpc(hip.FBstabMpcBatch(*shape, max_batch=B), wide)
    (sum((a * w).sum() for a, w in zip(seeds, (z2, l2, v2)))).backward()
    torch.cuda.synchronize()
    for a, w in ((z, z2), (l, l2), (v, v2)):
        assert torch.equal(a, w)
    keep = eflag == 0
    ref = solver.Adjoint({k: a.detach() for k, a in wide.items()}, z.detach(), l.detach(), v.detach(), *seeds, adj=True)
    torch.cuda.synchronize()
    keep &= ref["status"].cpu().numpy() == 0
    tab = R.mpc_sum_table(N, nx, nu, nc, tuple(a.detach().cpu().numpy() for a in (z, l, v)),
                          tuple(ref[k].cpu().numpy() for k in STEP), keep)
    for k in R.MPC_SEQ:
        g, w = data[k].grad, wide[k].grad
        if not data[k].requires_grad:
            assert g is None and w is None, k
            continue
        assert g.shape == data[k].shape, k
        if k in shared:
            R.check_sum(k, g.cpu().numpy(), tab[k], B)
            # ... and against the per-QP path's own gradients, summed over the batch in longdouble
            R.check_sum(k, g.cpu().numpy(), (w.cpu().numpy().astype(np.longdouble).sum(axis=0), tab[k][1]), B)
            assert np.abs(g.cpu().numpy()).max() > 0, k
        else:
            assert torch.equal(g, w), k
            assert not g[q].any(), k


@pytest.mark.parametrize("kind,shape", [("dense", (5, 2, 9)), ("mpc", (4, 5, 2, 7))], ids=["dense", "mpc"])
def test_host_pointers_equal_device_pointers(hip, kind, shape):
    """A reduced call on host pointers (one array downloaded per reduced slot, `out` on the host) returns the bits
    of the device-pointer call, per-QP slots, adj and status included."""
    import torch
    dev = torch.device("cuda:0")
    key = (kind, shape, C + 1)
    c = _cases[key] if key in _cases else Case(hip, *key)
    host = c.adjoint(reduce=c.matrices, out=c.out)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    out_dev = torch.from_numpy(c.out.view(np.uint8).reshape(c.B, 40).copy()).to(dev)
    on_dev = c.s.Adjoint({k: t(a) for k, a in c.data.items()}, *(t(a) for a in c.x), *(t(a) for a in c.seeds),
                         adj=True, reduce=c.matrices, out=out_dev)
    torch.cuda.synchronize()
    for k in c.names + STEP + ("status",):
        assert host[k].shape == tuple(on_dev[k].shape), k
        assert np.array_equal(host[k], on_dev[k].cpu().numpy()), k
    for k in c.matrices:
        assert host[k].shape[0] == 1 and np.abs(host[k]).max() > 0, k
