"""GPU checks of the record adjoint on the ROW-PAIR instances (<18,5,10>, <24,8,16>, <24,8,32>: stage widths up to
32, two QPs per wavefront): every new kernel - padded and exact - against the oracle in both forms of the costate
step and against the flat-vector adjoint of the same QPs (FBSTAB_HIP_FLAT_ADJOINT=1), both QPs of a wavefront and
the re-fetch, the rebuild of kept matrix copies, torch autograd on a wide shape, and the status of a QP whose
factorisation fails.  Handles are created under FBSTAB_HIP_FLAT_ADJOINT=0, which selects the record adjoint: a
row-pair handle's default stays the flat-vector adjoint until the two have been timed on the wide workloads
(test_the_knob_and_the_defaults).  The bars are those of tests/linear_reference.py (check_mpc_batch): residual within
3 x the oracle's, step within 1e-5 of the oracle's, the gradient table at rtol 1e-13."""
import numpy as np
import pytest

from fbstab_amd.hip_api import MPC_SEQ
from tools import fixtures as fx
from tests import helpers as H
from tests import linear_reference as LR

pytestmark = pytest.mark.gpu

CAP = "FBSTAB_HIP_MAX_WORKGROUPS"
FLAT = "FBSTAB_HIP_FLAT_ADJOINT"
RECORD_ADJOINT = "fbstab_mpc_r16_adjoint_kernel"
FLAT_ADJOINT = "fbstab_mpc_adjoint_kernel<64>"
STEP = ("dz", "dl", "dv")

_FAMILIES = {"dense_rows": fx.random_ltv_mpc, "bounds": fx.random_ltv_mpc_bounds,
             "sparse_rows": fx.random_ltv_mpc_sparse_rows}

# (instance, shape, exact or padded, family, seed of the QPs): dense rows are the family of the reference form of
# the costate step, bounds and sparse rows that of the row form (choose_costate_form).  The test puts every case
# through the flat-vector adjoint under the same rule first: a seed on which that yardstick fails is to be
# replaced, not the rule.
_CASES = [
    ("<18,5,10>", (3, 18, 5, 10), "exact", "dense_rows", 7301),
    ("<18,5,10>", (3, 18, 5, 10), "exact", "bounds", 7302),
    ("<18,5,10>", (3, 12, 5, 3), "padded", "dense_rows", 7303),
    ("<18,5,10>", (3, 12, 5, 3), "padded", "sparse_rows", 7304),
    ("<24,8,16>", (3, 24, 8, 16), "exact", "dense_rows", 7305),
    ("<24,8,16>", (3, 24, 8, 16), "exact", "bounds", 7306),
    ("<24,8,16>", (2, 14, 7, 11), "padded", "dense_rows", 7307),
    ("<24,8,16>", (2, 14, 7, 11), "padded", "sparse_rows", 7308),
    ("<24,8,32>", (2, 24, 8, 32), "exact", "dense_rows", 7309),
    ("<24,8,32>", (2, 24, 8, 32), "exact", "bounds", 7310),
    ("<24,8,32>", (3, 22, 3, 17), "padded", "dense_rows", 7311),
    ("<24,8,32>", (3, 22, 3, 17), "padded", "sparse_rows", 7312),
]


@pytest.fixture(scope="module")
def hip():
    from fbstab_amd import hip_api
    assert hip_api.load_library().fbstab_hip_device_count() >= 1
    return hip_api


def _flat_handle(hip, monkeypatch, p, max_batch=None):
    """A fresh handle of p's shape that runs the flat-vector adjoint (the knob is read at creation)."""
    monkeypatch.setenv(FLAT, "1")
    h = hip.FBstabMpcBatch(*p.sizes(), max_batch=max_batch or p.batch)
    monkeypatch.setenv(FLAT, "0")
    assert h.adjoint_kernel_name() == FLAT_ADJOINT
    return h


def test_the_knob_and_the_defaults(hip, monkeypatch):
    """FBSTAB_HIP_FLAT_ADJOINT, read at handle creation: unset, a one-row handle runs its record adjoint and a
    row-pair handle the flat-vector adjoint; 0 selects the record adjoint on both, 1 the flat-vector one on both;
    a flat-vector handle runs the flat-vector adjoint whatever it says."""
    name = lambda shape: hip.FBstabMpcBatch(*shape, max_batch=2).adjoint_kernel_name()
    one_row, row_pair, generic = (3, 12, 4, 20), (3, 18, 5, 10), (3, 30, 8, 40)
    assert hip.FBstabMpcBatch(*generic, max_batch=2).kernel_name() == "fbstab_mpc_kernel<64>"
    monkeypatch.delenv(FLAT, raising=False)
    assert name(one_row) == RECORD_ADJOINT + "<12,4,20>" and name(row_pair) == FLAT_ADJOINT and name(generic) == FLAT_ADJOINT
    monkeypatch.setenv(FLAT, "0")
    assert name(one_row) == RECORD_ADJOINT + "<12,4,20>" and name(row_pair) == RECORD_ADJOINT + "<18,5,10>"
    assert name(generic) == FLAT_ADJOINT
    monkeypatch.setenv(FLAT, "1")
    assert name(one_row) == FLAT_ADJOINT and name(row_pair) == FLAT_ADJOINT and name(generic) == FLAT_ADJOINT


@pytest.mark.parametrize("case", _CASES, ids=["%s-%s-%s" % (c[0], c[2], c[3]) for c in _CASES])
def test_record_adjoint_against_the_oracle_and_the_flat_adjoint(hip, oracle, monkeypatch, case):
    """Every row-pair adjoint kernel (padded and exact are code objects of their own) in both costate forms: the
    handle names the record kernel, all solves end in SUCCESS, the flat-vector adjoint of the same QPs passes the
    rule (the yardstick), the record adjoint passes it, and the two are not the same bits - the record kernel
    ran, not the flat one under another name."""
    inst, shape, _, family, seed = case
    monkeypatch.setenv(FLAT, "0")
    p = _FAMILIES[family](np.random.default_rng(seed), 3, *shape)
    s, x, out = H.cold_solve(hip, p)
    assert s.kernel_name() == "fbstab_mpc_r32_kernel" + inst
    assert s.adjoint_kernel_name().startswith(RECORD_ADJOINT)
    assert (out["eflag"] == 0).all(), out["eflag"]
    seeds = LR.random_seeds(np.random.default_rng(seed + 1000), p)
    flat = _flat_handle(hip, monkeypatch, p).Adjoint(p.arrays, *x, *seeds, adj=True)
    LR.check_mpc_batch(oracle, p, x, seeds, flat)
    res = s.Adjoint(p.arrays, *x, *seeds, adj=True)
    LR.check_mpc_batch(oracle, p, x, seeds, res)
    assert not all(np.array_equal(res[k], flat[k]) for k in STEP)


@pytest.mark.parametrize("inst,shape", [("<18,5,10>", (5, 16, 5, 9)), ("<24,8,16>", (4, 20, 6, 16))])
def test_both_qps_of_a_wavefront_refetch_and_queue_invariance(hip, oracle, monkeypatch, inst, shape):
    """24 QPs on two workgroups (both row pairs of each wavefront busy, every pair re-fetching: four row pairs
    for 24 QPs, so at least six of them sat in second row pairs wherever the queue put them), on the whole grid
    (one QP per wavefront) and QPs 0, 7, 23 alone: the 12 gradients and (dz, dl, dv) are the same bits.  All 24
    QPs of the packed run pass the rule against the oracle."""
    monkeypatch.setenv(FLAT, "0")
    p = fx.random_ltv_mpc(np.random.default_rng(5200 + shape[1]), 24, *shape)
    s, x, out = H.cold_solve(hip, p)
    assert s.kernel_name() == "fbstab_mpc_r32_kernel" + inst
    assert s.adjoint_kernel_name().startswith(RECORD_ADJOINT)
    seeds = LR.random_seeds(np.random.default_rng(10), p)
    full = s.Adjoint(p.arrays, *x, *seeds, adj=True)
    monkeypatch.setenv(CAP, "2")
    packed_h = hip.FBstabMpcBatch(*p.sizes(), max_batch=p.batch)
    assert packed_h.query()["workgroups"] == 2
    assert packed_h.adjoint_kernel_name().startswith(RECORD_ADJOINT)
    packed = packed_h.Adjoint(p.arrays, *x, *seeds, adj=True)
    monkeypatch.delenv(CAP)
    alone_h = hip.FBstabMpcBatch(*p.sizes(), max_batch=1)
    for q in (0, 7, 23):
        one = {k: np.ascontiguousarray(a[q:q + 1]) for k, a in p.arrays.items()}
        alone = alone_h.Adjoint(one, *(t[q:q + 1] for t in x), *(t[q:q + 1] for t in seeds), adj=True)
        for k in MPC_SEQ + STEP:
            assert np.array_equal(alone[k][0], full[k][q]), (q, k)
    for k in MPC_SEQ + STEP:
        assert np.array_equal(packed[k], full[k]), k
    assert (out["eflag"] == 0).all(), out["eflag"]
    LR.check_mpc_batch(oracle, p, x, seeds, packed)


@pytest.mark.parametrize("cap", [None, "1"], ids=["one_qp_per_wavefront", "one_wavefront"])
@pytest.mark.parametrize("inst,shape", [("<18,5,10>", (3, 18, 5, 10)), ("<24,8,16>", (3, 14, 7, 11))])
def test_failed_factorisation_is_reported_through_status(hip, monkeypatch, inst, shape, cap):
    """tests/test_gpu_dense_adjoint.py's construction on the row-pair kernels (exact and padded): a NaN in Q[0] of QP
    1 is a NaN on the diagonal of K at stage 0, which no pivot test accepts - an arithmetic outcome, not a fault:
    status 1, zero gradients and a zero adjoint for that QP (the contraction's ok == false branch), and the other
    two QPs bitwise what they are without it.  On ONE workgroup QPs 0 and 1 share a wavefront - one row pair leaves
    the step early while the other carries on - and QP 2 is fetched after the failure."""
    monkeypatch.setenv(FLAT, "0")
    ref = fx.random_ltv_mpc(np.random.default_rng(5400 + shape[1]), 3, *shape)
    s0, x, out = H.cold_solve(hip, ref)
    assert s0.kernel_name() == "fbstab_mpc_r32_kernel" + inst and (out["eflag"] == 0).all()
    bad = fx.MpcProblem(ref.N, ref.nx, ref.nu, ref.nc, {k: a.copy() for k, a in ref.arrays.items()})
    bad.arrays["Q"][1, 0] = np.nan
    if cap:
        monkeypatch.setenv(CAP, cap)
    s = hip.FBstabMpcBatch(*ref.sizes(), max_batch=3)
    if cap:
        monkeypatch.delenv(CAP)
        assert s.query()["workgroups"] == 1
    assert s.adjoint_kernel_name().startswith(RECORD_ADJOINT)
    seeds = LR.random_seeds(np.random.default_rng(14), ref)
    res = s.Adjoint(bad.arrays, *x, *seeds, adj=True)
    good = s.Adjoint(ref.arrays, *x, *seeds, adj=True)
    assert res["status"].tolist() == [0, 1, 0] and good["status"].tolist() == [0, 0, 0]
    for k in MPC_SEQ + STEP:
        assert np.array_equal(res[k][1], np.zeros_like(res[k][1])), k
        assert np.array_equal(res[k][[0, 2]], good[k][[0, 2]]) and np.abs(good[k][1]).max() > 0, k


def test_kept_matrices_are_rebuilt_after_an_adjoint(hip, monkeypatch):
    """The record adjoint leaves its flat step in the slots' matrix copies: a FBSTAB_HIP_KEEP_MATRICES solve after
    it builds them again - its (z, l, v) and SolverOut are bitwise those of the KEEP solve before the adjoint and
    of a handle that never ran one."""
    import torch
    monkeypatch.setenv(FLAT, "0")
    dev = torch.device("cuda:0")
    p = fx.random_ltv_mpc(np.random.default_rng(5301), 6, 4, 18, 5, 10)
    data = {k: torch.from_numpy(a).to(dev) for k, a in p.arrays.items()}
    seeds = [torch.from_numpy(t).to(dev) for t in LR.random_seeds(np.random.default_rng(11), p)]
    mk = lambda n: torch.zeros((p.batch, n), dtype=torch.float64, device=dev)

    def keep_solve(s):
        z, l, v, y = mk(p.nz), mk(p.nl), mk(p.nv), mk(p.nv)
        out = hip.out_to_numpy(s.Solve(data, z, l, v, y, keep_matrices=True))
        torch.cuda.synchronize()
        return (z, l, v), out

    def same(a, b):
        assert all(torch.equal(s, t) for s, t in zip(a[0], b[0]))
        for f in ("eflag", "residual", "newton_iters", "prox_iters", "initial_residual"):
            assert np.array_equal(a[1][f], b[1][f]), f

    s = hip.FBstabMpcBatch(*p.sizes(), max_batch=p.batch)
    assert s.kernel_name() == "fbstab_mpc_r32_kernel<18,5,10>"
    assert s.adjoint_kernel_name().startswith(RECORD_ADJOINT)
    first = keep_solve(s)
    assert (first[1]["eflag"] == 0).all()
    g = s.Adjoint(data, *first[0], *seeds)
    torch.cuda.synchronize()
    assert (g["status"] == 0).all()
    second = keep_solve(s)
    same(second, first)
    plain = hip.FBstabMpcBatch(*p.sizes(), max_batch=p.batch)
    keep_solve(plain)
    same(second, keep_solve(plain))


def test_autograd_on_a_wide_shape_matches_the_c_abi_and_zeroes_unsolved_qps(hip, monkeypatch):
    """tests/test_gpu_adjoint.py's autograd test at (4, 18, 5, 10), the record adjoint of <18,5,10> behind
    backward(): the gradients equal the C-ABI call's bitwise, and the QP made primal infeasible gets zeros."""
    import torch
    from fbstab_amd.autograd import solve_mpc
    monkeypatch.setenv(FLAT, "0")
    dev = torch.device("cuda:0")
    N, nx, nu, nc = 4, 18, 5, 10
    p = fx.random_ltv_mpc(np.random.default_rng(6061), 4, N, nx, nu, nc)
    # QP 1: u_0(0) <= -1 and u_0(0) >= 1 on stage 0's first two rows
    for r, sgn in ((0, 1.0), (1, -1.0)):
        p.arrays["E"][1, r:(N + 1) * nc * nx:nc][:nx] = 0.0
        for j in range(nu):
            p.arrays["L"][1, r + j * nc] = sgn if j == 0 else 0.0
        p.arrays["d"][1, r] = 1.0
    solver = hip.FBstabMpcBatch(N, nx, nu, nc, max_batch=p.batch)
    assert solver.adjoint_kernel_name().startswith(RECORD_ADJOINT)
    want = ("Q", "q", "A", "E", "d", "x0")
    data = {k: torch.from_numpy(v.copy()).to(dev).requires_grad_(k in want) for k, v in p.arrays.items()}
    z, l, v, out = solve_mpc(solver, data)
    eflag = hip.out_to_numpy(out)["eflag"]
    assert eflag[1] != 0 and (np.delete(eflag, 1) == 0).all(), eflag
    a, b, c = (torch.from_numpy(t).to(dev) for t in LR.random_seeds(np.random.default_rng(13), p))
    loss = (a * z).sum() + (b * l).sum() + (c * v).sum()
    loss.backward()
    ref = solver.Adjoint({k: t.detach() for k, t in data.items()}, z.detach(), l.detach(), v.detach(), a, b, c)
    torch.cuda.synchronize()
    for k in MPC_SEQ:
        if k not in want:
            assert data[k].grad is None, k
            continue
        g = data[k].grad.cpu().numpy()
        r = ref[k].cpu().numpy()
        assert np.array_equal(g[[0, 2, 3]], r[[0, 2, 3]]), k
        assert np.array_equal(g[1], np.zeros_like(g[1])), k
        assert np.abs(r[[0, 2, 3]]).max() > 0, k
