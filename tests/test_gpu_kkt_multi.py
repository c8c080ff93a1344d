"""GPU tests of the many-right-hand-side solves (fbstab_hip_mpc_kkt_solve_batch, fbstab_hip_mpc_x0_sensitivity_batch;
FBstabMpcBatch.KktSolve / X0Sensitivity, fbstab_amd.autograd.mpc_x0_sensitivity): every right-hand side against the
oracle's linear solver on one shape per solve kernel and on a stage beyond the LDS, a record handle left as it was,
bitwise invariance under the queue, the batch and the order of the right-hand sides, the x0 mode against the tangent
and the LQR gain, statuses and placement."""
import numpy as np
import pytest

from fbstab_amd.hip_api import MPC_SEQ
from tools import fixtures as fx
from oracle.oracle_py import default_options
from tests import helpers as H
from tests import linear_reference as LR
from tests import tangent_helpers as TH
from tests import kkt_multi_helpers as KH
from tests.kkt_multi_helpers import STEP
from tests.shapes import MPC_SHAPES

pytestmark = pytest.mark.gpu

CAP = "FBSTAB_HIP_MAX_WORKGROUPS"
FLAT = "FBSTAB_HIP_FLAT_ADJOINT"
GENERIC = "fbstab_mpc_kernel<64>"
WGLOBAL = (2, 53, 1, 1)
B, K = 3, 3


@pytest.fixture(scope="module")
def hip():
    from fbstab_amd import hip_api
    assert hip_api.load_library().fbstab_hip_device_count() >= 1
    return hip_api


def _arrays(p):
    return {k: np.ascontiguousarray(a) for k, a in p.arrays.items()}


def _check_against_the_oracle(oracle, p, x, seeds, res):
    """LR.check_mpc_batch on every right-hand side: status 0, the residual within 3 x the oracle's, the step within
    its forward error, (C, mus) those of the oracle.  (These calls return no gradients: the table rows of the rule
    are given the table of the returned step.)"""
    assert (res["status"] == 0).all()
    for k in range(seeds[0].shape[1]):
        one = {n: np.ascontiguousarray(res[n][:, k]) for n in STEP}
        one["status"] = res["status"]
        tabs = [LR.mpc_gradient_table(LR.one_qp(p, q), tuple(t[q] for t in x), tuple(one[n][q] for n in STEP))
                for q in range(p.batch)]
        one.update({name: np.stack([t[name] for t in tabs]) for name in MPC_SEQ})
        LR.check_mpc_batch(oracle, p, x, tuple(np.ascontiguousarray(g[:, k]) for g in seeds), one)


_FIRST = [next(i for i, (_, n) in enumerate(MPC_SHAPES) if n == name) for name in dict.fromkeys(n for _, n in MPC_SHAPES)]
_RUNS = [(MPC_SHAPES[i][0], MPC_SHAPES[i][1]) for i in _FIRST] + [(WGLOBAL, "wglobal")]


@pytest.mark.parametrize("shape,kern", _RUNS, ids=[k for _, k in _RUNS])
def test_every_right_hand_side_on_one_shape_per_solve_kernel(hip, oracle, monkeypatch, shape, kern):
    """Three random LTV QPs at the device's solutions, three random seeds each, on the handle of every solve kernel
    and on a stage that does not fit the LDS (the kernel's wglobal instance)."""
    assert len(_RUNS) == 7
    wg = kern == "wglobal"
    monkeypatch.setenv("FBSTAB_HIP_GENERIC", "1" if kern == GENERIC else "0")
    p = fx.random_ltv_mpc(np.random.default_rng(9100 + shape[1]), B, *shape, **(dict(dyn_noise=0.02) if wg else {}))
    s, x, out = H.cold_solve(hip, p)
    assert s.kernel_name() == (GENERIC if wg else kern) and (out["eflag"] == 0).all()
    if wg:
        assert s.query()["lds_bytes"] < 4096
    seeds = KH.random_seed_block(np.random.default_rng(shape[1]), p, K, B)
    res = s.KktSolve(_arrays(p), *x, *seeds)
    assert s.last_kernel_ms() > 0
    assert res["dz"].shape == (B, K, p.nz) and res["dl"].shape == (B, K, p.nl) and res["dv"].shape == (B, K, p.nv)
    _check_against_the_oracle(oracle, p, x, seeds, res)


def test_a_record_handle_is_left_as_it_was(hip, oracle, monkeypatch):
    """A one-row record handle on its record adjoint (FBSTAB_HIP_FLAT_ADJOINT=0): the call runs in a scratch of its
    own, so Adjoint(adj=True) before and after it returns the same bits, and the FBSTAB_HIP_KEEP_MATRICES solve behind
    it - which trusts the matrix copies the KEEP solve in front of it left in the handle's scratch - does too."""
    import torch
    monkeypatch.setenv(FLAT, "0")
    monkeypatch.setenv("FBSTAB_HIP_GENERIC", "0")
    dev = torch.device("cuda:0")
    shape, kern = MPC_SHAPES[1]
    p = fx.random_ltv_mpc(np.random.default_rng(9201), B, *shape)
    s = hip.FBstabMpcBatch(*shape, max_batch=B)
    assert s.kernel_name() == kern and s.adjoint_kernel_name().startswith("fbstab_mpc_r16_adjoint_kernel")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    data = {k: t(a) for k, a in p.arrays.items()}
    mk = lambda n: torch.zeros((B, n), dtype=torch.float64, device=dev)

    def keep_solve():
        z, l, v, y = mk(p.nz), mk(p.nl), mk(p.nv), mk(p.nv)
        out = hip.out_to_numpy(s.Solve(data, z, l, v, y, keep_matrices=True))
        torch.cuda.synchronize()
        return (z, l, v), out

    first = keep_solve()
    assert (first[1]["eflag"] == 0).all()
    x = first[0]
    g1 = LR.random_seeds(np.random.default_rng(5), p)
    before = s.Adjoint(data, *x, *(t(a) for a in g1), adj=True)
    torch.cuda.synchronize()
    again = keep_solve()   # (the record adjoint overwrites the copies: this solve rebuilds them)
    seeds = KH.random_seed_block(np.random.default_rng(6), p, K, B)
    res = s.KktSolve(data, *x, *(t(a) for a in seeds))
    torch.cuda.synchronize()
    assert s.last_kernel_ms() > 0
    behind = keep_solve()
    for a, b in ((again, first), (behind, first)):
        assert all(torch.equal(u, w) for u, w in zip(a[0], b[0]))
        for f in H.OUT_FIELDS:
            assert np.array_equal(a[1][f], b[1][f]), f
    after = s.Adjoint(data, *x, *(t(a) for a in g1), adj=True)
    torch.cuda.synchronize()
    for k in MPC_SEQ + STEP + ("status",):
        assert torch.equal(before[k], after[k]), k
    xs = tuple(a.cpu().numpy() for a in x)
    _check_against_the_oracle(oracle, p, xs, seeds, {k: a.cpu().numpy() for k, a in res.items()})


def test_bits_do_not_depend_on_the_queue_the_batch_or_the_order(hip, monkeypatch):
    """One workgroup (every QP re-fetched by the same wavefront) against the default grid; the batch of three against
    its QPs one at a time; right-hand sides 1 .. K-1 permuted; right-hand side 0 against the K = 1 call."""
    p = fx.random_ltv_mpc(np.random.default_rng(9301), B, 5, 6, 3, 8)
    s, x, out = H.cold_solve(hip, p)
    seeds = KH.random_seed_block(np.random.default_rng(8), p, 4, B)
    full = s.KktSolve(_arrays(p), *x, *seeds)
    assert (full["status"] == 0).all() and np.abs(full["dz"]).max(axis=2).min() > 0
    monkeypatch.setenv(CAP, "1")
    one_wg = hip.FBstabMpcBatch(*p.sizes(), max_batch=B)
    monkeypatch.delenv(CAP)
    assert one_wg.query()["workgroups"] == 1
    queued = one_wg.KktSolve(_arrays(p), *x, *seeds)
    for n in STEP + ("status",):
        assert np.array_equal(queued[n], full[n]), n
    alone_h = hip.FBstabMpcBatch(*p.sizes(), max_batch=1)
    for q in range(B):
        one = {k: np.ascontiguousarray(a[q:q + 1]) for k, a in p.arrays.items()}
        alone = alone_h.KktSolve(one, *(t[q:q + 1] for t in x), *(np.ascontiguousarray(g[q:q + 1]) for g in seeds))
        for n in STEP:
            assert np.array_equal(alone[n][0], full[n][q]), (q, n)
    perm = np.array([0, 3, 1, 2])
    moved = s.KktSolve(_arrays(p), *x, *(np.ascontiguousarray(g[:, perm]) for g in seeds))
    first = s.KktSolve(_arrays(p), *x, *(np.ascontiguousarray(g[:, :1]) for g in seeds))
    for n in STEP:
        assert np.array_equal(moved[n], full[n][:, perm]), n
        assert np.array_equal(first[n][:, 0], full[n][:, 0]), n


@pytest.mark.parametrize("shape", [(5, 6, 3, 8), (4, 13, 2, 6)], ids=["one_row", "row_pair"])
def test_x0_sensitivity_against_the_tangent(hip, oracle, shape):
    """Every column j of X0Sensitivity passes the tangent's own check for the direction x0 = e_j: its right-hand side
    (generated in the kernel: gz = 0, gl = -e_j, gv = 0 - the explicit call with those seeds returns the same bits)
    meets TH.assert_rhs's bound, as the seeds Tangent returns on the point replicated nx-fold do, and its step meets
    the residual rule against the oracle, as Tangent's does, within the forward error of Tangent's."""
    p = fx.random_ltv_mpc(np.random.default_rng(9400 + shape[1]), 2, *shape)
    s, x, out = H.cold_solve(hip, p)
    assert (out["eflag"] == 0).all()
    nx, nu = p.nx, p.nu
    res = s.X0Sensitivity(_arrays(p), *x, want=("dz", "dl", "dv", "gain"))
    assert (res["status"] == 0).all() and res["gain"].shape == (2, nu, nx) and res["dz"].shape == (2, nx, p.nz)
    gseed = KH.x0_seed_block(p)
    explicit = s.KktSolve(_arrays(p), *x, *gseed)
    for n in STEP:
        assert np.array_equal(explicit[n], res[n]), n
    assert np.array_equal(res["gain"], np.transpose(res["dz"][:, :, nx:nx + nu], (0, 2, 1)))
    wide = hip.FBstabMpcBatch(*p.sizes(), max_batch=nx)
    rep = lambda a: np.ascontiguousarray(np.repeat(a, nx, axis=0))
    for q in range(p.batch):
        one = LR.one_qp(p, q)
        xq = tuple(t[q] for t in x)
        tan = wide.Tangent(_arrays(one), *(rep(t[q:q + 1]) for t in x), {"x0": np.eye(nx)}, rhs=True)
        assert (tan["status"] == 0).all()
        for j in range(nx):
            d = {"x0": np.eye(nx)[j]}
            TH.assert_rhs(p, q, xq, d, tuple(g[j] for g in gseed), "generated")
            TH.assert_rhs(p, q, xq, d, tuple(tan[k][j] for k in ("gz", "gl", "gv")), "tangent")
            sj = tuple(g[j] for g in gseed)
            ref = LR.oracle_adjoint(oracle, p, q, xq, sj)
            r_orc = LR.adjoint_residual(p, q, xq, ref, sj)
            col = tuple(res[n][q, j] for n in STEP)
            tcol = tuple(tan[n][j] for n in STEP)
            r_col, r_tan = LR.adjoint_residual(p, q, xq, col, sj), LR.adjoint_residual(p, q, xq, tcol, sj)
            assert r_col <= 3 * r_orc and r_tan <= 3 * r_orc, (q, j, r_col, r_tan, r_orc)
            smax = max(np.abs(np.concatenate(tcol)).max(), 1.0)
            assert np.abs(np.concatenate(col) - np.concatenate(tcol)).max() <= 1e-5 * smax, (q, j)


def test_lqr_gain_from_one_call_on_a_handle_of_one_qp(hip):
    """The known answer of tests/test_gpu_tangent.py (all constraints inactive: du0/dx0 = -K_0 of the Riccati
    recursion), from ONE call on a max_batch = 1 handle; and the gain asked for alone."""
    N, nx, nu, nc = 8, 4, 2, 1
    p = fx.random_ltv_mpc(np.random.default_rng(4401), 1, N, nx, nu, nc)
    for k in ("q", "r", "c"):
        p.arrays[k][:] = 0.0
    p.arrays["E"][:] = 0.0
    p.arrays["L"][:] = 0.0
    p.arrays["d"][:] = -1.0   # 0 <= 1 on every row: inactive, y = 1, v = 0
    Kg = H.lqr_gain(p)
    s, x, out = H.cold_solve(hip, p, default_options(abs_tol=1e-11))
    assert (out["eflag"] == 0).all()
    res = s.X0Sensitivity(_arrays(p), *x)
    assert set(res) == {"dz", "gain", "status"} and (res["status"] == 0).all()
    np.testing.assert_allclose(res["gain"][0], Kg, rtol=1e-6, atol=1e-9 * np.abs(Kg).max())
    alone = s.X0Sensitivity(_arrays(p), *x, want=("gain",))
    assert set(alone) == {"gain", "status"} and np.array_equal(alone["gain"], res["gain"])


def test_mpc_x0_sensitivity_returns_detached_tensors_on_the_device(hip):
    import torch
    from fbstab_amd.autograd import mpc_x0_sensitivity
    dev = torch.device("cuda:0")
    p = fx.random_ltv_mpc(np.random.default_rng(9500), 2, 4, 5, 2, 6)
    s, x, out = H.cold_solve(hip, p)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    data = {k: t(a).requires_grad_(k == "x0") for k, a in p.arrays.items()}
    J = mpc_x0_sensitivity(s, data, *(t(a) for a in x))
    torch.cuda.synchronize()
    host = s.X0Sensitivity(_arrays(p), *x, want=("dz", "dl", "dv", "gain"))
    for k in STEP + ("gain", "status"):
        assert J[k].is_cuda and not J[k].requires_grad and J[k].grad_fn is None, k
        assert np.array_equal(J[k].cpu().numpy(), host[k]), k


def test_statuses_and_placement(hip):
    """A batch of three with QP 1 made indefinite (Q = -100 I on every stage): status [0, 1, 0], every right-hand side
    of QP 1 zero, QPs 0 and 2 the bits of the clean batch.  A host-pointer call returns the bits of the device-pointer
    call; a shared seed block (stride 0) those of its replicated form; rhs_stride = length + 3 leaves the NaN in the
    gaps; batch == 0 returns OK."""
    import torch
    dev = torch.device("cuda:0")
    ref = fx.random_ltv_mpc(np.random.default_rng(9601), B, 4, 5, 2, 6)
    s, x, out = H.cold_solve(hip, ref)
    assert (out["eflag"] == 0).all()
    bad = fx.MpcProblem(ref.N, ref.nx, ref.nu, ref.nc, {k: a.copy() for k, a in ref.arrays.items()})
    bad.arrays["Q"][1] = np.tile(-100.0 * np.eye(ref.nx).reshape(-1), ref.N + 1)
    seeds = KH.random_seed_block(np.random.default_rng(9), ref, K, B)
    good = s.KktSolve(_arrays(ref), *x, *seeds)
    res = s.KktSolve(_arrays(bad), *x, *seeds)
    sens = s.X0Sensitivity(_arrays(bad), *x, want=("dz", "dl", "dv", "gain"))
    assert good["status"].tolist() == [0, 0, 0] and res["status"].tolist() == [0, 1, 0]
    assert sens["status"].tolist() == [0, 1, 0]
    for n in STEP:
        assert np.array_equal(res[n][1], np.zeros_like(res[n][1])), n
        assert np.array_equal(res[n][[0, 2]], good[n][[0, 2]]) and np.abs(good[n][1]).max(axis=1).min() > 0, n
        assert np.array_equal(sens[n][1], np.zeros_like(sens[n][1])) and np.abs(sens[n][[0, 2]]).max() > 0, n
    assert not sens["gain"][1].any() and np.abs(sens["gain"][[0, 2]]).max() > 0
    # device pointers
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    data = {k: t(a) for k, a in ref.arrays.items()}
    on_dev = s.KktSolve(data, *(t(a) for a in x), *(t(a) for a in seeds))
    sens_host = s.X0Sensitivity(_arrays(ref), *x, want=("dz", "dl", "dv", "gain"))
    sens_dev = s.X0Sensitivity(data, *(t(a) for a in x), want=("dz", "dl", "dv", "gain"))
    torch.cuda.synchronize()
    for n in STEP + ("status",):
        assert np.array_equal(on_dev[n].cpu().numpy(), good[n]), n
        assert np.array_equal(sens_dev[n].cpu().numpy(), sens_host[n]), n
    assert np.array_equal(sens_dev["gain"].cpu().numpy(), sens_host["gain"])
    # one block of seeds for the whole batch
    shared = tuple(np.ascontiguousarray(g[1]) for g in seeds)
    copied = tuple(np.ascontiguousarray(np.repeat(g[None], B, axis=0)) for g in shared)
    a, b = s.KktSolve(_arrays(ref), *x, *shared), s.KktSolve(_arrays(ref), *x, *copied)
    a_dev = s.KktSolve(data, *(t(u) for u in x), *(t(u) for u in shared))
    torch.cuda.synchronize()
    for n in STEP:
        assert np.array_equal(a[n], b[n]) and np.array_equal(a_dev[n].cpu().numpy(), b[n]), n
    # vectors three doubles apart, QPs five: what lies between is not written
    lens = (ref.nz, ref.nl, ref.nv)
    pads = [np.full((B, K * (n + 3) + 5), np.nan) for n in lens]
    views = [pd[:, :K * (n + 3)].reshape(B, K, n + 3)[:, :, :n] for pd, n in zip(pads, lens)]
    rc, status = KH.kkt_solve_into(s, _arrays(ref), x, seeds, views)
    assert rc == 0 and status.tolist() == [0, 0, 0]
    for n, pd, vw, ln in zip(STEP, pads, views, lens):
        assert np.array_equal(vw, good[n]), n
        gaps = np.ones(pd.shape, dtype=bool)
        gaps[:, :K * (ln + 3)].reshape(B, K, ln + 3)[:, :, :ln] = False
        assert np.isnan(pd[gaps]).all() and gaps.sum() == B * (3 * K + 5), n
    # an empty batch
    rc, status = KH.kkt_solve_into(s, _arrays(ref), x, seeds, views, batch=0)
    assert rc == 0 and status.size == 0
    none = s.X0Sensitivity({k: a[:0] for k, a in _arrays(ref).items()}, *(a[:0] for a in x))
    assert none["dz"].shape == (0, ref.nx, ref.nz) and none["status"].shape == (0,)
