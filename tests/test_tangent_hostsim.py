"""CPU-only checks of the forward mode (fbstab_hip_mpc_tangent_batch, fbstab_hip_dense_tangent_batch): the export
and the argument validation of the C-ABI without a GPU, the direction arithmetic of fb_tangent.h compiled
single-threaded for the host (tests/hostsim/tangent.cc) against the numpy reference, and the whole tangent - host
direction, then the host adjoint - against the oracle's linear solver, central differences of the oracle's solves
and the adjoint's gradients."""
import ctypes as C

import numpy as np
import pytest

from fbstab_amd.hip_api import MPC_SEQ, DENSE_ARR
from oracle.oracle_py import default_options
from tools import fixtures as fx
from tests import helpers as H
from tests import linear_reference as LR
from tests import tangent_helpers as TH
from tests.hostsim import HostAdjoint, HostTangent

MPC_SHAPES = [(1, 2, 1, 1), (2, 3, 2, 4), (3, 12, 4, 20), (2, 34, 3, 5)]
DENSE_SHAPES = [(5, 2, 9), (30, 0, 40)]


@pytest.fixture(scope="module")
def host():
    return HostTangent()


# -- export and validation --------------------------------------------------------------------------------------
def _blocks(hip_api, kind):
    buf = np.zeros(64)
    data_t = hip_api._MpcBatch if kind == "mpc" else hip_api._DenseBatch
    n = len(data_t().base)
    data, ddata, x, dx = data_t(), data_t(), hip_api._VarBatch(), hip_api._VarBatch()
    for i in range(n):
        data.base[i], data.stride[i] = buf.ctypes.data, 8
        ddata.base[i], ddata.stride[i] = buf.ctypes.data, 8
    for i in range(3):
        x.base[i], x.stride[i] = buf.ctypes.data, 8
        dx.base[i], dx.stride[i] = buf.ctypes.data, 8
    return buf, dict(data=data, x=x, ddata=ddata, dx=dx)


@pytest.mark.parametrize("kind", ["mpc", "dense"])
def test_tangent_entry_points_are_exported_and_validate_without_gpu(kind):
    """Both symbols are in the library and in EXPORTED_SYMBOLS; a NULL handle, a NULL x and a NULL dx are each
    FBSTAB_HIP_ERR_ARGUMENT (no handle exists without a device, so the handle is NULL in all three; the dense
    entry point looks at its argument blocks first, the MPC one at the handle)."""
    from fbstab_amd import hip_api
    lib = hip_api.load_library()
    name = f"fbstab_hip_{kind}_tangent_batch"
    assert name in hip_api.EXPORTED_SYMBOLS
    fn = getattr(lib, name)
    buf, b = _blocks(hip_api, kind)
    st = np.zeros(2, dtype=np.int32)

    def call(null=(), batch=1):
        ref = lambda k: None if k in null else C.byref(b[k])
        rc = fn(None, batch, ref("data"), ref("x"), ref("ddata"), 0.0, ref("dx"), None, st.ctypes.data, 0, None)
        return rc, lib.fbstab_hip_last_error().decode()

    assert call() == (1, "null solver handle")
    assert call(batch=2) == (1, "null solver handle")
    rc, msg = call(null=("x",))
    assert rc == 1 and msg == ("null argument" if kind == "dense" else "null solver handle")
    rc, msg = call(null=("dx",))
    assert rc == 1 and msg == ("null argument" if kind == "dense" else "null solver handle")
    assert fn(None, 1, None, None, None, 0.0, None, None, None, 0, None) == 1


# -- the direction arithmetic -----------------------------------------------------------------------------------
def _mpc_shape_problem(shape):
    N, nx, nu, nc = shape
    lens = fx.MpcProblem(N, nx, nu, nc, {}).seq_lengths()
    return fx.MpcProblem(N, nx, nu, nc, {k: np.zeros((1, n)) for k, n in lens.items()})


def _dense_shape_problem(shape):
    p = fx.DenseProblem(*shape)
    p.arrays = {k: np.zeros((1, n)) for k, n in LR.lengths_of(p).items()}
    return p


def _cases(rng, p):
    """(label, perturbations): every array alone, all together (the matrices not symmetric), half of the slots
    null, and none."""
    names = [k for k in LR.names_of(p) if LR.lengths_of(p)[k] > 0]
    every = {k: a[0] for k, a in TH.random_directions(rng, p, 1, names).items()}
    out = [("only " + k, {k: every[k]}) for k in names]
    out.append(("all", every))
    out.append(("null slots", {k: (every[k] if i % 2 else None) for i, k in enumerate(names)}))
    out.append(("other null slots", {k: (None if i % 2 else every[k]) for i, k in enumerate(names)}))
    out.append(("nothing", {}))
    return out


@pytest.mark.parametrize("shape", MPC_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_mpc_direction_arithmetic_meets_the_rounding_bound(host, shape):
    """mpc_tangent_stage on the host, at a random point: every entry of (gz, gl, gv) within (T + 4) 2^-53 S of the
    longdouble reference, for each sequence perturbed alone, all together, with null slots and with
    non-symmetric dQ / dR (every random matrix direction is)."""
    p = _mpc_shape_problem(shape)
    rng = np.random.default_rng(sum(shape))
    x = (rng.standard_normal(p.nz), rng.standard_normal(p.nl), rng.standard_normal(p.nv))
    worst = 0.0
    for label, d in _cases(rng, p):
        got = host.rhs(p, x, d)
        assert all(np.isfinite(g).all() for g in got), label   # (every entry is written)
        worst = max(worst, TH.assert_rhs(p, 0, x, d, got, label))
        if label == "nothing":
            assert all(not g.any() for g in got)
    Q = rng.standard_normal(p.seq_lengths()["Q"])
    QT = Q.reshape(p.N + 1, p.nx, p.nx).transpose(0, 2, 1).reshape(-1)
    a, b = host.rhs(p, x, {"Q": Q}), host.rhs(p, x, {"Q": np.ascontiguousarray(QT)})
    assert all(np.array_equal(s, t) for s, t in zip(a, b))   # (dQ and dQ' have the same symmetric part)
    print("mpc direction", shape, "worst error / bound %.3f" % worst)


@pytest.mark.parametrize("shape", DENSE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_dense_direction_arithmetic_meets_the_rounding_bound(host, shape):
    """dense_tangent on the host: the same bound, with the images in one block of columns, in blocks of a few
    columns and column by column - and the same bits whatever the block (the chain of additions of every entry
    does not depend on it)."""
    p = _dense_shape_problem(shape)
    nz, nl, nv = shape
    rng = np.random.default_rng(sum(shape))
    x = (rng.standard_normal(nz), rng.standard_normal(nl), rng.standard_normal(nv))
    fixed = sum(n + (n & 1) for n in (nz, nl, nv, nz + nl + nv, nz))
    per_col = nz + nl + nv + 3
    worst = 0.0
    for label, d in _cases(rng, p):
        runs = []
        for cols in (nz, 3, 1):
            runs.append(host.rhs(p, x, d, budget=fixed + per_col * cols))
            assert host.cb == cols
        for r in runs[1:]:
            assert all(np.array_equal(s, t) for s, t in zip(runs[0], r)), label
        worst = max(worst, TH.assert_rhs(p, 0, x, d, runs[0], label))
    print("dense direction", shape, "worst error / bound %.3f" % worst)


# -- end to end on the host -----------------------------------------------------------------------------------
def _strict(p, q, z, v, tol=1e-3):
    _, _, _, _, A, b = H.mpc_explicit(p, q)
    return np.maximum(b - A @ z[q], v[q]).min() >= tol


def _symmetrised(p, d):
    d = dict(d)
    for k, n in (("Q", p.nx), ("R", p.nu)):
        M = d[k].reshape(d[k].shape[0], p.N + 1, n, n)
        d[k] = np.ascontiguousarray(0.5 * (M + M.transpose(0, 1, 3, 2))).reshape(d[k].shape)
    return d


def _duality_gap(p, q, x, gq, rhs, dq, adjoint):
    """|<g, dx> - sum_k <table_k, dtheta_k>| over the sum of the magnitudes of the terms of <g, dx>, in longdouble,
    both steps - dx for the seeds ``rhs``, the adjoint behind the table for the seeds ``gq`` - from
    ``adjoint(seeds)``."""
    LD = np.longdouble
    gg, dx = np.concatenate(gq).astype(LD), np.concatenate(adjoint(rhs)).astype(LD)
    tab = LR.mpc_gradient_table(LR.one_qp(p, q), x, adjoint(gq))
    other = sum(np.asarray(tab[k]).astype(LD) @ dq[k].astype(LD) for k in MPC_SEQ)
    return float(abs(gg @ dx - other) / np.abs(gg * dx).sum())


def test_tangent_end_to_end_on_the_host(host, oracle, oracle_fma):
    """Host direction, then the host adjoint (tests/hostsim/adjoint.cc), on random_ltv_mpc(default_rng(8801), 8, 6,
    4, 2, 6) at the oracle's solutions (abs_tol 1e-11; all 8 QPs strictly complementary at 1e-3), all twelve
    sequences perturbed:
      - the step leaves at most 3 x the oracle's residual of V dx = (gz, -gl, -C.gv) (longdouble);
      - it is within 1e-4 of its largest entry of the central differences (h = 1e-5) of the oracle's solves;
      - <g, dx> agrees with sum_k <gradient_table_k, dtheta_k>, relative to the sum of the magnitudes of the
        terms of <g, dx>, within 10 x the largest disagreement of the same two numbers computed with Oracle()
        and with Oracle(fma=True).  Measured: the oracles 3.57e-9 (so the bar is 3.6e-8, which the GPU tests
        take from tangent_helpers.DUALITY_BAR), the host logic 1.10e-9; central differences 1.88e-6."""
    rng = np.random.default_rng(8801)
    p = fx.random_ltv_mpc(rng, 8, 6, 4, 2, 6)
    opts = default_options(abs_tol=1e-11)
    z, l, v, _, out = oracle.solve_mpc(p, opts=opts)
    assert (out["eflag"] == 0).all()
    assert all(_strict(p, q, z, v) for q in range(p.batch))
    d = _symmetrised(p, TH.random_directions(rng, p, p.batch))
    g = LR.random_seeds(rng, p)
    hadj = HostAdjoint()
    # central differences of the oracle's solves along d
    h = 1e-5
    plus = fx.MpcProblem(*p.sizes(), {k: p.arrays[k] + h * d[k] for k in MPC_SEQ})
    minus = fx.MpcProblem(*p.sizes(), {k: p.arrays[k] - h * d[k] for k in MPC_SEQ})
    sp, sm = oracle.solve_mpc(plus, opts=opts), oracle.solve_mpc(minus, opts=opts)
    assert (sp[4]["eflag"] == 0).all() and (sm[4]["eflag"] == 0).all()
    worst_fd = worst_dual = oracle_dual = 0.0
    for q in range(p.batch):
        x = (z[q], l[q], v[q])
        dq = TH.one_direction(d, q)
        rhs = host.rhs(p, x, dq)
        TH.assert_rhs(p, q, x, dq, rhs)
        st, step, _ = hadj.adjoint(p, q, x, rhs, want=())
        assert st == 0
        ref = LR.oracle_adjoint(oracle, p, q, x, rhs)
        r_dev, r_orc = LR.adjoint_residual(p, q, x, step, rhs), LR.adjoint_residual(p, q, x, ref, rhs)
        assert r_dev <= 3 * r_orc, (q, r_dev, r_orc)
        fd = np.concatenate([(sp[i][q] - sm[i][q]) / (2 * h) for i in range(3)])
        dx = np.concatenate(step)
        err = np.abs(dx - fd).max() / np.abs(dx).max()
        worst_fd = max(worst_fd, err)
        assert err <= 1e-4, (q, err)
        # duality: the two sides with each oracle, then with the host logic
        gq = tuple(t[q] for t in g)
        for orc in (oracle, oracle_fma):
            oracle_dual = max(oracle_dual, _duality_gap(p, q, x, gq, rhs, dq,
                                                        lambda s: LR.oracle_adjoint(orc, p, q, x, s)))
        worst_dual = max(worst_dual, _duality_gap(p, q, x, gq, rhs, dq,
                                                  lambda s: hadj.adjoint(p, q, x, s, want=())[1]))
    print("tangent end to end: central differences %.2e, duality oracles %.2e host %.2e" % (worst_fd, oracle_dual,
                                                                                             worst_dual))
    assert worst_dual <= 10 * oracle_dual, (worst_dual, oracle_dual)


def test_dense_tangent_step_meets_the_residual_rule_on_the_host(host, oracle):
    """The dense twin of the residual rule: host direction, then the host dense adjoint
    (tests/hostsim/dense_adjoint.cc), at the oracle's solutions of four (20, 5, 40) QPs."""
    p = fx.synthetic_dense_batch(4, 20, 5, 40)
    sol = oracle.solve_dense(p)
    assert (sol[4]["eflag"] == 0).all()
    rng = np.random.default_rng(20540)
    d = TH.random_directions(rng, p, p.batch)
    hadj = HostAdjoint("dense")
    for q in range(p.batch):
        x = (sol[0][q], sol[1][q], sol[2][q])
        rhs = host.rhs(p, x, TH.one_direction(d, q))
        st, step, _ = hadj.adjoint(p, q, x, rhs, want=())
        assert st == 0
        ref = LR.oracle_adjoint(oracle, p, q, x, rhs)
        r_dev, r_orc = LR.adjoint_residual(p, q, x, step, rhs), LR.adjoint_residual(p, q, x, ref, rhs)
        assert r_dev <= 3 * r_orc, (q, r_dev, r_orc)
