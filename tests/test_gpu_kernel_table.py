"""GPU checks of the cells of the handles' kernel tables (fbstab_hip.hip: mpc_resolve_kernels,
dense_resolve_kernels) that no other test file launches: the adjoint and the traced solve of an MPC handle whose
stage does not fit the LDS, the batch and traced solves of a FBSTAB_HIP_DENSE_THREADS=64 handle, and the traced
solve on every dense layout (the four-wavefront kernel's own, K in global scratch, the iterate vectors there too).
Every case creates a handle with max_batch = 3, runs 3 QPs and holds the result to the bar the neighbouring test
of that operation uses; the shapes are the smallest that select the variant."""
import numpy as np
import pytest

from oracle.oracle_py import default_options
from tests import helpers as H
from tests import linear_reference as LR
from tests.hostsim import HostAdjoint
from tools import fixtures as fx

pytestmark = pytest.mark.gpu

B = 3
LDS = 160 * 1024
THREADS = "FBSTAB_HIP_DENSE_THREADS"

# MpcLayout::init (fb_mpc.h) carves seven stage matrices, twelve work matrices and two dozen vectors out of the LDS.
# A host program over it with N = 2 and nu = nc = 1 (the cheapest stage): 160 384 bytes at nx = 52, 166 432 at
# nx = 53 - the first past the 163 840 of the LDS.  From there on a launch asks for the reduction scratch and one
# stage's output slice alone (1 088 bytes).
WGLOBAL = (2, 53, 1, 1)

# DenseLayout::init (fb_dense.h), nthreads = 256, by the same kind of host program.  K is (nz + nl)^2 doubles of the
# LDS beside ten vectors of nz, six of nl and eight of nv: with nl = nv = 4 the carve is 162 464 bytes at nz = 135
# and would be 164 752 at nz = 136, where K (156 800 bytes) moves to global scratch.  At (140, 0) with K there the
# vectors take 163 792 bytes at nv = 2439 and would take 163 856 at nv = 2440, where they follow K.
K_GLOBAL = (136, 4, 4)
V_GLOBAL = (140, 0, 2440)
# (the v_global shape: as tests/test_gpu_dense_adjoint.py, every row from RELAX_FROM on is relaxed by RELAX - the
# generator's quarter of active rows is 610 on 140 variables, a degenerate vertex no two roundings walk to alike)
RELAX_FROM, RELAX = 40, 10.0


@pytest.fixture(scope="module")
def hip():
    from fbstab_amd import hip_api
    assert hip_api.load_library().fbstab_hip_device_count() >= 1
    return hip_api


def _arrays(p):
    return {k: np.ascontiguousarray(a) for k, a in p.arrays.items()}


def _one_dense(p, q):
    one = fx.DenseProblem(p.nz, p.nl, p.nv)
    one.arrays = {k: np.ascontiguousarray(a[q:q + 1]) for k, a in p.arrays.items()}
    return one


def _solve_batch(s, p):
    z, l, v, y = (np.zeros((p.batch, n)) for n in (p.nz, p.nl, p.nv, p.nv))
    out = s.Solve(_arrays(p), z, l, v, y)
    return (z, l, v, y), out


def _assert_parity(x, out, ref, o):
    """The bar of tests/test_gpu_components.py::test_random_shapes_on_every_dense_kernel."""
    oc = ref[4]
    assert np.array_equal(out["eflag"], oc["eflag"]) and (oc["eflag"] == 0).all()
    assert np.array_equal(out["prox_iters"], oc["prox_iters"])
    dn = np.abs(out["newton_iters"].astype(int) - oc["newton_iters"].astype(int))
    assert dn.max() <= 2, dn
    scale = 1.0 + np.abs(ref[0]).max(axis=1, keepdims=True)
    assert (np.abs(x[0] - ref[0]) <= 10 * o.abs_tol * scale).all()


def _assert_traces(oracle, s, p, one_qp, x, qps=range(B)):
    """QPs of the batch through the handle's traced solve, one call each: the records are the oracle's (the bar
    of tests/test_display.py), the FINAL record says SUCCESS, and the point is the batch call's."""
    for q in qps:
        one = one_qp(p, q)
        ref = oracle.solve_display(one, opts=default_options())
        z, l, v, y = (np.zeros((1, n)) for n in (p.nz, p.nl, p.nv, p.nv))
        out, rec = s.SolveTraced(_arrays(one), z, l, v, y)
        assert out["eflag"][0] == ref[4]["eflag"][0] == 0
        assert out["prox_iters"][0] == ref[4]["prox_iters"][0]
        H.records_agree(rec, ref[6], (p.nz, p.nl, p.nv, q))
        assert rec[-1, 0] == 5 and rec[-1, 1] == 0
        assert np.abs(z[0] - x[0][q]).max() <= 1e-5 * (1 + np.abs(x[0][q]).max())


def test_adjoint_and_traced_solve_of_a_stage_that_does_not_fit_the_lds(hip, oracle):
    """WGLOBAL - and not (2, 52, 1, 1) - runs the flat-vector kernels with the stage in global scratch: the adjoint
    (fbstab_mpc_adjoint_kernel<64, true>) by the rule of tests/test_gpu_adjoint.py, the traced solve
    (fbstab_mpc_kernel<64, false, true, true>) by that of tests/test_display.py."""
    N, nx, nu, nc = WGLOBAL
    below = hip.FBstabMpcBatch(N, nx - 1, nu, nc, max_batch=B)
    assert below.kernel_name() == "fbstab_mpc_kernel<64>" and 150 * 1024 < below.query()["lds_bytes"] <= LDS
    below.close()
    # (dynamics I + 0.02 randn, as tests/test_gpu_components.py::test_mpc_stage_wider_than_the_lds)
    p = fx.random_ltv_mpc(np.random.default_rng(5300), B, N, nx, nu, nc, dyn_noise=0.02)
    s = hip.FBstabMpcBatch(N, nx, nu, nc, max_batch=B)
    assert s.kernel_name() == "fbstab_mpc_kernel<64>" and s.adjoint_kernel_name() == "fbstab_mpc_adjoint_kernel<64>"
    assert s.sweep_adjoint_kernel_name() == "fbstab_sweep_costate_kernel"
    assert s.query()["lds_bytes"] < 4096
    x, out = _solve_batch(s, p)
    assert (out["eflag"] == 0).all()
    seeds = LR.random_seeds(np.random.default_rng(53), p)
    res = s.Adjoint(p.arrays, *x[:3], *seeds, adj=True)
    LR.check_mpc_batch(oracle, p, x[:3], seeds, res)
    _assert_traces(oracle, s, p, LR.one_qp, x)
    s.close()


@pytest.mark.parametrize("threads", ["64", "256"])
def test_batch_and_traced_solves_of_the_four_wavefront_policy_with_k_in_lds(hip, oracle, monkeypatch, threads):
    """(20, 5, 40) with FBSTAB_HIP_DENSE_THREADS: the batch on fbstab_dense_kernel<64> / <256>, the traced solve on
    fbstab_dense_kernel<256, true> with a layout of its own - at 64 threads not the handle's."""
    nz, nl, nv = 20, 5, 40
    monkeypatch.setenv(THREADS, threads)
    p = fx.synthetic_dense_batch(B, nz, nl, nv, first_id=640)
    s = hip.FBstabDenseBatch(nz, nl, nv, max_batch=B)
    assert s.query()["threads"] == int(threads)
    o = default_options()
    x, out = _solve_batch(s, p)
    _assert_parity(x, out, oracle.solve_dense(p, opts=o, nthreads=oracle.num_threads()), o)
    _assert_traces(oracle, s, p, _one_dense, x)
    s.close()


@pytest.mark.parametrize("shape,flags", [(K_GLOBAL, (1, 0)), (V_GLOBAL, (1, 1))], ids=["k_global", "v_global"])
def test_traced_solve_with_k_and_the_vectors_in_global_scratch(hip, oracle, shape, flags):
    """The smallest shapes for which DenseLayout::init moves K, and K and the iterate vectors, out of the LDS: the
    traced solve runs fbstab_dense_kernel<256, true, true[, true]> on the handle's layout and scratch, and the probe
    is refused (K must fit the LDS).  (v_global: the batch call solves the three QPs, the traced one QP 0 alone -
    one workgroup with everything in global memory: tracing all three made the case 6 s.)"""
    nz, nl, nv = shape
    layout = HostAdjoint("dense").layout
    assert (layout(nz, nl, nv)["k_global"], layout(nz, nl, nv)["v_global"]) == flags
    smaller = layout(nz, nl, nv - 1) if flags[1] else layout(nz - 1, nl, nv)
    assert (smaller["k_global"], smaller["v_global"]) != flags
    p = fx.synthetic_dense_batch(B, nz, nl, nv, first_id=1400)
    if flags[1]:
        p.arrays["b"] = p.arrays["b"].copy()
        p.arrays["b"][:, RELAX_FROM:] += RELAX
    s = hip.FBstabDenseBatch(nz, nl, nv, max_batch=B)
    q = s.query()
    assert q["threads"] == 256 and q["scratch_bytes"] >= (nz + nl) ** 2 * 8 * B
    o = default_options()
    x, out = _solve_batch(s, p)
    _assert_parity(x, out, oracle.solve_dense(p, opts=o, nthreads=oracle.num_threads()), o)
    _assert_traces(oracle, s, p, _one_dense, x, qps=range(1 if flags[1] else B))
    zero = lambda n: np.zeros(n)
    with pytest.raises(hip.FBstabHipError, match="K must fit the LDS"):
        s.debug_newton({k: a[0] for k, a in p.arrays.items()}, zero(nz), zero(nl), zero(nv), zero(nz), zero(nl), zero(nv))
    s.close()
