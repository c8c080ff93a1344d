"""Condensing on the device: fbstab_hip_mpc_condense_batch / fbstab_hip_mpc_expand_batch against the
extended-precision reference of tests/condense_helpers.py within its acceptance rule, the placements of the
C-ABI, determinism, and ``CondensedMpc.Solve`` end to end against ``FBstabMpcBatch.Solve`` and the oracle."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import condense_helpers as ch
from tests.helpers import mpc_explicit, natural_residual_norm

pytestmark = pytest.mark.gpu
MATRICES, VECTORS, ALL = 1, 2, 3
OUT_NAMES = ("H", "f", "A", "b")
OUT_SLOT = dict(H=0, f=1, A=4, b=5)


@pytest.fixture(scope="module")
def hip():
    from fbstab_amd import hip_api
    hip_api.load_library()
    return hip_api


@functools.lru_cache(maxsize=None)
def reference(name):
    """(reference, bound) of every QP of the fixture: computed once, shared by the tests, left unchanged."""
    p = ch.problem(name)
    return [ch.assert_condition(p, q) for q in range(p.batch)]


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def _out_lens(p):
    nzc = (p.N + 1) * p.nu
    return dict(H=nzc * nzc, f=nzc, A=p.nv * nzc, b=p.nv)


def condense_raw(hip, p, what=ALL, pad=0, shared=False, out_stride0=(), qps=None, fill=np.nan):
    """One call of fbstab_hip_mpc_condense_batch on device copies of ``p`` (the QPs ``qps``): (rc, dict name ->
    (rows, len + pad) numpy array as the device left it, pre-filled with ``fill``).  ``shared``: the matrix
    sequences are QP 0's, stride 0; ``out_stride0``: output slots given one image and stride 0."""
    import torch
    lib = hip.load_library()
    qps = list(range(p.batch)) if qps is None else qps
    B = len(qps)
    data = hip._MpcBatch()
    keep = []
    for i, k in enumerate(ch.MPC_NAMES):
        share = shared and k in ch.MATRIX_NAMES
        t = _dev(p.arrays[k][[0] if share else qps])
        keep.append(t)
        data.base[i], data.stride[i] = t.data_ptr(), (0 if share else t.shape[1])
    out = hip._DenseOutBatch()
    bufs = {}
    for k, n in _out_lens(p).items():
        rows = 1 if k in out_stride0 else B
        t = torch.full((rows, n + pad), fill, dtype=torch.float64, device="cuda")
        bufs[k] = t
        out.base[OUT_SLOT[k]], out.stride[OUT_SLOT[k]] = t.data_ptr(), (0 if k in out_stride0 else n + pad)
    rc = lib.fbstab_hip_mpc_condense_batch(*p.sizes(), B, C.byref(data), what, C.byref(out), 0, None)
    torch.cuda.synchronize()
    return rc, {k: t.cpu().numpy() for k, t in bufs.items()}


def _check_rule(p, name, res, qps, names=OUT_NAMES, pad=0):
    lens = _out_lens(p)
    worst = 0.0
    for row, q in enumerate(qps):
        ref, bound = reference(name)[q]
        got = ch.images({k: res[k][min(row, res[k].shape[0] - 1), :lens[k]] for k in OUT_NAMES}, p)
        worst = max(worst, ch.worst_ratio(got, ref, bound, names))
        assert ch.rule_violations(got, ref, bound, names) == [], (name, q)
        if pad:
            for k in names:
                assert np.isnan(res[k][row, lens[k]:]).all(), (k, "the doubles between two images were written")
    print(name, "worst error / bound:", worst)


# ---- 5. ALL against the reference, and the placements -------------------------------------------------------------
@pytest.mark.parametrize("name", ch.SHAPE_NAMES)
def test_condense_all_meets_the_rule(hip, name):
    p = ch.problem(name)
    rc, res = condense_raw(hip, p)
    assert rc == 0, hip.load_library().fbstab_hip_last_error()
    _check_rule(p, name, res, range(p.batch))
    rc, padded = condense_raw(hip, p, pad=3)
    assert rc == 0
    _check_rule(p, name, padded, range(p.batch), pad=3)
    lens = _out_lens(p)
    for k in OUT_NAMES:
        assert padded[k][:, :lens[k]].tobytes() == res[k].tobytes(), k


@pytest.mark.parametrize("name", ["small", "odd33", "double_integrator"])
def test_shared_model_gives_one_image(hip, name):
    p = ch.problem(name)
    rc, one = condense_raw(hip, p, shared=True, out_stride0=("H", "A"))
    assert rc == 0, hip.load_library().fbstab_hip_last_error()
    rc, per_qp = condense_raw(hip, p, shared=True)
    assert rc == 0
    for k in ("H", "A"):
        assert one[k].shape[0] == 1 and one[k][0].tobytes() == per_qp[k][0].tobytes(), k
        assert all(per_qp[k][q].tobytes() == per_qp[k][0].tobytes() for q in range(p.batch))
    for k in ("f", "b"):
        assert one[k].tobytes() == per_qp[k].tobytes(), k
    # QP 0 with its own matrices is the shared model's QP 0
    _check_rule(p, name, {k: one[k] for k in OUT_NAMES}, [0], names=("H", "A"))
    # some matrix sequence per QP and an output stride of 0: refused, nothing written
    rc, res = condense_raw(hip, p, out_stride0=("H", "A"))
    assert rc == 1 and b"stride 0" in hip.load_library().fbstab_hip_last_error()
    assert all(np.isnan(a).all() for a in res.values())
    rc, res = condense_raw(hip, p, shared=True, out_stride0=("f",))
    assert rc == 1


# ---- 6. independence and determinism ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "flat", "four_wave"])
def test_a_qp_does_not_depend_on_its_batch(hip, name):
    p = ch.problem(name)
    rc, res = condense_raw(hip, p)
    rc2, again = condense_raw(hip, p)
    assert rc == 0 and rc2 == 0
    nzc = (p.N + 1) * p.nu
    for k in OUT_NAMES:
        assert res[k].tobytes() == again[k].tobytes(), k
    for q in range(p.batch):
        H = res["H"][q].reshape(nzc, nzc)
        assert np.array_equal(H, H.T)
        rc, alone = condense_raw(hip, p, qps=[q])
        assert rc == 0
        for k in OUT_NAMES:
            assert alone[k][0].tobytes() == res[k][q].tobytes(), (k, q)


# ---- 7. VECTORS and MATRICES ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ch.SHAPE_NAMES)
def test_vectors_are_bitwise_those_of_all(hip, name):
    p = ch.problem(name)
    rc, res = condense_raw(hip, p)
    rcv, vec = condense_raw(hip, p, what=VECTORS)
    rcm, mat = condense_raw(hip, p, what=MATRICES)
    assert rc == 0 and rcv == 0 and rcm == 0
    for k in ("f", "b"):
        assert vec[k].tobytes() == res[k].tobytes(), k
        assert np.isnan(mat[k]).all(), k
    for k in ("H", "A"):
        assert mat[k].tobytes() == res[k].tobytes(), k
        assert np.isnan(vec[k]).all(), k


def test_unselected_slots_may_be_null(hip):
    import torch
    p = ch.problem("small")
    lib = hip.load_library()
    data = hip._MpcBatch()
    keep = [_dev(p.arrays[k]) for k in ch.MPC_NAMES]
    for i, t in enumerate(keep):
        data.base[i], data.stride[i] = t.data_ptr(), t.shape[1]
    lens = _out_lens(p)
    f = torch.full((p.batch, lens["f"]), np.nan, dtype=torch.float64, device="cuda")
    b = torch.full((p.batch, lens["b"]), np.nan, dtype=torch.float64, device="cuda")
    out = hip._DenseOutBatch()
    out.base[1], out.stride[1], out.base[5], out.stride[5] = f.data_ptr(), lens["f"], b.data_ptr(), lens["b"]
    assert lib.fbstab_hip_mpc_condense_batch(*p.sizes(), p.batch, C.byref(data), VECTORS, C.byref(out), 0, None) == 0
    torch.cuda.synchronize()
    rc, res = condense_raw(hip, p)
    assert f.cpu().numpy().tobytes() == res["f"].tobytes() and b.cpu().numpy().tobytes() == res["b"].tobytes()
    assert lib.fbstab_hip_mpc_condense_batch(*p.sizes(), p.batch, C.byref(data), ALL, C.byref(out), 0, None) == 1


# ---- 8. expand ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ch.SHAPE_NAMES)
def test_expand_meets_the_rule(hip, name):
    import torch
    from fbstab_amd.condense import CondensedMpc
    p = ch.problem(name)
    rng = np.random.default_rng(21)
    B, nzc = p.batch, (p.N + 1) * p.nu
    U, v, y = rng.standard_normal((B, nzc)), np.abs(rng.standard_normal((B, p.nv))), rng.standard_normal((B, p.nv))
    s = CondensedMpc(*p.sizes(), max_batch=B)
    z, l, vo, yo = s.Expand(p.arrays, U, v, y)
    assert vo.tobytes() == v.tobytes() and yo.tobytes() == y.tobytes()
    worst = 0.0
    for q in range(B):
        zr, lr, _, _ = ch.expand_reference(p, q, U[q], v[q], y[q])
        zb, lb = ch.expand_bound(p, q, U[q], v[q], y[q])
        ez, el = np.abs(z[q] - zr), np.abs(l[q] - lr)
        worst = max(worst, float((ez / np.where(zb > 0, zb, 1)).max()), float((el / np.where(lb > 0, lb, 1)).max()))
        assert (ez <= zb).all() and (el <= lb).all(), q
    print(name, "worst error / bound:", worst)
    # NULL output slots are skipped: l alone, into a padded array whose pad survives
    d = {k: _dev(a) for k, a in p.arrays.items()}
    lt = torch.full((B, p.nl + 2), np.nan, dtype=torch.float64, device="cuda")
    s._expand(d, _dev(U), _dev(v), None, None, lt[:, :p.nl], None, None)
    torch.cuda.synchronize()
    got = lt.cpu().numpy()
    assert got[:, :p.nl].tobytes() == np.ascontiguousarray(l).tobytes() and np.isnan(got[:, p.nl:]).all()
    zt = torch.full((B, p.nz), np.nan, dtype=torch.float64, device="cuda")
    s._expand(d, _dev(U), _dev(v), None, zt, None, None, None)
    assert zt.cpu().numpy().tobytes() == np.ascontiguousarray(z).tobytes()
    s.close()


# ---- 9. end to end ----------------------------------------------------------------------------------------------------
def _route_gap(za, zb):
    return float(np.abs(za - zb).max() / (1.0 + np.abs(zb).max()))


@pytest.mark.parametrize("name", ["small", "flat", "four_wave", "double_integrator", "servo_motor"])
def test_condensed_solve_end_to_end(hip, name):
    from oracle.oracle_py import Oracle, default_options
    from fbstab_amd.condense import CondensedMpc
    p = ch.problem(name)
    B = p.batch
    data = {k: np.ascontiguousarray(a) for k, a in p.arrays.items()}
    s = CondensedMpc(*p.sizes(), max_batch=B)
    z, l, v, y = (np.zeros((B, n)) for n in (p.nz, p.nl, p.nv, p.nv))
    out = s.Solve(data, z, l, v, y)
    assert (out["eflag"] == 0).all(), out["eflag"]
    for q in range(B):
        nr = natural_residual_norm(*mpc_explicit(p, q), z[q], l[q], v[q])
        print(name, q, "natural residual of the expanded point:", nr)
        assert nr <= 2e-6, (q, nr)
    # warm-started from its own result: at most as many Newton steps
    zw, lw, vw, yw = z.copy(), l.copy(), v.copy(), y.copy()
    warm = s.Solve(data, zw, lw, vw, yw, recondense="none")
    assert (warm["eflag"] == 0).all()
    assert (warm["newton_iters"] <= out["newton_iters"]).all(), (warm["newton_iters"], out["newton_iters"])
    # only x0 moved: "vectors" gives bitwise what "all" gives
    moved = dict(data, x0=data["x0"] * 0.9)
    ra = [np.zeros((B, n)) for n in (p.nz, p.nl, p.nv, p.nv)]
    rv = [np.zeros((B, n)) for n in (p.nz, p.nl, p.nv, p.nv)]
    oa = s.Solve(moved, *ra, recondense="all")
    s.Solve(data, *[np.zeros((B, n)) for n in (p.nz, p.nl, p.nv, p.nv)], recondense="all")
    ov = s.Solve(moved, *rv, recondense="vectors")
    for a, b in zip(ra, rv):
        assert a.tobytes() == b.tobytes()
    assert np.array_equal(oa["newton_iters"], ov["newton_iters"]) and np.array_equal(oa["eflag"], ov["eflag"])
    s.close()
    # the MPC solver on the same QPs, and the distance of the two routes against the oracle's own
    m = hip.FBstabMpcBatch(*p.sizes(), max_batch=B)
    zm, lm, vm, ym = (np.zeros((B, n)) for n in (p.nz, p.nl, p.nv, p.nv))
    om = m.Solve(data, zm, lm, vm, ym)
    m.close()
    assert (om["eflag"] == 0).all(), om["eflag"]
    orc = Oracle()
    o = default_options()
    zo, _, _, _, oo = orc.solve_mpc(p, opts=o)
    zc, _, vc, yc, oc = orc.solve_dense(ch.condensed_problem(p), opts=o)
    assert (oo["eflag"] == 0).all() and (oc["eflag"] == 0).all()
    zoc = np.stack([ch.expand_reference(p, q, zc[q], vc[q], yc[q])[0].astype(np.float64) for q in range(B)])
    gap_oracle, gap_device = _route_gap(zoc, zo), _route_gap(z, zm)
    print(name, "max|z - z_mpc| / (1 + max|z_mpc|): device", gap_device, "oracle's two routes", gap_oracle)
    assert gap_device < 10 * gap_oracle


# ---- above 64 KB of LDS the kernels need their attribute set -------------------------------------------------------
def test_shape_above_64_kb_of_lds(hip):
    from fbstab_amd.condense import CondensedMpc, condensed_sizes
    from tools import fixtures as fx
    sizes = (2, 64, 2, 2)
    assert 64 * 1024 < condensed_sizes(*sizes)["lds_bytes"] <= 160 * 1024
    p = fx.random_ltv_mpc(np.random.default_rng(31), 2, *sizes, dyn_noise=0.05)
    rc, res = condense_raw(hip, p)
    assert rc == 0, hip.load_library().fbstab_hip_last_error()
    lens = _out_lens(p)
    rng = np.random.default_rng(32)
    U, v, y = rng.standard_normal((2, 6)), np.abs(rng.standard_normal((2, p.nv))), rng.standard_normal((2, p.nv))
    s = CondensedMpc(*sizes, max_batch=2)
    z, l, _, _ = s.Expand(p.arrays, U, v, y)
    s.close()
    for q in range(2):
        ref, bound = ch.assert_condition(p, q)
        got = ch.images({k: res[k][q, :lens[k]] for k in OUT_NAMES}, p)
        assert ch.rule_violations(got, ref, bound) == [], q
        zr, lr, _, _ = ch.expand_reference(p, q, U[q], v[q], y[q])
        zb, lb = ch.expand_bound(p, q, U[q], v[q], y[q])
        assert (np.abs(z[q] - zr) <= zb).all() and (np.abs(l[q] - lr) <= lb).all(), q
