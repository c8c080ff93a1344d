"""Closed-loop sweeps of the condensed route on the device: the affine map of x0 against the extended-precision
reference within the existing acceptance rule, RECONDENSE mode against a loop over the public calls bit for bit,
AFFINE mode against the reference closed loop of tests/condense_sweep_helpers.py, independence of the grouping, and
the placements of ``CondensedMpc.RecedingSweep``."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import condense_helpers as ch
from tests import condense_sweep_helpers as sh

pytestmark = pytest.mark.gpu
LD = ch.LD
STEPS = sh.STEPS


@pytest.fixture(scope="module")
def hip():
    from fbstab_amd import hip_api
    hip_api.load_library()
    return hip_api


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


_LIVE = []


@functools.lru_cache(maxsize=None)
def solver(sizes):
    from fbstab_amd.condense import CondensedMpc
    _LIVE.append(CondensedMpc(*sizes, max_batch=ch.BATCH))
    return _LIVE[-1]


@pytest.fixture(scope="module", autouse=True)
def _release_the_solvers():
    """The solvers and sweeps the tests of this module share are released behind its last test: a handle holds a
    stream and scratch, and the modules behind this one start from the device as this one found it."""
    yield
    import torch
    torch.cuda.synchronize()
    while _LIVE:
        _LIVE.pop().close()
    solver.cache_clear()
    sweep.cache_clear()


def _data(p, x0=None, qps=None):
    d = {k: _dev(a if qps is None else a[qps]) for k, a in p.arrays.items()}
    if x0 is not None:
        d["x0"] = _dev(x0)
    return d


# ---- 1. the map on the device ---------------------------------------------------------------------------------------
def map_raw(hip, p, pad=0, shared=False, stride0=False, qps=None):
    """One call of fbstab_hip_mpc_condensed_x0_map_batch: (rc, (rows, len + pad) numpy array pre-filled with NaN)."""
    import torch
    lib = hip.load_library()
    qps = list(range(p.batch)) if qps is None else qps
    data, keep = hip._MpcBatch(), []
    for i, k in enumerate(ch.MPC_NAMES):
        share = shared and k in ch.MATRIX_NAMES
        t = _dev(p.arrays[k][[0] if share else qps])
        keep.append(t)
        data.base[i], data.stride[i] = t.data_ptr(), (0 if share else t.shape[1])
    n = ((p.N + 1) * p.nu + p.nv) * p.nx
    M = torch.full((1 if stride0 else len(qps), n + pad), np.nan, dtype=torch.float64, device="cuda")
    rc = lib.fbstab_hip_mpc_condensed_x0_map_batch(*p.sizes(), len(qps), C.byref(data), C.c_void_p(M.data_ptr()),
                                                   0 if stride0 else n + pad, 0, None)
    torch.cuda.synchronize()
    return rc, M.cpu().numpy()


@pytest.mark.parametrize("name", ["tiny", "small", "odd33", "flat", "four_wave"])
def test_device_map_meets_the_rule(hip, name):
    import torch
    p = ch.problem(name)
    cm = solver(p.sizes())
    m = cm.X0Map(_data(p))
    torch.cuda.synchronize()
    M, f0, b0 = (m[k].cpu().numpy() for k in ("M", "f0", "b0"))
    assert M.shape[0] == p.batch and not np.isnan(M).any()
    worst = 0.0
    for q in range(p.batch):
        F, G = sh.map_parts(p, M[q])
        for x in sh.test_states(p, q):
            worst = max(worst, sh.affine_ratio(p, q, F, G, f0[q], b0[q], x))
    print(name, "worst error / bound of base + M x:", worst)
    assert worst <= 1.0
    # padded strides: the same bits, and the pad survives
    rc, padded = map_raw(hip, p, pad=3)
    assert rc == 0, hip.load_library().fbstab_hip_last_error()
    n = M.shape[1]
    assert padded[:, :n].tobytes() == M.tobytes() and np.isnan(padded[:, n:]).all()
    # a trajectory alone gives the bits it has in the batch
    rc, alone = map_raw(hip, p, qps=[3])
    assert rc == 0 and alone[0].tobytes() == M[3].tobytes()


@pytest.mark.parametrize("name", ["small", "odd33"])
def test_shared_model_gives_one_map(hip, name):
    p = ch.problem(name)
    rc, one = map_raw(hip, p, shared=True, stride0=True)
    assert rc == 0, hip.load_library().fbstab_hip_last_error()
    rc, per_qp = map_raw(hip, p)
    assert rc == 0
    assert one.shape[0] == 1 and one[0].tobytes() == per_qp[0].tobytes()
    rc, res = map_raw(hip, p, stride0=True)     # some matrix sequence per QP: refused, nothing written
    assert rc == 1 and b"stride 0" in hip.load_library().fbstab_hip_last_error() and np.isnan(res).all()
    # the class asks for the one image by itself
    d = _data(p)
    for k in ch.MATRIX_NAMES:
        d[k] = d[k][:1]
    m = solver(p.sizes()).X0Map(d)
    assert m["M"].shape[0] == 1 and m["M"].cpu().numpy()[0].tobytes() == per_qp[0].tobytes()


# ---- the sweeps the tests share ------------------------------------------------------------------------------------
def run_sweep(name, mode, shift=False, T=0, retire=True, w="setup", steps=STEPS, qps=None, numpy_inputs=False):
    """``CondensedMpc.RecedingSweep`` on ``sh.setup(name)`` from a zero guess: the returned dict as numpy arrays plus
    ``z_end, l_end, v_end, y_end`` (the point left in the caller's arrays) and ``x_end``."""
    import torch
    p, A, B, wd = sh.setup(name)
    qps = list(range(p.batch)) if qps is None else qps
    n = len(qps)
    cm = solver(p.sizes())
    w = wd[:steps, qps] if isinstance(w, str) else w
    if numpy_inputs:
        data = {k: a[qps].copy() for k, a in p.arrays.items()}
        point = [np.zeros((n, m)) for m in (p.nz, p.nl, p.nv, p.nv)]
        r = cm.RecedingSweep(data, *point, A[qps], B[qps], steps, retire=retire, w=w, shift=shift, mode=mode,
                             log=("x", "U", "v"), traj_per_group=T)
        assert all(isinstance(a, np.ndarray) for a in r.values())
        r.update(z_end=point[0], l_end=point[1], v_end=point[2], y_end=point[3], x_end=data["x0"])
        return r
    data = _data(p, qps=qps)
    point = [torch.zeros((n, m), dtype=torch.float64, device="cuda") for m in (p.nz, p.nl, p.nv, p.nv)]
    r = cm.RecedingSweep(data, *point, _dev(A[qps]), _dev(B[qps]), steps, retire=retire,
                         w=None if w is None else _dev(w), shift=shift, mode=mode, log=("x", "U", "v"),
                         traj_per_group=T)
    assert all(a.is_cuda for a in r.values())
    torch.cuda.synchronize()
    from fbstab_amd import hip_api
    res = {k: (hip_api.out_to_numpy(a) if k == "out" else a.cpu().numpy()) for k, a in r.items()}
    res.update(z_end=point[0].cpu().numpy(), l_end=point[1].cpu().numpy(), v_end=point[2].cpu().numpy(),
               y_end=point[3].cpu().numpy(), x_end=data["x0"].cpu().numpy())
    return res


@functools.lru_cache(maxsize=None)
def sweep(name, mode, shift=False):
    """Computed once, shared by the tests, left unchanged."""
    return run_sweep(name, mode, shift)


def _same(a, b, keys=("u", "x", "U", "v", "eflag", "newton", "z_end", "l_end", "v_end", "y_end", "x_end")):
    return [k for k in keys if np.asarray(a[k]).tobytes() != np.asarray(b[k]).tobytes()]


def _check_plant(name, r, qps=None):
    """x_log[k + 1] and x_end within the plant bound of (x_log[k], u_log[k], w_k); zero once gone."""
    p, A, B, w = sh.setup(name)
    qps = list(range(p.batch)) if qps is None else qps
    steps = r["x"].shape[0]
    for k in range(steps):
        ref, S = sh.plant_reference(A[qps], B[qps], r["x"][k], r["u"][k], w[k, qps])
        nxt = r["x"][k + 1] if k + 1 < steps else r["x_end"]
        live = r["eflag"][k] != -1
        assert (np.abs(nxt.astype(LD) - ref)[live] <= sh.plant_bound(p.nx, p.nu, S)[live]).all(), (name, k)
        assert (nxt[~live] == 0.0).all() and (r["u"][k][~live] == 0.0).all()


# ---- 2. RECONDENSE mode is the public calls, bit for bit ---------------------------------------------------------
@pytest.mark.parametrize("name", ["double_integrator", "small", "four_wave"])
@pytest.mark.parametrize("shift", [False, True])
def test_recondense_sweep_is_a_loop_over_the_public_calls(hip, name, shift):
    import torch
    p, A, B, w = sh.setup(name)
    sizes = p.sizes()
    N, nx, nu, nc = sizes
    r = sweep(name, "recondense", shift)
    assert sh.retirement(r["eflag"]) == sh.RETIRES[name]
    assert ((r["eflag"] == 0) | (r["eflag"] == -1)).all()
    _check_plant(name, r)
    assert (r["u"] == r["U"][:, :, :nu]).all()
    cm = solver(sizes)
    data = _data(p)
    cm.Condense(data)
    U, v = np.zeros((p.batch, (N + 1) * nu)), np.zeros((p.batch, p.nv))
    for k in range(STEPS):
        if k > 0:
            U, v = r["U"][k - 1].copy(), r["v"][k - 1].copy()
            if shift:
                sh.shift_condensed(U, v, sizes)
        z = np.zeros((p.batch, N + 1, nx + nu))
        z[:, :, nx:] = U.reshape(p.batch, N + 1, nu)
        data["x0"] = _dev(r["x"][k])
        zd, ld, vd, yd = _dev(z.reshape(p.batch, -1)), _dev(np.zeros((p.batch, p.nl))), _dev(v), _dev(np.zeros_like(v))
        out = hip.out_to_numpy(cm.Solve(data, zd, ld, vd, yd, recondense="vectors"))
        torch.cuda.synchronize()
        gone = r["eflag"][k] == -1
        assert np.array_equal(out["newton_iters"], r["newton"][k]), k
        assert np.array_equal(out["eflag"][~gone], r["eflag"][k][~gone]), k
        first = gone & ((r["eflag"][k - 1] != -1) if k > 0 else True)
        assert (out["eflag"][first] != 0).all()
        Uk, vk = ch.u_of(p, zd.cpu().numpy()), vd.cpu().numpy()
        assert Uk[~gone].tobytes() == r["U"][k][~gone].tobytes() and vk[~gone].tobytes() == r["v"][k][~gone].tobytes(), k
        assert (r["U"][k][gone] == 0).all() and (r["v"][k][gone] == 0).all()
        if k + 1 == STEPS:
            # the point left in (z, l, v, y): the expansion of the last logged point at the last logged state
            ze, le, ve, ye = cm.Expand(data, _dev(r["U"][k]), _dev(r["v"][k]), _dev(r["y_end"]))
            for got, ref in ((r["z_end"], ze), (r["l_end"], le), (r["v_end"], ve), (r["y_end"], ye)):
                assert got.tobytes() == ref.cpu().numpy().tobytes()
            assert r["y_end"][~gone].tobytes() == yd.cpu().numpy()[~gone].tobytes()
            assert r["out"]["eflag"].tolist() == out["eflag"].tolist()


# ---- 3. AFFINE mode against the reference --------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["double_integrator", "small", "four_wave", "tiny"])
@pytest.mark.parametrize("shift", [False, True])
def test_affine_sweep_against_the_reference_loop(name, shift):
    ref = sh.oracle_loop(name, shift)
    a, rcd = sweep(name, "affine", shift), sweep(name, "recondense", shift)
    assert np.array_equal(a["eflag"], ref["eflag"])
    _check_plant(name, a)
    g_a, g_r = sh.gap(a["u"], ref["u"]), sh.gap(rcd["u"], ref["u"])
    g_fma = sh.gap(sh.oracle_loop(name, shift, "fma")["u"], ref["u"])
    g_aff_ref = sh.gap(sh.oracle_loop(name, shift, "affine")["u"], ref["u"])
    floor = STEPS * 2.0 ** -52
    print(name, "shift" if shift else "unshifted", "g_a", g_a, "g_r", g_r, "g_fma", g_fma, "g_aff_ref", g_aff_ref,
          "floor", floor)
    assert g_a <= 10 * max(g_r, g_fma, g_aff_ref, floor)
    assert np.array_equal(rcd["eflag"], ref["eflag"])


# ---- 4. independence ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "double_integrator"])
def test_results_do_not_depend_on_the_grouping(name):
    base = sweep(name, "affine")
    for T in (1, 2):
        assert _same(run_sweep(name, "affine", T=T), base) == [], T
    assert _same(run_sweep(name, "affine"), base) == []          # a second run
    # a trajectory alone, and the shared-map path of a one-trajectory batch, give the bits of the batch
    alone = run_sweep(name, "affine", qps=[3])
    for k in ("u", "x", "U", "v", "eflag", "newton"):
        assert alone[k][:, 0].tobytes() == np.ascontiguousarray(base[k][:, 3]).tobytes(), k
    assert alone["z_end"][0].tobytes() == base["z_end"][3].tobytes()
    assert alone["x_end"][0].tobytes() == base["x_end"][3].tobytes()


def test_without_retirement_every_step_is_solved():
    r = run_sweep("small", "affine", retire=False)
    assert not (r["eflag"] == -1).any()
    assert r["eflag"][3, 2] > 0                 # (the solve that retires trajectory 2 in the other sweeps)
    keep = sweep("small", "affine")
    live = [q for q in range(ch.BATCH) if q not in sh.RETIRES["small"]]
    assert r["u"][:, live].tobytes() == keep["u"][:, live].tobytes()


def test_no_disturbance_is_a_zero_disturbance():
    p = sh.setup("small")[0]
    none = run_sweep("small", "affine", w=None)
    zero = run_sweep("small", "affine", w=np.zeros((STEPS, p.batch, p.nx)))
    assert _same(none, zero) == []


@pytest.mark.parametrize("mode", ["affine", "recondense"])
def test_one_step_is_one_solve_and_one_plant_step(hip, mode):
    import torch
    name = "small"
    p, A, B, w = sh.setup(name)
    r = run_sweep(name, mode, steps=1)
    cm = solver(p.sizes())
    point = [torch.zeros((p.batch, m), dtype=torch.float64, device="cuda") for m in (p.nz, p.nl, p.nv, p.nv)]
    out = hip.out_to_numpy(cm.Solve(_data(p), *point, recondense="all"))
    torch.cuda.synchronize()
    assert (out["eflag"] == 0).all() and np.array_equal(r["eflag"][0], out["eflag"])
    assert np.array_equal(r["newton"][0], out["newton_iters"])
    for k, t in zip(("z_end", "l_end", "v_end", "y_end"), point):
        assert r[k].tobytes() == t.cpu().numpy().tobytes(), k
    assert r["u"][0].tobytes() == np.ascontiguousarray(r["z_end"][:, p.nx:p.nx + p.nu]).tobytes()
    assert r["x"][0].tobytes() == p.arrays["x0"].tobytes()
    _check_plant(name, r)


# ---- 5. placements ---------------------------------------------------------------------------------------------
def test_torch_inputs_stay_on_the_device_and_nothing_waits(hip):
    import torch
    name = "small"
    p, A, B, w = sh.setup(name)
    cm = solver(p.sizes())
    data = _data(p)
    point = [torch.zeros((p.batch, m), dtype=torch.float64, device="cuda") for m in (p.nz, p.nl, p.nv, p.nv)]
    Ad, Bd, wd = _dev(A), _dev(B), _dev(w)
    torch.cuda.synchronize()
    gen = cm.generation
    # a spin of some tens of milliseconds queued first: were the call to wait for the device or copy a result to the host, it would
    # return behind the spin; an event recorded right behind the call is still pending when it returns without
    torch.cuda._sleep(50_000_000)
    r = cm.RecedingSweep(data, *point, Ad, Bd, STEPS, w=wd, log=("x",))
    done = torch.cuda.Event()
    done.record()
    pending = not done.query()
    torch.cuda.synchronize()
    assert pending, "RecedingSweep waited for the device"
    assert cm.generation > gen
    assert set(r) == {"out", "u", "eflag", "newton", "x"} and all(a.is_cuda for a in r.values())
    base = sweep(name, "affine")
    assert r["u"].cpu().numpy().tobytes() == base["u"].tobytes()
    assert data["x0"].cpu().numpy().tobytes() == base["x_end"].tobytes()
    # the images left behind are those of the last step: the derivative calls work at the returned point
    data["x0"] = r["x"][-1].clone()
    live = base["eflag"][-1] == 0
    s = cm.X0Sensitivity(data, point[0], point[1], point[2], want=("gain",))
    torch.cuda.synchronize()
    assert (s["status"].cpu().numpy()[live] == 0).all() and np.isfinite(s["gain"].cpu().numpy()[live]).all()
    f_last = cm._img["f"].cpu().numpy()
    cm.Condense(data, "vectors")
    assert np.allclose(f_last[live], cm._img["f"].cpu().numpy()[live], rtol=1e-9, atol=1e-12)


def test_numpy_inputs_come_back_as_numpy():
    r = run_sweep("small", "affine", numpy_inputs=True)
    assert _same(r, sweep("small", "affine")) == []
