"""Closed-loop sweeps of the condensed route (fbstab_hip_mpc_condensed_x0_map_batch,
fbstab_hip_mpc_condensed_receding_sweep, fb_condense_sweep.h) without a GPU: the affine map of x0 from the device
logic compiled for one host thread against the extended-precision reference and the existing acceptance rule, the
rule against seeded defects, the step function against the bookkeeping of tests/closed_loop.logged_closed_loop, the
argument checks of the C-ABI, and the reference closed loop itself.

Measured here (host build, every QP, three states each), worst error / bound of base + M x:
tiny 0.016, small 0.0028, odd33 0.00036, flat 0.00026, four_wave 0.00098, double_integrator 1.9e-6."""
import ctypes as C

import numpy as np
import pytest

from tests import condense_helpers as ch
from tests import condense_sweep_helpers as sh
from tools import fixtures as fx

LD = ch.LD
MAP_SHAPES = ("tiny", "small", "odd33", "flat", "four_wave", "double_integrator")


@pytest.fixture(scope="module")
def host():
    return sh.HostSweep()


@pytest.fixture(scope="module")
def condense():
    return ch.HostCondense()


def _base(condense, p, q):
    """f_c(0), b_c(0) of QP ``q`` by the vectors kernel's host build."""
    r = condense.condense(sh.with_x0(p, np.zeros_like(p.arrays["x0"])), q, condense.VECTORS)
    return r["f"], r["b"]


# ---- 1. the map ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MAP_SHAPES)
def test_host_build_of_the_map_meets_the_rule(host, condense, name):
    p = ch.problem(name)
    worst = 0.0
    for q in range(p.batch):
        M = host.x0_map(p, q)
        assert not np.isnan(M).any()
        F, G = sh.map_parts(p, M)
        f0, b0 = _base(condense, p, q)
        for x in sh.test_states(p, q):
            worst = max(worst, sh.affine_ratio(p, q, F, G, f0, b0, x))
    print(name, "worst error / bound of base + M x:", worst)
    assert worst <= 1.0


def test_map_of_a_shared_model_is_the_image_of_qp_0(host):
    p = ch.problem("small")
    m = fx.MpcProblem(*p.sizes())
    m.arrays = {k: (np.repeat(a[:1], p.batch, axis=0) if k in ch.MATRIX_NAMES else a) for k, a in p.arrays.items()}
    assert host.x0_map(m, 3).tobytes() == host.x0_map(p, 0).tobytes()   # (q, r, c, d, x0 do not enter)


# ---- 2. the rule catches seeded defects on M ---------------------------------------------------------------------
def _numpy_map(p, q, defect=None):
    """F, G in float64 by the formulas of fb_condense_sweep.h, with one seeded defect."""
    N, nx, nu, nc = p.sizes()
    a = p.arrays
    mat = lambda k, i, r, c: a[k][q][i * r * c:(i + 1) * r * c].reshape(c, r).T
    Phi = [np.eye(nx)]
    for i in range(N):
        Phi.append(mat("A", i, nx, nx) @ Phi[i])
    G = np.vstack([(1.0 if defect == "G_sign" else -1.0) * mat("E", i, nc, nx) @ Phi[i] for i in range(N + 1)])
    F = [None] * (N + 1)
    P = np.zeros((nx, nx))
    for k in range(N, -1, -1):
        F[k] = np.zeros((nu, nx)) if defect == "S_dropped" else mat("S", k, nu, nx) @ Phi[k]
        if k < N:
            F[k] = F[k] + mat("B", k, nx, nu).T @ P
        elif defect == "B_at_N":      # (no branch for the last stage: the images of stage N - 1 and a stale P)
            F[k] = F[k] + mat("B", N - 1, nx, nu).T @ (mat("Q", N, nx, nx) @ Phi[N])
        P = mat("Q", k, nx, nx) @ Phi[k] + (mat("A", k, nx, nx).T @ P if k < N else 0.0)
    return np.vstack(F), G


@pytest.mark.parametrize("defect", ["S_dropped", "B_at_N", "G_sign", "one_entry_1e-9"])
def test_rule_catches_seeded_defects_on_the_map(host, condense, defect):
    caught = []
    for name in MAP_SHAPES:
        p = ch.problem(name)
        f0, b0 = _base(condense, p, 0)
        F, G = sh.map_parts(p, host.x0_map(p, 0))
        Fn, Gn = _numpy_map(p, 0)
        states = sh.test_states(p, 0)
        # (the float64 restatement itself is a correct map: it passes where the host build does)
        assert max(sh.affine_ratio(p, 0, Fn, Gn, f0, b0, x) for x in states) <= 1.0
        if defect == "one_entry_1e-9":
            # (... and looked at where that entry is the whole product: the unit state of its column)
            Fb, Gb = F.copy(), G.copy()
            for W in (Fb, Gb):
                i = np.unravel_index(np.argmax(np.abs(W)), W.shape)
                W[i] *= 1.0 + 1e-9
                states = states + [np.eye(p.nx)[i[1]]]
        else:
            Fb, Gb = _numpy_map(p, 0, defect)
        if max(sh.affine_ratio(p, 0, Fb, Gb, f0, b0, x) for x in states) > 1.0:
            caught.append(name)
    print(defect, "caught on", caught)
    assert caught, defect
    if defect in ("G_sign", "one_entry_1e-9"):
        assert caught == list(MAP_SHAPES)


# ---- 3. the step function on the host ---------------------------------------------------------------------------
def _scripted_loop(name, shift, retire):
    """condensed_closed_loop around a scripted solver: random points, a failure of trajectory 1 at step 2 and of
    trajectory 3 at steps 5 and 6.  Returns (log, the guesses and returns of every step)."""
    p, A, B, w = sh.setup(name)
    rng = np.random.default_rng(9)
    calls = []

    def solve(x, U, v):
        k = len(calls)
        out = np.zeros(p.batch, dtype=[("eflag", np.int32), ("newton_iters", np.int32)])
        out["newton_iters"] = rng.integers(1, 30, p.batch)
        out["eflag"][1] = 3 if k == 2 else 0
        out["eflag"][3] = 2 if k in (5, 6) else 0
        Un, vn = rng.standard_normal(U.shape), np.abs(rng.standard_normal(v.shape))
        calls.append(dict(gU=U.copy(), gv=v.copy(), U=Un, v=vn, out=out))
        return Un, vn, out
    return sh.condensed_closed_loop(solve, p, A, B, sh.STEPS, w=w, shift=shift, retire=retire), calls


@pytest.mark.parametrize("name", ["small", "double_integrator"])
@pytest.mark.parametrize("shift", [False, True])
@pytest.mark.parametrize("retire", [True, False])
def test_host_step_is_the_bookkeeping_of_logged_closed_loop(host, name, shift, retire):
    p, A, B, w = sh.setup(name)
    sizes = p.sizes()
    N, nx, nu, nc = sizes
    log, calls = _scripted_loop(name, shift, retire)
    if retire:
        assert sh.retirement(log["eflag"]) == {1: 2, 3: 5}
    else:
        assert not (log["eflag"] == -1).any() and (log["eflag"][5:7, 3] == 2).all()
    per_T = {}
    for T in (1, 2, 5):
        U, v = np.zeros((p.batch, (N + 1) * nu)), np.zeros((p.batch, p.nv))
        gone = np.zeros(p.batch, dtype=np.int32)
        rec = []
        for k, c in enumerate(calls):
            # the guess the step before left behind is the one the numpy loop handed to its solver
            assert U.tobytes() == c["gU"].tobytes() and v.tobytes() == c["gv"].tobytes(), (T, k)
            U[...] = c["U"]; v[...] = c["v"]
            x = log["x"][k].copy()
            last = k + 1 == len(calls)
            r = host.step(sizes, U, v, x, gone, c["out"]["eflag"], c["out"]["newton_iters"], A, B, w=w[k],
                          retire=retire, shift=shift and not last, T=T)
            for key in ("u", "x", "U", "v", "eflag", "newton"):
                assert r[key].tobytes() == log[key][k].tobytes(), (T, k, key)
            assert r["xkeep"].tobytes() == log["x"][k].tobytes()
            # the plant step against longdouble; a gone trajectory stays at the origin
            ref, S = sh.plant_reference(A, B, log["x"][k], log["u"][k], w[k])
            live = log["eflag"][k] != -1
            assert (np.abs(x.astype(LD) - ref)[live] <= sh.plant_bound(nx, nu, S)[live]).all(), (T, k)
            assert (x[~live] == 0.0).all() and (U[~live] == 0.0).all() and (v[~live] == 0.0).all()
            rec.append((x.copy(), U.copy(), v.copy(), gone.copy()))
        per_T[T] = rec
    for T in (2, 5):
        for a, b in zip(per_T[1], per_T[T]):
            assert all(s.tobytes() == t.tobytes() for s, t in zip(a, b)), T


def test_host_step_null_logs_and_affine_update(host, condense):
    """Without logs nothing but the state and the guess moves; the affine update is base + M x+ entry for entry, the
    same bits from a staged shared M, from memory, and for every T."""
    p, A, B, w = sh.setup("small")
    sizes = p.sizes()
    N, nx, nu, nc = sizes
    rng = np.random.default_rng(4)
    M = np.stack([host.x0_map(p, q) for q in range(p.batch)])
    base = [_base(condense, p, q) for q in range(p.batch)]
    f0, b0 = np.stack([f for f, _ in base]), np.stack([b for _, b in base])
    U0, v0 = rng.standard_normal((p.batch, (N + 1) * nu)), np.abs(rng.standard_normal((p.batch, p.nv)))
    eflag = np.array([0, 0, 4, 0, 0], dtype=np.int32)
    got = {}
    for key, (Mk, T, stage) in dict(per_qp=(M, 0, False), shared_mem=(M[:1], 2, False), shared_lds=(M[:1], 2, True),
                                    shared_lds_T5=(M[:1], 5, True), shared_lds_T1=(M[:1], 1, True)).items():
        U, v, x = U0.copy(), v0.copy(), p.arrays["x0"].copy()
        gone = np.zeros(p.batch, dtype=np.int32)
        r = host.step(sizes, U, v, x, gone, eflag, np.ones(p.batch), A, B, T=T, logs=False, affine=(Mk, f0, b0),
                      stage_m=stage)
        assert gone.tolist() == [0, 0, 1, 0, 0] and (x[2] == 0).all()
        got[key] = (r["f"], r["b"], x)
        for q in range(p.batch):
            F, G = sh.map_parts(p, Mk[0 if Mk.shape[0] == 1 else q])
            # (nx + 2 roundings on the sum of the magnitudes)
            for got_v, base_v, W in ((r["f"][q], f0[q], F), (r["b"][q], b0[q], G)):
                ref = base_v.astype(LD) + W.astype(LD) @ x[q].astype(LD)
                mag = np.abs(base_v) + np.abs(W) @ np.abs(x[q])
                assert (np.abs(got_v - ref) <= (nx + 2) * 2.0 ** -53 * mag).all(), (key, q)
    for key in ("shared_lds", "shared_lds_T5", "shared_lds_T1"):
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got[key], got["shared_mem"])), key
    assert all(a[0].tobytes() == b[0].tobytes() for a, b in zip(got["per_qp"], got["shared_mem"]))   # (QP 0's rows)


def test_host_begin_reads_the_guess_as_solve_does(host):
    p = ch.problem("small")
    N, nx, nu, nc = p.sizes()
    rng = np.random.default_rng(2)
    z, v = rng.standard_normal(p.nz), rng.standard_normal(p.nv)
    U, vc, gone = host.begin(p.sizes(), z, v)
    assert U.tobytes() == ch.u_of(p, z[None])[0].tobytes() and vc.tobytes() == v.tobytes() and gone == 0


# ---- 4. the C-ABI without a GPU ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from fbstab_amd import hip_api
    return hip_api.load_library()


def _sweep_lds(N, nx, nu, nc, T, staged):
    e = lambda n: n + (n & 1)
    ne = (N + 1) * (nu + nc)
    return 8 * ((e((ne | 1) * nx) if staged else 0) + T * (2 * e(nx) + e((N + 1) * nu) + e((N + 1) * nc) + 2))


def test_condensed_sweep_sizes(lib, host):
    for N, nx, nu, nc in [(1, 1, 1, 1), (3, 5, 2, 3), (2, 33, 3, 1), (8, 6, 8, 4), (10, 40, 3, 6), (10, 60, 4, 6)]:
        ne = (N + 1) * (nu + nc)
        for shared in (0, 1):
            used, lds, work = C.c_int(-1), C.c_longlong(-1), C.c_longlong(-1)
            assert lib.fbstab_hip_mpc_condensed_sweep_sizes(N, nx, nu, nc, 0, shared, C.byref(used), C.byref(lds),
                                                            C.byref(work)) == 0
            T = used.value
            staged = bool(shared) and _sweep_lds(N, nx, nu, nc, 1, True) <= 80 * 1024
            assert 1 <= T <= min(64, -(-1024 // ne))
            assert lds.value == _sweep_lds(N, nx, nu, nc, T, staged) and lds.value <= 80 * 1024
            assert T == min(64, -(-1024 // ne)) or _sweep_lds(N, nx, nu, nc, T + 1, staged) > 80 * 1024
            assert work.value == (N + 1) * nu + 2 * (N + 1) * nc + nx + 1
            h = host.sizes(N, nx, nu, nc, 0, bool(shared))
            assert (h["T"], h["total"] * 8, bool(h["m_lds"])) == (T, lds.value, staged)
            assert lib.fbstab_hip_mpc_condensed_sweep_sizes(N, nx, nu, nc, 3, shared, C.byref(used), C.byref(lds),
                                                            None) == 0
            assert used.value == 3 and lds.value == _sweep_lds(N, nx, nu, nc, 3, staged)
    assert host.sizes(10, 40, 3, 6)["ldm"] % 2 == 1
    lds = C.c_longlong(-1)
    assert lib.fbstab_hip_mpc_condensed_sweep_sizes(10, 40, 3, 6, 4096, 1, None, C.byref(lds), None) == 3
    assert lds.value == 0 and b"LDS" in lib.fbstab_hip_last_error()
    assert lib.fbstab_hip_mpc_condensed_sweep_sizes(0, 2, 1, 1, 0, 0, None, None, None) == 1
    assert lib.fbstab_hip_mpc_condensed_sweep_sizes(2, 2, 1, 1, -1, 0, None, None, None) == 1
    assert lib.fbstab_hip_mpc_condensed_sweep_sizes(2, 2, 1, 1, 0, 0, None, None, None) == 0


class _Call:
    """The two calls on valid arguments for (2, 3, 2, 2), batch 2; no pointer is followed before the device check.
    The handle is a stand-in that is never reached: every case fails before it, or at the NULL handle."""
    N, nx, nu, nc = 2, 3, 2, 2

    def __init__(self):
        from fbstab_amd import hip_api
        self.buf = np.zeros(4096)
        ptr = self.buf.ctypes.data
        n1, N, nx, nu, nc = self.N + 1, self.N, self.nx, self.nu, self.nc
        self.len = [n1 * nx * nx, n1 * nu * nu, n1 * nu * nx, n1 * nx, n1 * nu, N * nx * nx, N * nx * nu, N * nx,
                    n1 * nc * nx, n1 * nc * nu, n1 * nc, nx]
        self.data = hip_api._MpcBatch()
        for i, n in enumerate(self.len):
            self.data.base[i], self.data.stride[i] = ptr, n
        nz, nv = n1 * nu, n1 * nc
        self.olen = [nz * nz, nz, 0, 0, nv * nz, nv]
        self.dense = hip_api._DenseBatch()
        for i, n in enumerate(self.olen):
            if n:
                self.dense.base[i], self.dense.stride[i] = ptr, n
        self.x = hip_api._VarBatch()
        for i, n in enumerate([n1 * (nx + nu), n1 * nx, nv, nv]):
            self.x.base[i], self.x.stride[i] = ptr, n
        self.map_len = (nz + nv) * nx
        self.map = hip_api._CondensedMap(ptr, ptr, ptr, self.map_len, nz, nv)
        self.plant = hip_api._Plant(ptr, ptr, 0, 0)
        self.scenario = hip_api._SweepScenario(None, 0)
        self.log = hip_api._CondensedSweepLog(ptr, ptr, ptr, ptr, ptr, ptr)
        self.sizes = [self.N, self.nx, self.nu, self.nc]
        self.batch, self.steps, self.mode, self.T = 2, 3, 0, 0
        self.map_out, self.map_stride = ptr, self.map_len
        self.out, self.work = ptr, ptr
        self.null = ()

    def _ref(self, name):
        return None if name in self.null else C.byref(getattr(self, name))

    def x0_map(self, lib):
        rc = lib.fbstab_hip_mpc_condensed_x0_map_batch(*self.sizes, self.batch, self._ref("data"),
                                                       C.c_void_p(self.map_out), self.map_stride, 0, None)
        return rc, lib.fbstab_hip_last_error().decode()

    def sweep(self, lib):
        rc = lib.fbstab_hip_mpc_condensed_receding_sweep(
            None, *self.sizes, self.batch, self._ref("data"), self._ref("dense"), self._ref("map"), self._ref("x"),
            C.c_void_p(self.out), self._ref("plant"), self.steps, 1, self._ref("scenario"), self.mode,
            self._ref("log"), self.T, C.c_void_p(self.work), None)
        return rc, lib.fbstab_hip_last_error().decode()


def _bad_cases():
    def size(i):
        def f(c): c.sizes[i] = 0
        return f
    cases = {}
    for e in ("x0_map", "sweep"):
        for i, n in enumerate(("N", "nx", "nu", "nc")):
            cases[f"{e}_{n}_zero"] = (e, size(i))
        cases[f"{e}_negative_batch"] = (e, lambda c: setattr(c, "batch", -1))
        cases[f"{e}_null_data_block"] = (e, lambda c: setattr(c, "null", ("data",)))
        cases[f"{e}_null_data_pointer"] = (e, lambda c: c.data.base.__setitem__(5, None))
        cases[f"{e}_short_data_stride"] = (e, lambda c: c.data.stride.__setitem__(0, c.len[0] - 1))
    cases["x0_map_null_output"] = ("x0_map", lambda c: setattr(c, "map_out", None))
    cases["x0_map_short_stride"] = ("x0_map", lambda c: setattr(c, "map_stride", c.map_len - 1))
    cases["x0_map_stride_0_per_qp_model"] = ("x0_map", lambda c: setattr(c, "map_stride", 0))
    for name in ("dense", "x", "plant"):
        cases[f"sweep_null_{name}_block"] = ("sweep", lambda c, name=name: setattr(c, "null", (name,)))
    cases["sweep_null_out"] = ("sweep", lambda c: setattr(c, "out", None))
    cases["sweep_null_work"] = ("sweep", lambda c: setattr(c, "work", None))
    cases["sweep_null_plant_B"] = ("sweep", lambda c: setattr(c.plant, "B", None))
    cases["sweep_negative_steps"] = ("sweep", lambda c: setattr(c, "steps", -1))
    cases["sweep_shift_2"] = ("sweep", lambda c: setattr(c.scenario, "shift", 2))
    cases["sweep_mode_2"] = ("sweep", lambda c: setattr(c, "mode", 2))
    cases["sweep_mode_negative"] = ("sweep", lambda c: setattr(c, "mode", -1))
    cases["sweep_negative_traj_per_group"] = ("sweep", lambda c: setattr(c, "T", -1))
    cases["sweep_shared_x0"] = ("sweep", lambda c: c.data.stride.__setitem__(11, 0))
    cases["sweep_null_H"] = ("sweep", lambda c: c.dense.base.__setitem__(0, None))
    cases["sweep_f_stride_0"] = ("sweep", lambda c: c.dense.stride.__setitem__(1, 0))
    cases["sweep_short_b_stride"] = ("sweep", lambda c: c.dense.stride.__setitem__(5, c.olen[5] - 1))
    cases["sweep_null_y"] = ("sweep", lambda c: c.x.base.__setitem__(3, None))
    cases["sweep_short_z_stride"] = ("sweep", lambda c: c.x.stride.__setitem__(0, 1))
    cases["sweep_short_plant_stride"] = ("sweep", lambda c: setattr(c.plant, "stride_A", 2))
    cases["sweep_affine_null_map"] = ("sweep", lambda c: setattr(c, "null", ("map",)))
    cases["sweep_affine_null_M"] = ("sweep", lambda c: setattr(c.map, "M", None))
    cases["sweep_affine_null_b0"] = ("sweep", lambda c: setattr(c.map, "b0", None))
    cases["sweep_affine_short_M_stride"] = ("sweep", lambda c: setattr(c.map, "stride_M", c.map_len - 1))
    cases["sweep_affine_short_f0_stride"] = ("sweep", lambda c: setattr(c.map, "stride_f0", 1))
    return cases


@pytest.mark.parametrize("case", sorted(_bad_cases()))
def test_bad_arguments_are_refused_before_any_device_call(lib, case):
    entry, breaker = _bad_cases()[case]
    c = _Call()
    breaker(c)
    rc, msg = getattr(c, entry)(lib)
    assert rc == 1 and msg and "handle" not in msg, (rc, msg)


def test_valid_arguments_reach_the_handle_and_the_device_check(lib):
    # the sweep: everything that needs no handle passes, then the NULL handle is refused
    for setup in (lambda c: None, lambda c: setattr(c, "null", ("scenario", "log")),
                  lambda c: (setattr(c, "mode", 1), setattr(c, "null", ("map",))),
                  lambda c: (setattr(c.map, "stride_M", 0), setattr(c.map, "stride_f0", 0))):
        c = _Call()
        setup(c)
        rc, msg = c.sweep(lib)
        assert rc == 1 and "null dense solver handle" in msg, (rc, msg)
    # the map: batch 0 queues nothing; a shared model may ask for one image
    c = _Call()
    c.batch = 0
    assert c.x0_map(lib)[0] == 0
    c = _Call()
    c.batch = 0
    for i in (0, 1, 2, 5, 6, 8, 9):
        c.data.stride[i] = 0
    c.map_stride = 0
    assert c.x0_map(lib)[0] == 0
    if lib.fbstab_hip_device_count() == 0:
        rc, msg = _Call().x0_map(lib)
        assert rc == 2 and "device" in msg, (rc, msg)


# ---- 5. the reference closed loop is well posed ------------------------------------------------------------------
@pytest.mark.parametrize("name", sh.LOOP_FIXTURES)
@pytest.mark.parametrize("shift", [False, True])
def test_reference_closed_loop_is_well_posed(name, shift):
    """The two roundings of the oracle and its float64 affine map agree on every exit flag and Newton count, and
    the trajectories retire where the table of the sweep's tests says.  Gaps measured here (fma, affine), unshifted:
    double_integrator 1.8e-12, 1.2e-12; small 2.1e-13, 1.9e-13; tiny 5e-18, 4e-17; four_wave 1.8e-10, 1.6e-10."""
    a = sh.oracle_loop(name, shift)
    f = sh.oracle_loop(name, shift, "fma")
    g = sh.oracle_loop(name, shift, "affine")
    print(name, "shift" if shift else "unshifted", "fma gap", sh.gap(f["u"], a["u"]), "affine gap",
          sh.gap(g["u"], a["u"]))
    assert sh.retirement(a["eflag"]) == sh.RETIRES[name]
    live = a["eflag"] != -1
    assert (a["eflag"][live] == 0).all()        # every other solve ends in SUCCESS
    for other in (f, g):
        assert np.array_equal(other["eflag"], a["eflag"]) and np.array_equal(other["newton"], a["newton"])
    # the reference's vectors at a moved state are ch.condense_reference's, bit for bit
    p = sh.setup(name)[0]
    x = a["x"][3]
    fv, bv = sh.condenser(name).vectors(1, x[1])
    r = ch.condense_reference(sh.with_x0(p, x), 1)
    assert (fv == r["f"]).all() and (bv == r["b"]).all()
