"""CPU-only checks of the many-right-hand-side solves (fbstab_hip_mpc_kkt_solve_batch,
fbstab_hip_mpc_x0_sensitivity_batch): the device logic of fb_kkt_multi.h compiled single-threaded for the host
(tests/hostsim/kkt_multi.cc) against the oracle's linear solver, and the exports and the argument validation of the
C-ABI without a GPU."""
import numpy as np
import pytest

from tools import fixtures as fx
from tests import helpers as H
from tests import linear_reference as LR
from tests import kkt_multi_helpers as KH
from tests.kkt_multi_helpers import STEP

NRHS = 4


@pytest.fixture(scope="module")
def host():
    return KH.HostKktMulti()


def _problems(kats):
    """(those of test_adjoint_hostsim.py)"""
    out = [H.mpc_from_kat(k) for k in kats["mpc_end_to_end"]]
    out.append(fx.synthetic_mpc_batch(6))
    return out


# The residual rule of right-hand sides k >= 1, as a multiple of the oracle's longdouble residual: TWICE the worst
# ratio measured on this test's own cases, 7.635 (LABNOTES.md, "Many right-hand sides").  Right-hand side 0 keeps the
# project's 3.  Why the others need more: not because they are solved differently - every right-hand side, 0 or not,
# is asserted below to be the BITS of mpc_adjoint fed the same seed (tests/hostsim/adjoint.cc) - but because the
# rule of 3 is a statement about the 14 seeds the adjoint's host test draws, and the 66 further draws of this test
# reach into the tail of the ratio's distribution (median 0.81; one draw in 66 beyond 3, for which mpc_adjoint
# itself leaves the same 7.635).
RESOLVE_RULE = 2 * 7.635


def test_every_right_hand_side_against_the_oracles_residual(host, oracle, kats):
    """Four random seeds per point (the last with null gl / gv), at the oracle's solutions and at the origin.  Every
    right-hand side k is bitwise what the adjoint's host compilation returns for seed k alone.  Right-hand side 0,
    drawn as test_adjoint_hostsim.py draws its seed (the same stream, the same cases), leaves at most 3 x the
    longdouble residual of V (dz, dl, dv) = (gz, -gl, -C.gv) that the oracle's RiccatiLinearSolver leaves; the others,
    solved by the vector recursions on the stored factors alone, at most RESOLVE_RULE x (see there)."""
    from tests.hostsim import HostAdjoint
    adjoint = HostAdjoint()
    rng0, rng = np.random.default_rng(31), np.random.default_rng(4107)
    checked, worst = 0, [0.0, 0.0]
    for p in _problems(kats):
        sol = oracle.solve_mpc(p)
        for q in range(p.batch):
            points = [(sol[0][q], sol[1][q], sol[2][q]), (np.zeros(p.nz), np.zeros(p.nl), np.zeros(p.nv))]
            for x in points:
                first = LR.random_seeds(rng0, p, 1)
                gz, gl, gv = (np.concatenate([a, b]) for a, b in zip(first, KH.random_seed_block(rng, p, NRHS - 1)))
                gl[-1] = 0.0
                gv[-1] = 0.0
                res = host.solve(p, q, x, gz, gl, gv)
                # (a NULL slot is null for all right-hand sides of a call: the last seed's zero gl / gv rows, and
                # the same seed in a call of its own with the slots null)
                null = host.solve(p, q, x, gz[-1:], None, None)
                assert res["status"] == null["status"] == 0
                for k in range(NRHS):
                    seeds = (gz[k], gl[k], gv[k])
                    step = tuple(res[n][k] for n in STEP)
                    st, alone, _ = adjoint.adjoint(p, q, x, seeds, want=())
                    assert st == 0 and all(np.array_equal(a, b) for a, b in zip(alone, step)), (q, k)
                    if k == NRHS - 1:   # (the null gl / gv slots of the one-seed call: the same bits)
                        assert all(np.array_equal(null[n][0], s) for n, s in zip(STEP, step)), q
                    ref = LR.oracle_adjoint(oracle, p, q, x, seeds)
                    r_dev = LR.adjoint_residual(p, q, x, step, seeds)
                    r_orc = LR.adjoint_residual(p, q, x, ref, seeds)
                    worst[min(k, 1)] = max(worst[min(k, 1)], r_dev / r_orc)
                    assert r_dev <= (3 if k == 0 else RESOLVE_RULE) * r_orc, (q, k, r_dev, r_orc)
                    scale = max(np.abs(np.concatenate(step)).max(), 1.0)
                    assert np.abs(np.concatenate(step) - np.concatenate(ref)).max() <= 1e-5 * scale  # (cond(V) ~ 1e11)
                checked += 1
    print("worst residual / oracle's: %.3f (rhs 0), %.3f (rhs >= 1)" % tuple(worst))
    assert checked >= 2 * 7


def test_null_seed_slots_are_zero_seeds(host, oracle):
    p = fx.synthetic_mpc_batch(1)
    sol = oracle.solve_mpc(p)
    x = (sol[0][0], sol[1][0], sol[2][0])
    gz = np.random.default_rng(3).standard_normal((3, p.nz))
    a = host.solve(p, 0, x, gz)
    b = host.solve(p, 0, x, gz, np.zeros((3, p.nl)), np.zeros((3, p.nv)))
    assert a["status"] == b["status"] == 0
    for n in STEP:
        assert np.array_equal(a[n], b[n]), n


def test_right_hand_sides_do_not_depend_on_each_other(host, oracle):
    """Permuting right-hand sides 1 .. nrhs-1 permutes the outputs bitwise; right-hand side 0 is the nrhs = 1 call's,
    and the adjoint's own (tests/hostsim/adjoint.cc), bitwise."""
    from tests.hostsim import HostAdjoint
    p = fx.synthetic_mpc_batch(2)
    sol = oracle.solve_mpc(p)
    rng = np.random.default_rng(77)
    for q in range(p.batch):
        x = (sol[0][q], sol[1][q], sol[2][q])
        gz, gl, gv = KH.random_seed_block(rng, p, NRHS)
        base = host.solve(p, q, x, gz, gl, gv)
        perm = np.array([0, 3, 1, 2])
        moved = host.solve(p, q, x, gz[perm], gl[perm], gv[perm])
        one = host.solve(p, q, x, gz[:1], gl[:1], gv[:1])
        st, adj, _ = HostAdjoint().adjoint(p, q, x, (gz[0], gl[0], gv[0]), want=())
        assert base["status"] == moved["status"] == one["status"] == st == 0
        for n, a in zip(STEP, adj):
            assert np.array_equal(moved[n], base[n][perm]), n
            assert np.array_equal(one[n][0], base[n][0]), n
            assert np.array_equal(a, base[n][0]), n
            assert np.abs(base[n]).max() > 0


def test_x0_mode_is_the_explicit_call_and_the_gain_is_the_u0_rows(host, oracle, kats):
    """The x0 mode's generated right-hand sides (gz = 0, gl = -e_j in the l_0 block, gv = 0) give the bits of the
    explicit call with those seeds, and the gain is the u0 rows of stage 0 of the dz columns, bitwise - also when no
    step slot is taken."""
    for p in (_problems(kats)[0], fx.synthetic_mpc_batch(1)):
        sol = oracle.solve_mpc(p)
        x = (sol[0][0], sol[1][0], sol[2][0])
        res = host.x0_sensitivity(p, 0, x)
        ref = host.solve(p, 0, x, *KH.x0_seed_block(p))
        assert res["status"] == ref["status"] == 0
        for n in STEP:
            assert np.array_equal(res[n], ref[n]), n
        assert res["gain"].shape == (p.nu, p.nx)
        assert np.array_equal(res["gain"], res["dz"][:, p.nx:p.nx + p.nu].T)
        assert np.abs(res["gain"]).max() > 0
        alone = host.x0_sensitivity(p, 0, x, want=())
        assert np.array_equal(alone["gain"], res["gain"]) and set(alone) == {"gain", "status"}


def test_factorisation_failure_gives_status_1_and_zeros_for_every_right_hand_side(host):
    """An indefinite stage Hessian (Q = -I, the set-up of the adjoint's host test): status 1 and zeros in every
    output, for all right-hand sides, in both modes."""
    p = fx.synthetic_mpc_batch(1)
    p.arrays["Q"] = np.ascontiguousarray(np.tile(-np.eye(p.nx).reshape(-1), (1, p.N + 1)))
    x = (np.zeros(p.nz), np.zeros(p.nl), np.zeros(p.nv))
    res = host.solve(p, 0, x, np.ones((NRHS, p.nz)), np.ones((NRHS, p.nl)), np.ones((NRHS, p.nv)))
    sens = host.x0_sensitivity(p, 0, x)
    assert res["status"] == 1 and sens["status"] == 1
    for n in STEP:
        assert np.array_equal(res[n], np.zeros_like(res[n])), n
        assert np.array_equal(sens[n], np.zeros_like(sens[n])), n
    assert np.array_equal(sens["gain"], np.zeros((p.nu, p.nx)))


def test_entry_points_are_exported_and_bound():
    import ctypes as C
    from fbstab_amd import hip_api
    lib = hip_api.load_library()
    for name in ("fbstab_hip_mpc_kkt_solve_batch", "fbstab_hip_mpc_x0_sensitivity_batch"):
        assert name in hip_api.EXPORTED_SYMBOLS and getattr(lib, name).argtypes is not None, name
    assert C.sizeof(hip_api._MultiVarBatch) == 9 * 8
    assert hasattr(hip_api.FBstabMpcBatch, "KktSolve") and hasattr(hip_api.FBstabMpcBatch, "X0Sensitivity")
    from fbstab_amd import autograd
    assert "mpc_x0_sensitivity" in autograd.__all__ and "DETACHED" in autograd.mpc_x0_sensitivity.__doc__


# What a machine without a GPU can ask of fbstab_hip_mpc_kkt_solve_batch: no handle exists there, and what needs no
# handle is checked first - so each of these is refused for its own reason, before "null solver handle" and before any
# device call.  (stride, rhs_stride) of every slot: the default (64, 8) is in order for nrhs = 2.
_BAD = {
    "nrhs_0": (dict(nrhs=0), "fewer than one right-hand side"),
    "nrhs_negative": (dict(nrhs=-3), "fewer than one right-hand side"),
    "null_seed_block": (dict(null=("seed",)), "null seed or step block"),
    "null_step_block": (dict(null=("step",)), "null seed or step block"),
    "null_seed_z": (dict(seed_z=False), "null seed pointer (z)"),
    "seed_rhs_stride_0": (dict(seed=(64, 0)), "seed rhs_stride"),
    "seed_rhs_stride_negative": (dict(seed=(64, -8)), "seed rhs_stride"),
    "step_rhs_stride_0": (dict(step=(64, 0)), "step rhs_stride"),
    "seed_stride_below_its_vectors": (dict(batch=2, nrhs=3, seed=(16, 8)), "seed stride"),
    "seed_stride_negative": (dict(batch=2, seed=(-64, 8)), "seed stride"),
    "step_stride_below_its_vectors": (dict(batch=2, nrhs=3, step=(16, 8)), "step stride"),
    "step_stride_0": (dict(batch=2, step=(0, 8)), "step stride"),
}


@pytest.mark.parametrize("case", list(_BAD))
def test_bad_arguments_are_refused_before_the_handle_is_looked_at(case):
    from fbstab_amd import hip_api
    lib = hip_api.load_library()
    kw, msg = _BAD[case]
    rc, text = KH.handle_free_kkt_solve(lib, **kw)
    assert rc == 1 and msg in text, (rc, text)   # FBSTAB_HIP_ERR_ARGUMENT


@pytest.mark.parametrize("kw", [dict(), dict(batch=2), dict(batch=2, seed=(0, 8)), dict(nrhs=1, seed=(0, 0), step=(0, 0))],
                         ids=["valid", "batch2", "shared_seed", "one_rhs_ignores_rhs_stride"])
def test_calls_that_are_in_order_get_as_far_as_the_handle(kw):
    from fbstab_amd import hip_api
    lib = hip_api.load_library()
    assert KH.handle_free_kkt_solve(lib, **kw) == (1, "null solver handle")


def test_x0_sensitivity_without_a_handle():
    import ctypes as C
    from fbstab_amd import hip_api
    lib = hip_api.load_library()
    b, x = hip_api._MpcBatch(), hip_api._VarBatch()
    st = np.zeros(1, dtype=np.int32)
    rc = lib.fbstab_hip_mpc_x0_sensitivity_batch(None, 1, C.byref(b), C.byref(x), 0.0, None, None, 0, st.ctypes.data, 0,
                                                 None)
    assert rc == 1 and b"null solver handle" in lib.fbstab_hip_last_error()
