"""CPU-only checks of the dense many-right-hand-side solves (fbstab_hip_dense_kkt_solve_batch,
fbstab_hip_dense_jacobian_batch): the device logic of fb_dense_kkt_multi.h over DenseProblem compiled single-threaded
for the host (tests/hostsim/dense_kkt_multi.cc) against the dense adjoint's host compilation and the oracle's linear
solver, the stand-alone sanitizer build of the same file, and the exports and the argument validation of the C-ABI
without a GPU."""
import numpy as np
import pytest

from tools import fixtures as fx
from tests import linear_reference as LR
from tests import dense_kkt_multi_helpers as KH
from tests.dense_kkt_multi_helpers import STEP
from tests.hostsim import HostAdjoint
from tests.shapes import DENSE_KERNEL_SHAPES, RELAX_FROM, RELAX

NRHS = 4
# every entry of DENSE_KERNEL_SHAPES - the DenseProblem layouts, and the one-wavefront shapes, which the host runs
# through DenseProblem too (K in LDS) - and one more: the host's workgroup of one thread has a smaller reduction
# scratch than the device's 256, so that (20, 5, 2534), the smallest nv that moves the device's iterate vectors to
# global scratch, keeps them in LDS here; six rows more and the host takes that layout too
HOST_SHAPES = [s[0] for s in DENSE_KERNEL_SHAPES] + [(20, 5, 2540)]
HOST_LAYOUTS = [(0, 0), (0, 0), (0, 0), (0, 0), (1, 0), (1, 0), (1, 1)]   # (k_global, v_global) of lay.init(.., 1)
CASES = list(range(len(HOST_SHAPES)))
IDS = ["x".join(map(str, s)) for s in HOST_SHAPES]

# The residual rule, as a multiple of the oracle's longdouble residual of V (dz, dl, dv) = (gz, -gl, -C.gv): the
# project's 3.  Measured on this file's draws before it was asserted (LABNOTES.md, "Dense many right-hand sides"): the
# worst ratio over the 84 right-hand sides is 1.64, at (20, 5, 2540), and every right-hand side is the host ADJOINT's
# bits for its seed - so no draw needs the wider bar the MPC work met.
RULE = 3.0


@pytest.fixture(scope="module")
def host():
    return KH.HostDenseKktMulti()


@pytest.fixture(scope="module")
def adjoint():
    return HostAdjoint("dense")


_CACHE = {}


def _case(oracle, idx):
    """(problem, the oracle's solutions) of entry ``idx``, three QPs, the v-global shape with the relaxed b; computed
    once and left unchanged."""
    if idx not in _CACHE:
        nz, nl, nv = HOST_SHAPES[idx]
        p = fx.synthetic_dense_batch(3, nz, nl, nv, first_id=500 + 10 * idx)
        if nv >= DENSE_KERNEL_SHAPES[-1][0][2]:   # (the relaxed b of shapes.RELAX_FROM / RELAX, for the reason there)
            p.arrays["b"] = p.arrays["b"].copy()
            p.arrays["b"][:, RELAX_FROM:] += RELAX
        sol = oracle.solve_dense(p)
        assert (sol[4]["eflag"] == 0).all()
        _CACHE[idx] = (p, sol)
    return _CACHE[idx]


@pytest.mark.parametrize("idx", CASES, ids=IDS)
def test_every_right_hand_side_is_the_adjoints_and_meets_the_residual_rule(host, adjoint, oracle, idx):
    """Four random seeds per QP at the oracle's solutions (the last with null gl / gv).  Every right-hand side k is
    bitwise what hostsim_dense_adjoint returns for seed k alone, and leaves at most RULE x the longdouble residual
    that the oracle's DenseCholeskySolver leaves."""
    nz, nl, nv = HOST_SHAPES[idx]
    lay = adjoint.layout(nz, nl, nv, nthreads=1)
    assert (lay["k_global"], lay["v_global"]) == HOST_LAYOUTS[idx] and set(HOST_LAYOUTS) == {(0, 0), (1, 0), (1, 1)}
    p, sol = _case(oracle, idx)
    rng = np.random.default_rng(5200 + idx)
    worst = 0.0
    for q in range(p.batch):
        x = (sol[0][q], sol[1][q], sol[2][q])
        gz, gl, gv = KH.random_seed_block(rng, p, NRHS)
        gl[-1] = 0.0
        gv[-1] = 0.0
        res = host.solve(p, q, x, gz, gl, gv)
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
            worst = max(worst, r_dev / r_orc)
            print("qp %d rhs %d residual %.3e oracle's %.3e ratio %.3f" % (q, k, r_dev, r_orc, r_dev / r_orc))
            assert r_dev <= RULE * r_orc, (q, k, r_dev, r_orc)
    print("worst residual / oracle's on", (nz, nl, nv), "%.3f" % worst)


@pytest.mark.parametrize("idx", [2, 3, 4, 6], ids=[IDS[i] for i in (2, 3, 4, 6)])
def test_right_hand_sides_do_not_depend_on_each_other(host, oracle, idx):
    """Permuting the right-hand sides permutes the outputs bitwise, and right-hand side 0 is the nrhs = 1 call's."""
    p, sol = _case(oracle, idx)
    rng = np.random.default_rng(77 + idx)
    x = (sol[0][1], sol[1][1], sol[2][1])
    gz, gl, gv = KH.random_seed_block(rng, p, NRHS)
    base = host.solve(p, 1, x, gz, gl, gv)
    perm = np.array([2, 0, 3, 1])
    moved = host.solve(p, 1, x, gz[perm], gl[perm], gv[perm])
    one = host.solve(p, 1, x, gz[:1], gl[:1], gv[:1])
    assert base["status"] == moved["status"] == one["status"] == 0
    for n in STEP:
        assert np.array_equal(moved[n], base[n][perm]), n
        assert np.array_equal(one[n][0], base[n][0]), n
        assert base[n].size == 0 or np.abs(base[n]).max() > 0


@pytest.mark.parametrize("idx", CASES, ids=IDS)
def test_jacobian_mode_is_the_seeded_mode_on_unit_seeds(host, oracle, idx):
    """The generated right-hand sides of wrt = f, h, b (gz = -e_k, gl = e_k, gv = e_k) give the bits of the explicit
    call with those seeds spelled out - also with only the dz slot taken."""
    p, sol = _case(oracle, idx)
    x = (sol[0][0], sol[1][0], sol[2][0])
    for wrt in ("f", "h", "b"):
        if wrt == "h" and p.nl == 0:
            continue
        res = host.jacobian(p, 0, x, wrt)
        ref = host.solve(p, 0, x, *KH.unit_seed_block(p, wrt))
        assert res["status"] == ref["status"] == 0
        for n in STEP:
            assert np.array_equal(res[n], ref[n]), (wrt, n)
        assert np.abs(res["dz"]).max() > 0
        alone = host.jacobian(p, 0, x, wrt, want=("dz",))
        assert set(alone) == {"dz", "status"} and np.array_equal(alone["dz"], res["dz"])


@pytest.mark.parametrize("shape", [(20, 5, 40), (30, 0, 40)])
def test_factorisation_failure_gives_status_1_and_zeros_for_every_right_hand_side(host, shape):
    """A NaN in H[0] is a NaN on the diagonal of K, which ends the factorisation by Eigen's rule (the construction of
    the dense adjoint's status test): status 1 and zeros in every output, for all right-hand sides, in both modes."""
    p = fx.synthetic_dense_batch(1, *shape)
    p.arrays["H"] = p.arrays["H"].copy()
    p.arrays["H"][0, 0] = np.nan
    x = (np.zeros(p.nz), np.zeros(p.nl), np.zeros(p.nv))
    res = host.solve(p, 0, x, np.ones((NRHS, p.nz)), np.ones((NRHS, p.nl)), np.ones((NRHS, p.nv)))
    jac = host.jacobian(p, 0, x, "b")
    assert res["status"] == 1 and jac["status"] == 1
    for n in STEP:
        assert np.array_equal(res[n], np.zeros_like(res[n])), n
        assert np.array_equal(jac[n], np.zeros_like(jac[n])), n


def test_stand_alone_program_under_the_address_and_undefined_behaviour_sanitizers():
    """tests/hostsim/dense_kkt_multi.cc with its own main, one small QP per layout, every buffer exactly as long as
    the call may write: built with -fsanitize=address,undefined and run once, on the CPU."""
    rc, out = KH.build_and_run_sanitized()
    assert rc == 0 and "dense_kkt_multi: ok" in out, out
    assert "ERROR" not in out and "runtime error" not in out, out


def test_entry_points_are_exported_and_bound():
    from fbstab_amd import hip_api, autograd
    lib = hip_api.load_library()
    for name in ("fbstab_hip_dense_kkt_solve_batch", "fbstab_hip_dense_jacobian_batch"):
        assert name in hip_api.EXPORTED_SYMBOLS and getattr(lib, name).argtypes is not None, name
    assert hasattr(hip_api.FBstabDenseBatch, "KktSolve") and hasattr(hip_api.FBstabDenseBatch, "Jacobian")
    assert hip_api.FBstabDenseBatch.WRT == {"f": 1, "h": 3, "b": 5}   # FBSTAB_DENSE_f, _h, _b
    assert "dense_jacobian" in autograd.__all__ and "DETACHED" in autograd.dense_jacobian.__doc__


# What a machine without a GPU can ask of fbstab_hip_dense_kkt_solve_batch: no handle exists there, and what needs no
# handle is checked first - so each of these is refused for its own reason, before "null solver handle" and before any
# device call.  (stride, rhs_stride) of every slot: the default (64, 8) is in order for nrhs = 2.
_BAD = {
    "nrhs_0": (dict(nrhs=0), "fewer than one right-hand side"),
    "nrhs_negative": (dict(nrhs=-3), "fewer than one right-hand side"),
    "null_seed_block": (dict(null=("seed",)), "null seed or step block"),
    "null_step_block": (dict(null=("step",)), "null seed or step block"),
    "null_data_block": (dict(null=("data",)), "null argument"),
    "null_seed_z": (dict(seed_z=False), "null seed pointer (z)"),
    "seed_rhs_stride_below_the_length": (dict(seed=(64, 0)), "seed rhs_stride"),
    "step_rhs_stride_below_the_length": (dict(step=(64, 0)), "step rhs_stride"),
    "seed_stride_below_its_vectors": (dict(batch=2, nrhs=3, seed=(16, 8)), "seed stride"),
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


@pytest.mark.parametrize("wrt", [0, 2, 4, 6, -1], ids=["H", "G", "A", "NARR", "negative"])
def test_a_bad_wrt_is_refused_before_the_handle_is_looked_at(wrt):
    from fbstab_amd import hip_api
    lib = hip_api.load_library()
    rc, text = KH.handle_free_jacobian(lib, wrt)
    assert rc == 1 and "wrt must be" in text, (rc, text)


def test_jacobian_without_a_step_block_or_with_a_shared_one_is_refused():
    from fbstab_amd import hip_api
    lib = hip_api.load_library()
    rc, text = KH.handle_free_jacobian(lib, KH.WRT["b"], null=("step",))
    assert rc == 1 and "null step block" in text
    rc, text = KH.handle_free_jacobian(lib, KH.WRT["b"], batch=2, step=(0, 8))
    assert rc == 1 and "step stride" in text


@pytest.mark.parametrize("kw", [dict(), dict(batch=2), dict(batch=2, seed=(0, 8)), dict(nrhs=1, seed=(0, 0), step=(0, 0))],
                         ids=["valid", "batch2", "shared_seed", "one_rhs_ignores_rhs_stride"])
def test_calls_that_are_in_order_get_as_far_as_the_handle(kw):
    from fbstab_amd import hip_api
    lib = hip_api.load_library()
    assert KH.handle_free_kkt_solve(lib, **kw) == (1, "null solver handle")
    for wrt in ("f", "h", "b"):
        assert KH.handle_free_jacobian(lib, KH.WRT[wrt], batch=kw.get("batch", 1)) == (1, "null solver handle")
