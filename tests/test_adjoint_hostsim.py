"""CPU-only checks of the MPC adjoint (fbstab_hip_mpc_adjoint_batch): the export and the argument validation of
the C-ABI without a GPU, and the flat-vector adjoint of fb_mpc.h compiled single-threaded for the host
(tests/hostsim/adjoint.cc, against the shim hostsim.cc uses) against the oracle's linear solver."""
import ctypes as C

import numpy as np
import pytest

from fbstab_amd.hip_api import MPC_SEQ
from tools import fixtures as fx
from tests import helpers as H
from tests import linear_reference as LR
from tests.hostsim import HostAdjoint

@pytest.fixture(scope="module")
def host():
    return HostAdjoint()


def _problems(kats):
    out = [H.mpc_from_kat(k) for k in kats["mpc_end_to_end"]]
    out.append(fx.synthetic_mpc_batch(6))
    return out


def test_adjoint_residual_and_gradient_table_on_the_host(host, oracle, kats):
    """The device logic's (dz, dl, dv) leaves no more of V (dz, dl, dv) = (gz, -gl, -C.gv) than 3 x what the
    oracle's RiccatiLinearSolver leaves (longdouble residuals, at the oracle's solutions and at the origin), and
    its gradients are the table applied to its own adjoint."""
    rng = np.random.default_rng(31)
    checked = 0
    for p in _problems(kats):
        sol = oracle.solve_mpc(p)
        for q in range(p.batch):
            points = [(sol[0][q], sol[1][q], sol[2][q]), (np.zeros(p.nz), np.zeros(p.nl), np.zeros(p.nv))]
            for x in points:
                seeds = tuple(t[0] for t in LR.random_seeds(rng, p, 1))
                st, step, grads = host.adjoint(p, q, x, seeds)
                assert st == 0
                ref = LR.oracle_adjoint(oracle, p, q, x, seeds)
                r_dev = LR.adjoint_residual(p, q, x, step, seeds)
                r_orc = LR.adjoint_residual(p, q, x, ref, seeds)
                assert r_dev <= 3 * r_orc, (q, r_dev, r_orc)
                scale = max(np.abs(np.concatenate(step)).max(), 1.0)
                assert np.abs(np.concatenate(step) - np.concatenate(ref)).max() <= 1e-5 * scale  # (forward error: cond(V) ~ 1e11 at sigma = 1e-8)
                tab = LR.mpc_gradient_table(LR.one_qp(p, q), x, step)
                for k in MPC_SEQ:
                    np.testing.assert_allclose(grads[k], tab[k], rtol=1e-14, atol=1e-14 * scale, err_msg=k)
                checked += 1
    assert checked >= 2 * 7


def test_null_seeds_are_zero_and_unwanted_slots_are_not_written(host, oracle):
    p = fx.synthetic_mpc_batch(1)
    sol = oracle.solve_mpc(p)
    x = (sol[0][0], sol[1][0], sol[2][0])
    gz = np.random.default_rng(2).standard_normal(p.nz)
    st, a, g = host.adjoint(p, 0, x, (gz, None, None), want=("q", "E"))
    st0, b, g0 = host.adjoint(p, 0, x, (gz, np.zeros(p.nl), np.zeros(p.nv)), want=("q", "E"))
    assert st == st0 == 0 and set(g) == {"q", "E"}
    for s, t in zip(a, b):
        assert np.array_equal(s, t)
    assert np.array_equal(g["q"], g0["q"]) and np.array_equal(g["E"], g0["E"])


def test_factorisation_failure_gives_status_1_and_zero_gradients(host):
    """An indefinite stage Hessian (Q = -I) fails the Cholesky factorisation: status 1, every gradient and the
    adjoint zero."""
    p = fx.synthetic_mpc_batch(1)
    nx = p.nx
    p.arrays["Q"] = np.ascontiguousarray(np.tile(-np.eye(nx).reshape(-1), (1, p.N + 1)))
    x = (np.zeros(p.nz), np.zeros(p.nl), np.zeros(p.nv))
    st, step, grads = host.adjoint(p, 0, x, (np.ones(p.nz), np.ones(p.nl), np.ones(p.nv)))
    assert st == 1
    for t in step:
        assert np.array_equal(t, np.zeros_like(t))
    for k in MPC_SEQ:
        assert np.array_equal(grads[k], np.zeros_like(grads[k])), k


def test_adjoint_entry_point_is_exported_and_validates_without_gpu():
    from fbstab_amd import hip_api
    lib = hip_api.load_library()
    assert "fbstab_hip_mpc_adjoint_batch" in hip_api.EXPORTED_SYMBOLS
    b, x, s, g = hip_api._MpcBatch(), hip_api._VarBatch(), hip_api._VarBatch(), hip_api._MpcGradBatch()
    st = np.zeros(1, dtype=np.int32)
    rc = lib.fbstab_hip_mpc_adjoint_batch(None, 1, C.byref(b), C.byref(x), C.byref(s), 0.0, C.byref(g), None,
                                          st.ctypes.data, 0, None)
    assert rc == 1  # FBSTAB_HIP_ERR_ARGUMENT
    assert b"null solver handle" in lib.fbstab_hip_last_error()
    assert C.sizeof(hip_api._MpcGradBatch) == C.sizeof(hip_api._MpcBatch) == 12 * 16


_ENTRIES = ("adjoint_batch", "solve_batch")


@pytest.mark.parametrize("entry,case", [(e, c) for e in _ENTRIES for c in H.handle_free_cases(e)])
def test_mpc_bad_argument_calls_without_a_handle(entry, case):
    """tests/helpers.py: HANDLE_FREE_CASES on fbstab_hip_mpc_adjoint_batch and fbstab_hip_mpc_solve_batch.  Both
    look at the handle before anything else, so whatever else is wrong with the call the answer is the same one
    (recorded from the library as it was before the entry points shared their staging code)."""
    from fbstab_amd import hip_api
    lib = hip_api.load_library()
    assert H.handle_free_call(lib, "mpc", entry, **H.HANDLE_FREE_CASES[case]) == (1, "null solver handle")
