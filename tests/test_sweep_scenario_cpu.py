"""CPU-only checks of the scenario sweep (fbstab_hip_mpc_receding_sweep_scenario: a disturbed plant
x_(k+1) = A x_k + B u_k + w_k and a shifted warm start): the declaration, the export, the struct layout, the first
answer of the entry point without a device, the Python signatures, and dL/dw_k = mu_k - the costate the sweep
adjoint already logs - against central differences of the oracle's closed loop, with and without the shift."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from oracle.oracle_py import default_options
from tests import closed_loop as CL
from tests import sweep_adjoint_helpers as SH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "fbstab_hip_mpc_receding_sweep_scenario"


def test_header_declares_and_library_exports_the_entry_point():
    from fbstab_amd import hip_api
    text = open(os.path.join(ROOT, "include", "fbstab_hip.h")).read()
    assert re.search(r"\bint\s+" + NAME + r"\s*\(", text)
    m = re.search(r"typedef struct fbstab_sweep_scenario_t \{(.*?)\} fbstab_sweep_scenario_t;", text, re.S)
    assert m and re.search(r"const double\*\s*w;", m.group(1)) and re.search(r"\bint shift;", m.group(1))
    assert NAME in hip_api.EXPORTED_SYMBOLS
    getattr(hip_api.load_library(), NAME)


def test_scenario_struct_layout():
    from fbstab_amd import hip_api
    S = hip_api._SweepScenario
    assert S.w.offset == 0 and S.shift.offset == 8 and C.sizeof(S) == 16


def test_null_handle_is_an_argument_error_without_a_device():
    from fbstab_amd import hip_api
    lib = hip_api.load_library()
    sc = hip_api._SweepScenario(None, 1)
    ARG = 1  # FBSTAB_HIP_ERR_ARGUMENT
    for scenario in (None, C.byref(sc)):
        assert getattr(lib, NAME)(None, 1, None, None, None, None, 1, 1, None, None, None, None, None, scenario) == ARG
        assert b"null solver handle" in lib.fbstab_hip_last_error()


def test_python_entry_points_take_w_and_shift():
    from fbstab_amd import autograd, hip_api
    for fn in (autograd.closed_loop_mpc, hip_api.FBstabMpcBatch.RecedingSweep):
        par = inspect.signature(fn).parameters
        assert par["w"].default is None and par["shift"].default is False, fn
    # the calls that exist keep their meaning: nothing moved in front of the new arguments
    names = list(inspect.signature(autograd.closed_loop_mpc).parameters)
    assert names[:7] == ["solver", "data", "A", "B", "steps", "retire", "sigma"]


@pytest.mark.parametrize("shift", [False, True], ids=["unshifted", "shifted"])
def test_costate_is_the_disturbance_gradient_on_the_oracles_loop(oracle, shift):
    """sweep_adjoint_helpers.fd_problem() at abs_tol = 1e-11 with w = 1e-2 N(0, 1) from seed 77: central differences
    (h = 1e-5) of L = <cu, u> + <cx, x> along one random direction of w, against <mu, direction> with mu from the
    unchanged backward recursion on the disturbed (and shifted) loop's log, under the sweep adjoint's rule
    |fd - ad| <= 1e-4 max(|ad|, 1e-2 sum|grad|), on every trajectory that is strictly complementary at every step:
    7 of the 8."""
    p, A, B, cu, cx, dirs = SH.fd_problem()
    N, nx, nu, nc = p.sizes()
    o = default_options(abs_tol=1e-11)
    rng = np.random.default_rng(77)
    w = 1e-2 * rng.standard_normal((SH.FD_STEPS, SH.FD_TRAJ, nx))
    dw = rng.standard_normal(w.shape)
    solve = CL.oracle_solve(oracle, p, o)
    log = CL.logged_closed_loop(solve, p, A, B, SH.FD_STEPS, w=w, shift=shift)
    good = SH.strictly_complementary(p, log)
    assert len(good) == 7, good
    grads, status, mu = SH.reference_sweep_adjoint(SH.oracle_step_adjoint(oracle, p), p, A, B, log, cu, cx)
    assert (status == 0).all()
    gw = np.where((log["eflag"] == -1)[:, :, None], 0.0, mu)

    def loss(wk):
        r = CL.logged_closed_loop(solve, p, A, B, SH.FD_STEPS, w=wk, shift=shift)
        x = np.concatenate([r["x"][1:], r["x_end"][None]], 0)
        return (cu * r["u"]).sum(axis=(0, 2)) + (cx * x).sum(axis=(0, 2))

    fd = (loss(w + SH.FD_H * dw) - loss(w - SH.FD_H * dw)) / (2 * SH.FD_H)
    figures = []
    for q in good:
        ad = float((gw[:, q] * dw[:, q]).sum())
        figures.append((q, fd[q], ad, 1e-4 * max(abs(ad), 1e-2 * np.abs(gw[:, q]).sum())))
    for q, f, ad, bound in figures:
        print(f"w   q {q} shift {int(shift)} fd {f:+.9e} ad {ad:+.9e} |fd-ad| {abs(f - ad):.2e} bound {bound:.2e}")
    for q, f, ad, bound in figures:
        assert abs(f - ad) <= bound, (q, f, ad, bound)
