"""CPU-only checks of the dense adjoint (fbstab_hip_dense_adjoint_batch): the export and the argument validation
of the C-ABI without a GPU, and the adjoint of fb_dense.h with the contraction of fb_adjoint.h compiled
single-threaded for the host (tests/hostsim/dense_adjoint.cc, against the shim hostsim.cc uses) against the
oracle's linear solver and against central differences of active-set solves."""
import ctypes as C

import numpy as np
import pytest

from fbstab_amd.hip_api import DENSE_ARR
from tools import fixtures as fx
from tests import helpers as H
from tests import linear_reference as LR
from tests.hostsim import HostAdjoint

SHAPES = [(20, 5, 40), (30, 0, 40), (90, 20, 150)]
# the shapes on which the formulas were checked against central differences: with a quarter of the rows active
# (tools/fixtures.py: synthetic_dense_batch) fewer rows are active than there are variables
FD_SHAPES = [(20, 5, 40), (50, 10, 100), (30, 0, 40), (40, 8, 60), (56, 8, 128), (90, 20, 150)]


@pytest.fixture(scope="module")
def host():
    return HostAdjoint("dense")


def _problems(oracle, kats):
    out = []
    for k in kats["dense_end_to_end"]:
        p = H.dense_from_kat(k)
        if oracle.solve_dense(p)[4]["eflag"][0] == 0:
            out.append(p)
    assert len(out) >= 3
    out += [fx.synthetic_dense_batch(4, *s) for s in SHAPES]
    return out


def test_adjoint_residual_and_gradient_table_on_the_host(host, oracle, kats):
    """The device logic's (dz, dl, dv) leaves no more of V (dz, dl, dv) = (gz, -gl, -C.gv) than 3 x what the
    oracle's DenseCholeskySolver leaves (longdouble residuals, at the oracle's solutions and at the origin), and
    its six gradients are the table applied to its own adjoint."""
    rng = np.random.default_rng(41)
    checked = 0
    for p in _problems(oracle, kats):
        sol = oracle.solve_dense(p)
        assert (sol[4]["eflag"] == 0).all()
        for q in range(p.batch):
            points = [(sol[0][q], sol[1][q], sol[2][q]), (np.zeros(p.nz), np.zeros(p.nl), np.zeros(p.nv))]
            for x in points:
                seeds = tuple(t[0] for t in LR.random_seeds(rng, p, 1))
                st, step, grads = host.adjoint(p, q, x, seeds)
                assert st == 0
                ref = LR.oracle_adjoint(oracle, p, q, x, seeds)
                LR.check_step_and_table(p, q, x, seeds, step, grads, ref)
                checked += 1
    assert checked >= 2 * (3 + 4 * len(SHAPES))


def test_null_seeds_are_zero_and_unwanted_slots_are_not_written(host, oracle):
    p = fx.synthetic_dense_batch(1, 20, 5, 40)
    sol = oracle.solve_dense(p)
    x = (sol[0][0], sol[1][0], sol[2][0])
    gz = np.random.default_rng(2).standard_normal(p.nz)
    st, a, g = host.adjoint(p, 0, x, (gz, None, None), want=("f", "A"))
    st0, b, g0 = host.adjoint(p, 0, x, (gz, np.zeros(p.nl), np.zeros(p.nv)), want=("f", "A"))
    assert st == st0 == 0 and set(g) == {"f", "A"}
    for s, t in zip(a, b):
        assert np.array_equal(s, t) and np.abs(s).max() > 0
    assert np.array_equal(g["f"], g0["f"]) and np.array_equal(g["A"], g0["A"])


@pytest.mark.parametrize("shape", [(20, 5, 40), (30, 0, 40)])
def test_factorisation_failure_gives_status_1_and_zero_gradients(host, shape):
    """A NaN in H[0] is a NaN on the diagonal of K, which ends the factorisation by Eigen's rule
    (fb_dense.h: ldlt): status 1, every gradient and the adjoint zero."""
    p = fx.synthetic_dense_batch(1, *shape)
    p.arrays["H"] = p.arrays["H"].copy()
    p.arrays["H"][0, 0] = np.nan
    x = (np.zeros(p.nz), np.zeros(p.nl), np.zeros(p.nv))
    st, step, grads = host.adjoint(p, 0, x, (np.ones(p.nz), np.ones(p.nl), np.ones(p.nv)))
    assert st == 1
    for t in step:
        assert np.array_equal(t, np.zeros_like(t))
    for k in DENSE_ARR:
        assert np.array_equal(grads[k], np.zeros_like(grads[k])), k


@pytest.mark.parametrize("shape", FD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_central_differences_of_the_active_set_solution_map(host, shape):
    """On the generator's known solutions: QPs strictly complementary at 1e-3 with fewer than nz active rows plus
    equalities (at least 8 of 16).  For a random linear loss L = a'z + b'l + c'v, central differences of the
    active-set KKT solve along a random direction of each of the six arrays (symmetric for H) match the host
    adjoint's directional derivative to 1e-4."""
    nz, nl, nv = shape
    p = fx.synthetic_dense_batch(16, nz, nl, nv)
    z, l, v = (p.solution[k] for k in ("z", "l", "v"))
    strict = LR.strict_qps(p, z, v)
    assert len(strict) >= 8, len(strict)
    rng = np.random.default_rng(97)
    seeds = LR.random_seeds(rng, p)
    h = 1e-6
    worst = 0.0
    for q, act in strict:
        arr = {k: p.arrays[k][q] for k in DENSE_ARR}
        x0 = LR.active_set_solve(arr, nz, nl, nv, act)   # (the known solution, to rounding)
        assert max(np.abs(x0[0] - z[q]).max(), np.abs(x0[2] - v[q]).max()) <= 1e-9
        st, _, grads = host.adjoint(p, q, (z[q], l[q], v[q]), tuple(t[q] for t in seeds))
        assert st == 0
        dirs = LR.directions(rng, nz, nl, nv)
        loss = lambda x: sum(float(seeds[t][q] @ x[t]) for t in range(3))
        for k in DENSE_ARR:
            if dirs[k].size == 0:
                continue
            lp = loss(LR.active_set_solve({**arr, k: arr[k] + h * dirs[k]}, nz, nl, nv, act))
            lm = loss(LR.active_set_solve({**arr, k: arr[k] - h * dirs[k]}, nz, nl, nv, act))
            fd = (lp - lm) / (2 * h)
            ad = float(grads[k] @ dirs[k])
            bar = max(abs(ad), 1e-2 * np.abs(grads[k]).sum())
            worst = max(worst, abs(fd - ad) / bar)
            assert abs(fd - ad) <= 1e-4 * bar, (q, k, fd, ad)
    print("central differences", shape, "kept", len(strict), "worst relative error %.2e" % worst)


def test_adjoint_entry_point_is_exported_and_validates_without_gpu():
    """The checks that need no handle come first, so they can be exercised without a device: the required z seed,
    and strides below 1 on slots that are never empty; then the handle."""
    from fbstab_amd import hip_api
    lib = hip_api.load_library()
    assert "fbstab_hip_dense_adjoint_batch" in hip_api.EXPORTED_SYMBOLS
    assert C.sizeof(hip_api._DenseGradBatch) == C.sizeof(hip_api._DenseBatch) == 6 * 16
    buf = np.zeros(64)
    st = np.zeros(2, dtype=np.int32)

    def call(handle, batch, seed_z=True, x_stride=8, grad_stride=8):
        b, x, s, g = hip_api._DenseBatch(), hip_api._VarBatch(), hip_api._VarBatch(), hip_api._DenseGradBatch()
        for i in range(6):
            b.base[i], b.stride[i] = buf.ctypes.data, 8
        for i in range(3):
            x.base[i], x.stride[i] = buf.ctypes.data, x_stride
        if seed_z:
            s.base[0], s.stride[0] = buf.ctypes.data, 8
        g.base[1], g.stride[1] = buf.ctypes.data, grad_stride   # f_bar
        rc = lib.fbstab_hip_dense_adjoint_batch(handle, batch, C.byref(b), C.byref(x), C.byref(s), 0.0, C.byref(g),
                                                None, st.ctypes.data, 0, None)
        return rc, lib.fbstab_hip_last_error()

    rc, msg = call(None, 1)
    assert rc == 1 and b"null solver handle" in msg  # FBSTAB_HIP_ERR_ARGUMENT
    rc, msg = call(None, 1, seed_z=False)
    assert rc == 1 and b"null seed pointer (z)" in msg
    rc, msg = call(None, 2, x_stride=0)
    assert rc == 1 and b"variable stride smaller than the vector length" in msg
    rc, msg = call(None, 2, grad_stride=0)
    assert rc == 1 and b"gradient stride smaller than the array length" in msg
    rc, msg = call(None, 2)
    assert rc == 1 and b"null solver handle" in msg
    assert lib.fbstab_hip_dense_adjoint_batch(None, 1, None, None, None, 0.0, None, None, None, 0, None) == 1


# (rc, message) of every case of tests/helpers.py: HANDLE_FREE_CASES, recorded from the library as it was before
# the entry points shared their staging code.  fbstab_hip_dense_adjoint_batch checks what needs no handle first;
# fbstab_hip_dense_solve_batch looks at the handle before anything else.
_NO_HANDLE = (1, "null solver handle")
_HANDLE_FREE_EXPECTED = {
    "adjoint_batch": {
        "valid": _NO_HANDLE,
        "valid_batch2": _NO_HANDLE,
        "null_data": (1, "null argument"),
        "null_x": (1, "null argument"),
        "null_seed": (1, "null argument"),
        "null_grad": (1, "null argument"),
        "null_out": (1, "null argument"),
        "null_all": (1, "null argument"),
        "null_seed_z": (1, "null seed pointer (z)"),
        "null_seed_z_batch2": (1, "null seed pointer (z)"),
        "zero_data_stride": _NO_HANDLE,
        "zero_x_stride": (1, "variable stride smaller than the vector length"),
        "zero_seed_stride": (1, "seed stride smaller than the vector length"),
        "zero_grad_stride": (1, "gradient stride smaller than the array length"),
        "zero_adj_stride": (1, "adjoint stride smaller than the vector length"),
        "zero_strides": (1, "variable stride smaller than the vector length"),
        "zero_strides_batch1": _NO_HANDLE,
    },
    "solve_batch": {
        "valid": _NO_HANDLE,
        "valid_batch2": _NO_HANDLE,
        "null_data": _NO_HANDLE,
        "null_x": _NO_HANDLE,
        "null_out": _NO_HANDLE,
        "null_all": _NO_HANDLE,
        "zero_data_stride": _NO_HANDLE,
        "zero_x_stride": _NO_HANDLE,
        "zero_strides": _NO_HANDLE,
        "zero_strides_batch1": _NO_HANDLE,
    },
}


@pytest.mark.parametrize("entry,case", [(e, c) for e, t in _HANDLE_FREE_EXPECTED.items() for c in t])
def test_dense_bad_argument_calls_without_a_handle(entry, case):
    from fbstab_amd import hip_api
    assert set(_HANDLE_FREE_EXPECTED[entry]) == set(H.handle_free_cases(entry))
    lib = hip_api.load_library()
    rc, msg = H.handle_free_call(lib, "dense", entry, **H.HANDLE_FREE_CASES[case])
    assert (rc, msg) == _HANDLE_FREE_EXPECTED[entry][case]
