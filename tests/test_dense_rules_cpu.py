"""The rules of tests/dense_rules.py without a GPU: the path map from the compiled DenseLayout::init, the float64
restatements of every stage of fb_dense.h through the same rules the device is held to, a seeded defect per rule,
and the real header on one host thread (tests/hostsim/dense_stage.cc: DenseProblem<Ctx<1>>, the scalar assembly,
ldlt_impl, ldlt_solve_impl) - which shows the rules are not too tight for the actual code before anything reaches
a GPU - once more under the address and undefined-behaviour sanitizers as a stand-alone program."""
import itertools
import os
import subprocess

import numpy as np
import pytest

from tests import dense_rules as dr
from tests import dense_wave_rules as wr
from tests.hostsim import HostDenseStage, NO_CONTRACTION

GRID_NZ = (1, 2, 15, 16, 17, 20, 33, 40, 48, 49, 63, 64, 65, 66, 90, 96, 120, 128, 129, 130, 140, 257)
GRID_NL = (0, 1, 3, 5, 6, 12, 16, 19, 30, 32)
GRID_NV = (1, 2, 3, 4, 5, 7, 8, 12, 16, 30, 40, 64, 65, 68, 132, 330, 2435, 2497, 2534, 4000)


@pytest.fixture(scope="module")
def host():
    return HostDenseStage()


def _worst(rules, where):
    print("%s: %s" % (where, "  ".join("%s %.3f" % kv for kv in rules.items())))
    return max(rules.values()) if rules else 0.0


def _assert_all(rules, where):
    _worst(rules, where)
    for rule, worst in rules.items():
        assert worst <= 1.0, (where, rule, worst)


# ---- the path map ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def grid(host):
    out = {}
    for nz, nl, nv, want in itertools.product(GRID_NZ, GRID_NL, GRID_NV, (256, 64)):
        out[(nz, nl, nv, want)] = dr.path_of(host.layout, nz, nl, nv, want)
    return out


def test_every_device_shape_takes_the_path_its_test_names(host):
    for key, shapes in dr.STEP_SHAPES.items():
        for shape in shapes:
            assert dr.path_key(dr.path_of(host.layout, *shape, key[0])) == key, (shape, key)
    for name, cases in dr.FACTOR_CASES.items():
        for n, nv, want in cases:
            assert dr.path_key(dr.path_of(host.layout, n, 0, nv, want), False) == dr.FACTOR_PATHS[name], (name, n, nv)
    family_ns = {n for n, _, _, _ in dr.tied_images()} | {n for n, _, _ in dr.singular_images()}
    for n in sorted(family_ns | {dr.denormal_pivot_image()[0]}):
        for nv, want, rows in dr.FAMILY_PATHS:
            p = dr.path_of(host.layout, n, 0, nv, want)
            assert (p["threads"], p["factorisation"], p["substitution"]) == \
                ((want, "rows", "rows") if rows else (256, "impl", "wave")), (n, nv, want, p)
    for (shape, want), (placement, a_lds) in zip(dr.FEASIBILITY_CASES, dr.FEASIBILITY_PLACEMENTS):
        p = dr.path_of(host.layout, *shape, want)
        assert (p["placement"], p["a_lds"], p["threads"]) == (placement, a_lds, want), (shape, p)


def test_every_reachable_path_has_a_device_shape(grid):
    reached = {}
    for key, p in grid.items():
        reached.setdefault(dr.path_key(p), key)
    table = sorted(reached.items())
    print("\n".join("%-48s first at %s" % kv for kv in table))
    missing = {k: v for k, v in reached.items() if k not in dr.STEP_SHAPES}
    assert not missing, missing
    factor_paths = set(dr.FACTOR_PATHS.values())
    for k in reached:
        assert any(f[1:3] == k[2:4] for f in factor_paths), ("no `factor` size for", k)


def test_ldlt_fused_is_reached_by_no_shape(grid):
    """`init` clears `wave` only on its way to k_global, and `ldlt` takes ldlt_fused only when K is in LDS, the layout
    is not `wave` and nk <= 64: with nk <= 64, not `wave` means k_global."""
    assert not [k for k, p in grid.items() if p["factorisation"] == "fused"]


def test_the_invariant_behind_ldlt_fused(host):
    for nz, nl, nv, nt in itertools.product(GRID_NZ, GRID_NL, GRID_NV, (256, 64)):
        lay = host.layout(nz, nl, nv, nt)
        if nz + nl <= 64:
            assert lay["wave"] or lay["k_global"], (nz, nl, nv, nt)
        else:
            assert not lay["wave"]
        assert lay["lda"] == nv | 1 and (not lay["a_lds"] or not lay["k_global"])


# ---- the inputs of the order assertions ----------------------------------------------------------------------------------
def _order_inputs():
    for name, cases in dr.FACTOR_CASES.items():
        rows = dr.FACTOR_PATHS[name][1] == "rows"
        for n, _, _ in cases:
            K, _ = dr.images(n)
            for q in range(K.shape[0]):
                yield ("images", n, q), K[q], rows
    for n, img, _, name in dr.tied_images():
        for rows in (True, False):
            yield ("tied", name), img[0][:n, :n], rows
        yield ("tied in 66", name), dr.embed(img[0], n, 66), False
    yield ("handover",), dr.handover_image()[0][0], False


def test_no_close_step_in_the_inputs_of_the_order_assertions():
    for where, K, rows in _order_inputs():
        assert dr.close_share(K, rows) == 0.0, where


def test_orders_on_the_tied_family_against_eigen():
    """Reported, and pinned: neither variant follows Eigen's order on the whole tied family (both search the
    UPDATED diagonal, Eigen the assembled one)."""
    same = {True: [], False: []}
    for n, img, _, name in dr.tied_images():
        K = img[0][:n, :n]
        for rows in (True, False):
            mine = dr.elimination_order(dr.order_restated(K, rows), rows)
            same[rows].append(bool(np.array_equal(mine, dr.eigen_order(K))))
            print("tied '%s': %s order %s Eigen's" % (name, "ldlt_rows" if rows else "ldlt_impl",
                                                      "is" if same[rows][-1] else "is NOT"))
    assert not all(same[True]) and not all(same[False])


def test_ldlt_impl_order_is_the_updated_diagonal_by_position():
    """ldlt_impl's swaps restated against the swap-free statement of its rule: the updated diagonal, the first
    maximum by CURRENT position, no column check."""
    rule = wr.Defect(updated_diagonal=True, no_column_check=True)
    for where, K, rows in _order_inputs():
        if rows or K.shape[0] > 64:
            continue
        n = K.shape[0]
        want = wr.factor_restated(wr.pad64(dr.mirrored(K)), n, rule)[3][:n]
        assert np.array_equal(dr.elimination_order(dr.order_restated(K, False), False), want), where


# ---- the restatements pass every rule ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", dr.STEP_CASES, ids=str)
def test_step_restated_passes(host, case):
    shape, want = case
    path = dr.path_of(host.layout, *shape, want)
    rows = path["factorisation"] == "rows"
    for sigma in dr.SIGMAS:
        for adjoint in (False, True):
            d, xb = dr.step_inputs(*shape, sigma, adjoint)
            got = dr.step_restated(d, xb, sigma, path, adjoint=adjoint)
            _assert_all(dr.step_rules(d, xb, sigma, got, rows, adjoint=adjoint), ("restated", shape, want, sigma, adjoint))
            lo, hi = got["gam"].min(), got["gam"].max()
            if shape[2] >= 2 and not adjoint:
                assert lo <= 1e-11 and hi >= min(1e7, 0.3 / sigma), (shape, sigma, lo, hi)


def _factor_cases():
    return [(name, n, want) for name, cases in dr.FACTOR_CASES.items() for n, _, want in cases]


@pytest.mark.parametrize("case", _factor_cases(), ids=str)
def test_factor_restated_passes(case):
    name, n, want = case
    rows = dr.FACTOR_PATHS[name][1] == "rows"
    K, b = dr.images(n)
    for q in range(K.shape[0]):
        got = dr.factor_restated(K[q], b[q], rows, want)
        assert got["verdict"][0] == 1
        _assert_all(dr.image_rules(K[q], b[q], got, 0, rows), ("restated", name, n, q))


def test_families_restated():
    for rows in (True, False):
        for n, img, b, name in dr.tied_images():
            K = img[0][:n, :n]
            got = dr.factor_restated(K, b[0][:n], rows)
            _assert_all(dr.image_rules(K, b[0][:n], got, 0, rows), ("tied", name, rows))
        n, img, b, j = dr.denormal_pivot_image()
        got = dr.factor_restated(img[0][:n, :n], b[0][:n], rows)
        assert got["verdict"][0] == 1 and got["x"][0, j] == 0.0
        for n, img, name in dr.singular_images():
            got = dr.factor_restated(img[:n, :n], np.zeros(n), rows)
            documented = wr.factor_restated(img, n, wr.DEVICE_AS_DOCUMENTED)[0]
            assert bool(got["verdict"][0]) == documented, (name, rows)  # (the two variants agree on this family)


# ---- every seeded defect fails a rule ------------------------------------------------------------------------------------
def _step_fails(host, shape, want, defect, sigma=1e-8, adjoint=False):
    path = dr.path_of(host.layout, *shape, want)
    d, xb = dr.step_inputs(*shape, sigma, adjoint)
    got = dr.step_restated(d, xb, sigma, path, adjoint=adjoint, defect=defect)
    return _worst(dr.step_rules(d, xb, sigma, got, path["factorisation"] == "rows", adjoint=adjoint),
                  ("defect", shape, vars(defect)))


def test_assembly_defects_fail(host):
    """A skipped tile, a missing Gamma and a wrong read-side lda break the composite rule on both factorisations;
    a chunk that writes all its columns is caught by the sentinel above the diagonal."""
    for shape in ((33, 3, 16), (40, 30, 8)):  # mfma with rows, mfma with impl; nz is no multiple of 16
        assert _step_fails(host, shape, 256, dr.Defect(skip_last_row_tile=True)) > 1.0
        assert _step_fails(host, shape, 256, dr.Defect(gamma_missing=True)) > 1.0
        assert _step_fails(host, shape, 256, dr.Defect(lda_read_nv=True)) > 1.0
    for shape in ((63, 1, 3), (64, 1, 30)):  # lds with rows, lds with impl
        assert _step_fails(host, shape, 256, dr.Defect(gamma_missing=True)) > 1.0
    assert _step_fails(host, (64, 6, 68), 256, dr.Defect(gamma_missing=True)) > 1.0  # global
    # nv even: lda = nv + 1 differs from nv (an odd nv is its own lda: the defect does not exist there)
    assert _step_fails(host, (64, 1, 30), 256, dr.Defect(lda_read_nv=True)) > 1.0
    assert _step_fails(host, (64, 1, 30), 256, dr.Defect(chunk_writes_all=True)) > 1.0
    assert _step_fails(host, (90, 5, 3), 256, dr.Defect(chunk_writes_all=True)) > 1.0


def test_a_padded_column_from_column_0_changes_no_output(host):
    """The one seeded defect no rule CAN catch, and why: entry (i, j) of the tile product depends on columns i and j
    of the operands alone, a padded column therefore only on entries with i >= nz or j >= nz, and those the write
    mask (i < nz, j <= i) discards.  The clamp to nz - 1 only has to stay inside the LDS copy of A; column 0 does
    too.  Pinned as what it is: bit-identical outputs."""
    shape = (33, 3, 16)
    path = dr.path_of(host.layout, *shape, 256)
    d, xb = dr.step_inputs(*shape, 1e-8)
    a = dr.step_restated(d, xb, 1e-8, path)
    b = dr.step_restated(d, xb, 1e-8, path, defect=dr.Defect(pad_from_column_0=True))
    for k in a:
        assert np.array_equal(dr._bits(a[k]), dr._bits(b[k])), k


def test_factorisation_defects_fail():
    K, b = dr.images(66)
    got = dr.factor_restated(K[1], b[1], False, defect=dr.Defect(skip_middle_segment=True))
    assert _worst(dr.image_rules(K[1], b[1], got, 0, False), "middle segment") > 1.0
    got = dr.factor_restated(K[1], b[1], False, defect=dr.Defect(forward_undo=True))
    assert _worst(dr.image_rules(K[1], b[1], got, 0, False), "forward undo") > 1.0
    # the handover: the factors are valid LDL' factors of another order - only the order rule sees it
    Kh, bh = dr.handover_image()
    good = dr.ldlt_impl_restated(Kh[0], 256)[1]
    bad = dr.ldlt_impl_restated(Kh[0], 256, dr.Defect(handover_off_by_one=True))[1]
    assert good[64] == 128 and bad[64] == 64
    # ... and at 64 threads there is no handover to get wrong
    assert np.array_equal(dr.ldlt_impl_restated(Kh[0], 64, dr.Defect(handover_off_by_one=True))[1],
                          dr.ldlt_impl_restated(Kh[0], 64)[1])
    n, img, rhs, j = dr.denormal_pivot_image()
    for rows in (True, False):
        got = dr.factor_restated(img[0][:n, :n], rhs[0][:n], rows, defect=dr.Defect(pinv_threshold_zero=True))
        assert got["x"][0, j] != 0.0


# ---- the real header on one thread ---------------------------------------------------------------------------------------
HOST_STEP_SHAPES = [(1, 0, 1), (2, 1, 1), (16, 3, 8), (33, 3, 16), (40, 30, 8), (64, 1, 30), (64, 6, 68), (20, 5, 330),
                    (129, 12, 5), (20, 5, 2534)]


@pytest.mark.parametrize("shape", HOST_STEP_SHAPES, ids=str)
def test_the_header_on_one_thread_passes_the_step_rules(host, shape):
    """DenseProblem<Ctx<1>>: the LDS-scalar or the global assembly (FB_DENSE_NO_MFMA), ldlt_impl, ldlt_solve_impl,
    newton_step<false> and dense_adjoint, in every placement; and an H with a NaN upper triangle in the step changes
    no bit but wz."""
    for sigma in dr.SIGMAS:
        for adjoint in (False, True):
            d, xb = dr.step_inputs(*shape, sigma, adjoint)
            got = host.step(d, xb, sigma, adjoint=adjoint)
            _assert_all(dr.step_rules(d, xb, sigma, got, False, adjoint=adjoint), ("host", shape, sigma, adjoint))
            again = host.step(d, xb, sigma, adjoint=adjoint, h_step=dr.with_nan_upper(d["H"]))
            for k in got:
                if k != "wz" and shape[0] > 1:
                    assert np.array_equal(dr._bits(got[k]), dr._bits(again[k])), (shape, sigma, k)


def test_the_header_on_one_thread_passes_the_image_rules(host):
    for n in (1, 2, 33, 65, 66, 130):
        K, b = dr.images(n)
        got = host.factor(K, b)
        assert (got["verdict"] == 1).all()
        for q in range(K.shape[0]):
            _assert_all(dr.image_rules(K[q], b[q], got, q, False), ("host", n, q))
            want = dr.order_restated(K[q], False, nt=1)
            assert np.array_equal(got["perm"][q], want), (n, q)
    for n, img, b, name in dr.tied_images():
        K = img[:, :n, :n]
        got = host.factor(K, b[:, :n])
        _assert_all(dr.image_rules(K[0], b[0, :n], got, 0, False), ("host tied", name))
        assert np.array_equal(got["perm"][0], dr.order_restated(K[0], False, nt=1)), name
    n, img, b, j = dr.denormal_pivot_image()
    got = host.factor(img[:, :n, :n], b[:, :n])
    assert got["verdict"][0] == 1 and got["x"][0, j] == 0.0 and not np.signbit(got["x"][0, j])
    for n, img, name in dr.singular_images():
        got = host.factor(img[None, :n, :n], np.zeros((1, n)))
        assert bool(got["verdict"][0]) == dr.ldlt_impl_restated(img[:n, :n], 1)[0], name


def test_the_stand_alone_driver_runs_clean_under_the_sanitizers(tmp_path):
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim")
    exe = str(tmp_path / "dense_stage_sanitized")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", NO_CONTRACTION, "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-DDENSE_STAGE_MAIN", "-I" + os.path.join(here, "shim"),
                           "-Wno-attributes", "-Wno-unknown-pragmas", "-o", exe, os.path.join(here, "dense_stage.cc")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr
