"""GPU tests of the cooperative line-search pass of the record kernels at K step lengths per pass
(kCoopLineSearchTrials, fb_algorithm.h): a Newton step that fails f sufficient-decrease tests takes ceil(f / K)
passes, and the trial after the last ALLOWED test is taken as it is, whatever max_linesearch_iters is against K.

Every case solves host-pointer batches twice - SPREAD (one QP per wavefront: a pass has one owner) and under
FBSTAB_HIP_MAX_WORKGROUPS=2 at handle creation (every row busy: several rows search after a Newton step and their
passes follow each other) - requires the two bitwise equal and holds them to the strict rule of
test_gpu_parity.py::test_line_search_trial_limits_on_the_record_kernel against the oracle: exit flags, Newton and
proximal counts equal, solutions within 10 abs_tol (1 + |z|_inf) where the oracle converged.

Coverage is a condition: each case takes the histogram of f of ITS input from the oracle's trace
(tools/line_search_lengths.py) and asserts steps with one pass (f in [1, K]) and with two (f in [K + 1, 2 K]);
the N = 30 case also steps with more (f in (2 K, 20]).  K is read from the header, so the cases move with it."""
import os
import re

import numpy as np
import pytest

from tools import fixtures as fx
from tools import line_search_lengths as lsl
from oracle.oracle_py import default_options
from tests.helpers import _opts, OUT_FIELDS

pytestmark = pytest.mark.gpu

CAP = "FBSTAB_HIP_MAX_WORKGROUPS"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _shipped_k():
    """kCoopLineSearchTrials as the header states it."""
    with open(os.path.join(ROOT, "fbstab_amd", "csrc", "fb_algorithm.h")) as fh:
        m = re.search(r"constexpr int kCoopLineSearchTrials = (\d+);", fh.read())
    assert m, "fb_algorithm.h: kCoopLineSearchTrials not found"
    return int(m.group(1))


K = _shipped_k()


@pytest.fixture(scope="module")
def hip():
    from fbstab_amd import hip_api
    assert hip_api.load_library().fbstab_hip_device_count() >= 1
    return hip_api


def _solve(hip, monkeypatch, p, o, cap):
    """One host-pointer batch on a fresh handle -> ((z, l, v, y, out), kernel name, workgroups)."""
    if cap is None:
        monkeypatch.delenv(CAP, raising=False)
    else:
        monkeypatch.setenv(CAP, str(cap))
    s = hip.FBstabMpcBatch(*p.sizes(), max_batch=p.batch)
    monkeypatch.delenv(CAP, raising=False)
    s.UpdateOptions(_opts(hip, o))
    B = p.batch
    z = np.zeros((B, p.nz)); l = np.zeros((B, p.nl)); v = np.zeros((B, p.nv)); y = np.zeros((B, p.nv))
    out = s.Solve({k: np.ascontiguousarray(a) for k, a in p.arrays.items()}, z, l, v, y)
    name, wgs = s.kernel_name(), s.query()["workgroups"]
    s.close()
    return (z, l, v, y, out), name, wgs


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _check(hip, monkeypatch, oracle, p, o, kernel):
    spread, name, wgs = _solve(hip, monkeypatch, p, o, None)
    assert name == kernel and wgs == p.batch, (name, wgs)
    packed, name, wgs = _solve(hip, monkeypatch, p, o, 2)
    assert name == kernel and wgs == 2, (name, wgs)
    for what, a, b in zip("zlvy", spread[:4], packed[:4]):
        assert np.array_equal(_bits(a), _bits(b)), (what, np.nonzero((_bits(a) != _bits(b)).any(axis=1))[0])
    for f in OUT_FIELDS:
        assert np.array_equal(_bits(spread[4][f]), _bits(packed[4][f])), f
    cpu = oracle.solve_mpc(p, opts=o, nthreads=oracle.num_threads())
    assert np.array_equal(spread[4]["eflag"], cpu[4]["eflag"])
    dn = np.abs(spread[4]["newton_iters"].astype(int) - cpu[4]["newton_iters"].astype(int))
    assert dn.max() == 0, ((dn != 0).sum(), dn.max())
    assert np.array_equal(spread[4]["prox_iters"], cpu[4]["prox_iters"])
    ok = cpu[4]["eflag"] == 0
    scale = 1.0 + np.abs(cpu[0]).max(axis=1, keepdims=True)
    assert (np.abs(spread[0] - cpu[0])[ok] <= 10 * o.abs_tol * scale[ok]).all()


def _count(f, lo, hi):
    return int(((f >= lo) & (f <= hi)).sum())


def _assert_covered(f, three_passes=False):
    """Steps with one pass and with two (and with three) at the shipped K, by the oracle's trace."""
    assert _count(f, 1, K) >= 1, np.bincount(f)
    assert _count(f, K + 1, 2 * K) >= 1, np.bincount(f)
    if three_passes:
        assert _count(f, 2 * K + 1, 20) >= 1, np.bincount(f)


# -- max_linesearch_iters around the multiples of K ------------------------------------------------
@pytest.fixture(scope="module")
def headline_batch(oracle):
    p = fx.synthetic_mpc_batch(32, first_id=52000)
    return p, lsl.fails_of_problem(oracle, p)


@pytest.mark.parametrize("max_ls", sorted({0, 1, K - 1, K, K + 1, 2 * K - 1, 2 * K, 2 * K + 1, 20}))
def test_trial_limits_below_at_and_between_multiples_of_the_pass_width(hip, oracle, monkeypatch, headline_batch, max_ls):
    p, f = headline_batch
    # (the input's own histogram, default options: 118 / 175 / 53 / 6 steps with f in 1-4 / 5-8 / 9-16 / 17-20)
    _assert_covered(f, three_passes=True)
    _check(hip, monkeypatch, oracle, p, default_options(max_linesearch_iters=max_ls), "fbstab_mpc_r16_kernel<12,4,20>")


# -- fewer stages than rows (N = 1, 2), exactly one trip (N = 3), a last trip with idle rows (N = 4) -----------
@pytest.mark.parametrize("N", [1, 2, 3, 4])
def test_horizons_of_one_trip_and_less(hip, oracle, monkeypatch, N):
    p = fx.random_ltv_mpc_bounds(np.random.default_rng(11), 48, N, 12, 4, 20)
    f = lsl.fails_of_problem(oracle, p)
    _assert_covered(f)  # (N = 1: 14 steps with f in 1-4 and 4 with f in 5-8; N = 2, 3, 4 reach f in 9-16 as well)
    _check(hip, monkeypatch, oracle, p, default_options(), "fbstab_mpc_r16_kernel<12,4,20>")


# -- every other record instance ---------------------------------------------------------------------
# (seeds: the first from 11 upwards with which the 48 QPs reach f = 20 on the CPU - 13 for <12,4,32>, 11 for the others)
@pytest.mark.parametrize("shape,seed,kernel", [((5, 10, 3, 25), 13, "fbstab_mpc_r16_kernel<12,4,32>"),
                                               ((6, 18, 5, 10), 11, "fbstab_mpc_r32_kernel<18,5,10>"),
                                               ((5, 20, 6, 16), 11, "fbstab_mpc_r32_kernel<24,8,16>"),
                                               ((5, 24, 8, 32), 11, "fbstab_mpc_r32_kernel<24,8,32>")])
def test_every_record_instance(hip, oracle, monkeypatch, shape, seed, kernel):
    p = fx.random_ltv_mpc_bounds(np.random.default_rng(seed), 48, *shape)
    f = lsl.fails_of_problem(oracle, p)
    _assert_covered(f)
    assert f.max() == 20, np.bincount(f)
    _check(hip, monkeypatch, oracle, p, default_options(), kernel)
