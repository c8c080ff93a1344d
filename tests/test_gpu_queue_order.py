"""GPU tests of the longest-first queue of a record handle (fbstab_amd/csrc/fb_queue_order.h, fb_queue_order_plan.h):
behind a packed batch solve one workgroup sorts the QP indices by the Newton counts the solve wrote, and the next
solve of the same batch size hands its queue tickets out in that order.

The order is a hint: a QP's bits depend on nothing but the QP (tests/test_gpu_queue.py), so
every ordered solve is compared BITWISE with the same solve on a handle created under FBSTAB_HIP_QUEUE_ORDER=0, and
with the oracle's flags and counts at the strict bar.  The test knob FBSTAB_HIP_MAX_WORKGROUPS caps the grids at
two workgroups, so that every row re-fetches and the order decides which row meets which QP."""
import numpy as np
import pytest

from tools import fixtures as fx
from oracle.oracle_py import default_options
from tests.helpers import _opts, OUT_FIELDS

pytestmark = pytest.mark.gpu

CAP = "FBSTAB_HIP_MAX_WORKGROUPS"
KNOB = "FBSTAB_HIP_QUEUE_ORDER"
W = 2  # workgroups of every capped handle below


@pytest.fixture(scope="module")
def hip():
    from fbstab_amd import hip_api
    assert hip_api.load_library().fbstab_hip_device_count() >= 1
    return hip_api


def _rows(kernel):
    """QPs one workgroup holds at a time: four 16-lane rows, or two row pairs."""
    return 4 if "r16" in kernel else 2


# (id, kernel, problem): the BASELINE shape at N = 6 with at least four fetches per row, and once per other record
# instance (and on a padded shape) N = 4 and B = 2 x rows + 3
def _problem(which):
    rng = np.random.default_rng(13000)
    if which == "headline":
        return fx.synthetic_mpc_batch(37, N=6)
    if which == "boxed":
        return fx.boxed_mpc_batch(2 * W * 4 + 3, N=4)
    shape = {"18x5x10": (18, 5, 10), "20x6x16": (20, 6, 16), "20x6x30": (20, 6, 30), "padded": (10, 3, 14)}[which]
    rows = W * (4 if which == "padded" else 2)
    return fx.random_ltv_mpc(rng, 2 * rows + 3, 4, *shape)


CASES = [("headline", "fbstab_mpc_r16_kernel<12,4,20>"), ("boxed", "fbstab_mpc_r16_kernel<12,4,32>"),
         ("18x5x10", "fbstab_mpc_r32_kernel<18,5,10>"), ("20x6x16", "fbstab_mpc_r32_kernel<24,8,16>"),
         ("20x6x30", "fbstab_mpc_r32_kernel<24,8,32>"), ("padded", "fbstab_mpc_r16_kernel<12,4,20>")]


def _handle(hip, monkeypatch, p, ordered, cap=W, max_batch=None):
    """A handle for `p` whose grid is capped at `cap` workgroups, with the queue order on or off."""
    monkeypatch.setenv("FBSTAB_HIP_GENERIC", "0")
    monkeypatch.setenv(CAP, str(cap))
    if ordered:
        monkeypatch.delenv(KNOB, raising=False)
    else:
        monkeypatch.setenv(KNOB, "0")
    s = hip.FBstabMpcBatch(*p.sizes(), max_batch=max_batch or p.batch)
    monkeypatch.delenv(CAP)
    monkeypatch.delenv(KNOB, raising=False)
    s.UpdateOptions(_opts(hip, default_options()))
    assert s.query()["workgroups"] == cap
    return s


def _solve(s, p, B=None):
    """The first B QPs of `p` from the zero guess, host arrays: (z, l, v, y, out)."""
    B = B or p.batch
    z = np.zeros((B, p.nz)); l = np.zeros((B, p.nl)); v = np.zeros((B, p.nv)); y = np.zeros((B, p.nv))
    out = s.Solve({k: np.ascontiguousarray(a[:B]) for k, a in p.arrays.items()}, z, l, v, y)
    return z, l, v, y, out


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _assert_same_bits(a, b, what):
    """z, l, v, y and every SolverOut field but solve_time bitwise equal."""
    for name, x, y_ in zip("zlvy", a[:4], b[:4]):
        assert np.array_equal(_bits(x), _bits(y_)), (what, name)
    for f in OUT_FIELDS:
        assert np.array_equal(_bits(a[4][f]), _bits(b[4][f])), (what, f, a[4][f], b[4][f])


def _assert_is_the_order_of(order, counts, what):
    """`order`: a permutation of the batch along which `counts` do not increase, indices ascending inside equal
    counts - the stable descending sort of the counts clamped to [0, 255], and nothing else."""
    n = len(counts)
    assert order.shape == (n,) and np.array_equal(np.sort(order), np.arange(n)), (what, order)
    key = np.clip(counts, 0, 255)[order]
    assert (np.diff(key) <= 0).all(), (what, key)
    assert (np.diff(order)[np.diff(key) == 0] > 0).all(), (what, order, key)
    assert np.array_equal(order, np.argsort(-np.clip(counts, 0, 255), kind="stable")), what


@pytest.mark.parametrize("which,kern", CASES, ids=[c[0] for c in CASES])
def test_the_order_is_the_sorted_counts_and_an_ordered_solve_has_the_bits_of_an_unordered_one(hip, oracle, monkeypatch,
                                                                                              which, kern):
    """One solve installs the order (a permutation, counts non-increasing along it, indices ascending inside equal
    counts); a repeat solve runs by it and leaves the same array; the ordered solve is bitwise the solve of a
    handle without the order, and strict against the oracle."""
    p = _problem(which)
    B = p.batch
    s = _handle(hip, monkeypatch, p, ordered=True)
    assert s.kernel_name() == kern and B >= 2 * W * _rows(kern) + 3
    assert s.queue_order().size == 0
    first = _solve(s, p)
    order = s.queue_order()
    _assert_is_the_order_of(order, first[4]["newton_iters"], "first")
    assert len(set(first[4]["newton_iters"].tolist())) > 1, "a batch of equal counts orders nothing"
    second = _solve(s, p)
    assert np.array_equal(s.queue_order(), order)
    s.close()
    s0 = _handle(hip, monkeypatch, p, ordered=False)
    plain = _solve(s0, p)
    assert s0.queue_order().size == 0
    s0.close()
    _assert_same_bits(first, plain, "first (index order)")
    _assert_same_bits(second, plain, "second (ordered)")
    oc = oracle.solve_mpc(p, opts=default_options(), nthreads=oracle.num_threads())[4]
    for f in ("eflag", "prox_iters", "newton_iters"):
        assert np.array_equal(second[4][f], oc[f]), (f, second[4][f], oc[f])


def test_a_spread_launch_leaves_the_order_alone_and_one_qp_past_the_grid_is_ordered(hip, monkeypatch):
    """B = workgroups runs spread (one QP per wavefront, no queue to order): the stored order stays what it was.
    B = workgroups + 1 is packed: it installs an order and the next one runs by it.  All bitwise equal to the
    handle without the order."""
    cap = 3
    p = fx.synthetic_mpc_batch(cap + 1, first_id=13100, N=6)
    s = _handle(hip, monkeypatch, p, ordered=True, cap=cap)
    s0 = _handle(hip, monkeypatch, p, ordered=False, cap=cap)
    seen = []
    for B, n_after in ((cap, 0), (cap + 1, cap + 1), (cap, cap + 1), (cap + 1, cap + 1)):
        got, want = _solve(s, p, B), _solve(s0, p, B)
        assert (want[4]["eflag"] == 0).all()
        _assert_same_bits(got, want, "B = %d" % B)
        order = s.queue_order()
        assert order.size == n_after, (B, order)
        seen.append((order, got[4]["newton_iters"]))
    _assert_is_the_order_of(seen[1][0], seen[1][1], "packed")
    assert np.array_equal(seen[2][0], seen[1][0])  # (the spread launch in between)
    s.close()
    s0.close()


def test_the_order_lives_from_one_packed_batch_solve_to_the_next_of_its_size(hip, monkeypatch):
    """A solve of B - 5 QPs after one of B does not run by the old order (which names QPs it does not have: the bits
    of the unordered handle would not survive it) and installs its own; an adjoint call and a
    FBSTAB_HIP_KEEP_MATRICES solve in between leave the stored order as it is, and give the bits they give on the
    handle without one."""
    import torch
    dev = torch.device("cuda:0")
    p = _problem("headline")
    B = p.batch
    s = _handle(hip, monkeypatch, p, ordered=True)
    s0 = _handle(hip, monkeypatch, p, ordered=False)
    for b in (B, B, B - 5, B - 5):
        got, want = _solve(s, p, b), _solve(s0, p, b)
        assert (want[4]["eflag"] == 0).all()
        _assert_same_bits(got, want, "B = %d" % b)
        _assert_is_the_order_of(s.queue_order(), got[4]["newton_iters"], "B = %d" % b)
    order = s.queue_order()
    assert order.size == B - 5

    # the adjoint at the returned point, on the record adjoint kernel (it pulls QPs from the same queue word)
    z, l, v = got[:3]
    data = {k: np.ascontiguousarray(a[:B - 5]) for k, a in p.arrays.items()}
    gz = np.random.default_rng(13200).standard_normal(z.shape)
    assert s.adjoint_kernel_name() == "fbstab_mpc_r16_adjoint_kernel<12,4,20>"
    ga, gb = s.Adjoint(data, z, l, v, gz), s0.Adjoint(data, z, l, v, gz)
    assert sorted(ga) == sorted(gb) and (ga["status"] == 0).all()
    for k in ga:
        assert np.array_equal(_bits(ga[k]), _bits(gb[k])), k
    assert np.array_equal(s.queue_order(), order)

    # a KEEP solve: QP q in slot q, device pointers, as many QPs as the capped grid has slots
    K = W * 4
    res = []
    for h in (s, s0):
        d = {k: torch.from_numpy(np.ascontiguousarray(a[:K])).to(dev) for k, a in p.arrays.items()}
        x = [torch.zeros((K, n), dtype=torch.float64, device=dev) for n in (p.nz, p.nl, p.nv, p.nv)]
        out = hip.out_to_numpy(h.Solve(d, *x, keep_matrices=True))
        res.append(tuple(t.cpu().numpy() for t in x) + (out,))
    _assert_same_bits(res[0], res[1], "keep")
    assert (res[0][4]["eflag"] == 0).all()
    assert np.array_equal(s.queue_order(), order)

    # ... and the stored order still serves the next solve of its size
    _assert_same_bits(_solve(s, p, B - 5), want, "after the adjoint and the KEEP solve")
    assert np.array_equal(s.queue_order(), order)
    s.close()
    s0.close()
