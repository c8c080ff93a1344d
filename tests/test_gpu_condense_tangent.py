"""The forward mode of the condensed MPC route on the device (fbstab_hip_mpc_condensed_tangent_batch,
``CondensedMpc.Tangent``, ``forward_ad`` through ``autograd.solve_condensed_mpc``): the direction kernel against the
rounding bound of the seeds and, bit for bit, against the MPC tangent's; the step bit for bit against the condensed
adjoint fed the returned seeds; the duality with the adjoint's gradients; the placements of the C-ABI; torch.  Points
come from ``CondensedMpc.Solve`` (tests/test_gpu_condense_adjoint.py: ``solved``, computed once and left unchanged).
The five fixtures at their batch of 5 are the smallest shapes that cover odd image lengths (the unaligned head of
tangent_stage on odd QPs), nx > 32, nu > nx, and both dense kernels (four_wave: 72 condensed variables)."""
import types

import numpy as np
import pytest

from tests import condense_helpers as ch
from tests import condense_tangent_helpers as cth
from tests import tangent_helpers as TH
from tests import test_gpu_condense_adjoint as tca

pytestmark = pytest.mark.gpu
MPC_NAMES = ch.MPC_NAMES
SHAPES = ("tiny", "small", "odd33", "flat", "four_wave")
STEP, SEEDS = cth.STEP, cth.SEEDS
SUBSETS = (("x0",), ("A", "B"), ("q", "r", "c", "d"))


@pytest.fixture(scope="module")
def hip():
    from fbstab_amd import hip_api
    hip_api.load_library()
    return hip_api


def _solved(name, shared=False):
    return tca.solved(name, shared=True) if shared else tca.solved(name)   # (the cache keys of that module's own calls)


@pytest.fixture(scope="module")
def route():
    """route(name, shared=False) -> (CondensedMpc holding the images of the fixture, its data as numpy arrays, the
    problem, the point).  One object per fixture for the module, CLOSED at its teardown: a handle holds a stream, and
    handles left open change what later modules of the suite see (LABNOTES, the condensed sweep)."""
    from fbstab_amd.condense import CondensedMpc
    made = {}

    def get(name, shared=False):
        if (name, shared) not in made:
            p, x, _, _ = _solved(name, shared)
            data = {k: np.ascontiguousarray(a) for k, a in p.arrays.items()}
            cm = CondensedMpc(*p.sizes(), max_batch=p.arrays["x0"].shape[0])
            cm.Condense(data)
            made[name, shared] = (cm, data, p, x)
        return made[name, shared]
    yield get
    for cm, _, _, _ in made.values():
        cm.close()


# ---- 1. the seeds ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SHAPES)
def test_seeds_meet_the_rounding_bound(route, name):
    """All 12 sequences, and x0 alone, (A, B), (q, r, c, d) with the others NULL: every entry of (gz, gl, gv) within
    the bound of tangent_helpers.assert_rhs.  A slot of zeros gives the bits of a NULL slot."""
    cm, data, p, x = route(name)
    d = cth.directions(p, 61)
    worst = 0.0
    for names in (MPC_NAMES,) + SUBSETS:
        sub = {k: d[k] for k in names}
        res = cm.Tangent(data, *x, sub, rhs=True)
        assert (res["status"] == 0).all()
        for q in range(p.batch):
            xq = tuple(t[q] for t in x)
            worst = max(worst, TH.assert_rhs(p, q, xq, TH.one_direction(sub, q), tuple(res[k][q] for k in SEEDS),
                                             "+".join(names)))
        zeros = dict({k: np.zeros_like(d[k]) for k in MPC_NAMES}, **sub)
        same = cm.Tangent(data, *x, zeros, rhs=True)
        for k in SEEDS + STEP + ("status",):
            assert np.array_equal(res[k], same[k]), (names, k)
    print(name, "seeds: worst error / bound %.3f" % worst)


@pytest.mark.parametrize("name", ["small", "odd33"])
def test_seeds_are_the_mpc_tangents_bit_for_bit(hip, route, name):
    """The same device function with one thread per entry: the seeds FBstabMpcBatch.Tangent(rhs=True) writes for the
    same point and directions."""
    cm, data, p, x = route(name)
    d = cth.directions(p, 62)
    got = cm.Tangent(data, *x, d, rhs=True)
    m = hip.FBstabMpcBatch(*p.sizes(), max_batch=p.batch)
    ref = m.Tangent(data, *x, d, rhs=True)
    m.close()
    for k in SEEDS:
        assert got[k].tobytes() == ref[k].tobytes(), k


# ---- 2. the step ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,shared", [(n, False) for n in SHAPES] + [(n, True) for n in ("small", "flat", "four_wave")])
def test_step_and_status_are_the_adjoints_for_the_returned_seeds(route, name, shared):
    """dz, dl, dv and status are bitwise what CondensedMpc.Adjoint(adj=True) returns for the returned seeds - also
    with ONE image of H_c and A_c for the batch (stride 0)."""
    cm, data, p, x = route(name, shared)
    B = p.arrays["x0"].shape[0]
    assert cm._img["H"].shape[0] == (1 if shared else B)
    d = TH.random_directions(np.random.default_rng(63), p, B)
    t = cm.Tangent(data, *x, d, rhs=True)
    a = cm.Adjoint(data, *x, t["gz"], t["gl"], t["gv"], want=(), adj=True)
    assert (t["status"] == 0).all()
    for k in STEP + ("status",):
        assert t[k].tobytes() == a[k].tobytes(), k
    assert max(np.abs(t[k]).max() for k in STEP) > 0


@pytest.mark.parametrize("name", SHAPES)
def test_duality_with_the_adjoints_gradients(route, name):
    """<g, Tangent(dtheta)> against sum_k <Adjoint(g)[k], dtheta_k> for random g, relative to the sum of the
    magnitudes of the terms of <g, J dtheta>, within tangent_helpers.DUALITY_BAR; the value is printed."""
    cm, data, p, x = route(name)
    _, _, _, g = tca.solved(name)
    d = cth.directions(p, 64)
    t = cm.Tangent(data, *x, d)
    a = cm.Adjoint(data, *x, *g)
    assert (t["status"] == 0).all() and (a["status"] == 0).all()
    worst = 0.0
    for q in range(p.batch):
        worst = max(worst, cth.duality_number(tuple(s[q] for s in g), tuple(t[k][q] for k in STEP),
                                              {k: a[k][q] for k in MPC_NAMES}, TH.one_direction(d, q)))
    print(name, "duality on the device %.3e (bar %.1e)" % (worst, TH.DUALITY_BAR))
    assert worst <= TH.DUALITY_BAR, worst


# ---- 3. placements ----------------------------------------------------------------------------------------------------
def _same_bits(a, b, names, rows_a=slice(None), rows_b=slice(None), lens=None):
    for k in names:
        n = a[k].shape[1] if lens is None else lens[k]
        assert a[k][rows_a, :n].tobytes() == b[k][rows_b, :n].tobytes(), k


@pytest.mark.parametrize("name", ["small", "odd33", "four_wave"])
def test_placements_and_determinism(hip, name):
    p, x, img, _ = tca.solved(name)
    B = p.batch
    lens = dict(dz=p.nz, dl=p.nl, dv=p.nv, gz=p.nz, gl=p.nl, gv=p.nv)
    names = STEP + SEEDS
    d = cth.directions(p, 65)
    h = tca._handle(hip, p)
    res = cth.raw_tangent(hip, h._h, p, img, x, d)
    assert res["rc"] == 0, res["msg"]
    assert (res["status"] == 0).all() and np.isnan(res["work_tail"]).all()
    assert np.isnan(res["work_seeds"]).all(), "rhs is given: the tail of the work array is not addressed"
    assert all(np.isfinite(res[k]).all() for k in names)
    # padded strides with NaN behind every vector and image: the same bits, nothing written beyond a length
    padded = cth.raw_tangent(hip, h._h, p, img, x, d, pad=3)
    assert padded["rc"] == 0, padded["msg"]
    _same_bits(padded, res, names, lens=lens)
    for k in names:
        assert np.isnan(padded[k][:, lens[k]:]).all(), (k, "the doubles between two slots were written")
    # one direction for the batch (stride 0) against the replicated one
    one = {k: np.ascontiguousarray(a[2:3]) for k, a in d.items()}
    rep = {k: np.ascontiguousarray(np.repeat(a, B, axis=0)) for k, a in one.items()}
    s0, sr = cth.raw_tangent(hip, h._h, p, img, x, one), cth.raw_tangent(hip, h._h, p, img, x, rep)
    assert s0["rc"] == 0 and sr["rc"] == 0, (s0["msg"], sr["msg"])
    _same_bits(s0, sr, names)
    assert np.array_equal(s0["status"], sr["status"])
    _same_bits(s0, res, names, rows_a=slice(2, 3), rows_b=slice(2, 3))
    # a QP's bits do not depend on its batch
    for q in (0, 1, B - 1):
        alone = cth.raw_tangent(hip, h._h, p, img, x, d, qps=[q])
        assert alone["rc"] == 0, alone["msg"]
        _same_bits(alone, res, names, rows_b=slice(q, q + 1))
    # rhs NULL: the seeds live in the tail of the work array, and the step has the same bits
    null = cth.raw_tangent(hip, h._h, p, img, x, d, rhs=False)
    assert null["rc"] == 0 and set(null) & set(SEEDS) == set() and np.isnan(null["work_tail"]).all()
    _same_bits(null, res, STEP)
    assert np.array_equal(null["status"], res["status"])
    packed = np.concatenate([res[k].reshape(-1) for k in SEEDS])
    assert null["work_seeds"].tobytes() == packed.tobytes()
    # NaN in one QP's z leaves every other QP's bits unchanged
    zn = x[0].copy()
    zn[1, :] = np.nan
    bad = cth.raw_tangent(hip, h._h, p, img, (zn, x[1], x[2]), d)
    others = [q for q in range(B) if q != 1]
    assert bad["rc"] == 0, bad["msg"]
    _same_bits(bad, res, names, rows_a=others, rows_b=others)
    # batch 0: OK, nothing queued; a handle of another shape and a batch above max_batch are refused
    none = cth.raw_tangent(hip, h._h, p, img, x, d, batch=0)
    assert none["rc"] == 0 and all(np.isnan(none[k]).all() for k in names) and (none["status"] == -1).all()
    small = tca._handle(hip, p, max_batch=B - 1)
    r = cth.raw_tangent(hip, small._h, p, img, x, d)
    assert r["rc"] == 1 and "max_batch" in r["msg"] and all(np.isnan(r[k]).all() for k in names), r["msg"]
    small.close()
    h.close()


# ---- 4. torch ---------------------------------------------------------------------------------------------------------
def _loss(z, l, v):
    return (z * z.detach().cos()).sum() + (l * 0.5).sum() + (v * v.detach().sin()).sum()


@pytest.mark.parametrize("name,shared", [("small", False), ("four_wave", False), ("small", True)])
def test_forward_ad_through_solve_condensed_mpc(hip, name, shared):
    """Under forward_ad.dual_level the tangents of (z, l, v) equal ``cm.Tangent`` under the eflag and status mask, bit
    for bit - per-QP tangents, and with a shared model a ``(len,)`` and a ``(1, len)`` tangent; ONE Tangent call
    with the tangents that are present; and the backward on the same graph returns what it returns without any dual
    tensor."""
    import torch
    import torch.autograd.forward_ad as fwAD
    from fbstab_amd.autograd import solve_condensed_mpc
    from fbstab_amd.condense import CondensedMpc
    p, _, _, _ = _solved(name, shared)
    B = p.arrays["x0"].shape[0]
    cm = CondensedMpc(*p.sizes(), max_batch=B)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    prim = {k: t(a) for k, a in p.arrays.items()}
    rng = np.random.default_rng(66)
    dual_names = ("Q", "A", "q", "x0") if shared else ("R", "S", "B", "E", "c", "d", "x0")
    if shared:
        prim["Q"] = prim["Q"].reshape(-1)                      # (len,) and (1, len) are both shared
    tang = {k: t(rng.standard_normal(tuple(prim[k].shape))) for k in dual_names}
    grad_names = ("A", "q", "x0", "L")
    leaves = {k: a.clone().requires_grad_(k in grad_names) for k, a in prim.items()}
    asked = []
    method = cm.Tangent
    cm.Tangent = lambda *a, **kw: (asked.append(tuple(sorted(a[4]))), method(*a, **kw))[1]
    with fwAD.dual_level():
        data = {k: (fwAD.make_dual(a, tang[k]) if k in tang else a) for k, a in leaves.items()}
        z, l, v, out = solve_condensed_mpc(cm, data)
        tans = tuple(fwAD.unpack_dual(s).tangent for s in (z, l, v))
        _loss(z, l, v).backward()
    cm.Tangent = method
    assert asked == [tuple(sorted(dual_names))]              # ONE call, the tangents that are present
    eflag = hip.out_to_numpy(out)["eflag"]
    assert (eflag == 0).all(), eflag
    det = {k: (a.reshape(1, -1) if a.dim() == 1 else a) for k, a in prim.items()}
    dd = {k: (a.reshape(1, -1) if a.dim() == 1 else a) for k, a in tang.items()}
    ref = cm.Tangent(det, z.detach(), l.detach(), v.detach(), dd)
    assert (ref["status"] == 0).all()
    for got, k in zip(tans, STEP):
        assert got.cpu().numpy().tobytes() == ref[k].cpu().numpy().tobytes() and np.abs(ref[k].cpu().numpy()).max() > 0, k
    # the backward without any dual tensor
    plain = {k: a.clone().requires_grad_(k in grad_names) for k, a in prim.items()}
    z2, l2, v2, _ = solve_condensed_mpc(cm, plain)
    _loss(z2, l2, v2).backward()
    for k in grad_names:
        assert leaves[k].grad.shape == prim[k].shape
        assert leaves[k].grad.cpu().numpy().tobytes() == plain[k].grad.cpu().numpy().tobytes(), k
    cm.close()


def test_jvp_recondenses_stale_images_and_masks_failed_qps(hip):
    """``CondensedMpcSolveFunction.jvp`` on a forward's saved tensors after another ``Condense`` has replaced the
    images (``generation`` has moved): it re-condenses and returns the bits of a ``Tangent`` on fresh images; a QP whose
    record says anything but SUCCESS gets zero tangents, and ``out`` gets None."""
    import torch
    from fbstab_amd.autograd import CondensedMpcSolveFunction
    from fbstab_amd.condense import CondensedMpc
    p, x, _, _ = tca.solved("small")
    other = ch.problem("small")
    B = p.batch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    data = {k: t(a) for k, a in p.arrays.items()}
    xd = tuple(t(a) for a in x)
    d = {k: t(a) for k, a in cth.directions(p, 67, names=("Q", "B", "d", "x0")).items()}
    cm = CondensedMpc(*p.sizes(), max_batch=B)
    cm.Condense(data)
    ref = cm.Tangent(data, *xd, d)
    generation = cm.generation
    # the images of another problem: the same shape, x0 and the matrices scaled
    cm.Condense({k: t(a * (0.5 if k in ("x0", "Q", "A") else 1.0)) for k, a in other.arrays.items()})
    assert cm.generation != generation
    wrong = cm.Tangent(data, *xd, d)
    assert wrong["dz"].cpu().numpy().tobytes() != ref["dz"].cpu().numpy().tobytes()
    out = torch.zeros((B, 40), dtype=torch.uint8, device="cuda")
    out[1, 0] = 2                                            # (SolverOut::eflag of QP 1: not SUCCESS)
    ctx = types.SimpleNamespace(saved_tensors=tuple(data[k] for k in MPC_NAMES) + xd + (out,), shared=(), cm=cm,
                                sigma=0.0, generation=generation)
    tangents = tuple(d.get(k) for k in MPC_NAMES)
    dz, dl, dv, dout = CondensedMpcSolveFunction.jvp(ctx, None, None, *tangents)
    assert dout is None
    keep = [q for q in range(B) if q != 1]
    for got, k in zip((dz, dl, dv), STEP):
        a, b = got.cpu().numpy(), ref[k].cpu().numpy()
        assert a[keep].tobytes() == b[keep].tobytes() and not a[1].any() and np.abs(b[1]).max() > 0, k
    cm.close()
