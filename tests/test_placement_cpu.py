"""The placement detector detects (tests/placement_helpers.py, no GPU): the views land where the layouts say, hold
the packed arrays, the checker passes on an untouched buffer and reports a numpy stand-in that writes one double
past a slot, before a slot, or into the trailing gap of the last QP; the shared twin repeats the row; and blocks
filled from the views carry the addresses and strides of the views."""
import ctypes as C

import numpy as np
import pytest

from fbstab_amd import hip_api
from tests import placement_helpers as P

B = 3
LENS = dict(Q=8, q=5, A=12, x0=2, G=0)


def _packed(rng=None):
    rng = rng or np.random.default_rng(77)
    return {k: rng.standard_normal((B, n)) for k, n in LENS.items()}


def _addr(view):
    return view.ctypes.data


def test_records_land_at_the_documented_offsets_and_strides():
    a = _packed()
    p = P.records(a)
    rec = sum(n + P.GAP for n in LENS.values() if n)
    assert len(p.buffers) == 1 and p.buffers[0].data.size == B * rec
    base = p.buffers[0].data.ctypes.data
    off = 0
    for k, n in LENS.items():
        if n == 0:
            assert p.slots[k] is None and p[k].shape == (B, 0)
            continue
        assert p[k].shape == (B, n) and p[k].strides == (8 * rec, 8), k
        assert p[k].strides[0] > 8 * n
        assert _addr(p[k]) == base + 8 * off, k
        assert np.array_equal(p[k], a[k]) and np.array_equal(p.read(k), a[k]), k
        off += n + P.GAP
    # 8-byte aligned everywhere, 16-byte aligned only sometimes
    al = [_addr(p[k][q:]) % 16 for k, n in LENS.items() if n for q in range(B)]
    assert set(al) == {0, 8}, al
    # what is no slot is canary: GAP doubles behind every array of every record, the last QP's included
    assert p.buffers[0].gap.sum() == B * P.GAP * sum(1 for n in LENS.values() if n)
    assert p.buffers[0].gap[-P.GAP:].all()
    p.assert_intact()


def test_spread_uses_another_odd_pad_per_array():
    a = _packed()
    p = P.spread(a)
    pads = []
    for k, n in LENS.items():
        if n == 0:
            assert p.slots[k] is None
            continue
        buf, off, stride, rows, length = p.slots[k]
        assert (off, rows, length) == (0, B, n) and buf.data.size == B * stride
        assert p[k].strides == (8 * stride, 8) and _addr(p[k]) == buf.data.ctypes.data
        assert np.array_equal(p[k], a[k]) and np.array_equal(p.read(k), a[k])
        pads.append(stride - n)
        assert buf.gap.sum() == B * (stride - n) and buf.gap[-(stride - n):].all()
    assert pads == [1, 3, 5, 7]
    assert len(p.buffers) == 4
    p.assert_intact()


def test_canary_slots_and_gaps_hold_the_one_quiet_nan_pattern():
    a = _packed()
    for layout in P.LAYOUTS.values():
        p = layout(a, canary=("q", "x0"))
        for k in ("q", "x0"):
            assert (p.read(k).view(np.uint64) == P.CANARY).all()
        assert np.array_equal(p.read("Q"), a["Q"])
        for b in p.buffers:
            assert (b.bits[b.gap] == P.CANARY).all()
    x = np.array([P.CANARY], dtype=np.uint64).view(np.float64)[0]
    assert np.isnan(x) and (int(P.CANARY) >> 51) & 0xFFF == 0xFFF   # exponent all ones, quiet bit set
    assert np.isnan(x + 1.0) and np.isnan(0.0 * x)   # an over-read that reaches arithmetic shows


@pytest.mark.parametrize("layout", ["records", "spread"])
@pytest.mark.parametrize("where", ["past_a_slot", "before_a_slot", "trailing_gap_of_the_last_qp"])
def test_a_stand_in_overrun_is_reported(layout, where):
    """A numpy stand-in for a kernel that is one double off: the slot contents stay what they were, only a canary
    changes, and assert_gaps_intact names the buffer."""
    a = _packed()
    p = P.LAYOUTS[layout](a)
    p.assert_intact()
    buf, off, stride, rows, length = p.slots["A"]
    if where == "past_a_slot":
        at = off + 1 * stride + length          # one past QP 1's slot
    elif where == "before_a_slot":
        at = off + 1 * stride - 1               # one before QP 1's slot: the gap behind QP 0's record / row
    else:
        at = off + (rows - 1) * stride + length  # one past the LAST QP's slot: still inside the allocation
        assert at < buf.data.size
    assert buf.gap[at]
    buf.data[at] = 0.0
    for k in a:
        assert np.array_equal(p.read(k), a[k])
    with pytest.raises(AssertionError, match="canaries overwritten"):
        p.assert_intact()
    with pytest.raises(AssertionError, match="first at double %d" % at):
        P.assert_gaps_intact(buf)


def test_a_write_of_another_nan_is_reported_too():
    """The gaps are compared as bits: a NaN of another payload, or -0.0 for that matter, is a change."""
    p = P.spread(_packed())
    buf = p.slots["q"][0]
    buf.data[LENS["q"]] = np.nan
    assert np.isnan(buf.data[LENS["q"]])
    with pytest.raises(AssertionError):
        P.assert_gaps_intact(buf)


def test_the_shared_twin_repeats_the_row():
    a = _packed()
    p, twin = P.shared(a, ("Q", "A"))
    assert p.shared == ("Q", "A") and list(p.views) == list(a)
    for k in ("Q", "A"):
        assert p[k].shape == (1, LENS[k]) and np.array_equal(p[k][0], a[k][0])
        assert twin[k].shape == (B, LENS[k]) and all(np.array_equal(twin[k][q], a[k][0]) for q in range(B))
        buf = p.slots[k][0]
        assert buf.data.size == LENS[k] + P.GAP and buf.gap.sum() == P.GAP   # one row plus a gap
    for k in ("q", "x0"):
        assert np.array_equal(p[k], a[k]) and np.array_equal(twin[k], a[k]) and p[k].strides[0] > 8 * LENS[k]
    p.assert_intact()


@pytest.mark.parametrize("layout", ["records", "spread", "shared"])
def test_blocks_filled_from_the_views_carry_their_addresses_and_strides(layout):
    a = _packed()
    names = tuple(LENS)
    lens = tuple(LENS.values())
    p = P.shared(a, ("Q", "A"))[0] if layout == "shared" else P.LAYOUTS[layout](a)

    class Block(C.Structure):
        _fields_ = [("base", C.c_void_p * len(names)), ("stride", C.c_longlong * len(names))]

    blk, flags = Block(), []
    assert P.fill_block(blk, names, lens, p, B, flags) == B and not any(flags)
    for i, (k, n) in enumerate(zip(names, lens)):
        if n == 0:
            assert blk.base[i] is None and blk.stride[i] == 0
            continue
        buf, off, stride, rows, length = p.slots[k]
        assert blk.base[i] == buf.data.ctypes.data + 8 * off, k
        assert blk.stride[i] == (0 if k in p.shared else stride), k
        # QP b of the array lives at base + b * stride
        for q in range(B):
            row = (C.c_double * n).from_address(blk.base[i] + 8 * q * blk.stride[i])
            assert np.array_equal(np.frombuffer(row, dtype=np.float64), a[k][0 if k in p.shared else q]), (k, q)
    # the variables' block, through hip_api._fill_vars, keeps the views' strides as well
    v = P.records({k: a[k] for k in ("Q", "q", "A", "x0")}, canary=("x0",))
    vb = hip_api._fill_vars(tuple(v[k] for k in ("Q", "q", "A", "x0")), (8, 5, 12, 2), B, [])
    for i, k in enumerate(("Q", "q", "A", "x0")):
        assert vb.base[i] == _addr(v[k]) and vb.stride[i] == v.slots[k][2]
