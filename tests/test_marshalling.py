"""The three marshalling functions of fbstab_amd/hip_api.py that every entry point of the binding goes through:
_fill_block (a batch / direction / gradient block from a dict of arrays), _fill_vars (a _VarBatch) and _placement
(host or device, flags, stream, allocators).  CPU only: numpy arrays, no library handle."""
import numpy as np
import pytest

from fbstab_amd import hip_api as H

NAMES = ("H", "f", "G")
LENS = (6, 3, 0)  # (the third slot has length 0, as G of a dense handle with nl == 0)


def _block(arrays, B, **kw):
    b, flags = H._DenseBatch(), []
    rows = H._fill_block(b, NAMES, LENS, arrays, B, flags, **kw)
    return b, flags, rows


def test_shared_array_beside_a_batch_has_stride_0_and_beside_one_qp_its_length():
    shared, per_qp = np.zeros((1, 6)), np.zeros((3, 3))
    b, flags, rows = _block({"H": shared, "f": per_qp}, 3)
    assert (b.base[0], b.stride[0]) == (shared.ctypes.data, 0)
    assert (b.base[1], b.stride[1]) == (per_qp.ctypes.data, 3)
    assert rows == 3 and flags == [False, False]
    b, _, _ = _block({"H": shared, "f": np.zeros((1, 3))}, 1)
    assert (b.stride[0], b.stride[1]) == (6, 3)


def test_length_0_slot_is_null_with_stride_0():
    b, flags, _ = _block({"H": np.zeros((2, 6)), "f": np.zeros((2, 3)), "G": np.zeros((2, 0))}, 2)
    assert b.base[2] is None and b.stride[2] == 0
    assert len(flags) == 2  # (the empty array is not read)
    b, _, _ = _block({"H": np.zeros((2, 6)), "f": np.zeros((2, 3))}, 2)  # ... nor looked up
    assert b.base[2] is None and b.stride[2] == 0


def test_row_strided_view_gives_its_row_stride():
    wide = np.zeros((4, 10))
    b, _, _ = _block({"H": wide[:, :6], "f": wide[:, 6:9]}, 4)
    assert (b.base[0], b.stride[0]) == (wide.ctypes.data, 10)
    assert (b.base[1], b.stride[1]) == (wide.ctypes.data + 6 * 8, 10)


def test_optional_slot_given_none_or_left_out_is_null():
    b, flags, _ = _block({"H": None}, 2, optional=True)
    assert [b.base[i] for i in range(3)] == [None] * 3 and [b.stride[i] for i in range(3)] == [0] * 3
    assert flags == []
    f = np.zeros((2, 3))
    b, _, _ = _block({"f": f}, 2, optional=True)
    assert b.base[0] is None and (b.base[1], b.stride[1]) == (f.ctypes.data, 3)


def test_required_slot_given_none_asserts():
    with pytest.raises(AssertionError):
        _block({"H": None, "f": np.zeros((2, 3))}, 2)
    with pytest.raises(KeyError):
        _block({"H": np.zeros((2, 6))}, 2)


def test_wrong_dtype_and_wrong_trailing_length_assert():
    good = np.zeros((2, 3))
    with pytest.raises(AssertionError):
        _block({"H": np.zeros((2, 6), dtype=np.float32), "f": good}, 2)
    with pytest.raises(AssertionError):
        _block({"H": np.zeros((2, 5)), "f": good}, 2)
    with pytest.raises(AssertionError):
        _block({"H": np.zeros((2, 6)), "f": good}, 3)  # neither B rows nor one
    with pytest.raises(AssertionError):
        H._fill_vars((np.zeros((2, 4), dtype=np.int64),), (4,), 2, [])
    with pytest.raises(AssertionError):
        H._fill_vars((np.zeros((2, 5)),), (4,), 2, [])


def test_unshared_block_keeps_row_strides_and_reports_the_rows():
    one = np.zeros((1, 6))
    b, _, rows = _block({"H": one, "f": np.zeros((1, 3))}, None, shared=False)
    assert rows == 1 and b.stride[0] == 6


def test_var_batch_slots_and_the_batch_row_assertion():
    z, l, v = np.zeros((3, 4)), np.zeros((3, 0)), np.zeros((3, 8))[:, :5]
    flags = []
    vb = H._fill_vars((z, l, v), (4, 0, 5), 3, flags)
    assert (vb.base[0], vb.stride[0]) == (z.ctypes.data, 4)
    assert vb.base[1] is None and vb.stride[1] == 0
    assert (vb.base[2], vb.stride[2]) == (v.ctypes.data, 8)
    assert vb.base[3] is None and vb.stride[3] == 0  # (no y given)
    assert flags == [False, False]
    with pytest.raises(AssertionError):
        H._fill_vars((z, None, np.zeros((2, 5))), (4, 0, 5), 3, [])  # batch-row mismatch
    into = H._VarBatch()
    assert H._fill_vars((z,), (4,), None, [], vb=into) is into and into.base[0] == z.ctypes.data


def test_var_batch_required_and_optional_slots():
    z, gz = np.zeros((2, 4)), np.zeros((2, 4))
    with pytest.raises(AssertionError, match="z, l, v and gz are required"):
        H._fill_vars((z, None, None), (4, 2, 3), 2, [])
    with pytest.raises(AssertionError, match="z, l, v and gz are required"):
        H._fill_vars((None, None, None), (4, 2, 3), 2, [], optional=True)  # the first slot stays required
    sb = H._fill_vars((gz, None, None), (4, 2, 3), 2, [], optional=True)
    assert sb.base[0] == gz.ctypes.data and sb.base[1] is None and sb.base[2] is None


def test_placement_of_host_arrays():
    z = np.zeros((2, 4))
    where, flags, stream = H._placement([False, False], z, 0, async_=True, keep_matrices=True)
    assert where is H._Host and not where.on_dev
    assert flags == H.HOST_POINTERS and stream == 0  # (ASYNC and KEEP_MATRICES are device-pointer flags)
    out, status, zeros = where.out(z, 2), where.zeros(z, 2, "i4"), where.zeros(z, (2, 3))
    assert out.dtype == H.OUT_DTYPE and out.shape == (2,)
    assert status.dtype == np.int32 and status.shape == (2,) and zeros.dtype == np.float64 and zeros.shape == (2, 3)
    assert where.ptr(zeros) == zeros.ctypes.data
    assert H._placement([False], z, 1234)[2] == 1234  # the caller's stream stands


def test_placement_refuses_a_mix_of_host_and_device_arrays():
    with pytest.raises(AssertionError, match="mix of host and device arrays"):
        H._placement([True, False], np.zeros((1, 1)))
