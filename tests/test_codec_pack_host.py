"""engine._pack_values: the one place where a list of int8 arrays becomes the (blob, offsets, lengths) that every
``*_soft`` call of the coded links takes (fec_decode_soft, fec_decode_soft_rel, ldpc_decode_soft, rs_rel_from_soft).
Host only: NumPy, no GPU, no library."""
import numpy as np
import pytest

from ofdm_uhd_amd.engine import _pack_values


def _check_layout(vals, blob, offs, lens):
    """What every caller relies on: dtypes, one entry per array, offsets cumulative in values, every array where its
    offset says, and 8 zero values behind the last one."""
    sizes = [int(np.asarray(v).size) for v in vals]
    assert blob.dtype == np.int8 and offs.dtype == np.uint64 and lens.dtype == np.uint32
    assert blob.flags["C_CONTIGUOUS"] and blob.ndim == 1
    assert len(offs) == len(lens) == len(vals)
    assert offs.tolist() == [sum(sizes[:i]) for i in range(len(vals))]
    assert len(blob) == sum(sizes) + 8 and not blob[sum(sizes):].any()
    for v, o, n in zip(vals, offs, sizes):
        assert np.array_equal(blob[int(o):int(o) + n], np.asarray(v).astype(np.int8).reshape(-1))


def test_an_empty_list():
    for strict in (False, True):
        blob, offs, lens = _pack_values([], strict=strict)
        _check_layout([], blob, offs, lens)
        assert blob.tolist() == [0] * 8 and len(offs) == 0 and len(lens) == 0


def test_one_array_of_no_values():
    blob, offs, lens = _pack_values([np.zeros(0, np.int8)])
    _check_layout([np.zeros(0, np.int8)], blob, offs, lens)
    assert lens.tolist() == [0] and offs.tolist() == [0] and len(blob) == 8


def test_whole_bytes():
    rng = np.random.default_rng(3)
    vals = [rng.integers(-128, 128, n).astype(np.int8) for n in (8, 16, 24)]
    for strict in (False, True):
        blob, offs, lens = _pack_values(vals, strict=strict)
        _check_layout(vals, blob, offs, lens)
        assert lens.tolist() == [1, 2, 3] and offs.tolist() == [0, 8, 24]


def test_a_ragged_length_is_handed_on_as_one_byte():
    rng = np.random.default_rng(4)
    vals = [rng.integers(-128, 128, n).astype(np.int8) for n in (16, 12, 0, 8)]
    blob, offs, lens = _pack_values(vals)
    _check_layout(vals, blob, offs, lens)
    assert lens.tolist() == [2, 1, 0, 1]            # 12 values are no whole bytes: the length 1, which is no block
    assert offs.tolist() == [0, 16, 28, 28]         # ... and the offsets still advance by the 12 values
    with pytest.raises(ValueError):
        _pack_values(vals, strict=True)
    with pytest.raises(ValueError):
        _pack_values([np.zeros(12, np.int8)], strict=True)


def test_inputs_are_converted():
    rng = np.random.default_rng(5)
    wide = rng.integers(-128, 128, 32).astype(np.int64)
    strided = rng.integers(-128, 128, 48).astype(np.int8)[::2]      # 24 values, not contiguous
    square = rng.integers(-128, 128, (2, 8)).astype(np.int16)       # two dimensions: read row by row
    as_list = [1, -1, 0, 127, -128, 5, -5, 9]
    assert not strided.flags["C_CONTIGUOUS"]
    vals = [wide, strided, square, as_list]
    blob, offs, lens = _pack_values(vals)
    _check_layout(vals, blob, offs, lens)
    assert lens.tolist() == [4, 3, 2, 1] and offs.tolist() == [0, 32, 56, 72]
