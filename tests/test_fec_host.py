"""Coded links without a GPU: the NumPy model of tests/fec_cases.py against the code's known properties, the two length
functions through the loaded library, the ctypes mirror of ofdm_fec_cfg, and the host arithmetic of
csrc/fec_plan.h (lengths, batch layout, slicing) through the stand-alone checker tools/fec_plan_check.cpp."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import fec_cases as fc
import stage_harness as sh
from ofdm_uhd_amd import _abi, fec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_impulse_response():
    """133 / 171 octal in the 802.11a arrangement: a single 1 gives A = 1011011, B = 1111001."""
    c = fc.conv(np.array([1, 0, 0, 0, 0, 0, 0], np.uint8))
    assert "".join(map(str, c[0::2])) == "1011011"
    assert "".join(map(str, c[1::2])) == "1111001"


@pytest.mark.parametrize("C_", [1, 16])
def test_round_trip(C_):
    rng = np.random.default_rng(7)
    for n in list(range(17)) + [100]:
        p = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        blk = fc.encode(p, C_)
        assert len(blk) == 2 * n + 10 == fc.coded_len(n)
        assert fc.decode(blk, C_) == (1, p, 0)
    # the interleaver is a permutation of the bits, the identity for one column
    assert sorted(fc.perm(400, 16)) == list(range(400)) and fc.perm(400, 1).tolist() == list(range(400))


def test_four_flips_in_twenty_bytes():
    """d_free = 10: any 4 flipped coded bits (pad excluded) decode exactly, and all 4 are counted."""
    rng = np.random.default_rng(11)
    p = rng.integers(0, 256, 20, dtype=np.uint8).tobytes()
    for C_ in (1, 16):
        blk = fc.encode(p, C_)
        B = 8 * len(blk)
        sent = np.flatnonzero(fc.perm(B, C_) < B - 4)        # transmitted positions that carry a coded bit
        for _ in range(150):
            pos = rng.choice(sent, 4, replace=False)
            assert fc.decode(fc.flip(blk, pos), C_) == (1, p, 4)


def test_all_erasures():
    n = 12
    ok, payload, corrected = fc.decode_values(np.zeros(8 * fc.coded_len(n), np.int8))
    assert (ok, payload, corrected) == (0, bytes(n), 0)      # every tie keeps u = 0; CRC-32 of zeros is not zero


def test_lengths_that_are_no_block():
    for m in (0, 9, 11, 4091, 4092):
        assert fc.decode(bytes(m)) == (0, b"", 0)
    assert fc.decode_values(np.ones(81, np.int8)) == (0, b"", 0)


def test_length_functions_through_the_library():
    lib = _abi.load()
    n = C.c_uint32(0)
    for p in (0, 1, 100, 2040):
        assert lib.ofdm_fec_coded_len(p, C.byref(n)) == _abi.OFDM_OK and n.value == 2 * p + 10 == fec.coded_len(p)
        assert lib.ofdm_fec_payload_len(2 * p + 10, C.byref(n)) == _abi.OFDM_OK and n.value == p == fec.payload_len(2 * p + 10)
    assert lib.ofdm_fec_coded_len(2041, C.byref(n)) == _abi.OFDM_E_INVAL
    assert lib.ofdm_fec_coded_len(0xffffffff, C.byref(n)) == _abi.OFDM_E_INVAL
    assert lib.ofdm_fec_coded_len(0, None) == _abi.OFDM_E_INVAL
    for m in (0, 9, 11, 4091, 4092, 0xffffffff):
        assert lib.ofdm_fec_payload_len(m, C.byref(n)) == _abi.OFDM_E_INVAL and fec.payload_len(m) is None
    assert lib.ofdm_fec_payload_len(10, None) == _abi.OFDM_E_INVAL
    with pytest.raises(ValueError):
        fec.coded_len(2041)
    assert (fec.MAX_PAYLOAD, fec.MAX_CODED) == (fc.MAX_PAYLOAD, fc.MAX_CODED) == (2040, 4090)


def test_cfg_helpers():
    assert fec.as_cfg(None) is None and fec.as_cfg(False) is None
    assert fec.as_cfg(True).interleave_cols == 16 and fec.as_cfg(dict(interleave=4)).interleave_cols == 4
    assert fec.as_cfg(8).interleave_cols == 8 and fec.fec_cfg().struct_size == C.sizeof(_abi.ofdm_fec_cfg)
    for bad in (0, 3, 32, -1, 2.5, True):
        with pytest.raises(ValueError):
            fec.fec_cfg(bad)


def test_header_and_layout(tmp_path):
    sh.check_header_declares_and_library_exports(
        ["ofdm_fec_coded_len", "ofdm_fec_payload_len", "ofdm_fec_encode", "ofdm_fec_decode", "ofdm_fec_decode_soft",
         "ofdm_fec_last_ms"])
    got = sh.check_cfg_layout_matches_header(tmp_path, _abi.ofdm_fec_cfg, 32,
                                             (("max_payload", "OFDM_FEC_MAX_PAYLOAD"), ("max_coded", "OFDM_FEC_MAX_CODED")))
    assert (int(got["max_payload"]), int(got["max_coded"])) == (2040, 4090)


def test_plan_checker(tmp_path):
    """The host arithmetic as a program of its own (the build a sanitizer run uses adds -fsanitize=address,undefined)."""
    exe = str(tmp_path / "fec_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tools", "fec_plan_check.cpp")])
    out = subprocess.check_output([exe]).decode()
    assert out.strip().endswith("fec_plan_check ok")
