"""The LDPC coded-link layer without a GPU: the NumPy model of tests/ldpc_cases.py against its own consequences (the
table has no 4-cycles, every encoded word has a zero syndrome, known lengths, round trips on clean, hard-damaged and
erased input), the library's two length functions against the model over every length, the configuration helpers, the
header and the exports, and the host arithmetic of csrc/ldpc_plan.h through the stand-alone checker
tools/ldpc_plan_check.cpp."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ldpc_cases as lc
from ofdm_uhd_amd import _abi, ldpc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (0, 1, 91, 92, 93, 188, 189, 2012)


def rand_payload(n, seed=0):
    return np.random.default_rng(1000 * seed + n).integers(0, 256, n, dtype=np.uint8).tobytes()


# ---- 1. the table --------------------------------------------------------------------------------------------------------
def test_table_shape_and_degrees():
    assert lc.H.shape == (12, 24) and lc.N_ENTRIES == 83
    assert int((lc.H[:, :12] >= 0).sum()) == 58 and int((lc.H[:, 12:] >= 0).sum()) == 25
    assert [len(r) for r in lc.ROW_ENTRIES] == [7] * 6 + [6] + [7] * 5
    assert ((lc.H >= -1) & (lc.H < 64)).all()
    assert (lc.H[:, 12:] >= 0).sum(axis=0).tolist() == [3] + [2] * 11           # the staircase and its first column


def test_table_has_no_4_cycles():
    H = lc.H
    n = 0
    for r in range(12):
        for r2 in range(r + 1, 12):
            both = np.flatnonzero((H[r] >= 0) & (H[r2] >= 0))
            for a in range(len(both)):
                for b in range(a + 1, len(both)):
                    c, c2 = both[a], both[b]
                    assert (H[r, c] - H[r2, c] - H[r, c2] + H[r2, c2]) % 64 != 0, (r, r2, c, c2)
                    n += 1
    assert n > 0                                                                 # (there are rectangles to look at)


# ---- 2. the encoder ------------------------------------------------------------------------------------------------------
def test_every_encoded_word_has_a_zero_syndrome():
    rng = np.random.default_rng(3)
    info = rng.integers(0, 2, (200, lc.K_BITS), dtype=np.uint8)
    info[0] = 0
    info[1] = 1
    info[2:2 + 12] = 0
    for j in range(12):
        info[2 + j, 64 * j] = 1                                                  # one bit per info column
    cw = lc.encode_codeword(info)
    assert cw.shape == (200, lc.N_BITS) and np.array_equal(cw[:, :lc.K_BITS], info)    # systematic
    assert not lc.syndrome(cw).any()
    assert not cw[0].any()
    flipped = cw.copy()
    flipped[:, 700] ^= 1
    assert lc.syndrome(flipped).reshape(200, -1).sum(axis=1).tolist() == [int((lc.H[:, 700 // 64] >= 0).sum())] * 200


def test_blocks_of_the_model():
    for n in SIZES:
        p = rand_payload(n)
        b = lc.encode(p)
        assert len(b) == lc.coded_len(n)
        k = n + 4
        kws = lc.cw_info_lens(k)
        assert sum(kws) == k and all(kw == 96 for kw in kws[:-1]) and 1 <= kws[-1] <= 96
        info = b"".join(b[192 * w:192 * w + kw] for w, kw in enumerate(kws))    # systematic: the info bytes are on the air
        assert info[:n] == p and len(info) == k
    assert lc.coded_len(2013) is None
    with pytest.raises(AssertionError):
        lc.encode(bytes(2013))


# ---- 3. lengths: the library against the model -------------------------------------------------------------------------------
def test_length_functions_equal_the_model_for_every_length():
    assert (ldpc.MAX_PAYLOAD, ldpc.MAX_CODED) == (lc.MAX_PAYLOAD, lc.MAX_CODED) == (2012, 4032)
    prev = -1
    for n in range(2101):
        want = lc.coded_len(n)
        if want is None:
            assert n > 2012
            with pytest.raises(ValueError):
                ldpc.coded_len(n)
        else:
            assert ldpc.coded_len(n) == want > prev                             # strictly increasing in n
            prev = want
    blocks = 0
    for m in range(4201):
        assert ldpc.payload_len(m) == lc.payload_len(m), m
        assert (lc.payload_len(m) is not None) == (100 <= m <= 4032 and (m - 1) % 192 >= 96)
        blocks += lc.payload_len(m) is not None
    assert blocks == 2013
    assert {n: lc.coded_len(n) for n in (0, 92, 93, 188, 189, 2012)} == {0: 100, 92: 192, 93: 289, 188: 384, 189: 481, 2012: 4032}
    for m in (99, 193, 288, 4033):
        assert ldpc.payload_len(m) is None
    with pytest.raises(ValueError):
        ldpc.coded_len(-1)
    assert ldpc.payload_len(-1) is None and ldpc.payload_len(1 << 33) is None
    lib = _abi.load()
    v = C.c_uint32(77)
    assert lib.ofdm_ldpc_coded_len(5, None) == _abi.OFDM_E_INVAL and lib.ofdm_ldpc_payload_len(100, None) == _abi.OFDM_E_INVAL
    assert lib.ofdm_ldpc_payload_len(99, C.byref(v)) == _abi.OFDM_E_INVAL and v.value == 77


# ---- 4. round trips of the model -------------------------------------------------------------------------------------------
def test_model_round_trip_clean():
    for n in SIZES:
        p = rand_payload(n, 1)
        assert lc.decode(lc.encode(p)) == (1, p, 0, 1, 0)
    for m in (0, 99, 193, 288, 4033):
        assert lc.decode(bytes(m)) == lc.NO_BLOCK
    assert lc.decode_values(np.ones(801, np.int8)) == lc.NO_BLOCK


def test_model_round_trip_hard_damage():
    rng = np.random.default_rng(11)
    for n in SIZES:
        p = rand_payload(n, 2)
        b = lc.encode(p)
        pos = np.flatnonzero(rng.random(8 * len(b)) < 0.04)
        ok, got, corrected, iters, failed = lc.decode(lc.flip(b, pos))
        assert (ok, got, failed) == (1, p, 0) and corrected == len(pos) and 1 < iters <= 20


def test_model_round_trip_erasures():
    rng = np.random.default_rng(12)
    for n in SIZES:
        p = rand_payload(n, 3)
        v = lc.hard_values(lc.encode(p)).copy()
        v[rng.random(len(v)) < 0.25] = 0                                         # a quarter of the bits never arrived
        ok, got, corrected, iters, failed = lc.decode_values(v)
        assert (ok, got, corrected, failed) == (1, p, 0, 0) and 1 <= iters <= 20
    assert iters > 1                                                             # (the longest block needed more than one)
    # nothing but erasures: every check holds for the all-zero word, whose CRC field does not match
    z = lc.decode_values(np.zeros(8 * lc.coded_len(92), np.int8))
    assert z == (0, bytes(92), 0, 1, 0)
    # -128 reads as -127
    v = lc.hard_values(lc.encode(rand_payload(92, 4))).astype(np.int16) * 8
    v = np.clip(v, -128, 127).astype(np.int8)
    assert v.min() == -128 and lc.decode_values(v) == lc.decode_values(np.maximum(v, -127))


def test_max_iters_bounds_the_model():
    rng = np.random.default_rng(13)
    p = rand_payload(188, 5)
    b = lc.encode(p)
    bad = lc.flip(b, np.flatnonzero(rng.random(8 * len(b)) < 0.05))
    full = lc.decode(bad)
    assert full[0] == 1 and full[3] > 2
    one = lc.decode(bad, 1)
    assert one[3] == 1 and one[4] >= 1                                          # stopped by the limit, checks still open
    assert lc.decode(bad, full[3])[:2] == (1, p) and lc.decode(bad, full[3] - 1)[4] >= 1


def test_decode_many_is_decode_values():
    rng = np.random.default_rng(14)
    vals = [lc.awgn_values(lc.encode(rand_payload(n, 6)), 2.0, 0.5, rng) for n in (0, 93, 500)]
    vals.insert(1, np.zeros(8 * 99, np.int8))
    assert lc.decode_many(vals) == [lc.decode_values(v) for v in vals]
    assert lc.decode_many([]) == []


# ---- 5. configuration ------------------------------------------------------------------------------------------------------
def test_cfg_helpers():
    c = ldpc.ldpc_cfg()
    assert (c.struct_size, c.max_iters, list(c.reserved)) == (32, 20, [0] * 6)
    assert C.sizeof(_abi.ofdm_ldpc_cfg) == 32
    assert ldpc.ldpc_cfg(1).max_iters == 1 and ldpc.ldpc_cfg(64).max_iters == 64
    for bad in (0, 65, -1, True, 2.0, "20", None):
        with pytest.raises(ValueError):
            ldpc.ldpc_cfg(bad)
    assert ldpc.as_cfg(None) is None and ldpc.as_cfg(False) is None
    assert ldpc.as_cfg(True).max_iters == 20 and ldpc.as_cfg(7).max_iters == 7
    assert ldpc.as_cfg(dict(max_iters=3)).max_iters == 3 and ldpc.as_cfg({}).max_iters == 20
    assert ldpc.as_cfg(c) is c
    for bad in (0, 65, dict(max_iters=0), dict(iters=3), "x", 1.5):
        with pytest.raises(ValueError):
            ldpc.as_cfg(bad)


def test_header_and_exports():
    names = ("ofdm_ldpc_coded_len", "ofdm_ldpc_payload_len", "ofdm_ldpc_encode", "ofdm_ldpc_decode", "ofdm_ldpc_decode_soft",
             "ofdm_rx_ldpc_decode_soft", "ofdm_ldpc_last_ms")
    with open(os.path.join(ROOT, "include", "ofdm_hip.h")) as f:
        hdr = f.read()
    lib = _abi.load()
    for name in names:
        assert name + "(" in hdr and name in _abi.EXPORTS and hasattr(lib, name)
    assert "#define OFDM_LDPC_MAX_PAYLOAD 2012" in hdr and "#define OFDM_LDPC_MAX_CODED 4032" in hdr
    assert "#define OFDM_ABI_VERSION 6" in hdr and _abi.OFDM_ABI_VERSION == 6
    # the table in the header's comment is the model's
    rows = re.findall(r"^ \* +(\d+):((?: +(?:-|\d+)){12})$", hdr, re.M)
    assert [int(r[0]) for r in rows] == list(range(12))
    for i, (_, cells) in enumerate(rows):
        assert [(-1 if c == "-" else int(c)) for c in cells.split()] == list(lc.INFO_SHIFTS[i])


def test_ofdm_arguments_that_need_no_gpu():
    from ofdm_uhd_amd import rs
    assert rs.MAX_PAYLOAD_UNDER_LDPC == 1752 and rs.coded_len(1752) == ldpc.MAX_PAYLOAD < rs.coded_len(1753)


# ---- 6. the host arithmetic as a program of its own ------------------------------------------------------------------------
def test_plan_checker(tmp_path):
    exe = str(tmp_path / "ldpc_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tools", "ldpc_plan_check.cpp")])
    out = subprocess.check_output([exe]).decode()
    assert out.strip().endswith("ldpc_plan_check ok")
