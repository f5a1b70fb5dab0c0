"""The outer code without a GPU: the NumPy model of tests/rs_cases.py against its own consequences (the field, the
generator, zero syndromes by direct evaluation, systematic blocks, known lengths, round trips, every single error, exactly
16 and 17 errors, random words, the constructed miscorrection, bursts), the length functions through the loaded library
against the model, the header, the exports and the struct-free ABI, and the host arithmetic of csrc/rs_plan.h through the
stand-alone checker tools/rs_plan_check.cpp."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import rs_cases as rc
import stage_harness as sh
from ofdm_uhd_amd import _abi, rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KNOWN = {4: 36, 223: 255, 224: 288, 1784: 2040, 1785: 2073, 3568: 4080, 3569: 4113}


def rand_payload(n, seed=0):
    return np.random.default_rng(1000 * seed + n).integers(0, 256, n, dtype=np.uint8).tobytes()


# ---- 1. the field and the generator -------------------------------------------------------------------------------------
def test_field_and_generator():
    assert rc.EXP[8] == 0x1d and rc.EXP[255] == 1 and rc.EXP[0] == 1 and rc.EXP[1] == 2
    assert sorted(int(v) for v in rc.EXP[:255]) == list(range(1, 256))          # alpha generates the whole group
    for a in (1, 2, 0x1d, 0x80, 0xff):
        assert rc.gmul(a, rc.ginv(a)) == 1
        slow, x, y = 0, a, 0xc3                                                 # shift-and-add against the tables
        while y:
            if y & 1:
                slow ^= x
            x = (x << 1) ^ (0x11d if x & 0x80 else 0)
            y >>= 1
        assert rc.gmul(a, 0xc3) == slow
    g = rc.GEN
    assert len(g) == 33 and g[0] == 1 and all(g)                                # degree 32, monic, weight 33
    for i in range(40):
        assert (rc.poly_eval(g, int(rc.EXP[i])) == 0) == (i < 32)               # roots alpha^0 .. alpha^31, no others near
    assert rc.PARITY == _abi.OFDM_RS_PARITY == 32


# ---- 2. lengths -----------------------------------------------------------------------------------------------------------
def test_known_lengths():
    for k, f in KNOWN.items():
        assert rc.block_len(k) == f
    assert rs.coded_len(0) == 36 and rs.coded_len(219) == 255 and rs.coded_len(220) == 288 and rs.coded_len(1780) == 2040
    assert rs.coded_len(1781) == 2073 and rs.coded_len(3564) == 4080
    assert (rs.MAX_PAYLOAD, rs.MAX_CODED, rs.MAX_PAYLOAD_UNDER_FEC, rs.PARITY) == (3564, 4080, 1780, 32)
    from ofdm_uhd_amd import fec
    assert rs.coded_len(rs.MAX_PAYLOAD_UNDER_FEC) == fec.MAX_PAYLOAD < rs.coded_len(rs.MAX_PAYLOAD_UNDER_FEC + 1)
    with pytest.raises(ValueError):
        rs.coded_len(3565)
    with pytest.raises(ValueError):
        rs.coded_len(-1)


def test_length_functions_equal_the_model_for_every_n():
    lib = _abi.load()
    v = C.c_uint32(0)
    table = rc.length_table()
    assert len(table) == rc.MAX_PAYLOAD + 1                                     # no two payload lengths share a block length
    prev = None
    for n in range(rc.MAX_PAYLOAD + 1):
        assert lib.ofdm_rs_coded_len(n, C.byref(v)) == _abi.OFDM_OK
        f = v.value
        assert f == rc.coded_len(n) and table[f] == n
        assert prev is None or f - prev in (1, 33)                              # strictly increasing, in steps of 1 or 33
        prev = f
        assert lib.ofdm_rs_payload_len(f, C.byref(v)) == _abi.OFDM_OK and v.value == n
    for m in list(range(0, 4200)) + [0x7fffffff, 0xffffffff]:                   # gaps and out-of-range lengths are refused
        v.value = 77
        rc_ = lib.ofdm_rs_payload_len(m, C.byref(v))
        assert (rc_ == _abi.OFDM_OK) == (m in table), m
        assert rs.payload_len(m) == table.get(m) == rc.payload_len(m)
    gaps = [m for m in range(36, 4080) if m not in table]
    assert len(gaps) == 15 * 32 and gaps[0] == 256 and gaps[31] == 287 and gaps[-1] == 3857
    assert lib.ofdm_rs_coded_len(3565, C.byref(v)) == _abi.OFDM_E_INVAL
    assert lib.ofdm_rs_coded_len(0xffffffff, C.byref(v)) == _abi.OFDM_E_INVAL
    assert lib.ofdm_rs_coded_len(0, None) == _abi.OFDM_E_INVAL and lib.ofdm_rs_payload_len(36, None) == _abi.OFDM_E_INVAL


# ---- 3. the model against its own consequences ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", rc.SIZES)
def test_round_trip_systematic_zero_syndromes(n):
    p = rand_payload(n)
    b = rc.encode(p)
    k = n + 4
    W = rc.words(k)
    assert len(b) == rc.coded_len(n) == rs.coded_len(n)
    assert b[:k] == rc.info_bytes(p) and b[:n] == p                             # systematic
    buf = np.frombuffer(b, np.uint8)
    seen = np.zeros(len(b), int)
    for w in range(W):
        pos = rc.positions(k, w)
        seen[pos] += 1
        assert len(pos) == rc.cw_info(k, W, w) + 32 <= 255
        cw = [int(c) for c in buf[pos]]
        for i in range(32):                                                     # by direct evaluation, not by the decoder
            assert rc.poly_eval(cw, int(rc.EXP[i])) == 0
        assert rc.poly_eval(cw, int(rc.EXP[32])) != 0 or not any(cw)
    assert (seen == 1).all()                                                    # every byte in exactly one codeword
    assert sum(rc.cw_info(k, W, w) for w in range(W)) == k
    assert rc.decode(b) == (1, p, 0, 0)


def test_every_single_error_of_a_39_byte_block_is_corrected():
    p = b"\xa7\x01\xfe"
    b = rc.encode(p)
    assert len(b) == 39
    for at in range(39):
        for x in (0x01, 0x80, 0xff):
            assert rc.decode(rc.damage(b, [at], xor=x)) == (1, p, 1, 0), (at, x)


@pytest.mark.parametrize("length", [36, 40, 100, 255])
def test_16_errors_are_corrected_17_fail_random_words_fail(length):
    n = length - 36
    p = rand_payload(n, 1)
    b = rc.encode(p)
    assert len(b) == length and rc.words(n + 4) == 1
    rng = np.random.default_rng(length)
    for trial in range(6):
        d = rc.errors_per_codeword(b, 16, rng)
        assert rc.decode(d) == (1, p, 16, 0)
        d = rc.errors_per_codeword(b, 17, rng)
        k = n + 4
        assert rc.decode(d) == (int(d[:k] == b[:k]), d[:n], 0, 1)                # the received bytes, unchanged
        word = rng.integers(0, 256, length, dtype=np.uint8).tobytes()
        assert rc.decode(word) == (0, word[:n], 0, 1)
    assert rc.decode(bytes(length)) == (int(n == 0), bytes(n), 0, 0)            # all zeros: a codeword; its CRC fails but for n = 0


def test_the_constructed_miscorrection():
    for n, w in ((3, 0), (100, 0), (219, 0), (443, 1), (443, 2)):
        p = rand_payload(n, 2)
        b = rc.encode(p)
        m, other = rc.miscorrection(b, w=w, seed=n)
        assert sum(x != y for x, y in zip(m, b)) == 17 and sum(x != y for x, y in zip(m, other)) == 16
        k = n + 4
        for cw in range(rc.words(k)):                                           # `other` is made of codewords, too
            assert not rc.syndromes(np.frombuffer(other, np.uint8)[rc.positions(k, cw)]).any()
        got = rc.decode(m)
        assert got == (0, other[:n], 16, 0)                                     # the OTHER codeword: corrected 16, nothing failed, CRC fails


def test_bursts():
    p = rand_payload(443, 3)
    b = rc.encode(p)
    k, W = 447, 3
    assert len(b) == 543 and rc.words(k) == W
    for s in range(0, len(b) - 15 * W):                                         # 15 W + 1 wrong bytes at every start position
        d = rc.damage(b, np.arange(s, s + 15 * W + 1), xor=1 + s % 255)
        assert rc.decode(d) == (1, p, 15 * W + 1, 0), s
    for s in (0, 1, 2, 200, k - 16 * W, k, k + 1, len(b) - 16 * W):             # 16 W inside the info part or the parity part
        assert rc.decode(rc.damage(b, np.arange(s, s + 16 * W), xor=0x5a)) == (1, p, 16 * W, 0), s
    for s in (0, 100, k - 16 * W - 1):                                          # 16 W + 1 inside the info part: exactly one fails
        got = rc.decode(rc.damage(b, np.arange(s, s + 16 * W + 1), xor=0x33))
        assert got[0] == 0 and got[2:] == (32, 1), s


def test_lengths_that_are_no_block():
    for m in (0, 1, 35, 256, 287, 2041, 2072, 4081, 4091):
        assert rc.decode(bytes(m)) == (0, b"", 0, 0) and rc.payload_len(m) is None and rs.payload_len(m) is None


# ---- 4. header, exports, the struct-free ABI, the plan checker ------------------------------------------------------------
def test_header_exports_and_no_configuration_struct(tmp_path):
    hdr, code = sh.check_header_declares_and_library_exports(
        ["ofdm_rs_coded_len", "ofdm_rs_payload_len", "ofdm_rs_encode", "ofdm_rs_decode", "ofdm_rs_last_ms"])
    assert "outer code" in hdr
    for macro, value in (("OFDM_RS_PARITY", 32), ("OFDM_RS_MAX_PAYLOAD", 3564), ("OFDM_RS_MAX_CODED", 4080)):
        assert re.search(r"#define\s+%s\s+%d\b" % (macro, value), code) and getattr(_abi, macro) == value
    assert not re.search(r"\bofdm_rs_cfg\b", code) and not hasattr(_abi, "ofdm_rs_cfg")       # no parameters, no struct
    # the prototypes take no cfg argument; the C compiler takes the header
    assert re.search(r"int\s+ofdm_rs_encode\(ofdm_handle \*h, const uint8_t \*payloads,", code)
    assert re.search(r"int\s+ofdm_rs_decode\(ofdm_handle \*h, const uint8_t \*coded,", code)
    src = tmp_path / "use.c"
    src.write_text('#include "ofdm_hip.h"\nint main(void){ return OFDM_RS_MAX_CODED == OFDM_RS_MAX_PAYLOAD + 4 + 16 * OFDM_RS_PARITY ? 0 : 1; }\n')
    exe = str(tmp_path / "use")
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", "-o", exe + ".o", str(src)])
    lib = _abi.load()
    assert len(lib.ofdm_rs_encode.argtypes) == 8 and len(lib.ofdm_rs_decode.argtypes) == 11


def test_plan_checker(tmp_path):
    """The host arithmetic as a program of its own (the build a sanitizer run uses adds -fsanitize=address,undefined)."""
    exe = str(tmp_path / "rs_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tools", "rs_plan_check.cpp")])
    out = subprocess.check_output([exe]).decode()
    assert out.strip().endswith("rs_plan_check ok")


def test_limits_on_a_link():
    """ofdm_mod(rs=True).send_pkt's limits are those of the definition: the largest block a frame takes, and under an
    inner code the largest RS block that is still one of its payloads."""
    from ofdm_uhd_amd import fec
    assert rs.MAX_PAYLOAD_UNDER_FEC == max(n for n in range(rs.MAX_PAYLOAD + 1) if rs.coded_len(n) <= fec.MAX_PAYLOAD)
    assert rs.coded_len(rs.MAX_PAYLOAD) == rs.MAX_CODED
