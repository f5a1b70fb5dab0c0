"""Punctured rates of the coded links without a GPU: the length functions through the loaded library against the NumPy
model of tests/punct_cases.py, the model against its own consequences (the 802.11 puncturing matrices, the C' rule,
round trips, single flips, all erasures), the header, the exports and the ctypes mirror, and the host arithmetic of
csrc/punct_plan.h through the stand-alone checker tools/punct_plan_check.cpp."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import fec_cases as fc
import punct_cases as pc
import stage_harness as sh
from ofdm_uhd_amd import _abi, fec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# P at n = 0, 1, 2, 1026, 2040
KNOWN = {"2/3": (8, 9, 11, 1547, 3068), "3/4": (7, 8, 9, 1375, 2727), "5/6": (6, 7, 9, 1237, 2454)}
KNOWN_N = (0, 1, 2, 1026, 2040)


# ---- 1. length functions through the library ---------------------------------------------------------------------------
@pytest.mark.parametrize("rate", pc.RATES)
def test_length_functions_equal_the_model_for_every_n(rate):
    lib = _abi.load()
    rid = pc.RATE_ID[rate]
    v = C.c_uint32(0)
    table = pc.length_table(rate)
    assert len(table) == fc.MAX_PAYLOAD + 1                          # no two payload lengths share a block length
    prev = None
    for n in range(fc.MAX_PAYLOAD + 1):
        assert lib.ofdm_fec_coded_len_rate(rid, n, C.byref(v)) == _abi.OFDM_OK
        P = v.value
        assert table[P] == n
        assert prev is None or P - prev in (1, 2)                    # strictly increasing, in steps of 1 or 2
        prev = P
        assert lib.ofdm_fec_payload_len_rate(rid, P, C.byref(v)) == _abi.OFDM_OK and v.value == n
    for n in (0, 1, 2, 3, 5, 64, 301, 2040):                        # the closed form is the counted pattern
        assert pc.coded_len(n, rate) == fec.coded_len(n, rate) and pc.payload_len(pc.coded_len(n, rate), rate) == n
    # every length P never reaches, and every length out of range, is refused
    for m in list(range(0, 4100)) + [0x7fffffff, 0xffffffff]:
        rc = lib.ofdm_fec_payload_len_rate(rid, m, C.byref(v))
        assert (rc == _abi.OFDM_OK) == (m in table), m
        assert fec.payload_len(m, rate) == table.get(m)
    gaps = [m for m in range(min(table), max(table)) if m not in table]
    assert gaps and all(pc.payload_len(m, rate) is None for m in gaps)
    assert lib.ofdm_fec_coded_len_rate(rid, 2041, C.byref(v)) == _abi.OFDM_E_INVAL
    assert lib.ofdm_fec_coded_len_rate(rid, 0xffffffff, C.byref(v)) == _abi.OFDM_E_INVAL
    assert lib.ofdm_fec_coded_len_rate(rid, 0, None) == _abi.OFDM_E_INVAL
    assert lib.ofdm_fec_payload_len_rate(rid, table and min(table), None) == _abi.OFDM_E_INVAL
    with pytest.raises(ValueError):
        fec.coded_len(2041, rate)


def test_known_answers():
    for rate, want in KNOWN.items():
        assert tuple(fec.coded_len(n, rate) for n in KNOWN_N) == want == tuple(pc.coded_len(n, rate) for n in KNOWN_N)
        assert tuple(fec.payload_len(P, rate) for P in want) == KNOWN_N
    assert fec.payload_len(10, "2/3") is None and pc.payload_len(10, "2/3") is None      # 9 -> 11: a gap at 2/3
    assert fec.payload_len(3069, "2/3") is None and fec.payload_len(2728, "3/4") is None and fec.payload_len(2455, "5/6") is None
    assert fec.payload_len(5, "5/6") is None and fec.payload_len(0, "3/4") is None
    assert fec.MAX_PAYLOAD == 2040                                                       # unchanged


def test_rate_0_is_the_old_pair_and_rate_4_is_refused():
    lib = _abi.load()
    a, b = C.c_uint32(1), C.c_uint32(2)
    for n in list(range(0, 2044)) + [0xffffffff]:
        assert lib.ofdm_fec_coded_len_rate(0, n, C.byref(a)) == lib.ofdm_fec_coded_len(n, C.byref(b))
        assert n > 2040 or a.value == b.value == 2 * n + 10
    for m in list(range(0, 4094)) + [0xffffffff]:
        a.value = b.value = 77
        assert lib.ofdm_fec_payload_len_rate(0, m, C.byref(a)) == lib.ofdm_fec_payload_len(m, C.byref(b))
        assert a.value == b.value
    for rid in (4, 5, 0xffffffff):
        assert lib.ofdm_fec_coded_len_rate(rid, 0, C.byref(a)) == _abi.OFDM_E_INVAL
        assert lib.ofdm_fec_payload_len_rate(rid, 10, C.byref(a)) == _abi.OFDM_E_INVAL
    assert fec.coded_len(7) == fec.coded_len(7, "1/2") == fec.coded_len(7, None) == 24
    assert fec.payload_len(24) == fec.payload_len(24, "1/2") == 7


def test_cfg_helpers():
    assert fec.fec_cfg().rate == 0 and fec.fec_cfg(rate="1/2").rate == 0
    assert [fec.fec_cfg(rate=r).rate for r in pc.RATES] == [1, 2, 3] == [pc.RATE_ID[r] for r in pc.RATES]
    cfg = fec.as_cfg(dict(rate="3/4"))
    assert (cfg.rate, cfg.interleave_cols, cfg.struct_size) == (2, 16, 32)
    cfg = fec.as_cfg(dict(interleave=8, rate="5/6"))
    assert (cfg.rate, cfg.interleave_cols) == (3, 8)
    assert fec.as_cfg(True).rate == 0 and fec.as_cfg(4).rate == 0
    assert fec.coded_len(1026, cfg) == 1237 and fec.payload_len(1237, cfg) == 1026      # a cfg names its rate
    for bad in ("7/8", "1", 2, 0.75, ""):
        with pytest.raises(ValueError):
            fec.fec_cfg(rate=bad)


# ---- 2. the model against its own consequences -----------------------------------------------------------------------
def test_patterns_are_the_802_11_matrices():
    """802.11-2012 figure 18-9: per rate the rows A / B of the puncturing matrix over period / 2 trellis steps, 1 = sent;
    mother bit 2 t is A[t], 2 t + 1 is B[t]."""
    matrices = {"2/3": ("11", "10"), "3/4": ("110", "101"), "5/6": ("11010", "10101")}
    for rate, (rowA, rowB) in matrices.items():
        steps = len(rowA)
        assert pc.PERIOD[rate] == 2 * steps
        keep = sorted([2 * t for t in range(steps) if rowA[t] == "1"] + [2 * t + 1 for t in range(steps) if rowB[t] == "1"])
        assert tuple(keep) == pc.KEEP[rate]
        num, den = map(int, rate.split("/"))
        assert steps * den == len(keep) * num                         # `steps` info bits per len(keep) sent bits
        # the kept index of a long block is the pattern repeated, cut at 2T
        idx = pc.kept_index(rate, 5)
        assert idx.tolist() == [i for i in range(pc.mother_bits(5)) if i % (2 * steps) in keep]
        assert idx[-1] < 16 * 5 + 76


def test_the_column_rule():
    for P in range(6, 40):
        for C_ in fc.COLS:
            c = pc.cols(C_, P)
            assert c <= C_ and (8 * P) % c == 0 and (c == C_ or (8 * P) % (2 * c))
            assert (c != C_) == (C_ == 16 and P % 2 == 1)
            assert c == (8 if (C_ == 16 and P % 2) else C_)


@pytest.mark.parametrize("rate", pc.RATES)
def test_round_trip(rate):
    rng = np.random.default_rng(7)
    for n in (0, 1, 2, 3, 5, 64, 301):
        p = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        for C_ in (1, 8, 16):
            blk = pc.encode(p, C_, rate)
            assert len(blk) == pc.coded_len(n, rate) == fec.coded_len(n, rate)
            assert pc.decode(blk, C_, rate) == (1, p, 0)
            assert pc.decode_values(fc.hard_values(blk), C_, rate) == (1, p, 0)
            # the pad bits of the block are zero, and their values are ignored
            K = pc.kept_bits(rate, n)
            sent_pad = np.flatnonzero(fc.perm(8 * len(blk), pc.cols(C_, len(blk))) >= K)
            assert len(sent_pad) == 8 * len(blk) - K < 8
            assert not np.unpackbits(np.frombuffer(blk, np.uint8))[sent_pad].any()
            assert pc.decode(fc.flip(blk, sent_pad), C_, rate) == (1, p, 0)
    # what the depuncturer hands the decoder: zeros exactly at the positions that were not sent
    blk = pc.encode(b"abc", 1, rate)
    m = pc.mother_values(fc.hard_values(blk), 1, rate)                # (one column: sent order is coded order)
    assert len(m) == 8 * fc.coded_len(3)
    assert np.flatnonzero(m != 0).tolist() == pc.kept_index(rate, 3).tolist()
    assert np.array_equal(m[pc.kept_index(rate, 3)] > 0, fc.conv(fc.info_bits(b"abc"))[pc.kept_index(rate, 3)] != 0)


@pytest.mark.parametrize("rate", pc.RATES)
def test_a_single_flip_anywhere_is_corrected(rate):
    """The punctured codes' free distances are 6, 5 and 4: one flipped sent bit, wherever, decodes to the payload sent
    and is counted (the flipped pad bits are ignored: corrected 0)."""
    p = bytes([0xA7, 0x01, 0xFE])
    for C_ in (1, 16):
        blk = pc.encode(p, C_, rate)
        K = pc.kept_bits(rate, 3)
        where = fc.perm(8 * len(blk), pc.cols(C_, len(blk)))
        for j in range(8 * len(blk)):
            assert pc.decode(fc.flip(blk, [j]), C_, rate) == (1, p, 1 if where[j] < K else 0), (C_, j)


def test_all_erasures_decode_like_the_mother_code():
    n = 12
    want = fc.decode_values(np.zeros(8 * fc.coded_len(n), np.int8))
    assert want == (0, bytes(n), 0)
    for rate in pc.RATES:
        assert pc.decode_values(np.zeros(8 * pc.coded_len(n, rate), np.int8), 16, rate) == want


def test_lengths_that_are_no_block():
    for rate in pc.RATES:
        for m in (0, 5, KNOWN[rate][4] + 1, 4090):
            assert pc.decode(bytes(m), 16, rate) == (0, b"", 0)
        assert pc.decode_values(np.ones(8 * KNOWN[rate][0] + 1, np.int8), 16, rate) == (0, b"", 0)
    assert pc.decode(bytes(10), 16, "2/3") == (0, b"", 0) and pc.decode(bytes(10), 16, "3/4")[0] == 0


# ---- 3. header, exports, layout, the plan checker ----------------------------------------------------------------------
def test_header_exports_and_layout(tmp_path):
    hdr, code = sh.check_header_declares_and_library_exports(
        ["ofdm_fec_coded_len_rate", "ofdm_fec_payload_len_rate", "ofdm_fec_punct_last_ms", "ofdm_fec_encode", "ofdm_fec_decode",
         "ofdm_fec_decode_soft", "ofdm_rx_fec_decode_soft", "ofdm_fec_last_ms"])
    got = sh.check_cfg_layout_matches_header(
        tmp_path, _abi.ofdm_fec_cfg, 32,
        (("r12", "OFDM_FEC_RATE_1_2"), ("r23", "OFDM_FEC_RATE_2_3"), ("r34", "OFDM_FEC_RATE_3_4"), ("r56", "OFDM_FEC_RATE_5_6"),
         ("max_payload", "OFDM_FEC_MAX_PAYLOAD"), ("max_coded", "OFDM_FEC_MAX_CODED")))
    assert [int(got[k]) for k in ("r12", "r23", "r34", "r56")] == [0, 1, 2, 3]
    assert [_abi.OFDM_FEC_RATE_1_2, _abi.OFDM_FEC_RATE_2_3, _abi.OFDM_FEC_RATE_3_4, _abi.OFDM_FEC_RATE_5_6] == [0, 1, 2, 3]
    assert (int(got["max_payload"]), int(got["max_coded"])) == (2040, 4090)
    assert _abi.ofdm_fec_cfg.rate.offset == 8 and int(got["rate"]) == 8 and _abi.ofdm_fec_cfg.reserved.offset == 12
    assert C.sizeof(_abi.ofdm_fec_cfg) == 32


def test_plan_checker(tmp_path):
    """The host arithmetic as a program of its own (the build a sanitizer run uses adds -fsanitize=address,undefined)."""
    exe = str(tmp_path / "punct_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tools", "punct_plan_check.cpp")])
    out = subprocess.check_output([exe]).decode()
    assert out.strip().endswith("punct_plan_check ok")
