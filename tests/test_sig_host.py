"""The signal field without a GPU: the NumPy model of tests/sig_cases.py against the code's known properties (the Golay
weight distribution, 15 flipped bits corrected, whole copies erased), the 50 valid words through sig.coding and back,
the header and the exports, the payload limits against the codes' own length functions, the ValueErrors of ofdm_mod /
ofdm_demod that need no GPU, suggest_coding on hand-made quality records, the host arithmetic of csrc/sig_plan.h
through the stand-alone checker tools/sig_plan_check.cpp, and the seeded AWGN condition the GPU test relies on:
2048 random words at Es/N0 = -3 dB, values clip(rint(32 y), +-127), all decoded by the model."""
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import sig_cases as sc
from ofdm_uhd_amd import _abi, engine, fec, ldpc, ofdm, ofdm_packet_utils, options, rs, sig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIG_CALLS = ("ofdm_sig_word", "ofdm_sig_word_fields", "ofdm_sig_word_valid", "ofdm_sig_encode", "ofdm_sig_decode",
             "ofdm_sig_decode_soft", "ofdm_rx_sig_decode_soft", "ofdm_sig_last_ms")


# ---- 1. the code ---------------------------------------------------------------------------------------------------------
def test_weight_distribution_and_linearity():
    cb = sc.codebook()
    assert cb.shape == (4096, 24)
    assert np.bincount(cb.sum(axis=1), minlength=25).tolist() == [1 if i in (0, 24) else 759 if i in (8, 16) else 2576 if i == 12
                                                                  else 0 for i in range(25)]
    packed = np.packbits(cb, axis=1)
    packed = (packed[:, 0].astype(np.int64) << 16) | (packed[:, 1].astype(np.int64) << 8) | packed[:, 2]
    assert np.array_equal(packed >> 12, np.arange(4096))                 # systematic: the word's bits first, MSB first
    for a in (1, 0x555, 0x801, 0xFFF):
        assert np.array_equal(packed[np.arange(4096) ^ a], packed ^ packed[a])
    assert packed[0xFFF] == 0xFFFFFF and packed[1] == (0xC75 << 1) | 1   # g itself has weight 7: the parity bit is set


def test_field_image():
    for w in (0, 1, 0x480, 0xFFF, 0xB80):
        img = sc.field_bytes(w)
        assert len(img) == sig.FIELD_BYTES == 12 and img[:3] == img[3:6] == img[6:9] == img[9:]
        assert img[0] == w >> 4 and img[1] >> 4 == w & 0xF
        assert sc.decode_bytes(img) == (w, 2 * 4 * 8)                    # the nearest codewords differ in 8 of 24 bits, in 4 copies
        assert sc.decode_values(sc.clean_values(w)) == (w, 2 * 4 * 8 * 64)
    assert sc.decode_bytes(bytes(11)) == (sc.NO_WORD, 0) and sc.decode_values(np.zeros(88, np.int8)) == (sc.NO_WORD, 0)


# ---- 2. the words --------------------------------------------------------------------------------------------------------
def test_the_50_valid_words_round_trip_and_every_other_value_is_refused():
    valid = sc.valid_words()
    assert len(valid) == 50
    seen = set()
    for w in range(4096):
        if w not in valid:
            assert not sig.word_valid(w)
            with pytest.raises(ValueError):
                sig.coding(w)
            continue
        assert sig.word_valid(w)
        cod = sig.coding(w)
        codec, rate, rs_on, lg = sc.word_fields(w)
        assert (cod.codec, cod.rate, cod.rs) == (codec, rate, bool(rs_on))
        assert cod.interleave == ((1 << lg) if codec == sig.CODEC_FEC else 0)
        assert cod.word == w and sig.coding(cod) is cod
        # the keywords ofdm_mod takes, and back
        again = sig.coding(fec=cod.fec, ldpc=cod.ldpc(), rs=cod.rs)
        assert again == cod and again.word == w
        seen.add(cod)
    assert len(seen) == 50 and seen == set(sig.all_codings())
    for w in (-1, 4096, 0xFFFF, 1 << 40):
        assert not sig.word_valid(w)
        with pytest.raises(ValueError):
            sig.coding(w)
    assert sig.coding() == sig.coding(0) and sig.coding(rs=True).word == 0x080
    assert sig.coding(fec=True).word == (1 << 10) | (4 << 4)                                   # 16 columns, rate 1/2
    assert sig.coding(fec=dict(interleave=1, rate="3/4"), rs=True).word == (1 << 10) | (2 << 8) | (1 << 7)
    assert sig.coding(ldpc=dict(rate="5/6", max_iters=7)).word == (2 << 10) | (3 << 8)         # max_iters is not sent
    with pytest.raises(ValueError):
        sig.coding(fec=True, ldpc=True)
    with pytest.raises(ValueError):
        sig.coding(0, rs=True)
    with pytest.raises(ValueError):
        sig.Coding(sig.CODEC_LDPC, 0, False, 16).word


# ---- 3. the decoder model ------------------------------------------------------------------------------------------------
def test_model_corrects_15_flipped_bits_on_256_seeds():
    rng = np.random.default_rng(15)
    words = rng.integers(0, 4096, 256)
    for seed, w in enumerate(words):
        got, margin = sc.decode_values(sc.flipped(int(w), 15, seed))
        assert got == w and margin > 0, seed
        hard = np.packbits(sc.flipped(int(w), 15, seed) > 0).tobytes()
        assert sc.decode_bytes(hard)[0] == w, seed


def test_model_decodes_with_one_two_or_three_copies_erased():
    for w in (0, 0x480, 0xB80, 0xABC):
        for n in (1, 2, 3):
            for copies in itertools.combinations(range(4), n):
                assert sc.decode_values(sc.erased_copies(w, copies)) == (w, 2 * (4 - n) * 8 * 64), (w, copies)
        assert sc.decode_values(sc.erased_copies(w, (0, 1, 2, 3))) == (0, 0)


def test_tie_rule_and_all_zero():
    assert sc.decode_values(np.zeros(96, np.int8)) == (0, 0)
    assert sc.decode_values(sc.tie_values()) == (0xFF0, 0)
    v = np.full(96, -128, np.int8)
    assert sc.decode_values(v) == (0, 2 * 4 * 8 * 127)                  # -128 reads as -127


def test_seeded_awgn_condition():
    words, vals = sc.awgn_set()
    assert vals.shape == (2048, 96) and vals.dtype == np.int8
    assert (np.abs(vals.astype(np.int16)) == 127).any() and (vals == 0).any()          # the clip and the erasure occur
    hard_wrong = ((vals > 0) != np.tile(sc.codebook()[words], (1, 4)).astype(bool)).sum(axis=1)
    print("awgn set: hard bits wrong per field min %d median %d max %d" % (hard_wrong.min(), np.median(hard_wrong), hard_wrong.max()))
    assert np.median(hard_wrong) >= 10                                  # far from clean
    best, margin = sc.decode_many(vals)
    print("awgn set: %d of %d words wrong, smallest margin %d" % ((best != words).sum(), len(words), margin.min()))
    assert np.array_equal(best, words)
    for i in (0, 1, 2047):
        assert sc.decode_values(vals[i]) == (int(best[i]), int(margin[i]))


# ---- 4. the header, the exports, the lengths --------------------------------------------------------------------------------
def test_exports_equal_the_header():
    hdr = open(os.path.join(ROOT, "include", "ofdm_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(ofdm_[a-z_0-9]+)\s*\(", code))
    assert declared == set(_abi.EXPORTS) and len(set(_abi.EXPORTS)) == len(_abi.EXPORTS)
    lib = _abi.load()
    for name in SIG_CALLS:
        assert name in declared and hasattr(lib, name), name
    assert re.search(r"#define\s+OFDM_ABI_VERSION\s+6\b", code) and lib.ofdm_abi_version() == _abi.OFDM_ABI_VERSION == 6
    assert _abi.K_COUNT == 11 and re.search(r"OFDM_K_COUNT\s*=\s*11\b", code)
    for name, val in (("FIELD_BYTES", 12), ("CODEC_NONE", 0), ("CODEC_FEC", 1), ("CODEC_LDPC", 2), ("NO_WORD", 0xFFFF)):
        assert re.search(r"#define\s+OFDM_SIG_%s\s+(0x)?%s\b" % (name, "FFFF" if val == 0xFFFF else val), code)
        assert getattr(_abi, "OFDM_SIG_" + name) == val
    # the calls that take a handle refuse a null one
    assert lib.ofdm_sig_last_ms(None, None) == _abi.OFDM_E_INVAL
    assert lib.ofdm_sig_encode(None, None, None, None, None, 0, None, 0, None) == _abi.OFDM_E_INVAL
    assert lib.ofdm_sig_decode(None, None, None, None, 0, None, None) == _abi.OFDM_E_INVAL
    assert lib.ofdm_rx_sig_decode_soft(None, None, None, 0, None) == _abi.OFDM_E_INVAL
    assert lib.ofdm_sig_word(0, 0, 0, 0, None) == _abi.OFDM_E_INVAL


def test_max_payload_agrees_with_the_length_functions_for_all_50_codings():
    # what framed_len leaves a packet without padding: payload | CRC-32 | 0x55 within the whitening mask
    limit = len(ofdm_packet_utils.random_mask_tuple) - 4 - 1
    assert limit == 4091 and len(ofdm_packet_utils.make_packet(bytes(limit), 2, 2, pad_for_usrp=False)) == 4 + 4096
    with pytest.raises(ValueError):
        ofdm_packet_utils.whiten(bytes(limit + 1 + 4 + 1), 0)
    own = {sig.CODEC_NONE: lambda c: limit, sig.CODEC_FEC: lambda c: fec.MAX_PAYLOAD, sig.CODEC_LDPC: lambda c: ldpc.max_payload(c.rate)}
    shrunk = 0
    for cod in sig.all_codings():
        n = sig.max_payload(cod)
        assert sig.coded_len(n, cod) <= limit
        try:
            assert sig.coded_len(n + 1, cod) > limit
        except ValueError:
            pass                                                        # the code itself takes no more
        assert sig.coded_len(n, cod) == sig.body_len(n, cod) + 12
        # without the field the same search ends at the limits the link objects use today
        inner = own[cod.codec](cod)
        today = min(rs.max_payload_under(inner), rs.MAX_PAYLOAD) if cod.rs else inner
        assert today - 12 <= n <= today, str(cod)
        shrunk += n < today
        assert sig.max_payload(cod, block_limit=sig.coded_len(n, cod) - 1) < n or n == 0
    assert shrunk >= 3                                                  # uncoded, and the rate-1/2 convolutional code
    assert sig.max_payload(sig.coding()) == 4079 and sig.max_payload(sig.coding(fec=True)) == 2034
    assert sig.max_payload(sig.coding(ldpc=True)) == ldpc.MAX_PAYLOAD and sig.max_payload(sig.coding(rs=True)) == rs.MAX_PAYLOAD - 1
    with pytest.raises(ValueError):
        sig.max_payload(sig.coding(fec=True), block_limit=20)
    with pytest.raises(ValueError):
        sig.coded_len(2041, sig.coding(fec=True))


# ---- 5. the link objects' refusals that need no GPU -----------------------------------------------------------------------------
def test_value_errors_of_the_link_objects():
    opt = options.default_options(modulation="qpsk")
    for kw in (dict(fec=True), dict(fec=dict(rate="3/4")), dict(rs=True), dict(rs=dict(erasures=True)),
               dict(rs=dict(erasures=True, source="ldpc"), ldpc=True), dict(ldpc=dict(rate="2/3")),
               dict(ldpc=dict(max_iters=5, rate="1/2")), dict(ldpc=dict(max_iters=0)), dict(ldpc=65), dict(ldpc="1/2")):
        with pytest.raises(ValueError):
            ofdm.ofdm_demod(opt, sig=True, **kw)
    with pytest.raises(ValueError):
        ofdm.ofdm_mod(opt, pad_for_usrp=False, sig=True, fec=True, ldpc=True)
    with pytest.raises(ValueError):
        ofdm.ofdm_mod(opt, pad_for_usrp=False, sig=True, fec=dict(interleave=3))


# ---- 6. rate suggestion -----------------------------------------------------------------------------------------------------
def _records(snrs):
    q = np.zeros(len(snrs), engine.QUALITY_DTYPE)
    q["snr_preamble_db"] = snrs
    q["snr_decision_db"] = 99.0                                         # not what is read
    return q


def test_suggest_coding_on_hand_made_quality_records():
    table = sig.default_table()
    assert [str(c) for _, c in table] == ["ldpc 1/2", "ldpc 2/3", "ldpc 3/4", "ldpc 5/6", "uncoded"]
    thr = [t for t, _ in table]
    assert thr == sorted(thr)
    assert sig.suggest_coding(_records([]), table) is None and sig.suggest_coding([]) is None       # empty history
    # monotone in SNR: the chosen entry never moves back as the median grows
    picks = [[c for _, c in table].index(sig.suggest_coding(_records([s - 0.3, s, s + 0.2]), table, margin_db=1.0))
             for s in np.arange(-10.0, 20.0, 0.25)]
    assert picks == sorted(picks) and picks[0] == 0 and picks[-1] == len(table) - 1 and set(picks) == set(range(len(table)))
    # the margin is respected: a threshold is cleared at threshold + margin, not below
    for k in range(1, len(table)):
        assert sig.suggest_coding([thr[k] + 1.0], table, margin_db=1.0) == table[k][1]
        assert sig.suggest_coding([thr[k] + 0.99], table, margin_db=1.0) == table[k - 1][1]
        assert sig.suggest_coding([thr[k]], table, margin_db=0.0) == table[k][1]
    # the median, not the mean: one outlier does not move it
    assert sig.suggest_coding(_records([2.0, 2.1, 60.0]), table, margin_db=0.0) == table[1][1]
    # a table of the caller's, codings in any accepted form
    mine = [(0.0, sig.coding(fec=True, rs=True)), (6.0, sig.coding(fec=dict(rate="3/4")).word), (15.0, 0)]
    assert sig.suggest_coding([7.5], mine) == sig.coding(fec=dict(rate="3/4"))
    assert sig.suggest_coding([-30.0], mine) == sig.coding(fec=True, rs=True)
    with pytest.raises(ValueError):
        sig.suggest_coding([1.0], [(5.0, 0), (1.0, 0x080)])
    with pytest.raises(ValueError):
        sig.suggest_coding([1.0], [])


# ---- 7. the host arithmetic as a program of its own ----------------------------------------------------------------------------
def test_plan_checker(tmp_path):
    exe = str(tmp_path / "sig_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tools", "sig_plan_check.cpp")])
    out = subprocess.check_output([exe]).decode()
    assert out.strip().endswith("sig_plan_check ok")


def test_library_words_and_model_image_agree():
    """The library's word functions against the model's table, and the model's codeword against the polynomial division
    done a second way (long division on the bit vector)."""
    lib = _abi.load()
    assert [w for w in range(1 << 13) if lib.ofdm_sig_word_valid(w)] == sc.valid_words()
    for w in (1, 0x480, 0x7FF, 0xFFF):
        num = [(w >> (11 - j)) & 1 for j in range(12)] + [0] * 11
        g = [(sc.GEN >> (11 - j)) & 1 for j in range(12)]
        rem = list(num)
        for i in range(12):
            if rem[i]:
                for j in range(12):
                    rem[i + j] ^= g[j]
        assert sc.codeword_bits(w)[12:23] == rem[12:]
