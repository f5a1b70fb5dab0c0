"""The soft-output decoder without a GPU: the NumPy model of tests/fec_rel_cases.py (forward and backward sweeps) against
a second route of its own (a Viterbi run with one bit forbidden), against fec_cases's decoder, and against values known
by hand; the ctypes declarations of the three new entry points; ofdm_demod's argument checks (they run before the
constructor opens an engine)."""
import numpy as np
import pytest

import fec_cases as fc
import fec_rel_cases as fr
import punct_cases as pc
from ofdm_uhd_amd import _abi, ofdm, options


def _small_inputs():
    rng = np.random.default_rng(5)
    for n in (0, 3, 4):
        for C_ in (1, 16):
            blk = fc.encode(fr.case_payload(n), C_)
            x = fc.hard_values(blk).astype(np.float64)
            noisy = np.clip(np.rint(20.0 * x + 25.0 * rng.standard_normal(len(x))), -127, 127).astype(np.int8)
            hard = fc.hard_values(fc.flip(blk, rng.choice(8 * len(blk), 5, replace=False)))
            erased = noisy.copy()
            erased[rng.integers(0, 100, len(x)) < 20] = 0
            erased[8:30] = 0
            yield n, C_, "noisy", noisy
            yield n, C_, "hard", hard
            yield n, C_, "erased", erased


def test_sweeps_agree_with_the_forced_bit_route_at_every_info_bit():
    ties = 0
    for n, C_, kind, v in _small_inputs():
        nn, u, d = fr.deltas(v, C_)
        best = int(fr.sweeps(v, C_)[2][-1, 0])
        assert nn == n and len(d) == 8 * (n + 4)
        for t in range(len(d)):
            assert best - fr.forced_alternative(v, t, C_) == d[t], (n, C_, kind, t)
        assert (d >= 0).all() and not (d & 1).any(), (n, C_, kind)
        ties += int((d == 0).sum())
    assert ties > 0                                   # hard values and erasures do tie


@pytest.mark.parametrize("C_", [1, 16])
def test_the_first_three_fields_are_fec_cases(C_):
    for n in fr.SIZES:
        for kind in fr.KINDS:
            x = fr.case(n, C_, kind)
            want = fc.decode(x, C_) if kind == "flips" else fc.decode_values(x, C_)
            got = fr.case_model(n, C_, kind)
            assert got[:3] == want and got[3].dtype == np.uint8 and len(got[3]) == n, (n, kind)
    for level in (25, 26, 127):
        for n in (4, 219):
            v = fr.clean_values(n, C_, level)
            assert fr.decode_values(v, C_)[:3] == fc.decode_values(v, C_) == (1, fr.case_payload(n), 0)


def test_punctured_route_keeps_the_first_three_fields():
    rng = np.random.default_rng(6)
    for rate in pc.RATES:
        for n in (4, 37):
            blk = pc.encode(fr.case_payload(n), 16, rate)
            v = np.clip(np.rint(30.0 * fc.hard_values(blk) + 12.0 * rng.standard_normal(8 * len(blk))), -127, 127).astype(np.int8)
            got = fr.decode_values_rate(v, 16, rate)
            assert got[:3] == pc.decode_values(v, 16, rate) and len(got[3]) == n
            assert fr.decode_rate(blk, 16, rate)[:3] == (1, fr.case_payload(n), 0)
    assert pc.payload_len(6, "3/4") is None
    assert fr.same(fr.decode_rate(bytes(6), 16, "3/4"), (0, b"", 0, np.zeros(0, np.uint8)))


def test_all_zero_values_tie_everywhere():
    """Every path has metric 0: the decoded payload is all zeros (the tie rule), and so is every reliability."""
    for n in (0, 5, 12):
        ok, payload, corrected, q = fr.decode_values(np.zeros(8 * fc.coded_len(n), np.int8), 16)
        assert payload == bytes(n) and corrected == 0 and q.tolist() == [0] * n
        assert not fr.deltas(np.zeros(8 * fc.coded_len(n), np.int8), 16)[2].any()


@pytest.mark.parametrize("C_", [1, 16])
def test_clean_block_levels(C_):
    """Free distance 10: the nearest wrong path differs in 10 coded bits, Delta / 2 = 10 |v|.  250 at |v| = 25, the clamp
    255 from |v| = 26 on.  The block's ends are no different: the six tail steps leave room for a weight-10 detour from the
    last info bit, the first info bit starts one, and the four ignored pad positions lie behind step T - 1 -- so the
    model gives 10 |v| at every info bit, CRC bits included, and that is asserted."""
    for n in (0, 4, 12):
        for level in (1, 25, 26, 127):
            v = fr.clean_values(n, C_, level)
            _, _, d = fr.deltas(v, C_)
            assert (d == 20 * level).all(), (n, level)
            assert fr.decode_values(v, C_)[3].tolist() == [min(255, 10 * level)] * n


def test_no_block_lengths_give_nothing():
    for m in (0, 8, 9, 11, fc.MAX_CODED + 2):
        assert fr.same(fr.decode(bytes(m)), (0, b"", 0, np.zeros(0, np.uint8)))
        assert fr.same(fr.decode_values(np.ones(8 * m, np.int8)), (0, b"", 0, np.zeros(0, np.uint8)))
    assert fr.same(fr.decode_values(np.ones(8 * 10 + 3, np.int8)), (0, b"", 0, np.zeros(0, np.uint8)))


def test_the_library_declares_the_three_entry_points():
    lib = _abi.load()
    for name in ("ofdm_fec_decode_rel", "ofdm_fec_decode_soft_rel", "ofdm_rx_fec_decode_soft_rel"):
        assert name in _abi.EXPORTS and hasattr(lib, name)
    assert len(lib.ofdm_fec_decode_rel.argtypes) == len(lib.ofdm_fec_decode.argtypes) + 2
    assert len(lib.ofdm_rx_fec_decode_soft_rel.argtypes) == len(lib.ofdm_rx_fec_decode_soft.argtypes) + 2
    assert _abi.OFDM_ABI_VERSION == 6
    # a null handle is refused before any HIP call
    assert lib.ofdm_fec_decode_rel(None, None, None, None, None, 0, None, 0, None, None, None, None, 0) == _abi.OFDM_E_INVAL


def test_ofdm_demod_argument_checks():
    opt = options.default_options(modulation="qpsk", fft_length=64, occupied_tones=48, cp_length=16)
    for bad in (dict(rs=dict(erasures=True, source="fec")),                             # no inner code to ask
                dict(rs=dict(erasures=True, source="fec"), soft=True),
                dict(rs=dict(erasures=True, source="soft"), soft=True),                 # no such source
                dict(rs=dict(erasures=True, source="demapper"), soft=True, fec=True),
                dict(rs=dict(source="fec"), fec=True),                                  # needs erasures=True
                dict(rs=dict(erasures=True, source="fec", max_erasures=33), fec=True),
                dict(rs=dict(erasures=True), soft=True, fec=True),                      # as before: no source named
                dict(rs=dict(erasures=True))):
        with pytest.raises(ValueError):
            ofdm.ofdm_demod(opt, **bad)
    with pytest.raises(ValueError, match='source="fec"'):
        ofdm.ofdm_demod(opt, rs=dict(erasures=True), soft=True, fec=True)
