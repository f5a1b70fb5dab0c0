"""Host side of the wideband front end (ofdm_uhd_amd/ddc.py, the ofdm_ddc_* part of the C ABI) and the fixtures the GPU
tests use: no GPU needed.  The float64 model of the definition (ddc_cases.model) is applied to the two-link wideband
captures and its output is fed to the CPU oracle: every sent packet must come back."""
import ctypes
import re

import numpy as np
import pytest

import ddc_cases
import stage_harness as sh
from ofdm_uhd_amd import _abi, ddc, firdes

DDC_FUNCS = ("ofdm_set_ddc", "ofdm_ddc_reset", "ofdm_ddc_count", "ofdm_ddc", "ofdm_ddc_taps", "ofdm_ddc_last_ms")


@pytest.mark.parametrize("R", [2, 3, 4, 8, 64])
@pytest.mark.parametrize("occ_frac", [200 / 512.0, 48 / 64.0, 1200 / 2048.0])
def test_design_gives_odd_tap_counts_within_the_limit(R, occ_frac):
    taps = ddc.design(R, occ_frac)
    assert taps.dtype == np.float32
    assert len(taps) % 2 == 1 and 1 <= len(taps) <= _abi.OFDM_DDC_MAX_TAPS
    # the default transition is half the gap to the first alias, the edge the signal's plus half of it
    tw = (1.0 - occ_frac) / (2.0 * R)
    if firdes.compute_ntaps(1.0, tw) <= _abi.OFDM_DDC_MAX_TAPS:
        want = np.asarray(firdes.low_pass(1.0, 1.0, occ_frac / (2.0 * R) + tw / 2.0, tw), np.float32)
        assert np.array_equal(taps, want)
    else:                                  # (R = 64 at 3/4 occupancy: the transition is widened to fit the limit)
        assert len(taps) >= 1001
    assert abs(float(np.sum(taps.astype(np.float64))) - 1.0) < 1e-6


def test_design_caps_the_transition_at_the_tap_limit():
    taps = ddc.design(64, 0.99)            # half the gap would need > 16000 taps
    assert len(taps) % 2 == 1 and len(taps) <= _abi.OFDM_DDC_MAX_TAPS
    assert len(taps) >= 1001
    with pytest.raises(ValueError):
        ddc.design(4, 0.4, transition=1e-4)
    assert len(ddc.design(8, 0.75)) == 155 and len(ddc.design(4, 200 / 512.0)) == 31


@pytest.mark.parametrize("fc", [0.0, 0.25, -1.0 / 3.0 + 0.013, 0.5])
def test_bandpass_taps_is_the_float64_evaluation_rounded_once(fc):
    h = ddc.design(8, 0.75)
    k = np.arange(len(h))
    direct = (h.astype(np.float64) * np.exp(2j * np.pi * fc * k)).astype(np.complex64)
    got = ddc.bandpass_taps(h, fc)
    assert got.dtype == np.complex64
    # (exp(jx) against cos x + j sin x of the same float64 x: both correctly rounded to well below float32's ulp)
    assert np.max(np.abs(got.astype(np.complex128) - direct.astype(np.complex128))) <= 2.0 ** -24 * np.max(np.abs(h))
    assert np.array_equal(got.real, (h.astype(np.float64) * np.cos(2 * np.pi * fc * k)).astype(np.float32))
    assert np.array_equal(got.imag, (h.astype(np.float64) * np.sin(2 * np.pi * fc * k)).astype(np.float32))


def test_phase_step_and_count_follow_the_definition():
    assert ddc_cases.phase_step(0.25, 4) == 0 and ddc_cases.phase_step(0.5, 3) == 1 << 63 and ddc_cases.phase_step(-0.25, 3) == 1 << 62
    for first in (0, 1, 5, 64, 1000003):
        for n in (0, 1, 2, 63, 64, 65, 997):
            for R in (1, 2, 3, 8, 64):
                want = sum(1 for m in range(first // R, (first + n) // R + 2) if first <= m * R < first + n)
                assert ddc_cases.count(first, n, R) == want


def test_header_declares_the_ddc_entry_points_and_python_mirrors_them():
    hdr, code = sh.check_header_declares_and_library_exports(DDC_FUNCS)
    assert re.search(r"#define\s+OFDM_DDC_MAX_TAPS\s+1024\b", code) and _abi.OFDM_DDC_MAX_TAPS == 1024
    # each entry point names what it replaces
    for word in ("set_decim", "set_center_freq", "freq_xlating_fir_filter_ccf"):
        assert word in hdr, word


def test_ddc_cfg_layout_matches_header(tmp_path):
    sh.check_cfg_layout_matches_header(tmp_path, _abi.ofdm_ddc_cfg, 24 + 4 * 1024)


def test_ddc_cfg_builder():
    c = ddc.ddc_cfg(4, -0.25, occupied_fraction=200 / 512.0)
    assert (c.struct_size, c.decimation, c.ntaps, c.center_freq) == (ctypes.sizeof(_abi.ofdm_ddc_cfg), 4, 31, -0.25)
    assert np.array_equal(np.ctypeslib.as_array(c.taps)[:31], ddc.design(4, 200 / 512.0))
    c = ddc.ddc_cfg(3, 0.1, taps=[1.0, 0.5])
    assert c.ntaps == 2 and c.taps[1] == 0.5
    with pytest.raises(ValueError):
        ddc.ddc_cfg(3, 0.1)
    with pytest.raises(ValueError):
        ddc.ddc_cfg(3, 0.1, taps=np.zeros(1025, np.float32))


def test_entry_points_refuse_a_null_handle_without_a_gpu():
    lib = _abi.load()
    n = ctypes.c_uint64(0)
    assert lib.ofdm_set_ddc(None, None) == _abi.OFDM_E_INVAL
    assert lib.ofdm_ddc_count(None, 10, ctypes.byref(n)) == _abi.OFDM_E_INVAL
    assert lib.ofdm_ddc(None, None, 0, None, 0, ctypes.byref(n)) == _abi.OFDM_E_INVAL


@pytest.mark.parametrize("name", sorted(ddc_cases.CASES))
def test_model_output_decodes_in_the_oracle(orc, name):
    """Pins the fixtures: the float64 model of the definition, applied to each link of the wideband capture and
    rounded to complex64, gives a narrowband stream from which the oracle recovers every sent packet."""
    cap = ddc_cases.capture(name)
    R = cap["R"]
    for fc, sent in zip(cap["freqs"], cap["payloads"]):
        c = ddc.bandpass_taps(cap["taps"], fc)
        y, _ = ddc_cases.model(cap["wide"], c, R, ddc_cases.phase_step(fc, R))
        assert len(y) == ddc_cases.count(0, len(cap["wide"]), R)
        got = orc.rx(cap["cfg"], y.astype(np.complex64)).packets
        assert [ok for ok, _ in got] == [True] * 4, (name, fc)
        assert [p for _, p in got] == sent, (name, fc)
