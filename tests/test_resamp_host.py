"""Host side of the rational-rate front end (ofdm_uhd_amd/resample.py, the ofdm_resamp_* part of the C ABI) and the
fixtures the GPU tests use: no GPU needed.  The float64 model of the definition (resamp_cases.model) is applied to the
wideband captures and its output is fed to the CPU oracle: every sent packet must come back."""
import ctypes
import re

import numpy as np
import pytest

import resamp_cases
import stage_harness as sh
from ofdm_uhd_amd import _abi, ddc, firdes, ofdm, options, resample

RESAMP_FUNCS = ("ofdm_set_resamp", "ofdm_resamp_reset", "ofdm_resamp_count", "ofdm_resamp", "ofdm_resamp_taps",
                "ofdm_resamp_last_ms")


@pytest.mark.parametrize("name,ntaps", [("qpsk512_2_5", 39), ("qam16_512_4_3", 23), ("bpsk64_8_25", 481)])
def test_design_is_the_ddc_design_at_the_decimation_with_gain_L(name, ntaps):
    mod, N, occ, CP, L, M, freqs, plen = resamp_cases.CASES[name]
    of = occ / float(N)
    taps = resample.design(L, M, of)
    assert taps.dtype == np.float32 and len(taps) == ntaps and ntaps % 2 == 1
    tw = max((1.0 - of) / (2.0 * M), ddc._MIN_TRANSITION)
    want = np.asarray(firdes.low_pass(float(L), 1.0, of / (2.0 * M) + tw / 2.0, tw), np.float32)
    assert np.array_equal(taps, want)
    assert abs(float(np.sum(taps.astype(np.float64))) - L) < 1e-6 * L
    # the same shape as the DDC's prototype at R = M, L times as high
    assert np.allclose(taps, L * ddc.design(M, of).astype(np.float64), rtol=1e-6, atol=0)


def test_design_refuses_a_link_wider_than_the_capture():
    with pytest.raises(ValueError):
        resample.design(4, 3, 0.8)                 # 0.8 * 4 > 3
    with pytest.raises(ValueError):
        resample.design(2, 1, 0.51)
    assert len(resample.design(4, 3, 0.75)) % 2 == 1      # of * L == M: the link fills the capture
    for bad in ((0, 1), (65, 1), (1, 0), (1, 65)):
        with pytest.raises(ValueError):
            resample.design(bad[0], bad[1], 0.1)
    with pytest.raises(ValueError):
        resample.design(2, 5, 0.4, transition=1e-4)
    assert len(resample.design(1, 64, 0.99)) <= _abi.OFDM_RESAMP_MAX_TAPS


def test_count_against_brute_force_and_additive_over_segmentations():
    rng = np.random.default_rng(1)
    for L, M in ((1, 1), (1, 3), (2, 5), (3, 2), (5, 2), (7, 1), (8, 25), (64, 63), (63, 64)):
        for first in (0, 1, 5, 64, 1003):
            for n in (0, 1, 2, 24, 25, 26, 130):
                lo = first * L // M - 2
                want = sum(1 for m in range(max(lo, 0), (first + n) * L // M + 3) if first <= m * M // L < first + n)
                assert resamp_cases.count(first, n, L, M) == want == resample.count(first, n, L, M), (L, M, first, n)
            cuts = np.sort(rng.integers(0, 500, 6))
            parts = sum(resamp_cases.count(first + a, b - a, L, M) for a, b in zip(np.r_[0, cuts], np.r_[cuts, 500]))
            assert parts == resamp_cases.count(first, 500, L, M)


@pytest.mark.parametrize("L,M,first", [(2, 5, 0), (3, 4, 7), (5, 2, 1000003), (1, 3, 5), (7, 1, 3), (64, 63, 11)])
def test_per_phase_form_equals_the_convolution_form(L, M, first):
    rng = np.random.default_rng(L * 100 + M)
    x = rng.standard_normal(300) + 1j * rng.standard_normal(300)
    for ntaps in (1, L, 2 * L + 1, 155):
        h = (rng.standard_normal(ntaps) / np.sqrt(ntaps)).astype(np.float32)
        c = resample.bandpass_taps(h, 0.137, L)
        D = resamp_cases.phase_step(0.137, L, M)
        a, sa = resamp_cases.model_zero_stuffed(x, c, L, M, D, first)
        b, sb = resamp_cases.model(x, c, L, M, D, first)
        assert len(a) == len(b) == resamp_cases.count(first, len(x), L, M) > 0
        assert np.max(np.abs(a - b)) <= 1e-9 and np.max(np.abs(sa - sb)) <= 1e-9
        if ntaps < L:
            assert np.any(b == 0)             # a phase without a tap


def test_phase_step_follows_the_definition():
    assert resamp_cases.phase_step(-1e-20, 1, 4) == 0
    assert resamp_cases.phase_step(0.25, 1, 4) == 0 and resamp_cases.phase_step(0.5, 1, 3) == 1 << 63
    assert resamp_cases.phase_step(0.5, 2, 1) == 1 << 62 and resamp_cases.phase_step(-0.25, 2, 6) == 1 << 62
    # L = 1 is the DDC's
    import ddc_cases
    for fc in (0.0, 0.25, -1.0 / 3.0 + 0.013, 0.5):
        assert resamp_cases.phase_step(fc, 1, 3) == ddc_cases.phase_step(fc, 3)


@pytest.mark.parametrize("fc", [0.0, 0.25, -1.0 / 3.0 + 0.013, 0.5])
def test_bandpass_taps_is_the_float64_evaluation_rounded_once(fc):
    h = resample.design(8, 25, 0.75)
    k = np.arange(len(h))
    got = resample.bandpass_taps(h, fc, 8)
    direct = (h.astype(np.float64) * np.exp(2j * np.pi * fc * k / 8.0)).astype(np.complex64)
    assert got.dtype == np.complex64
    assert np.max(np.abs(got.astype(np.complex128) - direct.astype(np.complex128))) <= 2.0 ** -24 * np.max(np.abs(h))
    assert np.array_equal(resample.bandpass_taps(h, fc, 1), ddc.bandpass_taps(h, fc))


def test_header_declares_the_entry_points_and_the_library_exports_them():
    hdr, code = sh.check_header_declares_and_library_exports(RESAMP_FUNCS)
    assert re.search(r"#define\s+OFDM_RESAMP_MAX_TAPS\s+1024\b", code) and _abi.OFDM_RESAMP_MAX_TAPS == 1024
    assert "rational_resampler_ccf" in hdr


def test_resamp_cfg_layout_matches_header(tmp_path):
    sh.check_cfg_layout_matches_header(tmp_path, _abi.ofdm_resamp_cfg, 24 + 4 * 1024)


def test_resamp_cfg_builder():
    c = resample.resamp_cfg(2, 5, -0.21, occupied_fraction=200 / 512.0)
    assert (c.struct_size, c.interpolation, c.decimation, c.ntaps, c.center_freq) == (
        ctypes.sizeof(_abi.ofdm_resamp_cfg), 2, 5, 39, -0.21)
    assert np.array_equal(np.ctypeslib.as_array(c.taps)[:39], resample.design(2, 5, 200 / 512.0))
    c = resample.resamp_cfg(3, 2, taps=[1.0, 0.5])
    assert c.ntaps == 2 and c.taps[1] == 0.5 and c.center_freq == 0.0
    with pytest.raises(ValueError):
        resample.resamp_cfg(3, 2, 0.1)
    with pytest.raises(ValueError):
        resample.resamp_cfg(3, 2, 0.1, taps=np.zeros(1025, np.float32))


def test_entry_points_refuse_a_null_handle_without_a_gpu():
    lib = _abi.load()
    n = ctypes.c_uint64(0)
    assert lib.ofdm_set_resamp(None, None) == _abi.OFDM_E_INVAL
    assert lib.ofdm_resamp_count(None, 10, ctypes.byref(n)) == _abi.OFDM_E_INVAL
    assert lib.ofdm_resamp(None, None, 0, None, 0, ctypes.byref(n)) == _abi.OFDM_E_INVAL


def test_demod_refuses_two_front_ends_before_any_engine_exists(monkeypatch):
    from ofdm_uhd_amd import engine

    def no_engine(*a, **kw):
        raise AssertionError("an engine was created")
    monkeypatch.setattr(engine, "Engine", no_engine)
    with pytest.raises(ValueError):
        ofdm.ofdm_demod(options.default_options(modulation="qpsk"), ddc=dict(decimation=4, center_freq=0.25),
                        resample=dict(interpolation=2, decimation=5))


def test_command_line_options_reach_the_front_end():
    from ofdm_uhd_amd import benchmark_ofdm_rx
    opt, _ = benchmark_ofdm_rx.make_parser().parse_args(["--resamp-interp", "2", "--resamp-decim", "5", "--resamp-freq", "-0.21"])
    assert options.resamp_from_options(opt) == dict(interpolation=2, decimation=5, center_freq=-0.21)
    opt, _ = benchmark_ofdm_rx.make_parser().parse_args([])
    assert options.resamp_from_options(opt) is None and options.resamp_from_options(options.default_options()) is None
    opt, _ = benchmark_ofdm_rx.make_parser().parse_args(["--resamp-decim", "3"])
    assert options.resamp_from_options(opt) == dict(interpolation=1, decimation=3, center_freq=0.0)


@pytest.mark.parametrize("name", sorted(resamp_cases.CASES))
def test_model_output_decodes_in_the_oracle(orc, name):
    """Pins the fixtures: the float64 model of the definition, applied to each link of the wideband capture and
    rounded to complex64, gives a stream at the modem's rate from which the oracle recovers every sent packet."""
    cap = resamp_cases.capture(name)
    L, M = cap["L"], cap["M"]
    for fc, sent in zip(cap["freqs"], cap["payloads"]):
        c = resample.bandpass_taps(cap["taps"], fc, L)
        y, _ = resamp_cases.model(cap["wide"], c, L, M, resamp_cases.phase_step(fc, L, M))
        assert len(y) == resamp_cases.count(0, len(cap["wide"]), L, M)
        got = orc.rx(cap["cfg"], y.astype(np.complex64)).packets
        assert [ok for ok, _ in got] == [True] * 4, (name, fc)
        assert [p for _, p in got] == sent, (name, fc)
