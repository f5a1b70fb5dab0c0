"""Host side of the rational-rate transmit stage (ofdm_uhd_amd/tx_resample.py, the ofdm_tx_resamp_* part of the C ABI)
and the float64 model the GPU tests use: no GPU needed.  The model of the definition (tx_resamp_cases.model) builds the
wideband band of each case, the model of the receive stage (resamp_cases.model) tunes to each link and brings it back to
the modem's rate, and the CPU oracle must recover every packet."""
import ctypes
import re

import numpy as np
import pytest

import duc_cases
import resamp_cases
import stage_harness as sh
import tx_resamp_cases as cases
from ofdm_uhd_amd import _abi, benchmark_ofdm_tx, ddc, duc, firdes, ofdm, options, resample, transmit_path, tx_resample

FUNCS = ("ofdm_set_tx_resamp", "ofdm_tx_resamp_reset", "ofdm_tx_resamp_count", "ofdm_tx_resamp", "ofdm_tx_resamp_last_ms")
RATIOS = ((1, 1), (2, 1), (5, 2), (3, 4), (4, 3), (25, 8), (8, 25), (64, 63), (64, 1), (1, 64), (7, 64))


def test_cfg_layout_matches_header(tmp_path):
    st = _abi.ofdm_tx_resamp_cfg
    sh.check_cfg_layout_matches_header(tmp_path, st, 40 + 4 * 1024)
    assert [f for f, _ in st._fields_] == ["struct_size", "interpolation", "decimation", "ntaps", "out_format", "center_freq",
                                           "out_scale", "reserved", "taps"]


def test_header_declares_the_entry_points_and_python_mirrors_them():
    _, code = sh.check_header_declares_and_library_exports(FUNCS)
    assert re.search(r"#define\s+OFDM_TX_RESAMP_MAX_TAPS\s+1024\b", code) and _abi.OFDM_TX_RESAMP_MAX_TAPS == 1024


@pytest.mark.parametrize("occ_frac", [200 / 512.0, 48 / 64.0, 1200 / 2048.0])
@pytest.mark.parametrize("L,M", [(1, 1), (2, 1), (5, 2), (4, 3), (25, 8), (64, 63), (64, 1), (7, 7)])
def test_design_is_the_duc_design_where_the_output_rate_does_not_bind(L, M, occ_frac):
    taps = tx_resample.design(L, M, occ_frac)
    assert taps.dtype == np.float32 and len(taps) % 2 == 1 and 1 <= len(taps) <= _abi.OFDM_TX_RESAMP_MAX_TAPS
    assert np.array_equal(taps, duc.design(L, occ_frac))
    assert np.array_equal(tx_resample.design(L, M, occ_frac, 0.2 / L), duc.design(L, occ_frac, 0.2 / L))
    # ... which is the formula's float64 prototype to float32 rounding: gain L, edge of / (2L), half the gap to 1 / L
    e = occ_frac / (2.0 * L)
    tw = max(0.5 * (1.0 / L - 2 * e), ddc._MIN_TRANSITION)
    want = np.asarray(firdes.low_pass(float(L), 1.0, min(e + tw / 2, 0.5), tw, firdes.WIN_HAMMING))
    assert len(want) == len(taps) and np.max(np.abs(taps - want)) <= 2.0 ** -23 * np.max(np.abs(want))


@pytest.mark.parametrize("L,M,of", [(3, 4, 200 / 512.0), (2, 5, 0.3), (8, 25, 0.25), (1, 2, 0.4), (7, 64, 0.05), (1, 64, 1 / 64.0)])
def test_design_follows_the_formula_where_the_output_rate_binds(L, M, of):
    taps = tx_resample.design(L, M, of)
    e = of / (2.0 * L)
    tw = max(0.5 * (min(1.0 / L, 1.0 / M) - 2 * e), ddc._MIN_TRANSITION)
    want = np.asarray(firdes.low_pass(float(L), 1.0, min(e + tw / 2, 0.5), tw, firdes.WIN_HAMMING), np.float32)
    assert taps.dtype == np.float32 and len(taps) % 2 == 1 and len(taps) <= 1024 and np.array_equal(taps, want)
    assert abs(float(np.sum(taps.astype(np.float64))) - L) < 1e-5 * L
    tw = 0.5 * tw if 0.5 * tw >= ddc._MIN_TRANSITION else 2 * tw
    assert np.array_equal(tx_resample.design(L, M, of, tw),
                          np.asarray(firdes.low_pass(float(L), 1.0, min(e + tw / 2, 0.5), tw, firdes.WIN_HAMMING), np.float32))


def test_design_of_the_cases_and_its_errors():
    assert [len(tx_resample.design(L, M, occ / float(N))) for _, N, occ, _, L, M, _, _ in cases.CASES.values()] == [39, 41, 481]
    for L, M, of in ((3, 4, 0.76), (1, 2, 0.51), (8, 25, 0.33), (1, 64, 0.02)):
        with pytest.raises(ValueError, match="wider than the band"):
            tx_resample.design(L, M, of)
    tx_resample.design(3, 4, 0.75)                        # a link that just fills the band is designed
    with pytest.raises(ValueError, match="more than 1024 taps"):
        tx_resample.design(3, 4, 0.3, transition=0.002)
    with pytest.raises(ValueError, match="more than 1024 taps"):
        tx_resample.design(5, 2, 0.3, transition=0.002)
    for bad in ((0, 1), (65, 1), (1, 0), (1, 65)):
        with pytest.raises(ValueError):
            tx_resample.design(bad[0], bad[1], 0.01)
    for of in (0.0, -0.1, 1.01):
        with pytest.raises(ValueError):
            tx_resample.design(4, 1, of)


@pytest.mark.parametrize("L,M", RATIOS)
def test_count_agrees_with_brute_force_and_is_additive(L, M):
    rng = np.random.default_rng(L * 100 + M)
    for first in (0, 1, 7, M, M + 1, 1000003):
        for n in (0, 1, 2, M - 1, M, 3 * M + 1, 200):
            lo, hi = first * L // M - 2, (first + n) * L // M + 3
            brute = sum(1 for m in range(max(lo, 0), hi) if first <= m * M // L < first + n)
            assert tx_resample.count(first, n, L, M) == cases.count(first, n, L, M) == brute, (first, n)
            assert tx_resample.count(first, n, L, M) == resample.count(first, n, L, M)
        # additive over any segmentation, from first indices with first L no multiple of M included
        cuts = np.sort(rng.integers(0, 500, 6))
        parts = [tx_resample.count(first + a, b - a, L, M) for a, b in zip(np.r_[0, cuts], np.r_[cuts, 500])]
        assert sum(parts) == tx_resample.count(first, 500, L, M)
    assert M == 1 or any((f * L) % M for f in (1, 7, M + 1, 1000003))
    if L < M:
        assert 0 in [tx_resample.count(f, 1, L, M) for f in range(M)]
    if M == 1:
        assert tx_resample.count(5, 9, L, M) == 9 * L


def test_phase_step_follows_the_definition():
    for fc in (0.0, 0.25, -0.25, 0.5, -0.5, 0.1, -1.0 / 3.0 + 0.013, 1e-9, -1e-9):
        f = fc - np.floor(fc)
        want = int(f * 2.0 ** 64) if f < 1.0 else 0
        assert tx_resample.phase_step(fc) == cases.phase_step(fc) == duc_cases.phase_step(fc) == want, fc
    assert tx_resample.phase_step(-1e-20) == 0 and tx_resample.phase_step(0.5) == 1 << 63
    assert tx_resample.phase_step(-0.5) == 1 << 63 and tx_resample.phase_step(-0.25) == 3 << 62
    assert tx_resample.history(39, 5) == 7 and tx_resample.history(1, 3) == 0 and tx_resample.history(1024, 64) == 15


@pytest.mark.parametrize("L,M,ntaps", [(1, 1, 5), (2, 1, 7), (5, 2, 39), (3, 4, 41), (4, 3, 3), (25, 8, 481), (8, 25, 100),
                                       (7, 64, 6), (7, 64, 200), (64, 63, 1024), (1, 64, 130)])
def test_per_phase_model_equals_the_zero_stuffed_form(L, M, ntaps):
    rng = np.random.default_rng(ntaps)
    x = rng.standard_normal(40 + 3 * M + 2 * ntaps // L) + 1j * rng.standard_normal(40 + 3 * M + 2 * ntaps // L)
    h = rng.standard_normal(ntaps)
    for first in (0, 1000003):
        D = cases.phase_step(-1.0 / 3.0 + 0.013)
        y, s = cases.model(x, h, L, M, D, first)
        yz, sz = cases.model_zero_stuffed(x, h, L, M, D, first)
        assert len(y) == len(yz) == cases.count(first, len(x), L, M) > 0
        scale = 1.0 + np.max(s)
        assert np.max(np.abs(y - yz)) <= 1e-9 * scale and np.max(np.abs(s - sz)) <= 1e-9 * scale


def test_model_follows_the_definition_sample_by_sample():
    rng = np.random.default_rng(4)
    for L, M, ntaps in ((1, 1, 1), (3, 4, 2), (3, 2, 7), (4, 7, 9), (5, 2, 31)):
        x = rng.standard_normal(23) + 1j * rng.standard_normal(23)
        h = rng.standard_normal(ntaps)
        fc, first = -1.0 / 3.0 + 0.013, 1000003
        D = cases.phase_step(fc)
        y, s = cases.model(x, h, L, M, D, first)
        n0 = -(-first * L // M)
        assert len(y) == cases.count(first, 23, L, M)
        for o in range(len(y)):
            n = n0 + o
            i, p = n * M // L - first, n * M % L
            assert 0 <= i < 23
            v = sum(h[p + q * L] * x[i - q] for q in range(ntaps) if p + q * L < ntaps and i - q >= 0)
            sa = sum(abs(h[p + q * L]) * abs(x[i - q]) for q in range(ntaps) if p + q * L < ntaps and i - q >= 0)
            r = np.exp(2j * np.pi * (((n * D) % (1 << 64)) / 2.0 ** 64))
            assert abs(y[o] - v * r) <= 1e-12 * (1 + sa) and abs(s[o] - sa) <= 1e-12 * (1 + sa)


@pytest.mark.parametrize("L,ntaps", [(1, 5), (2, 31), (4, 31), (5, 155), (64, 1024), (3, 2)])
def test_model_with_decimation_one_is_the_duc_model(L, ntaps):
    rng = np.random.default_rng(L)
    x = rng.standard_normal(300) + 1j * rng.standard_normal(300)
    h = rng.standard_normal(ntaps)
    for first in (0, 12345):
        D = cases.phase_step(0.1234)
        y, s = cases.model(x, h, L, 1, D, first)
        yd, sd = duc_cases.model(x, h, L, D, first)
        assert len(y) == len(yd) == 300 * L
        assert np.max(np.abs(y - yd)) <= 1e-12 * (1 + np.max(sd)) and np.max(np.abs(s - sd)) <= 1e-12 * (1 + np.max(sd))
    assert np.array_equal(cases.bound(ntaps, L, sd), duc_cases.bound(ntaps, L, sd))   # ceil(ntaps / L) = Q + 1


def test_cfg_builder():
    c = tx_resample.tx_resamp_cfg(5, 2, -0.25, occupied_fraction=200 / 512.0)
    assert (c.struct_size, c.interpolation, c.decimation, c.ntaps, c.center_freq) == (
        ctypes.sizeof(_abi.ofdm_tx_resamp_cfg), 5, 2, 39, -0.25)
    assert (c.out_format, c.out_scale, c.reserved) == (_abi.OFDM_IQ_FC32, 0.0, 0)
    assert np.array_equal(np.ctypeslib.as_array(c.taps)[:39], tx_resample.design(5, 2, 200 / 512.0))
    c = tx_resample.tx_resamp_cfg(3, 4, taps=[1.0, 0.5], out_format="sc16", out_scale=1000.0)
    assert (c.ntaps, c.taps[1], c.center_freq) == (2, 0.5, 0.0) and (c.out_format, c.out_scale) == (_abi.OFDM_IQ_SC16, 1000.0)
    with pytest.raises(ValueError):
        tx_resample.tx_resamp_cfg(3, 4, 0.1)
    with pytest.raises(ValueError):
        tx_resample.tx_resamp_cfg(3, 4, 0.1, taps=np.zeros(1025, np.float32))
    with pytest.raises(ValueError):
        tx_resample.tx_resamp_cfg(3, 4, 0.1, taps=[1.0], out_format="u8")
    with pytest.raises(ValueError):
        tx_resample.tx_resamp_cfg(3, 4, 0.1, occupied_fraction=0.9)


def test_entry_points_refuse_a_null_handle_without_a_gpu():
    lib = _abi.load()
    n = ctypes.c_uint64(0)
    ms = ctypes.c_double(0)
    assert lib.ofdm_set_tx_resamp(None, None) == _abi.OFDM_E_INVAL
    assert lib.ofdm_tx_resamp_reset(None, 0) == _abi.OFDM_E_INVAL
    assert lib.ofdm_tx_resamp_count(None, 0, ctypes.byref(n)) == _abi.OFDM_E_INVAL
    assert lib.ofdm_tx_resamp(None, None, 0, None, None, 0, ctypes.byref(n)) == _abi.OFDM_E_INVAL
    assert lib.ofdm_tx_resamp_last_ms(None, ctypes.byref(ms)) == _abi.OFDM_E_INVAL


def test_modulator_refuses_both_stages_before_any_engine_exists(monkeypatch):
    def no_engine(*a, **kw):
        raise AssertionError("an engine was created")
    monkeypatch.setattr(ofdm.engine, "Engine", no_engine)
    opt = options.default_options(modulation="qpsk")
    with pytest.raises(ValueError, match="not both"):
        ofdm.ofdm_mod(opt, duc=dict(interpolation=4, center_freq=0.1), resample=dict(interpolation=5, decimation=2))
    opt.tx_amplitude = 0.25
    with pytest.raises(ValueError, match="not both"):
        transmit_path.transmit_path(opt, duc=dict(interpolation=4, center_freq=0.1),
                                    resample=dict(interpolation=5, decimation=2))


def test_command_line_flags_reach_the_transmit_path(monkeypatch):
    opts, _ = benchmark_ofdm_tx.make_parser().parse_args(["--tx-resamp-interp", "5", "--tx-resamp-decim", "2",
                                                          "--tx-resamp-freq", "-0.21"])
    assert (opts.tx_resamp_interp, opts.tx_resamp_decim, opts.tx_resamp_freq) == (5, 2, -0.21)
    assert options.tx_resamp_from_options(opts) == dict(interpolation=5, decimation=2, center_freq=-0.21)
    none, _ = benchmark_ofdm_tx.make_parser().parse_args([])
    assert options.tx_resamp_from_options(none) is None and options.tx_resamp_from_options(options.default_options()) is None
    only, _ = benchmark_ofdm_tx.make_parser().parse_args(["--tx-resamp-decim", "3"])
    assert options.tx_resamp_from_options(only) == dict(interpolation=1, decimation=3, center_freq=0.0)
    seen = {}

    class fake_mod(object):
        def __init__(self, o, **kw):
            seen.update(kw)

        def engine(self):
            return self

        def set_tx_amplitude(self, a):
            pass

    monkeypatch.setattr(transmit_path.ofdm, "ofdm_mod", fake_mod)
    transmit_path.transmit_path(opts)
    assert seen["resample"] == dict(interpolation=5, decimation=2, center_freq=-0.21) and seen["duc"] is None
    transmit_path.transmit_path(none)
    assert seen["resample"] is None
    transmit_path.transmit_path(none, resample=dict(interpolation=3, decimation=4))
    assert seen["resample"] == dict(interpolation=3, decimation=4)


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_model_band_decodes_through_the_receive_model_in_the_oracle(orc, name):
    """Float64 tx_resamp_cases.model (the links of a case, each added onto the band) -> the noise of resamp_cases ->
    float64 resamp_cases.model per link with resample.design(M, L, of) -> orc.rx: all four payloads of every link, and
    no part of the noisy band reaches the 16-bit rail at scale 2^15."""
    k = cases.links(name, orc)
    L, M = k["L"], k["M"]
    assert len(k["tx_taps"]) == {"qpsk512_5_2": 39, "qam16_512_3_4": 41, "bpsk64_25_8": 481}[name]
    wide = np.zeros(cases.count(0, len(k["x"][0]), L, M), np.complex128)
    for x, fc in zip(k["x"], k["freqs"]):
        wide += cases.model(x, k["tx_taps"], L, M, cases.phase_step(fc))[0]
    wide += cases.noise(len(wide), k["P"], L, M)
    wide = wide.astype(np.complex64)
    peak = float(max(np.max(np.abs(wide.real)), np.max(np.abs(wide.imag))))
    print("%s: peak |part| of the noisy band = %.3f" % (name, peak))
    assert peak < 32767 / 32768.0
    for fc, sent in zip(k["freqs"], k["payloads"]):
        c = resample.bandpass_taps(k["rx_taps"], fc, M)
        y, _ = resamp_cases.model(wide, c, M, L, resamp_cases.phase_step(fc, M, L))
        got = orc.rx(k["cfg"], y.astype(np.complex64)).packets
        assert [ok for ok, _ in got] == [True] * 4, (name, fc)
        assert [p for _, p in got] == sent, (name, fc)
