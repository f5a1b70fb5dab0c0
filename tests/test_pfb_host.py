"""Host side of the polyphase-FFT channeliser (pfb.design, pfb.pfb_cfg, the float64 model of pfb_cases, the ofdm_pfb_*
part of the C ABI): no GPU needed."""
import ctypes
import re

import numpy as np
import pytest

import ddc_cases
import pfb_cases
import stage_harness as sh
from ofdm_uhd_amd import _abi, ddc, ofdm, pfb

PFB_FUNCS = ("ofdm_set_pfb", "ofdm_pfb_reset", "ofdm_pfb_count", "ofdm_pfb", "ofdm_pfb_last_ms")


def test_design_is_the_ddc_design_at_decimation_m():
    for M, of, tr in ((2, 1200 / 2048.0, 0.1), (4, 200 / 512.0, None), (8, 0.75, None), (64, 0.75, None), (64, 0.2, 0.01)):
        assert np.array_equal(pfb.design(M, of, tr), ddc.design(M, of, tr))
    with pytest.raises(ValueError):
        pfb.design(4, 0.0)


def test_pfb_cfg_builder():
    c = pfb.pfb_cfg(4, occupied_fraction=200 / 512.0)
    assert (c.struct_size, c.nchannels, c.ntaps, c.nsel) == (ctypes.sizeof(_abi.ofdm_pfb_cfg), 4, 31, 4)
    assert list(c.channel)[:4] == [0, 1, 2, 3] and list(c.channel)[4:] == [0] * 60
    assert np.array_equal(np.ctypeslib.as_array(c.taps)[:31], ddc.design(4, 200 / 512.0))
    assert ctypes.sizeof(_abi.ofdm_pfb_cfg) == 16 + 64 + 4 * 1024
    # signed channels are taken mod M; repeats and any order are allowed
    c = pfb.pfb_cfg(8, [-4, -1, 3, 3, 0, 7], taps=[1.0, 0.5])
    assert c.nsel == 6 and list(c.channel)[:6] == [4, 7, 3, 3, 0, 7] and c.ntaps == 2 and c.taps[1] == 0.5
    assert pfb.pfb_cfg(64, [-32], taps=np.ones(1024, np.float32)).channel[0] == 32
    assert pfb.pfb_cfg(2, [1, 0], taps=[1.0]).nsel == 2                       # ntaps < M
    for bad in (dict(nchannels=0), dict(nchannels=1), dict(nchannels=3), dict(nchannels=12), dict(nchannels=128),
                dict(nchannels=4.5), dict(channels=[]), dict(channels=[0] * 5), dict(channels=[4]), dict(channels=[-3]),
                dict(channels=[0, 64]), dict(taps=[]), dict(taps=np.zeros(1025, np.float32)),
                dict(taps=[1.0, float("nan")]), dict(taps=[float("inf")])):
        kw = dict(nchannels=4, taps=np.ones(3, np.float32))
        kw.update(bad)
        with pytest.raises(ValueError):
            pfb.pfb_cfg(**kw)
    with pytest.raises(ValueError):
        pfb.pfb_cfg(4, [1])                           # neither taps nor occupied_fraction


@pytest.mark.parametrize("M,ntaps,first", [(2, 1024, 0), (4, 3, 7), (4, 31, 1000003), (8, 155, 5), (16, 17, 16), (64, 63, 0),
                                           (64, 1024, 1000003), (8, 1, 3)])
def test_model_is_the_ddc_model_with_the_grid_table(M, ntaps, first):
    rng = np.random.default_rng(M + ntaps)
    n = 700 + 3 * ntaps
    x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    h = pfb_cases.taps_for(rng, ntaps)
    k = np.arange(ntaps)
    for c in sorted({0, 1, M // 2, M - 1}):
        y, s = pfb_cases.model(x, h, M, c, first)
        table = h.astype(np.float64) * np.exp(2j * np.pi * ((c * k) % M) / M)
        y2, s2 = ddc_cases.model(x, table, M, 0, first)
        assert len(y) == len(y2) == pfb_cases.count(first, n, M) == ddc_cases.count(first, n, M)
        assert np.max(np.abs(y - y2)) <= 1e-12 * np.max(np.abs(y2))
        assert np.max(np.abs(s - s2)) <= 1e-12 * np.max(s2)
    for a, m in ((0, 0), (0, 1), (5, 2), (1000003, 4097), (63, 1)):
        assert pfb_cases.count(a, m, M) == ddc_cases.count(a, m, M)
    assert len(pfb_cases.model(x[:0], h, M, 0, first)[0]) == 0


@pytest.mark.parametrize("name", sorted(pfb_cases.ON_GRID))
def test_on_grid_captures_decode_through_the_float64_model(orc, name):
    """The reference chain alone passes the end-to-end condition the GPU test uses."""
    cap = ddc_cases.capture(name)
    M, chans = pfb_cases.ON_GRID[name]
    assert M == cap["R"] and [c / float(M) for c in chans] == [f % 1.0 for f in cap["freqs"]]
    for c, sent in zip(chans, cap["payloads"]):
        y, _ = pfb_cases.model(cap["wide"], cap["taps"], M, c)
        got = orc.rx(cap["cfg"], np.ascontiguousarray(y.astype(np.complex64))).packets
        assert [ok for ok, _ in got] == [True] * 4 and [p for _, p in got] == sent, (name, c)


def test_header_declares_the_channeliser_and_the_library_exports_it():
    _, code = sh.check_header_declares_and_library_exports(PFB_FUNCS)
    assert re.search(r"#define\s+OFDM_PFB_MAX_CHANNELS\s+64\b", code) and _abi.OFDM_PFB_MAX_CHANNELS == pfb.MAX_CHANNELS == 64
    assert re.search(r"#define\s+OFDM_PFB_MAX_TAPS\s+1024\b", code) and _abi.OFDM_PFB_MAX_TAPS == pfb.MAX_TAPS == 1024


def test_entry_points_refuse_a_null_handle_without_a_gpu():
    lib = _abi.load()
    n, ms = ctypes.c_uint64(7), ctypes.c_double(7.0)
    good = pfb.pfb_cfg(2, [1], taps=[1.0])
    wrong = pfb.pfb_cfg(2, [1], taps=[1.0])
    wrong.struct_size = 12
    assert lib.ofdm_set_pfb(None, None) == _abi.OFDM_E_INVAL
    assert lib.ofdm_set_pfb(None, ctypes.byref(good)) == _abi.OFDM_E_INVAL
    assert lib.ofdm_set_pfb(None, ctypes.byref(wrong)) == _abi.OFDM_E_INVAL
    assert lib.ofdm_pfb_reset(None, 0) == _abi.OFDM_E_INVAL
    assert lib.ofdm_pfb_count(None, 10, ctypes.byref(n)) == _abi.OFDM_E_INVAL
    assert lib.ofdm_pfb(None, None, 0, None, 0, 0, ctypes.byref(n)) == _abi.OFDM_E_INVAL
    assert lib.ofdm_pfb_last_ms(None, ctypes.byref(ms)) == _abi.OFDM_E_INVAL
    assert (n.value, ms.value) == (7, 7.0)            # nothing was written


def test_shapes_of_the_gpu_tests():
    assert sorted(pfb_cases.TAP_GRID) == list(pfb_cases.CHANNEL_COUNTS) == list(pfb.CHANNEL_COUNTS)
    for M, taps in pfb_cases.TAP_GRID.items():
        assert len(taps) <= 3 and set(taps) <= {1, M - 1, M, M + 1, 31, 155, 1024} and (M not in (2, 64) or 1024 in taps)
        n, tile = pfb_cases.stream_length(M), pfb_cases.tile_outputs(M) * M
        assert 2 * tile < n < 3 * tile and n % tile != 0 and n % M != 0
        sizes = pfb_cases.chunk_sizes(np.random.default_rng(M), 3 * tile + 1234 + 3 * 1024, M, 1024)
        assert {0, 1, M - 1, M, M + 1, 1022, 1023, 1024, 997, tile - 1, tile + 1} <= set(sizes)
        assert sum(sizes) == 3 * tile + 1234 + 3 * 1024


@pytest.mark.parametrize("kw", [
    dict(nchannels=3), dict(nchannels=128), dict(channels=[]), dict(channels=[4]), dict(channels=[0, 1, 2, 3, 0]),
    dict(taps=[]), dict(taps=[float("nan")]), dict(iq_format="u8"), dict(iq_scale=-1.0), dict(callback=3), dict(options=3),
])
def test_demod_channelizer_checks_its_arguments_before_any_engine_exists(kw, monkeypatch):
    sh.check_arguments_are_checked_before_any_engine_exists(
        monkeypatch, ofdm.ofdm_demod_channelizer, ("options", "nchannels"), dict(nchannels=4, channels=[1, 3]), kw)
    assert issubclass(ofdm.ofdm_demod_channelizer, ofdm.ofdm_demod_bank)
