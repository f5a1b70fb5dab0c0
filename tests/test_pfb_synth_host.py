"""Host side of the polyphase-FFT synthesis bank (pfb.synth_design, pfb.synth_cfg, the float64 model of pfb_synth_cases,
the ofdm_pfb_synth_* part of the C ABI): no GPU needed."""
import ctypes
import os
import re

import numpy as np
import pytest

import duc_cases
import pfb_cases
import pfb_synth_cases as sc
import stage_harness as sh
from ofdm_uhd_amd import _abi, duc, ofdm, pfb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYNTH_FUNCS = ("ofdm_set_pfb_synth", "ofdm_pfb_synth_reset", "ofdm_pfb_synth", "ofdm_pfb_synth_last_ms")


def test_header_declares_the_synthesis_bank_and_the_library_exports_it():
    sh.check_header_declares_and_library_exports(SYNTH_FUNCS)


def test_struct_layout_matches_the_header():
    hdr = open(os.path.join(ROOT, "include", "ofdm_hip.h")).read()
    body = re.search(r"typedef struct ofdm_pfb_synth_cfg \{(.*?)\} ofdm_pfb_synth_cfg;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(uint32_t|uint8_t|float)\s+(\w+)(?:\[(\w+)\])?;", body)
    ctype = {"uint32_t": ctypes.c_uint32, "uint8_t": ctypes.c_uint8, "float": ctypes.c_float}
    dims = {"OFDM_PFB_MAX_CHANNELS": 64, "OFDM_PFB_MAX_TAPS": 1024}
    assert [f[1] for f in fields] == [f[0] for f in _abi.ofdm_pfb_synth_cfg._fields_]
    off = 0
    for (t, name, dim), (pname, ptype) in zip(fields, _abi.ofdm_pfb_synth_cfg._fields_):
        want = ctype[t] * dims[dim] if dim else ctype[t]
        assert ctypes.sizeof(ptype) == ctypes.sizeof(want) and getattr(_abi.ofdm_pfb_synth_cfg, pname).offset == off, name
        off += ctypes.sizeof(want)
    assert ctypes.sizeof(_abi.ofdm_pfb_synth_cfg) == off == 24 + 64 + 4 * 1024


def test_design_is_the_duc_design_at_interpolation_m():
    for M, of, tr in ((2, 1200 / 2048.0, 0.1), (4, 200 / 512.0, None), (8, 0.75, None), (64, 0.75, None)):
        assert np.array_equal(pfb.synth_design(M, of, tr), duc.design(M, of, tr))
    with pytest.raises(ValueError):
        pfb.synth_design(4, 0.0)


def test_synth_cfg_builder_and_its_refusals():
    c = pfb.synth_cfg(4, None, occupied_fraction=200 / 512.0)
    assert (c.struct_size, c.nchannels, c.nsel, c.out_format, c.out_scale) == (ctypes.sizeof(_abi.ofdm_pfb_synth_cfg), 4, 4, 0, 0.0)
    assert list(c.channel)[:4] == [0, 1, 2, 3] and list(c.channel)[4:] == [0] * 60
    assert np.array_equal(np.ctypeslib.as_array(c.taps)[:c.ntaps], duc.design(4, 200 / 512.0))
    # signed channels are taken mod M, any order
    c = pfb.synth_cfg(8, [-4, -1, 3, 0], taps=[1.0, 0.5], out_format="sc16", out_scale=1000.0)
    assert c.nsel == 4 and list(c.channel)[:4] == [4, 7, 3, 0] and c.ntaps == 2 and c.taps[1] == 0.5
    assert (c.out_format, c.out_scale) == (_abi.OFDM_IQ_SC16, 1000.0)
    assert pfb.synth_cfg(64, [-32], taps=np.ones(1024, np.float32)).channel[0] == 32
    assert pfb.synth_cfg(2, [1, 0], taps=[1.0]).nsel == 2                       # ntaps < M
    for bad in (dict(nchannels=0), dict(nchannels=1), dict(nchannels=3), dict(nchannels=12), dict(nchannels=128),
                dict(nchannels=4.5), dict(channels=[]), dict(channels=[0, 1, 2, 3, 0]), dict(channels=[4]),
                dict(channels=[-3]), dict(channels=[1, 1]), dict(channels=[-1, 3]), dict(channels=[0, 2, 0]),
                dict(taps=[]), dict(taps=np.zeros(1025, np.float32)), dict(taps=[1.0, float("nan")]),
                dict(taps=[float("inf")]), dict(out_format="u8"), dict(out_scale=-1.0), dict(out_scale=float("nan"))):
        kw = dict(nchannels=4, channels=[1, 3], taps=np.ones(3, np.float32))
        kw.update(bad)
        with pytest.raises(ValueError):
            pfb.synth_cfg(**kw)
    with pytest.raises(ValueError):
        pfb.synth_cfg(4, [1])                           # neither taps nor occupied_fraction


@pytest.mark.parametrize("M", [32, 64])
def test_two_step_transform_is_the_plain_recursion_to_the_last_bit(M):
    rng = np.random.default_rng(M)
    w = sc.table(M)
    v = (rng.standard_normal((200, M)) + 1j * rng.standard_normal((200, M))).astype(np.complex64)
    v[:50, rng.permutation(M)[:M // 2]] = 0              # columns with channels that are not selected
    a, b = sc.dit(v, w), sc.dit_two_step(v, w)
    assert a.dtype == b.dtype == np.complex64 and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # ... and it is the transform of the definition: V_p = sum_c z_c w[(c p) mod M]
    idx = (np.arange(M)[:, None] * np.arange(M)[None, :]) % M
    want = v.astype(np.complex128) @ np.exp(2j * np.pi * idx / M)
    assert np.max(np.abs(a - want)) <= 8 * np.log2(M) * sc.EPS * np.max(np.sum(np.abs(v), axis=1))


@pytest.mark.parametrize("M", [2, 4, 8, 16])
def test_plain_recursion_is_the_transform_and_passes_channel_zero_through(M):
    rng = np.random.default_rng(M)
    w = sc.table(M)
    v = (rng.standard_normal((100, M)) + 1j * rng.standard_normal((100, M))).astype(np.complex64)
    idx = (np.arange(M)[:, None] * np.arange(M)[None, :]) % M
    want = v.astype(np.complex128) @ np.exp(2j * np.pi * idx / M)
    assert np.max(np.abs(sc.dit(v, w) - want)) <= 8 * np.log2(M) * sc.EPS * np.max(np.sum(np.abs(v), axis=1))
    v[:, 1:] = 0
    assert np.array_equal(sc.dit(v, w), np.repeat(v[:, :1], M, axis=1))      # channel 0 alone: V_p = x exactly


@pytest.mark.parametrize("M,ntaps,first", [(2, 1024, 0), (4, 3, 7), (4, 31, 1000003), (8, 155, 5), (16, 17, 16), (64, 63, 0),
                                           (64, 1024, 1000003), (8, 1, 3)])
def test_model_with_one_channel_is_the_duc_model_on_the_grid(M, ntaps, first):
    rng = np.random.default_rng(M + ntaps)
    n = 300 + 2 * ntaps // M
    x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    h = pfb_cases.taps_for(rng, ntaps)
    for c in sorted({0, 1, M // 2, M - 1}):
        y, s = sc.model(x[None], h, M, [c])
        fc = c / float(M) if c <= M // 2 else (c - M) / float(M)
        y2, s2 = duc_cases.model(x, h, M, duc_cases.phase_step(fc), first)
        assert len(y) == len(y2) == n * M
        assert np.max(np.abs(y - y2)) <= 1e-12 * np.max(np.abs(y2))
        assert np.max(np.abs(s - s2)) <= 1e-12 * np.max(s2)
    # several channels: the sum of the single ones
    y, s = sc.model(np.stack([x, 2 * x]), h, M, [0, M - 1])
    ya, sa = sc.model(x[None], h, M, [0])
    yb, sb = sc.model(2 * x[None], h, M, [M - 1])
    assert np.allclose(y, ya + yb, rtol=0, atol=1e-12 * np.max(np.abs(y))) and np.allclose(s, sa + sb)
    assert len(sc.model(x[None, :0], h, M, [0])[0]) == 0


def test_shapes_of_the_gpu_tests():
    for M, taps in sc.TAP_GRID.items():
        n, T = sc.stream_inputs(M), sc.tile_inputs(M)
        assert 2 * T < n < 3 * T and n % T != 0 and n * M < 10 ** 4
        for ntaps in taps:
            Q = sc.history(ntaps, M)
            sizes = sc.chunk_inputs(np.random.default_rng(M), 3 * T + 100 + 3 * Q, M, ntaps)
            assert sum(sizes) == 3 * T + 100 + 3 * Q and sizes[0] == 0
            assert {1, Q + 1, T - 1, T + 1} | ({Q} if Q else set()) | ({Q - 1} if Q > 1 else set()) <= set(sizes)


def test_entry_points_refuse_a_null_handle_without_a_gpu():
    lib = _abi.load()
    n, ms = ctypes.c_uint64(7), ctypes.c_double(7.0)
    good = pfb.synth_cfg(2, [1], taps=[1.0])
    assert lib.ofdm_set_pfb_synth(None, None) == _abi.OFDM_E_INVAL
    assert lib.ofdm_set_pfb_synth(None, ctypes.byref(good)) == _abi.OFDM_E_INVAL
    assert lib.ofdm_pfb_synth_reset(None, 0) == _abi.OFDM_E_INVAL
    assert lib.ofdm_pfb_synth(None, None, 0, 0, None, None, 0, ctypes.byref(n)) == _abi.OFDM_E_INVAL
    assert lib.ofdm_pfb_synth_last_ms(None, ctypes.byref(ms)) == _abi.OFDM_E_INVAL
    assert (n.value, ms.value) == (7, 7.0)            # nothing was written


@pytest.mark.parametrize("kw", [
    dict(nchannels=3), dict(nchannels=128), dict(channels=[]), dict(channels=[4]), dict(channels=[1, 1]),
    dict(channels=[-1, 3]), dict(taps=[]), dict(taps=[float("nan")]), dict(iq_format="u8"), dict(iq_scale=-1.0),
    dict(options=3),
])
def test_mod_channelizer_checks_its_arguments_before_any_engine_exists(kw, monkeypatch):
    sh.check_arguments_are_checked_before_any_engine_exists(
        monkeypatch, ofdm.ofdm_mod_channelizer, ("options", "nchannels"), dict(nchannels=4, channels=[1, 3]), kw)


def test_mod_channelizer_drops_a_failing_batch_on_every_link():
    sh.check_mod_links_drops_a_failing_batch_on_every_link(ofdm.ofdm_mod_channelizer, "pfb_synth",
                                                           pfb.synth_cfg(4, [0, 1, 2], taps=[1.0]))
