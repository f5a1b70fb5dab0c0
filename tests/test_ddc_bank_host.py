"""Host side of the DDC bank (ddc.bank_cfg, the ofdm_ddc_bank_* part of the C ABI, ofdm_demod_bank's argument checks):
no GPU needed."""
import ctypes

import numpy as np
import pytest

import ddc_bank_cases
import stage_harness as sh
from ofdm_uhd_amd import _abi, ddc, ofdm

BANK_FUNCS = ("ofdm_set_ddc_bank", "ofdm_ddc_bank_reset", "ofdm_ddc_bank_count", "ofdm_ddc_bank", "ofdm_ddc_bank_taps",
              "ofdm_ddc_bank_last_ms")


def test_bank_cfg_builder():
    c = ddc.bank_cfg(4, [0.25, -0.25, 0.1], occupied_fraction=200 / 512.0)
    assert (c.struct_size, c.decimation, c.ntaps, c.nlinks) == (ctypes.sizeof(_abi.ofdm_ddc_bank_cfg), 4, 31, 3)
    assert list(c.center_freq)[:3] == [0.25, -0.25, 0.1] and list(c.center_freq)[3:] == [0.0] * 5
    assert np.array_equal(np.ctypeslib.as_array(c.taps)[:31], ddc.design(4, 200 / 512.0))
    c = ddc.bank_cfg(3, [0.5] * 8, taps=[1.0, 0.5])
    assert c.nlinks == 8 and c.ntaps == 2 and c.taps[1] == 0.5 and c.center_freq[7] == 0.5
    assert ddc.bank_cfg(1, [-0.5], taps=np.ones(1024, np.float32)).ntaps == 1024
    for bad in (dict(center_freqs=[]), dict(center_freqs=[0.0] * 9), dict(center_freqs=[0.1], taps=[]),
                dict(center_freqs=[0.1], taps=np.zeros(1025, np.float32)), dict(center_freqs=[0.1, 0.5000001]),
                dict(center_freqs=[-0.51]), dict(center_freqs=[float("nan")])):
        kw = dict(taps=np.ones(3, np.float32))
        kw.update(bad)
        with pytest.raises(ValueError):
            ddc.bank_cfg(4, **kw)
    with pytest.raises(ValueError):
        ddc.bank_cfg(4, [0.1])                    # neither taps nor occupied_fraction


def test_bank_cfg_layout_matches_header(tmp_path):
    got = sh.check_cfg_layout_matches_header(tmp_path, _abi.ofdm_ddc_bank_cfg, 16 + 8 * 8 + 4 * 1024,
                                             macros=[("links", "OFDM_DDC_BANK_MAX_LINKS")])
    assert int(got["links"]) == _abi.OFDM_DDC_BANK_MAX_LINKS == ddc.MAX_LINKS == ddc_bank_cases.MAX_LINKS == 8


def test_header_declares_the_bank_and_the_library_exports_it():
    sh.check_header_declares_and_library_exports(BANK_FUNCS)
    # additions only: the single DDC's struct is what it was
    assert ctypes.sizeof(_abi.ofdm_ddc_cfg) == 24 + 4 * 1024


def test_entry_points_refuse_a_null_handle_without_a_gpu():
    lib = _abi.load()
    n, k, ms = ctypes.c_uint64(7), ctypes.c_int(7), ctypes.c_double(7.0)
    assert lib.ofdm_set_ddc_bank(None, None) == _abi.OFDM_E_INVAL
    assert lib.ofdm_set_ddc_bank(None, ctypes.byref(ddc.bank_cfg(2, [0.1], taps=[1.0]))) == _abi.OFDM_E_INVAL
    assert lib.ofdm_ddc_bank_reset(None, 0) == _abi.OFDM_E_INVAL
    assert lib.ofdm_ddc_bank_count(None, 10, ctypes.byref(n)) == _abi.OFDM_E_INVAL
    assert lib.ofdm_ddc_bank(None, None, 0, None, 0, 0, ctypes.byref(n)) == _abi.OFDM_E_INVAL
    assert lib.ofdm_ddc_bank_taps(None, 0, None, 0, ctypes.byref(k)) == _abi.OFDM_E_INVAL
    assert lib.ofdm_ddc_bank_last_ms(None, ctypes.byref(ms)) == _abi.OFDM_E_INVAL
    assert (n.value, k.value, ms.value) == (7, 7, 7.0)          # nothing was written


def test_tile_geometry_helper():
    for R in ddc_bank_cases.TAP_GRID:
        for K in ddc_bank_cases.LINK_COUNTS:
            assert ddc_bank_cases.tile_outputs(R, K) in (64, 256, 1024)
        n = ddc_bank_cases.stream_length(R)
        tile = ddc_bank_cases.tile_outputs(R, 8) * R
        assert n <= 60000 + 64 and n % tile != 0 and (R == 1 or n % R != 0)
        taps = ddc_bank_cases.TAP_GRID[R]
        assert len(taps) <= 3 and set(taps) <= {1, R - 1, 31, 155, 1024} and (R not in (2, 64) or 1024 in taps)
    f = ddc_bank_cases.frequencies(np.random.default_rng(1), (0.0, 0.25, -0.3, 0.5))
    assert len(f) == 8 and f[7] == f[2] and all(abs(v) <= 0.5 for v in f)
    assert len(ddc_bank_cases.pick(f, 3)) == 3 and ddc_bank_cases.pick(f, 3)[0] == ddc_bank_cases.pick(f, 3)[2]


@pytest.mark.parametrize("kw", [
    dict(center_freqs=[]), dict(center_freqs=[0.0] * 9), dict(center_freqs=[0.1, 0.6]), dict(center_freqs=[0.1], decimation=0),
    dict(center_freqs=[0.1], decimation=65), dict(center_freqs=[0.1], taps=[]), dict(center_freqs=[0.1], iq_format="u8"),
    dict(center_freqs=[0.1], iq_scale=-1.0), dict(center_freqs=[0.1], callback=3), dict(center_freqs=[0.1, 0.2], options=3),
])
def test_demod_bank_checks_its_arguments_before_any_engine_exists(kw, monkeypatch):
    sh.check_arguments_are_checked_before_any_engine_exists(
        monkeypatch, ofdm.ofdm_demod_bank, ("options", "center_freqs", "decimation"), dict(center_freqs=[0.25], decimation=4), kw)
