"""Host side of the wideband transmit stage (ofdm_uhd_amd/duc.py, the ofdm_duc_* part of the C ABI) and the float64
model the GPU tests use: no GPU needed.  The model of the definition (duc_cases.model) builds the two-link wideband
band, the model of the receive stage (ddc_cases.model) tunes to each link and the CPU oracle must recover every packet."""
import ctypes
import re

import numpy as np
import pytest

import ddc_cases
import duc_cases
import stage_harness as sh
from ofdm_uhd_amd import _abi, ddc, duc

DUC_FUNCS = ("ofdm_set_duc", "ofdm_duc_reset", "ofdm_duc", "ofdm_duc_last_ms")


def test_duc_cfg_layout_matches_header(tmp_path):
    sh.check_cfg_layout_matches_header(tmp_path, _abi.ofdm_duc_cfg, 32 + 4 * 1024)


def test_header_declares_the_duc_entry_points_and_python_mirrors_them():
    hdr, code = sh.check_header_declares_and_library_exports(DUC_FUNCS)
    assert re.search(r"#define\s+OFDM_DUC_MAX_TAPS\s+1024\b", code) and _abi.OFDM_DUC_MAX_TAPS == 1024
    for word in ("set_interp", "set_center_freq"):
        assert word in hdr, word


@pytest.mark.parametrize("L", [1, 2, 3, 4, 8, 64])
@pytest.mark.parametrize("occ_frac", [200 / 512.0, 48 / 64.0, 1200 / 2048.0])
def test_design_is_the_interpolation_times_the_ddc_design(L, occ_frac):
    taps = duc.design(L, occ_frac)
    base = ddc.design(L, occ_frac)
    assert taps.dtype == np.float32 and len(taps) % 2 == 1 and 1 <= len(taps) <= _abi.OFDM_DUC_MAX_TAPS
    assert np.array_equal(taps, (np.float32(L) * base).astype(np.float32))
    # unit pass-band gain after zero stuffing: the taps sum to L
    assert abs(float(np.sum(taps.astype(np.float64))) - L) < 1e-5 * L
    assert np.array_equal(duc.design(L, occ_frac, 0.2 / L), (np.float32(L) * ddc.design(L, occ_frac, 0.2 / L)).astype(np.float32))
    with pytest.raises(ValueError):
        duc.design(65, occ_frac)


def test_duc_cfg_builder():
    c = duc.duc_cfg(4, -0.25, occupied_fraction=200 / 512.0)
    assert (c.struct_size, c.interpolation, c.ntaps, c.center_freq) == (ctypes.sizeof(_abi.ofdm_duc_cfg), 4, 31, -0.25)
    assert (c.out_format, c.out_scale) == (_abi.OFDM_IQ_FC32, 0.0)
    assert np.array_equal(np.ctypeslib.as_array(c.taps)[:31], duc.design(4, 200 / 512.0))
    c = duc.duc_cfg(3, 0.1, taps=[1.0, 0.5], out_format="sc16", out_scale=1000.0)
    assert c.ntaps == 2 and c.taps[1] == 0.5 and (c.out_format, c.out_scale) == (_abi.OFDM_IQ_SC16, 1000.0)
    with pytest.raises(ValueError):
        duc.duc_cfg(3, 0.1)
    with pytest.raises(ValueError):
        duc.duc_cfg(3, 0.1, taps=np.zeros(1025, np.float32))
    with pytest.raises(ValueError):
        duc.duc_cfg(3, 0.1, taps=[1.0], out_format="u8")


def test_entry_points_refuse_a_null_handle_without_a_gpu():
    lib = _abi.load()
    n = ctypes.c_uint64(0)
    ms = ctypes.c_double(0)
    assert lib.ofdm_set_duc(None, None) == _abi.OFDM_E_INVAL
    assert lib.ofdm_duc_reset(None, 0) == _abi.OFDM_E_INVAL
    assert lib.ofdm_duc(None, None, 0, None, None, 0, ctypes.byref(n)) == _abi.OFDM_E_INVAL
    assert lib.ofdm_duc_last_ms(None, ctypes.byref(ms)) == _abi.OFDM_E_INVAL


def test_model_follows_the_definition_sample_by_sample():
    """The vectorised model against the definition's double sum written out, from a non-zero first index."""
    rng = np.random.default_rng(4)
    for L, ntaps in ((1, 1), (3, 2), (3, 7), (4, 4), (4, 5), (5, 31)):
        x = rng.standard_normal(23) + 1j * rng.standard_normal(23)
        h = rng.standard_normal(ntaps)
        fc, first = -1.0 / 3.0 + 0.013, 1000003
        D = duc_cases.phase_step(fc)
        y, s = duc_cases.model(x, h, L, D, first)
        assert len(y) == len(s) == 23 * L
        for o in range(len(y)):
            m, p = divmod(o, L)
            v = sum(h[p + q * L] * x[m - q] for q in range(ntaps) if p + q * L < ntaps and m - q >= 0)
            sa = sum(abs(h[p + q * L]) * abs(x[m - q]) for q in range(ntaps) if p + q * L < ntaps and m - q >= 0)
            n = first * L + o
            r = np.exp(2j * np.pi * (((n * D) % (1 << 64)) / 2.0 ** 64))
            assert abs(y[o] - v * r) <= 1e-12 * (1 + sa) and abs(s[o] - sa) <= 1e-12 * (1 + sa)
    assert duc_cases.phase_step(-1e-20) == 0 and duc_cases.phase_step(0.5) == 1 << 63 and duc_cases.phase_step(-0.25) == 3 << 62


@pytest.mark.parametrize("name", sorted(ddc_cases.CASES))
def test_model_band_decodes_through_the_ddc_model_in_the_oracle(orc, name):
    """Float64 duc_cases.model (two links, the second added onto the first) -> the noise of ddc_cases -> float64
    ddc_cases.model per link -> orc.rx: all four payloads of each link, and the noisy band's peak stays below 1."""
    k = duc_cases.links(name, orc)
    R = k["R"]
    wide = np.zeros(len(k["x"][0]) * R, np.complex128)
    for x, fc in zip(k["x"], k["freqs"]):
        wide += duc_cases.model(x, k["tx_taps"], R, duc_cases.phase_step(fc))[0]
    wide += duc_cases.noise(len(wide), k["P"], R)
    wide = wide.astype(np.complex64)
    peak = float(np.max(np.abs(wide)))
    print("%s: peak |sample| of the noisy two-link band = %.3f" % (name, peak))
    assert peak < 1.0
    for fc, sent in zip(k["freqs"], k["payloads"]):
        c = ddc.bandpass_taps(k["rx_taps"], fc)
        y, _ = ddc_cases.model(wide, c, R, ddc_cases.phase_step(fc, R))
        got = orc.rx(k["cfg"], y.astype(np.complex64)).packets
        assert [ok for ok, _ in got] == [True] * 4, (name, fc)
        assert [p for _, p in got] == sent, (name, fc)
