"""Host side of the resampler bank (resample.bank_cfg, the ofdm_resamp_bank_* part of the C ABI, the argument checks of
ofdm_demod_resamp_bank and of the command line): no GPU needed."""
import ctypes

import numpy as np
import pytest

import resamp_bank_cases as bc
import resamp_cases
import stage_harness as sh
from ofdm_uhd_amd import _abi, benchmark_ofdm_rx, ofdm, resample

BANK_FUNCS = ("ofdm_set_resamp_bank", "ofdm_resamp_bank_reset", "ofdm_resamp_bank_count", "ofdm_resamp_bank",
              "ofdm_resamp_bank_taps", "ofdm_resamp_bank_last_ms")


def test_bank_cfg_builder():
    c = resample.bank_cfg(2, 5, [0.22, -0.21, 0.1], occupied_fraction=200 / 512.0)
    want = resample.design(2, 5, 200 / 512.0)
    assert (c.struct_size, c.interpolation, c.decimation, c.ntaps, c.nlinks) == (
        ctypes.sizeof(_abi.ofdm_resamp_bank_cfg), 2, 5, len(want), 3)
    assert list(c.center_freq)[:3] == [0.22, -0.21, 0.1] and list(c.center_freq)[3:] == [0.0] * 5
    assert np.array_equal(np.ctypeslib.as_array(c.taps)[:len(want)], want)
    # the single resampler's configuration of the same link holds the same prototype
    one = resample.resamp_cfg(2, 5, 0.22, occupied_fraction=200 / 512.0)
    assert one.ntaps == c.ntaps and list(one.taps) == list(c.taps)
    c = resample.bank_cfg(3, 7, [0.5] * 8, taps=[1.0, 0.5], transition=None)
    assert c.nlinks == 8 and c.ntaps == 2 and c.taps[1] == 0.5 and c.center_freq[7] == 0.5
    assert resample.bank_cfg(64, 64, [-0.5], taps=np.ones(1024, np.float32)).ntaps == 1024
    for bad in (dict(center_freqs=[]), dict(center_freqs=[0.0] * 9), dict(center_freqs=[0.1], taps=[]),
                dict(center_freqs=[0.1], taps=np.zeros(1025, np.float32)), dict(center_freqs=[0.1, 0.5000001]),
                dict(center_freqs=[-0.51]), dict(center_freqs=[float("nan")])):
        kw = dict(taps=np.ones(3, np.float32))
        kw.update(bad)
        with pytest.raises(ValueError):
            resample.bank_cfg(2, 5, **kw)
    with pytest.raises(ValueError):
        resample.bank_cfg(2, 5, [0.1])                         # neither taps nor occupied_fraction
    for L, M in ((0, 5), (65, 5), (2, 0), (2, 65)):            # a ratio outside 1..64, with designed and with given taps
        with pytest.raises(ValueError):
            resample.bank_cfg(L, M, [0.1], occupied_fraction=0.4)
        with pytest.raises(ValueError):
            resample.bank_cfg(L, M, [0.1], taps=[1.0])
    with pytest.raises(ValueError):
        resample.bank_cfg(5, 2, [0.1], occupied_fraction=0.9)  # the link is wider than the capture


def test_bank_cfg_layout_matches_header(tmp_path):
    got = sh.check_cfg_layout_matches_header(        # five uint32, padded to the doubles
        tmp_path, _abi.ofdm_resamp_bank_cfg, 24 + 8 * 8 + 4 * 1024,
        macros=[("links", "OFDM_RESAMP_BANK_MAX_LINKS"), ("maxtaps", "OFDM_RESAMP_MAX_TAPS")])
    assert int(got["links"]) == _abi.OFDM_RESAMP_BANK_MAX_LINKS == resample.MAX_LINKS == bc.MAX_LINKS == 8
    assert int(got["maxtaps"]) == _abi.OFDM_RESAMP_MAX_TAPS == resample.MAX_TAPS


def test_header_declares_the_bank_and_the_library_exports_it():
    sh.check_header_declares_and_library_exports(BANK_FUNCS)
    # additions only: the single resampler's struct is what it was
    assert ctypes.sizeof(_abi.ofdm_resamp_cfg) == 24 + 4 * 1024


def test_entry_points_refuse_a_null_handle_without_a_gpu():
    lib = _abi.load()
    n, k, ms = ctypes.c_uint64(7), ctypes.c_int(7), ctypes.c_double(7.0)
    assert lib.ofdm_set_resamp_bank(None, None) == _abi.OFDM_E_INVAL
    assert lib.ofdm_set_resamp_bank(None, ctypes.byref(resample.bank_cfg(2, 5, [0.1], taps=[1.0]))) == _abi.OFDM_E_INVAL
    assert lib.ofdm_resamp_bank_reset(None, 0) == _abi.OFDM_E_INVAL
    assert lib.ofdm_resamp_bank_count(None, 10, ctypes.byref(n)) == _abi.OFDM_E_INVAL
    assert lib.ofdm_resamp_bank(None, None, 0, None, 0, 0, ctypes.byref(n)) == _abi.OFDM_E_INVAL
    assert lib.ofdm_resamp_bank_taps(None, 0, None, 0, ctypes.byref(k)) == _abi.OFDM_E_INVAL
    assert lib.ofdm_resamp_bank_last_ms(None, ctypes.byref(ms)) == _abi.OFDM_E_INVAL
    assert (n.value, k.value, ms.value) == (7, 7, 7.0)          # nothing was written


def test_grids_cover_what_they_claim():
    assert set(bc.TAP_GRID) == {(1, 1), (2, 5), (5, 2), (7, 1), (8, 25), (3, 25), (1, 64), (64, 1), (64, 63), (63, 64),
                                (64, 64)}
    assert {bc.chains(L, M) for L, M in bc.TAP_GRID} == {1, 4}
    assert bc.chains(1, 64) == 4 and bc.chains(3, 25) == 4 and bc.chains(64, 64) == 1 and bc.chains(1, 1) == 1
    for (L, M), taps in bc.TAP_GRID.items():
        n = bc.stream_length(L, M)
        tile = bc.tile_inputs(L, M, 8)
        assert tile == resamp_cases.tile_inputs(L, M)
        assert n <= 60000 + 64 and n % tile != 0 and (M == 1 or n % M != 0)
        assert len(taps) <= 3 and set(taps) <= {1, L - 1, 31, 155, 1024}
        assert (L, M) not in ((64, 64), (1, 64), (64, 1)) or 1024 in taps
        assert bc.far_start(M) % M != 0 or M == 1
    assert any(t < L for (L, M), taps in bc.TAP_GRID.items() for t in taps)      # phases without a tap
    f = bc.frequencies(np.random.default_rng(1), (0.0, 0.25, -0.3, 0.5))
    assert len(f) == 8 and f[7] == f[2] and 0.0 in f and 0.5 in f and all(abs(v) <= 0.5 for v in f)
    assert len(bc.pick(f, 3)) == 3 and bc.pick(f, 3)[0] == bc.pick(f, 3)[2]
    assert all(1 <= K <= 8 for _, _, _, K in bc.SEG_SHAPES)


@pytest.mark.parametrize("kw", [
    dict(center_freqs=[]), dict(center_freqs=[0.0] * 9), dict(center_freqs=[0.1, 0.6]), dict(center_freqs=[0.1], decimation=0),
    dict(center_freqs=[0.1], decimation=65), dict(center_freqs=[0.1], interpolation=0), dict(center_freqs=[0.1], interpolation=65),
    dict(center_freqs=[0.1], interpolation=0, taps=[1.0]), dict(center_freqs=[0.1], decimation=65, taps=[1.0]),
    dict(center_freqs=[0.1], interpolation=8, decimation=3),   # a 200 / 512 link is wider than a capture at 3 / 8 its rate
    dict(center_freqs=[0.1], taps=[]), dict(center_freqs=[0.1], iq_format="u8"),
    dict(center_freqs=[0.1], iq_scale=-1.0), dict(center_freqs=[0.1], callback=3), dict(center_freqs=[0.1, 0.2], options=3),
])
def test_demod_resamp_bank_checks_its_arguments_before_any_engine_exists(kw, monkeypatch):
    sh.check_arguments_are_checked_before_any_engine_exists(
        monkeypatch, ofdm.ofdm_demod_resamp_bank, ("options", "center_freqs", "interpolation", "decimation"),
        dict(center_freqs=[0.25], interpolation=2, decimation=5), kw)


@pytest.mark.parametrize("extra", [
    ["--ddc-decim", "4"], ["--ddc-freq", "0.1"], ["--ddc-decim", "4", "--ddc-freqs", "0.1,0.2"],
    ["--resamp-freq", "0.1"], ["--link-quality"], ["--csi-report", "csi.txt"], ["--suggest-map", "10"],
])
def test_command_line_refuses_what_the_bank_does_not_combine_with(extra, tmp_path, monkeypatch, capsys):
    base = ["-m", "qpsk", "--from-file", str(tmp_path / "none.dat"), "--to-file", str(tmp_path / "rx.txt"),
            "--resamp-interp", "2", "--resamp-decim", "5", "--resamp-freqs", "0.22,-0.21"]
    sh.check_command_line_refuses(monkeypatch, capsys, tmp_path, benchmark_ofdm_rx.main, base + extra, "--resamp-freqs")


def test_command_line_needs_a_ratio_and_numbers(tmp_path, capsys):
    base = ["-m", "qpsk", "--from-file", str(tmp_path / "none.dat"), "--to-file", str(tmp_path / "rx.txt")]
    for argv in (["--resamp-freqs", "0.1,0.2"], ["--resamp-interp", "2", "--resamp-decim", "5", "--resamp-freqs", "0.1,x"]):
        with pytest.raises(SystemExit) as e:
            benchmark_ofdm_rx.main(base + argv)
        assert e.value.code == 2 and "--resamp-freqs" in capsys.readouterr().err
    assert not list(tmp_path.iterdir())
