"""Host side of the resampler bank (resample.bank_cfg, the ofdm_resamp_bank_* part of the C ABI, the argument checks of
ofdm_demod_resamp_bank and of the command line): no GPU needed."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import resamp_bank_cases as bc
import resamp_cases
from ofdm_uhd_amd import _abi, benchmark_ofdm_rx, ofdm, options, resample

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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
    st = _abi.ofdm_resamp_bank_cfg
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ofdm_hip.h"', 'int main(void){',
             'printf("size %zu\\n", sizeof(ofdm_resamp_bank_cfg));', 'printf("links %d\\n", OFDM_RESAMP_BANK_MAX_LINKS);',
             'printf("maxtaps %d\\n", OFDM_RESAMP_MAX_TAPS);']
    for f, _ in st._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(ofdm_resamp_bank_cfg, %s));' % (f, f))
    lines.append('return 0;}')
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)])
    got = dict(l.split() for l in subprocess.check_output([exe]).decode().splitlines())
    assert int(got["size"]) == ctypes.sizeof(st) == 24 + 8 * 8 + 4 * 1024      # five uint32, padded to the doubles
    assert int(got["links"]) == _abi.OFDM_RESAMP_BANK_MAX_LINKS == resample.MAX_LINKS == bc.MAX_LINKS == 8
    assert int(got["maxtaps"]) == _abi.OFDM_RESAMP_MAX_TAPS == resample.MAX_TAPS
    for f, _ in st._fields_:
        assert int(got[f]) == getattr(st, f).offset, f


def test_header_declares_the_bank_and_the_library_exports_it():
    hdr = open(os.path.join(ROOT, "include", "ofdm_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(ofdm_[a-z_0-9]+)\s*\(", code))
    lib = _abi.load()
    for name in BANK_FUNCS:
        assert name in declared, name
        assert name in _abi.EXPORTS, name
        assert hasattr(lib, name), name
    # additions only: the version, the kernel table and the single resampler's struct are what they were
    assert re.search(r"#define\s+OFDM_ABI_VERSION\s+6\b", code) and lib.ofdm_abi_version() == 6
    assert _abi.K_COUNT == 11 and re.search(r"OFDM_K_COUNT\s*=\s*11\b", code)
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


def _opt():
    return options.default_options(modulation="qpsk")


@pytest.mark.parametrize("kw", [
    dict(center_freqs=[]), dict(center_freqs=[0.0] * 9), dict(center_freqs=[0.1, 0.6]), dict(center_freqs=[0.1], decimation=0),
    dict(center_freqs=[0.1], decimation=65), dict(center_freqs=[0.1], interpolation=0), dict(center_freqs=[0.1], interpolation=65),
    dict(center_freqs=[0.1], interpolation=0, taps=[1.0]), dict(center_freqs=[0.1], decimation=65, taps=[1.0]),
    dict(center_freqs=[0.1], interpolation=8, decimation=3),   # a 200 / 512 link is wider than a capture at 3 / 8 its rate
    dict(center_freqs=[0.1], taps=[]), dict(center_freqs=[0.1], iq_format="u8"),
    dict(center_freqs=[0.1], iq_scale=-1.0), dict(center_freqs=[0.1], callback=3), dict(center_freqs=[0.1, 0.2], options=3),
])
def test_demod_resamp_bank_checks_its_arguments_before_any_engine_exists(kw, monkeypatch):
    from ofdm_uhd_amd import engine

    def no_engine(*a, **k):
        raise AssertionError("an engine was created before the arguments were checked")
    monkeypatch.setattr(engine, "Engine", no_engine)
    args = dict(options=_opt(), center_freqs=[0.25], interpolation=2, decimation=5)
    args.update(kw)
    if args["options"] == 3:
        args["options"] = [_opt()] * 3            # three option sets for two links
    with pytest.raises(ValueError):
        ofdm.ofdm_demod_resamp_bank(args.pop("options"), args.pop("center_freqs"), args.pop("interpolation"),
                                    args.pop("decimation"), **args)


@pytest.mark.parametrize("extra", [
    ["--ddc-decim", "4"], ["--ddc-freq", "0.1"], ["--ddc-decim", "4", "--ddc-freqs", "0.1,0.2"],
    ["--resamp-freq", "0.1"], ["--link-quality"], ["--csi-report", "csi.txt"], ["--suggest-map", "10"],
])
def test_command_line_refuses_what_the_bank_does_not_combine_with(extra, tmp_path, monkeypatch, capsys):
    from ofdm_uhd_amd import engine

    def no_engine(*a, **k):
        raise AssertionError("an engine was created for a refused command line")
    monkeypatch.setattr(engine, "Engine", no_engine)
    base = ["-m", "qpsk", "--from-file", str(tmp_path / "none.dat"), "--to-file", str(tmp_path / "rx.txt"),
            "--resamp-interp", "2", "--resamp-decim", "5", "--resamp-freqs", "0.22,-0.21"]
    with pytest.raises(SystemExit) as e:
        benchmark_ofdm_rx.main(base + extra)
    assert e.value.code == 2 and "--resamp-freqs" in capsys.readouterr().err
    assert not list(tmp_path.iterdir())           # refused before a file was opened


def test_command_line_needs_a_ratio_and_numbers(tmp_path, capsys):
    base = ["-m", "qpsk", "--from-file", str(tmp_path / "none.dat"), "--to-file", str(tmp_path / "rx.txt")]
    for argv in (["--resamp-freqs", "0.1,0.2"], ["--resamp-interp", "2", "--resamp-decim", "5", "--resamp-freqs", "0.1,x"]):
        with pytest.raises(SystemExit) as e:
            benchmark_ofdm_rx.main(base + argv)
        assert e.value.code == 2 and "--resamp-freqs" in capsys.readouterr().err
    assert not list(tmp_path.iterdir())
