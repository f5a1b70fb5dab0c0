"""Host side of the transmit resampler bank (tx_resample.bank_cfg and bank_phase_steps, the ofdm_tx_resamp_bank_* part
of the C ABI, the float64 model, its bound and the float32 emulation, the argument checks of ofdm_mod_resamp_bank and
of the command line): no GPU needed."""
import ctypes

import numpy as np
import pytest

import stage_harness as sh
import tx_resamp_bank_cases as bc
import tx_resamp_cases
from ofdm_uhd_amd import _abi, benchmark_ofdm_tx, ofdm, tx_resample

BANK_FUNCS = ("ofdm_set_tx_resamp_bank", "ofdm_tx_resamp_bank_reset", "ofdm_tx_resamp_bank_count", "ofdm_tx_resamp_bank",
              "ofdm_tx_resamp_bank_taps", "ofdm_tx_resamp_bank_last_ms")


def test_bank_cfg_builder():
    c = tx_resample.bank_cfg(5, 2, [0.22, -0.21, 0.1], occupied_fraction=200 / 512.0)
    want = tx_resample.design(5, 2, 200 / 512.0)
    assert (c.struct_size, c.interpolation, c.decimation, c.ntaps, c.nlinks, c.out_format, c.out_scale) == (
        ctypes.sizeof(_abi.ofdm_tx_resamp_bank_cfg), 5, 2, len(want), 3, _abi.OFDM_IQ_FC32, 0.0)
    assert list(c.center_freq)[:3] == [0.22, -0.21, 0.1] and list(c.center_freq)[3:] == [0.0] * 5
    assert np.array_equal(np.ctypeslib.as_array(c.taps)[:len(want)], want)
    # the single stage's configuration of the same link holds the same prototype
    one = tx_resample.tx_resamp_cfg(5, 2, 0.22, occupied_fraction=200 / 512.0)
    assert one.ntaps == c.ntaps and list(one.taps) == list(c.taps)
    c = tx_resample.bank_cfg(3, 7, [0.5] * 8, taps=[1.0, 0.5], out_format="sc16", out_scale=1000.0)
    assert c.nlinks == 8 and c.ntaps == 2 and c.taps[1] == 0.5 and c.center_freq[7] == 0.5
    assert c.out_format == _abi.OFDM_IQ_SC16 and c.out_scale == 1000.0
    assert tx_resample.bank_cfg(64, 64, [-0.5], taps=np.ones(1024, np.float32)).ntaps == 1024
    for bad in (dict(center_freqs=[]), dict(center_freqs=[0.0] * 9), dict(center_freqs=[0.1], taps=[]),
                dict(center_freqs=[0.1], taps=np.zeros(1025, np.float32)), dict(center_freqs=[0.1, 0.5000001]),
                dict(center_freqs=[-0.51]), dict(center_freqs=[float("nan")]),
                dict(center_freqs=[0.1], taps=[1.0, float("inf")]), dict(center_freqs=[0.1], taps=[float("nan")]),
                dict(center_freqs=[0.1], out_format="u8"), dict(center_freqs=[0.1], out_format="sc16", out_scale=0.0),
                dict(center_freqs=[0.1], out_format="sc16", out_scale=-2.0),
                dict(center_freqs=[0.1], out_format="sc16", out_scale=float("inf"))):
        kw = dict(taps=np.ones(3, np.float32))
        kw.update(bad)
        with pytest.raises(ValueError):
            tx_resample.bank_cfg(5, 2, **kw)
    with pytest.raises(ValueError):
        tx_resample.bank_cfg(5, 2, [0.1])                         # neither taps nor occupied_fraction
    for L, M in ((0, 5), (65, 5), (2, 0), (2, 65)):               # a ratio outside 1..64, with designed and with given taps
        with pytest.raises(ValueError):
            tx_resample.bank_cfg(L, M, [0.1], occupied_fraction=0.4)
        with pytest.raises(ValueError):
            tx_resample.bank_cfg(L, M, [0.1], taps=[1.0])
    with pytest.raises(ValueError):
        tx_resample.bank_cfg(2, 5, [0.1], occupied_fraction=0.9)  # the link is wider than the band


def test_bank_cfg_layout_matches_header(tmp_path):
    got = sh.check_cfg_layout_matches_header(        # seven 32-bit fields, padded to the doubles
        tmp_path, _abi.ofdm_tx_resamp_bank_cfg, 32 + 8 * 8 + 4 * 1024,
        macros=[("links", "OFDM_TX_RESAMP_BANK_MAX_LINKS"), ("maxtaps", "OFDM_TX_RESAMP_MAX_TAPS")])
    assert int(got["links"]) == _abi.OFDM_TX_RESAMP_BANK_MAX_LINKS == tx_resample.MAX_LINKS == bc.MAX_LINKS == 8
    assert int(got["maxtaps"]) == _abi.OFDM_TX_RESAMP_MAX_TAPS == tx_resample.MAX_TAPS


def test_header_declares_the_bank_and_the_library_exports_it():
    sh.check_header_declares_and_library_exports(BANK_FUNCS)
    # additions only: the single stage's struct is what it was
    assert ctypes.sizeof(_abi.ofdm_tx_resamp_cfg) == 40 + 4 * 1024


def test_entry_points_refuse_a_null_handle_without_a_gpu():
    lib = _abi.load()
    n, k, ms = ctypes.c_uint64(7), ctypes.c_int(7), ctypes.c_double(7.0)
    assert lib.ofdm_set_tx_resamp_bank(None, None) == _abi.OFDM_E_INVAL
    assert lib.ofdm_set_tx_resamp_bank(None, ctypes.byref(tx_resample.bank_cfg(5, 2, [0.1], taps=[1.0]))) == _abi.OFDM_E_INVAL
    assert lib.ofdm_tx_resamp_bank_reset(None, 0) == _abi.OFDM_E_INVAL
    assert lib.ofdm_tx_resamp_bank_count(None, 10, ctypes.byref(n)) == _abi.OFDM_E_INVAL
    assert lib.ofdm_tx_resamp_bank(None, None, 0, 0, None, None, 0, ctypes.byref(n)) == _abi.OFDM_E_INVAL
    assert lib.ofdm_tx_resamp_bank_taps(None, 0, None, 0, ctypes.byref(k)) == _abi.OFDM_E_INVAL
    assert lib.ofdm_tx_resamp_bank_last_ms(None, ctypes.byref(ms)) == _abi.OFDM_E_INVAL
    assert (n.value, k.value, ms.value) == (7, 7, 7.0)          # nothing was written


def test_phase_steps_restate_the_definition():
    for fc, L, M in ((0.22, 5, 2), (-0.21, 5, 2), (0.3, 25, 8), (-0.17, 25, 8), (0.5, 64, 63), (-0.5, 1, 64), (0.0, 3, 4)):
        G, E, D = tx_resample.bank_phase_steps(fc, L, M)
        assert G == tx_resamp_cases.phase_step(fc / M)           # ONE double division, then the DDC's convention
        assert E == (L * G) % 2 ** 64 and D == (M * G) % 2 ** 64
        # the effective frequency D / 2^64 is fc modulo 1, to about M 2^-54
        d = (D / 2.0 ** 64 - fc) % 1.0
        assert min(d, 1.0 - d) <= M * 2.0 ** -53
    # a dyadic fc and a power of two M: D is the single stage's phase step, exactly
    for fc, M in ((0.25, 4), (-0.375, 1), (-0.125, 2), (0.5, 8)):
        assert tx_resample.bank_phase_steps(fc, 3, M)[2] == tx_resample.phase_step(fc)
    for L, M in ((0, 1), (1, 0), (65, 1), (1, 65)):
        with pytest.raises(ValueError):
            tx_resample.bank_phase_steps(0.1, L, M)


def test_input_side_shift_is_exact_on_random_indices():
    """k G + m E = n D modulo 2^64 wherever n M = k + m L: table angle plus input rotation is the rotation by n D."""
    rng = np.random.default_rng(20)
    for _ in range(2000):
        L, M = int(rng.integers(1, 65)), int(rng.integers(1, 65))
        fc = float(rng.uniform(-0.5, 0.5))
        G, E, D = tx_resample.bank_phase_steps(fc, L, M)
        m_new = int(rng.integers(0, 2 ** 56 + 1))                 # the newest input of an output, up to the index limit
        n = -(-m_new * L // M)                                    # the first output whose newest input is m_new or later
        i, p = n * M // L, n * M % L
        q = int(rng.integers(0, 1024 // L + 1))
        k, m = p + q * L, i - q
        assert n * M == k + m * L
        assert (k * G + m * E) % 2 ** 64 == (n * D) % 2 ** 64


def test_model_at_one_link_is_the_single_stage_model():
    rng = np.random.default_rng(21)
    for L, M, ntaps, fc, first in ((5, 2, 39, 0.22, 0), (3, 4, 50, -0.21, 1000003), (7, 64, 200, 0.5, 2 ** 40 - 5)):
        x = (rng.standard_normal(700) + 1j * rng.standard_normal(700)).astype(np.complex64)
        h = bc.taps_for(rng, ntaps)
        D = tx_resample.bank_phase_steps(fc, L, M)[2]
        y1, s1 = tx_resamp_cases.model(x, h, L, M, D, first)
        y, s = bc.model(x, h, L, M, [fc], first)
        assert np.array_equal(y, y1) and np.array_equal(s, s1)
        # and K links are the sum of K such models
        y2, s2 = bc.model(np.stack([x, x[::-1]]), h, L, M, [fc, -fc], first)
        yb, sb = tx_resamp_cases.model(x[::-1], h, L, M, tx_resample.bank_phase_steps(-fc, L, M)[2], first)
        assert np.array_equal(y2, y1 + yb) and np.array_equal(s2, s1 + sb)


@pytest.mark.parametrize("K,L,M,ntaps", bc.HOST_SHAPES)
def test_emulation_of_the_definition_stays_within_the_bound(K, L, M, ntaps):
    """The definition in float32 against the float64 model: negative frequencies and first != 0 included (G must be
    turns(fc / M): turns(fc) / M disagrees with the table by e^{j 2 pi k / M} for a negative fc)."""
    rng = np.random.default_rng(1000 * K + 10 * L + M)
    h = bc.taps_for(rng, ntaps)
    fcs = bc.freqs(K)
    assert K < 2 or any(f < 0 for f in fcs)
    nin = min(bc.stream_inputs(L, M), 3000)
    worst = 0.0
    for first in bc.FIRSTS:
        x = (rng.standard_normal((K, nin)) + 1j * rng.standard_normal((K, nin))).astype(np.complex64)
        y64, s = bc.model(x, h, L, M, fcs, first)
        assert len(y64) == tx_resample.count(first, nin, L, M) > 0
        add = (rng.standard_normal(len(y64)) + 1j * rng.standard_normal(len(y64))).astype(np.complex64)
        for a in (None, add):
            got = bc.emulate(x, h, L, M, fcs, first, add=a)
            want = y64 if a is None else y64 + a.astype(np.complex128)
            b = bc.bound(K, ntaps, L, s, a)
            err = np.abs(got.astype(np.complex128) - want)
            assert np.all(err <= b), (first, float(np.max(err / np.maximum(b, 1e-300))))
            worst = max(worst, float(np.max(err[b > 0] / b[b > 0])) if np.any(b > 0) else 0.0)
    print("K=%d %d/%d ntaps=%d: worst error / bound %.3f" % (K, L, M, ntaps, worst))


def test_emulation_with_a_negative_frequency_needs_the_one_division():
    """The trap in the definition: with G' = turns(fc) / M the phases of a negative fc leave the table's by k / M turn."""
    L, M, fc = 5, 2, -0.21
    G = tx_resample.bank_phase_steps(fc, L, M)[0]
    Gp = tx_resample.phase_step(fc) // M
    k = 1                                                   # tap 1: the table's angle is fc k / M
    want = (fc * k / M) % 1.0
    assert abs(G * k / 2.0 ** 64 - want) < 1e-12
    assert abs(Gp * k / 2.0 ** 64 - want) > 0.1


@pytest.mark.parametrize("kw", [
    dict(center_freqs=[]), dict(center_freqs=[0.0] * 9), dict(center_freqs=[0.1, 0.6]), dict(center_freqs=[0.1], decimation=0),
    dict(center_freqs=[0.1], decimation=65), dict(center_freqs=[0.1], interpolation=0), dict(center_freqs=[0.1], interpolation=65),
    dict(center_freqs=[0.1], interpolation=0, taps=[1.0]), dict(center_freqs=[0.1], decimation=65, taps=[1.0]),
    dict(center_freqs=[0.1], interpolation=3, decimation=8),   # a 200 / 512 link is wider than a band at 3 / 8 its rate
    dict(center_freqs=[0.1], taps=[]), dict(center_freqs=[0.1], taps=[float("nan")]), dict(center_freqs=[0.1], iq_format="u8"),
    dict(center_freqs=[0.1], iq_format="sc16", iq_scale=-1.0), dict(center_freqs=[0.1, 0.2], options=3),
])
def test_mod_resamp_bank_checks_its_arguments_before_any_engine_exists(kw, monkeypatch):
    sh.check_arguments_are_checked_before_any_engine_exists(
        monkeypatch, ofdm.ofdm_mod_resamp_bank, ("options", "center_freqs", "interpolation", "decimation"),
        dict(center_freqs=[0.25], interpolation=5, decimation=2), kw)


def test_mod_resamp_bank_is_a_links_modulator():
    assert issubclass(ofdm.ofdm_mod_resamp_bank, ofdm._ofdm_mod_links)
    assert ofdm.ofdm_mod_resamp_bank._stage == "tx_resamp_bank"
    cfg = tx_resample.bank_cfg(5, 2, [0.1], taps=np.ones(39, np.float32))
    assert ofdm.ofdm_mod_resamp_bank._history(None, cfg) == 7 == tx_resample.history(39, 5)


@pytest.mark.parametrize("extra", [
    ["--duc-interp", "4"], ["--duc-freq", "0.1"], ["--tx-resamp-freq", "0.1"],
])
def test_command_line_refuses_what_the_bank_does_not_combine_with(extra, tmp_path, monkeypatch, capsys):
    base = ["-m", "qpsk", "--to-file", str(tmp_path / "tx.dat"), "--tx-resamp-interp", "5", "--tx-resamp-decim", "2",
            "--tx-resamp-freqs", "0.22,-0.21"]
    sh.check_command_line_refuses(monkeypatch, capsys, tmp_path, benchmark_ofdm_tx.main, base + extra, "--tx-resamp-freqs")


def test_command_line_needs_a_ratio_numbers_and_a_band_wide_enough(tmp_path, monkeypatch, capsys):
    base = ["-m", "qpsk", "--to-file", str(tmp_path / "tx.dat")]
    for argv in (["--tx-resamp-freqs", "0.1,0.2"], ["--tx-resamp-interp", "5", "--tx-resamp-decim", "2", "--tx-resamp-freqs", "0.1,x"],
                 ["--tx-resamp-interp", "5", "--tx-resamp-decim", "2", "--tx-resamp-freqs", "0.1,0.7"],
                 ["--tx-resamp-interp", "3", "--tx-resamp-decim", "8", "--tx-resamp-freqs", "0.1"]):
        sh.check_command_line_refuses(monkeypatch, capsys, tmp_path, benchmark_ofdm_tx.main, base + argv, "--tx-resamp-freqs")
