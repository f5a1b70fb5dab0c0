"""The rational-rate front end on the GPU (k_resamp, Engine.resamp, ofdm_demod(resample=...)): against the float64
model of its definition, under arbitrary segmentation of the stream, end to end on wideband captures whose rate is no
integer multiple of the modem's, and at its edges."""
import numpy as np
import pytest

import resamp_cases
import stage_harness as sh
from ofdm_uhd_amd import engine, ofdm, predictive_sense, resample
from stage_harness import EPS, FCS, eng   # noqa: F401 (eng: one handle per file)

pytestmark = pytest.mark.gpu

STAGE = sh.STAGES["resamp"]
RATIOS = ((1, 1), (1, 3), (2, 5), (3, 2), (4, 3), (5, 2), (7, 1), (8, 25), (64, 63), (63, 64), (1, 64), (64, 1))
_stream, _options, _wide_sc16 = sh.rx_stream, sh.options_of, sh.wide_sc16


def _tap_counts(L):
    return sorted({1, 2, 31, 155, 1024} | ({L - 1} if L - 1 >= 1 else set()))


def _set(eng, L, M, taps, fc):
    eng.set_resamp(resample.resamp_cfg(L, M, fc, taps=taps))
    c = eng.resamp_taps()
    assert c.dtype == np.complex64 and len(c) == len(taps)
    return c


def _check_against_model(y, x, c, L, M, fc, first, what):
    sh.check_resamp_model(y, x, c, (L, M), fc, first, what)


@pytest.mark.parametrize("fmt", ["fc32", "sc16"])
@pytest.mark.parametrize("L,M", RATIOS)
def test_against_float64_model(eng, L, M, fmt):
    rng = np.random.default_rng(1000 + 64 * L + M)
    tile = resamp_cases.tile_inputs(L, M)
    n = min(2 * tile + tile // 3 + 5, 60000)
    while (M > 1 and n % M == 0) or n % tile == 0:     # neither a multiple of M nor of the tile
        n += 1
    eng.set_rx_iq_format(fmt)
    try:
        raw, x = _stream(rng, n, fmt)
        for ntaps in _tap_counts(L):
            taps = (rng.standard_normal(ntaps) / np.sqrt(ntaps)).astype(np.float32)
            for fc in FCS:
                c = _set(eng, L, M, taps, fc)
                # the table is the float64 evaluation rounded once (to the last bit or the libm's one next to it)
                assert np.max(np.abs(c - resample.bandpass_taps(taps, fc, L))) <= 2 * EPS * np.max(np.abs(taps))
                assert eng.resamp_count(n) == resamp_cases.count(0, n, L, M)
                y = eng.resamp(raw)
                _check_against_model(y, x, c, L, M, fc, 0, "L/M=%d/%d ntaps=%d fc=%g %s" % (L, M, ntaps, fc, fmt))
            # a stream that starts far from 0, at an index that is no multiple of M (the phase is n D)
            first = 1000003 if 1000003 % M else 1000004
            assert first % M != 0 or M == 1
            c = _set(eng, L, M, taps, FCS[2])
            eng.resamp_reset(first)
            assert eng.resamp_count(n) == resamp_cases.count(first, n, L, M)
            y = eng.resamp(raw)
            _check_against_model(y, x, c, L, M, FCS[2], first, "L/M=%d/%d ntaps=%d reset to %d %s" % (L, M, ntaps, first, fmt))
    finally:
        eng.set_rx_iq_format("fc32")
        eng.set_resamp(None)


@pytest.mark.parametrize("fmt", ["fc32", "sc16"])
@pytest.mark.parametrize("L,M,ntaps", [(2, 5, 39), (4, 3, 23), (8, 25, 481), (64, 63, 1024), (1, 64, 63), (64, 1, 1024),
                                       (3, 2, 2), (5, 7, 1)])
def test_any_segmentation_gives_the_same_bits(eng, L, M, ntaps, fmt):
    n = 3 * resamp_cases.tile_inputs(L, M) + 1234 + 2 * ((ntaps - 1) // L)
    sh.check_rx_segmentation(eng, STAGE, (L, M), ntaps, None, fmt, seed=77 * L + 5 * M + ntaps, n=n)


@pytest.mark.parametrize("name,fmt", [("qpsk512_2_5", "fc32"), ("qpsk512_2_5", "sc16"), ("qam16_512_4_3", "fc32"),
                                      ("bpsk64_8_25", "fc32")])
def test_links_end_to_end(orc, name, fmt):
    cap = resamp_cases.capture(name)
    L, M, cfg = cap["L"], cap["M"], cap["cfg"]
    wide = _wide_sc16(cap["wide"]) if fmt == "sc16" else cap["wide"]
    e = engine.Engine(cfg=cfg)
    try:
        for fc, sent in zip(cap["freqs"], cap["payloads"]):
            e.set_rx_iq_format(fmt)
            e.set_resamp(resample.resamp_cfg(L, M, fc, taps=cap["taps"]))
            y = e.resamp(wide)
            e.set_rx_iq_format("fc32")
            assert len(y) == resamp_cases.count(0, len(wide), L, M)
            got = e.rx(y)
            ref = orc.rx(cfg, y)
            assert got == ref.packets, (name, fc)                       # the parity bar, on the engine's own output
            assert [ok for ok, _ in got] == [True] * 4 and [p for _, p in got] == sent, (name, fc)
            # the same through ofdm_demod, one call and 5000-sample wideband chunks
            kw = dict(iq_format=fmt, resample=dict(interpolation=L, decimation=M, center_freq=fc, taps=cap["taps"]))
            d = ofdm.ofdm_demod(_options(cap), **kw)
            try:
                assert d.work(wide) == got, (name, fc)
                chunks = []
                for a in range(0, len(wide), 5000):
                    chunks += d.feed(wide[a:a + 5000])
                chunks += d.flush()
                assert chunks == got, (name, fc)
            finally:
                d.engine().close()
    finally:
        e.close()


def test_a_stream_fed_after_work_starts_afresh(orc):
    cap = resamp_cases.capture("qpsk512_2_5")
    L, M = cap["L"], cap["M"]
    kw = dict(resample=dict(interpolation=L, decimation=M, center_freq=cap["freqs"][1], taps=cap["taps"]))
    sh.check_a_stream_fed_after_work_starts_afresh(STAGE, (L, M), cap, kw)


def test_receive_path_and_command_line_take_the_front_end(orc, tmp_path):
    cap = resamp_cases.capture("qpsk512_2_5")

    def as_the_command_line(opt):      # the options' resamp_interp / resamp_decim / resamp_freq, as --resamp-* set them
        opt.resamp_interp, opt.resamp_decim, opt.resamp_freq = 2, 5, -0.21

    def taps_are_the_designed_ones(e):
        c = e.resamp_taps()
        assert np.max(np.abs(c - resample.bandpass_taps(resample.design(2, 5, 200 / 512.0), -0.21, 2))) <= 2 * EPS * 2
    sh.check_receive_path_and_command_line(
        cap, tmp_path, dict(resample=dict(interpolation=2, decimation=5, center_freq=0.22, taps=cap["taps"])),
        as_the_command_line, ["--resamp-interp", "2", "--resamp-decim", "5", "--resamp-freq", "0.22"],
        check_designed=taps_are_the_designed_ones)


def test_sensor_behind_the_front_end():
    cap = resamp_cases.capture("qpsk512_2_5")
    wide = cap["wide"]
    e = engine.Engine(cfg=cap["cfg"])
    try:
        argv = ["--resamp-interp", "2", "--resamp-decim", "5", "--resamp-freq", "0.22", "-s", "256", "--tune-delay", "4e-5",
                "--dwell-delay", "1.2e-4"]
        s = predictive_sense.sensor(argv, engine=e, threshold=1e-6, avg_iterations=2)
        # the engine came with a resampler of its own: the sensor puts it back
        own = resample.resamp_cfg(3, 2, 0.1, taps=np.ones(4, np.float32))
        e.set_resamp(own)
        got = s.run(wide)
        assert e.resamp_cfg is own and len(e.resamp_taps()) == 4
        # by hand: tune and resample, then sense the complex64 result
        e.set_resamp(interpolation=2, decimation=5, center_freq=0.22, occupied_fraction=0.8)
        y = e.resamp(wide)
        e.set_resamp(None)
        want = e.sense(s.sense_cfg(), y)
        assert len(want["msgs"]) >= 6 and len(want["hex"]) >= 2
        assert np.array_equal(got["msgs"], want["msgs"]) and got["hex"] == want["hex"]
        # and it is not what the sensor sees without the front end
        plain = predictive_sense.sensor(argv[6:], engine=e, threshold=1e-6, avg_iterations=2).run(wide)
        assert plain["msgs"].shape != want["msgs"].shape
    finally:
        e.close()


def test_invalid_arguments_are_refused(eng):
    bads = (dict(struct_size=12), dict(interpolation=0), dict(interpolation=65), dict(decimation=0), dict(decimation=65),
            dict(ntaps=0), dict(ntaps=1025), dict(center_freq=0.5000001), dict(center_freq=-0.51),
            dict(center_freq=float("nan")))
    base = lambda: resample.resamp_cfg(2, 5, 0.25, taps=np.ones(5, np.float32))
    sh.check_rx_single_invalid_arguments(eng, STAGE, (2, 5), base, bads, fed_sc16=3,
                                         count64=resamp_cases.count(3, 64, 2, 5))


def test_phase_step_and_index_limits(eng):
    """fc M / L a hair below a whole turn from the negative side: frac rounds up to 1 and the phase step is 0, not
    2^64; stream indices are refused before 64-bit arithmetic could wrap."""
    rng = np.random.default_rng(9)
    raw, x = _stream(rng, 700, "fc32")
    taps = (rng.standard_normal(9) / 3).astype(np.float32)
    try:
        c = _set(eng, 1, 4, taps, -1e-20)
        assert resamp_cases.phase_step(-1e-20, 1, 4) == 0
        eng.resamp_reset(1000003)
        _check_against_model(eng.resamp(raw), x, c, 1, 4, -1e-20, 1000003, "fc=-1e-20")
        c = _set(eng, 3, 4, taps, 0.2)
        lim = 1 << 56
        eng.resamp_reset(lim - 8)                    # a call may end on the limit itself
        assert eng.resamp_count(8) == resamp_cases.count(lim - 8, 8, 3, 4) == 6
        y = eng.resamp(raw[:8])
        _check_against_model(y, x[:8], c, 3, 4, 0.2, lim - 8, "at 2^56")
        with pytest.raises(ValueError):
            eng.resamp(raw[:1])                      # ... and none may pass it
        eng.resamp_reset(lim)                        # the limit is accepted as a reset value
        assert eng.resamp_count(0) == 0
        eng.resamp_reset(5)
        with pytest.raises(ValueError):
            eng.resamp_reset(lim + 1)
        assert eng.resamp_count(8) == resamp_cases.count(5, 8, 3, 4)   # the refused reset left the stream where it was
    finally:
        eng.set_resamp(None)


def test_capacity_error_leaves_the_stream_state(eng):
    raw, _ = _stream(np.random.default_rng(5), 5000, "fc32")
    sh.check_capacity_error_leaves_the_stream_state(eng, STAGE, (3, 4), 0.2, resample.design(3, 4, 0.4), raw)


def test_the_three_front_ends_keep_their_own_state(eng):
    """A handle may hold the DDC, the bank and the resampler: a call of one moves no other's stream."""
    from ofdm_uhd_amd import ddc
    rng = np.random.default_rng(6)
    raw, _ = _stream(rng, 3000, "fc32")
    taps = resample.design(2, 5, 0.4)
    try:
        eng.set_resamp(resample.resamp_cfg(2, 5, 0.1, taps=taps))
        want = eng.resamp(raw).copy()
        eng.resamp_reset(0)
        a = eng.resamp(raw[:1111])
        eng.set_ddc(ddc.ddc_cfg(3, 0.2, taps=ddc.design(3, 0.4)))
        eng.set_ddc_bank(ddc.bank_cfg(4, [0.1, -0.2], taps=ddc.design(4, 0.4)))
        eng.ddc(raw[:500])
        eng.ddc_bank(raw[:700])
        b = eng.resamp(raw[1111:])
        assert np.array_equal(np.concatenate([a, b]), want)
        assert eng.ddc_count(4) == ddc_count(500, 4, 3) and eng.ddc_bank_count(4) == ddc_count(700, 4, 4)
    finally:
        eng.set_ddc(None)
        eng.set_ddc_bank(None)
        eng.set_resamp(None)


def ddc_count(first, n, R):
    return -(-(first + n) // R) - -(-first // R)


def test_without_a_resampler_the_receiver_launches_what_it_launched(orc):
    cap = resamp_cases.capture("qpsk512_2_5")
    sh.check_receiver_launches_what_it_launched(STAGE, (2, 5), cap, cap["freqs"][0])
