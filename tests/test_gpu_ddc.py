"""The wideband front end on the GPU (k_ddc, Engine.ddc, ofdm_demod(ddc=...)): against the float64 model of its
definition, under arbitrary segmentation of the stream, end to end on two-link wideband captures, and at its edges."""
import numpy as np
import pytest

import ddc_cases
import stage_harness as sh
from ofdm_uhd_amd import ddc, engine, ofdm, predictive_sense
from stage_harness import EPS, FCS, eng   # noqa: F401 (eng: one handle per file)

pytestmark = pytest.mark.gpu

STAGE = sh.STAGES["ddc"]
DECIMS = (1, 2, 3, 4, 8, 64)
_stream, _options, _wide_sc16 = sh.rx_stream, sh.options_of, sh.wide_sc16


def _tap_counts(R):
    return sorted({1, 2, 31, 155, 1024} | ({R - 1} if R - 1 >= 1 else set()))


def _set(eng, R, taps, fc):
    eng.set_ddc(ddc.ddc_cfg(R, fc, taps=taps))
    c = eng.ddc_taps()
    assert c.dtype == np.complex64 and len(c) == len(taps)
    return c


def _check_against_model(y, x, c, R, fc, first, what):
    sh.check_ddc_model(y, x, c, (R,), fc, first, what)


@pytest.mark.parametrize("fmt", ["fc32", "sc16"])
@pytest.mark.parametrize("R", DECIMS)
def test_against_float64_model(eng, R, fmt):
    rng = np.random.default_rng(1000 + R)
    tile = ddc_cases.tile_outputs(R) * R
    n = min(2 * tile + tile // 3 + 5, 60000)
    while (R > 1 and n % R == 0) or n % tile == 0:     # neither a multiple of R nor of the tile
        n += 1
    eng.set_rx_iq_format(fmt)
    try:
        raw, x = _stream(rng, n, fmt)
        for ntaps in _tap_counts(R):
            taps = (rng.standard_normal(ntaps) / np.sqrt(ntaps)).astype(np.float32)
            for fc in FCS:
                c = _set(eng, R, taps, fc)
                # the table is the float64 evaluation rounded once (to the last bit or the libm's one next to it)
                assert np.max(np.abs(c - ddc.bandpass_taps(taps, fc))) <= 2 * EPS * np.max(np.abs(taps))
                assert eng.ddc_count(n) == ddc_cases.count(0, n, R)
                y = eng.ddc(raw)
                _check_against_model(y, x, c, R, fc, 0, "R=%d ntaps=%d fc=%g %s" % (R, ntaps, fc, fmt))
            # a stream that starts at an absolute index that is no multiple of R (and far from 0: the phase is m D)
            first = 1000003 if 1000003 % R else 1000004
            assert first % R != 0 or R == 1
            c = _set(eng, R, taps, FCS[2])            # the generic frequency: m D mod 2^64 at m of 10^4 .. 10^6
            assert ddc_cases.phase_step(FCS[2], R) % (1 << 32) != 0
            eng.ddc_reset(first)
            assert eng.ddc_count(n) == ddc_cases.count(first, n, R)
            y = eng.ddc(raw)
            _check_against_model(y, x, c, R, FCS[2], first, "R=%d ntaps=%d reset to %d %s" % (R, ntaps, first, fmt))
    finally:
        eng.set_rx_iq_format("fc32")
        eng.set_ddc(None)


@pytest.mark.parametrize("fmt", ["fc32", "sc16"])
@pytest.mark.parametrize("R,ntaps", [(1, 31), (2, 1024), (3, 155), (4, 31), (4, 3), (8, 155), (8, 7), (64, 1024), (64, 63),
                                     (5, 2), (17, 1)])
def test_any_segmentation_gives_the_same_bits(eng, R, ntaps, fmt):
    n = 3 * ddc_cases.tile_outputs(R) * R + 1234 + 2 * ntaps
    sh.check_rx_segmentation(eng, STAGE, (R,), ntaps, None, fmt, seed=77 * R + ntaps, n=n)


@pytest.mark.parametrize("name,fmt", [("qpsk512_r4", "fc32"), ("qpsk512_r4", "sc16"), ("qam16_2048_r2", "fc32"),
                                      ("bpsk64_r8", "fc32"), ("qpsk512_r3", "fc32")])
def test_two_links_end_to_end(orc, name, fmt):
    cap = ddc_cases.capture(name)
    R, cfg = cap["R"], cap["cfg"]
    wide = _wide_sc16(cap["wide"]) if fmt == "sc16" else cap["wide"]
    e = engine.Engine(cfg=cfg)
    try:
        for fc, sent in zip(cap["freqs"], cap["payloads"]):
            e.set_rx_iq_format(fmt)
            e.set_ddc(ddc.ddc_cfg(R, fc, taps=cap["taps"]))
            y = e.ddc(wide)
            e.set_rx_iq_format("fc32")
            assert len(y) == ddc_cases.count(0, len(wide), R)
            got = e.rx(y)
            ref = orc.rx(cfg, y)
            assert got == ref.packets, (name, fc)                       # the parity bar, on the engine's DDC output
            assert [ok for ok, _ in got] == [True] * 4 and [p for _, p in got] == sent, (name, fc)
            # the same through ofdm_demod, one call and 5000-sample wideband chunks
            kw = dict(iq_format=fmt, ddc=dict(decimation=R, center_freq=fc, taps=cap["taps"]))
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
    cap = ddc_cases.capture("qpsk512_r3")
    kw = dict(ddc=dict(decimation=cap["R"], center_freq=cap["freqs"][1], taps=cap["taps"]))
    sh.check_a_stream_fed_after_work_starts_afresh(STAGE, (cap["R"],), cap, kw)


def test_receive_path_and_command_line_take_the_front_end(orc, tmp_path):
    cap = ddc_cases.capture("qpsk512_r4")

    def as_the_command_line(opt):                         # the options' ddc_decim / ddc_freq, as --ddc-decim / --ddc-freq set them
        opt.ddc_decim, opt.ddc_freq = 4, -0.25
    sh.check_receive_path_and_command_line(cap, tmp_path, dict(ddc=dict(decimation=4, center_freq=0.25, taps=cap["taps"])),
                                           as_the_command_line, ["--ddc-decim", "4", "--ddc-freq", "0.25"])


@pytest.mark.parametrize("fmt", ["fc32", "sc16"])
def test_sensor_behind_the_front_end(fmt):
    cap = ddc_cases.capture("qpsk512_r4")
    wide = _wide_sc16(cap["wide"]) if fmt == "sc16" else cap["wide"]
    e = engine.Engine(cfg=cap["cfg"])
    try:
        argv = ["--ddc-decim", "4", "--ddc-freq", "0.25", "-s", "256", "--tune-delay", "4e-5", "--dwell-delay", "1.2e-4",
                "--iq-format", fmt]
        s = predictive_sense.sensor(argv, engine=e, threshold=1e-6, avg_iterations=2)
        assert (s.tune_delay, s.dwell_delay) == (1, 3)
        # the engine came with a front end of its own: the sensor puts it back
        own = ddc.ddc_cfg(3, 0.1, taps=np.ones(4, np.float32))
        e.set_ddc(own)
        got = s.run(wide)
        assert e.ddc_cfg is own and e.rx_iq_format == fmt
        assert np.max(np.abs(e.ddc_taps() - ddc.bandpass_taps(np.ones(4, np.float32), 0.1))) <= 2 * EPS
        # by hand: tune and decimate, then sense the complex64 result
        e.set_ddc(decimation=4, center_freq=0.25, occupied_fraction=0.8)
        y = e.ddc(wide)
        e.set_ddc(None)
        e.set_rx_iq_format("fc32")
        want = e.sense(s.sense_cfg(), y)
        assert len(want["msgs"]) >= 6 and len(want["hex"]) >= 2
        assert np.array_equal(got["msgs"], want["msgs"]) and got["hex"] == want["hex"]
        # and it is not what the sensor sees without the front end
        plain = predictive_sense.sensor(argv[4:], engine=e, threshold=1e-6, avg_iterations=2).run(wide)
        assert plain["msgs"].shape != want["msgs"].shape
    finally:
        e.close()


def test_designed_taps_are_the_default(orc):
    cap = ddc_cases.capture("qpsk512_r4")
    d = ofdm.ofdm_demod(_options(cap), ddc=dict(decimation=4, center_freq=-0.25))
    try:
        c = d.engine().ddc_taps()
        assert len(c) == 31 and np.max(np.abs(c - ddc.bandpass_taps(ddc.design(4, 200 / 512.0), -0.25))) <= 2 * EPS
        got = d.work(cap["wide"])
        assert [p for ok, p in got if ok] == cap["payloads"][1]
    finally:
        d.engine().close()


def test_invalid_arguments_are_refused(eng):
    bads = (dict(struct_size=12), dict(decimation=0), dict(decimation=65), dict(ntaps=0), dict(ntaps=1025),
            dict(center_freq=0.5000001), dict(center_freq=-0.51), dict(center_freq=float("nan")))
    sh.check_rx_single_invalid_arguments(eng, STAGE, (4,), lambda: ddc.ddc_cfg(4, 0.25, taps=np.ones(5, np.float32)), bads,
                                         fed_sc16=0, count64=16)


def test_phase_step_and_index_limits(eng):
    """fc R a hair below a whole turn from the negative side: frac rounds up to 1 and the phase step is 0, not 2^64;
    stream indices are refused before 64-bit arithmetic could wrap."""
    sh.check_phase_step_zero_and_index_limit(eng, STAGE, -1e-20, link=())


def test_capacity_error_leaves_the_stream_state(eng):
    raw, _ = _stream(np.random.default_rng(5), 5000, "fc32")
    sh.check_capacity_error_leaves_the_stream_state(eng, STAGE, (3,), 0.2, ddc.design(3, 0.4), raw)


def test_without_a_ddc_the_receiver_launches_what_it_launched(orc):
    cap = ddc_cases.capture("qpsk512_r4")
    sh.check_receiver_launches_what_it_launched(STAGE, (4,), cap, 0.25)
