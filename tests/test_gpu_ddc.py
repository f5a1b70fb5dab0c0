"""The wideband front end on the GPU (k_ddc, Engine.ddc, ofdm_demod(ddc=...)): against the float64 model of its
definition, under arbitrary segmentation of the stream, end to end on two-link wideband captures, and at its edges."""
import ctypes as C

import numpy as np
import pytest

import ddc_cases
from helpers import make_cfg
from ofdm_uhd_amd import _abi, benchmark_ofdm_rx, ddc, engine, iqio, ofdm, options, predictive_sense, receive_path

pytestmark = pytest.mark.gpu

FCS = (0.0, 0.25, -1.0 / 3.0 + 0.013, 0.5)
DECIMS = (1, 2, 3, 4, 8, 64)
EPS = 2.0 ** -24


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(cfg=make_cfg())
    yield e
    e.close()


def _tap_counts(R):
    return sorted({1, 2, 31, 155, 1024} | ({R - 1} if R - 1 >= 1 else set()))


def _stream(rng, n, fmt):
    """(samples in the receive format, the same samples converted to complex64)"""
    if fmt == "sc16":
        q = rng.integers(-32768, 32768, (n, 2)).astype(np.int16)
        return q, iqio.from_sc16(q)
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    return x, x


def _set(eng, R, taps, fc):
    eng.set_ddc(ddc.ddc_cfg(R, fc, taps=taps))
    c = eng.ddc_taps()
    assert c.dtype == np.complex64 and len(c) == len(taps)
    return c


def _check_against_model(y, x, c, R, fc, first, what):
    """The derived bound: |y - y64| <= (ntaps + 16) 2^-24 sum_k |c[k]| |x[mR - k]| per output -- a float32 sum of
    ntaps products in any order, 16 more roundings for the complex products and the rotation."""
    y64, s = ddc_cases.model(x, c, R, ddc_cases.phase_step(fc, R), first)
    assert len(y) == len(y64) == ddc_cases.count(first, len(x), R), what
    err = np.abs(y.astype(np.complex128) - y64)
    bound = (len(c) + 16) * EPS * s
    worst = float(np.max(err / np.maximum(bound, 1e-300))) if len(y) else 0.0
    print("%s: %d outputs, worst error / bound = %.3g" % (what, len(y), worst))
    assert np.all(err <= bound), what


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


def _chunk_sizes(rng, n, R, ntaps):
    tile = ddc_cases.tile_outputs(R) * R
    sizes = [s for s in (1, R - 1, R, ntaps - 2, ntaps, 997, tile - 1, tile + 1) if s >= 1]
    out, left = [], n
    seq = list(sizes)                       # every size once, then random draws (small ones weighted down)
    while left > 0:
        s = seq.pop(0) if seq else int(rng.choice(sizes, p=np.array([1.0 if v < 16 else 4.0 for v in sizes]) /
                                                  sum(1.0 if v < 16 else 4.0 for v in sizes)))
        s = min(s, left)
        out.append(s)
        left -= s
    return out


@pytest.mark.parametrize("fmt", ["fc32", "sc16"])
@pytest.mark.parametrize("R,ntaps", [(1, 31), (2, 1024), (3, 155), (4, 31), (4, 3), (8, 155), (8, 7), (64, 1024), (64, 63),
                                     (5, 2), (17, 1)])
def test_any_segmentation_gives_the_same_bits(eng, R, ntaps, fmt):
    rng = np.random.default_rng(77 * R + ntaps)
    tile = ddc_cases.tile_outputs(R) * R
    n = 3 * tile + 1234 + 2 * ntaps
    eng.set_rx_iq_format(fmt)
    try:
        raw, x = _stream(rng, n, fmt)
        taps = (rng.standard_normal(ntaps) / np.sqrt(ntaps)).astype(np.float32)
        fc = -1.0 / 3.0 + 0.013
        c = _set(eng, R, taps, fc)
        whole = eng.ddc(raw).copy()
        _check_against_model(whole, x, c, R, fc, 0, "whole R=%d ntaps=%d %s" % (R, ntaps, fmt))
        eng.ddc_reset(0)
        sizes = _chunk_sizes(rng, n, R, ntaps)
        assert any(s < ntaps - 1 for s in sizes) or ntaps <= 2
        parts, a, empty = [], 0, 0
        for s in sizes:
            want = ddc_cases.count(a, s, R)
            assert eng.ddc_count(s) == want
            y = eng.ddc(raw[a:a + s])
            assert len(y) == want
            empty += want == 0
            parts.append(y)
            a += s
        assert empty >= 1 or R == 1         # calls that produce nothing are part of the stream
        assert np.array_equal(np.concatenate(parts), whole)
        # ... and from a start that is no multiple of R
        first = 7 * R + 1
        eng.ddc_reset(first)
        w2 = eng.ddc(raw).copy()
        eng.ddc_reset(first)
        p2 = [eng.ddc(raw[i:i + 997]) for i in range(0, n, 997)]
        assert np.array_equal(np.concatenate(p2), w2)
    finally:
        eng.set_rx_iq_format("fc32")
        eng.set_ddc(None)


def _options(cap):
    return options.default_options(modulation=cap["mod"], fft_length=cap["N"], occupied_tones=cap["occ"], cp_length=cap["CP"])


def _wide_sc16(wide):
    """The capture as 16-bit IQ with its peak at half scale; nothing may saturate."""
    peak = float(max(np.max(np.abs(wide.real)), np.max(np.abs(wide.imag))))
    q = iqio.to_sc16(wide * np.float32(0.5 / peak))
    assert int(np.max(np.abs(q.astype(np.int32)))) < 32767, "a sample saturated"
    return q


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


def _record_ddc(d):
    """Keeps what the demodulator's front end hands to the receiver."""
    e, rec = d.engine(), []
    orig = e.ddc

    def ddc_and_keep(iq):
        y = orig(iq)
        rec.append(y.copy())
        return y
    e.ddc = ddc_and_keep
    return rec


def test_a_stream_fed_after_work_starts_afresh(orc):
    """work() on a capture whose length is no multiple of R and whose tail is loud, then feed() of another stream on
    the same demodulator: the front end's output and the packets are those of a fresh demodulator (no index, phase
    or filter history carried over)."""
    cap = ddc_cases.capture("qpsk512_r3")
    R, fc, wide = cap["R"], cap["freqs"][1], cap["wide"]
    rng = np.random.default_rng(3)
    loud = (30.0 * (rng.standard_normal(1000) + 1j * rng.standard_normal(1000))).astype(np.complex64)
    first = np.concatenate([wide[:len(wide) // 2], loud])
    while len(first) % R == 0:
        first = first[:-1]
    kw = dict(ddc=dict(decimation=R, center_freq=fc, taps=cap["taps"]))

    def stream(d):
        rec = _record_ddc(d)
        out = []
        for a in range(0, len(wide), 5000):
            out += d.feed(wide[a:a + 5000])
        out += d.flush()
        return np.concatenate(rec), out

    used, fresh = ofdm.ofdm_demod(_options(cap), **kw), ofdm.ofdm_demod(_options(cap), **kw)
    try:
        used.work(first)
        y_used, p_used = stream(used)
        y_fresh, p_fresh = stream(fresh)
        assert len(y_used) == len(y_fresh) == ddc_cases.count(0, len(wide), R)
        assert np.array_equal(y_used, y_fresh)
        assert p_used == p_fresh and [p for ok, p in p_fresh if ok] == cap["payloads"][1]
        # and a second stream after a flush, and a work() after a stream
        y_again, p_again = stream(used)
        assert np.array_equal(y_again, y_fresh) and p_again == p_fresh
        used.feed(first[:7001])
        assert used.work(wide) == p_fresh
    finally:
        used.engine().close()
        fresh.engine().close()


def test_receive_path_and_command_line_take_the_front_end(orc, tmp_path):
    cap = ddc_cases.capture("qpsk512_r4")
    sent = cap["payloads"][0]
    got = []
    rp = receive_path.receive_path(lambda ok, p: got.append((ok, p)), _options(cap),
                                   ddc=dict(decimation=4, center_freq=0.25, taps=cap["taps"]))
    try:
        assert rp.work(cap["wide"]) == got and [p for ok, p in got if ok] == sent
    finally:
        rp.ofdm_rx.engine().close()
    # the options' ddc_decim / ddc_freq, as --ddc-decim / --ddc-freq set them
    opt = _options(cap)
    opt.ddc_decim, opt.ddc_freq = 4, -0.25
    rp = receive_path.receive_path(None, opt)
    try:
        assert [p for ok, p in rp.work(cap["wide"]) if ok] == cap["payloads"][1]
    finally:
        rp.ofdm_rx.engine().close()
    # benchmark_ofdm_rx on a wideband capture file, whole and in chunks
    f = str(tmp_path / "wide.dat")
    sink = iqio.file_sink(f)
    sink.write(cap["wide"])
    sink.close()
    for extra in ([], ["--chunk-samples", "5000"]):
        acct = benchmark_ofdm_rx.main(["-m", "qpsk", "--from-file", f, "--to-file", str(tmp_path / "rx.txt"),
                                       "--ddc-decim", "4", "--ddc-freq", "0.25"] + extra)
        assert (acct.n_rcvd, acct.n_right) == (4, 4)
    # without the flags the wideband file is not a capture of this modem
    acct = benchmark_ofdm_rx.main(["-m", "qpsk", "--from-file", f, "--to-file", str(tmp_path / "rx.txt")])
    assert acct.n_right == 0


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


def _raw_cfg(**kw):
    c = ddc.ddc_cfg(4, 0.25, taps=np.ones(5, np.float32))
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_invalid_arguments_are_refused(eng):
    lib = _abi.load()
    eng.set_ddc(None)
    x = np.zeros(64, np.complex64)
    out64 = np.zeros(64, np.complex64)

    def raw_ddc():
        """ofdm_ddc itself (Engine.ddc asks ofdm_ddc_count first, which refuses on its own)"""
        n = C.c_uint64(0)
        return lib.ofdm_ddc(eng._h, x.ctypes.data_as(C.c_void_p), 64, out64.ctypes.data_as(C.c_void_p), 64, C.byref(n))

    assert raw_ddc() == _abi.OFDM_E_INVAL            # no configuration
    with pytest.raises(ValueError):
        eng.ddc(x)
    with pytest.raises(ValueError):
        eng.ddc_reset(0)
    eng.set_ddc(_raw_cfg())
    assert raw_ddc() == _abi.OFDM_OK
    eng.set_ddc(None)
    assert raw_ddc() == _abi.OFDM_E_INVAL            # ... and after a configuration was dropped
    for bad in (dict(struct_size=12), dict(decimation=0), dict(decimation=65), dict(ntaps=0), dict(ntaps=1025),
                dict(center_freq=0.5000001), dict(center_freq=-0.51), dict(center_freq=float("nan"))):
        with pytest.raises(ValueError):
            eng.set_ddc(_raw_cfg(**bad))
    for v in (float("nan"), float("inf")):
        c = _raw_cfg()
        c.taps[3] = v
        with pytest.raises(ValueError):
            eng.set_ddc(c)
    assert raw_ddc() == _abi.OFDM_E_INVAL            # a refused configuration changes nothing: still none in force
    eng.set_ddc(_raw_cfg(center_freq=0.5))           # the ends of the range are inside it
    eng.set_ddc(_raw_cfg(center_freq=-0.5))
    # a 16-bit pointer that is not 4-byte aligned
    eng.set_rx_iq_format("sc16")
    try:
        q = np.zeros(2 * 64 + 2, np.int16)
        out = np.zeros(64, np.complex64)
        n = C.c_uint64(0)
        rc = lib.ofdm_ddc(eng._h, C.c_void_p(q.ctypes.data + 2), 64, out.ctypes.data_as(C.c_void_p), 64, C.byref(n))
        assert rc == _abi.OFDM_E_INVAL
        assert eng.ddc_count(64) == 16               # ... and the stream did not move
    finally:
        eng.set_rx_iq_format("fc32")
        eng.set_ddc(None)


def test_phase_step_and_index_limits(eng):
    """fc R a hair below a whole turn from the negative side: frac rounds up to 1 and the phase step is 0, not 2^64;
    stream indices are refused before 64-bit arithmetic could wrap."""
    rng = np.random.default_rng(9)
    raw, x = _stream(rng, 700, "fc32")
    taps = (rng.standard_normal(9) / 3).astype(np.float32)
    try:
        c = _set(eng, 4, taps, -1e-20)
        assert ddc_cases.phase_step(-1e-20, 4) == 0
        eng.ddc_reset(1000003)
        _check_against_model(eng.ddc(raw), x, c, 4, -1e-20, 1000003, "fc=-1e-20")
        eng.ddc_reset(1 << 62)
        assert eng.ddc_count(8) == 2
        with pytest.raises(ValueError):
            eng.ddc_reset((1 << 62) + 1)
        assert eng.ddc_count(8) == 2                 # the refused reset left the stream where it was
    finally:
        eng.set_ddc(None)


def test_capacity_error_leaves_the_stream_state(eng):
    lib = _abi.load()
    rng = np.random.default_rng(5)
    raw, _ = _stream(rng, 5000, "fc32")
    taps = ddc.design(3, 0.4)
    eng.set_ddc(ddc.ddc_cfg(3, 0.2, taps=taps))
    try:
        want = eng.ddc(raw).copy()
        eng.ddc_reset(0)
        first = eng.ddc(raw[:1001])
        need = eng.ddc_count(3999)
        out = np.zeros(need, np.complex64)
        n = C.c_uint64(0)
        rc = lib.ofdm_ddc(eng._h, raw[1001:].ctypes.data_as(C.c_void_p), 3999, out.ctypes.data_as(C.c_void_p), need - 1,
                          C.byref(n))
        assert rc == _abi.OFDM_E_CAPACITY and n.value == need
        assert eng.ddc_count(3999) == need
        rest = eng.ddc(raw[1001:])
        assert np.array_equal(np.concatenate([first, rest]), want)
    finally:
        eng.set_ddc(None)


def test_without_a_ddc_the_receiver_launches_what_it_launched(orc):
    """Two handles demodulate the same narrowband stream: one never saw the front end, the other used it on another
    stream and dropped it.  Same packets, same per-kernel launch counts; the kernel table has no entry for the DDC."""
    cap = ddc_cases.capture("qpsk512_r4")
    cfg = cap["cfg"]
    a, b = engine.Engine(cfg=cfg), engine.Engine(cfg=cfg)
    try:
        b.set_ddc(ddc.ddc_cfg(4, 0.25, taps=cap["taps"]))
        y = b.ddc(cap["wide"])
        b.set_ddc(None)
        for e in (a, b):
            e.prof_enable(True)
            e.prof_reset()
        pa, pb = a.rx(y), b.rx(y)
        assert pa == pb and len(pa) == 4
        ca = {k: v[1] for k, v in a.prof().items()}
        cb = {k: v[1] for k, v in b.prof().items()}
        assert ca == cb and sum(ca.values()) > 0
        assert len(ca) == _abi.K_COUNT == 11 and not any("ddc" in k for k in ca)
        # with a front end configured the receiver's own launches stay what they are, and the DDC reports its time
        b.set_ddc(ddc.ddc_cfg(4, 0.25, taps=cap["taps"]))
        b.prof_reset()
        y2 = b.ddc(cap["wide"])
        assert np.array_equal(y2, y) and b.ddc_last_ms() > 0.0
        assert b.rx(y2) == pa
        assert {k: v[1] for k, v in b.prof().items()} == ca
    finally:
        a.close()
        b.close()
