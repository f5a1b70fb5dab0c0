"""The rational-rate front end on the GPU (k_resamp, Engine.resamp, ofdm_demod(resample=...)): against the float64
model of its definition, under arbitrary segmentation of the stream, end to end on wideband captures whose rate is no
integer multiple of the modem's, and at its edges."""
import ctypes as C

import numpy as np
import pytest

import resamp_cases
from helpers import make_cfg
from ofdm_uhd_amd import _abi, benchmark_ofdm_rx, engine, iqio, ofdm, options, predictive_sense, receive_path, resample

pytestmark = pytest.mark.gpu

FCS = (0.0, 0.25, -1.0 / 3.0 + 0.013, 0.5)
RATIOS = ((1, 1), (1, 3), (2, 5), (3, 2), (4, 3), (5, 2), (7, 1), (8, 25), (64, 63), (63, 64), (1, 64), (64, 1))
EPS = 2.0 ** -24


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(cfg=make_cfg())
    yield e
    e.close()


def _tap_counts(L):
    return sorted({1, 2, 31, 155, 1024} | ({L - 1} if L - 1 >= 1 else set()))


def _stream(rng, n, fmt):
    """(samples in the receive format, the same samples converted to complex64)"""
    if fmt == "sc16":
        q = rng.integers(-32768, 32768, (n, 2)).astype(np.int16)
        return q, iqio.from_sc16(q)
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    return x, x


def _set(eng, L, M, taps, fc):
    eng.set_resamp(resample.resamp_cfg(L, M, fc, taps=taps))
    c = eng.resamp_taps()
    assert c.dtype == np.complex64 and len(c) == len(taps)
    return c


def _check_against_model(y, x, c, L, M, fc, first, what):
    """The derived bound: |y - y64| <= (ceil(ntaps / L) + 16) 2^-24 sum |c| |x| per output -- a
    float32 sum of at most ceil(ntaps / L) products in any order, 16 more roundings for the complex products and the
    rotation."""
    y64, s = resamp_cases.model(x, c, L, M, resamp_cases.phase_step(fc, L, M), first)
    assert len(y) == len(y64) == resamp_cases.count(first, len(x), L, M), what
    err = np.abs(y.astype(np.complex128) - y64)
    bound = (-(-len(c) // L) + 16) * EPS * s
    worst = float(np.max(err / np.maximum(bound, 1e-300))) if len(y) else 0.0
    print("%s: %d outputs, worst error / bound = %.3g" % (what, len(y), worst))
    assert np.all(err <= bound), what


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


def _chunk_sizes(rng, n, L, M, ntaps):
    tile, Q = resamp_cases.tile_inputs(L, M), (ntaps - 1) // L
    sizes = [s for s in (1, M - 1, M, Q - 1, Q + 1, 997, tile - 1, tile + 1) if s >= 1]
    weights = np.array([1.0 if v < 16 else 4.0 for v in sizes])
    out, left = [], n
    seq = list(sizes)                       # every size once, then random draws (small ones weighted down)
    while left > 0:
        s = min(seq.pop(0) if seq else int(rng.choice(sizes, p=weights / weights.sum())), left)
        out.append(s)
        left -= s
    return out


@pytest.mark.parametrize("fmt", ["fc32", "sc16"])
@pytest.mark.parametrize("L,M,ntaps", [(2, 5, 39), (4, 3, 23), (8, 25, 481), (64, 63, 1024), (1, 64, 63), (64, 1, 1024),
                                       (3, 2, 2), (5, 7, 1)])
def test_any_segmentation_gives_the_same_bits(eng, L, M, ntaps, fmt):
    rng = np.random.default_rng(77 * L + 5 * M + ntaps)
    tile = resamp_cases.tile_inputs(L, M)
    n = 3 * tile + 1234 + 2 * ((ntaps - 1) // L)
    eng.set_rx_iq_format(fmt)
    try:
        raw, x = _stream(rng, n, fmt)
        taps = (rng.standard_normal(ntaps) / np.sqrt(ntaps)).astype(np.float32)
        fc = -1.0 / 3.0 + 0.013
        c = _set(eng, L, M, taps, fc)
        whole = eng.resamp(raw).copy()
        _check_against_model(whole, x, c, L, M, fc, 0, "whole L/M=%d/%d ntaps=%d %s" % (L, M, ntaps, fmt))
        eng.resamp_reset(0)
        parts, a, empty = [], 0, 0
        sizes = _chunk_sizes(rng, n, L, M, ntaps)
        if M > L:
            # one call that produces nothing for certain: cut the first longer chunk where a single sample completes no
            # output (between two outputs the input index advances by M / L > 1)
            k = next(i for i, s in enumerate(sizes) if s > 2 * M)
            at = sum(sizes[:k])
            lone = next(j for j in range(1, M + 1) if resamp_cases.count(at + j, 1, L, M) == 0)
            sizes[k:k + 1] = [lone, 1, sizes[k] - lone - 1]
        assert sum(sizes) == n and min(sizes) >= 1
        for s in sizes:
            want = resamp_cases.count(a, s, L, M)
            assert eng.resamp_count(s) == want
            y = eng.resamp(raw[a:a + s])
            assert len(y) == want
            empty += want == 0
            parts.append(y)
            a += s
        assert empty >= 1 or M <= L         # calls that produce nothing are part of the stream
        assert np.array_equal(np.concatenate(parts), whole)
        # ... and from a start that is no multiple of M
        first = 7 * M + 1
        eng.resamp_reset(first)
        w2 = eng.resamp(raw).copy()
        assert len(w2) == resamp_cases.count(first, n, L, M)
        eng.resamp_reset(first)
        p2 = [eng.resamp(raw[i:i + 997]) for i in range(0, n, 997)]
        assert np.array_equal(np.concatenate(p2), w2)
    finally:
        eng.set_rx_iq_format("fc32")
        eng.set_resamp(None)


def _options(cap):
    return options.default_options(modulation=cap["mod"], fft_length=cap["N"], occupied_tones=cap["occ"], cp_length=cap["CP"])


def _wide_sc16(wide):
    """The capture as 16-bit IQ with its peak at half scale; nothing may saturate."""
    peak = float(max(np.max(np.abs(wide.real)), np.max(np.abs(wide.imag))))
    q = iqio.to_sc16(wide * np.float32(0.5 / peak))
    assert int(np.max(np.abs(q.astype(np.int32)))) < 32767, "a sample saturated"
    return q


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


def _record_resamp(d):
    """Keeps what the demodulator's front end hands to the receiver."""
    e, rec = d.engine(), []
    orig = e.resamp

    def resamp_and_keep(iq):
        y = orig(iq)
        rec.append(y.copy())
        return y
    e.resamp = resamp_and_keep
    return rec


def test_a_stream_fed_after_work_starts_afresh(orc):
    """work() on a capture whose length is no multiple of M and whose tail is loud, then feed() of another stream on
    the same demodulator: the front end's output and the packets are those of a fresh demodulator (no index, phase
    or filter history carried over)."""
    cap = resamp_cases.capture("qpsk512_2_5")
    L, M, fc, wide = cap["L"], cap["M"], cap["freqs"][1], cap["wide"]
    rng = np.random.default_rng(3)
    loud = (30.0 * (rng.standard_normal(1000) + 1j * rng.standard_normal(1000))).astype(np.complex64)
    first = np.concatenate([wide[:len(wide) // 2], loud])
    while len(first) % M == 0:
        first = first[:-1]
    kw = dict(resample=dict(interpolation=L, decimation=M, center_freq=fc, taps=cap["taps"]))

    def stream(d):
        rec = _record_resamp(d)
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
        assert len(y_used) == len(y_fresh) == resamp_cases.count(0, len(wide), L, M)
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
    cap = resamp_cases.capture("qpsk512_2_5")
    sent = cap["payloads"][0]
    got = []
    rp = receive_path.receive_path(lambda ok, p: got.append((ok, p)), _options(cap),
                                   resample=dict(interpolation=2, decimation=5, center_freq=0.22, taps=cap["taps"]))
    try:
        assert rp.work(cap["wide"]) == got and [p for ok, p in got if ok] == sent
    finally:
        rp.ofdm_rx.engine().close()
    # the options' resamp_interp / resamp_decim / resamp_freq, as --resamp-* set them; the taps are the designed ones
    opt = _options(cap)
    opt.resamp_interp, opt.resamp_decim, opt.resamp_freq = 2, 5, -0.21
    rp = receive_path.receive_path(None, opt)
    try:
        c = rp.ofdm_rx.engine().resamp_taps()
        assert np.max(np.abs(c - resample.bandpass_taps(resample.design(2, 5, 200 / 512.0), -0.21, 2))) <= 2 * EPS * 2
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
                                       "--resamp-interp", "2", "--resamp-decim", "5", "--resamp-freq", "0.22"] + extra)
        assert (acct.n_rcvd, acct.n_right) == (4, 4)
    # without the flags the wideband file is not a capture of this modem
    acct = benchmark_ofdm_rx.main(["-m", "qpsk", "--from-file", f, "--to-file", str(tmp_path / "rx.txt")])
    assert acct.n_right == 0


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


def _raw_cfg(**kw):
    c = resample.resamp_cfg(2, 5, 0.25, taps=np.ones(5, np.float32))
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_invalid_arguments_are_refused(eng):
    lib = _abi.load()
    eng.set_resamp(None)
    x = np.zeros(64, np.complex64)
    out64 = np.zeros(64, np.complex64)

    def raw_resamp():
        """ofdm_resamp itself (Engine.resamp asks ofdm_resamp_count first, which refuses on its own)"""
        n = C.c_uint64(0)
        return lib.ofdm_resamp(eng._h, x.ctypes.data_as(C.c_void_p), 64, out64.ctypes.data_as(C.c_void_p), 64, C.byref(n))

    assert raw_resamp() == _abi.OFDM_E_INVAL            # no configuration
    for call in (lambda: eng.resamp(x), lambda: eng.resamp_reset(0), lambda: eng.resamp_count(8), eng.resamp_taps):
        with pytest.raises(ValueError):
            call()
    eng.set_resamp(_raw_cfg())
    assert raw_resamp() == _abi.OFDM_OK
    eng.set_resamp(None)
    assert raw_resamp() == _abi.OFDM_E_INVAL            # ... and after a configuration was dropped
    bads = (dict(struct_size=12), dict(interpolation=0), dict(interpolation=65), dict(decimation=0), dict(decimation=65),
            dict(ntaps=0), dict(ntaps=1025), dict(center_freq=0.5000001), dict(center_freq=-0.51),
            dict(center_freq=float("nan")))
    for bad in bads:
        with pytest.raises(ValueError):
            eng.set_resamp(_raw_cfg(**bad))
    for v in (float("nan"), float("inf")):
        c = _raw_cfg()
        c.taps[3] = v
        with pytest.raises(ValueError):
            eng.set_resamp(c)
    assert raw_resamp() == _abi.OFDM_E_INVAL            # a refused configuration changes nothing: still none in force
    # ... and with one in force it stays in force, stream state included
    eng.set_resamp(_raw_cfg())
    eng.resamp(x[:7])
    table = eng.resamp_taps()
    for bad in bads:
        with pytest.raises(ValueError):
            eng.set_resamp(_raw_cfg(**bad))
    assert np.array_equal(eng.resamp_taps(), table) and eng.resamp_count(64) == resamp_cases.count(7, 64, 2, 5)
    eng.set_resamp(_raw_cfg(center_freq=0.5))           # the ends of the range are inside it
    eng.set_resamp(_raw_cfg(center_freq=-0.5))
    # a 16-bit pointer that is not 4-byte aligned
    eng.set_rx_iq_format("sc16")
    try:
        q = np.zeros(2 * 64 + 2, np.int16)
        out = np.zeros(64, np.complex64)
        n = C.c_uint64(0)
        eng.resamp(q[:6].reshape(3, 2))
        rc = lib.ofdm_resamp(eng._h, C.c_void_p(q.ctypes.data + 2), 64, out.ctypes.data_as(C.c_void_p), 64, C.byref(n))
        assert rc == _abi.OFDM_E_INVAL
        assert eng.resamp_count(64) == resamp_cases.count(3, 64, 2, 5)    # ... and the stream did not move
    finally:
        eng.set_rx_iq_format("fc32")
        eng.set_resamp(None)


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
    lib = _abi.load()
    rng = np.random.default_rng(5)
    raw, _ = _stream(rng, 5000, "fc32")
    eng.set_resamp(resample.resamp_cfg(3, 4, 0.2, taps=resample.design(3, 4, 0.4)))
    try:
        want = eng.resamp(raw).copy()
        eng.resamp_reset(0)
        first = eng.resamp(raw[:1001])
        need = eng.resamp_count(3999)
        out = np.zeros(need, np.complex64)
        n = C.c_uint64(0)
        rc = lib.ofdm_resamp(eng._h, raw[1001:].ctypes.data_as(C.c_void_p), 3999, out.ctypes.data_as(C.c_void_p), need - 1,
                             C.byref(n))
        assert rc == _abi.OFDM_E_CAPACITY and n.value == need
        assert eng.resamp_count(3999) == need
        rest = eng.resamp(raw[1001:])
        assert np.array_equal(np.concatenate([first, rest]), want)
    finally:
        eng.set_resamp(None)


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
    """Two handles demodulate the same narrowband stream: one never saw the resampler, the other used it on another
    stream and dropped it.  Same packets, same per-kernel launch counts; the kernel table has no entry for it."""
    cap = resamp_cases.capture("qpsk512_2_5")
    cfg, fc = cap["cfg"], cap["freqs"][0]
    a, b = engine.Engine(cfg=cfg), engine.Engine(cfg=cfg)
    try:
        b.set_resamp(resample.resamp_cfg(2, 5, fc, taps=cap["taps"]))
        y = b.resamp(cap["wide"])
        b.set_resamp(None)
        for e in (a, b):
            e.prof_enable(True)
            e.prof_reset()
        pa, pb = a.rx(y), b.rx(y)
        assert pa == pb and len(pa) == 4
        ca = {k: v[1] for k, v in a.prof().items()}
        cb = {k: v[1] for k, v in b.prof().items()}
        assert ca == cb and sum(ca.values()) > 0
        assert len(ca) == _abi.K_COUNT == 11 and not any("resamp" in k for k in ca)
        # with a resampler configured the receiver's own launches stay what they are, and the stage reports its time
        b.set_resamp(resample.resamp_cfg(2, 5, fc, taps=cap["taps"]))
        with pytest.raises(ValueError):
            b.resamp_last_ms()                       # nothing timed yet
        b.prof_reset()
        y2 = b.resamp(cap["wide"])
        assert np.array_equal(y2, y) and b.resamp_last_ms() > 0.0
        assert b.rx(y2) == pa
        assert {k: v[1] for k, v in b.prof().items()} == ca
    finally:
        a.close()
        b.close()
