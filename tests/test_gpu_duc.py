"""The wideband transmit stage on the GPU (k_duc, Engine.duc, ofdm_mod(duc=...)): against the float64 model of its
definition, its exact identities, under arbitrary segmentation of the stream, end to end through the receive stage on
two-link bands built on the device, through the public objects, and at its edges."""
import ctypes as C

import numpy as np
import pytest

import ddc_cases
import duc_cases
from helpers import make_cfg
from ofdm_uhd_amd import (_abi, benchmark_ofdm_rx, benchmark_ofdm_tx, ddc, duc, engine, iqio, ofdm, options,
                          transmit_path)

pytestmark = pytest.mark.gpu

FCS = (0.0, 0.25, -1.0 / 3.0 + 0.013, 0.5)
INTERPS = (1, 2, 3, 4, 8, 64)
SCALE = 32768.0


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(cfg=make_cfg())
    yield e
    e.close()


def _tap_counts(L):
    return sorted(n for n in {1, 2, L - 1, L, L + 1, 31, 155, 1024} if n >= 1)


def _stream(rng, n, amp=1.0):
    return (amp * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)


def _set(eng, L, taps, fc, fmt="fc32"):
    eng.set_duc(duc.duc_cfg(L, fc, taps=taps, out_format=fmt))


def _as_complex(y, fmt):
    """The stored samples as float64 complex numbers, in units of the float output (int16 / full scale)."""
    if fmt == "sc16":
        assert y.dtype == np.int16 and y.ndim == 2 and y.shape[1] == 2
        return (y[:, 0].astype(np.float64) + 1j * y[:, 1].astype(np.float64)) / SCALE
    assert y.dtype == np.complex64
    return y.astype(np.complex128)


def _check_against_model(y, x, taps, L, fc, first, fmt, what, add=None):
    """The derived bound (duc_cases.bound): |y - y64| <= (Q + 1 + 16) 2^-24 s[n]; 16-bit output:
    |q - scale y64| <= 0.5 + scale bound per part wherever nothing clamps."""
    y64, s = duc_cases.model(x, taps, L, duc_cases.phase_step(fc), first)
    if add is not None:
        y64 = y64 + np.asarray(add).astype(np.complex128)
    assert len(y) == len(y64) == len(x) * L, what
    bound = duc_cases.bound(len(taps), L, s, add)
    d = _as_complex(y, fmt) - y64
    if fmt == "sc16":
        free = (np.abs(y64.real) * SCALE < 32767 - 1) & (np.abs(y64.imag) * SCALE < 32767 - 1)
        assert np.count_nonzero(free) > 0.9 * len(y), what
        err = np.maximum(np.abs(d.real), np.abs(d.imag))[free]
        bound = (0.5 / SCALE + bound)[free]
    else:
        err = np.abs(d)
    worst = float(np.max(err / np.maximum(bound, 1e-300))) if len(err) else 0.0
    print("%s: %d outputs, worst error / bound = %.3g" % (what, len(y), worst))
    assert np.all(err <= bound), what


@pytest.mark.parametrize("fmt", ["fc32", "sc16"])
@pytest.mark.parametrize("L", INTERPS)
def test_against_float64_model(eng, L, fmt):
    rng = np.random.default_rng(2000 + L)
    tile = duc_cases.tile_outputs(L)
    n = (2 * tile + tile // 3) // L + 5
    while (n * L) % tile == 0:
        n += 1
    x = _stream(rng, n, 0.05)
    try:
        for ntaps in _tap_counts(L):
            taps = (rng.standard_normal(ntaps) * np.sqrt(L / float(ntaps))).astype(np.float32)
            for fc in FCS:
                _set(eng, L, taps, fc, fmt)
                _check_against_model(eng.duc(x), x, taps, L, fc, 0, fmt, "L=%d ntaps=%d fc=%g %s" % (L, ntaps, fc, fmt))
        # once more far from index 0 with the generic frequency: n D mod 2^64 at n of 10^6 L
        taps = (rng.standard_normal(31) * np.sqrt(L / 31.0)).astype(np.float32)
        _set(eng, L, taps, FCS[2], fmt)
        assert duc_cases.phase_step(FCS[2]) % (1 << 32) != 0
        eng.duc_reset(1000003)
        _check_against_model(eng.duc(x), x, taps, L, FCS[2], 1000003, fmt, "L=%d reset to 1000003 %s" % (L, fmt))
    finally:
        eng.set_duc(None)


def test_unit_stage_returns_its_input(eng):
    x = _stream(np.random.default_rng(1), 5000)
    try:
        _set(eng, 1, [1.0], 0.0)
        assert np.array_equal(eng.duc(x), x)
    finally:
        eng.set_duc(None)


def _part_sum(a, b):
    """a + b formed in float32 part by part."""
    a, b = np.asarray(a, np.complex64), np.asarray(b, np.complex64)
    out = np.empty(len(a), np.complex64)
    out.real = a.real + b.real
    out.imag = a.imag + b.imag
    return out


@pytest.mark.parametrize("L,ntaps", [(1, 5), (3, 155), (4, 31), (64, 100)])
def test_add_is_one_float32_addition_per_part(eng, L, ntaps):
    rng = np.random.default_rng(31 * L)
    x = _stream(rng, 7000 // L + 3, 0.1)
    w = _stream(rng, len(x) * L, 0.1)
    taps = (rng.standard_normal(ntaps) * np.sqrt(L / float(ntaps))).astype(np.float32)
    try:
        _set(eng, L, taps, FCS[2])
        plain = eng.duc(x).copy()
        eng.duc_reset(0)
        want = _part_sum(w, plain)
        assert np.array_equal(eng.duc(x, add=w), want)
        _check_against_model(want, x, taps, L, FCS[2], 0, "fc32", "add L=%d" % L, add=w)
        # 16-bit output: the library's quantisation rule applied to that float32 sum
        _set(eng, L, taps, FCS[2], "sc16")
        q = eng.duc(x, add=w)
        assert q.dtype == np.int16 and np.array_equal(q, iqio.to_sc16(want))
        eng.duc_reset(0)
        assert np.array_equal(eng.duc(x), iqio.to_sc16(plain))
    finally:
        eng.set_duc(None)


def _chunk_sizes(rng, n, L, ntaps):
    Q = duc_cases.history(ntaps, L)
    tin = duc_cases.tile_outputs(L) // L
    sizes = [s for s in (0, 1, Q - 1, Q, Q + 1, 997, tin - 1, tin, tin + 1) if s >= 0]
    out, left = [], n
    seq = list(sizes)                       # every size once, then random draws
    while left > 0:
        s = min(seq.pop(0) if seq else int(rng.choice(sizes)), left)
        out.append(s)
        left -= s
    return out


@pytest.mark.parametrize("fmt", ["fc32", "sc16"])
@pytest.mark.parametrize("L,ntaps", [(1, 31), (2, 1024), (3, 155), (4, 31), (4, 3), (8, 155), (8, 7), (64, 1024), (64, 63),
                                     (5, 2), (17, 1)])
def test_any_segmentation_gives_the_same_bits(eng, L, ntaps, fmt):
    rng = np.random.default_rng(77 * L + ntaps)
    Q = duc_cases.history(ntaps, L)
    tin = duc_cases.tile_outputs(L) // L
    n = 3 * tin + 2 * Q + 1234 + (997 if L > 1 else 0)
    x = _stream(rng, n, 0.05)
    taps = (rng.standard_normal(ntaps) * np.sqrt(L / float(ntaps))).astype(np.float32)
    fc = FCS[2]
    try:
        _set(eng, L, taps, fc, fmt)
        whole = eng.duc(x).copy()
        _check_against_model(whole, x, taps, L, fc, 0, fmt, "whole L=%d ntaps=%d %s" % (L, ntaps, fmt))
        eng.duc_reset(0)
        sizes = _chunk_sizes(rng, n, L, ntaps)
        assert 0 in sizes and (Q < 2 or any(0 < s < Q for s in sizes))
        parts, a = [], 0
        for s in sizes:
            y = eng.duc(x[a:a + s])
            assert len(y) == s * L
            parts.append(y)
            a += s
        assert a == n and np.array_equal(np.concatenate(parts), whole)
        # ... and from a reset to a non-zero index
        first = 7 * 1024 + 5
        eng.duc_reset(first)
        w2 = eng.duc(x).copy()
        assert L == 1 and ntaps == 1 or not np.array_equal(w2, whole)
        eng.duc_reset(first)
        p2 = [eng.duc(x[i:i + 997]) for i in range(0, n, 997)]
        assert np.array_equal(np.concatenate(p2), w2)
    finally:
        eng.set_duc(None)


def _options(k):
    return options.default_options(modulation=k["mod"], fft_length=k["N"], occupied_tones=k["occ"], cp_length=k["CP"])


def _engine_tx(e):
    def tx(cfg, payloads, lead, tail):
        e.set_channel(sigma=0.0, lead=lead, tail=tail)
        try:
            return e.tx(payloads)
        finally:
            e.set_channel(enable=False)
    return tx


@pytest.mark.parametrize("name,fmt", [("qpsk512_r4", "fc32"), ("qpsk512_r4", "sc16"), ("qam16_2048_r2", "fc32"),
                                      ("bpsk64_r8", "fc32"), ("qpsk512_r3", "fc32")])
def test_two_links_end_to_end(orc, name, fmt):
    """Engine.tx -> Engine.duc per link (the second added onto the first) -> the noise of ddc_cases -> Engine.ddc ->
    Engine.rx per link: nothing but the noise is made on the host."""
    cfg0 = make_cfg(*ddc_cases.CASES[name][:4])
    e = engine.Engine(cfg=cfg0)
    try:
        k = duc_cases.links(name, tx=_engine_tx(e))
        R, (xa, xb), (fa, fb) = k["R"], k["x"], k["freqs"]
        e.set_duc(duc.duc_cfg(R, fa, taps=k["tx_taps"]))
        wa = e.duc(xa)
        noisy = (wa.astype(np.complex128) + duc_cases.noise(len(wa), k["P"], R)).astype(np.complex64)
        if fmt == "sc16":
            # the noise goes into the band before the second link is added onto it: the final store is the 16-bit one
            e.set_duc(duc.duc_cfg(R, fb, taps=k["tx_taps"], out_format="sc16"))
            wide = e.duc(xb, add=noisy)
            assert wide.dtype == np.int16 and wide.shape == (len(xa) * R, 2)
            assert int(wide.min()) > -32768 and int(wide.max()) < 32767, "a stored part sits on the rail"
        else:
            e.set_duc(duc.duc_cfg(R, fb, taps=k["tx_taps"]))
            both = e.duc(xb, add=wa)
            e.duc_reset(0)
            assert np.array_equal(both, _part_sum(wa, e.duc(xb)))
            wide = (both.astype(np.complex128) + duc_cases.noise(len(wa), k["P"], R)).astype(np.complex64)
            peak = float(np.max(np.abs(wide)))
            print("%s: peak |sample| of the noisy two-link band = %.3f" % (name, peak))
        e.set_duc(None)
        for fc, sent in zip((fa, fb), k["payloads"]):
            e.set_rx_iq_format(fmt)
            e.set_ddc(ddc.ddc_cfg(R, fc, taps=k["rx_taps"]))
            y = e.ddc(wide)
            e.set_rx_iq_format("fc32")
            e.set_ddc(None)
            got = e.rx(y)
            assert got == orc.rx(k["cfg"], y).packets, (name, fc)
            assert [ok for ok, _ in got] == [True] * 4 and [p for _, p in got] == sent, (name, fc)
    finally:
        e.close()


def _with_noise_floor(wide, R, lead, tail, seed=5):
    """Silence around the stream and a noise floor 30 dB below the link inside its band (the receiver's metric is 0/0
    on exact zeros)."""
    rng = np.random.default_rng(seed)
    x = np.concatenate([np.zeros(lead, np.complex64), wide, np.zeros(tail, np.complex64)])
    sigma = np.sqrt(float(np.mean(np.abs(wide) ** 2)) * R / 1e3)
    return (x + sigma * np.sqrt(0.5) * (rng.standard_normal(len(x)) + 1j * rng.standard_normal(len(x)))).astype(np.complex64)


@pytest.mark.parametrize("fmt", ["fc32", "sc16"])
def test_modulator_with_the_stage_feeds_the_demodulator_with_its_front_end(fmt):
    from helpers import make_payloads
    opt = options.default_options(modulation="qpsk", fft_length=512, occupied_tones=200, cp_length=128)
    opt.tx_amplitude = 0.25
    # 90-byte payloads fill their last symbol exactly at this geometry: no seeded fill symbols, whose values depend on a
    # packet's place in its batch, so three batches modulate to the samples of one
    sent = make_payloads(6, 90, seed=3)
    L, fc = 4, -0.25
    one = ofdm.ofdm_mod(opt, pad_for_usrp=False, iq_format=fmt, duc=dict(interpolation=L, center_freq=fc))
    three = ofdm.ofdm_mod(opt, pad_for_usrp=False, iq_format=fmt, duc=dict(interpolation=L, center_freq=fc))
    d = ofdm.ofdm_demod(opt, ddc=dict(decimation=L, center_freq=fc))
    try:
        for m in (one, three):
            m.engine().set_tx_amplitude(0.1)                    # (the modulator alone has unit gain: keep off the 16-bit rails)
        assert one.engine().duc_cfg.ntaps == 31 and one.engine().tx_iq_format == "fc32"
        assert one.flush(end=True) is None                      # nothing queued, nothing in flight
        for p in sent:
            one.send_pkt(p)
        whole = one.flush(end=True)
        _, nsamp = one.engine().tx_frame_count([len(p) for p in sent])
        Q = (31 - 1) // L
        assert len(whole) == (nsamp + Q) * L
        assert whole.dtype == (np.int16 if fmt == "sc16" else np.complex64)
        # three batches and the end: the stream continues across flush() calls
        sink = iqio.vector_sink()
        three.connect(sink)
        parts = []
        for batch in (sent[:2], sent[2:3], sent[3:]):
            for p in batch:
                three.send_pkt(p)
            parts.append(three.flush())
        three.send_pkt(eof=True)
        assert sum(len(p) for p in parts) == nsamp * L
        assert np.array_equal(sink.data(), whole)
        # ... and a second stream on the same modulator starts afresh
        for p in sent:
            three.send_pkt(p)
        assert np.array_equal(three.flush(end=True), whole)
        wide = iqio.from_sc16(whole) if fmt == "sc16" else whole
        got = d.work(_with_noise_floor(wide, L, 4096, 8192))
        assert [p for ok, p in got if ok] == sent
    finally:
        for o in (one, three, d):
            o.engine().close()


def test_transmit_path_and_command_line_take_the_stage(tmp_path):
    opt = options.default_options(modulation="qpsk", fft_length=512, occupied_tones=200, cp_length=128)
    opt.tx_amplitude = 0.25
    opt.duc_interp, opt.duc_freq = 4, 0.25
    tp = transmit_path.transmit_path(opt)
    try:
        cfg = tp.ofdm_tx.engine().duc_cfg
        assert (cfg.interpolation, cfg.center_freq, cfg.ntaps) == (4, 0.25, 31)
        tp.send_pkt(b"\x00\x01\x00\x00 one packet")
        y = tp.flush(end=True)
        assert y.dtype == np.complex64 and len(y) % 4 == 0
    finally:
        tp.ofdm_tx.engine().close()
    f = str(tmp_path / "wide.dat")
    npk = benchmark_ofdm_tx.main(["-m", "qpsk", "--to-file", f, "-M", "9e-6", "--duc-interp", "4", "--duc-freq", "0.25"])
    assert npk == 4
    wide = iqio.read_complex_binary(f)
    assert len(wide) % 4 == 0
    iqio.file_sink(f).write(_with_noise_floor(wide, 4, 4096, 8192))
    acct = benchmark_ofdm_rx.main(["-m", "qpsk", "--from-file", f, "--to-file", str(tmp_path / "rx.txt"),
                                   "--ddc-decim", "4", "--ddc-freq", "0.25"])
    assert (acct.n_rcvd, acct.n_right) == (4, 4)
    # tuned to the other side of the band there is nothing
    acct = benchmark_ofdm_rx.main(["-m", "qpsk", "--from-file", f, "--to-file", str(tmp_path / "rx.txt"),
                                   "--ddc-decim", "4", "--ddc-freq", "-0.25"])
    assert acct.n_right == 0


def test_device_pointer_path_behind_an_asynchronous_transmit():
    torch = pytest.importorskip("torch")
    from helpers import make_payloads
    cfg = make_cfg()
    pays = make_payloads(4, 100, seed=7)
    L = 4
    taps = duc.design(L, 200 / 512.0)
    host = engine.Engine(cfg=cfg)
    dev = engine.Engine(cfg=make_cfg(device_ptrs=True))
    try:
        x = host.tx(pays)
        host.set_duc(duc.duc_cfg(L, 0.25, taps=taps))
        want = host.duc(x)
        w = _stream(np.random.default_rng(2), len(x) * L, 0.1)
        host.duc_reset(0)
        want_add = host.duc(x, add=w)

        blob, offs, lens = engine.pack_payloads(pays)
        _, nsamp = dev.tx_frame_count(lens)
        assert nsamp == len(x)
        d_pay = torch.from_numpy(blob.copy()).cuda()
        d_iq = torch.zeros(nsamp, dtype=torch.complex64, device="cuda")
        d_out = torch.zeros(nsamp * L, dtype=torch.complex64, device="cuda")
        dev.set_duc(duc.duc_cfg(L, 0.25, taps=taps))
        torch.cuda.synchronize()
        assert dev.tx_device(d_pay.data_ptr(), offs, lens, d_iq.data_ptr(), nsamp, wait=False) == nsamp
        assert dev.duc_device(d_iq.data_ptr(), nsamp, d_out.data_ptr(), nsamp * L) == nsamp * L
        assert np.array_equal(d_iq.cpu().numpy(), x)
        assert np.array_equal(d_out.cpu().numpy(), want)
        # `add` aliasing the output: each sample is read before it is written
        d_out.copy_(torch.from_numpy(w))
        torch.cuda.synchronize()
        dev.duc_reset(0)
        assert dev.duc_device(d_iq.data_ptr(), nsamp, d_out.data_ptr(), nsamp * L, add_ptr=d_out.data_ptr()) == nsamp * L
        assert np.array_equal(d_out.cpu().numpy(), want_add)
        assert np.array_equal(want_add, _part_sum(w, want))
    finally:
        host.close()
        dev.close()


def _raw_cfg(**kw):
    c = duc.duc_cfg(4, 0.25, taps=np.ones(5, np.float32))
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_invalid_arguments_are_refused(eng):
    lib = _abi.load()
    eng.set_duc(None)
    x = np.zeros(64, np.complex64)
    out = np.zeros(4 * 64 + 1, np.complex64)

    def raw_duc(inp=None, outp=None, add=None, nin=64):
        n = C.c_uint64(0)
        return lib.ofdm_duc(eng._h, C.c_void_p(inp or x.ctypes.data), nin, C.c_void_p(add) if add else None,
                            C.c_void_p(outp or out.ctypes.data), 4 * 64, C.byref(n))

    assert raw_duc() == _abi.OFDM_E_INVAL            # no configuration
    with pytest.raises(ValueError):
        eng.duc(x)
    with pytest.raises(ValueError):
        eng.duc_reset(0)
    with pytest.raises(ValueError):
        eng.duc_last_ms()
    eng.set_duc(_raw_cfg())
    assert raw_duc() == _abi.OFDM_OK
    eng.set_duc(None)
    assert raw_duc() == _abi.OFDM_E_INVAL            # ... and after a configuration was dropped
    bads = (dict(struct_size=12), dict(interpolation=0), dict(interpolation=65), dict(ntaps=0), dict(ntaps=1025),
            dict(out_format=2), dict(out_format=1, out_scale=-1.0), dict(out_format=1, out_scale=float("inf")),
            dict(out_format=1, out_scale=float("nan")), dict(center_freq=0.5000001), dict(center_freq=-0.51),
            dict(center_freq=float("nan")))
    for bad in bads:
        with pytest.raises(ValueError):
            eng.set_duc(_raw_cfg(**bad))
    for v in (float("nan"), float("inf")):
        c = _raw_cfg()
        c.taps[3] = v
        with pytest.raises(ValueError):
            eng.set_duc(c)
    assert raw_duc() == _abi.OFDM_E_INVAL            # a refused configuration changes nothing: still none in force
    try:
        eng.set_duc(_raw_cfg(center_freq=0.5))       # the ends of the range are inside it
        eng.set_duc(_raw_cfg(center_freq=-0.5, out_format=1, out_scale=0.0))
        # ... and a refused one leaves the old one in force: 16-bit output, 4 outputs per input
        with pytest.raises(ValueError):
            eng.set_duc(_raw_cfg(interpolation=65))
        y = eng.duc(x)
        assert y.dtype == np.int16 and y.shape == (256, 2)
        # misaligned pointers: 4-byte for the 16-bit output, 8-byte for every float32 buffer
        assert raw_duc(outp=out.ctypes.data + 2) == _abi.OFDM_E_INVAL
        assert raw_duc(outp=out.ctypes.data + 4) == _abi.OFDM_OK
        assert raw_duc(inp=x.ctypes.data + 4, nin=60) == _abi.OFDM_E_INVAL
        assert raw_duc(add=out.ctypes.data + 4) == _abi.OFDM_E_INVAL
        eng.set_duc(_raw_cfg())
        assert raw_duc(outp=out.ctypes.data + 4) == _abi.OFDM_E_INVAL
        # indices: no output index may pass 2^63
        eng.duc_reset((1 << 63) // 4)
        with pytest.raises(ValueError):
            eng.duc_reset((1 << 63) // 4 + 1)
        assert raw_duc(nin=1) == _abi.OFDM_E_INVAL   # the stream stands at the limit: not one more sample
        assert raw_duc(nin=0) == _abi.OFDM_OK
        eng.duc_reset((1 << 63) // 4 - 64)
        assert raw_duc(nin=64) == _abi.OFDM_OK and raw_duc(nin=1) == _abi.OFDM_E_INVAL
    finally:
        eng.set_duc(None)


def test_a_tiny_negative_frequency_is_phase_step_zero(eng):
    rng = np.random.default_rng(9)
    x = _stream(rng, 700, 0.1)
    taps = (rng.standard_normal(9) / 3).astype(np.float32)
    try:
        assert duc_cases.phase_step(-1e-20) == 0
        _set(eng, 4, taps, -1e-20)
        eng.duc_reset(1000003)
        y = eng.duc(x)
        _check_against_model(y, x, taps, 4, -1e-20, 1000003, "fc32", "fc=-1e-20")
        _set(eng, 4, taps, 0.0)
        eng.duc_reset(1000003)
        assert np.array_equal(eng.duc(x), y)
    finally:
        eng.set_duc(None)


def test_capacity_error_leaves_the_stream_state(eng):
    lib = _abi.load()
    x = _stream(np.random.default_rng(5), 5000, 0.1)
    eng.set_duc(duc.duc_cfg(3, 0.2, taps=duc.design(3, 0.4)))
    try:
        want = eng.duc(x).copy()
        eng.duc_reset(0)
        first = eng.duc(x[:1001])
        out = np.zeros(3 * 3999, np.complex64)
        n = C.c_uint64(0)
        rc = lib.ofdm_duc(eng._h, x[1001:].ctypes.data_as(C.c_void_p), 3999, None, out.ctypes.data_as(C.c_void_p),
                          3 * 3999 - 1, C.byref(n))
        assert rc == _abi.OFDM_E_CAPACITY and n.value == 3 * 3999
        rest = eng.duc(x[1001:])
        assert np.array_equal(np.concatenate([first, rest]), want)
    finally:
        eng.set_duc(None)


def test_without_a_duc_transmitter_and_receiver_launch_what_they_launched(orc):
    """Two handles run the same TX + RX: one never saw the stage, the other used it and dropped it.  Same IQ bits,
    same packets, same per-kernel launch counts; the kernel table has no entry for the DUC."""
    from helpers import make_payloads
    cfg = make_cfg()
    pays = make_payloads(4, 100, seed=11)
    a, b = engine.Engine(cfg=cfg), engine.Engine(cfg=cfg)
    try:
        b.set_duc(duc.duc_cfg(4, 0.25, taps=duc.design(4, 200 / 512.0)))
        b.prof_enable(True)
        assert len(b.duc(_stream(np.random.default_rng(1), 3000, 0.1))) == 12000 and b.duc_last_ms() > 0.0
        b.set_duc(None)
        with pytest.raises(ValueError):
            b.duc_last_ms()
        for e in (a, b):
            e.set_channel(sigma=0.01, lead=1024, tail=1536)
            e.prof_enable(True)
            e.prof_reset()
        xa, xb = a.tx(pays), b.tx(pays)
        assert np.array_equal(xa, xb)
        pa, pb = a.rx(xa), b.rx(xb)
        assert pa == pb and [p for ok, p in pa if ok] == pays
        ca = {k: v[1] for k, v in a.prof().items()}
        cb = {k: v[1] for k, v in b.prof().items()}
        assert ca == cb and sum(ca.values()) > 0
        assert len(ca) == _abi.K_COUNT == 11 and not any("duc" in k for k in ca)
        # with a stage configured and used, the kernel table still counts only what it counted
        b.set_duc(duc.duc_cfg(4, 0.25, taps=duc.design(4, 200 / 512.0)))
        b.prof_reset()
        b.duc(xb)
        assert np.array_equal(b.tx(pays), xa) and b.rx(xa) == pa
        assert {k: v[1] for k, v in b.prof().items()} == ca
    finally:
        a.close()
        b.close()
