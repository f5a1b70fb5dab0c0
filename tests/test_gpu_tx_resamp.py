"""The rational-rate transmit stage on the GPU (k_tx_resamp, Engine.tx_resamp, ofdm_mod(resample=...)): against the
float64 model of its definition, bit for bit against the DUC at M = 1, under arbitrary segmentation of the stream, end
to end through the receive resampler on bands built on the device, through the public objects, and at its edges."""
import ctypes as C

import numpy as np
import pytest

import tx_resamp_cases as cases
from helpers import make_cfg, make_payloads
from ofdm_uhd_amd import (_abi, benchmark_ofdm_rx, benchmark_ofdm_tx, duc, engine, iqio, ofdm, options, resample,
                          transmit_path, tx_resample)

pytestmark = pytest.mark.gpu

FCS = (0.0, 0.25, -1.0 / 3.0 + 0.013, -0.5)
RATIOS = ((1, 1), (2, 1), (5, 2), (3, 4), (4, 3), (25, 8), (8, 25), (64, 63), (64, 1), (1, 64), (7, 64))
SCALE = 32768.0


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(cfg=make_cfg())
    yield e
    e.close()


def _tap_counts(L):
    return sorted(n for n in {1, L - 1, L, 39, 481, 1024} if n >= 1)


def _stream(rng, n, amp=1.0):
    return (amp * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)


def _taps(rng, ntaps, L):
    return (rng.standard_normal(ntaps) * np.sqrt(L / float(ntaps))).astype(np.float32)


def _set(eng, L, M, taps, fc, fmt="fc32"):
    eng.set_tx_resamp(tx_resample.tx_resamp_cfg(L, M, fc, taps=taps, out_format=fmt))


def _as_complex(y, fmt):
    """The stored samples as float64 complex numbers, in units of the float output (int16 / full scale)."""
    if fmt == "sc16":
        assert y.dtype == np.int16 and y.ndim == 2 and y.shape[1] == 2
        return (y[:, 0].astype(np.float64) + 1j * y[:, 1].astype(np.float64)) / SCALE
    assert y.dtype == np.complex64
    return y.astype(np.complex128)


def _check_against_model(y, x, taps, L, M, fc, first, fmt, what, add=None):
    """The derived bound (tx_resamp_cases.bound): |y - y64| <= (ceil(ntaps / L) + 16) 2^-24
    (s[n] + |add[n]|); 16-bit output: |q - scale y64| <= 0.5 + scale bound per part wherever nothing clamps.  Returns
    the worst error / bound."""
    y64, s = cases.model(x, taps, L, M, cases.phase_step(fc), first)
    if add is not None:
        y64 = y64 + np.asarray(add).astype(np.complex128)
    assert len(y) == len(y64) == cases.count(first, len(x), L, M), what
    bound = cases.bound(len(taps), L, s, add)
    d = _as_complex(y, fmt) - y64
    if fmt == "sc16":
        free = (np.abs(y64.real) * SCALE < 32767 - 1) & (np.abs(y64.imag) * SCALE < 32767 - 1)
        assert np.count_nonzero(free) > 0.9 * len(y), what
        err = np.maximum(np.abs(d.real), np.abs(d.imag))[free]
        bound = (0.5 / SCALE + bound)[free]
    else:
        err = np.abs(d)
    worst = float(np.max(err / np.maximum(bound, 1e-300))) if len(err) else 0.0
    assert np.all(err <= bound), "%s: worst error / bound = %.3g" % (what, worst)
    return worst


@pytest.mark.parametrize("fmt", ["fc32", "sc16"])
@pytest.mark.parametrize("L,M", RATIOS)
def test_against_float64_model(eng, L, M, fmt):
    rng = np.random.default_rng(3000 + 100 * L + M)
    tin = cases.tile_inputs(L, M)
    n = 3 * tin + tin // 3 + 5                                   # three tiles and a ragged end
    x = _stream(rng, n, 0.05)
    worst = 0.0
    try:
        for ti, ntaps in enumerate(_tap_counts(L)):
            taps = _taps(rng, ntaps, L)
            for fi, fc in enumerate(FCS):
                _set(eng, L, M, taps, fc, fmt)
                # with and without `add`, alternating so that every tap count and every frequency sees both
                add = _stream(rng, cases.count(0, n, L, M), 0.05) if (ti + fi) % 2 else None
                y = eng.tx_resamp(x, add=add)
                worst = max(worst, _check_against_model(y, x, taps, L, M, fc, 0, fmt, "L=%d M=%d ntaps=%d fc=%g %s add=%s" % (
                    L, M, ntaps, fc, fmt, add is not None), add=add))
        # once more far from index 0 with the generic frequency: n D mod 2^64 at input index 10^6
        for add_on in (False, True):
            taps = _taps(rng, 39, L)
            _set(eng, L, M, taps, FCS[2], fmt)
            assert cases.phase_step(FCS[2]) % (1 << 32) != 0
            eng.tx_resamp_reset(1000003)
            add = _stream(rng, cases.count(1000003, n, L, M), 0.05) if add_on else None
            worst = max(worst, _check_against_model(eng.tx_resamp(x, add=add), x, taps, L, M, FCS[2], 1000003, fmt,
                                                    "L=%d M=%d reset to 1000003 %s" % (L, M, fmt), add=add))
    finally:
        eng.set_tx_resamp(None)
    print("L=%d M=%d %s: worst error / bound = %.3g" % (L, M, fmt, worst))


@pytest.mark.parametrize("L", [1, 2, 4, 5, 8, 64])
def test_decimation_one_is_the_duc_bit_for_bit(eng, L):
    rng = np.random.default_rng(500 + L)
    tout = cases.tile_inputs(L, 1) * L
    n = (2 * tout + tout // 3) // L + 5
    x = _stream(rng, n, 0.05)
    w = _stream(rng, n * L, 0.05)
    try:
        for ntaps in (1, 31, 155, 1024):
            taps = _taps(rng, ntaps, L)
            for fmt in ("fc32", "sc16"):
                for add in (None, w):
                    for first in (0, 1000003):
                        eng.set_duc(duc.duc_cfg(L, FCS[2], taps=taps, out_format=fmt))
                        eng.duc_reset(first)
                        want = eng.duc(x, add=add)
                        _set(eng, L, 1, taps, FCS[2], fmt)
                        eng.tx_resamp_reset(first)
                        got = eng.tx_resamp(x, add=add)
                        assert got.dtype == want.dtype and np.array_equal(got, want), (L, ntaps, fmt, add is not None, first)
                        assert np.any(got)
    finally:
        eng.set_duc(None)
        eng.set_tx_resamp(None)


def test_unit_stage_returns_its_input(eng):
    x = _stream(np.random.default_rng(1), 5000)
    try:
        _set(eng, 1, 1, [1.0], 0.0)
        assert np.array_equal(eng.tx_resamp(x), x)
    finally:
        eng.set_tx_resamp(None)


def _part_sum(a, b):
    """a + b formed in float32 part by part."""
    a, b = np.asarray(a, np.complex64), np.asarray(b, np.complex64)
    out = np.empty(len(a), np.complex64)
    out.real = a.real + b.real
    out.imag = a.imag + b.imag
    return out


@pytest.mark.parametrize("L,M,ntaps", [(1, 1, 5), (5, 2, 39), (3, 4, 41), (64, 63, 100)])
def test_add_is_one_float32_addition_per_part(eng, L, M, ntaps):
    rng = np.random.default_rng(31 * L + M)
    x = _stream(rng, 7000 * M // L + 3, 0.1)
    w = _stream(rng, cases.count(0, len(x), L, M), 0.1)
    taps = _taps(rng, ntaps, L)
    try:
        _set(eng, L, M, taps, FCS[2])
        plain = eng.tx_resamp(x).copy()
        eng.tx_resamp_reset(0)
        want = _part_sum(w, plain)
        assert np.array_equal(eng.tx_resamp(x, add=w), want)
        _check_against_model(want, x, taps, L, M, FCS[2], 0, "fc32", "add L=%d M=%d" % (L, M), add=w)
        # 16-bit output: the library's quantisation rule applied to that float32 sum
        _set(eng, L, M, taps, FCS[2], "sc16")
        q = eng.tx_resamp(x, add=w)
        assert q.dtype == np.int16 and np.array_equal(q, iqio.to_sc16(want))
        eng.tx_resamp_reset(0)
        assert np.array_equal(eng.tx_resamp(x), iqio.to_sc16(plain))
        # `add` must hold exactly what the call produces from where the stream stands (hence the reset: the count of
        # a call depends on its first index)
        eng.tx_resamp_reset(0)
        for bad in (w[:-1], np.concatenate([w, w[:1]])):
            with pytest.raises(ValueError):
                eng.tx_resamp(x, add=bad)
        assert np.array_equal(eng.tx_resamp(x, add=w), q)
    finally:
        eng.set_tx_resamp(None)


def _chunk_sizes(rng, n, L, M, ntaps):
    Q = cases.history(ntaps, L)
    tin = cases.tile_inputs(L, M)
    sizes = [s for s in (0, 1, L - 1, M, Q - 1, Q + 1, 997, tin - 1, tin, tin + 1) if s >= 0]
    out, left = [], n
    # every size once, at L < M then M single inputs in a row (they complete L < M outputs: some call produces
    # nothing), then random draws
    seq = list(sizes) + ([1] * M if L < M else [])
    while left > 0:
        s = min(seq.pop(0) if seq else int(rng.choice(sizes + [int(rng.integers(1, 3000))])), left)
        out.append(s)
        left -= s
    return out


@pytest.mark.parametrize("fmt", ["fc32", "sc16"])
@pytest.mark.parametrize("L,M,ntaps", [(1, 1, 31), (2, 1, 1024), (5, 2, 39), (3, 4, 41), (25, 8, 481), (8, 25, 155),
                                       (64, 63, 1024), (7, 64, 200)])
def test_any_segmentation_gives_the_same_bits(eng, L, M, ntaps, fmt):
    rng = np.random.default_rng(77 * L + 13 * M + ntaps)
    Q = cases.history(ntaps, L)
    tin = cases.tile_inputs(L, M)
    n = 3 * tin + 2 * Q + 1234 + 997
    x = _stream(rng, n, 0.05)
    taps = _taps(rng, ntaps, L)
    fc = FCS[2]
    try:
        for first in (0, 7 * 1024 + 5):
            assert M == 1 or first == 0 or (first * L) % M != 0
            w = _stream(rng, cases.count(first, n, L, M), 0.05)
            for add in (None, w):
                _set(eng, L, M, taps, fc, fmt)
                eng.tx_resamp_reset(first)
                whole = eng.tx_resamp(x, add=add).copy()
                _check_against_model(whole, x, taps, L, M, fc, first, fmt, "whole L=%d M=%d ntaps=%d %s" % (L, M, ntaps, fmt),
                                     add=add)
                eng.tx_resamp_reset(first)
                sizes = _chunk_sizes(rng, n, L, M, ntaps) if first == 0 else [997] * (n // 997) + [n % 997]
                parts, a, o, empty = [], 0, 0, 0
                for s in sizes:
                    cnt = cases.count(first + a, s, L, M)
                    assert eng.tx_resamp_count(s) == cnt
                    y = eng.tx_resamp(x[a:a + s], add=None if add is None else add[o:o + cnt])
                    assert len(y) == cnt
                    empty += s > 0 and cnt == 0
                    parts.append(y)
                    a += s
                    o += cnt
                assert a == n and o == len(whole) and np.array_equal(np.concatenate(parts), whole)
                if first == 0:
                    assert 0 in sizes and (Q < 2 or any(0 < s < Q for s in sizes))
                    assert L >= M or empty > 0          # at L < M some call produced nothing
    finally:
        eng.set_tx_resamp(None)


def _engine_tx(e):
    def tx(cfg, payloads, lead, tail):
        e.set_channel(sigma=0.0, lead=lead, tail=tail)
        try:
            return e.tx(payloads)
        finally:
            e.set_channel(enable=False)
    return tx


@pytest.mark.parametrize("name,fmt", [("qpsk512_5_2", "fc32"), ("qpsk512_5_2", "sc16"), ("qam16_512_3_4", "fc32"),
                                      ("bpsk64_25_8", "fc32")])
def test_links_end_to_end(orc, name, fmt):
    """Engine.tx -> Engine.tx_resamp per link (the second added onto the first) -> the noise of resamp_cases ->
    Engine.resamp -> Engine.rx per link: nothing but the noise is made on the host."""
    cfg0 = make_cfg(*cases.CASES[name][:4])
    e = engine.Engine(cfg=cfg0)
    try:
        k = cases.links(name, tx=_engine_tx(e))
        L, M, xs, fs = k["L"], k["M"], k["x"], k["freqs"]
        nw = cases.count(0, len(xs[0]), L, M)
        e.set_tx_resamp(tx_resample.tx_resamp_cfg(L, M, fs[0], taps=k["tx_taps"]))
        wa = e.tx_resamp(xs[0])
        assert len(wa) == nw
        noise = cases.noise(nw, k["P"], L, M)
        if fmt == "sc16":
            # the noise goes into the band before the second link is added onto it: the final store is the 16-bit one
            assert len(xs) == 2
            noisy = (wa.astype(np.complex128) + noise).astype(np.complex64)
            e.set_tx_resamp(tx_resample.tx_resamp_cfg(L, M, fs[1], taps=k["tx_taps"], out_format="sc16"))
            wide = e.tx_resamp(xs[1], add=noisy)
            assert wide.dtype == np.int16 and wide.shape == (nw, 2)
            assert int(wide.min()) > -32768 and int(wide.max()) < 32767, "a stored part sits on the rail"
        else:
            both = wa
            if len(xs) == 2:
                e.set_tx_resamp(tx_resample.tx_resamp_cfg(L, M, fs[1], taps=k["tx_taps"]))
                both = e.tx_resamp(xs[1], add=wa)
                e.tx_resamp_reset(0)
                assert np.array_equal(both, _part_sum(wa, e.tx_resamp(xs[1])))
            wide = (both.astype(np.complex128) + noise).astype(np.complex64)
        e.set_tx_resamp(None)
        for fc, sent in zip(fs, k["payloads"]):
            e.set_rx_iq_format(fmt)
            e.set_resamp(resample.resamp_cfg(M, L, fc, taps=k["rx_taps"]))
            y = e.resamp(wide)
            e.set_rx_iq_format("fc32")
            e.set_resamp(None)
            got = e.rx(y)
            assert got == orc.rx(k["cfg"], y).packets, (name, fc)
            assert [ok for ok, _ in got] == [True] * 4 and [p for _, p in got] == sent, (name, fc)
    finally:
        e.close()


def _with_noise_floor(wide, ratio, lead, tail, seed=5):
    """Silence around the stream and a noise floor 30 dB below the link inside its band, which is 1 / ratio of the
    wideband one (the receiver's metric is 0/0 on exact zeros)."""
    rng = np.random.default_rng(seed)
    x = np.concatenate([np.zeros(lead, np.complex64), wide, np.zeros(tail, np.complex64)])
    sigma = np.sqrt(float(np.mean(np.abs(wide) ** 2)) * ratio / 1e3)
    return (x + sigma * np.sqrt(0.5) * (rng.standard_normal(len(x)) + 1j * rng.standard_normal(len(x)))).astype(np.complex64)


@pytest.mark.parametrize("fmt", ["fc32", "sc16"])
def test_modulator_with_the_stage_feeds_the_demodulator_with_its_resampler(fmt):
    opt = options.default_options(modulation="qpsk", fft_length=512, occupied_tones=200, cp_length=128)
    opt.tx_amplitude = 0.25
    # 90-byte payloads fill their last symbol exactly at this geometry: no seeded fill symbols, whose values depend on a
    # packet's place in its batch, so three batches modulate to the samples of one
    sent = make_payloads(6, 90, seed=3)
    L, M, fc = 5, 2, -0.21
    rs = dict(interpolation=L, decimation=M, center_freq=fc)
    one = ofdm.ofdm_mod(opt, pad_for_usrp=False, iq_format=fmt, resample=rs)
    three = ofdm.ofdm_mod(opt, pad_for_usrp=False, iq_format=fmt, resample=rs)
    d = ofdm.ofdm_demod(opt, resample=dict(interpolation=M, decimation=L, center_freq=fc))
    try:
        for m in (one, three):
            m.engine().set_tx_amplitude(0.1)                    # (the modulator alone has unit gain: keep off the 16-bit rails)
        assert one.engine().tx_resamp_cfg.ntaps == 39 and one.engine().tx_iq_format == "fc32" and one.engine().duc_cfg is None
        assert one.flush(end=True) is None                      # nothing queued, nothing in flight
        for p in sent:
            one.send_pkt(p)
        whole = one.flush(end=True)
        _, nsamp = one.engine().tx_frame_count([len(p) for p in sent])
        Q = (39 - 1) // L
        assert len(whole) == cases.count(0, nsamp + Q, L, M)
        assert whole.dtype == (np.int16 if fmt == "sc16" else np.complex64)
        # three batches and the end: the stream continues across flush() calls
        sink = iqio.vector_sink()
        three.connect(sink)
        parts = []
        for batch in (sent[:2], sent[2:3], sent[3:]):
            for p in batch:
                three.send_pkt(p)
            parts.append(three.flush())
        assert sum(len(p) for p in parts) == cases.count(0, nsamp, L, M)
        three.send_pkt(eof=True)                                # delivers the tail
        assert len(sink.data()) == len(whole) and np.array_equal(sink.data(), whole)
        # ... and a second stream on the same modulator starts afresh
        for p in sent:
            three.send_pkt(p)
        assert np.array_equal(three.flush(end=True), whole)
        wide = iqio.from_sc16(whole) if fmt == "sc16" else whole
        got = d.work(_with_noise_floor(wide, L / float(M), 4096, 8192))
        assert [p for ok, p in got if ok] == sent
    finally:
        for o in (one, three, d):
            o.engine().close()


def test_transmit_path_and_command_line_take_the_stage(tmp_path):
    opt = options.default_options(modulation="qpsk", fft_length=512, occupied_tones=200, cp_length=128)
    opt.tx_amplitude = 0.25
    opt.tx_resamp_interp, opt.tx_resamp_decim, opt.tx_resamp_freq = 5, 2, 0.22
    tp = transmit_path.transmit_path(opt)
    try:
        cfg = tp.ofdm_tx.engine().tx_resamp_cfg
        assert (cfg.interpolation, cfg.decimation, cfg.center_freq, cfg.ntaps) == (5, 2, 0.22, 39)
        tp.send_pkt(b"\x00\x01\x00\x00 one packet")
        y = tp.flush(end=True)
        assert y.dtype == np.complex64 and len(y) > 0
    finally:
        tp.ofdm_tx.engine().close()
    f = str(tmp_path / "wide.dat")
    npk = benchmark_ofdm_tx.main(["-m", "qpsk", "--to-file", f, "-M", "9e-6", "--tx-resamp-interp", "5",
                                  "--tx-resamp-decim", "2", "--tx-resamp-freq", "0.22"])
    assert npk == 4
    wide = iqio.read_complex_binary(f)
    iqio.file_sink(f).write(_with_noise_floor(wide, 2.5, 4096, 8192))
    acct = benchmark_ofdm_rx.main(["-m", "qpsk", "--from-file", f, "--to-file", str(tmp_path / "rx.txt"),
                                   "--resamp-interp", "2", "--resamp-decim", "5", "--resamp-freq", "0.22"])
    assert (acct.n_rcvd, acct.n_right) == (4, 4)
    # tuned to the other side of the band there is nothing
    acct = benchmark_ofdm_rx.main(["-m", "qpsk", "--from-file", f, "--to-file", str(tmp_path / "rx.txt"),
                                   "--resamp-interp", "2", "--resamp-decim", "5", "--resamp-freq", "-0.22"])
    assert acct.n_right == 0


def test_device_pointer_path_behind_an_asynchronous_transmit():
    torch = pytest.importorskip("torch")
    cfg = make_cfg()
    pays = make_payloads(4, 100, seed=7)
    L, M = 5, 2
    taps = tx_resample.design(L, M, 200 / 512.0)
    host = engine.Engine(cfg=cfg)
    dev = engine.Engine(cfg=make_cfg(device_ptrs=True))
    try:
        x = host.tx(pays)
        nw = cases.count(0, len(x), L, M)
        host.set_tx_resamp(tx_resample.tx_resamp_cfg(L, M, 0.22, taps=taps))
        want = host.tx_resamp(x)
        w = _stream(np.random.default_rng(2), nw, 0.1)
        host.tx_resamp_reset(0)
        want_add = host.tx_resamp(x, add=w)

        blob, offs, lens = engine.pack_payloads(pays)
        _, nsamp = dev.tx_frame_count(lens)
        assert nsamp == len(x)
        d_pay = torch.from_numpy(blob.copy()).cuda()
        d_iq = torch.zeros(nsamp, dtype=torch.complex64, device="cuda")
        d_out = torch.zeros(nw, dtype=torch.complex64, device="cuda")
        dev.set_tx_resamp(tx_resample.tx_resamp_cfg(L, M, 0.22, taps=taps))
        torch.cuda.synchronize()
        assert dev.tx_resamp_count(nsamp) == nw
        assert dev.tx_device(d_pay.data_ptr(), offs, lens, d_iq.data_ptr(), nsamp, wait=False) == nsamp
        assert dev.tx_resamp_device(d_iq.data_ptr(), nsamp, d_out.data_ptr(), nw) == nw
        assert np.array_equal(d_iq.cpu().numpy(), x)
        assert np.array_equal(d_out.cpu().numpy(), want)
        # `add` aliasing the output: each sample is read before it is written
        d_out.copy_(torch.from_numpy(w))
        torch.cuda.synchronize()
        dev.tx_resamp_reset(0)
        assert dev.tx_resamp_device(d_iq.data_ptr(), nsamp, d_out.data_ptr(), nw, add_ptr=d_out.data_ptr()) == nw
        assert np.array_equal(d_out.cpu().numpy(), want_add)
        assert np.array_equal(want_add, _part_sum(w, want))
        # ... and at M = 1 the aliased call gives the DUC's bits
        w4 = _stream(np.random.default_rng(3), nsamp * 4, 0.1)
        t4 = duc.design(4, 200 / 512.0)
        d_o4 = torch.from_numpy(w4).cuda()
        dev.set_duc(duc.duc_cfg(4, 0.25, taps=t4))
        torch.cuda.synchronize()
        assert dev.duc_device(d_iq.data_ptr(), nsamp, d_o4.data_ptr(), nsamp * 4, add_ptr=d_o4.data_ptr()) == nsamp * 4
        ref = d_o4.cpu().numpy()
        d_o4.copy_(torch.from_numpy(w4))
        dev.set_tx_resamp(tx_resample.tx_resamp_cfg(4, 1, 0.25, taps=t4))
        torch.cuda.synchronize()
        assert dev.tx_resamp_device(d_iq.data_ptr(), nsamp, d_o4.data_ptr(), nsamp * 4, add_ptr=d_o4.data_ptr()) == nsamp * 4
        assert np.array_equal(d_o4.cpu().numpy(), ref) and not np.array_equal(ref, w4)
    finally:
        host.close()
        dev.close()


def _raw_cfg(**kw):
    c = tx_resample.tx_resamp_cfg(4, 3, 0.25, taps=np.ones(5, np.float32))
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_invalid_arguments_are_refused(eng):
    lib = _abi.load()
    eng.set_tx_resamp(None)
    x = np.zeros(66, np.complex64)
    out = np.zeros(4 * 66 + 1, np.complex64)

    def raw(inp=None, outp=None, add=None, nin=66):
        n = C.c_uint64(0)
        return lib.ofdm_tx_resamp(eng._h, C.c_void_p(inp or x.ctypes.data), nin, C.c_void_p(add) if add else None,
                                  C.c_void_p(outp or out.ctypes.data), 4 * 66, C.byref(n))

    def raw_count(nin):
        n = C.c_uint64(0)
        return lib.ofdm_tx_resamp_count(eng._h, nin, C.byref(n))

    assert raw() == _abi.OFDM_E_INVAL                # no configuration
    assert raw_count(10) == _abi.OFDM_E_INVAL
    with pytest.raises(ValueError):
        eng.tx_resamp(x)
    with pytest.raises(ValueError):
        eng.tx_resamp_reset(0)
    with pytest.raises(ValueError):
        eng.tx_resamp_count(10)
    with pytest.raises(ValueError):
        eng.tx_resamp_last_ms()
    eng.set_tx_resamp(_raw_cfg())
    assert raw() == _abi.OFDM_OK
    eng.set_tx_resamp(None)
    assert raw() == _abi.OFDM_E_INVAL                # ... and after a configuration was dropped
    bads = (dict(struct_size=12), dict(interpolation=0), dict(interpolation=65), dict(decimation=0), dict(decimation=65),
            dict(ntaps=0), dict(ntaps=1025), dict(out_format=2), dict(out_format=1, out_scale=-1.0),
            dict(out_format=1, out_scale=float("inf")), dict(out_format=1, out_scale=float("nan")),
            dict(center_freq=0.5000001), dict(center_freq=-0.51), dict(center_freq=float("nan")))
    for bad in bads:
        with pytest.raises(ValueError):
            eng.set_tx_resamp(_raw_cfg(**bad))
    for v in (float("nan"), float("inf")):
        c = _raw_cfg()
        c.taps[3] = v
        with pytest.raises(ValueError):
            eng.set_tx_resamp(c)
    assert raw() == _abi.OFDM_E_INVAL                # a refused configuration changes nothing: still none in force
    try:
        eng.set_tx_resamp(_raw_cfg(center_freq=0.5))     # the ends of the range are inside it
        eng.set_tx_resamp(_raw_cfg(center_freq=-0.5, out_format=1, out_scale=0.0))
        # ... and a refused one leaves the old one in force: 16-bit output, 4 outputs per 3 inputs
        with pytest.raises(ValueError):
            eng.set_tx_resamp(_raw_cfg(decimation=65))
        y = eng.tx_resamp(x)
        assert y.dtype == np.int16 and y.shape == (88, 2)
        eng.tx_resamp_reset(0)
        # misaligned pointers: 4-byte for the 16-bit output, 8-byte for every float32 buffer
        assert raw(outp=out.ctypes.data + 2) == _abi.OFDM_E_INVAL
        assert raw(outp=out.ctypes.data + 4) == _abi.OFDM_OK
        assert raw(inp=x.ctypes.data + 4, nin=60) == _abi.OFDM_E_INVAL
        assert raw(add=out.ctypes.data + 4) == _abi.OFDM_E_INVAL
        eng.set_tx_resamp(_raw_cfg())
        assert raw(outp=out.ctypes.data + 4) == _abi.OFDM_E_INVAL
        # indices: the next input index stays at or below 2^56
        eng.tx_resamp_reset(1 << 56)
        with pytest.raises(ValueError):
            eng.tx_resamp_reset((1 << 56) + 1)
        assert raw(nin=1) == _abi.OFDM_E_INVAL       # the stream stands at the limit: not one more sample
        assert raw_count(1) == _abi.OFDM_E_INVAL
        assert raw(nin=0) == _abi.OFDM_OK
        eng.tx_resamp_reset((1 << 56) - 66)
        assert raw(nin=66) == _abi.OFDM_OK and raw(nin=1) == _abi.OFDM_E_INVAL
    finally:
        eng.set_tx_resamp(None)


def test_capacity_error_leaves_the_stream_state(eng):
    lib = _abi.load()
    x = _stream(np.random.default_rng(5), 5000, 0.1)
    eng.set_tx_resamp(tx_resample.tx_resamp_cfg(3, 4, 0.2, taps=tx_resample.design(3, 4, 0.4)))
    try:
        want = eng.tx_resamp(x).copy()
        eng.tx_resamp_reset(0)
        first = eng.tx_resamp(x[:1001])
        cnt = cases.count(1001, 3999, 3, 4)
        out = np.zeros(cnt, np.complex64)
        n = C.c_uint64(0)
        rc = lib.ofdm_tx_resamp(eng._h, x[1001:].ctypes.data_as(C.c_void_p), 3999, None, out.ctypes.data_as(C.c_void_p),
                                cnt - 1, C.byref(n))
        assert rc == _abi.OFDM_E_CAPACITY and n.value == cnt
        rest = eng.tx_resamp(x[1001:])
        assert np.array_equal(np.concatenate([first, rest]), want)
    finally:
        eng.set_tx_resamp(None)


def test_the_duc_and_this_stage_keep_separate_state_on_one_handle(eng):
    rng = np.random.default_rng(8)
    x = _stream(rng, 6000, 0.1)
    td, tr = duc.design(4, 0.4), tx_resample.design(5, 2, 0.4)
    try:
        eng.set_duc(duc.duc_cfg(4, 0.25, taps=td))
        want_d = eng.duc(x).copy()
        eng.set_tx_resamp(tx_resample.tx_resamp_cfg(5, 2, -0.2, taps=tr))
        want_r = eng.tx_resamp(x).copy()
        # the two streams interleaved, chunk by chunk, with a reset of one in the middle of the other
        eng.duc_reset(0)
        eng.tx_resamp_reset(0)
        pd, pr = [], []
        for a in range(0, 6000, 1000):
            pd.append(eng.duc(x[a:a + 1000]))
            pr.append(eng.tx_resamp(x[a:a + 1000]))
        assert np.array_equal(np.concatenate(pd), want_d) and np.array_equal(np.concatenate(pr), want_r)
        eng.duc_reset(0)
        half = eng.duc(x[:3000])
        eng.set_tx_resamp(tx_resample.tx_resamp_cfg(5, 2, -0.2, taps=tr))   # re-configuring one leaves the other's stream alone
        assert np.array_equal(np.concatenate([half, eng.duc(x[3000:])]), want_d)
        eng.tx_resamp(x[:3000])
        eng.set_duc(None)
        assert np.array_equal(eng.tx_resamp(x[3000:]), want_r[cases.count(0, 3000, 5, 2):])
    finally:
        eng.set_duc(None)
        eng.set_tx_resamp(None)


def test_without_the_stage_transmitter_and_receiver_launch_what_they_launched(orc):
    """Two handles run the same TX + RX: one never saw the stage, the other used it and dropped it.  Same IQ bits,
    same packets, same per-kernel launch counts; the kernel table has no entry for the stage."""
    cfg = make_cfg()
    pays = make_payloads(4, 100, seed=11)
    a, b = engine.Engine(cfg=cfg), engine.Engine(cfg=cfg)
    rcfg = tx_resample.tx_resamp_cfg(5, 2, 0.22, taps=tx_resample.design(5, 2, 200 / 512.0))
    try:
        b.set_tx_resamp(rcfg)
        b.prof_enable(True)
        assert len(b.tx_resamp(_stream(np.random.default_rng(1), 3000, 0.1))) == 7500 and b.tx_resamp_last_ms() > 0.0
        b.set_tx_resamp(None)
        with pytest.raises(ValueError):
            b.tx_resamp_last_ms()
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
        assert len(ca) == _abi.K_COUNT == 11 and not any("resamp" in k for k in ca)
        # with the stage configured and used, the kernel table still counts only what it counted
        b.set_tx_resamp(rcfg)
        b.prof_reset()
        b.tx_resamp(xb)
        assert np.array_equal(b.tx(pays), xa) and b.rx(xa) == pa
        assert {k: v[1] for k, v in b.prof().items()} == ca
    finally:
        a.close()
        b.close()
