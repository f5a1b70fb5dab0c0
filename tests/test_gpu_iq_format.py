"""16-bit IQ (sc16) at the engine boundary, on the GPU.

The conversion is one float32 operation per part (iqio.from_sc16 / to_sc16 are the normative definitions), so the
project's bar carries over: an engine in sc16 mode fed the int16 capture q computes bit for bit what a float engine
-- and the oracle -- compute from from_sc16(q), and its transmitter stores to_sc16 of what the float transmitter
stores."""

import numpy as np
import pytest

from helpers import loopback_stream, make_cfg, make_payloads
from ofdm_uhd_amd import _abi, config, engine, iqio, ofdm, options
from ofdm_uhd_amd.engine import pack_payloads

pytestmark = pytest.mark.gpu

# (copied from test_gpu_parity.CASES) mod, N, occ, CP, payload, packets, snr, cfo(bins)
CASES = [
    ("qpsk", 512, 200, 128, 1026, 6, 30.0, 0.0),
    ("bpsk", 512, 200, 128, 300, 5, 30.0, 0.05),
    ("qpsk", 512, 200, 128, 1026, 6, 30.0, 0.3),
    ("8psk", 256, 120, 64, 500, 4, 30.0, 0.0),
    ("qam16", 2048, 1200, 512, 4091, 3, 30.0, 0.0),
    ("qam64", 1024, 600, 256, 2000, 3, 36.0, 0.1),
    ("qam64", 4096, 2400, 1024, 4091, 3, 36.0, 0.0),
    ("qam256", 64, 48, 16, 100, 4, 55.0, 0.0),
    ("bpsk", 128, 64, 32, 64, 4, 30.0, 0.0),
    ("qpsk", 512, 200, 128, 1026, 4, 30.0, 1.3),
    ("qpsk", 512, 200, 128, 1026, 4, 30.0, -2.4),
]
A = _abi
ARRAY_TAPS = (A.TAP_RX_CHAN_FILT, A.TAP_RX_PRESEL, A.TAP_RX_FFT, A.TAP_RX_ACQ, A.TAP_RX_SINK, A.TAP_RX_PACKETS)
ALL_TAPS = ARRAY_TAPS + (A.TAP_RX_PEAKS, A.TAP_RX_ANGLES, A.TAP_RX_FRAMES)
STATS = ("symbols", "samples", "peaks", "frames", "headers_ok", "packets", "crc_ok", "chained_frames", "overflow")


def _eng(cfg, rx=None, tx=None, rx_scale=None, tx_scale=None):
    e = engine.Engine(cfg=cfg)
    if rx:
        e.set_rx_iq_format(rx, rx_scale)
    if tx:
        e.set_tx_iq_format(tx, tx_scale)
    return e


def _taps(e, taps=ALL_TAPS):
    return {t: e.tap(t) for t in taps}


def _same_taps(a, b):
    assert sorted(a) == sorted(b)
    for t in a:
        assert a[t].shape == b[t].shape, t
        assert np.array_equal(a[t], b[t], equal_nan=True), t


def _mask(taps):
    m = 0
    for t in taps:
        m |= 1 << t
    return m


# ---- 1. receive parity -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mod,N,occ,CP,plen,npkt,snr,cfo", CASES)
def test_rx_parity_sc16(orc, mod, N, occ, CP, plen, npkt, snr, cfo):
    """Engine A (sc16) on q = engine B (float) on from_sc16(q) = the oracle on from_sc16(q): packets, CRC verdicts,
    stats and every stage tap, with host pointers and with device pointers."""
    import torch
    cfg = make_cfg(mod, N, occ, CP)
    q = iqio.to_sc16(loopback_stream(orc, cfg, make_payloads(npkt, plen), snr_db=snr, cfo_bins=cfo))
    xf = iqio.from_sc16(q)
    ro = orc.rx(cfg, xf, _mask(ARRAY_TAPS))
    ea, eb = _eng(cfg, rx="sc16"), _eng(cfg)
    for e in (ea, eb):
        e.set_taps(*ARRAY_TAPS)
    pa, pb = ea.rx(q), eb.rx(xf)
    assert pa == pb == ro.packets and len(pa) >= 1
    for k in STATS:
        assert ea.last_stats[k] == eb.last_stats[k], k
        if k != "overflow":
            assert ea.last_stats[k] == ro.stats[k], k
    ta, tb = _taps(ea), _taps(eb)
    _same_taps(ta, tb)
    for t in ARRAY_TAPS:
        assert np.array_equal(ta[t], ro.tap(t), equal_nan=True), t
    for t in (A.TAP_RX_PEAKS, A.TAP_RX_FRAMES):
        assert ta[t].tolist() == ro.tap(t).tolist(), t
    assert np.array_equal(ta[A.TAP_RX_ANGLES], ro.tap(A.TAP_RX_ANGLES))
    ea.close()
    eb.close()
    # device pointers: the int16 capture lives in a torch tensor
    ed = engine.Engine(cfg=make_cfg(mod, N, occ, CP, device_ptrs=True))
    ed.set_rx_iq_format("sc16")
    ed.set_taps(*ARRAY_TAPS)
    dev = torch.device("cuda:0")
    d_q = torch.from_numpy(q.copy()).to(dev)
    assert d_q.dtype == torch.int16
    d_pay = torch.zeros(max(64, (plen + 64) * (npkt + 8)), dtype=torch.uint8, device=dev)
    n, off, ln, ok = ed.rx_device(d_q.data_ptr(), len(q), d_pay.data_ptr(), d_pay.numel(), npkt + 8)
    out = d_pay.cpu().numpy()
    assert [(bool(ok[i]), out[int(off[i]):int(off[i]) + int(ln[i])].tobytes()) for i in range(n)] == pa
    _same_taps(_taps(ed), ta)
    ed.close()


def test_rx_parity_other_scale(orc):
    """rx_scale = 1/32767 (not a power of two): still one float32 multiply, still A = B = oracle."""
    mod, N, occ, CP, plen, npkt, snr, cfo = CASES[0]
    cfg = make_cfg(mod, N, occ, CP)
    s = 1.0 / 32767.0
    q = iqio.to_sc16(loopback_stream(orc, cfg, make_payloads(npkt, plen), snr_db=snr, cfo_bins=cfo), 32767.0)
    xf = iqio.from_sc16(q, s)
    assert not np.array_equal(xf, iqio.from_sc16(q))
    ro = orc.rx(cfg, xf, _mask(ARRAY_TAPS))
    ea, eb = _eng(cfg, rx="sc16", rx_scale=s), _eng(cfg)
    for e in (ea, eb):
        e.set_taps(*ARRAY_TAPS)
    assert ea.rx(q) == eb.rx(xf) == ro.packets
    ta = _taps(ea)
    _same_taps(ta, _taps(eb))
    for t in ARRAY_TAPS:
        assert np.array_equal(ta[t], ro.tap(t), equal_nan=True), t
    ea.close()
    eb.close()


# ---- 2. the filter's boundary branch ---------------------------------------------------------------------------------
def test_filter_boundaries(orc):
    cfg = make_cfg("qpsk")
    q = iqio.to_sc16(loopback_stream(orc, cfg, make_payloads(3, 600), snr_db=30.0))
    ea, eb = _eng(cfg, rx="sc16"), _eng(cfg)
    for e in (ea, eb):
        e.set_taps(A.TAP_RX_CHAN_FILT)
    # shorter than one round of filter blocks; lengths that are no multiple of the block; one sample; nothing
    for n, origin in ((len(q), 0), (len(q) - 13, 0), (777, 0), (100, 0), (1, 0), (0, 0), (len(q) - 1, 12345),
                      (3001, 7), (1, 99)):
        for e in (ea, eb):
            e.set_origin(origin)
        pa, pb = ea.rx(q[:n]), eb.rx(iqio.from_sc16(q[:n]))
        assert pa == pb, (n, origin)
        assert ea.last_stats == eb.last_stats, (n, origin)
        if n:
            fa, fb = ea.tap(A.TAP_RX_CHAN_FILT), eb.tap(A.TAP_RX_CHAN_FILT)
            assert len(fa) == n and np.array_equal(fa, fb), (n, origin)
        if n == len(q):
            assert sum(ok for ok, _ in pa) >= 2
    # origin 0, whole capture: the oracle's filter output too
    for e in (ea, eb):
        e.set_origin(0)
    ea.rx(q)
    assert np.array_equal(ea.tap(A.TAP_RX_CHAN_FILT), orc.rx(cfg, iqio.from_sc16(q), 1 << A.TAP_RX_CHAN_FILT).tap(A.TAP_RX_CHAN_FILT))
    ea.close()
    eb.close()


# ---- 3. SYNC "fixed" -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("foff,rx_scale", [(0.0, None), (0.01, None), (0.0, 1.0 / 32767.0)])
def test_sync_fixed_sc16(foff, rx_scale):
    """(rx_scale 1/32767: the expand kernel's multiply is a real rounding, not an exponent shift)"""
    N, CP = 512, 128
    probe = engine.Engine(cfg=make_cfg("qpsk"))
    nsym1, _ = probe.tx_frame_count(np.full(1, 500, np.uint32))
    probe.close()
    opt = options.default_options(modulation="qpsk", fft_length=N, occupied_tones=200, cp_length=CP, sync="fixed",
                                  sync_nsymbols=int(nsym1), sync_freq_offset=foff)
    cfg = config.make_cfg(opt)
    ea, eb = _eng(cfg, rx="sc16", rx_scale=rx_scale), _eng(cfg)
    pay = make_payloads(12, 500, seed=9)
    eb.set_channel(sigma=0.002, lead=0, tail=2 * N)
    q = iqio.to_sc16(eb.tx(pay))
    xf = iqio.from_sc16(q, rx_scale)
    if rx_scale is not None:
        assert not np.array_equal(xf, iqio.from_sc16(q))
    for e in (ea, eb):
        e.set_taps(*ARRAY_TAPS)
    pa, pb = ea.rx(q), eb.rx(xf)
    assert pa == pb
    if foff == 0.0:
        assert len(pa) == len(pay) and [p for ok, p in pa if ok] == pay
    assert ea.last_stats == eb.last_stats
    fixed_taps = tuple(t for t in ALL_TAPS if t != A.TAP_RX_PRESEL)    # (SYNC "fixed" computes no timing metric)
    ta = _taps(ea, fixed_taps)
    _same_taps(ta, _taps(eb, fixed_taps))
    assert np.array_equal(ta[A.TAP_RX_CHAN_FILT], xf)          # chan_filt is the (expanded) input itself
    ea.close()
    eb.close()


# ---- 4. chunked streams ----------------------------------------------------------------------------------------------
def _capture(orc, npkt=90, seed=5, cfo_bins=0.07, snr_db=30.0):
    """(the capture of test_gpu_stream.py) bursts of packets of mixed sizes separated by silences, AWGN + CFO"""
    cfg = make_cfg("qpsk")
    rng = np.random.default_rng(seed)
    sizes = rng.integers(20, 1500, npkt)
    sizes[npkt // 3] = 4091
    pay = make_payloads(npkt, sizes, seed=seed)
    parts, k = [np.zeros(1500, np.complex64)], 0
    while k < npkt:
        n = int(rng.integers(1, 9))
        parts.append(orc.tx(cfg, pay[k:k + n]))
        parts.append(np.zeros(int(rng.integers(200, 60000)), np.complex64))
        k += n
    iq = np.concatenate(parts)
    psig = float(np.mean(np.abs(parts[1]) ** 2))
    orc.channel(iq, sigma=float(np.sqrt(psig / 10 ** (snr_db / 10))), cfo=cfo_bins * 2 * np.pi / cfg.fft_length, seed=77)
    return pay, iq


def test_feed_sc16_equals_one_shot(orc):
    pay, iq = _capture(orc)
    q = iqio.to_sc16(iq)
    opt = options.default_options(modulation="qpsk")
    d16 = ofdm.ofdm_demod(opt, iq_format="sc16")
    want = d16.work(q)
    good = [p for ok, p in want if ok]
    assert len(good) >= len(pay) * 0.6 and all(p in pay for p in good)
    assert ofdm.ofdm_demod(opt).work(iqio.from_sc16(q)) == want      # the float receiver on the expanded capture
    with pytest.raises(ValueError):
        d16.work(iq)                                                   # complex64 into an sc16 demodulator
    for chunking in ("131072", "50000", "random", "tiny-then-big", "one"):
        rng = np.random.default_rng(1)
        cuts, pos = [], 0
        while pos < len(q):
            if chunking == "random":
                n = int(rng.integers(1, 400000))
            elif chunking == "tiny-then-big":
                n = 1000 if pos < 20000 else 700000
            elif chunking == "one":
                n = len(q)
            else:
                n = int(chunking)
            cuts.append((pos, min(len(q), pos + n)))
            pos += n
        s = ofdm.ofdm_demod(opt, iq_format="sc16")
        got = []
        for a, b in cuts:
            got += s.feed(q[a:b])
            assert s._s_tail.dtype == np.int16                          # the carried tail stays 16-bit
        got += s.flush()
        assert got == want, chunking


# ---- 5. sensing ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("NS,tune,dwell,avg,rx_scale", [(64, 1, 6, 3, None), (256, 1, 6, 3, None), (4096, 1, 3, 2, None),
                                                        (256, 1, 6, 3, 1.0 / 32767.0), (4096, 1, 3, 2, 1.0 / 32767.0)])
def test_sense_sc16(orc, NS, tune, dwell, avg, rx_scale):
    """(rx_scale 1/32767: the sensor's load multiply is a real rounding, not an exponent shift)"""
    cfg = make_cfg("qpsk")
    q = iqio.to_sc16(loopback_stream(orc, cfg, make_payloads(24, 1026, seed=3), snr_db=30.0))
    xf = iqio.from_sc16(q, rx_scale)
    sc = config.make_sense_cfg(NS, tune, dwell, avg, 1, threshold=0.05)
    ea, eb = _eng(cfg, rx="sc16", rx_scale=rx_scale), _eng(cfg)

    def same(ra, rb):
        assert ra["msgs"].shape == rb["msgs"].shape and len(ra["hex"]) == len(rb["hex"]) >= 1
        assert np.array_equal(ra["msgs"], rb["msgs"]) and np.array_equal(ra["mean"], rb["mean"])
        assert np.array_equal(ra["bits"], rb["bits"]) and ra["hex"] == rb["hex"]

    ra, rb = ea.sense(sc, q), eb.sense(sc, xf)
    same(ra, rb)
    so = orc.sense(sc, xf)
    assert np.array_equal(ra["msgs"], so["msgs"]) and ra["hex"] == so["hex"]
    assert float(ra["msgs"].max()) > 0.0
    # fused into ofdm_rx
    for e in (ea, eb):
        e.set_rx_sense(sc)
    pa, pb = ea.rx(q), eb.rx(xf)
    assert pa == pb and sum(ok for ok, _ in pa) >= 20
    fa, fb = ea.rx_sense_result(len(q)), eb.rx_sense_result(len(q))
    same(fa, fb)
    same(fa, ra)
    ea.close()
    eb.close()


# ---- 6. transmit -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mod,N,occ,CP,plen,npkt,snr,cfo", CASES)
def test_tx_sc16_channel_off(mod, N, occ, CP, plen, npkt, snr, cfo):
    """ofdm_tx in sc16 mode stores to_sc16 of what it stores in float mode: the lean kernel, the tapped one (whose taps
    stay float and equal the float run's), the default scale, a saturating one (2^17) and 32767."""
    cfg = make_cfg(mod, N, occ, CP)
    e = engine.Engine(cfg=cfg)
    pay = make_payloads(npkt, plen)
    x = e.tx(pay)
    e.set_taps(A.TAP_TX_FREQ, A.TAP_TX_IFFT)
    assert np.array_equal(e.tx(pay), x)
    freq, ifft = e.tap(A.TAP_TX_FREQ), e.tap(A.TAP_TX_IFFT)
    for scale in (None, 2.0 ** 17, 32767.0):
        want = iqio.to_sc16(x, scale)
        if scale == 2.0 ** 17:
            assert int(np.max(want)) == 32767 and int(np.min(want)) == -32768      # it does saturate
        e.set_tx_iq_format("sc16", scale)
        e.set_taps()
        q = e.tx(pay)                                                              # LEAN kernel
        assert q.dtype == np.int16 and q.shape == (len(x), 2)
        assert np.array_equal(q, want), scale
        e.set_taps(A.TAP_TX_FREQ, A.TAP_TX_IFFT)
        assert np.array_equal(e.tx(pay), want), scale                              # tapped kernel
        assert np.array_equal(e.tap(A.TAP_TX_FREQ), freq) and np.array_equal(e.tap(A.TAP_TX_IFFT), ifft)
    e.set_tx_iq_format("fc32")
    e.set_taps()
    assert np.array_equal(e.tx(pay), x)
    e.close()


@pytest.mark.parametrize("cfo", [0.0, 0.05])
def test_tx_sc16_channel_on(cfo):
    """AWGN (+ carrier offset), noise-only lead-in and tail: the 16-bit run equals to_sc16 of the float run of the same
    handle within 1 LSB.  The float noise path uses hardware transcendentals; the margin covers only a difference in
    code generation between the two instantiations of the kernel.

    Measured on an MI355X (this test prints the figures): 0 of 906 498 parts differ, with and without the carrier
    offset -- the two instantiations' noise paths produce the same bits; the 1-LSB margin went unused."""
    N, CP = 512, 128
    cfg = make_cfg("qpsk")
    e = engine.Engine(cfg=cfg)
    pay = make_payloads(32, 1026, seed=8)
    e.set_channel(sigma=0.005, cfo=cfo * 2 * np.pi / N, lead=2 * N + 1, tail=(N + CP) + 2 * N)
    x = e.tx(pay)
    e.set_tx_iq_format("sc16")
    q = e.tx(pay)
    want = iqio.to_sc16(x)
    assert q.shape == want.shape
    d = np.abs(q.astype(np.int32) - want.astype(np.int32))
    print("tx sc16 channel on, cfo %g bins: %d of %d parts differ from to_sc16(float run), max %d LSB" % (
        cfo, int(np.count_nonzero(d)), d.size, int(d.max())))
    assert int(d.max()) <= 1
    # lead-in and tail are noise, not silence
    assert np.any(q[:2 * N + 1] != 0) and np.any(q[-2 * N:] != 0)
    # and the 16-bit stream decodes
    e.set_rx_iq_format("sc16")
    good = [p for ok, p in e.rx(q) if ok]
    assert len(good) >= len(pay) - 1 and all(p in pay for p in good)
    e.close()


@pytest.mark.parametrize("what", ["inf", "nan"])
def test_tx_sc16_non_finite(what):
    """The device quantiser's NaN -> 0 and +-inf -> saturation paths: an infinite noise amplitude puts +-inf, a NaN
    carrier offset NaN into every sample of the float run; the 16-bit run of the same handle stores to_sc16 of them."""
    N, CP = 512, 128
    e = engine.Engine(cfg=make_cfg("qpsk"))
    pay = make_payloads(4, 300, seed=12)
    if what == "inf":
        e.set_channel(sigma=float("inf"), lead=N + 1, tail=N)
    else:
        e.set_channel(sigma=0.001, cfo=float("nan"), lead=N + 1, tail=N)
    x = e.tx(pay)
    parts = x.view(np.float32)
    bad = ~np.isfinite(parts)
    if what == "inf":
        assert np.isinf(parts).any() and (parts[np.isinf(parts)] > 0).any() and (parts[np.isinf(parts)] < 0).any()
    else:
        assert np.isnan(parts).any()
    e.set_tx_iq_format("sc16")
    q = e.tx(pay)
    want = iqio.to_sc16(x)
    assert q.shape == want.shape
    qf, wf = q.reshape(-1), want.reshape(-1)
    assert np.array_equal(qf[bad], wf[bad])                         # NaN -> 0, +inf -> 32767, -inf -> -32768: exact
    if what == "inf":
        assert set(np.unique(wf[np.isinf(parts)]).tolist()) == {-32768, 32767}
    else:
        assert not wf[np.isnan(parts)].any()
    assert int(np.max(np.abs(qf.astype(np.int32) - wf.astype(np.int32)))) <= 1      # (the channel-on bound elsewhere)
    e.close()


# ---- 7. device loopback entirely in sc16 -----------------------------------------------------------------------------
def test_device_loopback_sc16():
    import torch
    dev = torch.device("cuda:0")
    N, CP, npkt = 512, 128, 256
    pay = make_payloads(npkt, 1026, seed=2)
    blob, offs, lens = pack_payloads(pay)
    sigma = float(np.sqrt(198.0 / 512.0 * 0.25 ** 2 * 0.99985 ** 2 / 1000.0))     # 30 dB (test_gpu_properties)
    d_blob = torch.from_numpy(blob.copy()).to(dev)
    d_pay = torch.zeros(npkt * 1100, dtype=torch.uint8, device=dev)

    def unpack(n, off, ln, ok):
        out = d_pay.cpu().numpy()
        return [(bool(ok[i]), out[int(off[i]):int(off[i]) + int(ln[i])].tobytes()) for i in range(n)]

    def fresh():
        e = engine.Engine(cfg=make_cfg("qpsk", device_ptrs=True))
        e.set_channel(sigma=sigma, lead=2 * N, tail=(N + CP) + 2 * N)
        return e

    e16 = fresh()
    e16.set_tx_iq_format("sc16")
    e16.set_rx_iq_format("sc16")
    _, nsamp = e16.tx_frame_count(lens)
    d_q = torch.zeros((nsamp, 2), dtype=torch.int16, device=dev)
    n = e16.tx_device(d_blob.data_ptr(), offs, lens, d_q.data_ptr(), nsamp, wait=False)
    got16 = unpack(*e16.rx_device(d_q.data_ptr(), n, d_pay.data_ptr(), d_pay.numel(), npkt + 16))
    assert n == nsamp
    # the float engine on the expanded buffer recovers the same packets
    ef = fresh()
    xf = iqio.from_sc16(d_q.cpu().numpy())
    d_x = torch.from_numpy(xf.view(np.float32).copy()).to(dev)
    gotf = unpack(*ef.rx_device(d_x.data_ptr(), n, d_pay.data_ptr(), d_pay.numel(), npkt + 16))
    assert got16 == gotf
    # the float loopback of the same seeds
    d_xf = torch.zeros(nsamp * 2, dtype=torch.float32, device=dev)
    nf = ef.tx_device(d_blob.data_ptr(), offs, lens, d_xf.data_ptr(), nsamp, wait=False)
    loopf = unpack(*ef.rx_device(d_xf.data_ptr(), nf, d_pay.data_ptr(), d_pay.numel(), npkt + 16))
    ok16, okf = sum(ok for ok, _ in got16), sum(ok for ok, _ in loopf)
    print("device loopback, %d packets at 30 dB: CRC ok sc16 %d, float %d" % (npkt, ok16, okf))
    assert ok16 >= okf - 1 and okf >= npkt - 2
    assert all(p in pay for ok, p in got16 if ok)
    e16.close()
    ef.close()


# ---- 8. pipelining ---------------------------------------------------------------------------------------------------
def test_pipelined_batches_sc16():
    """ofdm_rx_submit + ofdm_tx_async over ONE int16 buffer, a different payload set per batch: every batch returns its
    own payloads, exactly as when the calls are made one after the other."""
    import torch
    dev = torch.device("cuda:0")
    batches = []
    for b in range(5):
        pay = make_payloads(96, 1026, seed=140 + b)
        blob, offs, lens = pack_payloads(pay)
        batches.append((pay, torch.from_numpy(blob.copy()).to(dev), offs, lens))
    e = engine.Engine(cfg=make_cfg("qpsk", device_ptrs=True))
    e.set_tx_iq_format("sc16")
    e.set_rx_iq_format("sc16")
    e.set_channel(sigma=0.002, lead=1024, tail=1664)
    _, nsamp = e.tx_frame_count(batches[0][3])
    d_q = torch.zeros((nsamp, 2), dtype=torch.int16, device=dev)
    d_pay = torch.empty(96 * 1100, dtype=torch.uint8, device=dev)

    def unpack(npk, off, ln, ok):
        out = d_pay.cpu().numpy()
        return [(bool(ok[i]), out[int(off[i]):int(off[i]) + int(ln[i])].tobytes()) for i in range(npk)]

    seq, qs = [], []
    for pay, d_blob, offs, lens in batches:
        n = e.tx_device(d_blob.data_ptr(), offs, lens, d_q.data_ptr(), nsamp)
        qs.append(d_q.clone())
        seq.append(unpack(*e.rx_device(d_q.data_ptr(), n, d_pay.data_ptr(), d_pay.numel(), 200)))
        assert [p for ok, p in seq[-1] if ok] == pay
    e.prof_enable(True)
    pip = []
    n = e.tx_device(batches[0][1].data_ptr(), batches[0][2], batches[0][3], d_q.data_ptr(), nsamp, wait=False)
    for i in range(5):
        e.rx_submit_device(d_q.data_ptr(), n)
        if i == 0:
            with pytest.raises(ValueError):                   # the receive format is pinned while a stage is submitted
                e.set_rx_iq_format("fc32")
        if i + 1 < 5:
            _, d_blob, offs, lens = batches[i + 1]
            n_next = e.tx_device(d_blob.data_ptr(), offs, lens, d_q.data_ptr(), nsamp, wait=False)
        pip.append(unpack(*e.rx_device(d_q.data_ptr(), n, d_pay.data_ptr(), d_pay.numel(), 200)))
        n = n_next
    e.wait()
    assert pip == seq
    assert torch.equal(d_q, qs[-1])
    prof = e.prof()
    assert prof["k_tx_mod"][1] == 5 and prof["k_rx_demod"][1] == 5 and prof["k_chan_filter"][1] == 5
    # with a fused sensor the receiver reads the buffer to the end of ofdm_rx: a transmit into it is refused, as in
    # float mode; into another int16 buffer it is accepted
    e.set_rx_sense(config.make_sense_cfg(256, 1, 6, 3, 1, threshold=0.05))
    pay, d_blob, offs, lens = batches[0]
    n = e.tx_device(d_blob.data_ptr(), offs, lens, d_q.data_ptr(), nsamp)
    e.rx_submit_device(d_q.data_ptr(), n)
    with pytest.raises(ValueError):
        e.tx_device(batches[1][1].data_ptr(), batches[1][2], batches[1][3], d_q.data_ptr(), nsamp, wait=False)
    d_q2 = torch.zeros_like(d_q)
    e.tx_device(batches[1][1].data_ptr(), batches[1][2], batches[1][3], d_q2.data_ptr(), nsamp, wait=False)
    got = unpack(*e.rx_device(d_q.data_ptr(), n, d_pay.data_ptr(), d_pay.numel(), 200))
    e.wait()
    assert [p for ok, p in got if ok] == pay
    e.close()


# ---- 9. the defaults run what they always ran ------------------------------------------------------------------------
def test_default_formats_change_nothing(orc):
    mod, N, occ, CP, plen, npkt, snr, cfo = CASES[0]
    cfg = make_cfg(mod, N, occ, CP)
    pay = make_payloads(npkt, plen)
    x = loopback_stream(orc, cfg, pay, snr_db=snr, cfo_bins=cfo)
    e0, e1 = _eng(cfg), _eng(cfg)
    # e1 goes through the setters: to 16 bits and back, then the defaults by name
    e1.set_rx_iq_format("sc16", 1.0 / 32767.0)
    e1.set_tx_iq_format("sc16", 32767.0)
    e1.set_rx_iq_format("fc32")
    e1.set_tx_iq_format("fc32")
    res = []
    for e in (e0, e1):
        e.set_taps(*ARRAY_TAPS)
        e.prof_enable(True)
        e.prof_reset()
        iq = e.tx(pay)
        pk = e.rx(x)
        res.append((iq, pk, dict(e.last_stats), _taps(e), {k: v[1] for k, v in e.prof().items()}))
    assert np.array_equal(res[0][0], res[1][0]) and res[0][0].dtype == np.complex64
    assert res[0][1] == res[1][1] and res[0][2] == res[1][2]
    _same_taps(res[0][3], res[1][3])
    assert res[0][4] == res[1][4]                                   # the same launch counts, kernel by kernel
    assert res[0][4]["k_chan_filter"] == 1 and res[0][4]["k_tx_mod"] == 1 and res[0][4]["k_channel"] == 0
    e0.close()
    e1.close()


# ---- 10. errors ------------------------------------------------------------------------------------------------------
def test_error_returns(monkeypatch):
    cfg = make_cfg("qpsk")
    e = engine.Engine(cfg=cfg)
    lib, h = e._lib, e._h
    for fn in (lib.ofdm_set_rx_iq_format, lib.ofdm_set_tx_iq_format):
        assert fn(h, 2, 1.0) == A.OFDM_E_INVAL and fn(h, -1, 1.0) == A.OFDM_E_INVAL          # unknown format
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            assert fn(h, A.OFDM_IQ_SC16, bad) == A.OFDM_E_INVAL                               # scale
        assert fn(h, A.OFDM_IQ_FC32, float("nan")) == A.OFDM_OK                               # ignored with fc32
        assert fn(h, A.OFDM_IQ_SC16, 0.5) == A.OFDM_OK and fn(h, A.OFDM_IQ_FC32, 0.0) == A.OFDM_OK
    with pytest.raises(ValueError):
        e.set_rx_iq_format("sc8")
    with pytest.raises(ValueError):
        e.set_tx_iq_format("sc16", -3.0)
    # a dtype that does not match the format raises instead of being reinterpreted
    x = np.zeros(4096, np.complex64)
    q = np.zeros((4096, 2), np.int16)
    with pytest.raises(ValueError):
        e.rx(q)
    sc = config.make_sense_cfg(256, 1, 6, 3, 1, threshold=0.05)
    with pytest.raises(ValueError):
        e.sense(sc, q)
    e.set_rx_iq_format("sc16")
    with pytest.raises(ValueError):
        e.rx(x)
    with pytest.raises(ValueError):
        e.rx(x.view(np.float32))
    with pytest.raises(ValueError):
        e.sense(sc, x)
    assert e.rx(q) == [] and e.rx(q.reshape(-1)) == []              # flat 2n accepted
    # int16 handed to the float-only standalone channel
    with pytest.raises(ValueError):
        e.channel(q, sigma=0.001)
    # sc16 receive and the opt-in fused front end exclude each other
    e.set_rx_iq_format("fc32")
    monkeypatch.setenv("OFDM_FRONT", "1")
    with pytest.raises(ValueError):
        e.set_rx_iq_format("sc16")
    assert e.rx_iq_format == "fc32"
    monkeypatch.delenv("OFDM_FRONT")
    e.set_rx_iq_format("sc16")
    monkeypatch.setenv("OFDM_FRONT", "1")                           # switched on behind the setter's back: refused at the call
    with pytest.raises(ValueError):
        e.rx(q)
    monkeypatch.delenv("OFDM_FRONT")
    assert e.rx(q) == []
    e.close()


def test_sc16_pointers_must_be_dword_aligned():
    """A 16-bit sample is moved as one dword: a pointer that is not 4-byte aligned is refused (OFDM_E_INVAL) by
    ofdm_rx, ofdm_rx_submit, ofdm_sense and ofdm_tx before anything is queued; in float mode nothing is asked."""
    import torch
    dev = torch.device("cuda:0")
    e = engine.Engine(cfg=make_cfg("qpsk", device_ptrs=True))
    e.set_rx_iq_format("sc16")
    e.set_tx_iq_format("sc16")
    pay = make_payloads(2, 300, seed=1)
    blob, offs, lens = pack_payloads(pay)
    d_blob = torch.from_numpy(blob.copy()).to(dev)
    e.set_channel(sigma=0.002, lead=1024, tail=1664)
    _, nsamp = e.tx_frame_count(lens)
    d_q = torch.zeros((nsamp + 8, 2), dtype=torch.int16, device=dev)
    d_pay = torch.zeros(4096, dtype=torch.uint8, device=dev)
    odd = d_q.data_ptr() + 2
    sc = config.make_sense_cfg(256, 1, 6, 3, 1, threshold=0.05)
    with pytest.raises(ValueError):
        e.tx_device(d_blob.data_ptr(), offs, lens, odd, nsamp)
    with pytest.raises(ValueError):
        e.rx_device(odd, nsamp, d_pay.data_ptr(), d_pay.numel(), 8)
    with pytest.raises(ValueError):
        e.rx_submit_device(odd, nsamp)
    with pytest.raises(ValueError):
        e.sense(sc, odd, nsamp)
    assert not bool(d_q.any())                                      # nothing was written
    n = e.tx_device(d_blob.data_ptr(), offs, lens, d_q.data_ptr() + 4, nsamp)       # one sample further on: fine
    npk, off, ln, ok = e.rx_device(d_q.data_ptr() + 4, n, d_pay.data_ptr(), d_pay.numel(), 8)
    out = d_pay.cpu().numpy()
    assert [out[int(off[i]):int(off[i]) + int(ln[i])].tobytes() for i in range(npk) if ok[i]] == pay
    e.close()
