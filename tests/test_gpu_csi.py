"""Per-subcarrier channel state (ofdm_set_rx_csi / ofdm_rx_csi / ofdm_rx_csi_summary) on the GPU.

The rows are checked against a NumPy model over the stage taps (TAP_RX_FFT for the preamble, TAP_RX_ACQ for the
equaliser, TAP_RX_SINK for the slicer inputs) and against the link-quality record of the same packet.  On top of that:
CSI changes nothing else the receiver delivers, the gain follows a two-path channel, a narrowband interferer is found and
mapped around end to end, chunked streams give the rows of one call, the device summary equals a float64 reduction of
the rows, and the edge cases of the C ABI."""
import ctypes as C

import numpy as np
import pytest

from helpers import loopback_stream, make_cfg, make_payloads
from ofdm_uhd_amd import _abi, config, csi, engine, ofdm, options
from test_gpu_link_quality import CASES, _stream_capture

pytestmark = pytest.mark.gpu

KEYS = ("eq", "pre_power", "err", "ref")


def _c(arr, n):
    return np.array([complex(v.re, v.im) for v in arr[:n]], np.complex64)


def _smap(cfg):
    return config.carrier_map(cfg.occupied_tones, cfg.occupied_tones, cfg.carrier_map.decode("ascii") or "FE7F")


def _bits_equal(a, b):
    return all(a[k].shape == b[k].shape and np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in KEYS)


def _sum_equal(a, b):
    return a["npkt"] == b["npkt"] and all(np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64))
                                          for k in ("pre_power", "err", "ref", "inv_gain")) and \
        np.array_equal(a["ninv"], b["ninv"])


def _model_check(cfg, eng, recs, rows):
    N, occ, CP = cfg.fft_length, cfg.occupied_tones, cfg.cp_length
    zl = (N - occ + 1) // 2
    ks = _c(cfg.known_symbol, occ)
    pil = ks != 0
    cst = _c(cfg.constellation, cfg.arity)
    smap = np.asarray(_smap(cfg))
    fft, acq, sink = eng.tap(_abi.TAP_RX_FFT), eng.tap(_abi.TAP_RX_ACQ), eng.tap(_abi.TAP_RX_SINK)
    dem = eng.tap(_abi.TAP_RX_DEMAPPED).astype(bool)
    sink_row = np.cumsum(dem) - 1
    assert len(recs) == len(rows["eq"]) >= 1
    for p, r in enumerate(recs):
        fs, ns, coarse = int(r["first_symbol"]), int(r["nsym"]), int(r["coarse"])
        idx = np.arange(occ) + zl + coarse
        Y = np.where((idx >= 0) & (idx < N), fft[fs][np.clip(idx, 0, N - 1)], 0).astype(np.complex64)
        np.testing.assert_allclose(rows["pre_power"][p], Y.real * Y.real + Y.imag * Y.imag, rtol=1e-5)
        # the equaliser: ks / (comp Y) on even occupied indices, neighbour means on odd ones, the copy at the end
        a = np.float32(-2 * np.pi * coarse * CP / N)
        comp = np.complex64(np.cos(a) + 1j * np.sin(a))
        h = np.zeros(occ, np.complex64)
        h[0::2] = ks[0::2] / (comp * Y[0::2])
        h[1:occ - 1:2] = (h[0:occ - 2:2] + h[2::2][:len(h[1:occ - 1:2])]) / np.float32(2)
        if occ % 2 == 0:
            h[occ - 1] = h[occ - 2]
        eq = rows["eq"][p]
        np.testing.assert_allclose(eq, h, rtol=1e-5, atol=1e-6 * np.abs(h).max())
        want_acq = acq[fs][:occ]
        np.testing.assert_allclose(eq * comp * Y, want_acq, rtol=1e-5, atol=1e-5 * np.abs(want_acq).max())
        # decision energies per carrier: sink-map column c is occupied carrier smap[c]
        s = sink[sink_row[fs + 1:fs + 1 + ns], :len(smap)].astype(np.complex64)
        d = (s.real[..., None] - cst.real) ** 2 + (s.imag[..., None] - cst.imag) ** 2
        dec = cst[np.argmin(d, axis=-1)]
        e = np.zeros(occ)
        f = np.zeros(occ)
        e[smap] = np.sum(np.abs(s.astype(np.complex128) - dec) ** 2, axis=0)
        f[smap] = np.sum(np.abs(dec.astype(np.complex128)) ** 2, axis=0)
        np.testing.assert_allclose(rows["err"][p], e, rtol=1e-5, atol=1e-7 * max(e.max(), 1e-30))
        np.testing.assert_allclose(rows["ref"][p], f, rtol=1e-5)
        off = np.setdiff1d(np.arange(occ), smap)
        assert not rows["err"][p][off].any() and not rows["ref"][p][off].any()
        # the link-quality record of the same packet is the sum of the row
        np.testing.assert_allclose(rows["err"][p].astype(np.float64).sum(), r["err_energy"], rtol=1e-4)
        np.testing.assert_allclose(rows["ref"][p].astype(np.float64).sum(), r["ref_energy"], rtol=1e-4)
        pp = rows["pre_power"][p].astype(np.float64)
        np.testing.assert_allclose(pp[pil].sum(), r["pilot_power"] * pil.sum(), rtol=1e-4)
        np.testing.assert_allclose(pp[~pil].sum(), r["null_power"] * (~pil).sum(), rtol=1e-4)


def _instrumented(cfg):
    eng = engine.Engine(cfg=cfg)
    eng.set_taps(_abi.TAP_RX_FFT, _abi.TAP_RX_ACQ, _abi.TAP_RX_SINK, _abi.TAP_RX_DEMAPPED)
    eng.set_rx_quality(True)
    eng.set_rx_csi(True)
    return eng


@pytest.mark.parametrize("mod,N,occ,CP,plen,npkt,snr,cfo", CASES)
def test_csi_against_model(orc, mod, N, occ, CP, plen, npkt, snr, cfo):
    cfg = make_cfg(mod, N, occ, CP)
    eng = _instrumented(cfg)
    x = loopback_stream(orc, cfg, make_payloads(npkt, plen), snr_db=snr, cfo_bins=cfo)
    pk = eng.rx(x)
    assert len(pk) >= 1
    _model_check(cfg, eng, eng.rx_quality(), eng.rx_csi())
    eng.close()


@pytest.mark.parametrize("which", [0, 4, 9])
def test_csi_changes_nothing_else(orc, which):
    mod, N, occ, CP, plen, npkt, snr, cfo = CASES[which]
    cfg = make_cfg(mod, N, occ, CP)
    eng = engine.Engine(cfg=cfg)
    eng.set_rx_quality(True)
    x = loopback_stream(orc, cfg, make_payloads(npkt, plen), snr_db=snr, cfo_bins=cfo)
    pk0, pos0, st0, q0 = eng.rx(x), eng.rx_packet_pos(), dict(eng.last_stats), eng.rx_quality()
    with pytest.raises(ValueError):
        eng.rx_csi()                                        # that call ran without CSI
    eng.set_rx_csi(True)
    pk1, pos1, st1, q1 = eng.rx(x), eng.rx_packet_pos(), dict(eng.last_stats), eng.rx_quality()
    r1, s1 = eng.rx_csi(), eng.rx_csi_summary(False)
    pk2, r2, s2 = eng.rx(x), eng.rx_csi(), eng.rx_csi_summary(False)
    assert pk1 == pk0 == pk2 and pos1.tolist() == pos0.tolist() and st1 == st0
    assert all(np.array_equal(q1[f], q0[f]) for f in engine.QUALITY_DTYPE.names)
    assert len(r1["eq"]) == len(pk1) and _bits_equal(r1, r2) and _sum_equal(s1, s2)
    assert _sum_equal(s1, eng.rx_csi_summary(False))
    eng.set_rx_csi(False)
    assert eng.rx(x) == pk0 and dict(eng.last_stats) == st0
    n = C.c_int(-1)
    assert _abi.load().ofdm_rx_csi(eng._h, 0, 0, None, None, None, None, C.byref(n)) == _abi.OFDM_E_INVAL
    eng.close()


def _awgn(x, snr_db, psig, seed):
    rng = np.random.default_rng(seed)
    s = np.sqrt(psig / 10 ** (snr_db / 10.0) / 2)
    return (x + s * (rng.standard_normal(len(x)) + 1j * rng.standard_normal(len(x)))).astype(np.complex64)


def test_gain_follows_a_two_path_channel(orc):
    N, occ, CP = 512, 200, 128
    cfg = make_cfg("qpsk", N, occ, CP)
    pay = make_payloads(12, 800, seed=31)
    x = orc.tx(cfg, pay, lead=2 * N, tail=3 * N)
    psig = float(np.mean(np.abs(x[2 * N:-3 * N]) ** 2))
    g = 0.5 * np.exp(0.7j)
    y = x.astype(np.complex128)
    y[4:] += g * x[:-4]
    y = _awgn(y, 30.0, psig, 7)
    eng = engine.Engine(cfg=cfg)
    eng.set_rx_csi(True)
    pk = eng.rx(y)
    assert sum(ok for ok, _ in pk) >= 10
    rep = csi.carrier_report(eng.rx_csi_summary(), cfg)
    zl = config.zeros_on_left(N, occ)
    k = np.arange(occ) + zl - N // 2                         # frequency of occupied carrier i, in subcarrier spacings
    H = 10 * np.log10(np.abs(1 + g * np.exp(-2j * np.pi * k * 4 / N)) ** 2)
    got = rep["gain_db"]
    assert np.isfinite(got).all()
    dev = (got - got.mean()) - (H - H.mean())
    assert np.abs(dev).max() <= 1.0, np.abs(dev).max()
    eng.close()


def _interferer(n, N, zl, i0, width, power, seed):
    """Gaussian noise confined to occupied carriers [i0, i0 + width) (brick wall in a transform of the whole capture)."""
    rng = np.random.default_rng(seed)
    w = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    W = np.fft.fft(w)
    f = np.fft.fftfreq(n)
    lo, hi = (i0 + zl - N // 2 - 0.5) / N, (i0 + width - 1 + zl - N // 2 + 0.5) / N
    W[(f < lo) | (f > hi)] = 0
    v = np.fft.ifft(W)
    return v * np.sqrt(power / np.mean(np.abs(v) ** 2))


def _jammed(orc, cfg, pay, i0, seed):
    N = cfg.fft_length
    x = orc.tx(cfg, pay, lead=2 * N, tail=3 * N)
    psig = float(np.mean(np.abs(x[2 * N:-3 * N]) ** 2))
    per_carrier = psig / len(_smap(cfg))
    zl = config.zeros_on_left(N, cfg.occupied_tones)
    # 3 dB SIR per jammed carrier: at 0 dB the timing detector (the oracle's as well) loses about a third of the flags
    y = x + _interferer(len(x), N, zl, i0, 8, 0.5 * 8 * per_carrier, seed)
    return _awgn(y, 30.0, psig, seed + 1)


def test_narrowband_interferer_end_to_end(orc):
    N, occ, CP = 512, 200, 128
    i0 = 120                                                # jammed occupied carriers 120..127 (past the header's)
    jam = np.arange(i0, i0 + 8)
    cfg = make_cfg("qpsk", N, occ, CP)
    pay = make_payloads(40, 600, seed=8)
    eng = engine.Engine(cfg=cfg)
    eng.set_rx_csi(True)
    pk = eng.rx(_jammed(orc, cfg, pay, i0, 100))
    assert len(pk) >= 10                                    # (the report counts CRC failures too)
    assert sum(ok for ok, _ in pk) < 0.5 * len(pay), sum(ok for ok, _ in pk)   # the full map does not get through
    rep = csi.carrier_report(eng.rx_csi_summary(crc_ok_only=False), cfg)
    far = np.array([i for i in range(occ) if i < i0 - 4 or i > i0 + 7 + 4])
    med = np.median(rep["snr_preamble_db"][far])
    assert (rep["snr_preamble_db"][jam] <= med - 10).all(), (rep["snr_preamble_db"][jam], med)
    hx = csi.suggest_carrier_map(rep, cfg, 10.0)
    keep = set(config.carrier_map(occ, occ, hx, sink=True))
    assert not keep & set(jam.tolist())
    cur_far = [i for i in far if i in set(_smap(cfg))]
    assert len(keep & set(cur_far)) >= 0.9 * len(cur_far), (len(keep & set(cur_far)), len(cur_far))
    # the suggested map on both ends
    cfg2 = make_cfg("qpsk", N, occ, CP, carriers=hx)
    eng.set_carrier_map(hx)
    pk2 = eng.rx(_jammed(orc, cfg2, pay, i0, 200))
    assert sum(ok for ok, _ in pk2) >= 0.95 * len(pay), (len(pk2), sum(ok for ok, _ in pk2), hx)
    eng.close()


def test_stream_rows_equal_one_call(orc):
    iq = _stream_capture(orc)
    d = ofdm.ofdm_demod(options.default_options(modulation="qpsk"), csi=True)
    want_pk = d.work(iq)
    want = {k: v.copy() for k, v in d.last_csi.items()}
    want_rep = d.carrier_report()
    summ = d.engine().rx_csi_summary()
    assert len(want["eq"]) == len(want_pk) >= 15
    one = csi.carrier_report(summ, d.engine().cfg)
    for k in want_rep:
        np.testing.assert_allclose(want_rep[k], one[k], rtol=1e-12, atol=1e-12)
    for chunk in (131072, 50000, 300007):
        s = ofdm.ofdm_demod(options.default_options(modulation="qpsk"), csi=True)
        got_pk, got = [], []
        for a in range(0, len(iq), chunk):
            got_pk += s.feed(iq[a:a + chunk])
            got.append(s.last_csi)
            assert len(got[-1]["eq"]) == len(got_pk) - sum(len(g["eq"]) for g in got[:-1])
        got_pk += s.flush()
        got.append(s.last_csi)
        rows = {k: np.concatenate([g[k] for g in got]) for k in KEYS}
        assert got_pk == want_pk, chunk
        assert _bits_equal(rows, want), chunk
        rep = s.carrier_report()
        for k in want_rep:
            np.testing.assert_array_equal(rep[k], want_rep[k])


def test_summary_equals_float64_reduction(orc):
    cfg = make_cfg("qpsk")
    pay = make_payloads(300, 60, seed=12)
    x = loopback_stream(orc, cfg, pay, snr_db=30.0)
    eng = engine.Engine(cfg=cfg)
    eng.set_rx_csi(True)
    pk = eng.rx(x)
    assert len(pk) >= 250                                   # more than two summation chunks of 128 packets
    rows = eng.rx_csi()
    ok = np.array([o for o, _ in pk], bool)
    for only in (False, True):
        s = eng.rx_csi_summary(crc_ok_only=only)
        sel = ok if only else np.ones(len(pk), bool)
        assert s["npkt"] == int(sel.sum())
        for k in ("pre_power", "err", "ref"):
            np.testing.assert_allclose(s[k], rows[k][sel].astype(np.float64).sum(axis=0), rtol=1e-12)
        eq = rows["eq"][sel].astype(np.complex128)
        m = np.abs(eq) ** 2
        good = np.isfinite(eq.real) & np.isfinite(eq.imag) & (m != 0)
        np.testing.assert_allclose(s["inv_gain"], np.where(good, 1.0 / np.where(good, m, 1.0), 0).sum(axis=0), rtol=1e-12)
        assert np.array_equal(s["ninv"], good.sum(axis=0))
        assert _sum_equal(s, eng.rx_csi_summary(crc_ok_only=only))
    eng.close()


def test_csi_edges(orc):
    cfg = make_cfg("qpsk")
    eng = engine.Engine(cfg=cfg)
    lib = _abi.load()
    eng.set_rx_csi(True)
    x = loopback_stream(orc, cfg, make_payloads(5, 600, seed=2), snr_db=30.0)
    pk = eng.rx(x)
    rows = eng.rx_csi()
    assert len(rows["eq"]) == len(pk) == 5
    n = C.c_int(-1)
    buf = np.zeros((8, cfg.occupied_tones), np.float32)
    p = buf.ctypes.data_as(C.c_void_p)
    assert lib.ofdm_rx_csi(eng._h, 0, 0, None, None, None, None, C.byref(n)) == _abi.OFDM_OK and n.value == 5
    assert lib.ofdm_rx_csi(eng._h, 3, 3, None, p, None, None, C.byref(n)) == _abi.OFDM_E_INVAL
    assert lib.ofdm_rx_csi(eng._h, -1, 1, None, p, None, None, C.byref(n)) == _abi.OFDM_E_INVAL
    assert lib.ofdm_rx_csi(eng._h, 0, -1, None, p, None, None, C.byref(n)) == _abi.OFDM_E_INVAL
    assert lib.ofdm_rx_csi(eng._h, 0, 1, None, None, None, None, None) == _abi.OFDM_E_INVAL
    part = eng.rx_csi(first=2, count=2)
    assert all(np.array_equal(part[k].view(np.uint32), rows[k][2:4].view(np.uint32)) for k in KEYS)
    # a call that ran out of packet slots leaves no rows
    with pytest.raises(engine.EngineError):
        eng.rx(x, max_pkts=2)
    assert len(eng.rx_csi()["eq"]) == 0 and eng.rx_csi_summary()["npkt"] == 0
    # a capture without packets, an empty capture: no rows, an empty summary
    rng = np.random.default_rng(5)
    noise = (0.01 * (rng.standard_normal(30000) + 1j * rng.standard_normal(30000))).astype(np.complex64)
    for cap in (noise, np.zeros(0, np.complex64)):
        assert eng.rx(cap) == [] and len(eng.rx_csi()["eq"]) == 0
        s = eng.rx_csi_summary(False)
        assert s["npkt"] == 0 and not s["pre_power"].any() and not s["ninv"].any()
    eng.close()
    # SYNC "fixed"
    N, CP = 512, 128
    pay = make_payloads(6, 500, seed=21)
    nsym = len(orc.tx(make_cfg("qpsk", N, 200, CP), pay[:1])) // (N + CP)
    opt = options.default_options(modulation="qpsk", fft_length=N, occupied_tones=200, cp_length=CP, sync="fixed",
                                  sync_nsymbols=nsym, sync_freq_offset=0.0)
    fcfg = config.make_cfg(opt)
    feng = _instrumented(fcfg)
    fpk = feng.rx(loopback_stream(orc, fcfg, pay, snr_db=30.0, lead=0, tail=700))
    assert [q for ok, q in fpk if ok] == pay
    _model_check(fcfg, feng, feng.rx_quality(), feng.rx_csi())
    feng.close()
    # device pointers: the same rows and summary
    import torch
    heng = engine.Engine(cfg=cfg)
    heng.set_rx_csi(True)
    heng.rx(x)
    hrows, hsum = heng.rx_csi(), heng.rx_csi_summary(False)
    heng.close()
    dev = engine.Engine(cfg=make_cfg("qpsk", device_ptrs=True))
    dev.set_rx_csi(True)
    xd = torch.from_numpy(x.view(np.float32).copy()).cuda()
    cap = len(x) + 4096
    payd = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    npk, off, ln, okd = dev.rx_device(xd.data_ptr(), len(x), payd.data_ptr(), cap, 64)
    torch.cuda.synchronize()
    assert npk == 5
    assert _bits_equal(dev.rx_csi(), hrows) and _sum_equal(dev.rx_csi_summary(False), hsum)
    dev.close()
    xd.zero_()
    payd.zero_()
    torch.cuda.synchronize()
    del xd, payd
    torch.cuda.empty_cache()
