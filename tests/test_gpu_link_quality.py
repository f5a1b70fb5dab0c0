"""Per-packet link quality (ofdm_set_rx_quality / ofdm_rx_quality) on the GPU.

The reference for the figures is a NumPy model over the stage taps the parity tests hold bit-identical to the oracle:
the preamble row of TAP_RX_FFT gives the pilot / null powers, the rows of TAP_RX_SINK the slicer's inputs.  On top of
that: link quality changes nothing else the receiver delivers, its estimates follow the synthetic channel, chunked
streams give the records of one call, and the edge cases of the C ABI."""
import ctypes as C

import numpy as np
import pytest

from helpers import loopback_stream, make_cfg, make_payloads
from ofdm_uhd_amd import _abi, config, engine, ofdm, options

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


def _c(arr, n):
    return np.array([complex(v.re, v.im) for v in arr[:n]], np.complex64)


def _nmap(cfg):
    return len(config.carrier_map(cfg.occupied_tones, cfg.occupied_tones, cfg.carrier_map.decode("ascii") or "FE7F"))


def _same(a, b):
    """Two record arrays equal field by field (the struct's tail padding is not part of a record)."""
    return len(a) == len(b) and all(np.array_equal(a[f], b[f]) for f in engine.QUALITY_DTYPE.names)


def _model_check(cfg, eng, pk, recs):
    """Every record against the NumPy model of its definition (include/ofdm_hip.h)."""
    N, occ = cfg.fft_length, cfg.occupied_tones
    zl = (N - occ + 1) // 2
    ks = _c(cfg.known_symbol, occ)
    pil, nul = ks != 0, ks == 0
    cst = _c(cfg.constellation, cfg.arity)
    nmap = _nmap(cfg)
    fft, sink = eng.tap(_abi.TAP_RX_FFT), eng.tap(_abi.TAP_RX_SINK)
    dem = eng.tap(_abi.TAP_RX_DEMAPPED).astype(bool)
    sink_row = np.cumsum(dem) - 1
    assert len(recs) == len(pk)
    assert recs["flag"].tolist() == eng.rx_packet_pos().tolist()
    used = np.zeros(len(dem), bool)
    for r in recs:
        fs, ns = int(r["first_symbol"]), int(r["nsym"])
        assert ns >= 1 and int(r["ncarriers"]) == ns * nmap
        # the preamble opens the chain (not demapped); the packet's symbols follow it, every one demapped, none shared
        assert not dem[fs] and dem[fs + 1:fs + 1 + ns].all() and fs + 1 + ns <= len(dem)
        assert not used[fs + 1:fs + 1 + ns].any()
        used[fs + 1:fs + 1 + ns] = True
        # pilot / null bins of the preamble, read where frame acquisition reads them
        idx = np.arange(occ) + zl + int(r["coarse"])
        ok = (idx >= 0) & (idx < N)
        Y = np.where(ok, fft[fs][np.clip(idx, 0, N - 1)], 0).astype(np.complex128)
        p2 = np.abs(Y) ** 2
        np.testing.assert_allclose(r["pilot_power"], p2[pil].mean(), rtol=1e-4)
        np.testing.assert_allclose(r["null_power"], p2[nul].mean(), rtol=1e-4)
        # decision energies: nearest constellation point of every demapped carrier (float32 distances, first minimum,
        # as the frame sink's slicer)
        s = sink[sink_row[fs + 1:fs + 1 + ns], :nmap].reshape(-1)
        d = (s.real[:, None] - cst.real[None, :]) ** 2 + (s.imag[:, None] - cst.imag[None, :]) ** 2
        dec = cst[np.argmin(d, axis=1)].astype(np.complex128)
        np.testing.assert_allclose(r["err_energy"], np.sum(np.abs(s.astype(np.complex128) - dec) ** 2), rtol=1e-4)
        np.testing.assert_allclose(r["ref_energy"], np.sum(np.abs(dec) ** 2), rtol=1e-4)
        np.testing.assert_allclose(r["snr_decision_db"], 10 * np.log10(r["ref_energy"] / r["err_energy"]), rtol=1e-5,
                                   atol=1e-4)
        np.testing.assert_allclose(r["snr_preamble_db"], 10 * np.log10(max(r["pilot_power"] / r["null_power"] - 1, 1e-6)),
                                   rtol=1e-5, atol=1e-4)


@pytest.mark.parametrize("mod,N,occ,CP,plen,npkt,snr,cfo", CASES)
def test_quality_against_model(orc, mod, N, occ, CP, plen, npkt, snr, cfo):
    cfg = make_cfg(mod, N, occ, CP)
    eng = engine.Engine(cfg=cfg)
    x = loopback_stream(orc, cfg, make_payloads(npkt, plen), snr_db=snr, cfo_bins=cfo)
    eng.set_taps(_abi.TAP_RX_FFT, _abi.TAP_RX_SINK, _abi.TAP_RX_DEMAPPED, _abi.TAP_RX_FRAMES)
    eng.set_rx_quality(True)
    pk = eng.rx(x)
    assert len(pk) >= 1
    recs = eng.rx_quality()
    _model_check(cfg, eng, pk, recs)
    eng.close()


@pytest.mark.parametrize("which", [0, 2, 4, 9])
def test_quality_changes_nothing_else(orc, which):
    mod, N, occ, CP, plen, npkt, snr, cfo = CASES[which]
    cfg = make_cfg(mod, N, occ, CP)
    eng = engine.Engine(cfg=cfg)
    x = loopback_stream(orc, cfg, make_payloads(npkt, plen), snr_db=snr, cfo_bins=cfo)
    pk0, pos0, st0 = eng.rx(x), eng.rx_packet_pos(), dict(eng.last_stats)
    with pytest.raises(ValueError):
        eng.rx_quality()                                  # that call ran without link quality
    eng.set_rx_quality(True)
    pk1, pos1, st1, q1 = eng.rx(x), eng.rx_packet_pos(), dict(eng.last_stats), eng.rx_quality()
    pk2, q2 = eng.rx(x), eng.rx_quality()
    assert pk1 == pk0 == pk2 and pos1.tolist() == pos0.tolist() and st1 == st0
    assert len(q1) == len(pk1) and _same(q1, q2)          # bit-reproducible
    eng.set_rx_quality(False)
    assert eng.rx(x) == pk0 and dict(eng.last_stats) == st0
    eng.close()


def _pilot_power(orc, cfg):
    """Mean |X|^2 over the known carriers of the oracle's noiseless preamble (unnormalised transform)."""
    N, CP = cfg.fft_length, cfg.cp_length
    iq = orc.tx(cfg, make_payloads(1, 50))
    p = np.abs(np.fft.fft(iq[CP:CP + N].astype(np.complex128))) ** 2
    return float(p[p > 1e-9 * p.max()].mean())


def _capture(orc, cfg, pay, pilot_snr_db, cfo_bins=0.0, seed=11):
    """AWGN of per-bin power N sigma^2 that puts the preamble's known carriers pilot_snr_db above the noise."""
    N = cfg.fft_length
    sigma = np.sqrt(_pilot_power(orc, cfg) / (N * 10 ** (pilot_snr_db / 10.0)))
    iq = orc.tx(cfg, pay, lead=2 * N, tail=cfg.fft_length + cfg.cp_length + 2 * N)
    orc.channel(iq, sigma=float(sigma), cfo=cfo_bins * 2 * np.pi / N, seed=seed)
    return iq


def test_snr_follows_the_channel(orc):
    # (15 dB is the low end: at a pilot SNR of 10 dB the timing detector -- the oracle's as well -- raises no flag)
    cfg = make_cfg("qpsk", 512, 200, 128)
    eng = engine.Engine(cfg=cfg)
    eng.set_rx_quality(True)
    pay = make_payloads(16, 1026, seed=4)
    pre, dd = [], []
    for snr in (15.0, 25.0, 35.0):
        eng.rx(_capture(orc, cfg, pay, snr, seed=int(snr)))
        q = eng.rx_quality()
        assert len(q) >= 8, (snr, len(q))
        pre.append(float(np.median(q["snr_preamble_db"])))
        dd.append(float(np.median(q["snr_decision_db"])))
        assert abs(pre[-1] - snr) <= 1.0, (snr, pre)
        # the one-preamble channel estimate costs the decisions about 2.5 - 3.5 dB here (measured: 3.2, 3.0, 2.6)
        assert pre[-1] - 4.0 <= dd[-1] <= pre[-1] + 0.5, (snr, pre, dd)
    assert dd[1] - dd[0] >= 7.0 and dd[2] - dd[1] >= 7.0, dd
    eng.close()


@pytest.mark.parametrize("mod,N,occ,CP,cfo", [("qpsk", 512, 200, 128, c) for c in (0.0, 0.05, 0.1, 0.3, 1.3, -2.4)] +
                         [("qam16", 2048, 1200, 512, 0.1)])
def test_cfo_follows_the_channel(orc, mod, N, occ, CP, cfo):
    cfg = make_cfg(mod, N, occ, CP)
    eng = engine.Engine(cfg=cfg)
    eng.set_rx_quality(True)
    pk = eng.rx(loopback_stream(orc, cfg, make_payloads(6, 800, seed=9), snr_db=30.0, cfo_bins=cfo))
    q = eng.rx_quality()
    good = [i for i, (ok, _) in enumerate(pk) if ok]
    assert len(good) >= 3
    for i in good:
        assert abs(float(q["cfo_bins"][i]) - cfo) <= 0.02, (i, q["cfo_bins"][i], q["coarse"][i])
    eng.close()


def test_cfo_sync_fixed(orc):
    """SYNC "fixed": the fine part comes from the constant frequency input of the NCO."""
    N, CP, fo = 512, 128, 0.2
    probe = make_cfg("qpsk", N, 200, CP)
    pay = make_payloads(6, 500, seed=21)
    nsym = len(orc.tx(probe, pay[:1])) // (N + CP)
    opt = options.default_options(modulation="qpsk", fft_length=N, occupied_tones=200, cp_length=CP, sync="fixed",
                                  sync_nsymbols=nsym, sync_freq_offset=float(np.pi * fo))
    cfg = config.make_cfg(opt)
    eng = engine.Engine(cfg=cfg)
    x = loopback_stream(orc, cfg, pay, snr_db=30.0, cfo_bins=fo, lead=0, tail=700)
    eng.set_taps(_abi.TAP_RX_FFT, _abi.TAP_RX_SINK, _abi.TAP_RX_DEMAPPED)
    eng.set_rx_quality(True)
    pk = eng.rx(x)
    assert [p for ok, p in pk if ok] == pay
    q = eng.rx_quality()
    _model_check(cfg, eng, pk, q)
    assert np.all(np.abs(q["cfo_bins"] - fo) <= 0.02), q["cfo_bins"]
    eng.close()


def _stream_capture(orc):
    cfg = make_cfg("qpsk")
    rng = np.random.default_rng(3)
    npkt = 30
    pay = make_payloads(npkt, rng.integers(20, 1500, npkt), seed=3)
    parts, k = [np.zeros(1500, np.complex64)], 0
    while k < npkt:
        n = int(rng.integers(1, 7))
        parts.append(orc.tx(cfg, pay[k:k + n]))
        parts.append(np.zeros(int(rng.integers(200, 40000)), np.complex64))
        k += n
    iq = np.concatenate(parts)
    psig = float(np.mean(np.abs(parts[1]) ** 2))
    orc.channel(iq, sigma=float(np.sqrt(psig / 10 ** 2.5)), cfo=0.07 * 2 * np.pi / 512, seed=78)
    return iq


def test_stream_records_equal_one_call(orc):
    iq = _stream_capture(orc)
    seen = []
    d = ofdm.ofdm_demod(options.default_options(modulation="qpsk"), quality_callback=lambda ok, p, q: seen.append(q))
    want_pk = d.work(iq)
    want = d.last_quality.copy()
    assert len(want) == len(want_pk) >= 15 and _same(np.array(seen, engine.QUALITY_DTYPE), want)
    for chunk in (131072, 50000, 300007):
        seen = []
        s = ofdm.ofdm_demod(options.default_options(modulation="qpsk"), quality_callback=lambda ok, p, q: seen.append(q))
        got_pk, got = [], []
        for a in range(0, len(iq), chunk):
            got_pk += s.feed(iq[a:a + chunk])
            got.append(s.last_quality.copy())
            assert len(got[-1]) == len(got_pk) - sum(len(g) for g in got[:-1])
        got_pk += s.flush()
        got.append(s.last_quality.copy())
        got = np.concatenate(got)
        assert got_pk == want_pk, chunk
        assert _same(got, want), chunk
        assert _same(np.array(seen, engine.QUALITY_DTYPE), want), chunk


def test_quality_edges(orc):
    cfg = make_cfg("qpsk")
    eng = engine.Engine(cfg=cfg)
    lib = _abi.load()
    x = loopback_stream(orc, cfg, make_payloads(5, 600, seed=2), snr_db=30.0)
    n = C.c_int(-1)
    eng.rx(x)
    assert lib.ofdm_rx_quality(eng._h, None, 0, C.byref(n)) == _abi.OFDM_E_INVAL
    eng.set_rx_quality(True)
    pk = eng.rx(x)
    q = eng.rx_quality()
    assert len(q) == len(pk) == 5
    buf = np.zeros(8, engine.QUALITY_DTYPE)
    assert lib.ofdm_rx_quality(eng._h, buf.ctypes.data_as(C.c_void_p), 4, C.byref(n)) == _abi.OFDM_E_CAPACITY
    assert n.value == 5
    assert lib.ofdm_rx_quality(eng._h, None, 0, C.byref(n)) == _abi.OFDM_OK and n.value == 5
    # a capture without packets: no record
    rng = np.random.default_rng(5)
    noise = (0.01 * (rng.standard_normal(30000) + 1j * rng.standard_normal(30000))).astype(np.complex64)
    assert eng.rx(noise) == [] and len(eng.rx_quality()) == 0
    assert eng.rx(np.zeros(0, np.complex64)) == [] and len(eng.rx_quality()) == 0
    eng.close()
    # device pointers: the same records
    import torch
    dcfg = make_cfg("qpsk", device_ptrs=True)
    dev = engine.Engine(cfg=dcfg)
    dev.set_rx_quality(True)
    xd = torch.from_numpy(x.view(np.float32).copy()).cuda()
    cap = len(x) + 4096
    pay = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    npk, off, ln, ok = dev.rx_device(xd.data_ptr(), len(x), pay.data_ptr(), cap, 64)
    torch.cuda.synchronize()
    assert npk == len(pk) and ok.astype(bool).tolist() == [o for o, _ in pk]
    assert _same(dev.rx_quality(), q)
    dev.close()
    # leave nothing behind in torch's cached blocks: a later torch.empty() in this process may be handed this memory
    xd.zero_()
    pay.zero_()
    torch.cuda.synchronize()
    del xd, pay
    torch.cuda.empty_cache()
