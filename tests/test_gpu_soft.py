"""Soft-decision receive on the GPU (csrc/rx_soft.h: k_soft_demap; ofdm_set_rx_soft / ofdm_rx_soft /
ofdm_rx_fec_decode_soft).  The reference is the NumPy model of tests/soft_cases.py fed with the SAME call's own taps
(TAP_RX_SINK, TAP_RX_DEMAPPED), link-quality records and CSI ``eq`` rows, all of which other tests pin to the oracle:
every float32 operation of the definition is restated there, so the values are compared with array_equal.  On top of
that: the sign property on noisy captures, soft mode changes nothing else the receiver delivers, feed() equals work(),
the decoder call equals the model decoder on the model's values, and the layer on a frequency-selective link.

Every capture of the exact test holds, in this order: an empty packet, a one-byte packet, one that ends mid-symbol, one
whose message ends on a symbol boundary (where the geometry has such a length), a packet whose last two symbols were cut
off the air so that its chain consumes the next packet's preamble and first data symbol as data (that next packet is
swallowed), and one more packet behind them.

CPU pre-check of the link test (soft_cases.link_on_the_cpu: the coded blocks through the oracle's transmitter, the
float64 channel model of multipath_cases, the oracle's receiver with its taps, the soft model with hinv formed as
test_gpu_csi._model_check forms it, fec_cases.decode against fec_cases.decode_values): 16-QAM, N 512 / occ 200 / CP 128,
the six packets of test_gpu_fec.py (300, 301, 257, 400, 333, 300 bytes), paths (0, 1.0) and (9, 0.8 exp(2.1j)), noise
seed 7, scale 32.  Packets decoded to the payload sent, hard | soft, on the 1 dB grid:
    10 dB  000000 | 111111        13 dB  101101 | 111111        16 dB  111101 | 111111
    11 dB  100000 | 111111        14 dB  111101 | 111111        17 dB  111101 | 111111
    12 dB  100001 | 111111        15 dB  111101 | 111111        18 dB  111101 | 111111
(no decoder reported ok for a wrong payload anywhere on the grid; from 19 dB up the receiver's packet list on this
capture no longer is the six packets, so those levels are no candidates).  13 dB is the highest level at which hard
decoding loses at least two of the six while soft decoding returns all six: LINK_SNR_DB."""
import functools

import numpy as np
import pytest

import fec_cases as fc
import soft_cases as sc
from helpers import make_cfg
from ofdm_uhd_amd import _abi, engine, ofdm, options

pytestmark = pytest.mark.gpu

# mod, N, occ, CP, carriers, noise SNR in dB (the small geometries of test_gpu_link_quality.CASES; every constellation
# options.modulation accepts; 8PSK, 8-QAM and 64-QAM are the ones whose carriers straddle bytes)
GEOMS = [
    ("bpsk", 64, 48, 16, None, 30.0),
    ("qpsk", 64, 48, 16, None, 30.0),
    ("8psk", 64, 48, 16, None, 30.0),
    ("qam8", 64, 48, 16, None, 30.0),
    ("qam16", 64, 48, 16, None, 30.0),
    ("qam64", 64, 48, 16, None, 36.0),
    ("qam256", 64, 48, 16, None, 55.0),
    ("bpsk", 128, 64, 32, None, 30.0),
    ("8psk", 64, 48, 16, "F67F", 30.0),          # a carrier removed from the map: 45 carriers, nmap * nbits = 135
]
IDS = ["%s-%d%s" % (g[0], g[1], "-" + g[4] if g[4] else "") for g in GEOMS]
TAPS = (_abi.TAP_RX_FFT, _abi.TAP_RX_SINK, _abi.TAP_RX_DEMAPPED)


def _orc():
    from oracle import oracle
    oracle.lib()
    return oracle


def _cfg(g):
    mod, N, occ, CP, carriers, _ = g
    return make_cfg(mod, N, occ, CP, **({"carriers": carriers} if carriers else {}))


def _body(n, rng):
    """n bytes: a coded block where n is a block's length, so that the decoder has something to find"""
    if fc.is_block(n):
        return fc.encode(rng.integers(0, 256, (n - 10) // 2, dtype=np.uint8).tobytes())
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


@functools.lru_cache(maxsize=None)
def capture(gi, noisy):
    """(cfg, payload lengths, iq) of geometry gi."""
    g = GEOMS[gi]
    cfg = _cfg(g)
    orc = _orc()
    N, CP = cfg.fft_length, cfg.cp_length
    L = N + CP
    bps = len(sc.smap_of(cfg)) * (int(cfg.arity).bit_length() - 1)        # bits per symbol
    mid = 37 if (8 * (37 + 8)) % bps else 38
    bound = next((n for n in range(10, 400) if (8 * (n + 8)) % bps == 0), None)
    cut = max(60, 4 * bps // 8)                                            # needs four data symbols at least
    cut += cut % 2
    lens = [0, 1, mid] + ([bound] if bound else []) + [cut, 20, 30]
    rng = np.random.default_rng(100 + gi)
    pay = [_body(n, rng) for n in lens]
    k = lens.index(cut)
    a = orc.tx(cfg, pay[:k])
    b = orc.tx(cfg, pay[k:k + 1])
    c = orc.tx(cfg, pay[k + 1:])
    x = np.concatenate([np.zeros(2 * N, np.complex64), a, b[:len(b) - 2 * L], c, np.zeros(L + 2 * N, np.complex64)])
    if noisy:
        psig = float(np.mean(np.abs(a) ** 2))
        orc.channel(x, sigma=float(np.sqrt(psig / 10 ** (g[5] / 10.0))), seed=900 + gi)
    return cfg, tuple(lens), x


@functools.lru_cache(maxsize=None)
def run_case(gi, noisy, scale=32.0):
    """One receive call with everything the model needs, the model's values, and what the engine delivered."""
    cfg, lens, x = capture(gi, noisy)
    eng = engine.Engine(cfg=cfg)
    try:
        eng.set_taps(*TAPS)
        eng.set_rx_quality(True)
        eng.set_rx_csi(True)
        eng.set_rx_soft(True if scale == 32.0 else dict(scale=scale))
        pk = eng.rx(x)
        recs, rows = eng.rx_quality(), eng.rx_csi()
        want = sc.call_values(cfg, pk, recs, rows["eq"], eng.tap(_abi.TAP_RX_SINK), eng.tap(_abi.TAP_RX_DEMAPPED), scale)
        got = eng.rx_soft()
        dec = eng.rx_fec_decode_soft()
        stats = dict(eng.last_stats)
    finally:
        eng.close()
    return dict(cfg=cfg, lens=lens, pk=pk, want=want, got=got, dec=dec, stats=stats)


def _equal(got, want):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == np.int8 and a.shape == b.shape, i
        assert np.array_equal(a, b), (i, int(np.count_nonzero(a != b)), len(a))


@pytest.mark.parametrize("noisy", [False, True], ids=["clean", "noisy"])
@pytest.mark.parametrize("gi", range(len(GEOMS)), ids=IDS)
def test_values_equal_the_model(gi, noisy):
    r = run_case(gi, noisy)
    lens, pk = r["lens"], r["pk"]
    assert len(pk) >= len(lens) - 2, (len(pk), lens)          # (the swallowed packet is not delivered)
    _equal(r["got"], r["want"])
    assert [len(v) for v in r["got"]] == [8 * len(p) for _, p in pk]
    assert all(v.min(initial=0) >= -127 for v in r["got"])
    if not noisy:
        # the capture is what the file's docstring says: the short packets came back, the cut one swallowed its follower
        assert [len(p) for _, p in pk[:3]] == list(lens[:3]) and pk[0][0] and pk[1][0]
        assert r["stats"]["chained_frames"] >= 1 and any(not ok and len(p) == lens[-3] for ok, p in pk)
        # clean input: every value of a packet that came back whole is a decision, none an erasure
        assert all(np.all(v != 0) for (ok, _), v in zip(pk, r["got"]) if ok)


@pytest.mark.parametrize("gi", range(len(GEOMS)), ids=IDS)
def test_the_sign_is_the_delivered_bit(gi):
    """v != 0 implies (v > 0) == the delivered payload's bit (no seeded capture here has an equidistant pair)."""
    for noisy in (True, False):
        r = run_case(gi, noisy)
        for (ok, p), v in zip(r["pk"], r["got"]):
            bits = sc.hard_bits(p).astype(bool)
            nz = v != 0
            assert np.array_equal((v > 0)[nz], bits[nz])
            assert not ok or np.count_nonzero(nz) >= 0.9 * len(v)


@pytest.mark.parametrize("gi,noisy", [(1, False), (2, True), (4, True), (6, True), (8, False)])
def test_decoder_equals_the_model_decoder(gi, noisy):
    """rx_fec_decode_soft == fec_cases.decode_values(model values) in every field; lengths 0 and 1 are no block."""
    r = run_case(gi, noisy)
    want = [fc.decode_values(v) for v in r["want"]]
    assert [(int(ok), p, c) for ok, p, c in r["dec"]] == want
    assert want[0] == (0, b"", 0) and any(w[0] for w in want)
    if not noisy:
        # a packet whose values are all decisions decodes exactly as its hard bytes do
        full = [i for i, v in enumerate(r["want"]) if np.all(v != 0)]
        assert len(full) >= 4 and [want[i] for i in full] == [fc.decode(r["pk"][i][1]) for i in full]


def test_scale_is_applied():
    a, b = run_case(4, True), run_case(4, True, 5.0)
    _equal(b["got"], b["want"])
    assert a["pk"] == b["pk"]
    big = max(int(np.abs(v.astype(int)).max(initial=0)) for v in a["got"])
    small = max(int(np.abs(v.astype(int)).max(initial=0)) for v in b["got"])
    assert big == 127 and small < 127


@pytest.mark.parametrize("gi", [1, 5])
def test_soft_changes_nothing_else(gi):
    cfg, lens, x = capture(gi, True)
    eng = engine.Engine(cfg=cfg)
    try:
        eng.set_taps(*TAPS)
        eng.set_rx_quality(True)
        eng.set_rx_csi(True)

        def call():
            pk = eng.rx(x)
            return dict(pk=pk, pos=eng.rx_packet_pos().tolist(), st=dict(eng.last_stats), q=eng.rx_quality(), csi=eng.rx_csi(),
                        taps=[eng.tap(t) for t in TAPS])

        def same(a, b):
            assert a["pk"] == b["pk"] and a["pos"] == b["pos"] and a["st"] == b["st"]
            assert all(np.array_equal(a["q"][f], b["q"][f]) for f in engine.QUALITY_DTYPE.names)
            assert all(np.array_equal(a["csi"][k].view(np.uint32), b["csi"][k].view(np.uint32)) for k in a["csi"])
            assert all(np.array_equal(s.view(np.uint8), t.view(np.uint8)) for s, t in zip(a["taps"], b["taps"]))

        off = call()
        with pytest.raises(ValueError):
            eng.rx_soft()                                    # that call ran without soft values
        eng.set_rx_soft(True)
        on = call()
        v1 = eng.rx_soft()
        same(off, on)
        on2 = call()
        _equal(eng.rx_soft(), v1)                            # bit-reproducible
        same(off, on2)
        eng.set_rx_soft(None)
        with pytest.raises(ValueError):
            eng.rx_soft()                                    # the values went with the option
        same(off, call())
        # the caller's own settings keep answering as set: soft mode alone opens no tap, no records, no rows
        eng.set_taps()
        eng.set_rx_quality(False)
        eng.set_rx_csi(False)
        plain = eng.rx(x)
        eng.set_rx_soft(True)
        assert eng.rx(x) == plain == off["pk"]
        _equal(eng.rx_soft(), v1)
        for refused in (lambda: eng.tap(_abi.TAP_RX_SINK), lambda: eng.tap(_abi.TAP_RX_DEMAPPED), eng.rx_quality, eng.rx_csi):
            with pytest.raises(ValueError):
                refused()
    finally:
        eng.close()


def test_edges_and_refusals():
    cfg, lens, x = capture(1, True)
    eng = engine.Engine(cfg=cfg)
    lib = _abi.load()
    try:
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError):
                eng.set_rx_soft(bad)
        with pytest.raises(ValueError):
            eng.set_rx_soft(dict(gain=3))
        eng.set_rx_soft(True)
        pk = eng.rx(x)
        vals = eng.rx_soft()
        total = sum(len(v) for v in vals)
        assert len(vals) == len(pk) >= 4 and total > 0
        import ctypes as C
        n = C.c_int(-1)
        buf = np.zeros(total, np.int8)
        assert lib.ofdm_rx_soft(eng._h, buf.ctypes.data_as(C.c_void_p), total - 1, None, C.byref(n)) == _abi.OFDM_E_CAPACITY
        assert n.value == len(pk)
        assert lib.ofdm_rx_soft(eng._h, None, 0, None, None) == _abi.OFDM_E_INVAL
        ok = np.zeros(len(pk), np.uint8)
        corr = np.zeros(len(pk), np.uint32)
        poff = np.zeros(len(pk) + 1, np.uint64)
        out = np.zeros(total, np.uint8)
        args = (out.ctypes.data_as(C.c_void_p), len(out), poff.ctypes.data_as(C.POINTER(C.c_uint64)), ok.ctypes.data_as(C.c_void_p),
                corr.ctypes.data_as(C.POINTER(C.c_uint32)))
        n.value = -1
        assert lib.ofdm_rx_fec_decode_soft(eng._h, None, *args, len(pk) - 1, C.byref(n)) == _abi.OFDM_E_CAPACITY
        assert n.value == len(pk)
        # fewer packet slots than packets: the call fails as it always did, and leaves no values
        with pytest.raises(engine.EngineError):
            eng.rx(x, max_pkts=2)
        assert eng.rx_soft() == [] and eng.rx_fec_decode_soft() == []
        # a capture without packets, an empty capture
        rng = np.random.default_rng(5)
        noise = (0.01 * (rng.standard_normal(20000) + 1j * rng.standard_normal(20000))).astype(np.complex64)
        for cap in (noise, np.zeros(0, np.complex64)):
            assert eng.rx(cap) == [] and eng.rx_soft() == [] and eng.rx_fec_decode_soft() == []
        # timing: only with profiling on, and the kernel table is what it was
        eng.rx(x)
        with pytest.raises(ValueError):
            eng.rx_soft_last_ms()
        eng.prof_enable(True)
        eng.rx(x)
        assert eng.rx_soft_last_ms() > 0.0 and len(eng.prof()) == _abi.K_COUNT
        eng.prof_enable(False)
    finally:
        eng.close()


def test_device_pointers():
    torch = pytest.importorskip("torch")
    r = run_case(4, True)
    cfg, lens, x = capture(4, True)
    dev = engine.Engine(cfg=make_cfg(GEOMS[4][0], *GEOMS[4][1:4], device_ptrs=True))
    try:
        dev.set_rx_soft(True)
        xd = torch.from_numpy(x.view(np.float32).copy()).cuda()
        cap = len(x) + 4096
        pay = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        npk, off, ln, ok = dev.rx_device(xd.data_ptr(), len(x), pay.data_ptr(), cap, 64)
        assert npk == len(r["pk"])
        total = int(8 * ln.astype(np.int64).sum())
        vd = torch.full((total + 64,), 99, dtype=torch.int8, device="cuda")
        voff = dev.rx_soft_device(vd.data_ptr(), total)
        v = vd.cpu().numpy()
        assert voff.tolist() == (8 * off).tolist() and (v[total:] == 99).all()      # nothing behind the values
        _equal([v[int(voff[i]):int(voff[i + 1])] for i in range(npk)], r["want"])
        out = torch.full((cap,), 0xEE, dtype=torch.uint8, device="cuda")
        poff, dok, corr = dev.rx_fec_decode_soft_device(out.data_ptr(), cap)
        o = out.cpu().numpy()
        got = [(int(dok[i]), o[int(poff[i]):int(poff[i + 1])].tobytes(), int(corr[i])) for i in range(npk)]
        assert got == [(int(a), p, c) for a, p, c in r["dec"]] and (o[int(poff[npk]):] == 0xEE).all()
        for t in (xd, pay, vd, out):
            t.zero_()
        torch.cuda.synchronize()
        del xd, pay, vd, out
        torch.cuda.empty_cache()
    finally:
        dev.close()


def test_feed_equals_work():
    """A capture cut in two through feed() / flush() gives the last_soft of one work(), concatenated; with fec as well,
    the same decoded packets.  The capture is longer than two spans (the seven payloads four times over, 8000 silent
    samples between the bursts), so that either cut has feed() deliver packets before flush(): a shorter one leaves
    everything to flush(), which is one call on the whole capture (tests/test_gpu_coded_stream.py has the long form)."""
    opt = options.default_options(modulation="qam16")
    orc = _orc()
    cfg = make_cfg("qam16")
    rng = np.random.default_rng(77)
    pay = [_body(n, rng) for n in (210, 64, 0, 333, 100, 12, 250)]
    burst = orc.tx(cfg, pay)
    x = np.concatenate([np.zeros(1500, np.complex64)] + 4 * [burst, np.zeros(8000, np.complex64)])
    orc.channel(x, sigma=float(np.sqrt(np.mean(np.abs(burst) ** 2) / 10 ** 1.8)), seed=5)
    one = ofdm.ofdm_demod(opt, fec=True, soft=True)
    two = ofdm.ofdm_demod(opt, fec=True, soft=dict(scale=32))
    bare = ofdm.ofdm_demod(opt, soft=True)
    try:
        want_pk = one.work(x)
        want = [v.copy() for v in one.last_soft]
        assert len(x) >= 2 * one._stream_geometry()[1]
        assert len(want) == len(want_pk) >= 6 and one.last_fec and len(one.last_fec) == len(want_pk)
        raw = bare.work(x)                                       # soft without fec only fills last_soft
        _equal(bare.last_soft, want)
        assert bare.last_fec == [] and [len(v) for v in want] == [8 * len(p) for _, p in raw]
        assert want_pk == [(bool(d[0]), d[1]) for d in (fc.decode_values(v) for v in want)]
        for cutat in (len(x) // 2, len(x) // 3 + 11):
            got_pk, got = [], []
            for piece in (x[:cutat], x[cutat:]):
                got_pk += two.feed(piece)
                got += [v.copy() for v in two.last_soft]
                assert len(got) == len(got_pk)
            assert len(got_pk) >= 1                              # delivered by feed(), before flush()
            got_pk += two.flush()
            got += [v.copy() for v in two.last_soft]
            assert got_pk == want_pk
            _equal(got, want)
    finally:
        for o in (one, two, bare):
            o.engine().close()


def test_link_soft_decisions_recover_what_hard_decisions_lose():
    """The link of this file's docstring at LINK_SNR_DB.  Exact part: values and decoder output equal the model in every
    field.  Physical part: ofdm_demod(fec=True, soft=True) returns more decoded-ok packets than ofdm_demod(fec=True), and
    every ok payload is the one sent."""
    opt = options.default_options(modulation=sc.LINK_MOD, fft_length=sc.LINK_N, occupied_tones=sc.LINK_OCC, cp_length=sc.LINK_CP)
    pay = list(sc.link_payloads())
    mod = ofdm.ofdm_mod(opt, pad_for_usrp=False, fec=True)
    hard = ofdm.ofdm_demod(opt, fec=True)
    soft = ofdm.ofdm_demod(opt, fec=True, soft=True)
    eng = engine.Engine(opt)
    try:
        for p in pay:
            mod.send_pkt(p)
        iq = mod.flush()
        psig = float(np.mean(np.abs(iq.astype(np.complex128)) ** 2))
        ch = mod.engine()
        ch.set_multipath(sc.link_channel_cfg(sc.LINK_SNR_DB, psig))
        y = ch.multipath(sc.link_air(iq))
        eng.set_taps(*TAPS)
        eng.set_rx_quality(True)
        eng.set_rx_csi(True)
        eng.set_rx_soft(True)
        pk = eng.rx(y)
        assert len(pk) == len(pay)
        want = sc.call_values(eng.cfg, pk, eng.rx_quality(), eng.rx_csi()["eq"], eng.tap(_abi.TAP_RX_SINK),
                              eng.tap(_abi.TAP_RX_DEMAPPED))
        _equal(eng.rx_soft(), want)
        wdec = [fc.decode_values(v) for v in want]
        assert [(int(a), p, c) for a, p, c in eng.rx_fec_decode_soft()] == wdec
        got_h, got_s = hard.work(y), soft.work(y)
        print("link at %.0f dB: outer ok %s, hard ok %s, soft ok %s, corrected hard %s soft %s" % (
            sc.LINK_SNR_DB, [int(ok) for ok, _ in pk], [int(ok) for ok, _ in got_h], [int(ok) for ok, _ in got_s],
            [c for _, c in hard.last_fec], [c for _, c in soft.last_fec]))
        assert got_s == [(bool(w[0]), w[1]) for w in wdec]
        assert got_h == [(bool(d[0]), d[1]) for d in (fc.decode(p) for _, p in pk)]
        assert soft.last_fec == [(bool(ok), w[2]) for (ok, _), w in zip(pk, wdec)]
        assert soft.n_ok > hard.n_ok, (soft.n_ok, hard.n_ok)
        for got in (got_h, got_s):
            for (ok, p), sent in zip(got, pay):
                assert not ok or p == sent
    finally:
        for o in (mod, hard, soft):
            o.engine().close()
        eng.close()
