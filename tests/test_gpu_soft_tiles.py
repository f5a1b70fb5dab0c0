"""k_soft_demap (csrc/rx_soft.h) over many tiles per packet, every store shape and wide carrier maps: the captures of
soft_tile_cases.py (what each is for and that the oracle delivers it: test_soft_tile_cases_host.py).  The reference
throughout is the model soft_cases.call_values fed with the same call's TAP_RX_SINK / TAP_RX_DEMAPPED taps, link-quality
records and CSI ``eq`` rows; every comparison is array_equal on int8, no tolerance anywhere.

Per capture: the values, the packet list (the oracle's, with the lengths the host test fixes), 8 values per payload
byte, nothing below -127.  On the 64-QAM tile capture and the nmap = 258 capture, whose even-length bodies are coded
blocks: the decoder call against the model decoder in every field, a second call on a handle that has just run another
capture, the device-pointer form with a guard pattern behind the values, and feed() cut in the middle of the longest
packet against one work()."""
import functools

import numpy as np
import pytest

import fec_cases as fc
import soft_cases as sc
import soft_tile_cases as tc
from ofdm_uhd_amd import _abi, engine, ofdm, options

pytestmark = pytest.mark.gpu

TAPS = (_abi.TAP_RX_FFT, _abi.TAP_RX_SINK, _abi.TAP_RX_DEMAPPED)
TWO = ("qam64", "qam256-258")          # a tile case and a map-width case: no carrier string of their own


def _open(cfg):
    eng = engine.Engine(cfg=cfg)
    eng.set_taps(*TAPS)
    eng.set_rx_quality(True)
    eng.set_rx_csi(True)
    eng.set_rx_soft(True)
    return eng


def _call(eng, cfg, x):
    """One receive call: (packets, the model's values from the call's own taps, the engine's values)."""
    pk = eng.rx(x)
    want = sc.call_values(cfg, pk, eng.rx_quality(), eng.rx_csi()["eq"], eng.tap(_abi.TAP_RX_SINK), eng.tap(_abi.TAP_RX_DEMAPPED))
    return pk, want, eng.rx_soft()


@functools.lru_cache(maxsize=None)
def run_case(name):
    c = tc.case(name)
    eng = _open(c.cfg)
    try:
        pk, want, got = _call(eng, c.cfg, c.x)
        dec = eng.rx_fec_decode_soft() if name in TWO else None
        stats = dict(eng.last_stats)
    finally:
        eng.close()
    return dict(c=c, pk=pk, want=want, got=got, dec=dec, stats=stats)


def _equal(got, want):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == np.int8 and a.shape == b.shape, i
        assert np.array_equal(a, b), (i, len(a), np.flatnonzero(a != b)[:8].tolist())


@functools.lru_cache(maxsize=None)
def other_capture(name):
    """Another capture of the same geometry: other lengths, other bytes, other noise."""
    c = tc.case(name)
    from oracle import oracle as orc
    rng = np.random.default_rng(77)
    N = c.cfg.fft_length
    snr = tc.TILE_GRID[name][1] if name in tc.TILE_GRID else tc.WIDTH_GRID[name][7]
    a = orc.tx(c.cfg, [tc.body(n, rng) for n in (5, 32 * c.nbits + 7, 131, 64 * c.nbits + 2)])
    x = np.concatenate([np.zeros(2 * N, np.complex64), a, np.zeros(3 * N + c.cfg.cp_length, np.complex64)])
    orc.channel(x, sigma=float(np.sqrt(np.mean(np.abs(a) ** 2) / 10 ** (snr / 10.0))), seed=78)
    return x


@pytest.mark.parametrize("name", tc.ALL_CASES)
def test_values_equal_the_model(name, orc):
    r = run_case(name)
    c, pk = r["c"], r["pk"]
    _equal(r["got"], r["want"])
    assert [len(p) for _, p in pk] == list(c.lens)
    assert pk == orc.rx(c.cfg, c.x).packets
    assert [len(v) for v in r["got"]] == [8 * len(p) for _, p in pk]
    assert all(v.min(initial=0) >= -127 for v in r["got"])
    assert r["stats"]["chained_frames"] == (0 if c.cut is None else 1)
    # the comparison is not one of zeros: the packets that came back whole carry decisions throughout
    assert all(np.all(v != 0) for (ok, _), v in zip(pk, r["got"]) if ok)
    print("%s: %d packets, %d CRC-ok, longest %d bytes = %d tiles, %d store shapes" % (
        name, len(pk), sum(ok for ok, _ in pk), max(c.lens), max(tc.ntiles(n, c.nbits) for n in c.lens),
        len(tc.shape_set(c.lens, c.nbits))))


@pytest.mark.parametrize("name", TWO)
def test_decoder_equals_the_model_decoder(name):
    r = run_case(name)
    want = [fc.decode_values(v) for v in r["want"]]
    assert [(int(ok), p, c) for ok, p, c in r["dec"]] == want
    assert sum(w[0] for w in want) >= 2
    # every delivered block that came back CRC-ok decodes to something, and the long bodies are among them
    blocks = [w for (ok, p), w in zip(r["pk"], want) if ok and fc.is_block(len(p))]
    assert len(blocks) >= 2 and all(w[0] for w in blocks)
    assert max(len(w[1]) for w in blocks) >= 250


@pytest.mark.parametrize("name", TWO)
def test_second_call_on_a_used_handle(name):
    """Nothing of the call before -- staging, values, offsets -- survives into the next: another capture first (held to
    the model too), then the case, then the other one again."""
    r = run_case(name)
    c = r["c"]
    y = other_capture(name)
    eng = _open(c.cfg)
    try:
        pk0, want0, got0 = _call(eng, c.cfg, y)
        assert len(pk0) >= 3 and sum(len(p) for _, p in pk0) > 0
        _equal(got0, want0)
        pk, want, got = _call(eng, c.cfg, c.x)
        assert pk == r["pk"]
        _equal(got, want)
        _equal(got, r["got"])
        pk1, want1, got1 = _call(eng, c.cfg, y)
        assert pk1 == pk0
        _equal(got1, got0)
    finally:
        eng.close()


@pytest.mark.parametrize("name", TWO)
def test_device_pointers(name):
    torch = pytest.importorskip("torch")
    r = run_case(name)
    c = r["c"]
    mod, N, occ, CP = (tc.TILE_GRID[name][0], tc.TILE_N, tc.TILE_OCC, tc.TILE_CP) if name in tc.TILE_GRID else tc.WIDTH_GRID[name][:4]
    from helpers import make_cfg
    dev = engine.Engine(cfg=make_cfg(mod, N, occ, CP, device_ptrs=True))
    try:
        dev.set_rx_soft(True)
        x = np.ascontiguousarray(c.x)
        xd = torch.from_numpy(x.view(np.float32).copy()).cuda()
        cap = len(x) + 4096
        pay = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        npk, off, ln, ok = dev.rx_device(xd.data_ptr(), len(x), pay.data_ptr(), cap, 64)
        assert npk == len(r["pk"]) and ln.tolist() == list(c.lens)
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
        assert got == [(int(a), p, k) for a, p, k in r["dec"]] and (o[int(poff[npk]):] == 0xEE).all()
        for t in (xd, pay, vd, out):
            t.zero_()
        torch.cuda.synchronize()
        del xd, pay, vd, out
        torch.cuda.empty_cache()
    finally:
        dev.close()


@pytest.mark.parametrize("name", TWO)
def test_feed_equals_work(name):
    """The capture cut in the middle of its longest packet through feed() / flush(): last_soft, concatenated, is the
    last_soft of one work(), and that is what the engine call gave."""
    r = run_case(name)
    c = r["c"]
    mod, N, occ, CP = (tc.TILE_GRID[name][0], tc.TILE_N, tc.TILE_OCC, tc.TILE_CP) if name in tc.TILE_GRID else tc.WIDTH_GRID[name][:4]
    opt = options.default_options(modulation=mod, fft_length=N, occupied_tones=occ, cp_length=CP)
    one = ofdm.ofdm_demod(opt, soft=True)
    two = ofdm.ofdm_demod(opt, soft=True)
    try:
        x = np.ascontiguousarray(c.x)
        want_pk = one.work(x)
        want = [v.copy() for v in one.last_soft]
        assert want_pk == r["pk"]
        _equal(want, r["got"])
        cutat = tc.longest_cut(c)
        assert 0 < cutat < len(x)
        got_pk, got = [], []
        got_pk += two.feed(x[:cutat])
        got += [v.copy() for v in two.last_soft]
        assert len(got) == len(got_pk) < len(want_pk)              # the cut fell inside the burst
        got_pk += two.feed(x[cutat:])
        got += [v.copy() for v in two.last_soft]
        assert len(got) == len(got_pk)
        got_pk += two.flush()
        got += [v.copy() for v in two.last_soft]
        assert got_pk == want_pk
        _equal(got, want)
    finally:
        for o in (one, two):
            o.engine().close()
