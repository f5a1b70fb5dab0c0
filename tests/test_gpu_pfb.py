"""The polyphase-FFT channeliser on the GPU (k_pfb, Engine.pfb, ofdm_demod_channelizer): against the float64 model of its
definition within the derived bound, exact where it must be, independent of the selection and of the segmentation,
against the DDC bank, end to end on the on-grid two-link captures, at its edges, and beside the other stages."""
import ctypes as C

import numpy as np
import pytest

import ddc_cases
import duc_cases
import pfb_cases as pc
import stage_harness as sh
from helpers import make_cfg, make_payloads
from ofdm_uhd_amd import _abi, ddc, duc, engine, ofdm, pfb, resample, tx_resample
from stage_harness import EPS, eng   # noqa: F401 (eng: one handle per file)

pytestmark = pytest.mark.gpu

STAGE = sh.STAGES["pfb"]
_stream, _options, _engine_tx, _wide_sc16 = sh.rx_stream, sh.options_of, sh.engine_tx, sh.wide_sc16


def _check_against_model(y, x, h, M, chans, first, what):
    """Every output of every row within pfb_cases.bound of the float64 model; returns the worst error / bound."""
    worst = 0.0
    for i, c in enumerate(chans):
        y64, s = pc.model(x, h, M, c, first)
        assert len(y[i]) == len(y64) == pc.count(first, len(x), M), what
        err = np.abs(y[i].astype(np.complex128) - y64)
        bound = pc.bound(len(h), M, s)
        if len(err):
            worst = max(worst, float(np.max(err / np.maximum(bound, 1e-300))))
        assert np.all(err <= bound), (what, c)
    print("%s: %d x %d outputs, worst error / bound = %.3g" % (what, len(chans), y.shape[1], worst))
    return worst


@pytest.mark.parametrize("fmt", ["fc32", "sc16"])
@pytest.mark.parametrize("M", pc.CHANNEL_COUNTS)
def test_against_float64_model(eng, M, fmt):
    rng = np.random.default_rng(6000 + M)
    n = pc.stream_length(M)
    start = 1000003
    assert start % M != 0 and n % (pc.tile_outputs(M) * M) != 0
    eng.set_rx_iq_format(fmt)
    try:
        raw, x = _stream(rng, n, fmt)
        for ntaps in pc.TAP_GRID[M]:
            h = pc.taps_for(rng, ntaps)
            eng.set_pfb(pfb.pfb_cfg(M, taps=h))
            for first in (0, start):
                if first:
                    eng.pfb_reset(first)
                assert eng.pfb_count(n) == pc.count(first, n, M)
                y = eng.pfb(raw)
                assert y.shape == (M, pc.count(first, n, M)) and y.dtype == np.complex64
                _check_against_model(y, x, h, M, range(M), first, "M=%d ntaps=%d first=%d %s" % (M, ntaps, first, fmt))
    finally:
        eng.set_rx_iq_format("fc32")
        eng.set_pfb(None)


@pytest.mark.parametrize("M", pc.CHANNEL_COUNTS)
def test_a_single_unit_tap_gives_every_channel_the_decimated_input(eng, M):
    rng = np.random.default_rng(M)
    n = pc.stream_length(M)
    raw, x = _stream(rng, n, "fc32")
    try:
        eng.set_pfb(pfb.pfb_cfg(M, taps=[1.0]))
        for first in (0, 1000003):
            eng.pfb_reset(first)
            y = eng.pfb(raw)
            want = x[(-first) % M::M]
            assert y.shape == (M, len(want))
            for c in range(M):
                assert np.array_equal(y[c], want), (M, c, first)
    finally:
        eng.set_pfb(None)


@pytest.mark.parametrize("M,ntaps", [(4, 31), (8, 155), (16, 17), (32, 31), (64, 65)])
def test_selection_order_and_count_do_not_matter(eng, M, ntaps):
    rng = np.random.default_rng(300 + M)
    n = pc.tile_outputs(M) * M + 1001
    raw, _ = _stream(rng, n, "fc32")
    h = pc.taps_for(rng, ntaps)
    try:
        eng.set_pfb(pfb.pfb_cfg(M, taps=h))
        ref = eng.pfb(raw).copy()
        perm = [int(i) for i in rng.permutation(M)]
        assert perm != list(range(M))
        subset = sorted(int(i) for i in rng.choice(M, max(M // 2 - 1, 1), replace=False))
        repeated = [M - 1, 0, M - 1, M // 2, M - 1][:M]
        for sel in [perm, subset, repeated, [-1]] + [[c] for c in (0, M // 2, M - 1)]:
            eng.set_pfb(pfb.pfb_cfg(M, sel, taps=h))
            y = eng.pfb(raw)
            assert y.shape == (len(sel), ref.shape[1])
            for j, c in enumerate(sel):
                assert np.array_equal(y[j], ref[c % M]), (sel, j)
    finally:
        eng.set_pfb(None)


SEG_SHAPES = [(2, 1024), (4, 31), (4, 3), (8, 155), (8, 7), (16, 17), (64, 1024), (64, 63)]


@pytest.mark.parametrize("fmt", ["fc32", "sc16"])
@pytest.mark.parametrize("M,ntaps", SEG_SHAPES)
def test_any_segmentation_gives_the_same_bits(eng, M, ntaps, fmt):
    rng = np.random.default_rng(53 * M + ntaps)
    tile = pc.tile_outputs(M) * M
    n = 3 * tile + 1234 + 3 * ntaps
    K = min(M, 3)
    sel = [M - 1, 0, M // 2][:K]
    eng.set_rx_iq_format(fmt)
    try:
        raw, x = _stream(rng, n, fmt)
        h = pc.taps_for(rng, ntaps)
        eng.set_pfb(pfb.pfb_cfg(M, sel, taps=h))
        for first in (0, 7 * 1024 + 5):
            eng.pfb_reset(first)
            whole = eng.pfb(raw).copy()
            assert whole.shape == (K, pc.count(first, n, M))
            if first == 0:
                _check_against_model(whole, x, h, M, sel, 0, "whole M=%d ntaps=%d %s" % (M, ntaps, fmt))
            eng.pfb_reset(first)
            sizes = pc.chunk_sizes(rng, n, M, ntaps)
            assert sum(sizes) == n and {0, 1, M, M + 1, 997, tile - 1, tile + 1, ntaps} <= set(sizes)
            parts, a, empty = [], first, 0
            for s in sizes:
                want = pc.count(a, s, M)
                assert eng.pfb_count(s) == want
                y = eng.pfb(raw[a - first:a - first + s])
                assert y.shape == (K, want)
                empty += want == 0
                parts.append(y.copy())
                a += s
            assert empty >= 2                             # calls that produce nothing are part of the stream
            assert np.array_equal(np.concatenate(parts, axis=1), whole), (M, ntaps, first, fmt)
    finally:
        eng.set_rx_iq_format("fc32")
        eng.set_pfb(None)


@pytest.mark.parametrize("M,ntaps", [(4, 31), (8, 155), (64, 155)])
def test_against_the_ddc_bank_on_the_grid(eng, M, ntaps):
    """Same taps, R = M, fc = c / M: the two stages differ by no more than their two derived bounds."""
    rng = np.random.default_rng(900 + M)
    n = pc.stream_length(M)
    raw, x = _stream(rng, n, "fc32")
    h = pc.taps_for(rng, ntaps)
    chans = list(range(M)) if M <= 8 else [0, 1, 7, 31, 32, 33, 40, 63]
    fcs = [c / float(M) if c <= M // 2 else (c - M) / float(M) for c in chans]
    try:
        eng.set_pfb(pfb.pfb_cfg(M, chans, taps=h))
        y = eng.pfb(raw).copy()
        eng.set_ddc_bank(ddc.bank_cfg(M, fcs, taps=h))
        z = eng.ddc_bank(raw)
        assert y.shape == z.shape
        worst = 0.0
        for i, c in enumerate(chans):
            _, s = pc.model(x, h, M, c)
            tab = eng.ddc_bank_taps(i)
            _, s_ddc = ddc_cases.model(x, tab, M, ddc_cases.phase_step(fcs[i], M))
            bound = pc.bound(ntaps, M, s) + (ntaps + 16) * EPS * s_ddc
            err = np.abs(y[i].astype(np.complex128) - z[i].astype(np.complex128))
            worst = max(worst, float(np.max(err / bound)))
            assert np.all(err <= bound), (M, c)
        print("M=%d ntaps=%d: worst |pfb - bank| / (sum of the bounds) = %.3g" % (M, ntaps, worst))
    finally:
        eng.set_pfb(None)
        eng.set_ddc_bank(None)


@pytest.mark.parametrize("name,fmt", [("qpsk512_r4", "fc32"), ("qpsk512_r4", "sc16"), ("qam16_2048_r2", "fc32"),
                                      ("bpsk64_r8", "fc32")])
def test_two_links_end_to_end(orc, name, fmt):
    """Engine.tx -> Engine.duc per link (the second added onto the first) -> the noise of ddc_cases -> Engine.pfb ->
    Engine.rx per channel; then the same band through ofdm_demod_channelizer."""
    M, chans = pc.ON_GRID[name]
    e = engine.Engine(cfg=make_cfg(*ddc_cases.CASES[name][:4]))
    try:
        k = duc_cases.links(name, tx=_engine_tx(e))
        (xa, xb), (fa, fb) = k["x"], k["freqs"]
        assert M == k["R"]
        e.set_duc(duc.duc_cfg(M, fa, taps=k["tx_taps"]))
        wa = e.duc(xa)
        e.set_duc(duc.duc_cfg(M, fb, taps=k["tx_taps"]))
        both = e.duc(xb, add=wa)
        e.set_duc(None)
        wide = (both.astype(np.complex128) + duc_cases.noise(len(wa), k["P"], M)).astype(np.complex64)
        if fmt == "sc16":
            wide = _wide_sc16(wide)
        e.set_rx_iq_format(fmt)
        e.set_pfb(pfb.pfb_cfg(M, chans, taps=k["rx_taps"]))
        y = e.pfb(wide)                                   # one call, both links
        e.set_rx_iq_format("fc32")
        assert y.shape == (2, pc.count(0, len(wide), M))
        per_link = []
        for i, sent in enumerate(k["payloads"]):
            got = e.rx(y[i])
            assert got == orc.rx(k["cfg"], np.ascontiguousarray(y[i])).packets, (name, i)
            assert [ok for ok, _ in got] == [True] * 4 and [p for _, p in got] == sent, (name, i)
            per_link.append(got)
    finally:
        e.close()
    order = []
    signed = [c if c < M // 2 else c - M for c in chans]  # the signed spelling of the same channels
    ch = ofdm.ofdm_demod_channelizer(_options(k), M, signed, taps=k["rx_taps"], iq_format=fmt,
                                     callback=lambda pos, ok, p: order.append((pos, ok, p)))
    try:
        assert ch.work(wide) == per_link, name
        assert order == [(i, ok, p) for i in range(2) for ok, p in per_link[i]]   # position 0's packets, then 1's
        del order[:]
        chunks = [[], []]
        for a in range(0, len(wide), 5000):
            calls = len(order)
            out = ch.feed(wide[a:a + 5000])
            assert order[calls:] == [(i, ok, p) for i in range(2) for ok, p in out[i]]
            for i in range(2):
                chunks[i] += out[i]
        out = ch.flush()
        for i in range(2):
            chunks[i] += out[i]
        assert chunks == per_link, name
        assert ch.work(wide) == per_link                  # a stream starts afresh after a flush
        assert len(ch.links()) == 2 and ch.engine().pfb_cfg.nsel == 2
    finally:
        ch.close()
    assert ch.engine()._h.value is None and all(d.engine()._h.value is None for d in ch.links())


def test_layout_and_capacity(eng):
    sh.check_rx_layout_and_capacity(eng, STAGE, (4,), [3, 0, 1], pfb.design(4, 0.4), one_sel=[0])


def test_invalid_arguments_are_refused(eng):
    x = np.zeros(64, np.complex64)
    x[::3] = 1.0

    def index_limits_and_misaligned_buffers(lib, x, out):
        # index limits: the DDC bank's
        eng.pfb_reset(1 << 62)
        assert eng.pfb_count(8) == 2
        with pytest.raises(ValueError):
            eng.pfb_reset((1 << 62) + 1)
        assert eng.pfb_count(8) == 2                          # the refused reset left the stream where it was
        nn = C.c_uint64(0)
        assert lib.ofdm_pfb(eng._h, x.ctypes.data_as(C.c_void_p), (1 << 62) + 1, out.ctypes.data_as(C.c_void_p), 64, 64,
                            C.byref(nn)) == _abi.OFDM_E_INVAL
        eng.pfb_reset(0)
        # misaligned buffers: complex64 in and out on 8 bytes (16-bit in on 4: the harness)
        f = np.zeros(2 * 64 + 2, np.float32)
        assert lib.ofdm_pfb(eng._h, C.c_void_p(f.ctypes.data + 4), 64, out.ctypes.data_as(C.c_void_p), 64, 64,
                            C.byref(nn)) == _abi.OFDM_E_INVAL
        assert lib.ofdm_pfb(eng._h, x.ctypes.data_as(C.c_void_p), 64, C.c_void_p(f.ctypes.data + 4), 16, 16,
                            C.byref(nn)) == _abi.OFDM_E_INVAL
    base = lambda: pfb.pfb_cfg(4, [1, 3], taps=np.ones(5, np.float32))
    sh.check_rx_bank_invalid_arguments(eng, STAGE, (4,), base, x, nout=16, after62=(0, 1), still_refused=3, edge_sel=None,
                                       middle=index_limits_and_misaligned_buffers)


@pytest.mark.parametrize("fmt", ["fc32", "sc16"])
def test_device_pointers(fmt):
    import torch
    M, sel = 8, [5, 0, 7, 2, 5]
    rng = np.random.default_rng(31)
    n = 3 * pc.tile_outputs(M) * M + 77
    raw, _ = _stream(rng, n, fmt)
    host = engine.Engine(cfg=make_cfg())
    devE = engine.Engine(cfg=make_cfg(device_ptrs=True))
    try:
        x, y = sh.check_rx_device_pointers(torch, STAGE, host, devE, pfb.pfb_cfg(M, sel, taps=pfb.design(M, 0.75)), raw,
                                           len(sel), fmt)[:2]
        sh.release(torch, x, y)
    finally:
        host.close()
        devE.close()


def test_device_pointer_path_behind_an_asynchronous_transmit():
    """The channeliser's input is what tx_device(wait=False) -> duc_device is still producing on the same handle."""
    import torch
    cfg = make_cfg()
    pays = make_payloads(4, 100, seed=7)
    M = 4
    tx_taps, rx_taps = duc.design(M, 200 / 512.0), pfb.design(M, 200 / 512.0)
    host = engine.Engine(cfg=cfg)
    dev = engine.Engine(cfg=make_cfg(device_ptrs=True))
    try:
        x = host.tx(pays)
        host.set_duc(duc.duc_cfg(M, 0.25, taps=tx_taps))
        wide = host.duc(x)
        host.set_pfb(pfb.pfb_cfg(M, taps=rx_taps))
        want = host.pfb(wide)
        no = want.shape[1]
        blob, offs, lens = engine.pack_payloads(pays)
        _, nsamp = dev.tx_frame_count(lens)
        assert nsamp == len(x) and no == nsamp
        d_pay = torch.from_numpy(blob.copy()).cuda()
        d_iq = torch.zeros(nsamp, dtype=torch.complex64, device="cuda")
        d_wide = torch.zeros(nsamp * M, dtype=torch.complex64, device="cuda")
        d_out = torch.zeros((M, no), dtype=torch.complex64, device="cuda")
        dev.set_duc(duc.duc_cfg(M, 0.25, taps=tx_taps))
        dev.set_pfb(pfb.pfb_cfg(M, taps=rx_taps))
        torch.cuda.synchronize()
        assert dev.tx_device(d_pay.data_ptr(), offs, lens, d_iq.data_ptr(), nsamp, wait=False) == nsamp
        assert dev.duc_device(d_iq.data_ptr(), nsamp, d_wide.data_ptr(), nsamp * M) == nsamp * M
        assert dev.pfb_device(d_wide.data_ptr(), nsamp * M, d_out.data_ptr(), no, no) == no
        assert np.array_equal(d_wide.cpu().numpy(), wide)
        assert np.array_equal(d_out.cpu().numpy(), want)
        sh.release(torch, d_pay, d_iq, d_wide, d_out)
    finally:
        host.close()
        dev.close()


def test_the_other_stages_and_the_channeliser_do_not_disturb_each_other(eng):
    rng = np.random.default_rng(23)
    n = 9000
    raw, _ = _stream(rng, n, "fc32")
    nb = (0.1 * raw[:3000]).astype(np.complex64)
    t155, t31 = pc.taps_for(rng, 155), pc.taps_for(rng, 31)
    stages = {
        "pfb": (lambda: eng.set_pfb(pfb.pfb_cfg(8, [1, 6, 3], taps=t155)), lambda a, b: eng.pfb(raw[a:b]), n, 1777),
        "ddc": (lambda: eng.set_ddc(ddc.ddc_cfg(3, 0.2, taps=t31)), lambda a, b: eng.ddc(raw[a:b])[None], n, 1300),
        "ddc_bank": (lambda: eng.set_ddc_bank(ddc.bank_cfg(8, [0.125, -0.25], taps=t155)),
                     lambda a, b: eng.ddc_bank(raw[a:b]), n, 2111),
        "resamp": (lambda: eng.set_resamp(resample.resamp_cfg(2, 5, 0.1, taps=t31)), lambda a, b: eng.resamp(raw[a:b])[None],
                   n, 1501),
        "duc": (lambda: eng.set_duc(duc.duc_cfg(4, 0.25, taps=t31)), lambda a, b: eng.duc(nb[a:b])[None], len(nb), 700),
        "tx_resamp": (lambda: eng.set_tx_resamp(tx_resample.tx_resamp_cfg(5, 2, 0.1, taps=t31)),
                      lambda a, b: eng.tx_resamp(nb[a:b])[None], len(nb), 611),
    }
    off = dict(pfb=eng.set_pfb, ddc=eng.set_ddc, ddc_bank=eng.set_ddc_bank, resamp=eng.set_resamp, duc=eng.set_duc,
               tx_resamp=eng.set_tx_resamp)
    try:
        alone = sh.check_interleaved(stages, off)
        # dropping or resetting another stage leaves the channeliser's stream where it was, and the other way round
        eng.pfb(raw[:100])
        eng.ddc_bank_reset(0)
        eng.set_ddc(None)
        assert eng.pfb_count(4) == pc.count(n + 100, 4, 8)
        eng.set_pfb(None)
        assert eng.ddc_bank_count(8) == 1 and np.array_equal(eng.ddc_bank(raw), alone["ddc_bank"])
    finally:
        for f in off.values():
            f(None)


def test_a_handle_that_dropped_the_channeliser_runs_what_it_ran(orc):
    """Two handles transmit and demodulate the same packets: one never saw the channeliser, the other used it on another
    stream and dropped it.  Same IQ bits, same packets, same per-kernel launch counts; the kernel table has no entry for
    the stage."""
    cap = ddc_cases.capture("qpsk512_r4")
    cfg = cap["cfg"]
    pays = cap["payloads"][0]
    a, b = engine.Engine(cfg=cfg), engine.Engine(cfg=cfg)
    try:
        b.set_pfb(pfb.pfb_cfg(4, [1, 3], taps=cap["taps"]))
        y = b.pfb(cap["wide"])[0].copy()
        b.set_pfb(None)
        for e in (a, b):
            e.prof_enable(True)
            e.prof_reset()
        ia, ib = a.tx(pays), b.tx(pays)
        assert np.array_equal(ia, ib)
        pa, pb = a.rx(y), b.rx(y)
        assert pa == pb and [p for ok, p in pa if ok] == pays
        ca = {k: v[1] for k, v in a.prof().items()}
        cb = {k: v[1] for k, v in b.prof().items()}
        assert ca == cb and sum(ca.values()) > 0
        assert len(ca) == _abi.K_COUNT == 11 and not any("pfb" in k for k in ca)
        # with the channeliser configured the receiver's own launches stay what they are, and the stage reports its time
        b.set_pfb(pfb.pfb_cfg(4, [1, 3], taps=cap["taps"]))
        b.prof_reset()
        with pytest.raises(ValueError):
            b.pfb_last_ms()                               # no profiled call yet
        y2 = b.pfb(cap["wide"])
        assert np.array_equal(y2[0], y) and b.pfb_last_ms() > 0.0
        a.prof_reset()
        assert b.rx(y2[0]) == pa == a.rx(y)
        assert {k: v[1] for k, v in b.prof().items()} == {k: v[1] for k, v in a.prof().items()}
    finally:
        a.close()
        b.close()
