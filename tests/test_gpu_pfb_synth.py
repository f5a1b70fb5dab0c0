"""The polyphase-FFT synthesis bank on the GPU (k_pfb_synth, Engine.pfb_synth, ofdm_mod_channelizer): against the float64
model of its definition within the derived bound, exact where it must be (channel 0 alone is the DUC at fc = 0),
independent of the order of the selection and of the segmentation, against K DUC passes, end to end into the
channeliser, at its edges, and beside the other stages."""
import functools

import numpy as np
import pytest

import ddc_cases
import duc_cases
import pfb_cases as pc
import pfb_synth_cases as sc
import stage_harness as sh
from helpers import make_cfg, make_payloads
from ofdm_uhd_amd import _abi, duc, engine, iqio, ofdm, pfb
from stage_harness import SCALE, START, eng   # noqa: F401 (eng: one handle per file)

pytestmark = pytest.mark.gpu

STAGE = sh.STAGES["pfb_synth"]
_rows, _bits, _c64, _options = sh.rows, sh.bits, sh.c64, sh.options_of


@functools.lru_cache(maxsize=None)
def _reference(M, ntaps):
    """Computed once per shape and shared (read-only): the inputs of all M channels, the taps, the band to add onto and
    the float64 model's per-channel terms."""
    rng = np.random.default_rng(7000 + 13 * M + ntaps)
    nin = sc.stream_inputs(M)
    x = _rows(rng, M, nin)
    h = sc.taps_for(rng, ntaps)
    add = _rows(rng, 1, nin * M)[0]
    y, s = sc.model_terms(x, h, M, range(M))
    # a power of two (exact on the float32 inputs and on the linear model) that brings the band's peak to 1/8 .. 1/4
    band = y.sum(axis=0)
    g = 2.0 ** np.floor(np.log2(0.25 / max(np.max(np.abs(band.real)), np.max(np.abs(band.imag)))))
    x, y, s = (x * np.float32(g)).astype(np.complex64), y * g, s * g
    for a in (x, h, add, y, s):
        a.setflags(write=False)
    return x, h, add, y, s


def _subset(M):
    rng = np.random.default_rng(M)
    return [int(c) for c in rng.permutation(M)[:max(M // 2 - 1, 1)]]


@pytest.mark.parametrize("with_add", [False, True], ids=["plain", "add"])
@pytest.mark.parametrize("fmt", ["fc32", "sc16"])
@pytest.mark.parametrize("M", sc.CHANNEL_COUNTS)
def test_against_float64_model(eng, M, fmt, with_add):
    """Measured worst error / bound over all cases: see DESIGN.md section 7."""
    worst = 0.0
    try:
        for ntaps in sc.TAP_GRID[M]:
            x, h, add, y64, s = _reference(M, ntaps)
            nin = x.shape[1]
            assert nin % sc.tile_inputs(M) != 0 and START % sc.tile_inputs(M) != 0
            for chans in (list(range(M)), _subset(M)):
                want = y64[chans].sum(axis=0) + (add.astype(np.complex128) if with_add else 0.0)
                bound = sc.bound(ntaps, M, s[chans].sum(axis=0), add if with_add else None)
                if fmt == "sc16":
                    assert np.max(np.abs(want.real)) < 0.99 and np.max(np.abs(want.imag)) < 0.99  # nothing saturates
                eng.set_pfb_synth(pfb.synth_cfg(M, chans, taps=h, out_format=fmt))
                for first in (0, START):
                    eng.pfb_synth_reset(first)
                    out = eng.pfb_synth(x[chans], add=add if with_add else None)
                    assert len(out) == nin * M and out.dtype == (np.int16 if fmt == "sc16" else np.complex64)
                    if fmt == "sc16":                                  # per part: half a step of the 16-bit store
                        err, half = sc.sc16_error(_c64(out, fmt), want, SCALE)
                        bound_ = bound + half
                    else:
                        err, bound_ = np.abs(_c64(out, fmt) - want), bound
                    ratio = float(np.max(err / np.maximum(bound_, 1e-300)))
                    worst = max(worst, ratio)
                    print("M=%d ntaps=%d K=%d first=%d %s%s: worst error / bound = %.3g"
                          % (M, ntaps, len(chans), first, fmt, " add" if with_add else "", ratio))
                    assert np.all(err <= bound_), (M, ntaps, len(chans), first)
    finally:
        eng.set_pfb_synth(None)
    print("M=%d %s%s: worst error / bound over its cases = %.3g" % (M, fmt, " add" if with_add else "", worst))


@pytest.mark.parametrize("fmt", ["fc32", "sc16"])
@pytest.mark.parametrize("M,ntaps", [(2, 1024), (4, 31), (8, 155), (16, 17), (32, 31), (64, 65)])
def test_channel_zero_alone_is_the_duc_at_zero_frequency(eng, M, ntaps, fmt):
    sh.check_one_row_at_zero_frequency_is_the_single_stage(eng, STAGE, (M,), ntaps, fmt, seed=100 * M + ntaps, sel=[0])


@pytest.mark.parametrize("M,ntaps", [(8, 155), (32, 31), (64, 65)])
def test_order_of_the_channel_list_and_unselected_rows_do_not_matter(eng, M, ntaps):
    rng = np.random.default_rng(300 + M)
    nin = sc.tile_inputs(M) + 301
    x = _rows(rng, M, nin)
    h = sc.taps_for(rng, ntaps)
    try:
        eng.set_pfb_synth(pfb.synth_cfg(M, None, taps=h))
        ref = eng.pfb_synth(x).copy()
        perm = [int(i) for i in rng.permutation(M)]
        assert perm != list(range(M))
        eng.set_pfb_synth(pfb.synth_cfg(M, perm, taps=h))
        assert np.array_equal(eng.pfb_synth(x[perm]).view(np.uint32), ref.view(np.uint32))
        # a subset gives the bits of the full list with the other rows zero
        sub = _subset(M)
        z = np.zeros_like(x)
        z[sub] = x[sub]
        eng.set_pfb_synth(pfb.synth_cfg(M, None, taps=h))
        full = eng.pfb_synth(z).copy()
        eng.set_pfb_synth(pfb.synth_cfg(M, [c - M if c >= M // 2 else c for c in sub], taps=h))     # the signed spelling
        got = eng.pfb_synth(x[sub])
        assert np.array_equal(got.view(np.uint32), full.view(np.uint32)) and np.any(full != 0)
    finally:
        eng.set_pfb_synth(None)


SEG_SHAPES = [(M, t) for M in (2, 8, 64) for t in (min(sc.TAP_GRID[M]), max(sc.TAP_GRID[M]))]


@pytest.mark.parametrize("fmt", ["fc32", "sc16"])
@pytest.mark.parametrize("M,ntaps", SEG_SHAPES)
def test_any_segmentation_gives_the_same_bits(eng, M, ntaps, fmt):
    sh.check_tx_bank_segmentation(eng, STAGE, (M,), ntaps, [M - 1, 0, M // 2][:min(M, 3)], fmt, seed=53 * M + ntaps,
                                  far=7 * 1024 + 5)


@pytest.mark.parametrize("M,ntaps", [(4, 31), (8, 155), (64, 155)])
def test_against_k_duc_passes_on_the_grid(eng, M, ntaps):
    """Same taps, L = M, fc = c / M, one Engine.duc(..., add=band) per link: the two ways differ by no more than the sum
    of their derived bounds (duc_cases.bound per pass, its `add` being the band so far)."""
    rng = np.random.default_rng(900 + M)
    chans = list(range(M)) if M <= 8 else [0, 1, 7, 31, 32, 33, 40, 63]
    nin = sc.stream_inputs(M)
    x = _rows(rng, len(chans), nin)
    h = sc.taps_for(rng, ntaps)
    try:
        eng.set_pfb_synth(pfb.synth_cfg(M, chans, taps=h))
        y = eng.pfb_synth(x).copy()
        _, s_terms = sc.model_terms(x, h, M, chans)
        bound = sc.bound(ntaps, M, s_terms.sum(axis=0))
        band = None
        for i, c in enumerate(chans):
            eng.set_duc(duc.duc_cfg(M, c / float(M) if c <= M // 2 else (c - M) / float(M), taps=h))
            bound = bound + duc_cases.bound(ntaps, M, s_terms[i], band)
            band = eng.duc(x[i], add=band).copy()
        err = np.abs(y.astype(np.complex128) - band.astype(np.complex128))
        print("M=%d ntaps=%d K=%d: worst |bank - DUC passes| / (sum of the bounds) = %.3g"
              % (M, ntaps, len(chans), float(np.max(err / bound))))
        assert np.all(err <= bound)
    finally:
        eng.set_pfb_synth(None)
        eng.set_duc(None)


@pytest.mark.parametrize("M,ntaps", [(4, 31), (32, 155)])
def test_add_is_one_float32_addition_per_part(eng, M, ntaps):
    rng = np.random.default_rng(40 + M)
    sel = [1, M - 1, 0]
    nin = sc.tile_inputs(M) + 77
    x = _rows(rng, 3, nin)
    h = sc.taps_for(rng, ntaps)
    band = _rows(rng, 1, nin * M, amp=3.0)[0]
    try:
        eng.set_pfb_synth(pfb.synth_cfg(M, sel, taps=h))
        v = eng.pfb_synth(x).copy()
        eng.pfb_synth_reset(0)
        got = eng.pfb_synth(x, add=band)
        want = (v.real + band.real).astype(np.float32) + 1j * (v.imag + band.imag).astype(np.float32)
        assert np.array_equal(got, want.astype(np.complex64))
        with pytest.raises(ValueError):
            eng.pfb_synth(x, add=band[:-1])
        # 16-bit output: the sum is quantised, not the parts
        eng.set_pfb_synth(pfb.synth_cfg(M, sel, taps=h, out_format="sc16", out_scale=1000.0))
        small = (band * np.float32(0.01)).astype(np.complex64)
        got = eng.pfb_synth(x, add=small)
        sum32 = (v.real + small.real).astype(np.float32) + 1j * (v.imag + small.imag).astype(np.float32)
        assert np.array_equal(got, iqio.to_sc16(sum32.astype(np.complex64), 1000.0))
    finally:
        eng.set_pfb_synth(None)


def test_in_device_mode_add_may_be_the_output_buffer():
    import torch
    sh.check_in_device_mode_add_may_be_the_output_buffer(torch, STAGE, (8,), [5, 0, 7], ntaps=155, nin=2 * sc.tile_inputs(8) + 77)


ROUND_TRIPS = [(name, M, chans, "fc32") for name, (M, chans) in sorted(pc.ON_GRID.items())] + [("bpsk64_r8", 8, (1, 6, 3), "sc16")]


@pytest.mark.parametrize("name,M,chans,fmt", ROUND_TRIPS, ids=["%s-%d-%s" % (r[0], len(r[2]), r[3]) for r in ROUND_TRIPS])
def test_round_trip_into_the_channeliser(name, M, chans, fmt):
    """ofdm_mod_channelizer -> the noise of duc_cases (30 dB inside a link's band) -> ofdm_demod_channelizer: every
    payload of every link returns with its CRC good, in order; the band the K DUC passes build decodes to the same."""
    mod, N, occ, CP, R, _, transition, plen = ddc_cases.CASES[name]
    assert R == M
    k = dict(mod=mod, N=N, occ=occ, CP=CP)
    opt = _options(k)
    K = len(chans)
    sent = [make_payloads(4 - (i % 2), plen, seed=11 + 18 * i) for i in range(K)]      # streams of unequal length
    tx_taps = pfb.synth_design(M, occ / float(N), transition)
    rx_taps = pfb.design(M, occ / float(N), transition)
    Q = (len(tx_taps) - 1) // M
    amp = 0.05
    tx = ofdm.ofdm_mod_channelizer(opt, M, chans, taps=tx_taps, iq_format=fmt)
    plain = [ofdm.ofdm_mod(opt) for _ in range(K)]
    try:
        assert tx.flush(end=True) is None and len(tx.links()) == K and tx.engine().pfb_synth_cfg.nsel == K
        for m in tx.links() + plain:
            m.engine().set_tx_amplitude(amp)
        for i, pays in enumerate(sent):
            for p in pays:
                tx.send_pkt(i, p)
                plain[i].send_pkt(p)
        band = tx.flush(end=True)
        # the same streams by hand: padded with zeros to a common length, then Q zero columns
        nb = [m.flush() for m in plain]
        n = max(len(v) for v in nb)
        assert min(len(v) for v in nb) < n
        P = float(np.mean(np.abs(nb[0]) ** 2))                             # one link's narrowband power
        x = np.zeros((K, n + Q), np.complex64)
        for i, v in enumerate(nb):
            x[i, :len(v)] = v
        assert len(band) == (n + Q) * M and band.dtype == (np.int16 if fmt == "sc16" else np.complex64)
        e = tx.engine()
        assert np.array_equal(e.pfb_synth(x), band)
        # ... and by K DUC passes, each added onto the band so far
        passes = None
        for i, c in enumerate(chans):
            e.set_duc(duc.duc_cfg(M, c / float(M) if c <= M // 2 else (c - M) / float(M), taps=tx_taps))
            passes = e.duc(x[i], add=passes).copy()
        e.set_duc(None)
        e.pfb_synth_reset(0)
        # two batches continue the band: what the first flush leaves in the filter comes out in front of the second.
        # The same batches through the plain modulators, padded per batch as flush() pads them, through the bank in
        # two calls and the Q zero columns: the same bits, split at the same place
        halves = []
        for part in (slice(0, 1), slice(1, None)):
            for i, pays in enumerate(sent):
                for p in pays[part]:
                    tx.send_pkt(i, p)
                    plain[i].send_pkt(p)
            halves.append((tx.flush(end=part.start == 1), [m.flush() for m in plain]))
        assert tx.flush() is None and tx.flush(end=True) is None       # nothing queued, nothing in flight
        for j, (got, nbj) in enumerate(halves):
            nj = max(len(v) for v in nbj)
            xj = np.zeros((K, nj + (Q if j == 1 else 0)), np.complex64)
            for i, v in enumerate(nbj):
                xj[i, :len(v)] = v
            want = e.pfb_synth(xj)
            assert got.dtype == want.dtype == band.dtype and len(got) == xj.shape[1] * M
            assert np.array_equal(_bits(got), _bits(want)), (name, j)
        e.pfb_synth_reset(0)
    finally:
        tx.close()
        for m in plain:
            m.engine().close()
    assert tx.engine()._h.value is None and all(m.engine()._h.value is None for m in tx.links())

    def capture(wide):
        wide = _c64(wide, fmt) if wide.dtype == np.int16 else wide.astype(np.complex128)
        w = np.concatenate([np.zeros(2 * N * M), wide, np.zeros(3 * N * M)])
        w = (w + duc_cases.noise(len(w), P, M)).astype(np.complex64)
        if fmt == "sc16":
            assert np.max(np.abs(w.real)) < 0.99 and np.max(np.abs(w.imag)) < 0.99
            return iqio.to_sc16(w)
        return w

    rx = ofdm.ofdm_demod_channelizer(opt, M, chans, taps=rx_taps, iq_format=fmt)
    try:
        for what, wide in (("bank", band), ("DUC passes", passes)):
            got = rx.work(capture(wide))
            for i in range(K):
                assert [ok for ok, _ in got[i]] == [True] * len(sent[i]), (name, what, i)
                assert [p for _, p in got[i]] == sent[i], (name, what, i)
    finally:
        rx.close()


def test_layout_and_capacity(eng):
    sh.check_tx_bank_layout_and_capacity(eng, STAGE, (4,), [3, 0, 1], pfb.synth_design(4, 0.4), nin=1500, one_sel=[0])


def test_invalid_arguments_are_refused(eng):
    base = lambda: pfb.synth_cfg(4, [1, 3], taps=np.ones(5, np.float32))
    sh.check_tx_bank_invalid_arguments(eng, STAGE, (4,), base, nout=64, still_refused=1, edge_sel=None)


def test_device_pointer_path_behind_an_asynchronous_transmit():
    """The bank's input is what tx_device(wait=False) is still producing on the same handle; its band goes straight to
    the channeliser, which returns the links."""
    import torch
    cfg = make_cfg()
    pays = make_payloads(4, 100, seed=7)
    M = 4
    tx_taps, rx_taps = pfb.synth_design(M, 200 / 512.0), pfb.design(M, 200 / 512.0)
    host = engine.Engine(cfg=cfg)
    dev = engine.Engine(cfg=make_cfg(device_ptrs=True))
    try:
        x = host.tx(pays)
        host.set_pfb_synth(pfb.synth_cfg(M, [3], taps=tx_taps))
        wide = host.pfb_synth(x[None])
        host.set_pfb(pfb.pfb_cfg(M, [3, 1], taps=rx_taps))
        want = host.pfb(wide)
        blob, offs, lens = engine.pack_payloads(pays)
        _, nsamp = dev.tx_frame_count(lens)
        assert nsamp == len(x) and want.shape == (2, nsamp)
        d_pay = torch.from_numpy(blob.copy()).cuda()
        d_iq = torch.zeros(nsamp, dtype=torch.complex64, device="cuda")
        d_wide = torch.zeros(nsamp * M, dtype=torch.complex64, device="cuda")
        d_out = torch.zeros((2, nsamp), dtype=torch.complex64, device="cuda")
        dev.set_pfb_synth(pfb.synth_cfg(M, [3], taps=tx_taps))
        dev.set_pfb(pfb.pfb_cfg(M, [3, 1], taps=rx_taps))
        torch.cuda.synchronize()
        assert dev.tx_device(d_pay.data_ptr(), offs, lens, d_iq.data_ptr(), nsamp, wait=False) == nsamp
        assert dev.pfb_synth_device(d_iq.data_ptr(), nsamp, nsamp, d_wide.data_ptr(), nsamp * M) == nsamp * M
        assert dev.pfb_device(d_wide.data_ptr(), nsamp * M, d_out.data_ptr(), nsamp, nsamp) == nsamp
        assert np.array_equal(d_wide.cpu().numpy(), wide)
        assert np.array_equal(d_out.cpu().numpy(), want)
        sh.zero(torch, d_pay, d_iq, d_wide, d_out)
        del d_pay, d_iq, d_wide, d_out
        torch.cuda.empty_cache()
    finally:
        host.close()
        dev.close()


def test_the_channeliser_the_duc_and_the_bank_do_not_disturb_each_other(eng):
    rng = np.random.default_rng(23)
    n = 9000
    raw = _rows(rng, 1, n, amp=1.0)[0]
    nb = _rows(rng, 3, 1100)
    t155, t31 = sc.taps_for(rng, 155), sc.taps_for(rng, 31)
    stages = {
        "pfb": (lambda: eng.set_pfb(pfb.pfb_cfg(8, [1, 6, 3], taps=t155)), lambda a, b: eng.pfb(raw[a:b]), n, 1777),
        "duc": (lambda: eng.set_duc(duc.duc_cfg(4, 0.25, taps=t31)), lambda a, b: eng.duc(nb[0, a:b])[None], 1100, 301),
        "pfb_synth": (lambda: eng.set_pfb_synth(pfb.synth_cfg(8, [6, 1, 3], taps=t155)),
                      lambda a, b: eng.pfb_synth(nb[:, a:b])[None], 1100, 211),
    }
    off = dict(pfb=eng.set_pfb, duc=eng.set_duc, pfb_synth=eng.set_pfb_synth)
    try:
        alone = sh.check_interleaved(stages, off)
        # dropping or resetting another stage leaves the bank's stream where it was, and the other way round
        eng.pfb_synth_reset(0)
        a = eng.pfb_synth(nb[:, :500]).copy()
        eng.pfb_reset(0)
        eng.duc_reset(5)
        eng.set_duc(None)
        b = eng.pfb_synth(nb[:, 500:])
        assert np.array_equal(np.concatenate([a, b])[None], alone["pfb_synth"])
        eng.pfb(raw[:100])
        eng.set_pfb_synth(None)
        assert eng.pfb_count(4) == pc.count(100, 4, 8)
    finally:
        for f in off.values():
            f(None)


def test_a_handle_that_dropped_the_bank_runs_what_it_ran(orc):
    """Two handles transmit and demodulate the same packets: one never saw the synthesis bank, the other used it and
    dropped it.  Same IQ bits, same packets, same per-kernel launch counts; the kernel table has no entry for the stage."""
    cap = ddc_cases.capture("qpsk512_r4")
    cfg = cap["cfg"]
    pays = cap["payloads"][0]
    a, b = engine.Engine(cfg=cfg), engine.Engine(cfg=cfg)
    try:
        a.set_pfb(pfb.pfb_cfg(4, [1, 3], taps=cap["taps"]))
        link = a.pfb(cap["wide"])[0].copy()
        a.set_pfb(None)
        b.set_pfb_synth(pfb.synth_cfg(4, [1, 3], occupied_fraction=200 / 512.0))
        b.pfb_synth(_rows(np.random.default_rng(2), 2, 3000))
        b.set_pfb_synth(None)
        for e in (a, b):
            e.prof_enable(True)
            e.prof_reset()
        ia, ib = a.tx(pays), b.tx(pays)
        assert np.array_equal(ia, ib)
        pa, pb = a.rx(link), b.rx(link)
        assert pa == pb and [p for ok, p in pa if ok] == pays
        ca = {k: v[1] for k, v in a.prof().items()}
        cb = {k: v[1] for k, v in b.prof().items()}
        assert ca == cb and sum(ca.values()) > 0
        assert len(ca) == _abi.K_COUNT == 11 and not any("pfb" in k for k in ca)
        # with the bank configured the transmitter's and receiver's own launches stay what they are, and the stage
        # reports its time
        b.set_pfb_synth(pfb.synth_cfg(4, [1, 3], occupied_fraction=200 / 512.0))
        b.prof_reset()
        a.prof_reset()
        with pytest.raises(ValueError):
            b.pfb_synth_last_ms()                         # no profiled call yet
        b.pfb_synth(np.stack([ib, ib]))
        assert b.pfb_synth_last_ms() > 0.0
        assert np.array_equal(b.tx(pays), a.tx(pays)) and b.rx(link) == a.rx(link) == pa
        assert {k: v[1] for k, v in b.prof().items()} == {k: v[1] for k, v in a.prof().items()}
    finally:
        a.close()
        b.close()
