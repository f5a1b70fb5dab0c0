"""The polyphase-FFT synthesis bank on the GPU (k_pfb_synth, Engine.pfb_synth, ofdm_mod_channelizer): against the float64
model of its definition within the derived bound, exact where it must be (channel 0 alone is the DUC at fc = 0),
independent of the order of the selection and of the segmentation, against K DUC passes, end to end into the
channeliser, at its edges, and beside the other stages."""
import ctypes as C
import functools

import numpy as np
import pytest

import ddc_cases
import duc_cases
import pfb_cases as pc
import pfb_synth_cases as sc
from helpers import make_cfg, make_payloads
from ofdm_uhd_amd import _abi, duc, engine, iqio, ofdm, options, pfb

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
SCALE = 32768.0
AMP = 1.0 / 16.0           # keeps every band of these tests inside the 16-bit range (asserted where it matters)
START = 1000003            # a first input index that is a multiple of no tile


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(cfg=make_cfg())
    yield e
    e.close()


def _rows(rng, K, n, amp=AMP):
    return (amp * (rng.standard_normal((K, n)) + 1j * rng.standard_normal((K, n)))).astype(np.complex64)


def _bits(a):
    """The stored bits: -0 and +0 differ (int16 samples compare as they are)."""
    return a.view(np.uint32) if a.dtype == np.complex64 else a


def _c64(out, fmt):
    """The stage's output as complex128 samples."""
    return (iqio.from_sc16(out) if fmt == "sc16" else out).astype(np.complex128)


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
    rng = np.random.default_rng(100 * M + ntaps)
    x = _rows(rng, 1, sc.stream_inputs(M))
    h = sc.taps_for(rng, ntaps)
    try:
        eng.set_pfb_synth(pfb.synth_cfg(M, [0], taps=h, out_format=fmt))
        eng.set_duc(duc.duc_cfg(M, 0.0, taps=h, out_format=fmt))
        for first in (0, START):
            eng.pfb_synth_reset(first)
            eng.duc_reset(first)
            a, b = eng.pfb_synth(x), eng.duc(x[0])
            assert a.shape == b.shape and a.dtype == b.dtype
            assert np.array_equal(a, b), (M, ntaps, fmt, first)          # as numbers: the sign of a zero may differ
        assert np.any(a != 0)
    finally:
        eng.set_pfb_synth(None)
        eng.set_duc(None)


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
    rng = np.random.default_rng(53 * M + ntaps)
    T, Q = sc.tile_inputs(M), sc.history(ntaps, M)
    nin = 3 * T + 100 + 3 * Q
    sel = [M - 1, 0, M // 2][:min(M, 3)]
    K = len(sel)
    x = _rows(rng, K, nin)
    h = sc.taps_for(rng, ntaps)
    band = _rows(rng, 1, nin * M)[0]
    try:
        eng.set_pfb_synth(pfb.synth_cfg(M, sel, taps=h, out_format=fmt))
        for first, add in ((0, None), (7 * 1024 + 5, band)):
            eng.pfb_synth_reset(first)
            whole = eng.pfb_synth(x, add=add).copy()
            assert len(whole) == nin * M
            eng.pfb_synth_reset(first)
            sizes = sc.chunk_inputs(rng, nin, M, ntaps)
            assert sum(sizes) == nin and {0, 1, Q + 1, T - 1, T + 1} <= set(sizes)
            assert (Q in sizes or Q == 0) and (Q - 1 in sizes or Q <= 1)
            parts, a = [], 0
            for n in sizes:
                y = eng.pfb_synth(x[:, a:a + n], add=None if add is None else add[a * M:(a + n) * M])
                assert len(y) == n * M
                parts.append(y.copy())
                a += n
            got = np.concatenate(parts)
            assert got.dtype == whole.dtype and np.array_equal(_bits(got), _bits(whole)), (M, ntaps, first, fmt)
    finally:
        eng.set_pfb_synth(None)


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


def _zero(torch, *tensors):
    """Zero the test's device buffers before they are released: a later test's torch.empty() must not inherit this
    file's bytes."""
    for t in tensors:
        t.zero_()
    torch.cuda.synchronize()


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
    M, sel, ntaps = 8, [5, 0, 7], 155
    rng = np.random.default_rng(31)
    nin = 2 * sc.tile_inputs(M) + 77
    stride = nin + 5
    x = np.zeros((3, stride), np.complex64)
    x[:, :nin] = _rows(rng, 3, nin)
    band = _rows(rng, 1, nin * M)[0]
    h = sc.taps_for(rng, ntaps)
    host = engine.Engine(cfg=make_cfg())
    dev = engine.Engine(cfg=make_cfg(device_ptrs=True))
    try:
        for e in (host, dev):
            e.set_pfb_synth(pfb.synth_cfg(M, sel, taps=h))
            e.prof_enable(True)
        with pytest.raises(ValueError):
            dev.pfb_synth_last_ms()                       # no profiled call yet
        want = host.pfb_synth(x[:, :nin], add=band)
        d_x = torch.from_numpy(x).cuda()
        d_out = torch.from_numpy(band.copy()).cuda()
        torch.cuda.synchronize()
        assert dev.pfb_synth_device(d_x.data_ptr(), stride, nin, d_out.data_ptr(), nin * M, add_ptr=d_out.data_ptr()) == nin * M
        assert np.array_equal(d_out.cpu().numpy(), want)
        assert dev.pfb_synth_last_ms() > 0.0 and host.pfb_synth_last_ms() > 0.0
        # two halves through device pointers continue the stream
        dev.pfb_synth_reset(0)
        d_out.copy_(torch.from_numpy(band))
        torch.cuda.synchronize()
        n1 = nin // 2 + 1
        a = dev.pfb_synth_device(d_x.data_ptr(), stride, n1, d_out.data_ptr(), nin * M, add_ptr=d_out.data_ptr())
        b = dev.pfb_synth_device(d_x.data_ptr() + 8 * n1, stride, nin - n1, d_out.data_ptr() + 8 * a, nin * M - a,
                                 add_ptr=d_out.data_ptr() + 8 * a)
        assert a + b == nin * M and np.array_equal(d_out.cpu().numpy(), want)
        _zero(torch, d_x, d_out)
        del d_x, d_out
        torch.cuda.empty_cache()
    finally:
        host.close()
        dev.close()


def _options(k):
    return options.default_options(modulation=k["mod"], fft_length=k["N"], occupied_tones=k["occ"], cp_length=k["CP"])


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


def _raw(lib, h, x, stride, nin, out, cap, add=None):
    nn = C.c_uint64(0)
    rc = lib.ofdm_pfb_synth(h, x.ctypes.data_as(C.c_void_p), stride, nin, None if add is None else add.ctypes.data_as(C.c_void_p),
                            out.ctypes.data_as(C.c_void_p), cap, C.byref(nn))
    return rc, nn.value


def test_layout_and_capacity(eng):
    lib = _abi.load()
    rng = np.random.default_rng(5)
    M, sel, nin = 4, [3, 0, 1], 1500
    x = _rows(rng, 3, nin)
    h = pfb.synth_design(M, 0.4)
    Q = (len(h) - 1) // M
    eng.set_pfb_synth(pfb.synth_cfg(M, sel, taps=h))
    try:
        want = eng.pfb_synth(x).copy()
        # chan_stride > nin: the gaps are not read
        eng.pfb_synth_reset(0)
        wide = np.full((3, nin + 13), np.complex64(np.nan), np.complex64)
        wide[:, :nin] = x
        out = np.zeros(nin * M, np.complex64)
        assert _raw(lib, eng._h, wide, nin + 13, nin, out, nin * M) == (_abi.OFDM_OK, nin * M)
        assert np.array_equal(out, want)
        # out_cap one short: refused with *nout set, and the stream does not move
        eng.pfb_synth_reset(0)
        n1 = 401
        first = eng.pfb_synth(x[:, :n1]).copy()
        rest_in = np.ascontiguousarray(x[:, n1:])
        n2 = nin - n1
        sentinel = np.complex64(-7.5 + 3.25j)
        out = np.full(n2 * M, sentinel, np.complex64)
        assert _raw(lib, eng._h, rest_in, n2, n2, out, n2 * M - 1) == (_abi.OFDM_E_CAPACITY, n2 * M)
        assert np.all(out == sentinel)
        # chan_stride < nin with more than one channel
        assert _raw(lib, eng._h, rest_in, n2 - 1, n2, out, n2 * M)[0] == _abi.OFDM_E_INVAL
        assert np.all(out == sentinel)
        rest = eng.pfb_synth(rest_in)
        assert np.array_equal(np.concatenate([first, rest]), want)        # the stream continues bit for bit
        # calls of 0 and calls shorter than Q are part of the stream
        eng.pfb_synth_reset(0)
        assert Q >= 2
        parts = [eng.pfb_synth(x[:, a:b]).copy() for a, b in ((0, 0), (0, 1), (1, Q), (Q, Q), (Q, nin))]
        assert [len(p) for p in parts[:4]] == [0, M, (Q - 1) * M, 0] and np.array_equal(np.concatenate(parts), want)
        # one channel: the stride does not matter
        eng.set_pfb_synth(pfb.synth_cfg(M, [0], taps=h))
        one = eng.pfb_synth(x[1]).copy()
        eng.pfb_synth_reset(0)
        out = np.zeros(nin * M, np.complex64)
        assert _raw(lib, eng._h, np.ascontiguousarray(x[1]), 0, nin, out, nin * M) == (_abi.OFDM_OK, nin * M)
        assert np.array_equal(out, one)
    finally:
        eng.set_pfb_synth(None)


def _raw_cfg(**kw):
    c = pfb.synth_cfg(4, [1, 3], taps=np.ones(5, np.float32))
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_invalid_arguments_are_refused(eng):
    lib = _abi.load()
    eng.set_pfb_synth(None)
    x = np.zeros((2, 16), np.complex64)
    x[:, ::3] = 1.0
    out = np.zeros(64, np.complex64)
    assert _raw(lib, eng._h, x, 16, 16, out, 64)[0] == _abi.OFDM_E_INVAL            # no configuration
    for call in (lambda: eng.pfb_synth(x), lambda: eng.pfb_synth_reset(0), lambda: eng.pfb_synth_last_ms()):
        with pytest.raises(ValueError):
            call()
    good = _raw_cfg()
    eng.set_pfb_synth(good)
    assert _raw(lib, eng._h, x, 16, 16, out, 64) == (_abi.OFDM_OK, 64)
    y = out.copy()
    bad_chan, twice = _raw_cfg(), _raw_cfg()
    bad_chan.channel[1] = 4
    twice.channel[1] = 1
    bad_tap = []
    for v in (float("nan"), float("inf")):
        c = _raw_cfg()
        c.taps[3] = v
        bad_tap.append(c)
    refused = [_raw_cfg(**b) for b in (dict(struct_size=12), dict(nchannels=0), dict(nchannels=1), dict(nchannels=3),
                                       dict(nchannels=128), dict(ntaps=0), dict(ntaps=1025), dict(nsel=0), dict(nsel=5),
                                       dict(out_format=2), dict(out_format=1, out_scale=-1.0),
                                       dict(out_format=1, out_scale=float("inf")))]
    refused += [bad_chan, twice] + bad_tap
    for c in refused:
        with pytest.raises(ValueError) as info:
            eng.set_pfb_synth(c)
        assert str(info.value)                            # each refusal has its message
        assert eng.pfb_synth_cfg is good
    for c in refused:
        assert lib.ofdm_set_pfb_synth(eng._h, C.byref(c)) == _abi.OFDM_E_INVAL
    c = _raw_cfg()
    c.channel[2] = 200                                    # a channel beyond nsel is not looked at
    eng.set_pfb_synth(c)
    eng.set_pfb_synth(good)
    # a refused configuration leaves the one in force untouched: same stream position, same outputs
    a = eng.pfb_synth(x[:, :7]).copy()
    with pytest.raises(ValueError):
        eng.set_pfb_synth(twice)
    b = eng.pfb_synth(x[:, 7:])
    assert np.array_equal(np.concatenate([a, b]), y)
    # index limits: the DUC's, no output index past 2^63
    lim = (1 << 63) // 4
    eng.pfb_synth_reset(lim)
    with pytest.raises(ValueError):
        eng.pfb_synth_reset(lim + 1)
    assert _raw(lib, eng._h, x, 16, 1, out, 64)[0] == _abi.OFDM_E_INVAL              # one input more would pass it
    assert _raw(lib, eng._h, x, 16, 0, out, 64) == (_abi.OFDM_OK, 0)
    eng.pfb_synth_reset(lim - 16)
    assert _raw(lib, eng._h, x, 16, 16, out, 64) == (_abi.OFDM_OK, 64) and np.array_equal(out, y)
    eng.pfb_synth_reset(0)
    assert _raw(lib, eng._h, x, 1 << 62, 1 << 62, out, 64)[0] == _abi.OFDM_E_INVAL
    # a call too long for one grid (more than 2^31 - 1 tiles of 4096 / M input indices): refused before anything is
    # read or written, the stream stays where it was
    long_n = (1 << 31) * sc.tile_inputs(4) + 1
    assert _raw(lib, eng._h, x, long_n, long_n, out, 1 << 62) == (_abi.OFDM_E_INVAL, long_n * 4)
    assert b"too long" in lib.ofdm_last_error(eng._h)
    assert _raw(lib, eng._h, x, 16, 16, out, 64) == (_abi.OFDM_OK, 64) and np.array_equal(out, y)
    eng.pfb_synth_reset(0)
    # misaligned buffers: complex64 in, add and out on 8 bytes, 16-bit out on 4
    f = np.zeros(2 * 64 + 2, np.float32)
    nn = C.c_uint64(0)
    xp, op, odd = x.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), C.c_void_p(f.ctypes.data + 4)
    assert lib.ofdm_pfb_synth(eng._h, odd, 0, 16, None, op, 64, C.byref(nn)) == _abi.OFDM_E_INVAL
    assert lib.ofdm_pfb_synth(eng._h, xp, 16, 16, odd, op, 64, C.byref(nn)) == _abi.OFDM_E_INVAL
    assert lib.ofdm_pfb_synth(eng._h, xp, 16, 16, None, odd, 64, C.byref(nn)) == _abi.OFDM_E_INVAL
    assert lib.ofdm_pfb_synth(eng._h, xp, 16, 16, None, None, 64, C.byref(nn)) == _abi.OFDM_E_INVAL       # null iq_out
    assert lib.ofdm_pfb_synth(eng._h, None, 16, 16, None, op, 64, C.byref(nn)) == _abi.OFDM_E_INVAL       # null iq_in
    assert lib.ofdm_pfb_synth(eng._h, xp, 16, 16, None, op, 64, None) == _abi.OFDM_E_INVAL
    eng.set_pfb_synth(_raw_cfg(out_format=1))
    try:
        q = np.zeros(2 * 64 + 2, np.int16)
        assert lib.ofdm_pfb_synth(eng._h, xp, 16, 16, None, C.c_void_p(q.ctypes.data + 2), 64, C.byref(nn)) == _abi.OFDM_E_INVAL
        assert lib.ofdm_pfb_synth(eng._h, xp, 16, 16, None, C.c_void_p(q.ctypes.data + 4), 64, C.byref(nn)) == _abi.OFDM_OK
        assert np.array_equal(q[2:130].reshape(-1, 2), iqio.to_sc16(y))               # ... and the stream had not moved
    finally:
        eng.set_pfb_synth(None)
    assert _raw(lib, eng._h, x, 16, 16, out, 64)[0] == _abi.OFDM_E_INVAL            # ... and after it was dropped


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
        _zero(torch, d_pay, d_iq, d_wide, d_out)
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
        alone = {}
        for name, (cfg, run, total, _) in stages.items():
            cfg()
            alone[name] = run(0, total).copy()
            off[name](None)
        for cfg, _, _, _ in stages.values():
            cfg()
        parts = {name: [] for name in stages}
        pos = {name: 0 for name in stages}
        while any(pos[name] < stages[name][2] for name in stages):
            for name, (_, run, total, step) in stages.items():
                if pos[name] < total:
                    parts[name].append(run(pos[name], min(pos[name] + step, total)).copy())
                    pos[name] += step
        for name in stages:
            assert np.array_equal(np.concatenate(parts[name], axis=1), alone[name]), name
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
