"""The DUC bank on the GPU (k_duc_bank, Engine.duc_bank, ofdm_mod_bank): against the float64 model of its definition
within the derived bound, exact where it must be (one link is the DUC where the two definitions meet; segmentation; a
zero link; add; the 16-bit store; the table), against K DUC passes, end to end into the DDC bank, at its edges, and
beside the other stages."""
import ctypes as C
import functools

import numpy as np
import pytest

import ddc_cases
import duc_bank_cases as bc
import duc_cases
from helpers import make_cfg, make_payloads
from ofdm_uhd_amd import _abi, ddc, duc, engine, iqio, ofdm, options, pfb

pytestmark = pytest.mark.gpu

SCALE = 32768.0
AMP = 1.0 / 16.0
START = 1000003             # a first input index that is a multiple of no tile
FAR = (1 << 40) - 5         # ... and one near 2^40

# (K, ntaps) per interpolation: K in {1, 2, 3, 8}; ntaps 1, L - 1 (phases without a tap), 1024 at L = 1 and L = 64
MODEL_SHAPES = {
    1: [(8, 33), (2, 1024), (1, 1)],
    2: [(8, 25), (3, 1)],
    3: [(3, 50), (2, 2)],
    4: [(1, 31), (3, 31), (8, 3)],
    8: [(8, 155), (2, 7)],
    64: [(2, 1024), (3, 63), (8, 65), (1, 1)],
}


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
    return (iqio.from_sc16(out) if fmt == "sc16" else out).astype(np.complex128)


@functools.lru_cache(maxsize=None)
def _inputs(K, L, ntaps):
    """Computed once per shape and shared (read-only): the K streams, the taps, the frequencies and a band to add onto,
    scaled by a power of two so that the band stays inside the 16-bit range."""
    rng = np.random.default_rng(9000 + 1000 * K + 13 * L + ntaps)
    nin = bc.stream_inputs(L)
    x, h, fcs = _rows(rng, K, nin), bc.taps_for(rng, ntaps), tuple(bc.freqs(K))
    add = _rows(rng, 1, nin * L)[0]
    _, s = bc.model(x, h, L, fcs)
    g = np.float32(2.0 ** np.floor(np.log2(0.4 / max(float(np.max(s)), 1e-30))))      # |band| <= s <= 0.4, |add| small
    x = (x * min(g, np.float32(1.0))).astype(np.complex64)
    for a in (x, h, add):
        a.setflags(write=False)
    return x, h, fcs, add


@functools.lru_cache(maxsize=None)
def _reference(K, L, ntaps, first):
    x, h, fcs, _ = _inputs(K, L, ntaps)
    y, s = bc.model(x, h, L, fcs, first)
    y.setflags(write=False)
    s.setflags(write=False)
    return y, s


@pytest.mark.parametrize("with_add", [False, True], ids=["plain", "add"])
@pytest.mark.parametrize("fmt", ["fc32", "sc16"])
@pytest.mark.parametrize("L", sorted(MODEL_SHAPES))
def test_against_float64_model(eng, L, fmt, with_add):
    """Measured worst error / bound over all cases: see DESIGN.md section 7."""
    worst = 0.0
    try:
        for K, ntaps in MODEL_SHAPES[L]:
            x, h, fcs, add = _inputs(K, L, ntaps)
            nin = x.shape[1]
            assert (nin * L) % bc.tile_outputs(L) != 0
            eng.set_duc_bank(duc.bank_cfg(L, fcs, taps=h, out_format=fmt))
            for first in (0, START, FAR):
                y64, s = _reference(K, L, ntaps, first)
                want = y64 + (add.astype(np.complex128) if with_add else 0.0)
                bound = bc.bound(K, ntaps, L, s, add if with_add else None)
                if fmt == "sc16":
                    assert np.max(np.abs(want.real)) < 0.99 and np.max(np.abs(want.imag)) < 0.99  # nothing saturates
                eng.duc_bank_reset(first)
                out = eng.duc_bank(x, add=add if with_add else None)
                assert len(out) == nin * L and out.dtype == (np.int16 if fmt == "sc16" else np.complex64)
                if fmt == "sc16":                                  # per part: half a step of the 16-bit store
                    err, half = bc.sc16_error(_c64(out, fmt), want, SCALE)
                    bound_ = bound + half
                else:
                    err, bound_ = np.abs(_c64(out, fmt) - want), bound
                    assert np.all(out[bound == 0] == 0)            # a phase without a tap, nothing under the taps: 0
                ratio = float(np.max(err / np.maximum(bound_, 1e-300)))
                worst = max(worst, ratio)
                print("L=%d K=%d ntaps=%d first=%d %s%s: worst error / bound = %.3g"
                      % (L, K, ntaps, first, fmt, " add" if with_add else "", ratio))
                assert np.all(err <= bound_), (L, K, ntaps, first)
                assert np.any(out != 0)
    finally:
        eng.set_duc_bank(None)
    print("L=%d %s%s: worst error / bound over its cases = %.3g" % (L, fmt, " add" if with_add else "", worst))


SEG_SHAPES = [(1, 1024, 2), (2, 25, 8), (3, 2, 2), (4, 31, 3), (8, 155, 8), (64, 1024, 2), (64, 1, 1)]


@pytest.mark.parametrize("fmt", ["fc32", "sc16"])
@pytest.mark.parametrize("L,ntaps,K", SEG_SHAPES)
def test_any_segmentation_gives_the_same_bits(eng, L, ntaps, K, fmt):
    rng = np.random.default_rng(53 * L + ntaps)
    Ti, Q = max(bc.tile_outputs(L) // L, 1), bc.history(ntaps, L)
    nin = 3 * Ti + 100 + 3 * Q
    x, h, fcs = _rows(rng, K, nin), bc.taps_for(rng, ntaps), bc.freqs(K)
    band = _rows(rng, 1, nin * L)[0]
    try:
        eng.set_duc_bank(duc.bank_cfg(L, fcs, taps=h, out_format=fmt))
        for first, add in ((0, None), (FAR, band)):
            eng.duc_bank_reset(first)
            whole = eng.duc_bank(x, add=add).copy()
            assert len(whole) == nin * L and np.any(whole != 0)
            eng.duc_bank_reset(first)
            sizes = bc.chunk_inputs(rng, nin, L, ntaps)
            assert sum(sizes) == nin and {0, 1, Q + 1, Ti + 1} <= set(sizes) and (Ti - 1 in sizes or Ti == 1)
            assert (Q in sizes or Q == 0) and (Q - 1 in sizes or Q <= 1)
            parts, a = [], 0
            for n in sizes:
                y = eng.duc_bank(x[:, a:a + n], add=None if add is None else add[a * L:(a + n) * L])
                assert len(y) == n * L
                parts.append(y.copy())
                a += n
            got = np.concatenate(parts)
            assert got.dtype == whole.dtype and np.array_equal(_bits(got), _bits(whole)), (L, ntaps, K, first, fmt)
    finally:
        eng.set_duc_bank(None)


@pytest.mark.parametrize("fmt", ["fc32", "sc16"])
@pytest.mark.parametrize("L,ntaps", [(1, 1024), (2, 25), (3, 2), (4, 31), (8, 155), (64, 65)])
def test_one_link_at_zero_frequency_is_the_duc_at_zero_frequency(eng, L, ntaps, fmt):
    rng = np.random.default_rng(100 * L + ntaps)
    x = _rows(rng, 1, bc.stream_inputs(L))
    h = bc.taps_for(rng, ntaps)
    try:
        eng.set_duc_bank(duc.bank_cfg(L, [0.0], taps=h, out_format=fmt))
        eng.set_duc(duc.duc_cfg(L, 0.0, taps=h, out_format=fmt))
        for first in (0, START):
            eng.duc_bank_reset(first)
            eng.duc_reset(first)
            a, b = eng.duc_bank(x), eng.duc(x[0])
            assert a.shape == b.shape and a.dtype == b.dtype
            assert np.array_equal(a, b), (L, ntaps, fmt, first)          # as numbers: the sign of a zero may differ
        assert np.any(a != 0)
    finally:
        eng.set_duc_bank(None)
        eng.set_duc(None)


@pytest.mark.parametrize("L", [1, 4])
def test_one_link_with_the_unit_tap_is_the_duc_at_any_frequency(eng, L):
    """h = {1.0}: the table is (1, 0), the chain is one exact product, and what is left is r, the phase convention and
    the gr_complex product -- the DUC's, bit for bit, whatever fc and wherever the stream starts."""
    rng = np.random.default_rng(77 + L)
    x = _rows(rng, 1, bc.stream_inputs(L), amp=1.0)
    try:
        for fc in bc.freqs(8) + [-1e-20, 1.0 / 3.0]:
            eng.set_duc_bank(duc.bank_cfg(L, [fc], taps=[1.0]))
            eng.set_duc(duc.duc_cfg(L, fc, taps=[1.0]))
            for first in (0, START, FAR):
                eng.duc_bank_reset(first)
                eng.duc_reset(first)
                a, b = eng.duc_bank(x), eng.duc(x[0])
                assert np.array_equal(a, b) and np.any(a != 0), (L, fc, first)
    finally:
        eng.set_duc_bank(None)
        eng.set_duc(None)


@pytest.mark.parametrize("L,ntaps", [(4, 31), (1, 33), (64, 155)])
def test_a_link_of_zeros_changes_no_value(eng, L, ntaps):
    rng = np.random.default_rng(300 + L)
    nin = bc.stream_inputs(L)
    x, h = _rows(rng, 3, nin), bc.taps_for(rng, ntaps)
    z = np.zeros((1, nin), np.complex64)
    fcs = bc.freqs(3)
    try:
        eng.set_duc_bank(duc.bank_cfg(L, fcs, taps=h))
        ref = eng.duc_bank(x).copy()
        assert np.any(ref != 0)
        eng.set_duc_bank(duc.bank_cfg(L, fcs + [0.37], taps=h))
        assert np.array_equal(eng.duc_bank(np.concatenate([x, z])), ref)
        eng.set_duc_bank(duc.bank_cfg(L, [0.37] + fcs, taps=h))
        assert np.array_equal(eng.duc_bank(np.concatenate([z, x])), ref)
        # the order of the list is part of the configuration: the same links in another order are the same signal
        eng.set_duc_bank(duc.bank_cfg(L, fcs[::-1], taps=h))
        other = eng.duc_bank(x[::-1])
        _, s = bc.model(x, h, L, fcs)
        assert np.all(np.abs(other.astype(np.complex128) - ref.astype(np.complex128)) <= 2 * bc.bound(3, ntaps, L, s))
    finally:
        eng.set_duc_bank(None)


@pytest.mark.parametrize("L,ntaps", [(4, 31), (64, 155)])
def test_add_is_one_float32_addition_per_part_and_sc16_is_the_store_of_the_same_value(eng, L, ntaps):
    rng = np.random.default_rng(40 + L)
    nin = bc.stream_inputs(L)
    x, h, fcs = _rows(rng, 3, nin), bc.taps_for(rng, ntaps), bc.freqs(3)
    band = _rows(rng, 1, nin * L, amp=3.0)[0]
    try:
        eng.set_duc_bank(duc.bank_cfg(L, fcs, taps=h))
        v = eng.duc_bank(x).copy()
        eng.duc_bank_reset(0)
        got = eng.duc_bank(x, add=band)
        want = (v.real + band.real).astype(np.float32) + 1j * (v.imag + band.imag).astype(np.float32)
        assert np.array_equal(got, want.astype(np.complex64))
        with pytest.raises(ValueError):
            eng.duc_bank(x, add=band[:-1])
        # 16-bit output: the transmit rule on the same float32 value, and on the sum where there is an add
        for scale in (None, 1000.0):
            eng.set_duc_bank(duc.bank_cfg(L, fcs, taps=h, out_format="sc16", out_scale=scale))
            assert np.array_equal(eng.duc_bank(x), iqio.to_sc16(v, scale or SCALE))
            small = (band * np.float32(0.01)).astype(np.complex64)
            eng.duc_bank_reset(0)
            sum32 = (v.real + small.real).astype(np.float32) + 1j * (v.imag + small.imag).astype(np.float32)
            assert np.array_equal(eng.duc_bank(x, add=small), iqio.to_sc16(sum32.astype(np.complex64), scale or SCALE))
    finally:
        eng.set_duc_bank(None)


def test_table_is_the_ddc_banks():
    e = engine.Engine(cfg=make_cfg())
    try:
        rng = np.random.default_rng(8)
        h, fcs = bc.taps_for(rng, 155), bc.freqs(8)
        e.set_duc_bank(duc.bank_cfg(8, fcs, taps=h))
        e.set_ddc_bank(ddc.bank_cfg(8, fcs, taps=h))
        for i, fc in enumerate(fcs):
            t = e.duc_bank_taps(i)
            assert t.dtype == np.complex64 and len(t) == 155
            assert np.array_equal(t, e.ddc_bank_taps(i))
            # NumPy's table: the same float64 formula, another libm -- a last float64 bit may move one float32 rounding
            ref = ddc.bandpass_taps(h, fc)
            assert np.all(np.abs(t.astype(np.complex128) - ref.astype(np.complex128)) <= 2.0 ** -23 * np.abs(h)), i
            assert np.mean(t == ref) > 0.99
        assert np.array_equal(e.duc_bank_taps(2), h.astype(np.complex64))        # fc = 0: the taps themselves
        k = C.c_int(0)
        lib = _abi.load()
        for link in (8, 9, -1):
            assert lib.ofdm_duc_bank_taps(e._h, link, None, 0, C.byref(k)) == _abi.OFDM_E_INVAL
        assert lib.ofdm_duc_bank_taps(e._h, 7, None, 0, C.byref(k)) == _abi.OFDM_OK and k.value == 155
        small = np.zeros(100, np.complex64)
        assert lib.ofdm_duc_bank_taps(e._h, 7, small.ctypes.data_as(C.c_void_p), 100, C.byref(k)) == _abi.OFDM_E_CAPACITY
    finally:
        e.close()


@pytest.mark.parametrize("L,ntaps,K", [(4, 31, 2), (4, 31, 8), (8, 155, 8), (3, 50, 3), (1, 33, 8)])
def test_against_k_duc_passes(eng, L, ntaps, K):
    """Same taps and frequencies, one Engine.duc(..., add=band) per link: the two ways differ by no more than the sum
    of their derived bounds (duc_cases.bound per pass, its `add` being the band so far)."""
    rng = np.random.default_rng(900 + L + K)
    nin = bc.stream_inputs(L)
    x, h, fcs = _rows(rng, K, nin), bc.taps_for(rng, ntaps), bc.freqs(K)
    try:
        for first in (0, START):
            eng.set_duc_bank(duc.bank_cfg(L, fcs, taps=h))
            eng.duc_bank_reset(first)
            y = eng.duc_bank(x).copy()
            _, s_terms = bc.model_terms(x, h, L, fcs, first)
            bound = bc.bound(K, ntaps, L, s_terms.sum(axis=0))
            band = None
            for i, fc in enumerate(fcs):
                eng.set_duc(duc.duc_cfg(L, fc, taps=h))
                eng.duc_reset(first)
                bound = bound + duc_cases.bound(ntaps, L, s_terms[i], band)
                band = eng.duc(x[i], add=band).copy()
            err = np.abs(y.astype(np.complex128) - band.astype(np.complex128))
            print("L=%d ntaps=%d K=%d first=%d: worst |bank - DUC passes| / (sum of the bounds) = %.3g"
                  % (L, ntaps, K, first, float(np.max(err / np.maximum(bound, 1e-300)))))
            assert np.all(err <= bound) and np.any(y != 0)
    finally:
        eng.set_duc_bank(None)
        eng.set_duc(None)


def _zero(torch, *tensors):
    """Zero the test's device buffers before they are released: a later test's torch.empty() must not inherit this
    file's bytes."""
    for t in tensors:
        t.zero_()
    torch.cuda.synchronize()


def test_in_device_mode_add_may_be_the_output_buffer():
    import torch
    L, ntaps = 8, 155
    rng = np.random.default_rng(31)
    nin = bc.stream_inputs(L)
    stride = nin + 5
    fcs = bc.freqs(3)
    x = np.zeros((3, stride), np.complex64)
    x[:, :nin] = _rows(rng, 3, nin)
    band = _rows(rng, 1, nin * L)[0]
    h = bc.taps_for(rng, ntaps)
    host = engine.Engine(cfg=make_cfg())
    dev = engine.Engine(cfg=make_cfg(device_ptrs=True))
    try:
        for e in (host, dev):
            e.set_duc_bank(duc.bank_cfg(L, fcs, taps=h))
            e.prof_enable(True)
        with pytest.raises(ValueError):
            dev.duc_bank_last_ms()                       # no profiled call yet
        want = host.duc_bank(x[:, :nin], add=band)
        d_x = torch.from_numpy(x).cuda()
        d_out = torch.from_numpy(band.copy()).cuda()
        torch.cuda.synchronize()
        assert dev.duc_bank_device(d_x.data_ptr(), stride, nin, d_out.data_ptr(), nin * L, add_ptr=d_out.data_ptr()) == nin * L
        assert np.array_equal(d_out.cpu().numpy(), want)
        assert dev.duc_bank_last_ms() > 0.0 and host.duc_bank_last_ms() > 0.0
        # two halves through device pointers continue the stream
        dev.duc_bank_reset(0)
        d_out.copy_(torch.from_numpy(band))
        torch.cuda.synchronize()
        n1 = nin // 2 + 1
        a = dev.duc_bank_device(d_x.data_ptr(), stride, n1, d_out.data_ptr(), nin * L, add_ptr=d_out.data_ptr())
        b = dev.duc_bank_device(d_x.data_ptr() + 8 * n1, stride, nin - n1, d_out.data_ptr() + 8 * a, nin * L - a,
                                add_ptr=d_out.data_ptr() + 8 * a)
        assert a + b == nin * L and np.array_equal(d_out.cpu().numpy(), want)
        _zero(torch, d_x, d_out)
        del d_x, d_out
        torch.cuda.empty_cache()
    finally:
        host.close()
        dev.close()


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


@pytest.mark.parametrize("name,fmt", [("qpsk512_r4", "fc32"), ("qpsk512_r4", "sc16"), ("qpsk512_r3", "fc32"),
                                      ("qpsk512_r3", "sc16")])
def test_two_links_end_to_end_into_the_ddc_bank(name, fmt):
    """Engine.tx -> Engine.duc_bank (both links in one pass) -> the noise of duc_cases (30 dB inside a link's band) ->
    ofdm_demod_bank: every packet of both links returns CRC-ok with its payload; and the same through ofdm_mod_bank."""
    e = engine.Engine(cfg=make_cfg(*ddc_cases.CASES[name][:4]))
    try:
        k = duc_cases.links(name, tx=_engine_tx(e))
        R, x, fcs = k["R"], np.stack(k["x"]), list(k["freqs"])
        noise = duc_cases.noise(x.shape[1] * R, k["P"], R).astype(np.complex64)
        e.set_duc_bank(duc.bank_cfg(R, fcs, taps=k["tx_taps"], out_format=fmt))
        # the noise goes in as the band the links are added onto: the final store is the stage's own, 16-bit or not
        wide = e.duc_bank(x, add=noise).copy()
        assert len(wide) == x.shape[1] * R and wide.dtype == (np.int16 if fmt == "sc16" else np.complex64)
        if fmt == "sc16":
            assert int(wide.min()) > -32768 and int(wide.max()) < 32767, "a stored part sits on the rail"
    finally:
        e.close()
    opt = _options(k)
    rx = ofdm.ofdm_demod_bank(opt, fcs, R, taps=k["rx_taps"], iq_format=fmt)
    tx = ofdm.ofdm_mod_bank(opt, fcs, R, taps=k["tx_taps"], iq_format=fmt)
    try:
        got = rx.work(wide)
        for i in range(2):
            assert [ok for ok, _ in got[i]] == [True] * 4, (name, fmt, i)
            assert [p for _, p in got[i]] == k["payloads"][i], (name, fmt, i)
        # the modulator bank: the same payloads, the second link one packet short so that flush() pads it
        assert tx.flush(end=True) is None and len(tx.links()) == 2 and tx.engine().duc_bank_cfg.nlinks == 2
        sent = [k["payloads"][0], k["payloads"][1][:3]]
        plain = ofdm.ofdm_mod(opt)
        try:
            for m in tx.links() + [plain]:
                m.engine().set_tx_amplitude(0.05)          # two links and the noise stay inside the 16-bit range
            for p in sent[0]:
                plain.send_pkt(p)
            P = float(np.mean(np.abs(plain.flush()) ** 2))     # one link's narrowband power
        finally:
            plain.engine().close()
        for i, pays in enumerate(sent):
            for p in pays:
                tx.send_pkt(i, p)
        band = tx.flush(end=True)
        Q = (len(k["tx_taps"]) - 1) // R
        assert band.dtype == wide.dtype and len(band) % R == 0 and len(band) // R > Q
        N = k["N"]
        w = np.concatenate([np.zeros(2 * N * R), _c64(band, fmt), np.zeros(3 * N * R)])
        w = (w + duc_cases.noise(len(w), P, R)).astype(np.complex64)
        if fmt == "sc16":
            assert np.max(np.abs(w.real)) < 0.99 and np.max(np.abs(w.imag)) < 0.99
            w = iqio.to_sc16(w)
        got = rx.work(w)
        for i in range(2):
            assert [ok for ok, _ in got[i]] == [True] * len(sent[i]) and [p for _, p in got[i]] == sent[i], (name, fmt, i)
    finally:
        rx.close()
        tx.close()
    assert tx.engine()._h.value is None and all(m.engine()._h.value is None for m in tx.links())


def test_mod_bank_pads_tails_resets_and_drops_a_failing_batch():
    opt = options.default_options(modulation="qpsk", fft_length=512, occupied_tones=200, cp_length=128)
    L, fcs = 4, [0.25, -0.2371, 0.01]
    taps = duc.design(L, 200 / 512.0)
    Q = (len(taps) - 1) // L
    sent = [make_payloads(3 - (i % 2), 100, seed=11 + 18 * i) for i in range(3)]      # streams of unequal length
    tx = ofdm.ofdm_mod_bank(opt, fcs, L, taps=taps)
    plain = [ofdm.ofdm_mod(opt) for _ in range(3)]
    try:
        assert Q >= 2 and tx.flush() is None
        for i, pays in enumerate(sent):
            for p in pays:
                tx.send_pkt(i, p)
                plain[i].send_pkt(p)
        band = tx.flush(end=True)
        nb = [m.flush() for m in plain]
        n = max(len(v) for v in nb)
        assert min(len(v) for v in nb) < n
        x = np.zeros((3, n + Q), np.complex64)
        for i, v in enumerate(nb):
            x[i, :len(v)] = v
        e = tx.engine()
        assert len(band) == (n + Q) * L and np.array_equal(_bits(e.duc_bank(x)), _bits(band))      # ... and it had reset
        e.duc_bank_reset(0)
        # two batches continue the band; the tail comes with end=True
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
            xj = np.zeros((3, nj + (Q if j == 1 else 0)), np.complex64)
            for i, v in enumerate(nbj):
                xj[i, :len(v)] = v
            want = e.duc_bank(xj)
            assert len(got) == xj.shape[1] * L and np.array_equal(_bits(got), _bits(want)), j
        e.duc_bank_reset(0)
        # a failing batch (link 1 holds something the engine cannot frame) is dropped on ALL links, link 0's that was
        # already modulated and link 2's that was not yet; the band has not moved
        tx.send_pkt(0, sent[0][0])
        tx.links()[1]._pending.append(object())
        tx.send_pkt(2, sent[2][0])
        with pytest.raises(Exception):
            tx.flush()
        assert all(not m._pending for m in tx.links()) and tx.flush() is None and tx.flush(end=True) is None
        tx.send_pkt(0, sent[0][0])
        plain[0].send_pkt(sent[0][0])
        one = plain[0].flush()
        x1 = np.zeros((3, len(one)), np.complex64)
        x1[0] = one
        got = tx.flush().copy()
        e.duc_bank_reset(0)
        assert np.array_equal(_bits(got), _bits(e.duc_bank(x1))) and np.any(got != 0)
    finally:
        tx.close()
        for m in plain:
            m.engine().close()


def _raw(lib, h, x, stride, nin, out, cap, add=None):
    nn = C.c_uint64(0)
    rc = lib.ofdm_duc_bank(h, x.ctypes.data_as(C.c_void_p), stride, nin, None if add is None else add.ctypes.data_as(C.c_void_p),
                           out.ctypes.data_as(C.c_void_p), cap, C.byref(nn))
    return rc, nn.value


def test_layout_and_capacity(eng):
    lib = _abi.load()
    rng = np.random.default_rng(5)
    L, fcs, nin = 4, bc.freqs(3), 700
    x = _rows(rng, 3, nin)
    h = duc.design(L, 0.4)
    Q = (len(h) - 1) // L
    eng.set_duc_bank(duc.bank_cfg(L, fcs, taps=h))
    try:
        want = eng.duc_bank(x).copy()
        # link_stride > nin: the gaps are not read
        eng.duc_bank_reset(0)
        wide = np.full((3, nin + 13), np.complex64(np.nan), np.complex64)
        wide[:, :nin] = x
        out = np.zeros(nin * L, np.complex64)
        assert _raw(lib, eng._h, wide, nin + 13, nin, out, nin * L) == (_abi.OFDM_OK, nin * L)
        assert np.array_equal(out, want)
        # out_cap one short: refused with *nout set, and the stream does not move
        eng.duc_bank_reset(0)
        n1 = 401
        first = eng.duc_bank(x[:, :n1]).copy()
        rest_in = np.ascontiguousarray(x[:, n1:])
        n2 = nin - n1
        sentinel = np.complex64(-7.5 + 3.25j)
        out = np.full(n2 * L, sentinel, np.complex64)
        assert _raw(lib, eng._h, rest_in, n2, n2, out, n2 * L - 1) == (_abi.OFDM_E_CAPACITY, n2 * L)
        assert np.all(out == sentinel)
        # link_stride < nin with more than one link
        assert _raw(lib, eng._h, rest_in, n2 - 1, n2, out, n2 * L)[0] == _abi.OFDM_E_INVAL
        assert np.all(out == sentinel)
        rest = eng.duc_bank(rest_in)
        assert np.array_equal(np.concatenate([first, rest]), want)        # the stream continues bit for bit
        # calls of 0 and calls shorter than Q are part of the stream
        eng.duc_bank_reset(0)
        assert Q >= 2
        parts = [eng.duc_bank(x[:, a:b]).copy() for a, b in ((0, 0), (0, 1), (1, Q), (Q, Q), (Q, nin))]
        assert [len(p) for p in parts[:4]] == [0, L, (Q - 1) * L, 0] and np.array_equal(np.concatenate(parts), want)
        # one link: the stride does not matter
        eng.set_duc_bank(duc.bank_cfg(L, [fcs[1]], taps=h))
        one = eng.duc_bank(x[1]).copy()
        eng.duc_bank_reset(0)
        out = np.zeros(nin * L, np.complex64)
        assert _raw(lib, eng._h, np.ascontiguousarray(x[1]), 0, nin, out, nin * L) == (_abi.OFDM_OK, nin * L)
        assert np.array_equal(out, one)
    finally:
        eng.set_duc_bank(None)


def _raw_cfg(**kw):
    c = duc.bank_cfg(4, [0.2, -0.3], taps=np.ones(5, np.float32))
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_invalid_arguments_are_refused(eng):
    lib = _abi.load()
    eng.set_duc_bank(None)
    x = np.zeros((2, 16), np.complex64)
    x[:, ::3] = 1.0
    out = np.zeros(64, np.complex64)
    assert _raw(lib, eng._h, x, 16, 16, out, 64)[0] == _abi.OFDM_E_INVAL            # no configuration
    for call in (lambda: eng.duc_bank(x), lambda: eng.duc_bank_reset(0), lambda: eng.duc_bank_last_ms(),
                 lambda: eng.duc_bank_taps(0)):
        with pytest.raises(ValueError):
            call()
    good = _raw_cfg()
    eng.set_duc_bank(good)
    table = eng.duc_bank_taps(1)
    assert _raw(lib, eng._h, x, 16, 16, out, 64) == (_abi.OFDM_OK, 64)
    y = out.copy()
    bad_fc = []
    for v in (0.5000001, -0.51, float("nan"), float("inf")):
        c = _raw_cfg()
        c.center_freq[1] = v
        bad_fc.append(c)
    bad_tap = []
    for v in (float("nan"), float("inf")):
        c = _raw_cfg()
        c.taps[3] = v
        bad_tap.append(c)
    refused = [_raw_cfg(**b) for b in (dict(struct_size=12), dict(interpolation=0), dict(interpolation=65), dict(ntaps=0),
                                       dict(ntaps=1025), dict(nlinks=0), dict(nlinks=9), dict(out_format=2),
                                       dict(out_format=1, out_scale=-1.0), dict(out_format=1, out_scale=float("inf")))]
    refused += bad_fc + bad_tap
    for c in refused:
        with pytest.raises(ValueError) as info:
            eng.set_duc_bank(c)
        assert str(info.value)                            # each refusal has its message
        assert eng.duc_bank_cfg is good
    for c in refused:
        assert lib.ofdm_set_duc_bank(eng._h, C.byref(c)) == _abi.OFDM_E_INVAL
    c = _raw_cfg()
    c.center_freq[2] = 7.0                                # a frequency beyond nlinks is not looked at
    eng.set_duc_bank(c)
    eng.set_duc_bank(good)
    # a refused configuration leaves the one in force untouched: same table, same stream position, same outputs
    a = eng.duc_bank(x[:, :7]).copy()
    with pytest.raises(ValueError):
        eng.set_duc_bank(bad_fc[0])
    assert np.array_equal(eng.duc_bank_taps(1), table)
    b = eng.duc_bank(x[:, 7:])
    assert np.array_equal(np.concatenate([a, b]), y)
    # the ends of the frequency range are inside it
    eng.set_duc_bank(duc.bank_cfg(4, [0.5, -0.5], taps=np.ones(5, np.float32)))
    eng.set_duc_bank(good)
    # index limits: the DUC's, no output index past 2^63
    lim = (1 << 63) // 4
    eng.duc_bank_reset(lim)
    with pytest.raises(ValueError):
        eng.duc_bank_reset(lim + 1)
    assert _raw(lib, eng._h, x, 16, 1, out, 64)[0] == _abi.OFDM_E_INVAL              # one input more would pass it
    assert _raw(lib, eng._h, x, 16, 0, out, 64) == (_abi.OFDM_OK, 0)
    eng.duc_bank_reset(0)
    assert _raw(lib, eng._h, x, 1 << 62, 1 << 62, out, 64)[0] == _abi.OFDM_E_INVAL
    # a call too long for one grid: refused before anything is read or written, the stream stays where it was
    long_n = (1 << 31) * (bc.tile_outputs(4) // 4) + 1
    assert _raw(lib, eng._h, x, long_n, long_n, out, 1 << 62) == (_abi.OFDM_E_INVAL, long_n * 4)
    assert b"too long" in lib.ofdm_last_error(eng._h)
    assert _raw(lib, eng._h, x, 16, 16, out, 64) == (_abi.OFDM_OK, 64) and np.array_equal(out, y)
    eng.duc_bank_reset(0)
    # misaligned buffers: complex64 in, add and out on 8 bytes, 16-bit out on 4
    f = np.zeros(2 * 64 + 2, np.float32)
    nn = C.c_uint64(0)
    xp, op, odd = x.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), C.c_void_p(f.ctypes.data + 4)
    assert lib.ofdm_duc_bank(eng._h, odd, 0, 16, None, op, 64, C.byref(nn)) == _abi.OFDM_E_INVAL
    assert lib.ofdm_duc_bank(eng._h, xp, 16, 16, odd, op, 64, C.byref(nn)) == _abi.OFDM_E_INVAL
    assert lib.ofdm_duc_bank(eng._h, xp, 16, 16, None, odd, 64, C.byref(nn)) == _abi.OFDM_E_INVAL
    assert lib.ofdm_duc_bank(eng._h, xp, 16, 16, None, None, 64, C.byref(nn)) == _abi.OFDM_E_INVAL       # null iq_out
    assert lib.ofdm_duc_bank(eng._h, None, 16, 16, None, op, 64, C.byref(nn)) == _abi.OFDM_E_INVAL       # null iq_in
    assert lib.ofdm_duc_bank(eng._h, xp, 16, 16, None, op, 64, None) == _abi.OFDM_E_INVAL
    eng.set_duc_bank(_raw_cfg(out_format=1))
    try:
        q = np.zeros(2 * 64 + 2, np.int16)
        assert lib.ofdm_duc_bank(eng._h, xp, 16, 16, None, C.c_void_p(q.ctypes.data + 2), 64, C.byref(nn)) == _abi.OFDM_E_INVAL
        assert lib.ofdm_duc_bank(eng._h, xp, 16, 16, None, C.c_void_p(q.ctypes.data + 4), 64, C.byref(nn)) == _abi.OFDM_OK
        assert np.array_equal(q[2:130].reshape(-1, 2), iqio.to_sc16(y))               # ... and the stream had not moved
    finally:
        eng.set_duc_bank(None)
    assert _raw(lib, eng._h, x, 16, 16, out, 64)[0] == _abi.OFDM_E_INVAL            # ... and after it was dropped


def test_device_pointer_path_behind_an_asynchronous_transmit():
    """The bank's input is what tx_device(wait=False) is still producing on the same handle."""
    import torch
    pays = make_payloads(4, 100, seed=7)
    L, fcs = 4, [0.25, -0.2371]
    taps = duc.design(L, 200 / 512.0)
    host = engine.Engine(cfg=make_cfg())
    dev = engine.Engine(cfg=make_cfg(device_ptrs=True))
    try:
        x = host.tx(pays)
        host.set_duc_bank(duc.bank_cfg(L, fcs, taps=taps))
        # the two links are the two halves of the buffer the transmitter fills
        nin = len(x) // 2
        wide = host.duc_bank(np.stack([x[:nin], x[nin:2 * nin]]))
        blob, offs, lens = engine.pack_payloads(pays)
        _, nsamp = dev.tx_frame_count(lens)
        assert nsamp == len(x)
        d_pay = torch.from_numpy(blob.copy()).cuda()
        d_iq = torch.zeros(nsamp, dtype=torch.complex64, device="cuda")
        d_wide = torch.zeros(nin * L, dtype=torch.complex64, device="cuda")
        dev.set_duc_bank(duc.bank_cfg(L, fcs, taps=taps))
        torch.cuda.synchronize()
        assert dev.tx_device(d_pay.data_ptr(), offs, lens, d_iq.data_ptr(), nsamp, wait=False) == nsamp
        assert dev.duc_bank_device(d_iq.data_ptr(), nin, nin, d_wide.data_ptr(), nin * L) == nin * L
        assert np.array_equal(d_wide.cpu().numpy(), wide) and np.any(wide != 0)
        _zero(torch, d_pay, d_iq, d_wide)
        del d_pay, d_iq, d_wide
        torch.cuda.empty_cache()
    finally:
        host.close()
        dev.close()


def test_the_bank_the_duc_and_the_synthesis_bank_do_not_disturb_each_other(eng):
    rng = np.random.default_rng(23)
    nb = _rows(rng, 3, 1100)
    t155, t31 = bc.taps_for(rng, 155), bc.taps_for(rng, 31)
    stages = {
        "duc_bank": (lambda: eng.set_duc_bank(duc.bank_cfg(8, bc.freqs(3), taps=t155)),
                     lambda a, b: eng.duc_bank(nb[:, a:b])[None], 1100, 177),
        "duc": (lambda: eng.set_duc(duc.duc_cfg(4, 0.25, taps=t31)), lambda a, b: eng.duc(nb[0, a:b])[None], 1100, 301),
        "pfb_synth": (lambda: eng.set_pfb_synth(pfb.synth_cfg(8, [6, 1, 3], taps=t155)),
                      lambda a, b: eng.pfb_synth(nb[:, a:b])[None], 1100, 211),
    }
    off = dict(duc_bank=eng.set_duc_bank, duc=eng.set_duc, pfb_synth=eng.set_pfb_synth)
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
        # dropping or resetting another stage leaves the bank's stream where it was
        eng.duc_bank_reset(0)
        a = eng.duc_bank(nb[:, :500]).copy()
        eng.pfb_synth_reset(0)
        eng.duc_reset(5)
        eng.set_duc(None)
        eng.set_pfb_synth(None)
        b = eng.duc_bank(nb[:, 500:])
        assert np.array_equal(np.concatenate([a, b])[None], alone["duc_bank"])
    finally:
        for f in off.values():
            f(None)


def test_a_handle_that_dropped_the_bank_launches_what_it_launched():
    """Two handles transmit the same packets: one never saw the bank, the other used it and dropped it.  Same IQ bits,
    same per-kernel launch counts; the kernel table has no entry for the stage."""
    pays = make_payloads(3, 100, seed=3)
    a, b = engine.Engine(cfg=make_cfg()), engine.Engine(cfg=make_cfg())
    try:
        b.set_duc_bank(duc.bank_cfg(4, [0.2, -0.3], occupied_fraction=200 / 512.0))
        b.duc_bank(_rows(np.random.default_rng(2), 2, 3000))
        b.set_duc_bank(None)
        for e in (a, b):
            e.prof_enable(True)
            e.prof_reset()
        ia, ib = a.tx(pays), b.tx(pays)
        assert np.array_equal(ia, ib)
        ca = {k: v[1] for k, v in a.prof().items()}
        cb = {k: v[1] for k, v in b.prof().items()}
        assert ca == cb and sum(ca.values()) > 0
        assert len(ca) == _abi.K_COUNT == 11 and not any("duc" in k for k in ca)
    finally:
        a.close()
        b.close()
