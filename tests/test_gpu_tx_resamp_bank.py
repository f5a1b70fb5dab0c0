"""The transmit resampler bank on the GPU (k_tx_resamp_bank, Engine.tx_resamp_bank, ofdm_mod_resamp_bank): against the
float64 model of its definition within the derived bound, exact where it must be (one link is the single stage where
the two definitions meet; segmentation; a zero link; add; the 16-bit store; the table), against K passes of the single
stage, end to end into the receive bank at the mirror ratio, at its edges, and beside the other stages."""
import ctypes as C
import functools

import numpy as np
import pytest

import tx_resamp_bank_cases as bc
import tx_resamp_cases as cases
from helpers import make_cfg, make_payloads
from ofdm_uhd_amd import (_abi, benchmark_ofdm_rx, benchmark_ofdm_tx, duc, engine, iqio, ofdm, options, pfb, resample,
                          tx_resample)

pytestmark = pytest.mark.gpu

SCALE = 32768.0
AMP = 1.0 / 16.0
START = 1000003             # a first input index that is a multiple of no tile
FAR = (1 << 40) - 5         # ... and one near 2^40
assert (0, START, FAR) == bc.FIRSTS

# (L, M, ntaps, K)
MODEL_SHAPES = [(5, 2, 39, 2), (25, 8, 481, 8), (3, 4, 50, 3), (1, 1, 33, 8), (64, 63, 1024, 2), (2, 5, 25, 4),
                (4, 6, 31, 8), (7, 64, 200, 3), (1, 64, 1024, 2)]
SEG_SHAPES = [(5, 2, 39, 2), (25, 8, 481, 8), (64, 63, 1024, 2), (2, 5, 25, 8), (64, 1, 1, 1)]
# frequencies with turns(fc) = M turns(fc / M) exactly for every M that is a power of two: both signs, zero, the edges
DYADIC = [0.1875, -0.3125, 0.0, 0.5, -0.0625, 0.4375, -0.5, 0.25]


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


def _same_phase_per_output(fc, L, M):
    """The single stage's phase step per output is the bank's: both float64 models coincide."""
    return tx_resample.phase_step(fc) == tx_resample.bank_phase_steps(fc, L, M)[2]


@functools.lru_cache(maxsize=None)
def _inputs(L, M, ntaps, K):
    """Computed once per shape and shared (read-only): the K streams, the taps, the frequencies and a band to add onto
    (one sample longer than any call's output), scaled by a power of two so that the band stays inside the 16-bit
    range."""
    rng = np.random.default_rng(9000 + 1000 * K + 13 * L + 7 * M + ntaps)
    nin = bc.stream_inputs(L, M)
    x, h, fcs = _rows(rng, K, nin), bc.taps_for(rng, ntaps), tuple(bc.freqs(K))
    add = _rows(rng, 1, cases.count(0, nin, L, M) + 1)[0]
    _, s = bc.model(x, h, L, M, fcs)
    g = np.float32(2.0 ** np.floor(np.log2(0.3 / max(float(np.max(s)), 1e-30))))      # |band| <= s <= 0.3, |add| small
    x = (x * min(g, np.float32(1.0))).astype(np.complex64)
    for a in (x, h, add):
        a.setflags(write=False)
    return x, h, fcs, add


@functools.lru_cache(maxsize=None)
def _reference(L, M, ntaps, K, first):
    x, h, fcs, _ = _inputs(L, M, ntaps, K)
    y, s = bc.model(x, h, L, M, fcs, first)
    y.setflags(write=False)
    s.setflags(write=False)
    return y, s


@pytest.mark.parametrize("with_add", [False, True], ids=["plain", "add"])
@pytest.mark.parametrize("fmt", ["fc32", "sc16"])
@pytest.mark.parametrize("L,M,ntaps,K", MODEL_SHAPES)
def test_against_float64_model(eng, L, M, ntaps, K, fmt, with_add):
    """Measured worst error / bound over all cases: see DESIGN.md section 7."""
    x, h, fcs, add_all = _inputs(L, M, ntaps, K)
    nin = x.shape[1]
    assert nin % bc.tile_inputs(L, M) != 0 and (M == 1 or nin % M != 0)
    worst = 0.0
    try:
        eng.set_tx_resamp_bank(tx_resample.bank_cfg(L, M, fcs, taps=h, out_format=fmt))
        for first in bc.FIRSTS:
            y64, s = _reference(L, M, ntaps, K, first)
            no = cases.count(first, nin, L, M)
            assert len(y64) == no > 0
            add = add_all[:no] if with_add else None
            want = y64 + (add.astype(np.complex128) if with_add else 0.0)
            bound = bc.bound(K, ntaps, L, s, add)
            if fmt == "sc16":
                assert np.max(np.abs(want.real)) < 0.99 and np.max(np.abs(want.imag)) < 0.99  # nothing saturates
            eng.tx_resamp_bank_reset(first)
            assert eng.tx_resamp_bank_count(nin) == no
            out = eng.tx_resamp_bank(x, add=add)
            assert len(out) == no and out.dtype == (np.int16 if fmt == "sc16" else np.complex64)
            if fmt == "sc16":                                  # per part: half a step of the 16-bit store
                err, half = bc.sc16_error(_c64(out, fmt), want, SCALE)
                bound_ = bound + half
            else:
                err, bound_ = np.abs(_c64(out, fmt) - want), bound
                assert np.all(out[bound == 0] == 0)            # a phase without a tap, nothing under the taps: 0
            ratio = float(np.max(err / np.maximum(bound_, 1e-300)))
            worst = max(worst, ratio)
            assert np.all(err <= bound_), (L, M, ntaps, K, first, ratio)
            assert np.any(out != 0)
    finally:
        eng.set_tx_resamp_bank(None)
    print("%d/%d ntaps=%d K=%d %s%s: worst error / bound over its starts = %.3g"
          % (L, M, ntaps, K, fmt, " add" if with_add else "", worst))


@pytest.mark.parametrize("fmt", ["fc32", "sc16"])
@pytest.mark.parametrize("L,M,ntaps,K", SEG_SHAPES)
def test_any_segmentation_gives_the_same_bits(eng, L, M, ntaps, K, fmt):
    rng = np.random.default_rng(53 * L + 7 * M + ntaps)
    Ti, Q = bc.tile_inputs(L, M), bc.history(ntaps, L)
    nin = 3 * Ti + 100 + 3 * Q
    x, h, fcs = _rows(rng, K, nin), bc.taps_for(rng, ntaps), bc.freqs(K)
    band = _rows(rng, 1, cases.count(0, nin, L, M) + 1)[0]
    try:
        eng.set_tx_resamp_bank(tx_resample.bank_cfg(L, M, fcs, taps=h, out_format=fmt))
        for first, add in ((0, None), (FAR, band)):
            no = cases.count(first, nin, L, M)
            eng.tx_resamp_bank_reset(first)
            whole = eng.tx_resamp_bank(x, add=None if add is None else add[:no]).copy()
            assert len(whole) == no and np.any(whole != 0)
            eng.tx_resamp_bank_reset(first)
            sizes = bc.chunk_inputs(rng, nin, L, M, ntaps)
            assert sum(sizes) == nin and {0, 1, Q + 1, Ti + 1, Ti - 1} <= set(sizes)
            assert (Q in sizes or Q == 0) and (Q - 1 in sizes or Q <= 1)
            parts, a, o = [], 0, 0
            for n in sizes:
                cnt = eng.tx_resamp_bank_count(n)
                y = eng.tx_resamp_bank(x[:, a:a + n], add=None if add is None else add[o:o + cnt])
                assert len(y) == cnt == cases.count(first + a, n, L, M)         # the count is what the call returns
                parts.append(y.copy())
                a += n
                o += cnt
            got = np.concatenate(parts)
            assert got.dtype == whole.dtype and np.array_equal(_bits(got), _bits(whole)), (L, M, ntaps, K, first, fmt)
    finally:
        eng.set_tx_resamp_bank(None)


@pytest.mark.parametrize("fmt", ["fc32", "sc16"])
@pytest.mark.parametrize("L,M,ntaps", [(5, 2, 39), (1, 1, 1024), (3, 4, 2), (25, 8, 481), (64, 63, 65)])
def test_one_link_at_zero_frequency_is_the_single_stage_at_zero_frequency(eng, L, M, ntaps, fmt):
    rng = np.random.default_rng(100 * L + M + ntaps)
    x = _rows(rng, 1, bc.stream_inputs(L, M))
    h = bc.taps_for(rng, ntaps)
    try:
        eng.set_tx_resamp_bank(tx_resample.bank_cfg(L, M, [0.0], taps=h, out_format=fmt))
        eng.set_tx_resamp(tx_resample.tx_resamp_cfg(L, M, 0.0, taps=h, out_format=fmt))
        for first in (0, START):
            eng.tx_resamp_bank_reset(first)
            eng.tx_resamp_reset(first)
            a, b = eng.tx_resamp_bank(x), eng.tx_resamp(x[0])
            assert a.shape == b.shape and a.dtype == b.dtype
            assert np.array_equal(a, b), (L, M, ntaps, fmt, first)          # as numbers: the sign of a zero may differ
        assert np.any(a != 0)
    finally:
        eng.set_tx_resamp_bank(None)
        eng.set_tx_resamp(None)


@pytest.mark.parametrize("L,M", [(1, 1), (4, 1), (5, 2), (3, 4), (2, 5)])
def test_one_link_with_the_unit_tap_is_the_single_stage_at_any_matching_frequency(eng, L, M):
    """h = {1.0}: the table is (1, 0), the chain is one exact product, and what is left is r, the phase convention and
    the gr_complex product -- the single stage's, bit for bit, wherever the stream starts, at every fc whose phase step
    per output is the same in both definitions: turns(fc) = M turns(fc / M).  A dyadic fc fits an M that is a power of
    two, fc = 5 j / 2^20 fits M = 5; both signs."""
    rng = np.random.default_rng(77 + L + M)
    x = _rows(rng, 1, bc.stream_inputs(L, M), amp=1.0)
    fcs = [s * 5.0 * j / 2.0 ** 20 for j in (1, 3, 20001, 104857) for s in (1, -1)] if M == 5 else DYADIC + [-0.1875, 3.0 / 1024]
    try:
        for fc in fcs:
            assert abs(fc) <= 0.5 and _same_phase_per_output(fc, L, M), (fc, L, M)
            eng.set_tx_resamp_bank(tx_resample.bank_cfg(L, M, [fc], taps=[1.0]))
            eng.set_tx_resamp(tx_resample.tx_resamp_cfg(L, M, fc, taps=[1.0]))
            for first in (0, START, FAR):
                eng.tx_resamp_bank_reset(first)
                eng.tx_resamp_reset(first)
                a, b = eng.tx_resamp_bank(x), eng.tx_resamp(x[0])
                assert len(a) == len(b) and np.array_equal(a, b) and np.any(a != 0), (L, M, fc, first)
    finally:
        eng.set_tx_resamp_bank(None)
        eng.set_tx_resamp(None)


@pytest.mark.parametrize("L,M,ntaps", [(5, 2, 39), (1, 1, 33), (25, 8, 481), (7, 64, 200)])
def test_a_link_of_zeros_changes_no_value(eng, L, M, ntaps):
    rng = np.random.default_rng(300 + L + M)
    nin = bc.stream_inputs(L, M)
    x, h = _rows(rng, 3, nin), bc.taps_for(rng, ntaps)
    z = np.zeros((1, nin), np.complex64)
    fcs = bc.freqs(3)
    try:
        eng.set_tx_resamp_bank(tx_resample.bank_cfg(L, M, fcs, taps=h))
        ref = eng.tx_resamp_bank(x).copy()
        assert np.any(ref != 0)
        eng.set_tx_resamp_bank(tx_resample.bank_cfg(L, M, fcs + [0.37], taps=h))
        assert np.array_equal(eng.tx_resamp_bank(np.concatenate([x, z])), ref)
        eng.set_tx_resamp_bank(tx_resample.bank_cfg(L, M, [0.37] + fcs, taps=h))
        assert np.array_equal(eng.tx_resamp_bank(np.concatenate([z, x])), ref)
        # the order of the list is part of the configuration: the same links in another order are the same signal
        eng.set_tx_resamp_bank(tx_resample.bank_cfg(L, M, fcs[::-1], taps=h))
        other = eng.tx_resamp_bank(x[::-1])
        _, s = bc.model(x, h, L, M, fcs)
        assert np.all(np.abs(other.astype(np.complex128) - ref.astype(np.complex128)) <= 2 * bc.bound(3, ntaps, L, s))
    finally:
        eng.set_tx_resamp_bank(None)


@pytest.mark.parametrize("L,M,ntaps", [(5, 2, 39), (64, 63, 155), (2, 5, 25)])
def test_add_is_one_float32_addition_per_part_and_sc16_is_the_store_of_the_same_value(eng, L, M, ntaps):
    rng = np.random.default_rng(40 + L + M)
    nin = bc.stream_inputs(L, M)
    no = cases.count(0, nin, L, M)
    x, h, fcs = _rows(rng, 3, nin), bc.taps_for(rng, ntaps), bc.freqs(3)
    band = _rows(rng, 1, no, amp=3.0)[0]
    try:
        eng.set_tx_resamp_bank(tx_resample.bank_cfg(L, M, fcs, taps=h))
        v = eng.tx_resamp_bank(x).copy()
        assert len(v) == no
        eng.tx_resamp_bank_reset(0)
        got = eng.tx_resamp_bank(x, add=band)
        want = (v.real + band.real).astype(np.float32) + 1j * (v.imag + band.imag).astype(np.float32)
        assert np.array_equal(got, want.astype(np.complex64))
        eng.tx_resamp_bank_reset(0)                       # (the count is the stream's: from the same start)
        for wrong in (band[:-1], np.concatenate([band, band[:1]])):
            with pytest.raises(ValueError):
                eng.tx_resamp_bank(x, add=wrong)
        # 16-bit output: the transmit rule on the same float32 value, and on the sum where there is an add
        for scale in (None, 1000.0):
            eng.set_tx_resamp_bank(tx_resample.bank_cfg(L, M, fcs, taps=h, out_format="sc16", out_scale=scale))
            assert np.array_equal(eng.tx_resamp_bank(x), iqio.to_sc16(v, scale or SCALE))
            small = (band * np.float32(0.01)).astype(np.complex64)
            eng.tx_resamp_bank_reset(0)
            sum32 = (v.real + small.real).astype(np.float32) + 1j * (v.imag + small.imag).astype(np.float32)
            assert np.array_equal(eng.tx_resamp_bank(x, add=small), iqio.to_sc16(sum32.astype(np.complex64), scale or SCALE))
    finally:
        eng.set_tx_resamp_bank(None)


def test_table_is_the_receive_banks_at_the_mirror_ratio():
    e = engine.Engine(cfg=make_cfg())
    try:
        rng = np.random.default_rng(8)
        h, fcs = bc.taps_for(rng, 155), bc.freqs(8)
        for L, M in ((5, 2), (25, 8), (3, 64)):
            e.set_tx_resamp_bank(tx_resample.bank_cfg(L, M, fcs, taps=h))
            e.set_resamp_bank(resample.bank_cfg(M, L, fcs, taps=h))            # interpolation = M
            for i, fc in enumerate(fcs):
                t = e.tx_resamp_bank_taps(i)
                assert t.dtype == np.complex64 and len(t) == 155
                assert np.array_equal(_bits(t), _bits(e.resamp_bank_taps(i))), (L, M, i)
                # NumPy's table: the same float64 formula, another libm -- a last float64 bit may move one float32 rounding
                ref = resample.bandpass_taps(h, fc, M)
                assert np.all(np.abs(t.astype(np.complex128) - ref.astype(np.complex128)) <= 2.0 ** -23 * np.abs(h)), i
                assert np.mean(t == ref) > 0.99
            assert np.array_equal(e.tx_resamp_bank_taps(2), h.astype(np.complex64))        # fc = 0: the taps themselves
        k = C.c_int(0)
        lib = _abi.load()
        for link in (8, 9, -1):
            assert lib.ofdm_tx_resamp_bank_taps(e._h, link, None, 0, C.byref(k)) == _abi.OFDM_E_INVAL
        assert lib.ofdm_tx_resamp_bank_taps(e._h, 7, None, 0, C.byref(k)) == _abi.OFDM_OK and k.value == 155
        small = np.zeros(100, np.complex64)
        assert lib.ofdm_tx_resamp_bank_taps(e._h, 7, small.ctypes.data_as(C.c_void_p), 100, C.byref(k)) == _abi.OFDM_E_CAPACITY
    finally:
        e.close()


@pytest.mark.parametrize("L,M,ntaps,K", [(5, 2, 39, 2), (5, 2, 39, 8), (3, 4, 50, 8), (25, 8, 481, 2)])
def test_against_k_single_stage_passes(eng, L, M, ntaps, K):
    """Same taps and frequencies, one Engine.tx_resamp(..., add=band) per link, at frequencies where both float64
    models coincide: the two ways differ by no more than the bank's bound plus the sum of the passes'
    tx_resamp_cases.bound (a pass's `add` being the band so far)."""
    rng = np.random.default_rng(900 + L + K)
    nin = bc.stream_inputs(L, M)
    x, h, fcs = _rows(rng, K, nin), bc.taps_for(rng, ntaps), DYADIC[:K]
    assert all(_same_phase_per_output(fc, L, M) for fc in fcs)
    try:
        for first in (0, START):
            eng.set_tx_resamp_bank(tx_resample.bank_cfg(L, M, fcs, taps=h))
            eng.tx_resamp_bank_reset(first)
            y = eng.tx_resamp_bank(x).copy()
            _, s_terms = bc.model_terms(x, h, L, M, fcs, first)
            bound = bc.bound(K, ntaps, L, s_terms.sum(axis=0))
            band = None
            for i, fc in enumerate(fcs):
                eng.set_tx_resamp(tx_resample.tx_resamp_cfg(L, M, fc, taps=h))
                eng.tx_resamp_reset(first)
                bound = bound + cases.bound(ntaps, L, s_terms[i], band)
                band = eng.tx_resamp(x[i], add=band).copy()
            err = np.abs(y.astype(np.complex128) - band.astype(np.complex128))
            print("%d/%d ntaps=%d K=%d first=%d: worst |bank - passes| / (sum of the bounds) = %.3g"
                  % (L, M, ntaps, K, first, float(np.max(err / np.maximum(bound, 1e-300)))))
            assert len(y) == len(band) and np.all(err <= bound) and np.any(y != 0)
    finally:
        eng.set_tx_resamp_bank(None)
        eng.set_tx_resamp(None)


def _zero(torch, *tensors):
    """Zero the test's device buffers before they are released: a later test's torch.empty() must not inherit this
    file's bytes."""
    for t in tensors:
        t.zero_()
    torch.cuda.synchronize()


def test_in_device_mode_add_may_be_the_output_buffer():
    import torch
    L, M, ntaps = 5, 2, 39
    rng = np.random.default_rng(31)
    nin = bc.stream_inputs(L, M)
    no = cases.count(0, nin, L, M)
    stride = nin + 5
    fcs = bc.freqs(3)
    x = np.zeros((3, stride), np.complex64)
    x[:, :nin] = _rows(rng, 3, nin)
    band = _rows(rng, 1, no)[0]
    h = bc.taps_for(rng, ntaps)
    host = engine.Engine(cfg=make_cfg())
    dev = engine.Engine(cfg=make_cfg(device_ptrs=True))
    try:
        for e in (host, dev):
            e.set_tx_resamp_bank(tx_resample.bank_cfg(L, M, fcs, taps=h))
            e.prof_enable(True)
        with pytest.raises(ValueError):
            dev.tx_resamp_bank_last_ms()                       # no profiled call yet
        want = host.tx_resamp_bank(x[:, :nin], add=band)
        d_x = torch.from_numpy(x).cuda()
        d_out = torch.from_numpy(band.copy()).cuda()
        torch.cuda.synchronize()
        assert dev.tx_resamp_bank_device(d_x.data_ptr(), stride, nin, d_out.data_ptr(), no, add_ptr=d_out.data_ptr()) == no
        assert np.array_equal(d_out.cpu().numpy(), want)
        assert dev.tx_resamp_bank_last_ms() > 0.0 and host.tx_resamp_bank_last_ms() > 0.0
        # two halves through device pointers continue the stream
        dev.tx_resamp_bank_reset(0)
        d_out.copy_(torch.from_numpy(band))
        torch.cuda.synchronize()
        n1 = nin // 2 + 1
        a = dev.tx_resamp_bank_device(d_x.data_ptr(), stride, n1, d_out.data_ptr(), no, add_ptr=d_out.data_ptr())
        b = dev.tx_resamp_bank_device(d_x.data_ptr() + 8 * n1, stride, nin - n1, d_out.data_ptr() + 8 * a, no - a,
                                      add_ptr=d_out.data_ptr() + 8 * a)
        assert a == cases.count(0, n1, L, M) and a + b == no and np.array_equal(d_out.cpu().numpy(), want)
        _zero(torch, d_x, d_out)
        del d_x, d_out
        torch.cuda.empty_cache()
    finally:
        host.close()
        dev.close()


def _options(k):
    return options.default_options(modulation=k["mod"], fft_length=k["N"], occupied_tones=k["occ"], cp_length=k["CP"])


def _case(name):
    mod, N, occ, CP, L, M, freqs, plen = cases.CASES[name]
    pays = [make_payloads(4, plen, seed=s) for s in (11, 29)]
    k = dict(mod=mod, N=N, occ=occ, CP=CP)
    return k, L, M, list(freqs), pays, tx_resample.design(L, M, occ / float(N)), resample.design(M, L, occ / float(N))


def _link_power(opt, pays, amplitude):
    plain = ofdm.ofdm_mod(opt)
    try:
        plain.engine().set_tx_amplitude(amplitude)
        for p in pays:
            plain.send_pkt(p)
        return float(np.mean(np.abs(plain.flush()) ** 2))     # one link's narrowband power
    finally:
        plain.engine().close()


@pytest.mark.parametrize("name,fmt", [("qpsk512_5_2", "fc32"), ("qpsk512_5_2", "sc16"), ("bpsk64_25_8", "fc32")])
def test_two_links_end_to_end_into_the_receive_bank(name, fmt):
    """ofdm_mod_resamp_bank (both links in one pass) -> the noise of tx_resamp_cases (30 dB inside a link's band) ->
    ofdm_demod_resamp_bank at the mirror ratio: every packet of both links returns CRC-ok with its payload, from one
    flush(end=True) and from a band made across several flush() calls."""
    k, L, M, fcs, pays, tx_taps, rx_taps = _case(name)
    opt, N = _options(k), k["N"]
    Q = cases.history(len(tx_taps), L)
    amplitude = 0.05                                       # two links and the noise stay inside the 16-bit range
    P = _link_power(opt, pays[0], amplitude)
    tx = ofdm.ofdm_mod_resamp_bank(opt, fcs, L, M, taps=tx_taps, iq_format=fmt)
    rx = ofdm.ofdm_demod_resamp_bank(opt, fcs, M, L, taps=rx_taps, iq_format=fmt)
    try:
        assert tx.flush(end=True) is None and len(tx.links()) == 2 and tx.engine().tx_resamp_bank_cfg.nlinks == 2
        for m in tx.links():
            m.engine().set_tx_amplitude(amplitude)
        _, nsamp = tx.links()[0].engine().tx_frame_count([len(p) for p in pays[0]])
        bands = []
        # whole: one batch and the tail
        for i in range(2):
            for p in pays[i]:
                tx.send_pkt(i, p)
        bands.append(tx.flush(end=True))
        assert len(bands[0]) == cases.count(0, nsamp + Q, L, M)
        # three batches: the band continues across flush() calls, end=True pushes the tail out and resets
        parts = []
        for part, end in ((slice(0, 1), False), (slice(1, 3), False), (slice(3, 4), True)):
            for i in range(2):
                for p in pays[i][part]:
                    tx.send_pkt(i, p)
            parts.append(tx.flush(end=end))
        assert tx.flush() is None and tx.flush(end=True) is None       # nothing queued, nothing in flight
        bands.append(np.concatenate(parts))
        assert len(bands[1]) == len(bands[0])
        for band in bands:
            assert band.dtype == (np.int16 if fmt == "sc16" else np.complex64)
            w = np.concatenate([np.zeros(2 * N * L // M), _c64(band, fmt), np.zeros(3 * N * L // M)])
            w = (w + cases.noise(len(w), P, L, M)).astype(np.complex64)
            if fmt == "sc16":
                assert np.max(np.abs(w.real)) < 0.99 and np.max(np.abs(w.imag)) < 0.99
                w = iqio.to_sc16(w)
            got = rx.work(w)
            for i in range(2):
                assert [ok for ok, _ in got[i]] == [True] * 4 and [p for _, p in got[i]] == pays[i], (name, fmt, i)
    finally:
        rx.close()
        tx.close()
    assert tx.engine()._h.value is None and all(m.engine()._h.value is None for m in tx.links())


def test_mod_resamp_bank_pads_tails_resets_and_drops_a_failing_batch():
    opt = options.default_options(modulation="qpsk", fft_length=512, occupied_tones=200, cp_length=128)
    L, M, fcs = 5, 2, [0.22, -0.21, 0.01]
    taps = tx_resample.design(L, M, 200 / 512.0)
    Q = cases.history(len(taps), L)
    sent = [make_payloads(3 - (i % 2), 100, seed=11 + 18 * i) for i in range(3)]      # streams of unequal length
    tx = ofdm.ofdm_mod_resamp_bank(opt, fcs, L, M, taps=taps)
    plain = [ofdm.ofdm_mod(opt) for _ in range(3)]
    try:
        assert Q >= 2 and tx.flush() is None
        e = tx.engine()
        # two batches continue the band; the tail comes with end=True, which also starts the bank afresh
        halves = []
        for part in (slice(0, 1), slice(1, None)):
            for i, pays in enumerate(sent):
                for p in pays[part]:
                    tx.send_pkt(i, p)
                    plain[i].send_pkt(p)
            halves.append((tx.flush(end=part.start == 1), [m.flush() for m in plain]))
        assert tx.flush() is None and tx.flush(end=True) is None       # nothing queued, nothing in flight
        pos = 0
        for j, (got, nbj) in enumerate(halves):
            nj = max(len(v) for v in nbj)
            assert j == 0 or min(len(v) for v in nbj) < nj
            xj = np.zeros((3, nj + (Q if j == 1 else 0)), np.complex64)
            for i, v in enumerate(nbj):
                xj[i, :len(v)] = v
            want = e.tx_resamp_bank(xj)                                   # (the bank had reset: the same stream again)
            assert len(got) == cases.count(pos, xj.shape[1], L, M) and np.array_equal(_bits(got), _bits(want)), j
            pos += xj.shape[1]
        e.tx_resamp_bank_reset(0)
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
        e.tx_resamp_bank_reset(0)
        assert np.array_equal(_bits(got), _bits(e.tx_resamp_bank(x1))) and np.any(got != 0)
    finally:
        tx.close()
        for m in plain:
            m.engine().close()


def _raw(lib, h, x, stride, nin, out, cap, add=None):
    nn = C.c_uint64(0)
    rc = lib.ofdm_tx_resamp_bank(h, x.ctypes.data_as(C.c_void_p), stride, nin,
                                 None if add is None else add.ctypes.data_as(C.c_void_p),
                                 out.ctypes.data_as(C.c_void_p), cap, C.byref(nn))
    return rc, nn.value


def test_layout_and_capacity(eng):
    lib = _abi.load()
    rng = np.random.default_rng(5)
    L, M, fcs, nin = 5, 2, bc.freqs(3), 700
    x = _rows(rng, 3, nin)
    h = tx_resample.design(L, M, 0.4)
    Q = cases.history(len(h), L)
    no = cases.count(0, nin, L, M)
    eng.set_tx_resamp_bank(tx_resample.bank_cfg(L, M, fcs, taps=h))
    try:
        want = eng.tx_resamp_bank(x).copy()
        assert len(want) == no
        # link_stride > nin: the gaps are not read
        eng.tx_resamp_bank_reset(0)
        wide = np.full((3, nin + 13), np.complex64(np.nan), np.complex64)
        wide[:, :nin] = x
        out = np.zeros(no, np.complex64)
        assert _raw(lib, eng._h, wide, nin + 13, nin, out, no) == (_abi.OFDM_OK, no)
        assert np.array_equal(out, want)
        # out_cap one short: refused with *nout set, and the stream does not move
        eng.tx_resamp_bank_reset(0)
        n1 = 401
        first = eng.tx_resamp_bank(x[:, :n1]).copy()
        rest_in = np.ascontiguousarray(x[:, n1:])
        n2 = nin - n1
        no2 = eng.tx_resamp_bank_count(n2)
        assert len(first) + no2 == no
        sentinel = np.complex64(-7.5 + 3.25j)
        out = np.full(no2, sentinel, np.complex64)
        assert _raw(lib, eng._h, rest_in, n2, n2, out, no2 - 1) == (_abi.OFDM_E_CAPACITY, no2)
        assert np.all(out == sentinel) and eng.tx_resamp_bank_count(n2) == no2
        # link_stride < nin with more than one link
        assert _raw(lib, eng._h, rest_in, n2 - 1, n2, out, no2)[0] == _abi.OFDM_E_INVAL
        assert np.all(out == sentinel)
        rest = eng.tx_resamp_bank(rest_in)
        assert np.array_equal(np.concatenate([first, rest]), want)        # the stream continues bit for bit
        # calls of 0 and calls shorter than Q are part of the stream
        eng.tx_resamp_bank_reset(0)
        assert Q >= 2
        parts = [eng.tx_resamp_bank(x[:, a:b]).copy() for a, b in ((0, 0), (0, 1), (1, Q), (Q, Q), (Q, nin))]
        assert [len(p) for p in parts[:4]] == [0, cases.count(0, 1, L, M), cases.count(1, Q - 1, L, M), 0]
        assert np.array_equal(np.concatenate(parts), want)
        # one link: the stride does not matter
        eng.set_tx_resamp_bank(tx_resample.bank_cfg(L, M, [fcs[1]], taps=h))
        one = eng.tx_resamp_bank(x[1]).copy()
        eng.tx_resamp_bank_reset(0)
        out = np.zeros(no, np.complex64)
        assert _raw(lib, eng._h, np.ascontiguousarray(x[1]), 0, nin, out, no) == (_abi.OFDM_OK, no)
        assert np.array_equal(out, one)
    finally:
        eng.set_tx_resamp_bank(None)


def _raw_cfg(**kw):
    c = tx_resample.bank_cfg(5, 2, [0.2, -0.3], taps=np.ones(6, np.float32))
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_invalid_arguments_are_refused(eng):
    lib = _abi.load()
    eng.set_tx_resamp_bank(None)
    x = np.zeros((2, 16), np.complex64)
    x[:, ::3] = 1.0
    out = np.zeros(64, np.complex64)
    nn = C.c_uint64(0)
    assert _raw(lib, eng._h, x, 16, 16, out, 64)[0] == _abi.OFDM_E_INVAL            # no configuration
    assert lib.ofdm_tx_resamp_bank_count(eng._h, 16, C.byref(nn)) == _abi.OFDM_E_INVAL
    for call in (lambda: eng.tx_resamp_bank(x), lambda: eng.tx_resamp_bank_reset(0), lambda: eng.tx_resamp_bank_last_ms(),
                 lambda: eng.tx_resamp_bank_taps(0), lambda: eng.tx_resamp_bank_count(4)):
        with pytest.raises(ValueError):
            call()
    good = _raw_cfg()
    eng.set_tx_resamp_bank(good)
    table = eng.tx_resamp_bank_taps(1)
    assert _raw(lib, eng._h, x, 16, 16, out, 64) == (_abi.OFDM_OK, 40)
    y = out[:40].copy()
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
    refused = [_raw_cfg(**b) for b in (dict(struct_size=12), dict(interpolation=0), dict(interpolation=65),
                                       dict(decimation=0), dict(decimation=65), dict(ntaps=0),
                                       dict(ntaps=1025), dict(nlinks=0), dict(nlinks=9), dict(out_format=2),
                                       dict(out_format=1, out_scale=-1.0), dict(out_format=1, out_scale=float("inf")))]
    refused += bad_fc + bad_tap
    messages = set()
    for c in refused:
        with pytest.raises(ValueError) as info:
            eng.set_tx_resamp_bank(c)
        assert str(info.value)                            # each refusal has its message
        messages.add(str(info.value))
        assert eng.tx_resamp_bank_cfg is good
    assert len(messages) == 9         # struct_size, L, M, ntaps, nlinks, format, scale, frequency, taps: one each
    for c in refused:
        assert lib.ofdm_set_tx_resamp_bank(eng._h, C.byref(c)) == _abi.OFDM_E_INVAL
    c = _raw_cfg()
    c.center_freq[2] = 7.0                                # a frequency beyond nlinks is not looked at
    eng.set_tx_resamp_bank(c)
    eng.set_tx_resamp_bank(good)
    # a refused configuration leaves the one in force untouched: same table, same stream position, same outputs
    a = eng.tx_resamp_bank(x[:, :7]).copy()
    with pytest.raises(ValueError):
        eng.set_tx_resamp_bank(bad_fc[0])
    assert np.array_equal(eng.tx_resamp_bank_taps(1), table)
    b = eng.tx_resamp_bank(x[:, 7:])
    assert np.array_equal(np.concatenate([a, b]), y)
    # the ends of the frequency range are inside it
    eng.set_tx_resamp_bank(tx_resample.bank_cfg(5, 2, [0.5, -0.5], taps=np.ones(6, np.float32)))
    eng.set_tx_resamp_bank(good)
    # index limit: the single stage's, no input index past 2^56
    lim = 1 << 56
    eng.tx_resamp_bank_reset(lim)
    with pytest.raises(ValueError):
        eng.tx_resamp_bank_reset(lim + 1)
    assert _raw(lib, eng._h, x, 16, 1, out, 64)[0] == _abi.OFDM_E_INVAL              # one input more would pass it
    assert lib.ofdm_tx_resamp_bank_count(eng._h, 1, C.byref(nn)) == _abi.OFDM_E_INVAL
    assert _raw(lib, eng._h, x, 16, 0, out, 64) == (_abi.OFDM_OK, 0)
    eng.tx_resamp_bank_reset(0)
    assert _raw(lib, eng._h, x, 1 << 57, 1 << 57, out, 64)[0] == _abi.OFDM_E_INVAL
    # a call too long for one grid: refused before anything is read or written, the stream stays where it was
    long_n = (1 << 31) * bc.tile_inputs(5, 2) + 1
    assert _raw(lib, eng._h, x, long_n, long_n, out, 1 << 62) == (_abi.OFDM_E_INVAL, cases.count(0, long_n, 5, 2))
    assert b"too long" in lib.ofdm_last_error(eng._h)
    assert _raw(lib, eng._h, x, 16, 16, out, 64) == (_abi.OFDM_OK, 40) and np.array_equal(out[:40], y)
    eng.tx_resamp_bank_reset(0)
    # misaligned buffers: complex64 in, add and out on 8 bytes, 16-bit out on 4
    f = np.zeros(2 * 64 + 2, np.float32)
    xp, op, odd = x.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), C.c_void_p(f.ctypes.data + 4)
    assert lib.ofdm_tx_resamp_bank(eng._h, odd, 0, 16, None, op, 64, C.byref(nn)) == _abi.OFDM_E_INVAL
    assert lib.ofdm_tx_resamp_bank(eng._h, xp, 16, 16, odd, op, 64, C.byref(nn)) == _abi.OFDM_E_INVAL
    assert lib.ofdm_tx_resamp_bank(eng._h, xp, 16, 16, None, odd, 64, C.byref(nn)) == _abi.OFDM_E_INVAL
    assert lib.ofdm_tx_resamp_bank(eng._h, xp, 16, 16, None, None, 64, C.byref(nn)) == _abi.OFDM_E_INVAL       # null iq_out
    assert lib.ofdm_tx_resamp_bank(eng._h, None, 16, 16, None, op, 64, C.byref(nn)) == _abi.OFDM_E_INVAL       # null iq_in
    assert lib.ofdm_tx_resamp_bank(eng._h, xp, 16, 16, None, op, 64, None) == _abi.OFDM_E_INVAL
    eng.set_tx_resamp_bank(_raw_cfg(out_format=1))
    try:
        q = np.zeros(2 * 64 + 2, np.int16)
        assert lib.ofdm_tx_resamp_bank(eng._h, xp, 16, 16, None, C.c_void_p(q.ctypes.data + 2), 64, C.byref(nn)) == _abi.OFDM_E_INVAL
        assert lib.ofdm_tx_resamp_bank(eng._h, xp, 16, 16, None, C.c_void_p(q.ctypes.data + 4), 64, C.byref(nn)) == _abi.OFDM_OK
        assert np.array_equal(q[2:82].reshape(-1, 2), iqio.to_sc16(y))               # ... and the stream had not moved
    finally:
        eng.set_tx_resamp_bank(None)
    assert _raw(lib, eng._h, x, 16, 16, out, 64)[0] == _abi.OFDM_E_INVAL            # ... and after it was dropped


def test_device_pointer_path_behind_an_asynchronous_transmit():
    """The bank's input is what tx_device(wait=False) is still producing on the same handle."""
    import torch
    pays = make_payloads(4, 100, seed=7)
    L, M, fcs = 5, 2, [0.22, -0.21]
    taps = tx_resample.design(L, M, 200 / 512.0)
    host = engine.Engine(cfg=make_cfg())
    dev = engine.Engine(cfg=make_cfg(device_ptrs=True))
    try:
        x = host.tx(pays)
        host.set_tx_resamp_bank(tx_resample.bank_cfg(L, M, fcs, taps=taps))
        # the two links are the two halves of the buffer the transmitter fills
        nin = len(x) // 2
        wide = host.tx_resamp_bank(np.stack([x[:nin], x[nin:2 * nin]]))
        no = len(wide)
        blob, offs, lens = engine.pack_payloads(pays)
        _, nsamp = dev.tx_frame_count(lens)
        assert nsamp == len(x)
        d_pay = torch.from_numpy(blob.copy()).cuda()
        d_iq = torch.zeros(nsamp, dtype=torch.complex64, device="cuda")
        d_wide = torch.zeros(no, dtype=torch.complex64, device="cuda")
        dev.set_tx_resamp_bank(tx_resample.bank_cfg(L, M, fcs, taps=taps))
        torch.cuda.synchronize()
        assert dev.tx_device(d_pay.data_ptr(), offs, lens, d_iq.data_ptr(), nsamp, wait=False) == nsamp
        assert dev.tx_resamp_bank_device(d_iq.data_ptr(), nin, nin, d_wide.data_ptr(), no) == no
        assert np.array_equal(d_wide.cpu().numpy(), wide) and np.any(wide != 0)
        _zero(torch, d_pay, d_iq, d_wide)
        del d_pay, d_iq, d_wide
        torch.cuda.empty_cache()
    finally:
        host.close()
        dev.close()


def test_the_bank_and_the_other_transmit_stages_do_not_disturb_each_other(eng):
    rng = np.random.default_rng(23)
    nb = _rows(rng, 3, 1100)
    t155, t39 = bc.taps_for(rng, 155), bc.taps_for(rng, 39)
    stages = {
        "tx_resamp_bank": (lambda: eng.set_tx_resamp_bank(tx_resample.bank_cfg(25, 8, bc.freqs(3), taps=t155)),
                           lambda a, b: eng.tx_resamp_bank(nb[:, a:b]), 1100, 177),
        "tx_resamp": (lambda: eng.set_tx_resamp(tx_resample.tx_resamp_cfg(5, 2, 0.25, taps=t39)),
                      lambda a, b: eng.tx_resamp(nb[0, a:b]), 1100, 301),
        "duc_bank": (lambda: eng.set_duc_bank(duc.bank_cfg(8, bc.freqs(3), taps=t155)),
                     lambda a, b: eng.duc_bank(nb[:, a:b]), 1100, 259),
        "pfb_synth": (lambda: eng.set_pfb_synth(pfb.synth_cfg(8, [6, 1, 3], taps=t155)),
                      lambda a, b: eng.pfb_synth(nb[:, a:b]), 1100, 211),
    }
    off = dict(tx_resamp_bank=eng.set_tx_resamp_bank, tx_resamp=eng.set_tx_resamp, duc_bank=eng.set_duc_bank,
               pfb_synth=eng.set_pfb_synth)
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
            assert np.array_equal(np.concatenate(parts[name]), alone[name]), name
        # dropping or resetting another stage leaves the bank's stream where it was
        eng.tx_resamp_bank_reset(0)
        a = eng.tx_resamp_bank(nb[:, :500]).copy()
        eng.pfb_synth_reset(0)
        eng.tx_resamp_reset(5)
        eng.duc_bank_reset(9)
        eng.set_tx_resamp(None)
        eng.set_duc_bank(None)
        eng.set_pfb_synth(None)
        b = eng.tx_resamp_bank(nb[:, 500:])
        assert np.array_equal(np.concatenate([a, b]), alone["tx_resamp_bank"])
    finally:
        for f in off.values():
            f(None)


def test_a_handle_that_dropped_the_bank_launches_what_it_launched():
    """Two handles transmit the same packets: one never saw the bank, the other used it and dropped it.  Same IQ bits,
    same per-kernel launch counts; the kernel table has no entry for the stage."""
    pays = make_payloads(3, 100, seed=3)
    a, b = engine.Engine(cfg=make_cfg()), engine.Engine(cfg=make_cfg())
    try:
        b.set_tx_resamp_bank(tx_resample.bank_cfg(5, 2, [0.2, -0.3], occupied_fraction=200 / 512.0))
        assert len(b.tx_resamp_bank(_rows(np.random.default_rng(2), 2, 3000))) == 7500
        b.set_tx_resamp_bank(None)
        for e in (a, b):
            e.prof_enable(True)
            e.prof_reset()
        ia, ib = a.tx(pays), b.tx(pays)
        assert np.array_equal(ia, ib)
        ca = {k: v[1] for k, v in a.prof().items()}
        cb = {k: v[1] for k, v in b.prof().items()}
        assert ca == cb and sum(ca.values()) > 0
        assert len(ca) == _abi.K_COUNT == 11 and not any("resamp" in k for k in ca)
    finally:
        a.close()
        b.close()


def test_command_line_places_every_link_on_the_band(tmp_path):
    f = str(tmp_path / "wide.dat")
    npk = benchmark_ofdm_tx.main(["-m", "qpsk", "--to-file", f, "-M", "9e-6", "--tx-amplitude", "0.1", "--tx-resamp-interp", "5",
                                  "--tx-resamp-decim", "2", "--tx-resamp-freqs", "0.22,-0.21"])
    assert npk == 4
    wide = iqio.read_complex_binary(f)
    assert len(wide) > 0 and np.any(wide != 0)
    # silence around the band and a noise floor 30 dB below one link inside its band (half the band's power, 2 / 5 of
    # its width): the receiver's metric is 0/0 on exact zeros
    rng = np.random.default_rng(5)
    w = np.concatenate([np.zeros(4096, np.complex64), wide, np.zeros(8192, np.complex64)])
    sigma = np.sqrt(0.5 * float(np.mean(np.abs(wide) ** 2)) * 2.5 / 1e3)
    w = (w + sigma * np.sqrt(0.5) * (rng.standard_normal(len(w)) + 1j * rng.standard_normal(len(w)))).astype(np.complex64)
    iqio.file_sink(f).write(w)
    accts = benchmark_ofdm_rx.main(["-m", "qpsk", "--from-file", f, "--to-file", str(tmp_path / "rx.txt"),
                                    "--resamp-interp", "2", "--resamp-decim", "5", "--resamp-freqs", "0.22,-0.21"])
    assert [(a.n_rcvd, a.n_right) for a in accts] == [(4, 4), (4, 4)]
    # one of the links alone, through the single stage's flag, is still what it was
    assert benchmark_ofdm_tx.main(["-m", "qpsk", "--to-file", f, "-M", "9e-6", "--tx-resamp-interp", "5",
                                   "--tx-resamp-decim", "2", "--tx-resamp-freq", "0.22"]) == 4
