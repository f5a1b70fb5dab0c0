"""The transmit resampler bank on the GPU (k_tx_resamp_bank, Engine.tx_resamp_bank, ofdm_mod_resamp_bank): against the
float64 model of its definition within the derived bound, exact where it must be (one link is the single stage where
the two definitions meet; segmentation; a zero link; add; the 16-bit store; the table), against K passes of the single
stage, end to end into the receive bank at the mirror ratio, at its edges, and beside the other stages."""
import ctypes as C
import functools

import numpy as np
import pytest

import stage_harness as sh
import tx_resamp_bank_cases as bc
import tx_resamp_cases as cases
from helpers import make_cfg, make_payloads
from ofdm_uhd_amd import (_abi, benchmark_ofdm_rx, benchmark_ofdm_tx, duc, engine, iqio, ofdm, options, pfb, resample,
                          tx_resample)
from stage_harness import FAR, SCALE, START, eng   # noqa: F401 (eng: one handle per file)

pytestmark = pytest.mark.gpu

STAGE = sh.STAGES["tx_resamp_bank"]
assert (0, START, FAR) == bc.FIRSTS
_rows, _bits, _c64, _options = sh.rows, sh.bits, sh.c64, sh.options_of

# (L, M, ntaps, K)
MODEL_SHAPES = [(5, 2, 39, 2), (25, 8, 481, 8), (3, 4, 50, 3), (1, 1, 33, 8), (64, 63, 1024, 2), (2, 5, 25, 4),
                (4, 6, 31, 8), (7, 64, 200, 3), (1, 64, 1024, 2)]
SEG_SHAPES = [(5, 2, 39, 2), (25, 8, 481, 8), (64, 63, 1024, 2), (2, 5, 25, 8), (64, 1, 1, 1)]
# frequencies with turns(fc) = M turns(fc / M) exactly for every M that is a power of two: both signs, zero, the edges
DYADIC = [0.1875, -0.3125, 0.0, 0.5, -0.0625, 0.4375, -0.5, 0.25]


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
    sh.check_tx_bank_segmentation(eng, STAGE, (L, M), ntaps, bc.freqs(K), fmt, seed=53 * L + 7 * M + ntaps, far=FAR,
                                  band_spare=1)


@pytest.mark.parametrize("fmt", ["fc32", "sc16"])
@pytest.mark.parametrize("L,M,ntaps", [(5, 2, 39), (1, 1, 1024), (3, 4, 2), (25, 8, 481), (64, 63, 65)])
def test_one_link_at_zero_frequency_is_the_single_stage_at_zero_frequency(eng, L, M, ntaps, fmt):
    sh.check_one_row_at_zero_frequency_is_the_single_stage(eng, STAGE, (L, M), ntaps, fmt, seed=100 * L + M + ntaps, sel=[0.0])


@pytest.mark.parametrize("L,M", [(1, 1), (4, 1), (5, 2), (3, 4), (2, 5)])
def test_one_link_with_the_unit_tap_is_the_single_stage_at_any_matching_frequency(eng, L, M):
    """h = {1.0}: the table is (1, 0), the chain is one exact product, and what is left is r, the phase convention and
    the gr_complex product -- the single stage's, bit for bit, wherever the stream starts, at every fc whose phase step
    per output is the same in both definitions: turns(fc) = M turns(fc / M).  A dyadic fc fits an M that is a power of
    two, fc = 5 j / 2^20 fits M = 5; both signs."""
    fcs = [s * 5.0 * j / 2.0 ** 20 for j in (1, 3, 20001, 104857) for s in (1, -1)] if M == 5 else DYADIC + [-0.1875, 3.0 / 1024]
    for fc in fcs:
        assert abs(fc) <= 0.5 and _same_phase_per_output(fc, L, M), (fc, L, M)
    sh.check_one_link_with_the_unit_tap_is_the_single_stage(eng, STAGE, (L, M), seed=77 + L + M, fcs=fcs)


@pytest.mark.parametrize("L,M,ntaps", [(5, 2, 39), (1, 1, 33), (25, 8, 481), (7, 64, 200)])
def test_a_link_of_zeros_changes_no_value(eng, L, M, ntaps):
    sh.check_a_link_of_zeros_changes_no_value(eng, STAGE, (L, M), ntaps, seed=300 + L + M)


@pytest.mark.parametrize("L,M,ntaps", [(5, 2, 39), (64, 63, 155), (2, 5, 25)])
def test_add_is_one_float32_addition_per_part_and_sc16_is_the_store_of_the_same_value(eng, L, M, ntaps):
    sh.check_bank_add_and_sc16_store(eng, STAGE, (L, M), ntaps, seed=40 + L + M)


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
    assert all(_same_phase_per_output(fc, L, M) for fc in DYADIC[:K])
    sh.check_against_k_single_stage_passes(eng, STAGE, (L, M), ntaps, K, seed=900 + L + K, fcs=DYADIC[:K])


def test_in_device_mode_add_may_be_the_output_buffer():
    import torch
    sh.check_in_device_mode_add_may_be_the_output_buffer(torch, STAGE, (5, 2), bc.freqs(3), ntaps=39, nin=bc.stream_inputs(5, 2))


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
        sh.check_mod_bank_continues_and_drops_a_failing_batch(tx, plain, sent, STAGE, (L, M), Q)
    finally:
        tx.close()
        for m in plain:
            m.engine().close()


def test_layout_and_capacity(eng):
    sh.check_tx_bank_layout_and_capacity(eng, STAGE, (5, 2), bc.freqs(3), tx_resample.design(5, 2, 0.4), nin=700,
                                         one_sel=[bc.freqs(3)[1]])


def test_invalid_arguments_are_refused(eng):
    base = lambda: tx_resample.bank_cfg(5, 2, [0.2, -0.3], taps=np.ones(6, np.float32))
    sh.check_tx_bank_invalid_arguments(eng, STAGE, (5, 2), base, nout=40, still_refused=0, edge_sel=[0.5, -0.5])


def test_device_pointer_path_behind_an_asynchronous_transmit():
    import torch
    sh.check_bank_device_pointer_path_behind_an_asynchronous_transmit(torch, STAGE, (5, 2), [0.22, -0.21],
                                                                      tx_resample.design(5, 2, 200 / 512.0))


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
        alone = sh.check_interleaved(stages, off)
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
    sh.check_a_handle_that_dropped_the_bank_launches_what_it_launched(STAGE, (5, 2), [0.2, -0.3], nout=7500)


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
