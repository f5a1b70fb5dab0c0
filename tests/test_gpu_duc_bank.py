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
import stage_harness as sh
from helpers import make_cfg, make_payloads
from ofdm_uhd_amd import _abi, ddc, duc, engine, iqio, ofdm, options, pfb
from stage_harness import FAR, SCALE, START, eng   # noqa: F401 (eng: one handle per file)

pytestmark = pytest.mark.gpu

STAGE = sh.STAGES["duc_bank"]
_rows, _bits, _c64, _options, _engine_tx = sh.rows, sh.bits, sh.c64, sh.options_of, sh.engine_tx

# (K, ntaps) per interpolation: K in {1, 2, 3, 8}; ntaps 1, L - 1 (phases without a tap), 1024 at L = 1 and L = 64
MODEL_SHAPES = {
    1: [(8, 33), (2, 1024), (1, 1)],
    2: [(8, 25), (3, 1)],
    3: [(3, 50), (2, 2)],
    4: [(1, 31), (3, 31), (8, 3)],
    8: [(8, 155), (2, 7)],
    64: [(2, 1024), (3, 63), (8, 65), (1, 1)],
}


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
    sh.check_tx_bank_segmentation(eng, STAGE, (L,), ntaps, bc.freqs(K), fmt, seed=53 * L + ntaps, far=FAR)


@pytest.mark.parametrize("fmt", ["fc32", "sc16"])
@pytest.mark.parametrize("L,ntaps", [(1, 1024), (2, 25), (3, 2), (4, 31), (8, 155), (64, 65)])
def test_one_link_at_zero_frequency_is_the_duc_at_zero_frequency(eng, L, ntaps, fmt):
    sh.check_one_row_at_zero_frequency_is_the_single_stage(eng, STAGE, (L,), ntaps, fmt, seed=100 * L + ntaps, sel=[0.0])


@pytest.mark.parametrize("L", [1, 4])
def test_one_link_with_the_unit_tap_is_the_duc_at_any_frequency(eng, L):
    """h = {1.0}: the table is (1, 0), the chain is one exact product, and what is left is r, the phase convention and
    the gr_complex product -- the DUC's, bit for bit, whatever fc and wherever the stream starts."""
    sh.check_one_link_with_the_unit_tap_is_the_single_stage(eng, STAGE, (L,), seed=77 + L, fcs=bc.freqs(8) + [-1e-20, 1.0 / 3.0])


@pytest.mark.parametrize("L,ntaps", [(4, 31), (1, 33), (64, 155)])
def test_a_link_of_zeros_changes_no_value(eng, L, ntaps):
    sh.check_a_link_of_zeros_changes_no_value(eng, STAGE, (L,), ntaps, seed=300 + L)


@pytest.mark.parametrize("L,ntaps", [(4, 31), (64, 155)])
def test_add_is_one_float32_addition_per_part_and_sc16_is_the_store_of_the_same_value(eng, L, ntaps):
    sh.check_bank_add_and_sc16_store(eng, STAGE, (L,), ntaps, seed=40 + L)


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
    sh.check_against_k_single_stage_passes(eng, STAGE, (L,), ntaps, K, seed=900 + L + K, fcs=bc.freqs(K))


def test_in_device_mode_add_may_be_the_output_buffer():
    import torch
    sh.check_in_device_mode_add_may_be_the_output_buffer(torch, STAGE, (8,), bc.freqs(3), ntaps=155, nin=bc.stream_inputs(8))


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
        sh.check_mod_bank_continues_and_drops_a_failing_batch(tx, plain, sent, STAGE, (L,), Q)
    finally:
        tx.close()
        for m in plain:
            m.engine().close()


def test_layout_and_capacity(eng):
    sh.check_tx_bank_layout_and_capacity(eng, STAGE, (4,), bc.freqs(3), duc.design(4, 0.4), nin=700, one_sel=[bc.freqs(3)[1]])


def test_invalid_arguments_are_refused(eng):
    base = lambda: duc.bank_cfg(4, [0.2, -0.3], taps=np.ones(5, np.float32))
    sh.check_tx_bank_invalid_arguments(eng, STAGE, (4,), base, nout=64, still_refused=0, edge_sel=[0.5, -0.5])


def test_device_pointer_path_behind_an_asynchronous_transmit():
    import torch
    sh.check_bank_device_pointer_path_behind_an_asynchronous_transmit(torch, STAGE, (4,), [0.25, -0.2371],
                                                                      duc.design(4, 200 / 512.0))


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
        alone = sh.check_interleaved(stages, off)
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
    sh.check_a_handle_that_dropped_the_bank_launches_what_it_launched(STAGE, (4,), [0.2, -0.3], nout=12000)
