"""The wideband transmit stage on the GPU (k_duc, Engine.duc, ofdm_mod(duc=...)): against the float64 model of its
definition, its exact identities, under arbitrary segmentation of the stream, end to end through the receive stage on
two-link bands built on the device, through the public objects, and at its edges."""
import numpy as np
import pytest

import ddc_cases
import duc_cases
import stage_harness as sh
from helpers import make_cfg
from ofdm_uhd_amd import ddc, duc, engine
from stage_harness import FCS, eng   # noqa: F401 (eng: one handle per file)

pytestmark = pytest.mark.gpu

STAGE = sh.STAGES["duc"]
INTERPS = (1, 2, 3, 4, 8, 64)
_stream, _part_sum, _engine_tx = sh.tx_stream, sh.part_sum, sh.engine_tx


def _tap_counts(L):
    return sorted(n for n in {1, 2, L - 1, L, L + 1, 31, 155, 1024} if n >= 1)


def _set(eng, L, taps, fc, fmt="fc32"):
    eng.set_duc(duc.duc_cfg(L, fc, taps=taps, out_format=fmt))


def _check_against_model(y, x, taps, L, fc, first, fmt, what, add=None):
    sh.check_tx_model(y, x, taps, STAGE, (L,), fc, first, fmt, what, add=add)


@pytest.mark.parametrize("fmt", ["fc32", "sc16"])
@pytest.mark.parametrize("L", INTERPS)
def test_against_float64_model(eng, L, fmt):
    rng = np.random.default_rng(2000 + L)
    tile = duc_cases.tile_outputs(L)
    n = (2 * tile + tile // 3) // L + 5
    while (n * L) % tile == 0:
        n += 1
    x = _stream(rng, n, 0.05)
    try:
        for ntaps in _tap_counts(L):
            taps = (rng.standard_normal(ntaps) * np.sqrt(L / float(ntaps))).astype(np.float32)
            for fc in FCS:
                _set(eng, L, taps, fc, fmt)
                _check_against_model(eng.duc(x), x, taps, L, fc, 0, fmt, "L=%d ntaps=%d fc=%g %s" % (L, ntaps, fc, fmt))
        # once more far from index 0 with the generic frequency: n D mod 2^64 at n of 10^6 L
        taps = (rng.standard_normal(31) * np.sqrt(L / 31.0)).astype(np.float32)
        _set(eng, L, taps, FCS[2], fmt)
        assert duc_cases.phase_step(FCS[2]) % (1 << 32) != 0
        eng.duc_reset(1000003)
        _check_against_model(eng.duc(x), x, taps, L, FCS[2], 1000003, fmt, "L=%d reset to 1000003 %s" % (L, fmt))
    finally:
        eng.set_duc(None)


def test_unit_stage_returns_its_input(eng):
    sh.check_unit_stage_returns_its_input(eng, STAGE, (1,))


@pytest.mark.parametrize("L,ntaps", [(1, 5), (3, 155), (4, 31), (64, 100)])
def test_add_is_one_float32_addition_per_part(eng, L, ntaps):
    rng = np.random.default_rng(31 * L)
    x = _stream(rng, 7000 // L + 3, 0.1)
    w = _stream(rng, len(x) * L, 0.1)
    taps = (rng.standard_normal(ntaps) * np.sqrt(L / float(ntaps))).astype(np.float32)
    sh.check_single_add_is_one_float32_addition_per_part(eng, STAGE, (L,), taps, x, w)


def _chunk_sizes(rng, n, L, ntaps):
    Q = duc_cases.history(ntaps, L)
    tin = duc_cases.tile_outputs(L) // L
    sizes = [s for s in (0, 1, Q - 1, Q, Q + 1, 997, tin - 1, tin, tin + 1) if s >= 0]
    out, left = [], n
    seq = list(sizes)                       # every size once, then random draws
    while left > 0:
        s = min(seq.pop(0) if seq else int(rng.choice(sizes)), left)
        out.append(s)
        left -= s
    return out


@pytest.mark.parametrize("fmt", ["fc32", "sc16"])
@pytest.mark.parametrize("L,ntaps", [(1, 31), (2, 1024), (3, 155), (4, 31), (4, 3), (8, 155), (8, 7), (64, 1024), (64, 63),
                                     (5, 2), (17, 1)])
def test_any_segmentation_gives_the_same_bits(eng, L, ntaps, fmt):
    rng = np.random.default_rng(77 * L + ntaps)
    Q = duc_cases.history(ntaps, L)
    tin = duc_cases.tile_outputs(L) // L
    n = 3 * tin + 2 * Q + 1234 + (997 if L > 1 else 0)
    x = _stream(rng, n, 0.05)
    taps = (rng.standard_normal(ntaps) * np.sqrt(L / float(ntaps))).astype(np.float32)
    fc = FCS[2]
    try:
        _set(eng, L, taps, fc, fmt)
        whole = eng.duc(x).copy()
        _check_against_model(whole, x, taps, L, fc, 0, fmt, "whole L=%d ntaps=%d %s" % (L, ntaps, fmt))
        eng.duc_reset(0)
        sizes = _chunk_sizes(rng, n, L, ntaps)
        assert 0 in sizes and (Q < 2 or any(0 < s < Q for s in sizes))
        parts, a = [], 0
        for s in sizes:
            y = eng.duc(x[a:a + s])
            assert len(y) == s * L
            parts.append(y)
            a += s
        assert a == n and np.array_equal(np.concatenate(parts), whole)
        # ... and from a reset to a non-zero index
        first = 7 * 1024 + 5
        eng.duc_reset(first)
        w2 = eng.duc(x).copy()
        assert L == 1 and ntaps == 1 or not np.array_equal(w2, whole)
        eng.duc_reset(first)
        p2 = [eng.duc(x[i:i + 997]) for i in range(0, n, 997)]
        assert np.array_equal(np.concatenate(p2), w2)
    finally:
        eng.set_duc(None)


@pytest.mark.parametrize("name,fmt", [("qpsk512_r4", "fc32"), ("qpsk512_r4", "sc16"), ("qam16_2048_r2", "fc32"),
                                      ("bpsk64_r8", "fc32"), ("qpsk512_r3", "fc32")])
def test_two_links_end_to_end(orc, name, fmt):
    """Engine.tx -> Engine.duc per link (the second added onto the first) -> the noise of ddc_cases -> Engine.ddc ->
    Engine.rx per link: nothing but the noise is made on the host."""
    cfg0 = make_cfg(*ddc_cases.CASES[name][:4])
    e = engine.Engine(cfg=cfg0)
    try:
        k = duc_cases.links(name, tx=_engine_tx(e))
        R, (xa, xb), (fa, fb) = k["R"], k["x"], k["freqs"]
        e.set_duc(duc.duc_cfg(R, fa, taps=k["tx_taps"]))
        wa = e.duc(xa)
        noisy = (wa.astype(np.complex128) + duc_cases.noise(len(wa), k["P"], R)).astype(np.complex64)
        if fmt == "sc16":
            # the noise goes into the band before the second link is added onto it: the final store is the 16-bit one
            e.set_duc(duc.duc_cfg(R, fb, taps=k["tx_taps"], out_format="sc16"))
            wide = e.duc(xb, add=noisy)
            assert wide.dtype == np.int16 and wide.shape == (len(xa) * R, 2)
            assert int(wide.min()) > -32768 and int(wide.max()) < 32767, "a stored part sits on the rail"
        else:
            e.set_duc(duc.duc_cfg(R, fb, taps=k["tx_taps"]))
            both = e.duc(xb, add=wa)
            e.duc_reset(0)
            assert np.array_equal(both, _part_sum(wa, e.duc(xb)))
            wide = (both.astype(np.complex128) + duc_cases.noise(len(wa), k["P"], R)).astype(np.complex64)
            peak = float(np.max(np.abs(wide)))
            print("%s: peak |sample| of the noisy two-link band = %.3f" % (name, peak))
        e.set_duc(None)
        for fc, sent in zip((fa, fb), k["payloads"]):
            e.set_rx_iq_format(fmt)
            e.set_ddc(ddc.ddc_cfg(R, fc, taps=k["rx_taps"]))
            y = e.ddc(wide)
            e.set_rx_iq_format("fc32")
            e.set_ddc(None)
            got = e.rx(y)
            assert got == orc.rx(k["cfg"], y).packets, (name, fc)
            assert [ok for ok, _ in got] == [True] * 4 and [p for _, p in got] == sent, (name, fc)
    finally:
        e.close()


@pytest.mark.parametrize("fmt", ["fc32", "sc16"])
def test_modulator_with_the_stage_feeds_the_demodulator_with_its_front_end(fmt):
    sh.check_modulator_with_the_stage_feeds_the_demodulator(
        STAGE, (4,), fmt, dict(duc=dict(interpolation=4, center_freq=-0.25)), dict(ddc=dict(decimation=4, center_freq=-0.25)),
        ntaps=31, ratio=4, unconfigured=())


def test_transmit_path_and_command_line_take_the_stage(tmp_path):
    def as_the_command_line(opt):
        opt.duc_interp, opt.duc_freq = 4, 0.25
    sh.check_transmit_path_and_command_line(
        STAGE, tmp_path, as_the_command_line, dict(interpolation=4, center_freq=0.25, ntaps=31),
        tx_flags=["--duc-interp", "4", "--duc-freq", "0.25"], rx_flags=["--ddc-decim", "4", "--ddc-freq", "0.25"],
        rx_flags_other=["--ddc-decim", "4", "--ddc-freq", "-0.25"], ratio=4, period=4)


def test_device_pointer_path_behind_an_asynchronous_transmit():
    torch = pytest.importorskip("torch")
    sh.check_single_device_pointer_path_behind_an_asynchronous_transmit(torch, STAGE, (4,), 0.25, duc.design(4, 200 / 512.0))


def test_invalid_arguments_are_refused(eng):
    bads = (dict(struct_size=12), dict(interpolation=0), dict(interpolation=65), dict(ntaps=0), dict(ntaps=1025),
            dict(out_format=2), dict(out_format=1, out_scale=-1.0), dict(out_format=1, out_scale=float("inf")),
            dict(out_format=1, out_scale=float("nan")), dict(center_freq=0.5000001), dict(center_freq=-0.51),
            dict(center_freq=float("nan")))
    sh.check_tx_single_invalid_arguments(eng, STAGE, lambda: duc.duc_cfg(4, 0.25, taps=np.ones(5, np.float32)), 64, (4,), bads,
                                         still_refused=dict(interpolation=65), sc16_shape=(256, 2))


def test_a_tiny_negative_frequency_is_phase_step_zero(eng):
    rng = np.random.default_rng(9)
    x = _stream(rng, 700, 0.1)
    taps = (rng.standard_normal(9) / 3).astype(np.float32)
    try:
        assert duc_cases.phase_step(-1e-20) == 0
        _set(eng, 4, taps, -1e-20)
        eng.duc_reset(1000003)
        y = eng.duc(x)
        _check_against_model(y, x, taps, 4, -1e-20, 1000003, "fc32", "fc=-1e-20")
        _set(eng, 4, taps, 0.0)
        eng.duc_reset(1000003)
        assert np.array_equal(eng.duc(x), y)
    finally:
        eng.set_duc(None)


def test_capacity_error_leaves_the_stream_state(eng):
    x = _stream(np.random.default_rng(5), 5000, 0.1)
    sh.check_capacity_error_leaves_the_stream_state(eng, STAGE, (3,), 0.2, duc.design(3, 0.4), x)


def test_without_a_duc_transmitter_and_receiver_launch_what_they_launched(orc):
    sh.check_transmitter_and_receiver_launch_what_they_launched(STAGE, (4,), 0.25, duc.design(4, 200 / 512.0),
                                                                nout=12000)
