"""The rational-rate transmit stage on the GPU (k_tx_resamp, Engine.tx_resamp, ofdm_mod(resample=...)): against the
float64 model of its definition, bit for bit against the DUC at M = 1, under arbitrary segmentation of the stream, end
to end through the receive resampler on bands built on the device, through the public objects, and at its edges."""
import numpy as np
import pytest

import stage_harness as sh
import tx_resamp_cases as cases
from helpers import make_cfg
from ofdm_uhd_amd import duc, engine, resample, tx_resample
from stage_harness import eng   # noqa: F401 (one handle per file)

pytestmark = pytest.mark.gpu

STAGE = sh.STAGES["tx_resamp"]
FCS = (0.0, 0.25, -1.0 / 3.0 + 0.013, -0.5)
RATIOS = ((1, 1), (2, 1), (5, 2), (3, 4), (4, 3), (25, 8), (8, 25), (64, 63), (64, 1), (1, 64), (7, 64))
_stream, _part_sum, _engine_tx = sh.tx_stream, sh.part_sum, sh.engine_tx


def _tap_counts(L):
    return sorted(n for n in {1, L - 1, L, 39, 481, 1024} if n >= 1)


def _taps(rng, ntaps, L):
    return (rng.standard_normal(ntaps) * np.sqrt(L / float(ntaps))).astype(np.float32)


def _set(eng, L, M, taps, fc, fmt="fc32"):
    eng.set_tx_resamp(tx_resample.tx_resamp_cfg(L, M, fc, taps=taps, out_format=fmt))


def _check_against_model(y, x, taps, L, M, fc, first, fmt, what, add=None):
    return sh.check_tx_model(y, x, taps, STAGE, (L, M), fc, first, fmt, what, add=add)


@pytest.mark.parametrize("fmt", ["fc32", "sc16"])
@pytest.mark.parametrize("L,M", RATIOS)
def test_against_float64_model(eng, L, M, fmt):
    rng = np.random.default_rng(3000 + 100 * L + M)
    tin = cases.tile_inputs(L, M)
    n = 3 * tin + tin // 3 + 5                                   # three tiles and a ragged end
    x = _stream(rng, n, 0.05)
    worst = 0.0
    try:
        for ti, ntaps in enumerate(_tap_counts(L)):
            taps = _taps(rng, ntaps, L)
            for fi, fc in enumerate(FCS):
                _set(eng, L, M, taps, fc, fmt)
                # with and without `add`, alternating so that every tap count and every frequency sees both
                add = _stream(rng, cases.count(0, n, L, M), 0.05) if (ti + fi) % 2 else None
                y = eng.tx_resamp(x, add=add)
                worst = max(worst, _check_against_model(y, x, taps, L, M, fc, 0, fmt, "L=%d M=%d ntaps=%d fc=%g %s add=%s" % (
                    L, M, ntaps, fc, fmt, add is not None), add=add))
        # once more far from index 0 with the generic frequency: n D mod 2^64 at input index 10^6
        for add_on in (False, True):
            taps = _taps(rng, 39, L)
            _set(eng, L, M, taps, FCS[2], fmt)
            assert cases.phase_step(FCS[2]) % (1 << 32) != 0
            eng.tx_resamp_reset(1000003)
            add = _stream(rng, cases.count(1000003, n, L, M), 0.05) if add_on else None
            worst = max(worst, _check_against_model(eng.tx_resamp(x, add=add), x, taps, L, M, FCS[2], 1000003, fmt,
                                                    "L=%d M=%d reset to 1000003 %s" % (L, M, fmt), add=add))
    finally:
        eng.set_tx_resamp(None)
    print("L=%d M=%d %s: worst error / bound = %.3g" % (L, M, fmt, worst))


@pytest.mark.parametrize("L", [1, 2, 4, 5, 8, 64])
def test_decimation_one_is_the_duc_bit_for_bit(eng, L):
    rng = np.random.default_rng(500 + L)
    tout = cases.tile_inputs(L, 1) * L
    n = (2 * tout + tout // 3) // L + 5
    x = _stream(rng, n, 0.05)
    w = _stream(rng, n * L, 0.05)
    try:
        for ntaps in (1, 31, 155, 1024):
            taps = _taps(rng, ntaps, L)
            for fmt in ("fc32", "sc16"):
                for add in (None, w):
                    for first in (0, 1000003):
                        eng.set_duc(duc.duc_cfg(L, FCS[2], taps=taps, out_format=fmt))
                        eng.duc_reset(first)
                        want = eng.duc(x, add=add)
                        _set(eng, L, 1, taps, FCS[2], fmt)
                        eng.tx_resamp_reset(first)
                        got = eng.tx_resamp(x, add=add)
                        assert got.dtype == want.dtype and np.array_equal(got, want), (L, ntaps, fmt, add is not None, first)
                        assert np.any(got)
    finally:
        eng.set_duc(None)
        eng.set_tx_resamp(None)


def test_unit_stage_returns_its_input(eng):
    sh.check_unit_stage_returns_its_input(eng, STAGE, (1, 1))


@pytest.mark.parametrize("L,M,ntaps", [(1, 1, 5), (5, 2, 39), (3, 4, 41), (64, 63, 100)])
def test_add_is_one_float32_addition_per_part(eng, L, M, ntaps):
    rng = np.random.default_rng(31 * L + M)
    x = _stream(rng, 7000 * M // L + 3, 0.1)
    w = _stream(rng, cases.count(0, len(x), L, M), 0.1)
    sh.check_single_add_is_one_float32_addition_per_part(eng, STAGE, (L, M), _taps(rng, ntaps, L), x, w)


def _chunk_sizes(rng, n, L, M, ntaps):
    Q = cases.history(ntaps, L)
    tin = cases.tile_inputs(L, M)
    sizes = [s for s in (0, 1, L - 1, M, Q - 1, Q + 1, 997, tin - 1, tin, tin + 1) if s >= 0]
    out, left = [], n
    # every size once, at L < M then M single inputs in a row (they complete L < M outputs: some call produces
    # nothing), then random draws
    seq = list(sizes) + ([1] * M if L < M else [])
    while left > 0:
        s = min(seq.pop(0) if seq else int(rng.choice(sizes + [int(rng.integers(1, 3000))])), left)
        out.append(s)
        left -= s
    return out


@pytest.mark.parametrize("fmt", ["fc32", "sc16"])
@pytest.mark.parametrize("L,M,ntaps", [(1, 1, 31), (2, 1, 1024), (5, 2, 39), (3, 4, 41), (25, 8, 481), (8, 25, 155),
                                       (64, 63, 1024), (7, 64, 200)])
def test_any_segmentation_gives_the_same_bits(eng, L, M, ntaps, fmt):
    rng = np.random.default_rng(77 * L + 13 * M + ntaps)
    Q = cases.history(ntaps, L)
    tin = cases.tile_inputs(L, M)
    n = 3 * tin + 2 * Q + 1234 + 997
    x = _stream(rng, n, 0.05)
    taps = _taps(rng, ntaps, L)
    fc = FCS[2]
    try:
        for first in (0, 7 * 1024 + 5):
            assert M == 1 or first == 0 or (first * L) % M != 0
            w = _stream(rng, cases.count(first, n, L, M), 0.05)
            for add in (None, w):
                _set(eng, L, M, taps, fc, fmt)
                eng.tx_resamp_reset(first)
                whole = eng.tx_resamp(x, add=add).copy()
                _check_against_model(whole, x, taps, L, M, fc, first, fmt, "whole L=%d M=%d ntaps=%d %s" % (L, M, ntaps, fmt),
                                     add=add)
                eng.tx_resamp_reset(first)
                sizes = _chunk_sizes(rng, n, L, M, ntaps) if first == 0 else [997] * (n // 997) + [n % 997]
                parts, a, o, empty = [], 0, 0, 0
                for s in sizes:
                    cnt = cases.count(first + a, s, L, M)
                    assert eng.tx_resamp_count(s) == cnt
                    y = eng.tx_resamp(x[a:a + s], add=None if add is None else add[o:o + cnt])
                    assert len(y) == cnt
                    empty += s > 0 and cnt == 0
                    parts.append(y)
                    a += s
                    o += cnt
                assert a == n and o == len(whole) and np.array_equal(np.concatenate(parts), whole)
                if first == 0:
                    assert 0 in sizes and (Q < 2 or any(0 < s < Q for s in sizes))
                    assert L >= M or empty > 0          # at L < M some call produced nothing
    finally:
        eng.set_tx_resamp(None)


@pytest.mark.parametrize("name,fmt", [("qpsk512_5_2", "fc32"), ("qpsk512_5_2", "sc16"), ("qam16_512_3_4", "fc32"),
                                      ("bpsk64_25_8", "fc32")])
def test_links_end_to_end(orc, name, fmt):
    """Engine.tx -> Engine.tx_resamp per link (the second added onto the first) -> the noise of resamp_cases ->
    Engine.resamp -> Engine.rx per link: nothing but the noise is made on the host."""
    cfg0 = make_cfg(*cases.CASES[name][:4])
    e = engine.Engine(cfg=cfg0)
    try:
        k = cases.links(name, tx=_engine_tx(e))
        L, M, xs, fs = k["L"], k["M"], k["x"], k["freqs"]
        nw = cases.count(0, len(xs[0]), L, M)
        e.set_tx_resamp(tx_resample.tx_resamp_cfg(L, M, fs[0], taps=k["tx_taps"]))
        wa = e.tx_resamp(xs[0])
        assert len(wa) == nw
        noise = cases.noise(nw, k["P"], L, M)
        if fmt == "sc16":
            # the noise goes into the band before the second link is added onto it: the final store is the 16-bit one
            assert len(xs) == 2
            noisy = (wa.astype(np.complex128) + noise).astype(np.complex64)
            e.set_tx_resamp(tx_resample.tx_resamp_cfg(L, M, fs[1], taps=k["tx_taps"], out_format="sc16"))
            wide = e.tx_resamp(xs[1], add=noisy)
            assert wide.dtype == np.int16 and wide.shape == (nw, 2)
            assert int(wide.min()) > -32768 and int(wide.max()) < 32767, "a stored part sits on the rail"
        else:
            both = wa
            if len(xs) == 2:
                e.set_tx_resamp(tx_resample.tx_resamp_cfg(L, M, fs[1], taps=k["tx_taps"]))
                both = e.tx_resamp(xs[1], add=wa)
                e.tx_resamp_reset(0)
                assert np.array_equal(both, _part_sum(wa, e.tx_resamp(xs[1])))
            wide = (both.astype(np.complex128) + noise).astype(np.complex64)
        e.set_tx_resamp(None)
        for fc, sent in zip(fs, k["payloads"]):
            e.set_rx_iq_format(fmt)
            e.set_resamp(resample.resamp_cfg(M, L, fc, taps=k["rx_taps"]))
            y = e.resamp(wide)
            e.set_rx_iq_format("fc32")
            e.set_resamp(None)
            got = e.rx(y)
            assert got == orc.rx(k["cfg"], y).packets, (name, fc)
            assert [ok for ok, _ in got] == [True] * 4 and [p for _, p in got] == sent, (name, fc)
    finally:
        e.close()


@pytest.mark.parametrize("fmt", ["fc32", "sc16"])
def test_modulator_with_the_stage_feeds_the_demodulator_with_its_resampler(fmt):
    sh.check_modulator_with_the_stage_feeds_the_demodulator(
        STAGE, (5, 2), fmt, dict(resample=dict(interpolation=5, decimation=2, center_freq=-0.21)),
        dict(resample=dict(interpolation=2, decimation=5, center_freq=-0.21)), ntaps=39, ratio=5 / 2.0,
        unconfigured=("duc",))


def test_transmit_path_and_command_line_take_the_stage(tmp_path):
    def as_the_command_line(opt):
        opt.tx_resamp_interp, opt.tx_resamp_decim, opt.tx_resamp_freq = 5, 2, 0.22
    sh.check_transmit_path_and_command_line(
        STAGE, tmp_path, as_the_command_line, dict(interpolation=5, decimation=2, center_freq=0.22, ntaps=39),
        tx_flags=["--tx-resamp-interp", "5", "--tx-resamp-decim", "2", "--tx-resamp-freq", "0.22"],
        rx_flags=["--resamp-interp", "2", "--resamp-decim", "5", "--resamp-freq", "0.22"],
        rx_flags_other=["--resamp-interp", "2", "--resamp-decim", "5", "--resamp-freq", "-0.22"], ratio=2.5, period=1)


def test_device_pointer_path_behind_an_asynchronous_transmit():
    torch = pytest.importorskip("torch")

    def at_decimation_one(dev, d_iq, nsamp):
        """... and at M = 1 the aliased call gives the DUC's bits"""
        w4 = _stream(np.random.default_rng(3), nsamp * 4, 0.1)
        t4 = duc.design(4, 200 / 512.0)
        d_o4 = torch.from_numpy(w4).cuda()
        dev.set_duc(duc.duc_cfg(4, 0.25, taps=t4))
        torch.cuda.synchronize()
        assert dev.duc_device(d_iq.data_ptr(), nsamp, d_o4.data_ptr(), nsamp * 4, add_ptr=d_o4.data_ptr()) == nsamp * 4
        ref = d_o4.cpu().numpy()
        d_o4.copy_(torch.from_numpy(w4))
        dev.set_tx_resamp(tx_resample.tx_resamp_cfg(4, 1, 0.25, taps=t4))
        torch.cuda.synchronize()
        assert dev.tx_resamp_device(d_iq.data_ptr(), nsamp, d_o4.data_ptr(), nsamp * 4, add_ptr=d_o4.data_ptr()) == nsamp * 4
        assert np.array_equal(d_o4.cpu().numpy(), ref) and not np.array_equal(ref, w4)
    sh.check_single_device_pointer_path_behind_an_asynchronous_transmit(
        torch, STAGE, (5, 2), 0.22, tx_resample.design(5, 2, 200 / 512.0), more=at_decimation_one)


def test_invalid_arguments_are_refused(eng):
    bads = (dict(struct_size=12), dict(interpolation=0), dict(interpolation=65), dict(decimation=0), dict(decimation=65),
            dict(ntaps=0), dict(ntaps=1025), dict(out_format=2), dict(out_format=1, out_scale=-1.0),
            dict(out_format=1, out_scale=float("inf")), dict(out_format=1, out_scale=float("nan")),
            dict(center_freq=0.5000001), dict(center_freq=-0.51), dict(center_freq=float("nan")))
    base = lambda: tx_resample.tx_resamp_cfg(4, 3, 0.25, taps=np.ones(5, np.float32))
    sh.check_tx_single_invalid_arguments(eng, STAGE, base, 66, (4, 3), bads, still_refused=dict(decimation=65),
                                         sc16_shape=(88, 2))


def test_capacity_error_leaves_the_stream_state(eng):
    x = _stream(np.random.default_rng(5), 5000, 0.1)
    sh.check_capacity_error_leaves_the_stream_state(eng, STAGE, (3, 4), 0.2, tx_resample.design(3, 4, 0.4), x)


def test_the_duc_and_this_stage_keep_separate_state_on_one_handle(eng):
    rng = np.random.default_rng(8)
    x = _stream(rng, 6000, 0.1)
    td, tr = duc.design(4, 0.4), tx_resample.design(5, 2, 0.4)
    try:
        eng.set_duc(duc.duc_cfg(4, 0.25, taps=td))
        want_d = eng.duc(x).copy()
        eng.set_tx_resamp(tx_resample.tx_resamp_cfg(5, 2, -0.2, taps=tr))
        want_r = eng.tx_resamp(x).copy()
        # the two streams interleaved, chunk by chunk, with a reset of one in the middle of the other
        eng.duc_reset(0)
        eng.tx_resamp_reset(0)
        pd, pr = [], []
        for a in range(0, 6000, 1000):
            pd.append(eng.duc(x[a:a + 1000]))
            pr.append(eng.tx_resamp(x[a:a + 1000]))
        assert np.array_equal(np.concatenate(pd), want_d) and np.array_equal(np.concatenate(pr), want_r)
        eng.duc_reset(0)
        half = eng.duc(x[:3000])
        eng.set_tx_resamp(tx_resample.tx_resamp_cfg(5, 2, -0.2, taps=tr))   # re-configuring one leaves the other's stream alone
        assert np.array_equal(np.concatenate([half, eng.duc(x[3000:])]), want_d)
        eng.tx_resamp(x[:3000])
        eng.set_duc(None)
        assert np.array_equal(eng.tx_resamp(x[3000:]), want_r[cases.count(0, 3000, 5, 2):])
    finally:
        eng.set_duc(None)
        eng.set_tx_resamp(None)


def test_without_the_stage_transmitter_and_receiver_launch_what_they_launched(orc):
    sh.check_transmitter_and_receiver_launch_what_they_launched(STAGE, (5, 2), 0.22, tx_resample.design(5, 2, 200 / 512.0),
                                                                nout=7500)
