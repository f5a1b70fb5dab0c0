"""The DDC bank on the GPU (k_ddc_bank, Engine.ddc_bank, ofdm_demod_bank): every link bit for bit the single DDC, under
any segmentation, link order and link count; end to end on the two-link wideband captures; layout, errors, independence
from the single DDC, device pointers."""
import numpy as np
import pytest

import ddc_bank_cases as bc
import ddc_cases
import stage_harness as sh
from helpers import make_cfg
from ofdm_uhd_amd import config, ddc, engine, ofdm, options
from stage_harness import eng   # noqa: F401 (one handle per file)

pytestmark = pytest.mark.gpu

STAGE = sh.STAGES["ddc_bank"]
_stream, _options = sh.rx_stream, sh.options_of


@pytest.mark.parametrize("fmt", ["fc32", "sc16"])
@pytest.mark.parametrize("R", sorted(bc.TAP_GRID))
def test_every_link_is_the_single_ddc_bit_for_bit(eng, R, fmt):
    n = bc.stream_length(R)
    tile = bc.tile_outputs(R, 8) * R
    assert n % tile != 0 and n % (ddc_cases.tile_outputs(R) * R) != 0 and (R == 1 or n % R != 0)
    start = 1000003 if 1000003 % R else 1000004
    assert start % R != 0 or R == 1
    sh.check_every_link_is_the_single_stage(eng, STAGE, (R,), fmt, seed=4000 + R, n=n, start=start)


SEG_SHAPES = [(1, 31, 2), (2, 1024, 8), (3, 155, 3), (4, 31, 4), (8, 155, 4), (64, 1024, 8), (64, 63, 2), (17, 1, 3)]


@pytest.mark.parametrize("fmt", ["fc32", "sc16"])
@pytest.mark.parametrize("R,ntaps,K", SEG_SHAPES)
def test_any_segmentation_gives_the_same_bits(eng, R, ntaps, K, fmt):
    n = 3 * bc.tile_outputs(R, K) * R + 1234 + 2 * ntaps
    sh.check_rx_segmentation(eng, STAGE, (R,), ntaps, K, fmt, seed=91 * R + ntaps + K, n=n)


@pytest.mark.parametrize("R,ntaps", [(4, 31), (8, 155), (64, 63)])
def test_link_order_and_count_do_not_matter(eng, R, ntaps):
    sh.check_link_order_and_count_do_not_matter(eng, STAGE, (R,), ntaps, seed=17 + R)


@pytest.mark.parametrize("name,fmt", [("qpsk512_r4", "fc32"), ("qpsk512_r4", "sc16"), ("qam16_2048_r2", "fc32"),
                                      ("bpsk64_r8", "fc32"), ("qpsk512_r3", "fc32")])
def test_two_links_end_to_end(orc, name, fmt):
    cap = ddc_cases.capture(name)
    R, cfg, freqs = cap["R"], cap["cfg"], list(cap["freqs"])
    wide = sh.wide_sc16(cap["wide"]) if fmt == "sc16" else cap["wide"]
    e = engine.Engine(cfg=cfg)
    try:
        e.set_rx_iq_format(fmt)
        e.set_ddc_bank(ddc.bank_cfg(R, freqs, taps=cap["taps"]))
        y = e.ddc_bank(wide)                              # one call, both links
        e.set_rx_iq_format("fc32")
        assert y.shape == (2, ddc_cases.count(0, len(wide), R))
        per_link = []
        for i, sent in enumerate(cap["payloads"]):
            got = e.rx(y[i])
            assert got == orc.rx(cfg, np.ascontiguousarray(y[i])).packets, (name, i)
            assert [ok for ok, _ in got] == [True] * 4 and [p for _, p in got] == sent, (name, i)
            per_link.append(got)
    finally:
        e.close()
    order = []
    bank = ofdm.ofdm_demod_bank(_options(cap), freqs, R, taps=cap["taps"], iq_format=fmt,
                                callback=lambda link, ok, p: order.append((link, ok, p)))
    try:
        assert bank.work(wide) == per_link, name
        assert order == [(i, ok, p) for i in range(2) for ok, p in per_link[i]]   # link 0's packets, then link 1's
        del order[:]
        chunks = [[], []]
        for a in range(0, len(wide), 5000):
            calls = len(order)
            out = bank.feed(wide[a:a + 5000])
            assert [(l, ok, p) for l, ok, p in order[calls:]] == [(i, ok, p) for i in range(2) for ok, p in out[i]]
            for i in range(2):
                chunks[i] += out[i]
        out = bank.flush()
        for i in range(2):
            chunks[i] += out[i]
        assert chunks == per_link, name
        assert bank.work(wide) == per_link                # a stream starts afresh after a flush
    finally:
        bank.close()
    assert bank.engine()._h.value is None and all(d.engine()._h.value is None for d in bank.links())
    for i, fc in enumerate(freqs):
        d = ofdm.ofdm_demod(_options(cap), iq_format=fmt, ddc=dict(decimation=R, center_freq=fc, taps=cap["taps"]))
        try:
            assert d.work(wide) == per_link[i], (name, fc)
        finally:
            d.engine().close()


def test_links_that_differ_in_modulation_and_the_command_line(orc, tmp_path):
    cap = ddc_cases.capture("qpsk512_r4")
    sh.check_links_that_differ_in_modulation_and_the_command_line(
        cap, tmp_path, lambda opts: ofdm.ofdm_demod_bank(opts, cap["freqs"], 4, taps=cap["taps"]), ["--ddc-decim", "4"],
        freq_flag=(["--ddc-freq", "0.25"], ["--ddc-freq", "-0.25"]), freqs_flag=["--ddc-freqs", "0.25,-0.25"])


def test_layout_and_capacity(eng):
    fcs = [0.2, -0.1, 0.37]
    sh.check_rx_layout_and_capacity(eng, STAGE, (3,), fcs, ddc.design(3, 0.4), one_sel=fcs[1:2])


def test_invalid_arguments_are_refused(eng):
    base = lambda: ddc.bank_cfg(4, [0.25, -0.1], taps=np.ones(5, np.float32))
    sh.check_rx_bank_invalid_arguments(eng, STAGE, (4,), base, np.zeros(64, np.complex64), nout=16, after62=(0, 1),
                                       still_refused=5, edge_sel=[0.5, -0.5])


def test_phase_step_and_index_limits(eng):
    """As the DDC's test of the same name: fc R a hair below a whole turn gives phase step 0; stream indices are refused
    before 64-bit arithmetic could wrap."""
    sh.check_phase_step_zero_and_index_limit(eng, STAGE, [0.3, -1e-20], link=(1,))


def test_bank_and_single_ddc_on_one_handle_do_not_disturb_each_other(eng):
    rng = np.random.default_rng(23)
    n = 9000
    raw, _ = _stream(rng, n, "fc32")
    t_bank, t_one = bc.taps_for(rng, 155), bc.taps_for(rng, 31)
    fcs = [0.11, -0.4, 0.25]
    try:
        eng.set_ddc_bank(ddc.bank_cfg(8, fcs, taps=t_bank))
        bank_alone = eng.ddc_bank(raw).copy()
        eng.set_ddc_bank(None)
        eng.set_ddc(ddc.ddc_cfg(3, 0.2, taps=t_one))
        one_alone = eng.ddc(raw).copy()
        # both configured, calls interleaved, different chunkings and different stream origins
        eng.set_ddc_bank(ddc.bank_cfg(8, fcs, taps=t_bank))
        eng.set_ddc(ddc.ddc_cfg(3, 0.2, taps=t_one))
        pb, po, ib, io = [], [], 0, 0
        while ib < n or io < n:
            if ib < n:
                pb.append(eng.ddc_bank(raw[ib:ib + 1777]).copy())
                ib += 1777
            if io < n:
                po.append(eng.ddc(raw[io:io + 1300]).copy())
                io += 1300
        assert np.array_equal(np.concatenate(pb, axis=1), bank_alone)
        assert np.array_equal(np.concatenate(po), one_alone)
        # dropping or resetting one leaves the other's stream where it was
        eng.ddc_bank(raw[:100])
        eng.ddc(raw[:50])
        eng.ddc_reset(0)
        assert eng.ddc_bank_count(4) == ddc_cases.count(n + 100, 4, 8)
        eng.set_ddc_bank(None)
        assert eng.ddc_count(2) == ddc_cases.count(0, 2, 3) and np.array_equal(eng.ddc(raw), one_alone)
    finally:
        eng.set_ddc_bank(None)
        eng.set_ddc(None)


def test_without_a_bank_the_receiver_launches_what_it_launched(orc):
    cap = ddc_cases.capture("qpsk512_r4")
    sh.check_receiver_launches_what_it_launched(STAGE, (4,), cap, cap["freqs"])


@pytest.mark.parametrize("fmt", ["fc32", "sc16"])
def test_device_pointers(fmt):
    """Driven as tools/bench_ddc.py drives ddc_device: torch buffers, raw pointers."""
    import torch
    R, K = 8, 5
    rng = np.random.default_rng(31)
    n = 3 * bc.tile_outputs(R, K) * R + 77
    raw, _ = _stream(rng, n, fmt)
    taps = ddc.design(R, 0.75)
    fcs = [float(f) for f in rng.uniform(-0.5, 0.5, K)]
    host = engine.Engine(cfg=make_cfg())
    opt = options.default_options(modulation="qpsk")
    devE = engine.Engine(cfg=config.make_cfg(opt, device_ptrs=True))
    try:
        sh.check_rx_device_pointers(torch, STAGE, host, devE, ddc.bank_cfg(R, fcs, taps=taps), raw, K, fmt)
    finally:
        host.close()
        devE.close()
