"""The resampler bank on the GPU (k_resamp_bank, Engine.resamp_bank, ofdm_demod_resamp_bank): every link bit for bit the
single resampler, under any segmentation, link order and link count; end to end on the two-link wideband captures;
layout, errors, independence from the other front ends, device pointers."""
import ctypes as C

import numpy as np
import pytest

import resamp_bank_cases as bc
import resamp_cases
import stage_harness as sh
from ofdm_uhd_amd import _abi, config, ddc, engine, ofdm, resample
from stage_harness import eng   # noqa: F401 (one handle per file)

pytestmark = pytest.mark.gpu

STAGE = sh.STAGES["resamp_bank"]
_stream, _options = sh.rx_stream, sh.options_of


@pytest.mark.parametrize("fmt", ["fc32", "sc16"])
@pytest.mark.parametrize("L,M", sorted(bc.TAP_GRID))
def test_every_link_is_the_single_resampler_bit_for_bit(eng, L, M, fmt):
    n = bc.stream_length(L, M)
    tile = bc.tile_inputs(L, M, 8)
    assert n % tile != 0 and (M == 1 or n % M != 0)
    sh.check_every_link_is_the_single_stage(eng, STAGE, (L, M), fmt, seed=5000 + 64 * L + M, n=n, start=bc.far_start(M))


@pytest.mark.parametrize("fmt", ["fc32", "sc16"])
@pytest.mark.parametrize("L,M,ntaps,K", bc.SEG_SHAPES)
def test_any_segmentation_gives_the_same_bits(eng, L, M, ntaps, K, fmt):
    n = 3 * bc.tile_inputs(L, M, K) + 1234 + 2 * ((ntaps - 1) // L)
    sh.check_rx_segmentation(eng, STAGE, (L, M), ntaps, K, fmt, seed=77 * L + 5 * M + ntaps + K, n=n)


@pytest.mark.parametrize("L,M,ntaps", [(2, 5, 39), (8, 25, 481), (3, 25, 155), (64, 64, 1024)])
def test_link_order_and_count_do_not_matter(eng, L, M, ntaps):
    sh.check_link_order_and_count_do_not_matter(eng, STAGE, (L, M), ntaps, seed=17 + 64 * L + M)


@pytest.mark.parametrize("name,fmt", [("qpsk512_2_5", "fc32"), ("qpsk512_2_5", "sc16"), ("bpsk64_8_25", "fc32")])
def test_two_links_end_to_end(orc, name, fmt):
    cap = resamp_cases.capture(name)
    L, M, cfg, freqs = cap["L"], cap["M"], cap["cfg"], list(cap["freqs"])
    wide = sh.wide_sc16(cap["wide"]) if fmt == "sc16" else cap["wide"]
    # per link, what ofdm_demod(resample=...) returns: CRC-ok, the transmitted payloads
    per_link = []
    for fc, sent in zip(freqs, cap["payloads"]):
        d = ofdm.ofdm_demod(_options(cap), iq_format=fmt,
                            resample=dict(interpolation=L, decimation=M, center_freq=fc, taps=cap["taps"]))
        try:
            got = d.work(wide)
        finally:
            d.engine().close()
        assert [ok for ok, _ in got] == [True] * 4 and [p for _, p in got] == sent, (name, fc)
        per_link.append(got)
    order = []
    bank = ofdm.ofdm_demod_resamp_bank(_options(cap), freqs, L, M, taps=cap["taps"], iq_format=fmt,
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
        assert bank.work(wide) == per_link                 # a stream starts afresh after a flush
        # the bank's streams are the single stage's, and the oracle's receiver finds the same packets in them
        e = bank.engine()
        e.set_rx_iq_format(fmt)
        e.resamp_bank_reset(0)
        y = e.resamp_bank(wide)
        assert y.shape == (2, resamp_cases.count(0, len(wide), L, M))
        for i in range(2):
            assert orc.rx(cfg, np.ascontiguousarray(y[i])).packets == per_link[i], (name, i)
    finally:
        bank.close()
    assert bank.engine()._h.value is None and all(d.engine()._h.value is None for d in bank.links())


def test_links_that_differ_in_modulation_and_the_command_line(orc, tmp_path):
    cap = resamp_cases.capture("qpsk512_2_5")
    sh.check_links_that_differ_in_modulation_and_the_command_line(
        cap, tmp_path, lambda opts: ofdm.ofdm_demod_resamp_bank(opts, list(cap["freqs"]), 2, 5, taps=cap["taps"]),
        ["--resamp-interp", "2", "--resamp-decim", "5"], freq_flag=(["--resamp-freq", "0.22"], ["--resamp-freq", "-0.21"]),
        freqs_flag=["--resamp-freqs", "0.22,-0.21"])


def test_layout_and_capacity(eng):
    fcs = [0.2, -0.1, 0.37]
    sh.check_rx_layout_and_capacity(eng, STAGE, (2, 5), fcs, resample.design(2, 5, 0.4), one_sel=fcs[1:2])


def test_invalid_arguments_are_refused(eng):
    """Every refusal is made on the host, before any launch: the buffers handed over are valid throughout."""
    x = np.zeros(64, np.complex64)
    x[::3] = 1.0

    def index_limit_and_null_pointers(lib, x, out):
        # the index limit is the resampler's
        eng.resamp_bank_reset(1 << 56)
        with pytest.raises(ValueError):
            eng.resamp_bank_reset((1 << 56) + 1)
        assert STAGE.raw(eng._h, x, out, 64, 64)[0] == _abi.OFDM_E_INVAL          # the index would pass 2^56
        eng.resamp_bank_reset(0)
        nn = C.c_uint64(0)
        xp, op = x.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
        assert lib.ofdm_resamp_bank(eng._h, None, 64, op, 64, 64, C.byref(nn)) == _abi.OFDM_E_INVAL
        assert lib.ofdm_resamp_bank(eng._h, xp, 64, None, 64, 64, C.byref(nn)) == _abi.OFDM_E_INVAL
        assert lib.ofdm_resamp_bank(eng._h, xp, 64, op, 64, 64, None) == _abi.OFDM_E_INVAL
        assert eng.resamp_bank_count(64) == resamp_cases.count(0, 64, 2, 5)     # ... and the stream did not move
    base = lambda: resample.bank_cfg(2, 5, [0.25, -0.1], taps=np.ones(5, np.float32))
    sh.check_rx_bank_invalid_arguments(eng, STAGE, (2, 5), base, x, nout=resamp_cases.count(0, 64, 2, 5),
                                       after62=(resamp_cases.count(62, 2, 2, 5), 1), still_refused=7, edge_sel=[0.5, -0.5],
                                       middle=index_limit_and_null_pointers)


def test_the_front_ends_on_one_handle_do_not_disturb_each_other(eng):
    """The bank, resamp, ddc and ddc_bank configured on one handle, calls interleaved in different chunkings: each gives
    the bits of an uninterrupted run."""
    rng = np.random.default_rng(23)
    n = 9000
    raw, _ = _stream(rng, n, "fc32")
    t_rb, t_rs, t_dd, t_db = bc.taps_for(rng, 155), bc.taps_for(rng, 39), bc.taps_for(rng, 31), bc.taps_for(rng, 63)
    fcs = [0.11, -0.4, 0.25]
    cfgs = dict(resamp_bank=lambda: resample.bank_cfg(8, 25, fcs, taps=t_rb),
                resamp=lambda: resample.resamp_cfg(2, 5, 0.2, taps=t_rs),
                ddc=lambda: ddc.ddc_cfg(3, 0.2, taps=t_dd),
                ddc_bank=lambda: ddc.bank_cfg(4, [0.3, -0.2], taps=t_db))
    steps = dict(resamp_bank=1777, resamp=1300, ddc=2111, ddc_bank=901)
    stages = {name: (lambda name=name: getattr(eng, "set_" + name)(cfgs[name]()),
                     lambda a, b, name=name: getattr(eng, name)(raw[a:b]), n, steps[name]) for name in cfgs}
    off = {name: getattr(eng, "set_" + name) for name in cfgs}
    try:
        alone = sh.check_interleaved(stages, off)
        # dropping or resetting another stage leaves the bank's stream where it was, and the other way round
        eng.resamp_bank(raw[:100])
        eng.resamp(raw[:50])
        eng.resamp_reset(0)
        eng.set_ddc_bank(None)
        assert eng.resamp_bank_count(25) == resamp_cases.count(n + 100, 25, 8, 25)
        eng.set_resamp_bank(None)
        assert eng.resamp_count(5) == resamp_cases.count(0, 5, 2, 5) and np.array_equal(eng.resamp(raw), alone["resamp"])
    finally:
        eng.set_resamp_bank(None)
        eng.set_resamp(None)
        eng.set_ddc(None)
        eng.set_ddc_bank(None)


def test_without_a_bank_the_receiver_launches_what_it_launched(orc):
    cap = resamp_cases.capture("qpsk512_2_5")
    sh.check_receiver_launches_what_it_launched(STAGE, (2, 5), cap, cap["freqs"])


@pytest.mark.parametrize("fmt", ["fc32", "sc16"])
def test_device_pointers(fmt):
    """Driven as tools/bench_resamp_bank.py drives resamp_bank_device: torch buffers, raw pointers; a row goes straight
    into rx_device."""
    import torch
    cap = resamp_cases.capture("qpsk512_2_5")
    K = 5
    wide = sh.wide_sc16(cap["wide"]) if fmt == "sc16" else cap["wide"]
    fcs = list(cap["freqs"]) + [0.4, -0.45, 0.01]
    host = engine.Engine(cfg=cap["cfg"])
    devE = engine.Engine(cfg=config.make_cfg(_options(cap), device_ptrs=True))
    x = y = pay = None
    try:
        x, y, want, no, stride = sh.check_rx_device_pointers(
            torch, STAGE, host, devE, resample.bank_cfg(2, 5, fcs, taps=cap["taps"]), wide, K, fmt, clear_between=True)
        dev = x.device
        # row 1 goes straight into the receiver (complex64, whatever the wideband format)
        host.set_rx_iq_format("fc32")
        devE.set_rx_iq_format("fc32")
        pk = host.rx(want[1])
        assert [ok for ok, _ in pk] == [True] * 4 and [p for _, p in pk] == cap["payloads"][1]
        pcap = no + 4096
        pay = torch.zeros(pcap, dtype=torch.uint8, device=dev)
        npk, poff, ln, ok = devE.rx_device(y.data_ptr() + 8 * stride, no, pay.data_ptr(), pcap, 64)
        torch.cuda.synchronize()
        assert npk == 4 and ok.astype(bool).tolist() == [True] * 4
        b = pay.cpu().numpy()
        assert [bytes(b[int(poff[i]):int(poff[i]) + int(ln[i])]) for i in range(npk)] == [p for _, p in pk]
    finally:
        host.close()
        devE.close()
        # leave nothing behind in torch's cached blocks
        for t in (x, y, pay):
            if t is not None:
                t.zero_()
        torch.cuda.synchronize()
        del x, y, pay
        torch.cuda.empty_cache()
