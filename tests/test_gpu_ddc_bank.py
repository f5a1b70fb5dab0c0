"""The DDC bank on the GPU (k_ddc_bank, Engine.ddc_bank, ofdm_demod_bank): every link bit for bit the single DDC, under
any segmentation, link order and link count; end to end on the two-link wideband captures; layout, errors, independence
from the single DDC, device pointers."""
import ctypes as C

import numpy as np
import pytest

import ddc_bank_cases as bc
import ddc_cases
import test_gpu_ddc as single
from helpers import make_cfg
from ofdm_uhd_amd import _abi, benchmark_ofdm_rx, config, ddc, engine, iqio, ofdm, options

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
_stream = single._stream


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(cfg=make_cfg())
    yield e
    e.close()


def _check_against_model(y, x, c, R, fc, first, what):
    """The DDC's derived bound: |y - y64| <= (ntaps + 16) 2^-24 sum_k |c[k]| |x[mR - k]| per output."""
    y64, s = ddc_cases.model(x, c, R, ddc_cases.phase_step(fc, R), first)
    assert len(y) == len(y64) == ddc_cases.count(first, len(x), R), what
    err = np.abs(y.astype(np.complex128) - y64)
    bound = (len(c) + 16) * EPS * s
    worst = float(np.max(err / np.maximum(bound, 1e-300))) if len(y) else 0.0
    print("%s: %d outputs, worst error / bound = %.3g" % (what, len(y), worst))
    assert np.all(err <= bound), what


def _singles(eng, R, taps, fcs, raw, first):
    """What the single DDC gives for each frequency on the same handle: (outputs, tables)."""
    ys, cs = [], []
    for fc in fcs:
        eng.set_ddc(ddc.ddc_cfg(R, fc, taps=taps))
        if first:
            eng.ddc_reset(first)
        ys.append(eng.ddc(raw).copy())
        cs.append(eng.ddc_taps())
    eng.set_ddc(None)
    return ys, cs


@pytest.mark.parametrize("fmt", ["fc32", "sc16"])
@pytest.mark.parametrize("R", sorted(bc.TAP_GRID))
def test_every_link_is_the_single_ddc_bit_for_bit(eng, R, fmt):
    rng = np.random.default_rng(4000 + R)
    n = bc.stream_length(R)
    tile = bc.tile_outputs(R, 8) * R
    assert n % tile != 0 and n % (ddc_cases.tile_outputs(R) * R) != 0 and (R == 1 or n % R != 0)
    start = 1000003 if 1000003 % R else 1000004
    assert start % R != 0 or R == 1
    freqs = bc.frequencies(rng, single.FCS)
    eng.set_rx_iq_format(fmt)
    try:
        raw, x = _stream(rng, n, fmt)
        for ntaps in bc.TAP_GRID[R]:
            taps = bc.taps_for(rng, ntaps)
            for first in (0, start):
                want, tabs = _singles(eng, R, taps, freqs, raw, first)
                by_fc = dict(zip(freqs, zip(want, tabs)))
                for K in bc.LINK_COUNTS:
                    fcs = bc.pick(freqs, K)
                    eng.set_ddc_bank(ddc.bank_cfg(R, fcs, taps=taps))
                    if first:
                        eng.ddc_bank_reset(first)
                    assert eng.ddc_bank_count(n) == ddc_cases.count(first, n, R)
                    y = eng.ddc_bank(raw)
                    assert y.shape == (K, ddc_cases.count(first, n, R)) and y.dtype == np.complex64
                    for i, fc in enumerate(fcs):
                        what = "R=%d ntaps=%d K=%d link %d fc=%g first=%d %s" % (R, ntaps, K, i, fc, first, fmt)
                        assert np.array_equal(y[i], by_fc[fc][0]), what
                        assert np.array_equal(eng.ddc_bank_taps(i), by_fc[fc][1]), what
                # one link of the largest bank against the float64 model: the file stands on its own
                i = 2 + (ntaps + (first > 0)) % 5
                _check_against_model(y[i], x, eng.ddc_bank_taps(i), R, freqs[i], first,
                                     "R=%d ntaps=%d K=8 link %d first=%d %s" % (R, ntaps, i, first, fmt))
    finally:
        eng.set_rx_iq_format("fc32")
        eng.set_ddc_bank(None)
        eng.set_ddc(None)


SEG_SHAPES = [(1, 31, 2), (2, 1024, 8), (3, 155, 3), (4, 31, 4), (8, 155, 4), (64, 1024, 8), (64, 63, 2), (17, 1, 3)]


@pytest.mark.parametrize("fmt", ["fc32", "sc16"])
@pytest.mark.parametrize("R,ntaps,K", SEG_SHAPES)
def test_any_segmentation_gives_the_same_bits(eng, R, ntaps, K, fmt):
    rng = np.random.default_rng(91 * R + ntaps + K)
    tile = bc.tile_outputs(R, K) * R
    n = 3 * tile + 1234 + 2 * ntaps
    fcs = [float(f) for f in rng.uniform(-0.5, 0.5, K)]
    fcs[0] = -1.0 / 3.0 + 0.013
    eng.set_rx_iq_format(fmt)
    try:
        raw, x = _stream(rng, n, fmt)
        taps = bc.taps_for(rng, ntaps)
        eng.set_ddc_bank(ddc.bank_cfg(R, fcs, taps=taps))
        whole = eng.ddc_bank(raw).copy()
        assert whole.shape == (K, ddc_cases.count(0, n, R))
        _check_against_model(whole[K - 1], x, eng.ddc_bank_taps(K - 1), R, fcs[K - 1], 0, "whole R=%d ntaps=%d K=%d %s" % (R, ntaps, K, fmt))
        eng.ddc_bank_reset(0)
        sizes = single._chunk_sizes(rng, n, R, ntaps)     # 1, R-1, R, ntaps-2, ntaps, 997, tile-1, tile+1, then draws
        assert any(s < ntaps - 1 for s in sizes) or ntaps <= 2
        parts, a, empty = [], 0, 0
        for s in sizes:
            want = ddc_cases.count(a, s, R)
            assert eng.ddc_bank_count(s) == want
            y = eng.ddc_bank(raw[a:a + s])
            assert y.shape == (K, want)
            empty += want == 0
            parts.append(y.copy())
            a += s
        assert empty >= 1 or R == 1                       # calls that produce nothing are part of the stream
        assert np.array_equal(np.concatenate(parts, axis=1), whole)
        # ... and from a start that is no multiple of R
        first = 7 * R + 1
        eng.ddc_bank_reset(first)
        w2 = eng.ddc_bank(raw).copy()
        eng.ddc_bank_reset(first)
        p2 = [eng.ddc_bank(raw[i:i + 997]).copy() for i in range(0, n, 997)]
        assert np.array_equal(np.concatenate(p2, axis=1), w2)
    finally:
        eng.set_rx_iq_format("fc32")
        eng.set_ddc_bank(None)


@pytest.mark.parametrize("R,ntaps", [(4, 31), (8, 155), (64, 63)])
def test_link_order_and_count_do_not_matter(eng, R, ntaps):
    rng = np.random.default_rng(17 + R)
    n = bc.tile_outputs(R, 8) * R + 1001
    raw, _ = _stream(rng, n, "fc32")
    taps = bc.taps_for(rng, ntaps)
    fcs = [float(f) for f in rng.uniform(-0.5, 0.5, 7)]
    try:
        eng.set_ddc_bank(ddc.bank_cfg(R, fcs, taps=taps))
        ref = eng.ddc_bank(raw).copy()
        perm = [int(i) for i in rng.permutation(7)]
        assert perm != list(range(7))
        eng.set_ddc_bank(ddc.bank_cfg(R, [fcs[i] for i in perm], taps=taps))
        y = eng.ddc_bank(raw)
        for j, i in enumerate(perm):
            assert np.array_equal(y[j], ref[i]), (j, i)
        for i in (0, 3, 6):                               # first of a group, last of a group, the odd one out
            eng.set_ddc_bank(ddc.bank_cfg(R, [fcs[i]], taps=taps))
            assert np.array_equal(eng.ddc_bank(raw)[0], ref[i]), i
        # equal frequencies give equal outputs
        eng.set_ddc_bank(ddc.bank_cfg(R, [fcs[1]] * 5, taps=taps))
        y = eng.ddc_bank(raw)
        for j in range(5):
            assert np.array_equal(y[j], ref[1])
    finally:
        eng.set_ddc_bank(None)


def _options(cap):
    return options.default_options(modulation=cap["mod"], fft_length=cap["N"], occupied_tones=cap["occ"], cp_length=cap["CP"])


@pytest.mark.parametrize("name,fmt", [("qpsk512_r4", "fc32"), ("qpsk512_r4", "sc16"), ("qam16_2048_r2", "fc32"),
                                      ("bpsk64_r8", "fc32"), ("qpsk512_r3", "fc32")])
def test_two_links_end_to_end(orc, name, fmt):
    cap = ddc_cases.capture(name)
    R, cfg, freqs = cap["R"], cap["cfg"], list(cap["freqs"])
    wide = single._wide_sc16(cap["wide"]) if fmt == "sc16" else cap["wide"]
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
    # a list of option sets, one per link: the second link demodulated as BPSK finds no good packet
    o_ok, o_other = _options(cap), _options(cap)
    o_other.modulation = "bpsk"
    bank = ofdm.ofdm_demod_bank([o_ok, o_other], cap["freqs"], 4, taps=cap["taps"])
    try:
        out = bank.work(cap["wide"])
        assert [p for ok, p in out[0] if ok] == cap["payloads"][0] and not any(ok for ok, _ in out[1])
    finally:
        bank.close()
    f = str(tmp_path / "wide.dat")
    sink = iqio.file_sink(f)
    sink.write(cap["wide"])
    sink.close()
    to = str(tmp_path / "rx.txt")
    for extra in ([], ["--chunk-samples", "5000"]):
        accts = benchmark_ofdm_rx.main(["-m", "qpsk", "--from-file", f, "--to-file", to, "--ddc-decim", "4",
                                        "--ddc-freqs", "0.25,-0.25"] + extra)
        assert [(a.n_rcvd, a.n_right) for a in accts] == [(4, 4), (4, 4)]
        assert (tmp_path / "rx.txt.link0").exists() and (tmp_path / "rx.txt.link1").exists()
    with pytest.raises(SystemExit):
        benchmark_ofdm_rx.main(["-m", "qpsk", "--from-file", f, "--to-file", to, "--ddc-decim", "4", "--ddc-freq", "0.25",
                                "--ddc-freqs", "0.25,-0.25"])
    # without the new flag: one account, as before
    acct = benchmark_ofdm_rx.main(["-m", "qpsk", "--from-file", f, "--to-file", to, "--ddc-decim", "4", "--ddc-freq", "-0.25"])
    assert (acct.n_rcvd, acct.n_right) == (4, 4)


def _raw_bank(lib, h, x, out, stride, cap, n=None):
    nn = C.c_uint64(0)
    rc = lib.ofdm_ddc_bank(h, x.ctypes.data_as(C.c_void_p), len(x) if n is None else n, out.ctypes.data_as(C.c_void_p),
                           stride, cap, C.byref(nn))
    return rc, nn.value


def test_layout_and_capacity(eng):
    lib = _abi.load()
    rng = np.random.default_rng(5)
    raw, _ = _stream(rng, 5000, "fc32")
    fcs = [0.2, -0.1, 0.37]
    eng.set_ddc_bank(ddc.bank_cfg(3, fcs, taps=ddc.design(3, 0.4)))
    try:
        want = eng.ddc_bank(raw).copy()
        no = want.shape[1]
        # link_stride > nout: the gaps keep what they held
        eng.ddc_bank_reset(0)
        sentinel = np.complex64(-7.5 + 3.25j)
        out = np.full((3, no + 13), sentinel, np.complex64)
        assert _raw_bank(lib, eng._h, raw, out, no + 13, no) == (_abi.OFDM_OK, no)
        assert np.array_equal(out[:, :no], want) and np.all(out[:, no:] == sentinel)
        # out_cap one short: refused with *nout set, and the stream does not move
        eng.ddc_bank_reset(0)
        first = eng.ddc_bank(raw[:1001]).copy()
        need = eng.ddc_bank_count(3999)
        out = np.full((3, need), sentinel, np.complex64)
        rest_in = np.ascontiguousarray(raw[1001:])
        assert _raw_bank(lib, eng._h, rest_in, out, need, need - 1) == (_abi.OFDM_E_CAPACITY, need)
        assert np.all(out == sentinel) and eng.ddc_bank_count(3999) == need
        # link_stride < nout with more than one link
        assert _raw_bank(lib, eng._h, rest_in, out, need - 1, need) == (_abi.OFDM_E_INVAL, need)
        assert eng.ddc_bank_count(3999) == need
        rest = eng.ddc_bank(rest_in)
        assert np.array_equal(np.concatenate([first, rest], axis=1), want)
        # one link: the stride does not matter
        eng.set_ddc_bank(ddc.bank_cfg(3, fcs[1:2], taps=ddc.design(3, 0.4)))
        out = np.zeros(no, np.complex64)
        assert _raw_bank(lib, eng._h, raw, out, 0, no) == (_abi.OFDM_OK, no)
        assert np.array_equal(out, want[1])
    finally:
        eng.set_ddc_bank(None)


def _raw_cfg(**kw):
    c = ddc.bank_cfg(4, [0.25, -0.1], taps=np.ones(5, np.float32))
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_invalid_arguments_are_refused(eng):
    lib = _abi.load()
    eng.set_ddc_bank(None)
    x = np.zeros(64, np.complex64)
    out = np.zeros((2, 64), np.complex64)
    k = C.c_int(0)
    assert _raw_bank(lib, eng._h, x, out, 64, 64)[0] == _abi.OFDM_E_INVAL          # no configuration
    for call in (lambda: eng.ddc_bank(x), lambda: eng.ddc_bank_reset(0), lambda: eng.ddc_bank_count(4),
                 lambda: eng.ddc_bank_taps(0), lambda: eng.ddc_bank_last_ms()):
        with pytest.raises(ValueError):
            call()
    good = _raw_cfg()
    eng.set_ddc_bank(good)
    table = eng.ddc_bank_taps(1)
    assert _raw_bank(lib, eng._h, x, out, 64, 64) == (_abi.OFDM_OK, 16)
    y = out[:, :16].copy()
    bad_fc = []
    for v in (0.5000001, -0.51, float("nan")):
        c = _raw_cfg()
        c.center_freq[1] = v
        bad_fc.append(c)
    bad_tap = []
    for v in (float("nan"), float("inf")):
        c = _raw_cfg()
        c.taps[3] = v
        bad_tap.append(c)
    refused = [_raw_cfg(**b) for b in (dict(struct_size=12), dict(decimation=0), dict(decimation=65), dict(ntaps=0),
                                       dict(ntaps=1025), dict(nlinks=0), dict(nlinks=9))] + bad_fc + bad_tap
    for c in refused:
        with pytest.raises(ValueError):
            eng.set_ddc_bank(c)
        assert eng.ddc_bank_cfg is good
    # a frequency beyond nlinks is not looked at
    c = _raw_cfg()
    c.center_freq[2] = 3.0
    eng.set_ddc_bank(c)
    eng.set_ddc_bank(good)
    for c in refused[:3]:
        with pytest.raises(ValueError):
            eng.set_ddc_bank(c)
    # ... a refused configuration left the one in force untouched: same table, same stream position, same outputs
    assert np.array_equal(eng.ddc_bank_taps(1), table)
    eng.ddc_bank(x[:62])
    with pytest.raises(ValueError):
        eng.set_ddc_bank(refused[5])
    assert eng.ddc_bank_count(2) == 0 and eng.ddc_bank_count(3) == 1                # still 62 samples into the stream
    eng.ddc_bank_reset(0)
    assert np.array_equal(eng.ddc_bank(x), y)
    # link >= nlinks
    for link in (2, 8, -1):
        assert lib.ofdm_ddc_bank_taps(eng._h, link, None, 0, C.byref(k)) == _abi.OFDM_E_INVAL
    assert lib.ofdm_ddc_bank_taps(eng._h, 1, None, 0, C.byref(k)) == _abi.OFDM_OK and k.value == 5
    # the ends of the frequency range are inside it
    eng.set_ddc_bank(ddc.bank_cfg(4, [0.5, -0.5], taps=np.ones(5, np.float32)))
    # a 16-bit pointer that is not 4-byte aligned
    eng.set_rx_iq_format("sc16")
    try:
        q = np.zeros(2 * 64 + 2, np.int16)
        nn = C.c_uint64(0)
        rc = lib.ofdm_ddc_bank(eng._h, C.c_void_p(q.ctypes.data + 2), 64, out.ctypes.data_as(C.c_void_p), 64, 64, C.byref(nn))
        assert rc == _abi.OFDM_E_INVAL
        assert eng.ddc_bank_count(64) == 16               # ... and the stream did not move
    finally:
        eng.set_rx_iq_format("fc32")
        eng.set_ddc_bank(None)
    assert _raw_bank(lib, eng._h, x, out, 64, 64)[0] == _abi.OFDM_E_INVAL          # ... and after it was dropped


def test_phase_step_and_index_limits(eng):
    """As the DDC's test of the same name: fc R a hair below a whole turn gives phase step 0; stream indices are refused
    before 64-bit arithmetic could wrap."""
    rng = np.random.default_rng(9)
    raw, x = _stream(rng, 700, "fc32")
    taps = (rng.standard_normal(9) / 3).astype(np.float32)
    try:
        eng.set_ddc_bank(ddc.bank_cfg(4, [0.3, -1e-20], taps=taps))
        assert ddc_cases.phase_step(-1e-20, 4) == 0
        eng.ddc_bank_reset(1000003)
        _check_against_model(eng.ddc_bank(raw)[1], x, eng.ddc_bank_taps(1), 4, -1e-20, 1000003, "fc=-1e-20")
        eng.ddc_bank_reset(1 << 62)
        assert eng.ddc_bank_count(8) == 2
        with pytest.raises(ValueError):
            eng.ddc_bank_reset((1 << 62) + 1)
        assert eng.ddc_bank_count(8) == 2                 # the refused reset left the stream where it was
    finally:
        eng.set_ddc_bank(None)


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
    """Two handles demodulate the same narrowband stream: one never saw the bank, the other used it on another stream
    and dropped it.  Same packets, same per-kernel launch counts; the kernel table has no entry for the bank."""
    cap = ddc_cases.capture("qpsk512_r4")
    cfg = cap["cfg"]
    a, b = engine.Engine(cfg=cfg), engine.Engine(cfg=cfg)
    try:
        b.set_ddc_bank(ddc.bank_cfg(4, cap["freqs"], taps=cap["taps"]))
        y = b.ddc_bank(cap["wide"])[0].copy()
        b.set_ddc_bank(None)
        for e in (a, b):
            e.prof_enable(True)
            e.prof_reset()
        pa, pb = a.rx(y), b.rx(y)
        assert pa == pb and len(pa) == 4
        ca = {k: v[1] for k, v in a.prof().items()}
        cb = {k: v[1] for k, v in b.prof().items()}
        assert ca == cb and sum(ca.values()) > 0
        assert len(ca) == _abi.K_COUNT == 11 and not any("ddc" in k for k in ca)
        # with a bank configured the receiver's own launches stay what they are, and the bank reports its time
        b.set_ddc_bank(ddc.bank_cfg(4, cap["freqs"], taps=cap["taps"]))
        b.prof_reset()
        with pytest.raises(ValueError):
            b.ddc_bank_last_ms()                          # no profiled call yet
        y2 = b.ddc_bank(cap["wide"])
        assert np.array_equal(y2[0], y) and b.ddc_bank_last_ms() > 0.0
        assert b.rx(y2[0]) == pa
        assert {k: v[1] for k, v in b.prof().items()} == ca
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("fmt", ["fc32", "sc16"])
def test_device_pointers(fmt):
    """Driven as tools/bench_ddc.py drives ddc_device: torch buffers, raw pointers."""
    import torch
    dev = torch.device("cuda", 0)
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
        for e in (host, devE):
            e.set_rx_iq_format(fmt)
            e.set_ddc_bank(ddc.bank_cfg(R, fcs, taps=taps))
            e.prof_enable(True)
        want = host.ddc_bank(raw)
        no = want.shape[1]
        stride = no + 3
        x = torch.from_numpy(np.ascontiguousarray(raw)).to(dev)
        y = torch.full((K, stride), -2.0 + 1.0j, dtype=torch.complex64, device=dev)
        got = devE.ddc_bank_device(x.data_ptr(), n, y.data_ptr(), stride, no)
        torch.cuda.synchronize()
        assert got == no
        out = y.cpu().numpy()
        assert np.array_equal(out[:, :no], want) and np.all(out[:, no:] == np.complex64(-2.0 + 1.0j))
        assert devE.ddc_bank_last_ms() > 0.0
        # two halves through device pointers continue the stream
        devE.ddc_bank_reset(0)
        h1 = n // 2 + 1
        n1 = devE.ddc_bank_device(x.data_ptr(), h1, y.data_ptr(), stride, stride)
        off = h1 * (4 if fmt == "sc16" else 8)            # bytes per wideband sample
        n2 = devE.ddc_bank_device(x.data_ptr() + off, n - h1, y.data_ptr() + 8 * n1, stride, stride - n1)
        torch.cuda.synchronize()
        assert n1 + n2 == no and np.array_equal(y.cpu().numpy()[:, :no], want)
    finally:
        host.close()
        devE.close()
