"""The resampler bank on the GPU (k_resamp_bank, Engine.resamp_bank, ofdm_demod_resamp_bank): every link bit for bit the
single resampler, under any segmentation, link order and link count; end to end on the two-link wideband captures;
layout, errors, independence from the other front ends, device pointers."""
import ctypes as C

import numpy as np
import pytest

import resamp_bank_cases as bc
import resamp_cases
import test_gpu_resamp as single
from helpers import make_cfg
from ofdm_uhd_amd import _abi, benchmark_ofdm_rx, config, ddc, engine, iqio, ofdm, options, resample

pytestmark = pytest.mark.gpu

_stream = single._stream
_check_against_model = single._check_against_model   # (ceil(ntaps / L) + 16) 2^-24 sum |c| |x| per output, DESIGN.md section 7


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(cfg=make_cfg())
    yield e
    e.close()


def _singles(eng, L, M, taps, fcs, raw, first):
    """What the single resampler gives for each frequency on the same handle: (outputs, tables)."""
    ys, cs = [], []
    for fc in fcs:
        eng.set_resamp(resample.resamp_cfg(L, M, fc, taps=taps))
        if first:
            eng.resamp_reset(first)
        ys.append(eng.resamp(raw).copy())
        cs.append(eng.resamp_taps())
    eng.set_resamp(None)
    return ys, cs


@pytest.mark.parametrize("fmt", ["fc32", "sc16"])
@pytest.mark.parametrize("L,M", sorted(bc.TAP_GRID))
def test_every_link_is_the_single_resampler_bit_for_bit(eng, L, M, fmt):
    rng = np.random.default_rng(5000 + 64 * L + M)
    n = bc.stream_length(L, M)
    tile = bc.tile_inputs(L, M, 8)
    assert n % tile != 0 and (M == 1 or n % M != 0)
    start = bc.far_start(M)
    freqs = bc.frequencies(rng, single.FCS)
    assert 0.5 in freqs and 0.0 in freqs
    eng.set_rx_iq_format(fmt)
    try:
        raw, x = _stream(rng, n, fmt)
        for ntaps in bc.TAP_GRID[(L, M)]:
            taps = bc.taps_for(rng, ntaps)
            for first in (0, start):
                no = resamp_cases.count(first, n, L, M)
                want, tabs = _singles(eng, L, M, taps, freqs, raw, first)
                by_fc = dict(zip(freqs, zip(want, tabs)))
                for K in bc.LINK_COUNTS:
                    fcs = bc.pick(freqs, K)
                    eng.set_resamp_bank(resample.bank_cfg(L, M, fcs, taps=taps))
                    if first:
                        eng.resamp_bank_reset(first)
                    assert eng.resamp_bank_count(n) == no
                    y = eng.resamp_bank(raw)
                    assert y.shape == (K, no) and y.dtype == np.complex64
                    for i, fc in enumerate(fcs):
                        what = "L/M=%d/%d ntaps=%d K=%d link %d fc=%g first=%d %s" % (L, M, ntaps, K, i, fc, first, fmt)
                        assert np.array_equal(y[i], by_fc[fc][0]), what
                        assert np.array_equal(eng.resamp_bank_taps(i), by_fc[fc][1]), what
                # one link of the largest bank against the float64 model: the file stands on its own
                i = 2 + (ntaps + (first > 0)) % 5
                _check_against_model(y[i], x, eng.resamp_bank_taps(i), L, M, freqs[i], first,
                                     "L/M=%d/%d ntaps=%d K=8 link %d first=%d %s" % (L, M, ntaps, i, first, fmt))
    finally:
        eng.set_rx_iq_format("fc32")
        eng.set_resamp_bank(None)
        eng.set_resamp(None)


@pytest.mark.parametrize("fmt", ["fc32", "sc16"])
@pytest.mark.parametrize("L,M,ntaps,K", bc.SEG_SHAPES)
def test_any_segmentation_gives_the_same_bits(eng, L, M, ntaps, K, fmt):
    rng = np.random.default_rng(77 * L + 5 * M + ntaps + K)
    tile = bc.tile_inputs(L, M, K)
    n = 3 * tile + 1234 + 2 * ((ntaps - 1) // L)
    fcs = [float(f) for f in rng.uniform(-0.5, 0.5, K)]
    fcs[0] = -1.0 / 3.0 + 0.013
    eng.set_rx_iq_format(fmt)
    try:
        raw, x = _stream(rng, n, fmt)
        taps = bc.taps_for(rng, ntaps)
        eng.set_resamp_bank(resample.bank_cfg(L, M, fcs, taps=taps))
        whole = eng.resamp_bank(raw).copy()
        assert whole.shape == (K, resamp_cases.count(0, n, L, M))
        _check_against_model(whole[K - 1], x, eng.resamp_bank_taps(K - 1), L, M, fcs[K - 1], 0,
                             "whole L/M=%d/%d ntaps=%d K=%d %s" % (L, M, ntaps, K, fmt))
        eng.resamp_bank_reset(0)
        sizes = single._chunk_sizes(rng, n, L, M, ntaps)   # 1, M-1, M, Q-1, Q+1, 997, tile-1, tile+1, then draws
        if M > L:
            # one call that produces nothing for certain: cut the first longer chunk where a single sample completes no
            # output (between two outputs the input index advances by M / L > 1)
            k = next(i for i, s in enumerate(sizes) if s > 2 * M)
            at = sum(sizes[:k])
            lone = next(j for j in range(1, M + 1) if resamp_cases.count(at + j, 1, L, M) == 0)
            sizes[k:k + 1] = [lone, 1, sizes[k] - lone - 1]
        assert sum(sizes) == n and min(sizes) >= 1
        parts, a, empty = [], 0, 0
        for s in sizes:
            want = resamp_cases.count(a, s, L, M)
            assert eng.resamp_bank_count(s) == want
            y = eng.resamp_bank(raw[a:a + s])
            assert y.shape == (K, want)
            empty += want == 0
            parts.append(y.copy())
            a += s
        assert empty >= 1 or M <= L                        # calls that produce nothing are part of the stream
        assert np.array_equal(np.concatenate(parts, axis=1), whole)
        # ... and from a start that is no multiple of M
        first = 7 * M + 1
        eng.resamp_bank_reset(first)
        w2 = eng.resamp_bank(raw).copy()
        assert w2.shape == (K, resamp_cases.count(first, n, L, M))
        eng.resamp_bank_reset(first)
        p2 = [eng.resamp_bank(raw[i:i + 997]).copy() for i in range(0, n, 997)]
        assert np.array_equal(np.concatenate(p2, axis=1), w2)
    finally:
        eng.set_rx_iq_format("fc32")
        eng.set_resamp_bank(None)


@pytest.mark.parametrize("L,M,ntaps", [(2, 5, 39), (8, 25, 481), (3, 25, 155), (64, 64, 1024)])
def test_link_order_and_count_do_not_matter(eng, L, M, ntaps):
    rng = np.random.default_rng(17 + 64 * L + M)
    n = bc.tile_inputs(L, M, 8) + 1001
    raw, _ = _stream(rng, n, "fc32")
    taps = bc.taps_for(rng, ntaps)
    fcs = [float(f) for f in rng.uniform(-0.5, 0.5, 7)]
    try:
        eng.set_resamp_bank(resample.bank_cfg(L, M, fcs, taps=taps))
        ref = eng.resamp_bank(raw).copy()
        perm = [int(i) for i in rng.permutation(7)]
        assert perm != list(range(7))
        eng.set_resamp_bank(resample.bank_cfg(L, M, [fcs[i] for i in perm], taps=taps))
        y = eng.resamp_bank(raw)
        for j, i in enumerate(perm):
            assert np.array_equal(y[j], ref[i]), (j, i)
        for i in (0, 3, 6):                                # first of a group, last of a group, the odd one out
            eng.set_resamp_bank(resample.bank_cfg(L, M, [fcs[i]], taps=taps))
            assert np.array_equal(eng.resamp_bank(raw)[0], ref[i]), i
        # equal frequencies give equal outputs
        eng.set_resamp_bank(resample.bank_cfg(L, M, [fcs[1]] * 5, taps=taps))
        y = eng.resamp_bank(raw)
        for j in range(5):
            assert np.array_equal(y[j], ref[1])
    finally:
        eng.set_resamp_bank(None)


def _options(cap):
    return options.default_options(modulation=cap["mod"], fft_length=cap["N"], occupied_tones=cap["occ"], cp_length=cap["CP"])


@pytest.mark.parametrize("name,fmt", [("qpsk512_2_5", "fc32"), ("qpsk512_2_5", "sc16"), ("bpsk64_8_25", "fc32")])
def test_two_links_end_to_end(orc, name, fmt):
    cap = resamp_cases.capture(name)
    L, M, cfg, freqs = cap["L"], cap["M"], cap["cfg"], list(cap["freqs"])
    wide = single._wide_sc16(cap["wide"]) if fmt == "sc16" else cap["wide"]
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
    freqs = list(cap["freqs"])
    # a list of option sets, one per link: the second link demodulated as BPSK finds no good packet
    o_ok, o_other = _options(cap), _options(cap)
    o_other.modulation = "bpsk"
    bank = ofdm.ofdm_demod_resamp_bank([o_ok, o_other], freqs, 2, 5, taps=cap["taps"])
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
    base = ["-m", "qpsk", "--from-file", f, "--to-file", to, "--resamp-interp", "2", "--resamp-decim", "5"]
    for extra in ([], ["--chunk-samples", "5000"]):
        accts = benchmark_ofdm_rx.main(base + ["--resamp-freqs", "0.22,-0.21"] + extra)
        assert [(a.n_rcvd, a.n_right) for a in accts] == [(4, 4), (4, 4)]
        assert (tmp_path / "rx.txt.link0").exists() and (tmp_path / "rx.txt.link1").exists()
    with pytest.raises(SystemExit):
        benchmark_ofdm_rx.main(base + ["--resamp-freq", "0.22", "--resamp-freqs", "0.22,-0.21"])
    # without the new flag: one account, as before
    acct = benchmark_ofdm_rx.main(base + ["--resamp-freq", "-0.21"])
    assert (acct.n_rcvd, acct.n_right) == (4, 4)


def _raw_bank(lib, h, x, out, stride, cap, n=None):
    nn = C.c_uint64(0)
    rc = lib.ofdm_resamp_bank(h, x.ctypes.data_as(C.c_void_p), len(x) if n is None else n, out.ctypes.data_as(C.c_void_p),
                              stride, cap, C.byref(nn))
    return rc, nn.value


def test_layout_and_capacity(eng):
    lib = _abi.load()
    rng = np.random.default_rng(5)
    raw, _ = _stream(rng, 5000, "fc32")
    fcs = [0.2, -0.1, 0.37]
    taps = resample.design(2, 5, 0.4)
    eng.set_resamp_bank(resample.bank_cfg(2, 5, fcs, taps=taps))
    try:
        want = eng.resamp_bank(raw).copy()
        no = want.shape[1]
        assert no == resamp_cases.count(0, 5000, 2, 5)
        # link_stride > nout: the gaps keep what they held
        eng.resamp_bank_reset(0)
        sentinel = np.complex64(-7.5 + 3.25j)
        out = np.full((3, no + 13), sentinel, np.complex64)
        assert _raw_bank(lib, eng._h, raw, out, no + 13, no) == (_abi.OFDM_OK, no)
        assert np.array_equal(out[:, :no], want) and np.all(out[:, no:] == sentinel)
        # out_cap one short: refused with *nout set, and the stream does not move
        eng.resamp_bank_reset(0)
        first = eng.resamp_bank(raw[:1001]).copy()
        need = eng.resamp_bank_count(3999)
        out = np.full((3, need), sentinel, np.complex64)
        rest_in = np.ascontiguousarray(raw[1001:])
        assert _raw_bank(lib, eng._h, rest_in, out, need, need - 1) == (_abi.OFDM_E_CAPACITY, need)
        assert np.all(out == sentinel) and eng.resamp_bank_count(3999) == need
        # link_stride < nout with more than one link
        assert _raw_bank(lib, eng._h, rest_in, out, need - 1, need) == (_abi.OFDM_E_INVAL, need)
        assert eng.resamp_bank_count(3999) == need
        # the retried call gives the bits of an uninterrupted run
        rest = eng.resamp_bank(rest_in)
        assert np.array_equal(np.concatenate([first, rest], axis=1), want)
        # one link: the stride does not matter
        eng.set_resamp_bank(resample.bank_cfg(2, 5, fcs[1:2], taps=taps))
        out = np.zeros(no, np.complex64)
        assert _raw_bank(lib, eng._h, raw, out, 0, no) == (_abi.OFDM_OK, no)
        assert np.array_equal(out, want[1])
    finally:
        eng.set_resamp_bank(None)


def _raw_cfg(**kw):
    c = resample.bank_cfg(2, 5, [0.25, -0.1], taps=np.ones(5, np.float32))
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_invalid_arguments_are_refused(eng):
    """Every refusal is made on the host, before any launch: the buffers handed over are valid throughout."""
    lib = _abi.load()
    eng.set_resamp_bank(None)
    x = np.zeros(64, np.complex64)
    x[::3] = 1.0
    out = np.zeros((2, 64), np.complex64)
    k = C.c_int(0)
    no = resamp_cases.count(0, 64, 2, 5)
    assert _raw_bank(lib, eng._h, x, out, 64, 64)[0] == _abi.OFDM_E_INVAL          # no configuration
    for call in (lambda: eng.resamp_bank(x), lambda: eng.resamp_bank_reset(0), lambda: eng.resamp_bank_count(4),
                 lambda: eng.resamp_bank_taps(0), lambda: eng.resamp_bank_last_ms()):
        with pytest.raises(ValueError):
            call()
    good = _raw_cfg()
    eng.set_resamp_bank(good)
    table = eng.resamp_bank_taps(1)
    assert _raw_bank(lib, eng._h, x, out, 64, 64) == (_abi.OFDM_OK, no)
    y = out[:, :no].copy()
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
    refused = [_raw_cfg(**b) for b in (dict(struct_size=12), dict(interpolation=0), dict(interpolation=65), dict(decimation=0),
                                       dict(decimation=65), dict(ntaps=0), dict(ntaps=1025), dict(nlinks=0),
                                       dict(nlinks=9))] + bad_fc + bad_tap
    for c in refused:
        with pytest.raises(ValueError):
            eng.set_resamp_bank(c)
        assert eng.resamp_bank_cfg is good
    # a frequency beyond nlinks is not looked at
    c = _raw_cfg()
    c.center_freq[2] = 3.0
    eng.set_resamp_bank(c)
    eng.set_resamp_bank(good)
    # ... a refused configuration left the one in force untouched: same table, same stream position, same outputs
    assert np.array_equal(eng.resamp_bank_taps(1), table)
    eng.resamp_bank(x[:62])
    with pytest.raises(ValueError):
        eng.set_resamp_bank(refused[7])
    assert eng.resamp_bank_count(2) == resamp_cases.count(62, 2, 2, 5)              # still 62 samples into the stream
    assert eng.resamp_bank_count(3) == resamp_cases.count(62, 3, 2, 5) == 1
    eng.resamp_bank_reset(0)
    assert np.array_equal(eng.resamp_bank(x), y)
    # link >= nlinks
    for link in (2, 8, -1):
        assert lib.ofdm_resamp_bank_taps(eng._h, link, None, 0, C.byref(k)) == _abi.OFDM_E_INVAL
    assert lib.ofdm_resamp_bank_taps(eng._h, 1, None, 0, C.byref(k)) == _abi.OFDM_OK and k.value == 5
    # the index limit is the resampler's
    eng.resamp_bank_reset(1 << 56)
    with pytest.raises(ValueError):
        eng.resamp_bank_reset((1 << 56) + 1)
    assert _raw_bank(lib, eng._h, x, out, 64, 64)[0] == _abi.OFDM_E_INVAL          # the index would pass 2^56
    eng.resamp_bank_reset(0)
    # null pointers
    nn = C.c_uint64(0)
    assert lib.ofdm_resamp_bank(eng._h, None, 64, out.ctypes.data_as(C.c_void_p), 64, 64, C.byref(nn)) == _abi.OFDM_E_INVAL
    assert lib.ofdm_resamp_bank(eng._h, x.ctypes.data_as(C.c_void_p), 64, None, 64, 64, C.byref(nn)) == _abi.OFDM_E_INVAL
    assert lib.ofdm_resamp_bank(eng._h, x.ctypes.data_as(C.c_void_p), 64, out.ctypes.data_as(C.c_void_p), 64, 64, None) == _abi.OFDM_E_INVAL
    assert eng.resamp_bank_count(64) == no                 # ... and the stream did not move
    # the ends of the frequency range are inside it
    eng.set_resamp_bank(resample.bank_cfg(2, 5, [0.5, -0.5], taps=np.ones(5, np.float32)))
    # a 16-bit pointer that is not 4-byte aligned
    eng.set_rx_iq_format("sc16")
    try:
        q = np.zeros(2 * 64 + 2, np.int16)
        rc = lib.ofdm_resamp_bank(eng._h, C.c_void_p(q.ctypes.data + 2), 64, out.ctypes.data_as(C.c_void_p), 64, 64, C.byref(nn))
        assert rc == _abi.OFDM_E_INVAL
        assert eng.resamp_bank_count(64) == no             # ... and the stream did not move
    finally:
        eng.set_rx_iq_format("fc32")
        eng.set_resamp_bank(None)
    assert _raw_bank(lib, eng._h, x, out, 64, 64)[0] == _abi.OFDM_E_INVAL          # ... and after it was dropped


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
    try:
        alone = {}
        for name, mk in cfgs.items():
            getattr(eng, "set_" + name)(mk())
            alone[name] = getattr(eng, name)(raw).copy()
            getattr(eng, "set_" + name)(None)
        for name, mk in cfgs.items():
            getattr(eng, "set_" + name)(mk())
        parts = {name: [] for name in cfgs}
        at = {name: 0 for name in cfgs}
        while any(a < n for a in at.values()):
            for name in cfgs:
                if at[name] < n:
                    parts[name].append(getattr(eng, name)(raw[at[name]:at[name] + steps[name]]).copy())
                    at[name] += steps[name]
        for name in cfgs:
            assert np.array_equal(np.concatenate(parts[name], axis=-1), alone[name]), name
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
    """Two handles demodulate the same narrowband stream: one never saw the bank, the other used it on another stream
    and dropped it.  Same packets, same per-kernel launch counts; the kernel table has no entry for the bank."""
    cap = resamp_cases.capture("qpsk512_2_5")
    cfg = cap["cfg"]
    a, b = engine.Engine(cfg=cfg), engine.Engine(cfg=cfg)
    try:
        b.set_resamp_bank(resample.bank_cfg(2, 5, cap["freqs"], taps=cap["taps"]))
        y = b.resamp_bank(cap["wide"])[0].copy()
        b.set_resamp_bank(None)
        for e in (a, b):
            e.prof_enable(True)
            e.prof_reset()
        pa, pb = a.rx(y), b.rx(y)
        assert pa == pb and len(pa) == 4
        ca = {k: v[1] for k, v in a.prof().items()}
        cb = {k: v[1] for k, v in b.prof().items()}
        assert ca == cb and sum(ca.values()) > 0
        assert len(ca) == _abi.K_COUNT == 11 and not any("resamp" in k for k in ca)
        # with a bank configured the receiver's own launches stay what they are, and the bank reports its time
        b.set_resamp_bank(resample.bank_cfg(2, 5, cap["freqs"], taps=cap["taps"]))
        b.prof_reset()
        with pytest.raises(ValueError):
            b.resamp_bank_last_ms()                        # no profiled call yet
        y2 = b.resamp_bank(cap["wide"])
        assert np.array_equal(y2[0], y) and b.resamp_bank_last_ms() > 0.0
        assert b.rx(y2[0]) == pa
        assert {k: v[1] for k, v in b.prof().items()} == ca
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("fmt", ["fc32", "sc16"])
def test_device_pointers(fmt):
    """Driven as tools/bench_resamp_bank.py drives resamp_bank_device: torch buffers, raw pointers; a row goes straight
    into rx_device."""
    import torch
    dev = torch.device("cuda", 0)
    cap = resamp_cases.capture("qpsk512_2_5")
    L, M, K = 2, 5, 5
    wide = single._wide_sc16(cap["wide"]) if fmt == "sc16" else cap["wide"]
    n = len(wide)
    fcs = list(cap["freqs"]) + [0.4, -0.45, 0.01]
    host = engine.Engine(cfg=cap["cfg"])
    devE = engine.Engine(cfg=config.make_cfg(_options(cap), device_ptrs=True))
    x = y = pay = None
    try:
        for e in (host, devE):
            e.set_rx_iq_format(fmt)
            e.set_resamp_bank(resample.bank_cfg(L, M, fcs, taps=cap["taps"]))
            e.prof_enable(True)
        want = host.resamp_bank(wide)
        no = want.shape[1]
        stride = no + 3
        x = torch.from_numpy(np.array(wide)).to(dev)           # (a writable copy: the capture is read-only)
        y = torch.full((K, stride), -2.0 + 1.0j, dtype=torch.complex64, device=dev)
        got = devE.resamp_bank_device(x.data_ptr(), n, y.data_ptr(), stride, no)
        torch.cuda.synchronize()
        assert got == no
        out = y.cpu().numpy()
        assert np.array_equal(out[:, :no], want) and np.all(out[:, no:] == np.complex64(-2.0 + 1.0j))
        assert devE.resamp_bank_last_ms() > 0.0
        # two halves through device pointers continue the stream
        devE.resamp_bank_reset(0)
        y.fill_(0)
        h1 = n // 2 + 1
        n1 = devE.resamp_bank_device(x.data_ptr(), h1, y.data_ptr(), stride, stride)
        off = h1 * (4 if fmt == "sc16" else 8)             # bytes per wideband sample
        n2 = devE.resamp_bank_device(x.data_ptr() + off, n - h1, y.data_ptr() + 8 * n1, stride, stride - n1)
        torch.cuda.synchronize()
        assert n1 + n2 == no and np.array_equal(y.cpu().numpy()[:, :no], want)
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
