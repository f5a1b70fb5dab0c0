"""The memory-polynomial stage on the GPU (csrc/mempoly.h, ofdm_set_mempoly / ofdm_mempoly; Engine.dpd and Engine.pa are
its two slots): bit for bit the NumPy float32 model of the definition (mempoly_cases; test_mempoly_host.py holds the
model to the float64 one), in both output formats and on both slots, across any chunking, at its anchors, in its
statistics, through the refusals, and end to end: ofdm_mod(cfr=, dpd=) -> Engine.pa -> ofdm_demod.

CPU pre-check of the end-to-end scenario (the oracle's transmitter at N = 512 / occ = 200 / CP = 128 / QPSK and
amplitude 0.32, rms 0.2 at the data symbols; six 400-byte packets; cfr_cases.model at 7 dB with H = 16, threshold
0.4477; the float32 models of the predistorter and of dpd.example_pa() chained; the table trained on a probe of payload
seed 1 in two iterations, on the same float32 models: -55.8 / -57.0 dB), the error of the amplifier's output against
a[0][0] times the CFR stage's output, and the oracle's receiver on the amplifier's output:
  payload seed 3     -57.04 dB with the predistorter (float64 models: -57.04), -25.43 dB without: 31.6 dB; 6 of 6 decode
  payload seed 7     -57.25 dB (float64 -57.25), -25.42 dB without: 31.8 dB; 6 of 6 decode
  payload seed 31    -56.65 dB (float64 -56.65), -25.41 dB without: 31.2 dB; 6 of 6 decode
A probe of payload seed 2 and a third iteration move no figure by more than 0.02 dB.  The predistorter takes the peak
from 0.4477 to 0.497 .. 0.502.  The test uses payload seed 3 and the condition the issue sets, 20 dB."""
import ctypes as C

import numpy as np
import pytest

import cfr_cases as cc
import mempoly_cases as mc
import stage_harness as sh
from helpers import make_payloads
from ofdm_uhd_amd import _abi, cfr, dpd, engine, iqio, ofdm, options
from stage_harness import eng  # noqa: F401  (the module's engine)

pytestmark = pytest.mark.gpu

COUNTS = ("n", "n_over", "peak_in", "peak_out")
SUMS = ("sum_in", "sum_out")
SLOTS = ("dpd", "pa")


def _set(eng, slot, cfg):
    getattr(eng, "set_" + slot)(cfg)


def _run(eng, slot, name, **kw):
    _set(eng, slot, mc.cfg_of(name, **kw))
    return getattr(eng, slot)(mc.input_of(name))


@pytest.fixture(scope="module")
def models():
    return {name: mc.model_of(name) for name in mc.NAMES}


# ---- 1. the model, bit for bit -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slot", SLOTS)
@pytest.mark.parametrize("fmt", ["fc32", "sc16"])
@pytest.mark.parametrize("name", mc.NAMES)
def test_every_case_is_the_model_bit_for_bit(eng, models, name, fmt, slot):
    y = _run(eng, slot, name, out_format=fmt, out_scale=30000.0 if fmt == "sc16" else None)
    want = models[name].y
    if fmt == "sc16":
        assert y.dtype == np.int16 and np.array_equal(y, iqio.to_sc16(want, 30000.0))
        assert np.abs(y).max() > 3000                                                    # (the samples use the range)
    else:
        assert y.dtype == np.complex64 and np.array_equal(y.view(np.uint32), want.view(np.uint32))


# ---- 2. chunks -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["fc32", "sc16"])
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("M", [3, 8])
def test_a_stream_in_chunks_is_the_stream_in_one_call_bit_for_bit(eng, M, reverse, fmt):
    chunks = [1, 2, M - 2, M - 1, M, 997, 1023, 1025]
    if reverse:
        chunks = chunks[::-1]
    x = mc.stream(sum(chunks), seed=5)
    coef = mc.table(M, 3, seed=50 + M)
    want = mc.model(x, coef)
    limit = float(np.sqrt(np.median(want.yy)))
    cfg = dpd.mempoly_cfg(coef, out_format=fmt, limit=limit)
    eng.set_dpd(cfg)
    whole = eng.dpd(x)
    st_whole = eng.dpd_stats()
    assert 0 < st_whole["n_over"] < len(x)
    eng.dpd_reset()
    parts, a = [], 0
    empty = np.zeros(0, np.complex64)
    for n in chunks:
        assert len(eng.dpd(empty)) == 0
        parts.append(eng.dpd(x[a:a + n]))
        a += n
    assert len(eng.dpd(empty)) == 0
    assert np.array_equal(sh.bits(np.concatenate(parts)), sh.bits(whole))
    st = eng.dpd_stats()
    assert [st[k] for k in COUNTS] == [st_whole[k] for k in COUNTS]
    for k in SUMS:
        assert st[k] == pytest.approx(st_whole[k], rel=1e-9)
    if fmt == "fc32":
        assert np.array_equal(whole.view(np.uint32), want.y.view(np.uint32))


def test_calls_interleaved_on_the_two_slots_disturb_neither(eng, models):
    a, b = "m8k5", "example_pa"
    xa, xb = mc.input_of(a), mc.input_of(b)
    eng.set_dpd(mc.cfg_of(a, limit=0.2))
    eng.set_pa(mc.cfg_of(b, out_format="sc16", out_scale=30000.0))
    cuts_a, cuts_b = [0, 5, 1030, 1031, 2000, len(xa)], [0, 1, 3, 1500, 1501, len(xb)]
    ya, yb = [], []
    for i in range(5):
        ya.append(eng.dpd(xa[cuts_a[i]:cuts_a[i + 1]]))
        yb.append(eng.pa(xb[cuts_b[i]:cuts_b[i + 1]]))
    assert np.array_equal(np.concatenate(ya).view(np.uint32), models[a].y.view(np.uint32))
    assert np.array_equal(np.concatenate(yb), iqio.to_sc16(models[b].y, 30000.0))
    got, want = eng.dpd_stats(), mc.statistics(models[a], 0.2)
    assert [got[k] for k in COUNTS] == [want[k] for k in COUNTS] and got["n_over"] > 0
    assert eng.pa_stats()["n"] == len(xb) and eng.pa_stats()["n_over"] == 0
    # a reset or a new configuration of one slot leaves the other's stream where it is
    eng.set_pa(mc.cfg_of(b))
    half = len(xa) // 2
    eng.dpd_reset()
    first = eng.dpd(xa[:half])
    eng.pa(xb[:100])
    eng.pa_reset()
    eng.set_pa(None)
    assert eng.pa_cfg is None
    assert np.array_equal(np.concatenate([first, eng.dpd(xa[half:])]).view(np.uint32), models[a].y.view(np.uint32))


# ---- 3. anchors ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slot", SLOTS)
def test_identity_returns_the_inputs_values(eng, slot):
    x = mc.stream(mc.length(8), seed=9)
    for M, K in ((1, 1), (3, 3), (8, 5)):
        _set(eng, slot, dpd.mempoly_cfg(dpd.identity(M, K)))
        assert np.array_equal(getattr(eng, slot)(x), x)         # (values: a zero's sign may differ, by the definition)
    _set(eng, slot, dpd.mempoly_cfg(dpd.identity(3, 3), out_format="sc16", out_scale=1000.0))
    assert np.array_equal(getattr(eng, slot)(x), iqio.to_sc16(x, 1000.0))


def test_one_tap_of_order_1_is_the_gr_complex_product(eng):
    x = mc.stream(mc.length(1), seed=10)
    g = np.complex64(0.75 - 0.5j)
    eng.set_dpd(coef=[[g]])
    want = np.empty(len(x), np.complex64)
    want.real = g.real * x.real - g.imag * x.imag
    want.imag = g.real * x.imag + g.imag * x.real
    assert np.array_equal(eng.dpd(x).view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("m", [1, 2, 7])
def test_a_single_linear_tap_delays_by_exactly_m(eng, m):
    x = mc.stream(mc.length(8), seed=11)
    a = np.zeros((8, 2), np.complex64)
    a[m, 0] = 1.0
    eng.set_pa(coef=a)
    y = eng.pa(x)
    assert np.array_equal(y[m:], x[:len(x) - m]) and not y[:m].any()
    # the next call begins with the carried samples
    assert np.array_equal(eng.pa(x[:50])[:m], x[len(x) - m:])


# ---- 4. statistics -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", mc.NAMES)
def test_statistics_are_the_models(eng, models, name):
    mag = np.sqrt(models[name].yy.astype(np.float64))
    limit = float(np.float32(0.5 * (mag.min() + mag.max())))   # between the smallest and the largest |y|
    _run(eng, "dpd", name, limit=limit)
    got, want = eng.dpd_stats(), mc.statistics(models[name], limit)
    print(name, got)
    assert 0 < want["n_over"] < want["n"]
    assert [got[k] for k in COUNTS] == [want[k] for k in COUNTS]
    for k in SUMS:
        # the terms are the model's float32 values bit for bit: only the order of the float64 additions differs
        assert got[k] == pytest.approx(want[k], rel=1e-9, abs=0.0)
    # they accumulate over calls, and a reset or a new configuration starts them afresh
    eng.dpd(mc.input_of(name)[:100])
    assert eng.dpd_stats()["n"] == want["n"] + 100 and eng.dpd_stats()["n_over"] >= want["n_over"]
    eng.dpd_reset()
    zero = eng.dpd_stats()
    assert all(zero[k] == 0 for k in COUNTS + SUMS)
    eng.dpd(mc.input_of(name)[:100])
    eng.set_dpd(mc.cfg_of(name))
    zero = eng.dpd_stats()
    assert all(zero[k] == 0 for k in COUNTS + SUMS)
    # without a limit nothing is counted
    eng.dpd(mc.input_of(name))
    inf = eng.dpd_stats()
    assert inf["n_over"] == 0 and inf["peak_out"] == want["peak_out"]


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------
def _raw(eng, slot, cfg):
    return eng._lib.ofdm_set_mempoly(eng._h, slot, C.byref(cfg)), (eng._lib.ofdm_last_error(eng._h) or b"").decode()


def _err(eng):
    return eng._lib.ofdm_last_error(eng._h).decode()


def test_every_refusal_has_its_message_and_leaves_the_stream_as_it_was(eng):
    name = "m3k3"
    x = mc.input_of(name)
    want = mc.model_of(name).y
    half = len(x) // 2
    eng.set_dpd(mc.cfg_of(name))
    first = eng.dpd(x[:half])
    good = mc.cfg_of(name)
    DPD = _abi.OFDM_MEMPOLY_DPD

    def changed(**kw):
        cfg = mc.cfg_of(name)
        for k, v in kw.items():
            if k == "coef":
                setattr(cfg.coef[v[0]], v[1], v[2])
            else:
                setattr(cfg, k, v)
        return cfg
    nan, inf = float("nan"), float("inf")
    bad = [(changed(struct_size=good.struct_size - 4), "struct_size"),
           (changed(memory=0), "memory"), (changed(memory=9), "memory"),
           (changed(orders=0), "orders"), (changed(orders=6), "orders"),
           (changed(coef=(0, "re", nan)), "coef"), (changed(coef=(2 * 5 + 2, "im", inf)), "coef"),
           (changed(coef=(1 * 5 + 1, "re", -inf)), "coef"),
           (changed(limit=0.0), "limit"), (changed(limit=-1.0), "limit"), (changed(limit=nan), "limit"),
           (changed(limit=-inf), "limit"), (changed(out_format=7), "out_format"),
           (changed(out_format=_abi.OFDM_IQ_SC16, out_scale=-1.0), "out_scale")]
    for cfg, word in bad:
        rc, msg = _raw(eng, DPD, cfg)
        assert rc == _abi.OFDM_E_INVAL and word in msg, (word, msg)
    # entries outside the (memory, orders) corner are not looked at, and +inf is a limit
    assert _raw(eng, _abi.OFDM_MEMPOLY_PA, changed(coef=(0 * 5 + 3, "re", nan), limit=inf))[0] == _abi.OFDM_OK
    eng.set_pa(None)
    # a slot that does not exist, through every entry point
    n = C.c_uint64(0)
    st = _abi.ofdm_mempoly_stats()
    ms = C.c_double(0)
    buf = np.zeros(4096, np.complex64)             # every pointer below lies inside it
    buf[1500:2500] = x[half:half + 1000]
    p = buf.ctypes.data + 8 * 1500
    for slot in (2, 0xFFFFFFFF):
        rc, msg = _raw(eng, slot, good)
        assert rc == _abi.OFDM_E_INVAL and "slot" in msg
        assert eng._lib.ofdm_mempoly_reset(eng._h, slot) == _abi.OFDM_E_INVAL and "slot" in _err(eng)
        assert eng._lib.ofdm_mempoly_stats(eng._h, slot, C.byref(st)) == _abi.OFDM_E_INVAL and "slot" in _err(eng)
        rc = eng._lib.ofdm_mempoly(eng._h, slot, C.c_void_p(p), 1000, C.c_void_p(buf.ctypes.data), 1000, C.byref(n))
        assert rc == _abi.OFDM_E_INVAL and "slot" in _err(eng)
        assert eng._lib.ofdm_mempoly_last_ms(eng._h, slot, C.byref(ms)) == _abi.OFDM_E_INVAL
    # calls that are refused: overlapping buffers, a short output, a misaligned pointer, a call too long (nothing is
    # touched: the fourth is refused by its length alone), and they move nothing
    for out in (p, p + 8 * 999, p - 8 * 999):
        rc = eng._lib.ofdm_mempoly(eng._h, DPD, C.c_void_p(p), 1000, C.c_void_p(out), 1000, C.byref(n))
        assert rc == _abi.OFDM_E_INVAL and "overlaps" in _err(eng)
    rc = eng._lib.ofdm_mempoly(eng._h, DPD, C.c_void_p(p), 1000, C.c_void_p(p + 8 * 1000), 999, C.byref(n))
    assert rc == _abi.OFDM_E_CAPACITY and n.value == 1000
    rc = eng._lib.ofdm_mempoly(eng._h, DPD, C.c_void_p(p + 4), 1000, C.c_void_p(buf.ctypes.data), 1000, C.byref(n))
    assert rc == _abi.OFDM_E_INVAL and "aligned" in _err(eng)
    long = 2 ** 34 + 1
    rc = eng._lib.ofdm_mempoly(eng._h, DPD, C.c_void_p(p), long, C.c_void_p(p + 8 * long), long, C.byref(n))
    assert rc == _abi.OFDM_E_INVAL and "too long" in _err(eng)
    assert eng.dpd_stats()["n"] == half
    # the stream continues as if none of these calls had been made
    assert np.array_equal(np.concatenate([first, eng.dpd(x[half:])]).view(np.uint32), want.view(np.uint32))
    assert eng.dpd_stats()["n"] == len(x)


@pytest.mark.parametrize("slot", SLOTS)
def test_calls_on_a_slot_that_was_not_set_are_refused(eng, slot):
    other = SLOTS[1 - SLOTS.index(slot)]
    _set(eng, other, mc.cfg_of("m3k3"))            # the other slot's configuration does not stand in
    _set(eng, slot, None)
    assert getattr(eng, slot + "_cfg") is None
    with pytest.raises(ValueError):
        getattr(eng, slot)(np.zeros(10, np.complex64))
    n = C.c_uint64(0)
    x, y = np.zeros(10, np.complex64), np.zeros(10, np.complex64)
    number = {"dpd": _abi.OFDM_MEMPOLY_DPD, "pa": _abi.OFDM_MEMPOLY_PA}[slot]
    rc = eng._lib.ofdm_mempoly(eng._h, number, C.c_void_p(x.ctypes.data), 10, C.c_void_p(y.ctypes.data), 10, C.byref(n))
    assert rc == _abi.OFDM_E_INVAL and "without ofdm_set_mempoly" in _err(eng)
    for call in ("_reset", "_stats", "_last_ms"):
        with pytest.raises(ValueError):
            getattr(eng, slot + call)()
    _set(eng, slot, mc.cfg_of("m3k3"))
    with pytest.raises(ValueError):
        getattr(eng, slot)(np.zeros((10, 2), np.int16))
    # the kernel table is what it was, and each slot reports its own time
    eng.prof_enable(True)
    try:
        eng.prof_reset()
        getattr(eng, slot)(mc.input_of("m3k3"))
        assert getattr(eng, slot + "_last_ms")() > 0.0
        with pytest.raises(ValueError):
            getattr(eng, other + "_last_ms")()     # that slot ran no profiled call
        ca = sh.launches(eng)
        assert len(ca) == _abi.K_COUNT == 11 and sum(ca.values()) == 0
    finally:
        eng.prof_enable(False)


# ---- 6. end to end -------------------------------------------------------------------------------------------------------
AMP = 0.32          # rms 0.2 at N = 512 / occ = 200: sqrt(200 / 512) * 0.32


def _modulator(**kw):
    opt = options.default_options(modulation="qpsk", fft_length=512, occupied_tones=200, cp_length=128)
    m = ofdm.ofdm_mod(opt, pad_for_usrp=False, **kw)
    m.engine().set_tx_amplitude(AMP)
    m.set_cfr_amplitude(AMP)
    return m


def _stream(m, payloads):
    for p in payloads:
        m.send_pkt(p)
    return m.flush(end=True)


def test_ofdm_mod_with_cfr_and_dpd_through_the_amplifier_feeds_ofdm_demod():
    """CFR at 7 dB, the predistorter trained on a probe of payload seed 1, dpd.example_pa(), ofdm_demod: the figures of
    the CPU pre-check are in the file's docstring."""
    stage = dict(papr_db=7.0, half_width=16)
    sent = make_payloads(6, 400, seed=3)
    pa = dpd.example_pa()
    g = complex(pa[0, 0])
    raw, limited = _modulator(), _modulator(cfr=stage)
    opt = options.default_options(modulation="qpsk", fft_length=512, occupied_tones=200, cp_length=128)
    rx = ofdm.ofdm_demod(opt)
    air = engine.Engine(opt)
    tx = None
    try:
        # the table: the probe through both slots on the GPU, the fit on the host
        probe = _stream(limited, make_payloads(6, 400, seed=1))
        air.set_pa(coef=pa)
        coef, nmse = dpd.train(air, probe, memory=3, orders=3, iterations=2)
        print("training: %s dB" % ", ".join("%.2f" % v for v in nmse))
        assert coef.shape == (3, 3) and len(nmse) == 2 and np.array_equal(dpd.coef_of(air.dpd_cfg), coef)
        tx = _modulator(cfr=stage, dpd=dict(coef=coef, limit=1.0))
        e = tx.engine()
        assert e.cfr_cfg.out_format == _abi.OFDM_IQ_FC32 and e.dpd_cfg.out_format == _abi.OFDM_IQ_FC32
        assert tx.last_dpd is None
        iq, s, x = _stream(tx, sent), _stream(limited, sent), _stream(raw, sent)
        assert len(iq) == len(s) == len(x) + 16 and iq.dtype == np.complex64
        # the stream is the float32 models chained: CFR's of the modulator's own samples, then this stage's
        A = cfr.threshold_for(7.0, AMP * np.sqrt(200 / 512.0))
        assert np.float32(A) == np.float32(e.cfr_cfg.threshold)
        s_model = cc.model(np.concatenate([x, np.zeros(16, np.complex64)]), A, cfr.design(16)).y
        assert np.array_equal(s.view(np.uint32), s_model.view(np.uint32))
        assert np.array_equal(iq.view(np.uint32), mc.model(s_model, coef).y.view(np.uint32))
        r = tx.last_dpd
        print("dpd end to end:", r)
        assert set(r) == {"gain_db", "peak_expansion_db", "share_over"}
        assert r["peak_expansion_db"] > 0.0 and r["share_over"] == 0.0 and abs(r["gain_db"]) < 1.0
        # through the amplifier, with and without the predistorter
        air.pa_reset()
        v = air.pa(iq)
        assert np.array_equal(v.view(np.uint32), mc.model(iq, pa).y.view(np.uint32))
        air.pa_reset()
        v0 = air.pa(s)
        ref = g * s.astype(np.complex128)
        with_dpd, without = dpd.nmse_db(v, ref), dpd.nmse_db(v0, ref)
        in_float64 = dpd.nmse_db(dpd.apply64(dpd.apply64(s, coef), pa), ref)
        print("NMSE against a[0][0] s: %.2f dB with the predistorter (float64 models %.2f dB), %.2f dB without" % (
            with_dpd, in_float64, without))
        assert abs(with_dpd - in_float64) <= 1.0
        assert with_dpd <= without - 20.0
        got = rx.work(np.concatenate([v, np.zeros(2048, np.complex64)]))
        assert [p for ok, p in got if ok] == sent
        # a second stream starts afresh, and another table goes in between streams
        assert np.array_equal(_stream(tx, sent), iq) and tx.last_dpd == r
        tx.set_dpd_coef(dpd.identity(1, 1))
        assert np.array_equal(_stream(tx, sent), s)
    finally:
        for m in (raw, limited, rx, tx):
            if m is not None:
                m.engine().close()
        air.close()


def test_ofdm_mod_with_dpd_alone_stores_the_16_bit_samples_and_without_it_is_what_it_was():
    sent = make_payloads(2, 200, seed=4)
    coef = mc.table(2, 2, seed=77)
    plain = _modulator()
    tx = _modulator(iq_format="sc16", iq_scale=30000.0, dpd=dict(coef=coef, limit=0.3))
    try:
        assert plain.last_dpd is None and plain.engine().dpd_cfg is None
        with pytest.raises(ValueError):
            plain.set_dpd_coef(coef)
        x = _stream(plain, sent)
        assert tx.engine().dpd_cfg.out_format == _abi.OFDM_IQ_SC16
        y = _stream(tx, sent)
        want = mc.model(x, coef)
        assert y.dtype == np.int16 and np.array_equal(y, iqio.to_sc16(want.y, 30000.0))
        r, r_model = tx.last_dpd, dpd.report(mc.statistics(want, 0.3))
        assert 0.0 < r["share_over"] == r_model["share_over"] and r["peak_expansion_db"] == r_model["peak_expansion_db"]
        assert r["gain_db"] == pytest.approx(r_model["gain_db"], abs=1e-6)
        assert tx.flush(end=True) is None          # nothing queued, nothing running: the stage has no tail
        with pytest.raises(ValueError):
            ofdm.ofdm_mod(options.default_options(modulation="qpsk"), dpd=dict(coef=coef, gain=1.0))
    finally:
        plain.engine().close()
        tx.engine().close()
