"""k_sense's dwell loop and launch geometry against the oracle (sense_cases.py: what the captures are, and
test_sense_cases_host.py: that every round and every lane of them decides part of every message).  Every other sensor
test runs one round and one launch; here the software-pipelined loop makes 2, 3 and 15 trips with dead groups and dead
workgroups in the last one, forced through OFDM_SENSE_SPLIT at every S and reached without it by two captures that are
large enough, the second of which needs two launches.  The oracle has no geometry: one result per capture, computed
once.  The bar is that of test_gpu_sense._compare: identical message bodies, means, decisions and hex maps."""
import numpy as np
import pytest

import sense_cases as sn
from helpers import loopback_stream, make_cfg, make_payloads
from ofdm_uhd_amd import config, engine, iqio
from test_gpu_sense import _compare

pytestmark = pytest.mark.gpu
KNOB = "OFDM_SENSE_SPLIT"
THREE_ROUNDS = sn.BY_ID["s256-dead-groups"]         # split 1, dwell 18 on G = 8: rounds of 8, 8 and 2 vectors


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(cfg=make_cfg("qpsk"))
    yield e
    e.close()


def _knob(monkeypatch, split):
    if split is None:
        monkeypatch.delenv(KNOB, raising=False)
    else:
        monkeypatch.setenv(KNOB, str(split))


def _run(orc, monkeypatch, e, c):
    sc, x, ref = sn.reference(orc, c)
    _knob(monkeypatch, c.split)
    got = e.sense(sc, x)
    assert len(got["msgs"]) == c.nmsgs and len(got["hex"]) == c.nmsgs // (c.avg + c.skip) >= 1
    _compare(got, ref, sc)
    return got


@pytest.mark.parametrize("c", sn.FORCED, ids=sn.ids(sn.FORCED))
def test_forced_geometry(eng, orc, monkeypatch, c):
    _run(orc, monkeypatch, eng, c)


@pytest.mark.parametrize("value", ["0", "-5", "1000000", "x"])
def test_knob_is_clamped(eng, orc, monkeypatch, value):
    """Whatever the knob holds ends up in [1, max_split]: dwell 32 on G = 8 runs as four rounds of one workgroup (0, -5,
    not a number) or one round of four (a million), never as anything the default could not choose."""
    c = sn.BY_ID["s256-nothing-dead"]
    sc, x, ref = sn.reference(orc, c)
    assert sn.geometry(c.S, c.dwell, c.nmsgs, 1).rounds == 4 and sn.geometry(c.S, c.dwell, c.nmsgs, 10 ** 6).nsplit == 4
    monkeypatch.setenv(KNOB, value)
    _compare(eng.sense(sc, x), ref, sc)


@pytest.mark.parametrize("c", sn.NATURAL, ids=sn.ids(sn.NATURAL))
def test_natural_geometry(eng, orc, monkeypatch, c):
    """The knob unset: 70 messages of the default sensor (nsplit 30, two rounds), and 65 537 messages (two launches)."""
    assert c.split is None
    _run(orc, monkeypatch, eng, c)


@pytest.mark.parametrize("c", sn.SC16, ids=sn.ids(sn.SC16))
def test_forced_geometry_sc16(orc, monkeypatch, c):
    """k_sense<NS, sc16> is an instantiation of its own: three rounds on 16-bit counts, the oracle on from_sc16 of them."""
    e = engine.Engine(cfg=make_cfg("qpsk"))
    e.set_rx_iq_format("sc16", c.rx_scale)
    try:
        got = _run(orc, monkeypatch, e, c)
    finally:
        e.close()
    assert float(got["msgs"].max()) > 0.0


def _fused_cfg():
    c = THREE_ROUNDS
    # 30 dB SNR puts the out-of-band noise floor near 5e-3 per bin: threshold between it and the signal
    return config.make_sense_cfg(c.S, c.tune, c.dwell, c.avg, c.skip, 0.05, sn.case_window(c))


@pytest.mark.parametrize("fmt", ["fc32", "sc16"])
def test_fused_three_rounds(orc, monkeypatch, fmt):
    """The sensor riding on ofdm_rx (second stream, same IQ buffer) with a three-round dwell: equal to the standalone
    call at the same split, to the standalone call at the default split, and to the oracle."""
    cfg = make_cfg("qpsk")
    iq = loopback_stream(orc, cfg, make_payloads(24, 300, seed=9), snr_db=30.0)
    x = iqio.to_sc16(iq) if fmt == "sc16" else iq
    xf = iqio.from_sc16(x) if fmt == "sc16" else iq
    sc = _fused_cfg()
    ref = orc.sense(sc, xf)
    assert len(ref["msgs"]) >= 6 and sn.geometry(sc.fft_size, sc.dwell_delay, len(ref["msgs"]), 1).rounds == 3
    e = engine.Engine(cfg=cfg)
    if fmt == "sc16":
        e.set_rx_iq_format("sc16")
    try:
        _knob(monkeypatch, None)
        plain = e.rx(x)
        default_split = e.sense(sc, x)
        _knob(monkeypatch, 1)
        alone = e.sense(sc, x)
        e.set_rx_sense(sc)
        fused_pk = e.rx(x)
        fused = e.rx_sense_result(len(x))
        fused_pk2 = e.rx(x)                     # second call: buffers are reused
        fused2 = e.rx_sense_result(len(x))
        e.set_rx_sense(None)
    finally:
        e.close()
    assert fused_pk == plain == fused_pk2 and len(plain) == 24 and all(ok for ok, _ in plain)
    for r in (default_split, alone, fused, fused2):
        _compare(r, ref, sc)


def test_window_reupload(eng, orc, monkeypatch):
    """Same S, other taps: sense_enqueue uploads the window again (and again on the way back)."""
    c = THREE_ROUNDS
    sc_a, x, ref_a = sn.reference(orc, c)
    sc_b = sn.sense_cfg(c, window=(0.5 + np.random.default_rng(77).random(c.S)).tolist())
    ref_b = orc.sense(sc_b, x)
    assert not np.array_equal(ref_a["msgs"], ref_b["msgs"])
    _knob(monkeypatch, c.split)
    for sc, ref in ((sc_a, ref_a), (sc_b, ref_b), (sc_a, ref_a), (sc_b, ref_b)):
        _compare(eng.sense(sc, x), ref, sc)


@pytest.mark.parametrize("value,rnd", [("nan", 1), ("inf", 2)])
def test_nonfinite_in_a_later_round(eng, orc, monkeypatch, value, rnd):
    """One NaN sample makes its vector's whole spectrum NaN, which the max-hold ignores (accrue_stats' `>`); one +Inf
    sample makes it Inf where the transform only adds it and NaN where it meets Inf - Inf or 0 * Inf, the same bins in
    engine and oracle since both run one schedule (sensor parity)."""
    c = THREE_ROUNDS
    sc, x, ref0 = sn.reference(orc, c)
    geo = sn.case_geometry(c)
    f = rnd * geo.stride + 1                       # an accrued vector of that round, message 0 (the one decided on)
    assert geo.slots[f][0] == rnd >= 1
    x2 = x.copy()
    x2[(c.tune + f) * c.S + 5] = {"nan": np.nan, "inf": np.inf}[value]
    ref = orc.sense(sc, x2)
    _knob(monkeypatch, c.split)
    got = eng.sense(sc, x2)
    assert np.array_equal(got["msgs"], ref["msgs"], equal_nan=True)
    assert np.array_equal(got["mean"], ref["mean"], equal_nan=True)
    assert np.array_equal(got["bits"], ref["bits"]) and got["hex"] == ref["hex"]
    assert not np.isnan(got["msgs"]).any()         # (powers are never NaN in a message: the atomicMax on bit patterns)
    if value == "nan":
        assert np.isfinite(got["msgs"]).all()
        # the poisoned vector is out, nothing else changed: message 0 lost the bin that vector held
        assert np.array_equal(got["msgs"][1:], ref0["msgs"][1:]) and (got["msgs"][0] <= ref0["msgs"][0]).all()
        assert not np.array_equal(got["msgs"][0], ref0["msgs"][0])
    else:
        assert np.isinf(got["msgs"][0]).any() and np.isfinite(got["msgs"][1:]).all()
        assert np.isinf(got["mean"][0]).any() and got["bits"][0][np.isinf(got["mean"][0])].max() == 0
