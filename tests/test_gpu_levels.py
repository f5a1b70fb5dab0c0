"""The engine against the oracle across input level: the captures of level_cases.py (what each is for and what the oracle
does with it: test_level_cases_host.py), every one through test_gpu_parity._check_rx -- all taps array_equal, packets,
flags, frames and the eight counters exact -- and then check_rx_tap_free: the lean kernel and the device-side counts.

No tolerance anywhere.  Finite input is held to the full bar also where it goes non-finite inside (e = +64, +70, +110,
+125: _check_rx compares the symbol taps with equal_nan = True, and +125 puts NaN into the filtered stream itself, which
is then compared with equal_nan = True as well).  A capture with a non-finite SAMPLE is held to: packets, flags, frames,
counters and the metric exact; the filtered stream array_equal with equal_nan = True; the other float taps equal outside
the symbols that hold a non-finite value on the oracle's side."""
import numpy as np
import pytest

import level_cases as lc
from ofdm_uhd_amd import _abi
from test_gpu_parity import STAT_KEYS, _check_rx, check_rx_tap_free

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engines():
    """One engine per geometry, reused across the levels (and one more for the 16-bit input format)."""
    from ofdm_uhd_amd import engine
    made = {}

    def get(geom, fmt=None):
        if (geom, fmt) not in made:
            e = engine.Engine(cfg=lc.cfg_of(geom))
            if fmt:
                e.set_rx_iq_format(fmt)
            made[(geom, fmt)] = e
        return made[(geom, fmt)]
    yield get
    for e in made.values():
        e.close()


def _both_paths(orc, eng, cfg, x, ro):
    pk = _check_rx(orc, cfg, eng, x, ro)
    check_rx_tap_free(eng, x, ro, eng.rx_packet_pos().tolist())
    return pk


@pytest.mark.parametrize("geom,e", lc.UNIFORM, ids=lc.UNIFORM_IDS)
def test_uniform_level(orc, engines, geom, e):
    cfg, x, ro = lc.uniform(orc, geom, e)
    eng = engines(geom)
    if e == 125:
        # the filtered stream itself holds NaN (finite input, the transform overflows): the same NaNs at the same places
        eng.set_taps(_abi.TAP_RX_CHAN_FILT)
        eng.rx(x)
        a, b = eng.tap(_abi.TAP_RX_CHAN_FILT), ro.tap(_abi.TAP_RX_CHAN_FILT)
        assert lc.n_nonfinite(b) > 0 and np.array_equal(a, b, equal_nan=True)
        _nan_bar(eng, x, ro, whole=True)
        return
    pk = _both_paths(orc, eng, cfg, x, ro)
    if lc.WINDOW[0] <= e <= lc.WINDOW[1] and geom in lc.SMALL:
        assert [p for ok, p in pk if ok] == lc.payloads(geom)


@pytest.mark.parametrize("k,order", lc.STEPS, ids=lc.STEP_IDS)
def test_two_bursts(orc, engines, k, order):
    cfg, x, ro, pay = lc.step(orc, k, order)
    _both_paths(orc, engines(lc.STEP_GEOM), cfg, x, ro)


def test_sc16_low_level(orc, engines):
    """rms ~ 10 counts: the engine's 16-bit path on q against the oracle on from_sc16(q)."""
    cfg, q, ro = lc.sc16(orc)
    pk = _both_paths(orc, engines("qpsk-512", "sc16"), cfg, q, ro)
    assert [p for ok, p in pk if ok] == lc.payloads("qpsk-512")


def _rows_finite(a):
    return np.isfinite(a.view(np.float32).reshape(len(a), -1)).all(axis=1)


def _nan_bar(eng, x, ro, whole=False):
    """The bar for a capture whose filtered stream holds non-finite values (module docstring).  whole: finite input --
    nothing is left out, every tap is compared in full with equal_nan = True."""
    eng.set_taps(*lc.RX_TAPS)
    pk = eng.rx(x)
    assert pk == ro.packets
    assert eng.tap(_abi.TAP_RX_PACKETS).tobytes() == ro.tap(_abi.TAP_RX_PACKETS).tobytes()
    assert eng.tap(_abi.TAP_RX_PEAKS).tolist() == ro.tap(_abi.TAP_RX_PEAKS).tolist()
    assert eng.tap(_abi.TAP_RX_FRAMES).tolist() == ro.tap(_abi.TAP_RX_FRAMES).tolist()
    for k in STAT_KEYS:
        assert eng.last_stats[k] == ro.stats[k], k
    assert eng.last_stats["overflow"] == 0
    assert np.array_equal(eng.tap(_abi.TAP_RX_METRIC), ro.tap(_abi.TAP_RX_METRIC))
    assert np.array_equal(eng.tap(_abi.TAP_RX_CHAN_FILT), ro.tap(_abi.TAP_RX_CHAN_FILT), equal_nan=True)
    # the pre-selection is finite on both sides by construction (M <= 1024 also for NaN) and has no symbols to leave out
    assert np.array_equal(eng.tap(_abi.TAP_RX_PRESEL), ro.tap(_abi.TAP_RX_PRESEL))
    # the flag angles: one per flag; those the oracle has finite
    a, b = eng.tap(_abi.TAP_RX_ANGLES), ro.tap(_abi.TAP_RX_ANGLES)
    assert a.shape == b.shape
    fin = np.isfinite(b) | whole
    assert np.array_equal(a[fin], b[fin], equal_nan=True)
    for tap in (_abi.TAP_RX_FFT, _abi.TAP_RX_ACQ, _abi.TAP_RX_SINK):
        a, b = eng.tap(tap), ro.tap(tap)
        assert a.shape == b.shape, tap
        fin = _rows_finite(b) | whole
        assert np.array_equal(a[fin], b[fin], equal_nan=True), tap
    check_rx_tap_free(eng, x, ro, eng.rx_packet_pos().tolist())
    return pk


@pytest.mark.parametrize("value,position", lc.POISON, ids=lc.POISON_IDS)
def test_one_nonfinite_sample(orc, engines, value, position):
    cfg, x, ro, i = lc.poisoned(orc, value, position)
    _nan_bar(engines("qpsk-512"), x, ro)
