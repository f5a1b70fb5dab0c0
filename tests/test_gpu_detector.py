"""The engine's OFDM_TAP_RX_RUN_AVG -- the average k_peak starts every run from -- against the oracle (bit for bit)
and, on its own, against the float64 recurrence of tests/test_detector_average.py (a); on the fused front end, across
k_sync segments, with the tap off; and the engine's accepted range of alpha."""
import numpy as np
import pytest

import np_model as npm
from helpers import (DETECTOR_ALPHAS, DETECTOR_GEOMS, detector_capture, loopback_stream, make_cfg, make_payloads,
                     noise_capture, run_avg_tolerance)
from ofdm_uhd_amd import _abi

pytestmark = pytest.mark.gpu

TAPS = (_abi.TAP_RX_METRIC, _abi.TAP_RX_PRESEL, _abi.TAP_RX_RUN_AVG)
CASES = [(g, s, a, rf) for g in DETECTOR_GEOMS for s in (12.0, 30.0) for a in DETECTOR_ALPHAS
         for rf in ((0.2, 0.2), (0.5, 0.2))]
_X = {}


def _x(orc, geom, snr, lead=None):
    key = (geom, snr, lead)
    if key not in _X:
        _X[key] = detector_capture(orc, *geom, snr, lead=lead)
    return _X[key]


def _cfg(geom, alpha, rise, fall):
    cfg = make_cfg("qpsk", *geom)
    cfg.peak_rise, cfg.peak_fall, cfg.peak_alpha = rise, fall, alpha
    return cfg


def _check(orc, cfg, x):
    from ofdm_uhd_amd import engine
    eng = engine.Engine(cfg=cfg)
    ro = orc.rx(cfg, x, sum(1 << t for t in TAPS))
    eng.set_taps(*TAPS)
    pk = eng.rx(x)
    rows = eng.tap(_abi.TAP_RX_RUN_AVG)
    assert np.array_equal(rows, ro.tap(_abi.TAP_RX_RUN_AVG))
    assert eng.tap(_abi.TAP_RX_PEAKS).tolist() == ro.tap(_abi.TAP_RX_PEAKS).tolist() and pk == ro.packets
    # the engine's rows on their own against float64, from the engine's own metric taps (the ranges are the oracle's)
    u, u32 = eng.tap(_abi.TAP_RX_METRIC), eng.tap(_abi.TAP_RX_PRESEL)
    ref = npm.run_start_avg(u, u32, ro.tap(orc.TAP_RANGES), cfg.peak_alpha, rows[:, 0].astype(np.int64))
    assert len(rows) > 0
    assert np.all(np.abs(rows[:, 1] - ref) <= run_avg_tolerance(cfg.peak_alpha) * (1.0 + np.abs(ref)))
    eng.close()
    return rows


@pytest.mark.parametrize("geom,snr,alpha,rf", CASES)
def test_run_avg_parity_and_float64(orc, geom, snr, alpha, rf):
    _check(orc, _cfg(geom, alpha, *rf), _x(orc, geom, snr))


@pytest.mark.parametrize("alpha", DETECTOR_ALPHAS)
def test_run_avg_designed_captures(orc, alpha):
    """a burst 200 samples after a tile boundary; a noise-only stream whose runs all come from the noise"""
    geom = (512, 200, 128)
    rows = _check(orc, _cfg(geom, alpha, 0.5, 0.2), _x(orc, geom, 30.0, 2 * 2048 + 200))
    assert rows[0, 0] // 2048 == 2
    _check(orc, _cfg((64, 48, 16), alpha, 0.8, 0.6), noise_capture(orc))


@pytest.mark.parametrize("alpha", [0.001, 0.005])
def test_run_avg_fused_front_end(orc, monkeypatch, alpha):
    monkeypatch.setenv("OFDM_FRONT", "1")
    _check(orc, _cfg((512, 200, 128), alpha, 0.5, 0.2), _x(orc, (512, 200, 128), 30.0))


def test_run_avg_across_sync_segments(orc):
    """a stream over several 32-tile k_sync segments: the rows of the oracle's single sequential pass"""
    cfg = make_cfg("qpsk", 64, 48, 16)
    cfg.peak_alpha = 0.005
    x = loopback_stream(orc, cfg, make_payloads(400, 200, seed=4), snr_db=30.0)
    assert len(x) > 3 * 32 * 2048
    rows = _check(orc, cfg, x)
    assert len(rows) >= 400


def test_run_avg_changes_nothing_and_is_refused_when_off(orc):
    from ofdm_uhd_amd import engine
    cfg = _cfg((512, 200, 128), 0.002, 0.5, 0.2)
    x = _x(orc, (512, 200, 128), 12.0)
    eng = engine.Engine(cfg=cfg)
    pk0 = eng.rx(x)
    peaks0 = eng.tap(_abi.TAP_RX_PEAKS).tolist()
    with pytest.raises(ValueError):
        eng.tap(_abi.TAP_RX_RUN_AVG)                 # not enabled
    eng.set_taps(_abi.TAP_RX_RUN_AVG)
    assert eng.rx(x) == pk0 and eng.tap(_abi.TAP_RX_PEAKS).tolist() == peaks0
    assert len(eng.tap(_abi.TAP_RX_RUN_AVG)) > 0
    eng.close()


def test_engine_alpha_range():
    from ofdm_uhd_amd import engine
    for alpha in (0.0, -0.001, 0.0051, 0.01, 0.25, float("nan")):
        cfg = make_cfg("qpsk")
        cfg.peak_alpha = alpha
        with pytest.raises(ValueError):
            engine.Engine(cfg=cfg)
    cfg = make_cfg("qpsk")
    cfg.peak_alpha = 0.005
    engine.Engine(cfg=cfg).close()
