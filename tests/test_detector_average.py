"""The peak detector's running average at the first sample of every run (OFDM_TAP_RX_RUN_AVG), held to float64.

Engine and oracle evaluate gr_peak_detector_fb's average avg = alpha*u + (1-alpha)*avg in ONE normative closed form
over 2048-sample tiles and agree on it bit for bit, so parity cannot see an error they share.
Here the oracle's tap -- the value the state machine starts each run from -- is compared with a float64 recurrence:
(a) over the very samples the closed form weights, which leaves only its own rounding; (b) over the exact metric, the
block's own semantics; (c) the flags of the normative, the literal float32 and the float64 evaluation may differ only
on runs the float64 machine decides by less than 1e-5; (d) alpha outside (0, 0.005] is refused."""
import functools

import numpy as np
import pytest

import np_model as npm
from helpers import (DETECTOR_ALPHAS, DETECTOR_GEOMS, DETECTOR_RISE_FALL, detector_capture, make_cfg, noise_capture,
                     run_avg_tolerance)
from ofdm_uhd_amd import _abi

SNRS = (12.0, 30.0, 60.0)
GRID = [(g, s, a) for g in DETECTOR_GEOMS for s in SNRS for a in DETECTOR_ALPHAS]   # x the four rise / fall pairs
TAPS = (1 << _abi.TAP_RX_METRIC) | (1 << _abi.TAP_RX_PRESEL) | (1 << _abi.TAP_RX_RUN_AVG)
# largest pre-selection error |u32 - u| allowed outside the exact ranges (premise of (b), asserted there; the grid
# shows 1.4e-6 -- the ill-conditioned places where the pre-selection is off by up to 1e-3 are evaluated exactly)
PRESEL_OUT = 1.5e-5
MARGIN = 1e-5


@functools.lru_cache(maxsize=8)
def _capture(orc, geom, snr, lead):
    return detector_capture(orc, *geom, snr, lead=lead)


def _case(orc, x, geom, alpha, rise, fall):
    cfg = make_cfg("qpsk", *geom)
    cfg.peak_rise, cfg.peak_fall, cfg.peak_alpha = rise, fall, alpha
    r = orc.rx(cfg, x, TAPS)
    assert r.presel_miss == 0                       # every sample above theta lies in an exact range
    u, u32, rg = r.tap(_abi.TAP_RX_METRIC), r.tap(_abi.TAP_RX_PRESEL), r.tap(orc.TAP_RANGES)
    rows = r.tap(_abi.TAP_RX_RUN_AVG)
    avg_u = npm.detector_avg(u, alpha)
    flags, runs, margin = npm.peak_detect_margins(u, rise, fall, alpha, avg=avg_u)
    return dict(rows=rows, u=u, u32=u32, ranges=rg, avg_u=avg_u, f64=flags, runs=runs, margin=margin,
                norm=r.tap(_abi.TAP_RX_PEAKS), lit=r.tap(orc.TAP_PEAKS_GR))


def _check_against_float64(c, alpha):
    """(a): rows sorted, one per maximal run u > theta, and the average within run_avg_tolerance(alpha) of float64."""
    rows = c["rows"]
    starts = rows[:, 0].astype(np.int64)
    assert np.array_equal(starts, c["runs"][:, 0])
    ref = npm.run_start_avg(c["u"], c["u32"], c["ranges"], alpha, starts)
    err = np.abs(rows[:, 1] - ref)
    tol = min(run_avg_tolerance(alpha), 5e-6)      # (the cap only binds outside the accepted range)
    bad = np.flatnonzero(err > tol * (1.0 + np.abs(ref)))
    assert len(bad) == 0, "run at %d: tap %r, float64 %r (tol %.2e)" % (starts[bad[0]], rows[bad[0], 1], ref[bad[0]], tol)


def _check_flags(c):
    """(c): the three evaluations raise the same flags except inside runs decided by less than MARGIN."""
    runs, marginal = c["runs"], c["margin"] < MARGIN

    def settled(flags):
        out = []
        for p in np.asarray(flags, np.int64).tolist():
            k = int(np.searchsorted(runs[:, 0], p, "right")) - 1
            assert k >= 0 and runs[k, 0] <= p <= runs[k, 1], p          # every flag lies in a run
            if not marginal[k]:
                out.append(p)
        return out
    assert settled(c["norm"]) == settled(c["lit"]) == settled(c["f64"])


def test_tolerance_is_tight():
    """The bound the float64 comparison uses: Q40 (about decay^-2048 * 2^-41 / (e * alpha)) plus 24 float32 ulps, never
    looser than 5e-6 on the accepted range, and what lets alpha = 0.01 through is already 1e-2."""
    assert all(run_avg_tolerance(a) <= 5e-6 for a in DETECTOR_ALPHAS)
    assert 0.9e-6 < run_avg_tolerance(0.005) - 24 * 2.0 ** -24 < 1.1e-6
    assert run_avg_tolerance(0.01) > 1e-2


@pytest.mark.parametrize("geom,snr,alpha", GRID)
def test_run_start_average_against_float64(orc, geom, snr, alpha):
    """(a) Same operation, high precision.  The tap holds float32(avg_in * decay^s + (B_pre + X(s)) / decay^(Tl - s)):
    the exact metric inside each tile's range enters as Q40-rounded float64 products (<= 2^-41 each, carried back by
    1 / decay^(Tl - s): helpers.q40_bound, 1.0e-6 at alpha = 0.005), the pre-selection outside it as float32 sums of
    values in [-1, theta) (<= 24 ulps of 2^-24 in all, relative to 1).  A float64 recurrence over those same samples
    must therefore agree to tol * (1 + |avg|), tol = q40_bound(alpha) + 24 * 2^-24 <= 2.4e-6."""
    x = _capture(orc, geom, snr, None)
    for rise, fall in DETECTOR_RISE_FALL:
        c = _case(orc, x, geom, alpha, rise, fall)
        assert len(c["rows"]) >= 4                   # (a run per preamble at least)
        _check_against_float64(c, alpha)


@pytest.mark.parametrize("geom,snr,alpha", GRID)
def test_run_start_average_against_the_blocks_recurrence(orc, geom, snr, alpha):
    """(b) Against gr_peak_detector_fb's own semantics: float64 recurrence over the exact metric everywhere.  The average
    is an alpha-weighted mean (weights sum below 1), so it moves by at most the largest pre-selection error of the
    samples outside the ranges: |tap - ref| <= tol_a * (1 + |ref|) + PRESEL_OUT, PRESEL_OUT = 1.5e-5 (the figure the
    literal-recurrence test's float32 accuracy implies away from the exactly evaluated, ill-conditioned tiles; asserted
    here as the premise)."""
    x = _capture(orc, geom, snr, None)
    for rise, fall in DETECTOR_RISE_FALL:
        c = _case(orc, x, geom, alpha, rise, fall)
        v = npm.detector_input(c["u"], c["u32"], c["ranges"])
        assert np.abs(v - c["u"].astype(np.float64)).max() <= PRESEL_OUT
        rows = c["rows"]
        ref = c["avg_u"][rows[:, 0].astype(np.int64)]
        assert np.all(np.abs(rows[:, 1] - ref) <= run_avg_tolerance(alpha) * (1.0 + np.abs(ref)) + PRESEL_OUT)


@pytest.mark.parametrize("geom,snr,alpha", GRID)
def test_flags_differ_only_on_marginal_runs(orc, geom, snr, alpha):
    """(c) Flags with an explicit marginal rule: normative (TAP_RX_PEAKS), literal float32 (ORC_TAP_PEAKS_GR) and
    float64 (np_model.peak_detect_margins) may disagree only on a run whose float64 margin -- the smallest
    |u - avg*factor| / (1 + |avg|) over its comparisons -- is below 1e-5; every other flag is the same in all three."""
    x = _capture(orc, geom, snr, None)
    for rise, fall in DETECTOR_RISE_FALL:
        _check_flags(_case(orc, x, geom, alpha, rise, fall))


@pytest.mark.parametrize("alpha", DETECTOR_ALPHAS)
def test_designed_captures(orc, alpha):
    """(a) and (c) where the Q40 bound is worst -- a burst starting 200 samples after a tile boundary (lead = 2 tiles
    + 200) -- and on a noise-only stream of 16 tiles at N = 64 where every run comes from the noise."""
    geom = (512, 200, 128)
    x = _capture(orc, geom, 30.0, 2 * 2048 + 200)
    for rise, fall in DETECTOR_RISE_FALL:
        c = _case(orc, x, geom, alpha, rise, fall)
        assert c["rows"][0, 0] // 2048 == 2          # the first run starts in the burst's first tile
        _check_against_float64(c, alpha)
        _check_flags(c)
    x = noise_capture(orc)
    c = _case(orc, x, (64, 48, 16), alpha, 0.8, 0.6)
    assert len(c["rows"]) >= 3
    _check_against_float64(c, alpha)
    _check_flags(c)


@pytest.mark.parametrize("alpha", [0.0, -0.001, 0.0051, 0.01, 0.25, float("nan")])
def test_oracle_refuses_alpha_outside_range(orc, alpha):
    """(d) The accepted range is (0, 0.005]: no capture can compare engine and oracle outside it."""
    cfg = make_cfg("qpsk")
    cfg.peak_alpha = alpha
    with pytest.raises(ValueError):
        orc.rx(cfg, np.zeros(4096, np.complex64))


@pytest.mark.parametrize("alpha", [0.005, 1e-6])
def test_oracle_accepts_alpha_in_range(orc, alpha):
    cfg = make_cfg("qpsk")
    cfg.peak_alpha = alpha
    x = _capture(orc, (512, 200, 128), 30.0, None)
    r = orc.rx(cfg, x, 1 << _abi.TAP_RX_RUN_AVG)
    assert r.tap(_abi.TAP_RX_RUN_AVG).shape[1] == 2 and len(r.tap(_abi.TAP_RX_RUN_AVG)) >= 4


def test_engine_refuses_alpha_outside_range_without_a_gpu():
    """ofdm_create checks the configuration before it touches a device."""
    from ofdm_uhd_amd import engine
    for alpha in (0.0, -0.001, 0.0051, 0.01, 0.25, float("nan")):
        cfg = make_cfg("qpsk")
        cfg.peak_alpha = alpha
        with pytest.raises(ValueError, match="alpha"):
            engine.Engine(cfg=cfg)
