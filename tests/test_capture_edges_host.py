"""The reference side of the capture-edge cases (capture_edge_cases.py): on EVERY case the C oracle and the independent
float64 model (np_model.rx) raise the same flags, accept the same frames with the same symbol counts and deliver the same
packets, and the filtered stream and the metric stay within the bounds of test_oracle.py.  That is what lets
test_gpu_capture_edges.py hold the engine to the oracle with array_equal.  No case is left out: one on which the two
sides disagreed would have to be replaced in capture_edge_cases.py, not waived here.

Also here: the oracle's bit-reproducible atan2 (orc_atan2f, what both sides evaluate for complex_to_arg) against
np.arctan2 in float64, and the results it defines where it differs from libm."""
import numpy as np
import pytest

import capture_edge_cases as cc
import np_model as npm
from ofdm_uhd_amd import _abi


def _against_model(orc, case):
    cid, cfg = case[:2]
    x = cc.samples(case)
    ro = cc.reference(orc, case)
    m = npm.rx(cfg, x)
    y, u = ro.tap(_abi.TAP_RX_CHAN_FILT), ro.tap(_abi.TAP_RX_METRIC).astype(np.float64)
    assert len(y) == len(u) == len(x) == ro.stats["samples"], cid
    if len(x):
        # the bounds of test_oracle.test_rx_matches_numpy_model
        assert np.abs(y - m["y"]).max() < 2e-6, cid
        assert np.all(np.abs(u - m["u"]) <= 1e-5 * (1.0 + (m["u"] + 1.0))), cid
    assert ro.tap(_abi.TAP_RX_PEAKS).tolist() == m["peaks"].tolist(), cid
    assert [tuple(f) for f in ro.tap(_abi.TAP_RX_FRAMES).tolist()] == [tuple(f) for f in m["frames"]], cid
    assert ro.packets == m["packets"], cid
    assert ro.stats["peaks"] == len(m["peaks"]) and ro.stats["frames"] == len(m["frames"]), cid
    assert ro.stats["symbols"] == sum(K + 1 for _, K in m["frames"]) == len(ro.tap(_abi.TAP_RX_FFT)), cid
    assert len(m["pos"]) == len(ro.packets) and set(m["pos"]) <= set(ro.tap(_abi.TAP_RX_PEAKS).tolist()), cid
    assert ro.stats["packets"] == len(ro.packets) and ro.stats["crc_ok"] == sum(ok for ok, _ in ro.packets), cid
    return ro


@pytest.mark.parametrize("i", range(cc.NCHUNKS))
@pytest.mark.parametrize("family", cc.EXHAUSTIVE)
def test_sweep_oracle_equals_model(orc, family, i):
    """Every length of the END sweep and every offset of the FRONT sweep at 64/48/16."""
    for case in cc.chunk(orc, family, i):
        _against_model(orc, case)
        cc.release(case)


@pytest.mark.parametrize("family", cc.STRUCTURED + ("end-qam16-2048",))
def test_structured_oracle_equals_model(orc, family):
    cs = cc.cases(orc, family)
    assert len(cs) >= 7
    for case in cs:
        _against_model(orc, case)


@pytest.mark.parametrize("family", cc.SC16)
def test_sc16_oracle_equals_model(orc, family):
    """The cases the engine also takes as 16-bit samples: both references on the quantised values."""
    for case in cc.sc16_cases(orc, family):
        _against_model(orc, case)


@pytest.mark.parametrize("geom", list(cc.GEOMS))
def test_end_sweep_takes_every_outcome(orc, geom):
    """flag lost -> (flag refused) -> header incomplete -> payload short at every K -> complete, in this order as the
    capture grows, every K from 0 to the full frame's (capture_edge_cases.end_outcomes asserts it); in the sweep each
    K step lies exactly where the sampler's inequality puts it: the frame of flag p has k data symbols from
    e = p + 2 + k L on (p + 1 + k L < nsamples; sampler_K's (ns - p - 2) / L)."""
    rows = cc.end_outcomes(orc, geom)
    b = cc.base(orc, geom)
    L = cc.GEOMS[geom].N + cc.GEOMS[geom].CP
    for e, outcome, K, refused in rows:
        if K is not None:
            assert K == min(b.K, (e - b.last - 2) // L), (e, K)
    if geom == cc.SWEEP:
        first = {}
        for e, outcome, K, refused in rows:
            first.setdefault(K, e)
        assert [first[k] for k in range(1, b.K + 1)] == [b.last + 2 + k * L for k in range(1, b.K + 1)]
        # some lengths leave a flag raised and refused (the one the burst's end triggers, if no other)
        assert any(r for _, _, _, r in rows)


def test_short_captures_have_no_frame_below_the_first_window(orc):
    """The sampler's first call needs L + N + 1 samples: a shorter capture has no frame whatever it holds, and a capture
    of 0 .. 8 samples has neither flag nor frame nor a single metric sample out of place."""
    for geom in (cc.SWEEP,) + cc.SUBSET:
        g = cc.GEOMS[geom]
        for case in cc.short_cases(orc, geom):
            ro = cc.reference(orc, case)
            if len(case[2]) <= g.N + g.CP + g.N:
                assert ro.stats["frames"] == 0 and ro.packets == [], case[0]
            assert len(ro.tap(_abi.TAP_RX_METRIC)) == len(case[2])


def test_grid_positions(orc):
    """The GRID captures put what they name where they name it (the builder asserts the flags; here: the lengths)."""
    for cid, cfg, x in cc.grid_cases(orc):
        kind, what, n = cid.split("-")
        if what == "len":
            assert len(x) == int(n)
        elif what == "flag":
            assert int(n) in cc.reference(orc, (cid, cfg, x)).tap(_abi.TAP_RX_PEAKS).tolist()


# ---- orc_atan2f ------------------------------------------------------------------------------------------------------
# Measured here over the points below: worst |orc_atan2f - arctan2| = 2.67e-7 = 2.24 * 2^-23 (about 3 ulp of a result
# near pi / 2, not the "~2 ulp" the code's comment gives).  The bar is the next whole multiple of 2^-23.
ATAN2_BAR = 3 * 2.0 ** -23


def _atan2f(orc, y, x):
    f = orc.lib().orc_atan2f
    return np.array([f(a, b) for a, b in zip(y.tolist(), x.tolist())], np.float32)


def test_atan2f_against_float64(orc):
    rng = np.random.default_rng(23)
    n = 150000
    parts = []
    for sy in (1, -1):
        for sx in (1, -1):                                      # every quadrant, magnitudes 1e-30 .. 1e30 on both parts
            parts.append((sy * 10.0 ** rng.uniform(-30, 30, n), sx * 10.0 ** rng.uniform(-30, 30, n)))
    y = np.concatenate([p[0] for p in parts]).astype(np.float32)
    x = np.concatenate([p[1] for p in parts]).astype(np.float32)
    # comparable magnitudes (every angle, not only the axes' neighbourhoods) replace a third of the points
    k = len(y) // 3
    th = rng.uniform(-np.pi, np.pi, k)
    r = 10.0 ** rng.uniform(-30, 30, k)
    y[:k], x[:k] = (r * np.sin(th)).astype(np.float32), (r * np.cos(th)).astype(np.float32)
    assert len(y) == 600000
    got = _atan2f(orc, y, x).astype(np.float64)
    want = np.arctan2(y.astype(np.float64), x.astype(np.float64))
    err = np.abs(got - want)
    print("orc_atan2f: worst |error| %.3e = %.2f * 2^-23" % (err.max(), err.max() / 2.0 ** -23))
    assert err.max() <= ATAN2_BAR
    assert ATAN2_BAR <= 4 * 2.0 ** -23


def test_atan2f_edges(orc):
    f = orc.lib().orc_atan2f
    F = np.float32
    big, tiny, sub = float(F(3e38)), float(F(1.2e-38)), float(F(1e-45))
    pi, h = float(F(np.pi)), float(F(np.pi / 2))
    # axes, exactly
    assert f(0.0, 1.0) == 0.0 and f(1.0, 0.0) == h and f(-1.0, 0.0) == -h and f(0.0, -1.0) == pi
    assert f(big, 0.0) == h and f(-sub, 0.0) == -h and f(1.0, -0.0) == h
    # overflow and underflow of y / x: the quotient becomes Inf or 0, the result the axis
    for y, x in ((big, tiny), (big, sub), (1.0, sub), (-big, tiny), (big, -tiny), (-big, -tiny),
                 (tiny, big), (sub, big), (sub, 1.0), (-tiny, big), (tiny, -big), (-tiny, -big), (big, big), (sub, sub),
                 (big, -big), (-sub, sub), (np.inf, 1.0), (-np.inf, -1.0), (1.0, np.inf), (1.0, -np.inf)):
        want = np.arctan2(np.float64(F(y)), np.float64(F(x)))
        assert abs(float(f(y, x)) - want) <= ATAN2_BAR, (y, x)
    # the defined results where libm differs: x == 0 and y == 0 give +0 whatever the signs (libm: +-0 and +-pi); a
    # negative zero y counts as not negative (libm: -pi); Inf / Inf is NaN (libm: pi / 4).  They are what both sides
    # evaluate -- documented here, not to be changed.
    for y in (0.0, -0.0):
        for x in (0.0, -0.0):
            v = f(y, x)
            assert v == 0.0 and not np.signbit(v)
        assert f(y, -1.0) == pi
        v = f(y, 1.0)
        assert v == 0.0 and not np.signbit(v)
    assert np.isnan(f(np.inf, np.inf)) and np.isnan(f(-np.inf, np.inf)) and np.isnan(f(np.nan, 1.0))
