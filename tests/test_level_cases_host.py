"""The oracle across input level -- on the CPU.  Keeps the table of DESIGN.md section 2, "Input level", true and shows
that every capture of level_cases.py reaches the constant it is for; test_gpu_levels.py then compares the engine with
the oracle on the same captures.

What the oracle does with the loopback captures (4 packets, 30 dB, 0.05 bins; nominal rms 0.13 .. 0.18) times 2^e:

    e <= -20      no timing flag at all (window terms round to nothing in Q23.40: R = 0, M = 0)
    -19           one flag at the most, no header
    -18, -17      flags and headers; CRCs pass raggedly (bpsk-64: 1 of 4 at -18, all at -17; the other two: none)
    -16, -15      every packet CRC-ok, but for one of qam16-256's four at -15
    -14 .. +7     every packet CRC-ok, every geometry, every exponent   (level_cases.WINDOW)
    -11 .. +6     flag positions identical to e = 0                     (level_cases.SAME_FLAGS)
    -16 .. -13    flag positions differ from e = 0; at +7 too for qpsk-512 and bpsk-64, qam16-256 still identical
    +8            every header parses, every CRC fails
    >= +9         flags still rise (4 and more), no packet is recovered

(The issue that asked for this table had measured even exponents only and put the window's low edge at -16; the odd
ones show the edge is ragged between -18 and -14.)

The flags of e = 0 are the high-precision reference inside the window: np_model.sync_metric is float64 with no fixed
point and is exactly invariant under a power of two (checked below, not merely claimed), so what a float64 evaluation
gives at the nominal level is what it gives at every level.

The issue that asked for these cases expected the channel filter's transform to overflow at e = +110.  It does not: a
512-point transform of samples of magnitude 2^110 stays below 2^128.  At +110 (as at +70) it is the correlator's
products that are Inf and Inf - Inf = NaN; the filter overflows at +125, which is therefore a case of its own."""
import numpy as np
import pytest

import level_cases as lc
import np_model
from ofdm_uhd_amd import _abi

F32_MAX = float(np.finfo(np.float32).max)
HOST_ONLY = tuple(e for e in range(-20, 11) if e not in lc.EXPONENTS)     # the table's rows in between
DIFFERENT_FLAGS = {(g, e) for g in lc.SMALL for e in (-16, -15, -14, -13)} | {("qpsk-512", 7), ("bpsk-64", 7)}


def _flags(ro):
    return ro.tap(_abi.TAP_RX_PEAKS).tolist()


def _y(ro):
    return ro.tap(_abi.TAP_RX_CHAN_FILT)


def _metric_ok(ro, n):
    m = ro.tap(_abi.TAP_RX_METRIC)
    assert len(m) == n and np.isfinite(m).all()
    assert -1.0 <= float(m.min()) and float(m.max()) <= 1023.0         # u = mean of M - 1, 0 <= M <= 1024


# ---- the table ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", lc.SMALL)
def test_working_window(orc, geom):
    g, pay = lc.GEOMS[geom], lc.payloads(geom)
    nominal = _flags(lc.uniform(orc, geom, 0)[2])
    assert len(nominal) == g.npkt + 1                                   # one per packet and one in the capture's tail
    for e in sorted(set(lc.EXPONENTS + HOST_ONLY + (0,))):
        cfg, x, ro = lc.uniform(orc, geom, e)
        st, good, fl = ro.stats, lc.ok_payloads(ro), _flags(ro)
        print(geom, e, "flags", len(fl), "headers", st["headers_ok"], "crc_ok", st["crc_ok"], "same flags", fl == nominal)
        _metric_ok(ro, len(x))
        if e <= -20:
            assert fl == [] and ro.packets == []
            assert float(ro.tap(_abi.TAP_RX_METRIC).max()) == -1.0      # R = 0 -> M = 0 on every sample
        if e == -19:
            assert len(fl) <= 1 and st["headers_ok"] == 0
        if e == -18:
            assert len(fl) >= g.npkt and st["headers_ok"] >= 1 and len(good) < g.npkt
        if e == -17:
            assert st["headers_ok"] == g.npkt and len(good) == (g.npkt if geom == "bpsk-64" else 0)
        if lc.WINDOW[0] <= e <= lc.WINDOW[1] or e == -16:
            assert good == pay, e
        if e == -15:
            assert len(good) == (g.npkt - 1 if geom == "qam16-256" else g.npkt)
        if lc.SAME_FLAGS[0] <= e <= lc.SAME_FLAGS[1]:
            assert fl == nominal, e
        if (geom, e) in DIFFERENT_FLAGS:
            assert fl != nominal, e
        if (geom, e) == ("qam16-256", 7):
            assert fl == nominal
        if e == 8:
            assert st["headers_ok"] == g.npkt and st["crc_ok"] == 0 and len(ro.packets) == g.npkt
        if e >= 9:
            assert st["crc_ok"] == 0
            assert len(fl) >= (4 if e <= 110 else 1)                    # (+125: NaN blocks in y, anything from 1 to 36)


def test_float64_metric_is_scale_free(orc):
    """np_model.sync_metric (float64, no fixed point, no clamp but M <= 1024) of y * 2^e is bit for bit that of y: the
    flags of the nominal level are the float64 answer at every level."""
    cfg, x, ro = lc.uniform(orc, "qpsk-512", 0)
    y = _y(ro).astype(np.complex128)
    u0, P0 = np_model.sync_metric(cfg, y)
    assert float(u0.max()) > 0.0
    for e in (-70, -16, 7, 64):
        u, P = np_model.sync_metric(cfg, y * 2.0 ** e)
        assert np.array_equal(u, u0), e
        assert np.array_equal(P, P0 * 4.0 ** e), e


METRIC_CASES = [("qpsk-512", e) for e in (0, -18, -16, 6, 7, 8, 14, 64, 70, 110, 125)] + [
    ("bpsk-64", 7), ("qam16-256", 14), ("qam64-4096", 7), ("qam64-4096", 14)]


@pytest.mark.parametrize("geom,e", METRIC_CASES, ids=["%s-e%+d" % c for c in METRIC_CASES])
def test_metric_restated(orc, geom, e):
    """The oracle's metric tap against level_cases.q40_metric of its own filtered stream, bit for bit: pins the clamp at
    511, the LSB, M's two special cases and -- where products are Inf - Inf -- the rule for a NaN term."""
    cfg, x, ro = lc.uniform(orc, geom, e)
    assert np.array_equal(ro.tap(_abi.TAP_RX_METRIC), lc.q40_metric(cfg, _y(ro)))


def test_4096_row(orc):
    """qam64 4096 / 2400 / 1024: the detector needs more than the 2N lead-in to settle at this size, so the capture's
    first packet is lost at every level; the second is recovered inside the window."""
    pay = lc.payloads("qam64-4096")
    for e in lc.EXPONENTS_4096:
        cfg, x, ro = lc.uniform(orc, "qam64-4096", e)
        print("qam64-4096", e, ro.stats)
        assert 30000 <= len(x) <= 42000
        _metric_ok(ro, len(x))
        assert ro.stats["peaks"] == 2
        assert lc.ok_payloads(ro) == (pay[1:] if e <= lc.WINDOW[1] else [])


# ---- each case reaches what it is for ----------------------------------------------------------------------------------
def _longest_run(mask):
    best = run = 0
    for v in mask.tolist():
        run = run + 1 if v else 0
        best = max(best, run)
    return best


@pytest.mark.parametrize("geom", list(lc.GEOMS))
def test_clamp_reach(orc, geom):
    """|y|^2 > 511 on the filtered stream (the energy term of R as the metric forms it): nowhere up to the nominal level,
    somewhere from +6, on all of the signal at +14 -- at N = 4096 a whole 2048-term window, whose sum 2048 * 511 * 2^40 is
    just under 2^60."""
    g = lc.GEOMS[geom]
    exps = lc.EXPONENTS if geom in lc.SMALL else lc.EXPONENTS_4096
    lead, tail = 2 * g.N, (g.N + g.CP) + 2 * g.N
    for e in exps:
        cfg, x, ro = lc.uniform(orc, geom, e)
        y = _y(ro)
        nc = lc.n_clamped(y)
        print(geom, e, "clamped", nc, "of", len(y))
        if e <= 0:
            assert nc == 0
        if e == 6:
            assert 0 < nc < len(y) // 10
        if e == 7:
            assert nc > len(y) // 10
        if 14 <= e < 125:
            sig = y[lead + g.N:len(y) - tail]
            assert lc.n_clamped(sig) >= 0.999 * len(sig)
            with np.errstate(over="ignore"):
                en = sig.real * sig.real + sig.imag * sig.imag
            assert _longest_run(en > np.float32(511.0)) >= g.N // 2       # a window of nothing but clamped terms


@pytest.mark.parametrize("geom", lc.SMALL)
def test_floor_and_overflow_reach(orc, geom):
    D = lc.GEOMS[geom].N // 2
    for e in (-140, -120):                  # subnormal input, subnormal filtered samples
        cfg, x, ro = lc.uniform(orc, geom, e)
        assert lc.n_subnormal(x) > 0 and lc.n_subnormal(_y(ro)) > 0
        assert lc.n_nonfinite(_y(ro)) == 0
    for e in (-70, -24):                    # normal numbers, every term below half an LSB
        cfg, x, ro = lc.uniform(orc, geom, e)
        y = _y(ro).astype(np.complex128)
        assert lc.n_subnormal(x) == 0 and 0.0 < float((np.abs(y) ** 2).max()) < 2.0 ** -41
    # +64: every term finite, the float32 window sums of the pre-selection overflow
    cfg, x, ro = lc.uniform(orc, geom, 64)
    y = _y(ro)
    en = y.real.astype(np.float64) ** 2 + y.imag.astype(np.float64) ** 2
    assert float(en.max()) < F32_MAX
    cs = np.concatenate([[0.0], np.cumsum(en)])
    assert float((cs[D:] - cs[:-D]).max()) > F32_MAX
    # +70 and +110: |y|^2 itself is Inf in float32 (and the correlator's products Inf - Inf = NaN); y stays finite
    for e in (70, 110):
        cfg, x, ro = lc.uniform(orc, geom, e)
        y = _y(ro)
        with np.errstate(over="ignore"):
            assert np.isinf(y.real * y.real + y.imag * y.imag).any()
        assert lc.n_nonfinite(x) == 0 and lc.n_nonfinite(y) == 0
    # +125: finite input, the filter's transform overflows and makes Inf - Inf = NaN
    cfg, x, ro = lc.uniform(orc, geom, 125)
    assert lc.n_nonfinite(x) == 0 and lc.n_nonfinite(_y(ro)) > 0
    assert np.isnan(_y(ro).view(np.float32)).any()
    for e in (64, 70, 110, 125):
        assert np.isfinite(lc.uniform(orc, geom, e)[2].tap(_abi.TAP_RX_PRESEL)).all()   # M <= 1024 also for NaN


@pytest.mark.parametrize("k,order", lc.STEPS, ids=lc.STEP_IDS)
def test_two_bursts(orc, k, order):
    """Strong burst = packets 0 .. 2, weak burst (2^-k) = packets 3 .. 5.  What the oracle recovers:
        k = 6   strong -> weak: 0 1 2 5      weak -> strong: 3 4 5 1 2
        k = 13  strong -> weak: 0 1 2 4 5    weak -> strong: 3 4 5        (the strong burst is lost behind the step)"""
    cfg, x, ro, pay = lc.step(orc, k, order)
    got = [pay.index(p) for p in lc.ok_payloads(ro)]
    print(k, order, got, ro.stats)
    assert len(x) <= 40000
    _metric_ok(ro, len(x))
    assert got == {(6, "strong-weak"): [0, 1, 2, 5], (6, "weak-strong"): [3, 4, 5, 1, 2],
                   (13, "strong-weak"): [0, 1, 2, 4, 5], (13, "weak-strong"): [3, 4, 5]}[(k, order)]
    if order == "strong-weak":
        assert any(i >= lc.STEP_NPKT for i in got)                      # a packet of the weak burst, behind the step
    # the step is what it says: the bursts' levels are 2^k apart
    half = len(x) // 2
    a, b = (x[:half], x[half:]) if order == "strong-weak" else (x[half:], x[:half])
    ratio = np.sqrt(np.mean(np.abs(a.astype(np.complex128)) ** 2) / np.mean(np.abs(b.astype(np.complex128)) ** 2))
    assert 0.9 * 2.0 ** k < ratio < 1.1 * 2.0 ** k


def test_sc16_capture(orc):
    cfg, q, ro = lc.sc16(orc)
    assert q.dtype == np.int16 and q.shape == (len(lc.base_capture(orc, "qpsk-512")), 2)
    rms = float(np.sqrt(np.mean(q.astype(np.float64) ** 2) * 2.0))
    print("sc16 rms", rms, "peak", int(np.abs(q).max()))
    assert 8.0 < rms < 12.0
    assert lc.ok_payloads(ro) == lc.payloads("qpsk-512")


@pytest.mark.parametrize("value,position", lc.POISON, ids=lc.POISON_IDS)
def test_one_nonfinite_sample(orc, value, position):
    """The call returns, the metric is finite everywhere (a NaN term is -511, M <= 1024 also for NaN), and the poison
    stays inside the filter blocks whose window holds the sample: all 358 outputs of each for NaN / Inf, whole blocks
    (one at least) for 3e38, which overflows only where the transform's sums get large enough."""
    cfg, x, ro, i = lc.poisoned(orc, value, position)
    base = lc.base_capture(orc, "qpsk-512")
    assert lc.n_nonfinite(x) == (0 if value == "3e38" else 1) and np.array_equal(np.delete(x, i), np.delete(base, i))
    _metric_ok(ro, len(x))
    y = _y(ro)
    bad = ~np.isfinite(y.view(np.float32).reshape(-1, 2)).all(axis=1)
    blocks = lc.filter_blocks(cfg, i)
    assert len(blocks) == (1 if position == "lead-in" else 2)           # the other two straddle a block boundary
    inside = np.zeros(len(y), bool)
    hit = 0
    for lo, hi in blocks:
        assert hi - lo + 1 == 358
        inside[lo:hi + 1] = True
        n = int(bad[lo:hi + 1].sum())
        assert n in (0, 358)
        hit += n == 358
    assert not (bad & ~inside).any()
    assert hit == len(blocks) if value != "3e38" else hit >= 1
    y0 = _y(lc.uniform(orc, "qpsk-512", 0)[2])
    assert np.array_equal(y[~inside], y0[~inside])                      # every other block: the clean capture's bits
    assert np.array_equal(ro.tap(_abi.TAP_RX_METRIC), lc.q40_metric(cfg, y))     # a NaN term counts as -511
    print(value, position, i, ro.stats, _flags(ro))
    nominal = _flags(lc.uniform(orc, "qpsk-512", 0)[2])
    if position == "lead-in":                                           # "not cosmetic": it costs the first two packets
        assert lc.ok_payloads(ro) == lc.payloads("qpsk-512")[2:] and _flags(ro)[1:] == nominal[1:]
    else:
        assert 1 <= len(lc.ok_payloads(ro)) < 4
