"""What the captures of slicer_cases.py hold, and the engine's three slicer rules against the full search -- on the CPU.

1.  test_gpu_slicer.py compares engine and oracle on these captures; that comparison pins a fall-through only if the
capture sends points through it.  The populations below are conditions on the captures (counted by slicer_cases.classify
on the oracle's sink tap), with floors well under what the seeds give:

    row          points   sign path   inside eps   beyond 8 levels
    bpsk-128       7006      6572         53            381         (the exact two-point table: see impaired_capture)
    qpsk-512       7326      5503        193           1630
    qpsk-64        9522      8960         16            546
    row          points   in table   outside outer level   near a midpoint   beyond 64 amax
    qam16-256      3776     2428          1247                  140               101
    qam64-128      2538     1825           659                  107                54
    qam256-64      2438     2031           348                   67                59
    qam256-512     2772     2333           338                  211               101
    qam16-2048    10782     6240          4069                 1241               473
    8psk-256       4838 points, all through the full search

The 10 % floor on points outside the outermost level holds for every grid row (12 % to 38 %).

2.  The engine's rules restated in float32 NumPy (slicer_cases.engine_rule: the sign rule with its eps and bound tests,
the grid rule's ka / kb, four candidates and lowest-index tie-break, the fall-throughs) against the float32 full search,
first minimum (slicer_cases.full_search = the oracle's sink_slicer), over every sink point of every row and over points
no capture can place: signed zeros, parts exactly on a level, on a midpoint, on eps, on either bound, one ulp either
side of each, and the corners outside the table.  engine.hip argues for its constants in comments; this is the check."""
import numpy as np
import pytest

import slicer_cases as sc
from helpers import make_cfg
from ofdm_uhd_amd import _abi

F32 = np.float32


def _points(ro):
    x = ro.tap(_abi.TAP_RX_SINK).ravel()
    return x[(x.real != 0) | (x.imag != 0)]


@pytest.mark.parametrize("r", sc.ROWS, ids=sc.IDS)
def test_class_populations(orc, r):
    cfg, x, pay, ro = sc.reference(orc, r)
    c = sc.classify(cfg, ro.tap(_abi.TAP_RX_SINK))
    print(sc.IDS[sc.ROWS.index(r)], c, [ok for ok, _ in ro.packets])
    assert c["nonfinite"] == 0
    oks = [ok for ok, _ in ro.packets]
    assert any(oks) and not all(oks)
    assert any(len(p) > 0 for ok, p in ro.packets if not ok)         # a failed packet with bytes to compare
    s = sc.slicer_of(cfg)
    if r.mod in ("bpsk", "qpsk"):
        assert s.sign_kind == (1 if r.mod == "bpsk" else 2)
        assert c["sign_eps"] >= 10 and c["sign_beyond"] >= 30 and c["sign"] >= 1000
        assert c["full"] == c["sign_eps"] + c["sign_beyond"]
    elif r.mod == "8psk":
        assert s.sign_kind == 0 and not s.grid
        assert c["full"] == c["n"] >= 1000
    else:
        assert s.grid and s.idx.shape == {"qam16": (4, 4), "qam64": (8, 8), "qam256": (16, 16)}[r.mod]
        assert c["grid_beyond"] >= 30 and c["grid_midpoint"] >= 10
        assert c["grid_outside"] >= 0.10 * c["n"]
        assert c["grid_inside"] + c["grid_outside"] + c["grid_beyond"] == c["n"]


def _ulps(v):
    v = F32(v)
    return [np.nextafter(v, F32(-np.inf)), v, np.nextafter(v, F32(np.inf))]


def synthesized(s):
    """Every pair of the parts listed in the module docstring."""
    parts = [F32(0.0), F32(-0.0)]
    lv = sorted(set(np.concatenate([s.pos.real, s.pos.imag]).tolist()))
    mids = [F32(0.5) * (F32(a) + F32(b)) for a, b in zip(lv[:-1], lv[1:])]
    marks = list(lv) + mids
    if s.sign_kind:
        marks += [s.sign_eps, -s.sign_eps, s.sign_bound, -s.sign_bound]
    if s.grid:
        marks += [s.bound, -s.bound]
    amax = max(abs(v) for v in lv)
    # the corners outside the table, near and far, and the smallest and largest finite magnitudes
    marks += [sgn * f * amax for sgn in (-1.0, 1.0) for f in (1.5, 7.0, 63.0, 1000.0)]
    marks += [1e-30, -1e-30, 3e38, -3e38]
    for m in marks:
        parts += _ulps(m)
    parts = np.array(sorted(set(float(p) for p in parts)) + [-0.0], F32)      # (set() folds -0.0 into 0.0)
    re, im = np.meshgrid(parts, parts, indexing="ij")
    return (re.ravel() + 1j * im.ravel()).astype(np.complex64)


def _tables():
    out = {}
    for mod in ("bpsk", "qpsk", "8psk", "qam16", "qam64", "qam256"):
        cfg = make_cfg(mod, 512, 200, 128)
        out[mod] = sc.slicer_of(cfg)
        if mod == "bpsk":
            cfg.constellation[1].im = 0.0
            out["bpsk-exact"] = sc.slicer_of(cfg)
    return out


def test_stock_tables_take_the_expected_rule():
    t = _tables()
    assert t["bpsk"].sign_kind == 0 and not t["bpsk"].grid       # (-1 + 1.2e-16j: not a sign table for ofdm_create)
    assert t["bpsk-exact"].sign_kind == 1
    assert t["qpsk"].sign_kind == 2 and not t["qpsk"].grid
    assert t["8psk"].sign_kind == 0 and not t["8psk"].grid
    for mod in ("qam16", "qam64", "qam256"):
        assert t[mod].sign_kind == 0 and t[mod].grid


@pytest.mark.parametrize("r", sc.ROWS, ids=sc.IDS)
def test_rule_equals_full_search_on_captures(orc, r):
    cfg, x, pay, ro = sc.reference(orc, r)
    s, pts = sc.slicer_of(cfg), _points(ro)
    want = sc.full_search(s, pts)
    bad = np.flatnonzero(sc.engine_rule(s, pts) != want)
    assert len(bad) == 0, (pts[bad[:8]], want[bad[:8]])


@pytest.mark.parametrize("name", ["bpsk", "bpsk-exact", "qpsk", "8psk", "qam16", "qam64", "qam256"])
def test_rule_equals_full_search_on_synthesized_points(name):
    s = _tables()[name]
    pts = synthesized(s)
    path = sc.paths(s, pts)
    want = sc.full_search(s, pts)
    bad = np.flatnonzero(sc.engine_rule(s, pts) != want)
    assert len(bad) == 0, (len(bad), pts[bad[:8]], want[bad[:8]], path[bad[:8]])
    # the points do enter each rule the table has, and leave it through each fall-through
    if s.sign_kind:
        assert (path == 1).any() and (path == 0).any()
    if s.grid:
        assert (path == 2).any() and (path == 0).any()


@pytest.mark.parametrize("name", ["bpsk-exact", "qpsk", "qam16", "qam64", "qam256"])
def test_the_statement_can_fail(name):
    """The comparison is not vacuous.  With the bound tests gone the rule leaves the full search's answer far outside the
    table, where a step between levels is below the rounding of the distances (all of them equal, or infinite: the
    first entry wins); with the tie-break turned round, on exact midpoints.  (No capture of slicer_cases.ROWS tells
    either mutant from the rule: a part exactly on a float32 midpoint does not come out of a noisy channel, and the
    equaliser's 1e2..1e3 is not far enough.  The synthesized points are what pins them.)"""
    s = _tables()[name]
    pts = synthesized(s)
    want = sc.full_search(s, pts)
    assert (sc.engine_rule(s, pts, bounded=False) != want).any()
    if s.grid:
        assert (sc.engine_rule(s, pts, tie_low=False) != want).any()
