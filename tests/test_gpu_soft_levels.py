"""k_soft_demap (csrc/rx_soft.h) across input level and on captures with a non-finite sample: the captures of
level_cases.py, unchanged, with soft values on.  The reference is the model soft_cases.call_values fed with the same
call's TAP_RX_SINK / TAP_RX_DEMAPPED taps, link-quality records and CSI ``eq`` rows; every comparison is array_equal on
int8, no tolerance anywhere.

The kernel guards against NaN, Inf, overflow and underflow in four places: soft_weight (a carrier whose |eq|^2 is 0 or
not finite weighs 0), the v == v test in front of the clamp, the dead packet (mean weight 0 or not finite: all values
0), and D0 - D1 = Inf - Inf for a slicer input that is not finite.  What a capture reaches of them, found with the
oracle on the CPU before this file was written:

  * uniform levels 2^-18 .. 2^+8 (and 2^+14 for bpsk-64) deliver non-empty packets with mean carrier weights from about
    1e-10 to 1e6 (1.1e9 at 2^+14): the weight, gain and clamp arithmetic far from its nominal range, all of it finite;
  * the "data-symbol" poison delivers a 300-byte packet five of whose slicer rows are not finite in every column: the
    Inf - Inf path and the v == v test, whose values must be 0;
  * from 2^+64 up the receiver delivers empty packets only, and the kernel returns for an empty packet before it forms a
    weight: the packet-wide zero (mean weight 0 or not finite) is not reachable through ofdm_rx at any level of
    level_cases.py; nor is a single carrier's zero weight, which needs |Y| = 0 or above 2^63 at a pilot of a preamble
    the receiver still accepts.  Both stay covered on the model alone, by test_soft_host.py.

Exact scaling: a capture times 2^e (e = -8, -4, +4) whose packet list and slicer inputs are bit-equal to those of e = 0
and whose eq rows are exactly 2^-e times those of e = 0 -- checked on the engine's own outputs -- must give bit-equal
values: every weight is scaled by 2^(2e), so is their mean, the gain by 2^(-2e), and the product w * g is unchanged.
At e = -8 the receiver does not meet that precondition (test_exact_scaling has the reason)."""
import numpy as np
import pytest

import level_cases as lc
import soft_cases as sc
from ofdm_uhd_amd import _abi

pytestmark = pytest.mark.gpu

TAPS = (_abi.TAP_RX_FFT, _abi.TAP_RX_SINK, _abi.TAP_RX_DEMAPPED)
GEOMS = ("bpsk-64", "qam16-256")
UNIFORM = [(g, e) for g in GEOMS for e in (-18, -16, -12, 6, 7, 8)] + [("bpsk-64", 14)]
SCALED = [(g, e) for g in GEOMS for e in (-8, -4, 4)]


@pytest.fixture(scope="module")
def engines():
    """One engine per geometry: taps, link quality, CSI and soft values on."""
    from ofdm_uhd_amd import engine
    made = {}

    def get(geom):
        if geom not in made:
            e = engine.Engine(cfg=lc.cfg_of(geom))
            e.set_taps(*TAPS)
            e.set_rx_quality(True)
            e.set_rx_csi(True)
            e.set_rx_soft(True)
            made[geom] = e
        return made[geom]
    yield get
    for e in made.values():
        e.close()


def _call(eng, cfg, x):
    pk = eng.rx(x)
    recs, eq = eng.rx_quality(), eng.rx_csi()["eq"]
    sink, dem = eng.tap(_abi.TAP_RX_SINK), eng.tap(_abi.TAP_RX_DEMAPPED)
    with np.errstate(all="ignore"):
        want = sc.call_values(cfg, pk, recs, eq, sink, dem)
    return dict(pk=pk, recs=recs, eq=eq, sink=sink, dem=dem, want=want, got=eng.rx_soft())


def _equal(got, want):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == np.int8 and a.shape == b.shape, i
        assert np.array_equal(a, b), (i, len(a), np.flatnonzero(a != b)[:8].tolist())


def _mean_weights(cfg, r):
    smap = sc.smap_of(cfg)
    return [float(sc.mean_weight(sc.weights(eq), smap)) for eq in r["eq"]]


@pytest.mark.parametrize("geom,e", UNIFORM, ids=["%s-e%+d" % c for c in UNIFORM])
def test_uniform_level(orc, engines, geom, e):
    cfg, x, ro = lc.uniform(orc, geom, e)
    r = _call(engines(geom), cfg, x)
    assert r["pk"] == ro.packets
    assert any(len(p) > 0 for _, p in r["pk"])
    _equal(r["got"], r["want"])
    assert [len(v) for v in r["got"]] == [8 * len(p) for _, p in r["pk"]]
    assert all(v.min(initial=0) >= -127 for v in r["got"])
    # not a comparison of zeros: the weights are finite and the CRC-ok packets carry decisions
    w = _mean_weights(cfg, r)
    print("%s e%+d: %d packets, mean weight %.3g .. %.3g" % (geom, e, len(r["pk"]), min(w), max(w)))
    assert all(np.isfinite(v) and v > 0 for v in w)
    assert all(np.count_nonzero(v) > 0.9 * len(v) for (ok, p), v in zip(r["pk"], r["got"]) if ok and len(p))


def _ulps(a, b):
    """Largest distance in float32 steps between two arrays of finite float32 parts of like sign."""
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    return int(np.abs(ia - ib).max(initial=0))


@pytest.mark.parametrize("geom,e", SCALED, ids=["%s-e%+d" % c for c in SCALED])
def test_exact_scaling(orc, engines, geom, e):
    """The precondition is taken packet by packet on the engine's own outputs (its sink rows bit-equal to those of e = 0,
    its eq row exactly 2^-e times that of e = 0), the packet list and the demapped symbols for the whole call; the claim
    -- values bit-equal to those of e = 0 -- is asserted for every packet that meets it.

    At e = +-4 every packet has to meet it: up to the synchroniser everything scales exactly, and its Q23.40 window sums
    (LSB 2^-40, level_cases.py) are about 2^(2e) in size, so what their rounding changes stays below the float32 they
    are converted to as long as 2^-41 / 2^(2e) is well under 2^-25.  At e = -8 it is not (2^-41 / 2^-16 = 2^-25): the
    flag's angle, and with it the NCO and every slicer input, moves by float32 steps.  That is the receiver (DESIGN.md
    section 2, "Input level": the synchroniser is not scale-free), not k_soft_demap.  Measured on an MI355X at e = -8: no
    packet of either geometry meets the precondition; the slicer inputs differ from those of e = 0 by up to 41 float32
    steps at qam16-256 and 107 520 at bpsk-64 (a part next to zero); none of the 1 920 /
    6 400 values differs all the same.  At e = +-4 all four packets of both meet it, and no value differs.  The exponent
    stays in the grid: its packet list is that of e = 0, its values equal the model, and any packet that does meet the
    precondition is held to the claim."""
    cfg, x0, _ = lc.uniform(orc, geom, 0)
    _, x, _ = lc.uniform(orc, geom, e)
    eng = engines(geom)
    a, b = _call(eng, cfg, x0), _call(eng, cfg, x)
    assert b["pk"] == a["pk"] and len(a["pk"]) >= 4, "packet list at e = %+d differs from e = 0" % e
    assert np.array_equal(b["dem"], a["dem"])
    assert np.array_equal(b["recs"]["first_symbol"], a["recs"]["first_symbol"]) and np.array_equal(b["recs"]["nsym"], a["recs"]["nsym"])
    _equal(a["got"], a["want"])
    _equal(b["got"], b["want"])
    assert sum(len(v) for v in a["got"]) > 0
    nmap = len(sc.smap_of(cfg))
    sink_row = np.cumsum(a["dem"].astype(bool)) - 1
    scaled = (a["eq"].astype(np.complex128) * 2.0 ** -e).astype(np.complex64)
    met, worst = 0, 0
    for k, rec in enumerate(a["recs"]):
        fs, ns = int(rec["first_symbol"]), int(rec["nsym"])
        rows = sink_row[fs + 1:fs + 1 + ns]
        sa, sb = a["sink"][rows, :nmap], b["sink"][rows, :nmap]
        same_sink = np.array_equal(sa.view(np.uint32), sb.view(np.uint32))
        same_eq = np.array_equal(b["eq"][k].view(np.uint32), scaled[k].view(np.uint32))
        worst = max(worst, _ulps(sa.view(np.float32), sb.view(np.float32)))
        if same_sink and same_eq:
            met += 1
            assert np.array_equal(b["got"][k], a["got"][k]), k                      # the claim
    differing = sum(int(np.count_nonzero(u != v)) for u, v in zip(a["got"], b["got"]))
    print("%s e%+d: %d of %d packets meet the precondition; slicer inputs differ by up to %d float32 steps, %d of %d values differ" % (
        geom, e, met, len(a["pk"]), worst, differing, sum(len(v) for v in a["got"])))
    if abs(e) <= 4:
        assert met == len(a["pk"]), "sink rows or eq rows at e = %+d do not scale exactly" % e


@pytest.mark.parametrize("value,position", lc.POISON, ids=lc.POISON_IDS)
def test_one_nonfinite_sample(orc, engines, value, position):
    cfg, x, ro, i = lc.poisoned(orc, value, position)
    r = _call(engines("qpsk-512"), cfg, x)
    assert r["pk"] == ro.packets and len(r["pk"]) >= 1
    _equal(r["got"], r["want"])
    assert [len(v) for v in r["got"]] == [8 * len(p) for _, p in r["pk"]]
    if position != "data-symbol":
        return
    # a delivered 300-byte packet holds non-finite slicer rows among its own; every value that comes from them is 0
    smap = sc.smap_of(cfg)
    nmap, nbits = len(smap), int(cfg.arity).bit_length() - 1
    sink_row = np.cumsum(r["dem"].astype(bool)) - 1
    hit = 0
    for (ok, p), rec, v in zip(r["pk"], r["recs"], r["got"]):
        fs, ns = int(rec["first_symbol"]), int(rec["nsym"])
        rows = r["sink"][sink_row[fs + 1:fs + 1 + ns], :nmap]
        bad = ~np.isfinite(rows.view(np.float32).reshape(len(rows), -1)).all(axis=1)
        if len(p) != 300 or not bad.any():
            continue
        hit += 1
        ncar = sc.carriers_needed(len(p), nbits)
        car, bit, idx, mb, e = sc.placement(len(p), nbits, ncar)
        from_bad = bad[car // nmap]
        assert from_bad.any() and not v[idx[from_bad]].any()
        assert np.count_nonzero(v[idx[~from_bad]]) > 0.9 * np.count_nonzero(~from_bad)
    assert hit >= 1
