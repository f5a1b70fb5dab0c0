"""Captures whose ends, starts and flag positions sit on the receiver's own grids and inequalities, shared by
test_capture_edges_host.py (oracle against the float64 model on every case) and test_gpu_capture_edges.py (engine against
oracle on every case).

Every other receive test feeds a comfortable capture: lead = 2N, tail = L + 2N.  Here a base capture per geometry
(orc.tx + orc.channel, 30 dB, 0.05 bins, 2 .. 3 packets of 60 .. 300 bytes) is cut, started late or shifted so that

  END    it ends at length e around the last packet's flag p and around every step of the sampler's acceptance test
         b + L + N < nsamples and of its symbol count (ns - p - 2) / L (csrc/rx_demod.h k_frames / sampler_K);
  SHORT  it is shorter than a correlator delay, a symbol, the sampler's first window, the channel filter's taps, one
         overlap-save block, one 2048-sample tile -- once opening with a preamble, once noise alone;
  FRONT  it starts at offset s inside the lead-in, the first preamble's prefix and body, and around the first flag;
  GRID   the last packet's flag, or the capture's end, falls on a boundary of the 2048-sample tile or of the 32-tile
         segment (sample 65536) of k_sync.

Builders return lists of (id, cfg, x), every x read-only; the oracle's result per case is computed once (reference) and
shared.  The module asserts its own conditions: the positions it aims at are reached, and an END sweep takes every
outcome class of OUTCOMES.  No GPU and no engine here; the oracle comes in as the `orc` fixture."""
import collections

import numpy as np

from helpers import make_cfg, make_payloads
from ofdm_uhd_amd import _abi, iqio

Geom = collections.namedtuple("Geom", "mod N occ CP sizes snr seed")
GEOMS = collections.OrderedDict([
    ("qpsk-64", Geom("qpsk", 64, 48, 16, (60, 100, 60), 30.0, 5)),           # the workhorse: ~2 000 samples
    ("qpsk-128", Geom("qpsk", 128, 64, 32, (120, 60, 90), 30.0, 2)),
    ("qpsk-512", Geom("qpsk", 512, 200, 128, (300, 150), 30.0, 3)),
    ("qam16-2048", Geom("qam16", 2048, 1200, 512, (300, 200), 30.0, 4)),     # multi-wave frames: END only
])
# (The seeds are chosen for conditioning of the REFERENCE pair, oracle against float64 model, never by what the engine
#  does: where a burst ends the window energy collapses and the metric amplifies the float32 rounding of the oracle's
#  FFT filter, at N = 64 up to the bound of test_oracle.py itself -- over the 800 cuts of the sweeps about one channel
#  seed in four keeps every cut under it, the others exceed it by up to 3x in a handful of cuts.  model_margin() is the
#  measure; test_capture_edges_host.py holds every case to the bound.)
SWEEP = "qpsk-64"                                   # every e / every s
SUBSET = ("qpsk-128", "qpsk-512")                   # structured subsets of END / FRONT; SHORT
CFO_BINS = 0.05
TILE, SEGMENT = 2048, 32 * 2048                     # SYNC_TILE and the 32-tile segment of csrc/rx_sync.h
RX_TAPS = (_abi.TAP_RX_CHAN_FILT, _abi.TAP_RX_METRIC, _abi.TAP_RX_PRESEL, _abi.TAP_RX_FFT, _abi.TAP_RX_ACQ,
           _abi.TAP_RX_SINK, _abi.TAP_RX_PACKETS)       # = test_gpu_parity.RX_TAPS
_MASK = sum(1 << t for t in RX_TAPS)

# what an END sweep must pass through, from the shortest capture to the full one (classify())
# "flag-refused" (the flag raised, its frame not accepted: peaks > frames) lies between the first two where it occurs at
# all.  The detector raises a flag some tens of samples behind p, and by then the sampler's window, which the frame
# before left ending at or behind p, is usually complete: the last packet's own flag is refused at 512/200/128 only.
# Everywhere the flag that the burst's end triggers is raised and refused at some length; classify() reports any such
# flag as `refused`.
OUTCOMES = ("flag-lost", "header-incomplete", "payload-short", "complete")

_CFG, _BASE, _CASES, _REF = {}, {}, {}, {}


def cfg_of(geom):
    if geom not in _CFG:
        g = GEOMS[geom]
        _CFG[geom] = make_cfg(g.mod, g.N, g.occ, g.CP)
    return _CFG[geom]


def payloads(geom):
    g = GEOMS[geom]
    return make_payloads(len(g.sizes), g.sizes, seed=g.seed)


def filter_grid(orc, cfg):
    """(ntaps, F, B): the channel filter's taps, transform length and overlap-save block."""
    nt = int(cfg.ntaps)
    F = orc.filter_fft_len(nt)
    return nt, F, F - nt + 1


def capture(orc, geom, lead=None, tail=None, seed=None, npkt=None):
    """helpers.loopback_stream with the geometry's payloads and seed (a copy: the channel's seed is an argument here)."""
    g, cfg = GEOMS[geom], cfg_of(geom)
    N, L = g.N, g.N + g.CP
    lead = 2 * N if lead is None else lead
    tail = L + 2 * N if tail is None else tail
    pay = payloads(geom)[:npkt]
    x = orc.tx(cfg, pay, lead=lead, tail=tail)
    core = x[lead:len(x) - tail] if tail else x[lead:]
    sigma = float(np.sqrt(float(np.mean(np.abs(core) ** 2)) / 10 ** (g.snr / 10.0)))
    orc.channel(x, sigma=sigma, cfo=CFO_BINS * 2 * np.pi / N, seed=0xC0FFEE + (g.seed if seed is None else seed))
    return x


def packet_starts(orc, geom, lead, npkt=None):
    """First sample of every packet's preamble (its cyclic prefix) in capture(..., lead=lead)."""
    g, cfg = GEOMS[geom], cfg_of(geom)
    out, at = [], lead
    for p in payloads(geom)[:npkt]:
        out.append(at)
        at += len(orc.tx(cfg, [p]))
    return out


def flag_of(peaks, start, g, ntaps):
    """The flag of the packet whose preamble starts at `start`: the plateau ends with the preamble (start + L - 1) as
    the channel filter delays it ((ntaps - 1) / 2), the first data symbol drags the flag by a few samples; it is the one
    flag within a prefix of that sample."""
    want = start + g.N + g.CP - 1 + (ntaps - 1) // 2
    near = [int(p) for p in peaks if abs(int(p) - want) <= g.CP]
    assert len(near) == 1, (start, want, list(peaks))
    return near[0]


Base = collections.namedtuple("Base", "cfg x lead peaks frames first last K packets")


def base(orc, geom):
    """The geometry's full capture and what the oracle finds in it: first / last = flags of the first and last packet,
    K = data symbols of the last packet's frame."""
    if geom not in _BASE:
        g = GEOMS[geom]
        lead = 2 * g.N
        x = capture(orc, geom)
        x.setflags(write=False)
        r = orc.rx(cfg_of(geom), x, 0)
        peaks = r.tap(_abi.TAP_RX_PEAKS).tolist()
        frames = [tuple(int(v) for v in f) for f in r.tap(_abi.TAP_RX_FRAMES)]
        starts = packet_starts(orc, geom, lead)
        first, last = (flag_of(peaks, s, g, int(cfg_of(geom).ntaps)) for s in (starts[0], starts[-1]))
        K = dict(frames)[last]
        # the full capture is sound: the last packet's header parses and its payload comes back
        assert K >= 1 and r.packets and r.packets[-1] == (True, payloads(geom)[-1]), (geom, frames, r.packets)
        _BASE[geom] = Base(cfg_of(geom), x, lead, peaks, frames, first, last, K, list(r.packets))
        r.close()
    return _BASE[geom]


def model_margin(orc, cfg, x):
    """Largest |oracle metric - float64 metric| over the bound test_oracle.py allows it, 1e-5 (1 + M-bar)."""
    import np_model as npm
    if len(x) == 0:
        return 0.0
    r = orc.rx(cfg, x, 1 << _abi.TAP_RX_METRIC)
    uo = r.tap(_abi.TAP_RX_METRIC).astype(np.float64)
    r.close()
    u = npm.sync_metric(cfg, npm.chan_filter(cfg, x))[0]
    return float(np.max(np.abs(uo - u) / (1e-5 * (2.0 + u))))


def _case(cid, cfg, x):
    x = np.ascontiguousarray(x, np.complex64)
    x.setflags(write=False)
    return (cid, cfg, x)


def accepted_from(orc, geom):
    """e*: the shortest length at which the oracle's sampler accepts the last packet's frame.  Acceptance is monotone
    in the length (b + L + N < nsamples), so bisection finds it; both sides of the step are asserted."""
    b = base(orc, geom)
    L = GEOMS[geom].N + GEOMS[geom].CP

    def acc(e):
        r = orc.rx(b.cfg, b.x[:e], 0)
        got = b.last in [int(f[0]) for f in r.tap(_abi.TAP_RX_FRAMES)]
        r.close()
        return got
    lo, hi = b.last, min(len(b.x), b.last + 3 * L + 2)
    assert not acc(lo) and acc(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if acc(mid) else (mid, hi)
    return hi


def end_lengths(orc, geom):
    b = base(orc, geom)
    L = GEOMS[geom].N + GEOMS[geom].CP
    if geom == SWEEP:
        return list(range(b.last - 2, b.last + (b.K + 2) * L + 3))
    es = accepted_from(orc, geom)
    out = {b.last + d for d in (-1, 0, 1)} | {es + d for d in (-1, 0, 1)}
    for k in range(0, b.K + 2):
        out |= {b.last + 2 + k * L + d for d in (-1, 0, 1)}
    return sorted(e for e in out if 0 <= e <= len(b.x))


def end_cases(orc, geom):
    """The base capture cut to every length of end_lengths."""
    key = ("end", geom)
    if key not in _CASES:
        b = base(orc, geom)
        assert end_lengths(orc, geom)[-1] <= len(b.x)
        _CASES[key] = [_case("end-%s-e%d" % (geom, e), b.cfg, b.x[:e]) for e in end_lengths(orc, geom)]
    return _CASES[key]


def short_lengths(orc, geom):
    g, cfg = GEOMS[geom], cfg_of(geom)
    N, L, D = g.N, g.N + g.CP, g.N // 2
    nt, F, B = filter_grid(orc, cfg)
    out = set(range(0, 9)) | {D - 1, D, D + 1, N - 1, N, N + 1, L + N - 1, L + N, L + N + 1, L + N + 2, nt - 1, nt,
                              B - 1, B, B + 1, F, TILE - 1, TILE, TILE + 1}
    return sorted(n for n in out if n >= 0)


def short_cases(orc, geom):
    """Captures of short_lengths samples: the start of a capture that opens with a preamble (lead = 0), and noise."""
    key = ("short", geom)
    if key not in _CASES:
        cfg = cfg_of(geom)
        sig = capture(orc, geom, lead=0, tail=TILE + 1)
        noise = np.zeros(TILE + 1, np.complex64)
        orc.channel(noise, sigma=0.05, seed=GEOMS[geom].seed + 40)
        assert len(sig) >= TILE + 1
        out = []
        for n in short_lengths(orc, geom):
            out.append(_case("short-%s-sig-n%d" % (geom, n), cfg, sig[:n]))
            out.append(_case("short-%s-noise-n%d" % (geom, n), cfg, noise[:n]))
        _CASES[key] = out
    return _CASES[key]


def front_offsets(orc, geom):
    b, g = base(orc, geom), GEOMS[geom]
    if geom == SWEEP:
        return list(range(b.lead - 3, b.first + 4))
    return sorted({b.lead, b.lead + g.CP - 1, b.lead + g.CP, b.lead + g.CP + g.N // 2, b.first - 1, b.first, b.first + 1})


def front_cases(orc, geom):
    """The base capture from offset s on."""
    key = ("front", geom)
    if key not in _CASES:
        b = base(orc, geom)
        _CASES[key] = [_case("front-%s-s%d" % (geom, s), b.cfg, b.x[s:]) for s in front_offsets(orc, geom)]
    return _CASES[key]


# ---- GRID: flags and capture ends on the tile and segment boundaries --------------------------------------------------
def _run_of(orc, cfg, x, p):
    """First and last sample of the run u > theta = -max(rise, fall) that holds flag p (the plateau)."""
    r = orc.rx(cfg, x, 1 << _abi.TAP_RX_METRIC)
    u = r.tap(_abi.TAP_RX_METRIC)
    r.close()
    theta = -max(np.float32(cfg.peak_rise), np.float32(cfg.peak_fall))
    a = z = p
    while a > 0 and u[a - 1] > theta:
        a -= 1
    while z + 1 < len(u) and u[z + 1] > theta:
        z += 1
    return a, z


def flag_at(orc, geom, target, npkt=2):
    """(x, lead): a capture of npkt packets whose last packet's flag is sample `target`.  The flag follows the lead one
    for one except for the noise under the plateau, which moves with it: a few corrections reach the target, over a few
    channel seeds if need be (and past the seeds whose burst end is ill-conditioned for the reference pair).  The position is asserted."""
    g, cfg = GEOMS[geom], cfg_of(geom)
    b = base(orc, geom)
    rel = packet_starts(orc, geom, 0, npkt)[-1]
    guess = target - (b.last - packet_starts(orc, geom, b.lead)[-1]) - rel
    for seed in range(100, 116):
        lead = guess
        for _ in range(6):
            x = capture(orc, geom, lead=lead, seed=seed, npkt=npkt)
            r = orc.rx(cfg, x, 0)
            p = flag_of(r.tap(_abi.TAP_RX_PEAKS).tolist(), lead + rel, g, int(cfg.ntaps))
            r.close()
            if p == target:
                if model_margin(orc, cfg, x) > 0.5:
                    break                       # ill-conditioned where the burst ends (see GEOMS): the next seed
                return x, lead
            lead += target - p
    raise AssertionError("no lead puts the flag of %s at %d" % (geom, target))


def grid_cases(orc):
    """64/48/16: the last packet's flag at 2047 / 2048 / 2049 and at 65535 / 65536 / 65537, its whole plateau across each
    of the two boundaries, and total lengths 2048 m + d, 65536 + d."""
    key = ("grid",)
    if key not in _CASES:
        geom = SWEEP
        cfg = cfg_of(geom)
        out = []
        for bound in (TILE, SEGMENT):
            for d in (-1, 0, 1):
                x, _ = flag_at(orc, geom, bound + d)
                out.append(_case("grid-flag-%d" % (bound + d), cfg, x))
            # the plateau astride the boundary: the run begins before it, the flag (the run's maximum, near its end) lies
            # behind it
            x, _ = flag_at(orc, geom, bound + 4)
            a, z = _run_of(orc, cfg, x, bound + 4)
            assert a < bound - 1 and z > bound, (bound, a, z)
            out.append(_case("grid-plateau-%d" % bound, cfg, x))
            if bound == SEGMENT:
                long = x
        short = base(orc, geom).x
        assert len(short) > TILE + 1 and len(long) > SEGMENT + 1
        for d in (-1, 0, 1):
            out.append(_case("grid-len-%d" % (TILE + d), cfg, short[:TILE + d]))
            for m in (2, 31):
                out.append(_case("grid-len-%d" % (m * TILE + d), cfg, long[:m * TILE + d]))
            out.append(_case("grid-len-%d" % (SEGMENT + d), cfg, long[:SEGMENT + d]))
        _CASES[key] = out
    return _CASES[key]


# ---- the families as the tests address them ---------------------------------------------------------------------------
FAMILIES = collections.OrderedDict(
    [("end-" + g, lambda orc, g=g: end_cases(orc, g)) for g in GEOMS] +
    [("short-" + g, lambda orc, g=g: short_cases(orc, g)) for g in (SWEEP,) + SUBSET] +
    [("front-" + g, lambda orc, g=g: front_cases(orc, g)) for g in (SWEEP,) + SUBSET] +
    [("grid", grid_cases)])
EXHAUSTIVE = ("end-" + SWEEP, "front-" + SWEEP)             # the sweeps; every other family is a structured subset
STRUCTURED = tuple(f for f in FAMILIES if f not in EXHAUSTIVE and f != "end-qam16-2048")
NCHUNKS = 8                                                 # the sweeps are run in this many parametrised pieces


def geom_of(family):
    return SWEEP if family == "grid" else family.split("-", 1)[1]


def cases(orc, family):
    return FAMILIES[family](orc)


def chunk(orc, family, i):
    """Piece i of NCHUNKS of a sweep, in order."""
    cs = cases(orc, family)
    n = -(-len(cs) // NCHUNKS)
    return cs[i * n:(i + 1) * n]


def as_sc16(case):
    """The case quantised to 16 bits (iqio.to_sc16, default scale): what the engine's sc16 input takes; reference() gives
    the oracle the same values (iqio.from_sc16)."""
    cid, cfg, x = case
    q = iqio.to_sc16(x)
    q.setflags(write=False)
    return (cid + "-sc16", cfg, q)


def samples(case):
    """The case's samples as complex64, whatever its format."""
    x = case[2]
    return iqio.from_sc16(x) if x.dtype == np.int16 else x


SC16 = tuple("short-" + g for g in (SWEEP,) + SUBSET) + tuple("end-" + g for g in SUBSET)


def sc16_cases(orc, family):
    key = ("sc16", family)
    if key not in _CASES:
        _CASES[key] = [as_sc16(c) for c in cases(orc, family)]
    return _CASES[key]


def reference(orc, case, taps=True):
    """The oracle's result on the case (with the taps of test_gpu_parity._check_rx, or none), computed once."""
    cid, cfg, x = case
    key = (cid, bool(taps))
    if key not in _REF:
        _REF[key] = orc.rx(cfg, samples(case), _MASK if taps else 0)
    return _REF[key]


_POS = {}


def packet_positions(case):
    """The flag every delivered packet belongs to, from the float64 model (the oracle does not report it;
    test_capture_edges_host.py holds the model's flags, frames and packets equal to the oracle's on every case)."""
    import np_model as npm
    if case[0] not in _POS:
        _POS[case[0]] = [int(p) for p in npm.rx(case[1], samples(case))["pos"]]
    return _POS[case[0]]


def release(case):
    """Drops the cached results of a case (the sweeps hold hundreds)."""
    for t in (False, True):
        r = _REF.pop((case[0], t), None)
        if r is not None:
            r.close()


def classify(orc, geom, ro):
    """Outcome of an END case, from the oracle's result: (what became of the last packet, K of its frame, refused).
    refused: the capture ends with a flag the detector raised and the sampler never reached (peaks > frames)."""
    b = base(orc, geom)
    peaks = ro.tap(_abi.TAP_RX_PEAKS).tolist()
    frames = dict((int(f[0]), int(f[1])) for f in ro.tap(_abi.TAP_RX_FRAMES))
    refused = ro.stats["peaks"] > ro.stats["frames"]
    assert set(frames) <= set(peaks) and (not refused or peaks[-1] not in frames)
    if b.last not in peaks:
        return "flag-lost", None, refused
    if b.last not in frames:
        return "flag-refused", None, refused
    K = frames[b.last]
    if ro.stats["headers_ok"] < len(b.packets):
        return "header-incomplete", K, refused
    if len(ro.packets) < len(b.packets):
        return "payload-short", K, refused
    assert ro.packets == b.packets
    return "complete", K, refused


def end_outcomes(orc, geom):
    """[(e, outcome, K, refused)] over the geometry's END cases; asserts that the lengths pass through the classes of
    OUTCOMES in order, take every K from 0 to the full frame's -- 'payload-short' up to one symbol short of it -- and, in
    the sweep, that some length leaves a raised flag without a frame."""
    b = base(orc, geom)
    assert len(b.packets) == len(GEOMS[geom].sizes)            # (so headers_ok / packets count the last packet's)
    rows = []
    for c in end_cases(orc, geom):
        rows.append((len(c[2]),) + classify(orc, geom, reference(orc, c, taps=False)))
    seen = [r[1] for r in rows if r[1] != "flag-refused"]
    assert all(r[3] for r in rows if r[1] == "flag-refused")
    # (a frame of one data symbol -- N = 2048 -- goes from header-incomplete straight to complete)
    want = [o for o in OUTCOMES if o != "payload-short" or b.K > 1]
    assert [o for i, o in enumerate(seen) if i == 0 or seen[i - 1] != o] == want, (geom, sorted(set(seen)))
    assert sorted({r[2] for r in rows if r[2] is not None}) == list(range(0, b.K + 1)), geom
    assert b.K == 1 or any(r[1] == "payload-short" and r[2] == b.K - 1 for r in rows)
    assert geom != SWEEP or any(r[3] for r in rows)
    return rows
