"""The spectrum sensor's launch geometry and the captures that walk it, shared by test_sense_cases_host.py (the
restated geometry, the oracle against a float64 model, and that every round and every lane of every case decides
something) and test_gpu_sense_geometry.py (engine against oracle).

csrc/engine_sense.inc (sense_enqueue) picks, per call,

    G         = max(1, 256 / (S/8))            transforms side by side in a workgroup
    max_split = ceil(dwell / G)
    nsplit    = max(1, min(max_split, want))   want = ceil(2048 / nmsgs), or OFDM_SENSE_SPLIT
    stride    = nsplit * G
    rounds    = ceil(dwell / stride)           trips of k_sense's software-pipelined loop
    launches  = ceil(nmsgs / 65535)            (p.msg0)

and accrued vector f of a message runs in slot (round, workgroup, group) = (f // stride, (f % stride) // G, f % G).
Without the knob rounds >= 2 needs nmsgs * dwell > 2048 * G, millions of samples at every S; the forced cases set it
and stay small, the two natural cases are that large.

The captures.  Every vector is complex white noise (per-bin power 5e-8 at level 1) and every message gives
min(dwell, S) of its accrued vectors a tone on a bin of their own (2e-5 .. 5e-4, on both sides of the 1e-4 threshold):
such a vector holds the max-hold at its bin whatever the noise does, so a kernel that drops, repeats or misplaces it
changes the message.  With dwell <= S that is every single vector.  S = 64 has fewer bins than the longer dwells have
vectors (and in one row than it has lanes): there the tones go to one vector per lane first, the round rotating with
lane and message, and to the dwell's last vector always (in the 3G + 1 rows it is the last round's only one).  The
tune-delay vectors and the tail behind the last whole message carry a tone a hundred times louder than anything
accrued: reading one of them shows.  The window is a seeded asymmetric one, 0.5 + U(0, 1), unless the case keeps the
default.  No GPU and no engine here; the oracle comes in as the `orc` fixture.  Results are computed once and are
read-only."""
import collections

import numpy as np

from ofdm_uhd_amd import config, iqio

WORKGROUPS_WANTED = 2048        # sense_enqueue: "enough workgroups to fill 256 CUs a few times over"
MAX_GRID_Y = 65535              # messages per launch

Geometry = collections.namedtuple("Geometry", "G nsplit stride rounds launches slots")


def geometry(S, dwell, nmsgs, split=None):
    """sense_enqueue's choice restated; slots[f] = (round, workgroup, group) of accrued vector f."""
    G = max(1, 256 // (S // 8))
    max_split = -(-dwell // G)
    want = -(-WORKGROUPS_WANTED // nmsgs) if split is None else max(1, int(split))
    nsplit = max(1, min(max_split, want))
    stride = nsplit * G
    rounds = -(-dwell // stride)
    f = np.arange(dwell)
    slots = np.stack([f // stride, (f % stride) // G, f % G], axis=1)
    return Geometry(G, nsplit, stride, rounds, -(-nmsgs // MAX_GRID_Y), slots)


def live_groups(geo):
    """[round][workgroup] -> number of live groups."""
    n = np.zeros((geo.rounds, geo.nsplit), np.int64)
    np.add.at(n, (geo.slots[:, 0], geo.slots[:, 1]), 1)
    return n


# ---- the float64 model ---------------------------------------------------------------------------------------------------
def np_sense_powers(sc, iq):
    """|fft(vector * window)|^2 of every accrued vector in float64: [message][accrued vector][bin]."""
    S = sc.fft_size
    w = np.array(sc.window[:S], np.float64)
    per = sc.tune_delay + sc.dwell_delay
    nm = (len(iq) // S) // per
    v = iq[:nm * per * S].astype(np.complex128).reshape(nm, per, S)[:, sc.tune_delay:, :]
    return np.abs(np.fft.fft(v * w, axis=2)) ** 2


def np_sense_msgs(sc, iq):
    """Independent float64 model of the sensor graph."""
    return np_sense_powers(sc, iq).max(axis=1)


def np_sense_decide(sc, msgs):
    """sense_loop's tail on float32 message bodies: float64 sum in message order / avg, threshold, half swap.
    -> mean [ndec][S], bits [ndec][S] (ascending frequency)."""
    S, per = sc.fft_size, sc.avg_msgs + sc.skip_msgs
    nd = len(msgs) // per
    mean, bits = np.zeros((nd, S), np.float64), np.zeros((nd, S), np.uint8)
    for d in range(nd):
        acc = np.zeros(S, np.float64)
        for k in range(sc.avg_msgs):
            acc = acc + msgs[d * per + k].astype(np.float64)
        acc = acc / float(sc.avg_msgs)
        mean[d] = np.concatenate([acc[S // 2:], acc[:S // 2]])
        bits[d] = (mean[d] <= sc.threshold).astype(np.uint8)
    return mean, bits


# ---- the cases -------------------------------------------------------------------------------------------------------------
# window: "seeded" = 0.5 + U(0, 1) from the case's seed, "default" = make_sense_cfg's Blackman-Harris.
# fmt / rx_scale: what the engine is handed ("fc32": complex64; "sc16": iqio.to_sc16 of the same capture at level 2^6).
# last: live groups per workgroup in the last round.
Case = collections.namedtuple("Case", "id S tune dwell avg skip nmsgs split window fmt rx_scale rounds last seed")

SIZES = (64, 128, 256, 512, 1024, 2048, 4096)
AVG_SKIP = ((1, 0), (2, 0), (1, 2), (2, 1))             # k_sense_decide's per = 1, 2, 3, 3
THRESHOLD = 1.0e-4
NOISE_FLOOR = 5.0e-8             # mean noise power per bin at level 1: a tone of 2e-5 keeps its bin at 5 sigma


def _rows(G):
    """(name, split, dwell, rounds, live groups per workgroup in the last round)"""
    q = max(1, G // 4)
    return (("dead-groups", 1, 2 * G + q, 3, (q,)),
            ("one-live-group", 2, 3 * G + 1, 2, (G, 1)),
            ("nothing-dead", 2, 4 * G, 2, (G, G)),
            ("dead-workgroups", 3, 3 * G + 1, 2, (1, 0, 0)))


def _forced():
    out = []
    for si, S in enumerate(SIZES):
        G = max(1, 256 // (S // 8))
        for ri, (name, split, dwell, rounds, last) in enumerate(_rows(G)):
            i = len(out)
            avg, skip = AVG_SKIP[(si + ri) % 4]
            out.append(Case("s%d-%s" % (S, name), S, i % 3, dwell, avg, skip, 3, split, "seeded", "fc32", None, rounds,
                            last, 1000 + i))
    # the benchmark's geometry (BASELINE config 5): one workgroup per message walks the whole dwell
    out.append(Case("s4096-c5-15-rounds", 4096, 2, 15, 1, 0, 2, 1, "seeded", "fc32", None, 15, (1,), 1100))
    return out


FORCED = _forced()
NATURAL = [
    # the default sensor once a capture holds more than 68 messages: nsplit 30, two rounds
    Case("default-70-messages", 256, 24, 244, 10, 1, 70, None, "default", "fc32", None, 2, (4,) + (0,) * 29, 1200),
    # more messages than one grid holds: the second launch starts at msg0 = 65535
    Case("two-launches", 64, 0, 1, 10, 1, 65537, None, "default", "fc32", None, 1, (1,), 1201),
]
SC16_SCALES = {64: None, 512: None, 1024: 1.0 / 32767.0, 2048: None, 4096: 1.0 / 32767.0}
SC16 = [c._replace(id=c.id + "-sc16", fmt="sc16", rx_scale=SC16_SCALES[c.S], seed=c.seed + 500)
        for c in FORCED if c.id.endswith("dead-groups") and c.S in SC16_SCALES]
CASES = FORCED + NATURAL + SC16
BY_ID = collections.OrderedDict((c.id, c) for c in CASES)
SC16_LEVEL = 2.0 ** 6            # noise of ~10 counts rms per part at S = 4096 (tones 2 .. 11), ~80 at S = 64 (150 .. 730)


def ids(cases):
    return [c.id for c in cases]


def case_geometry(c):
    return geometry(c.S, c.dwell, c.nmsgs, c.split)


def case_window(c):
    if c.window == "default":
        return None
    return (0.5 + np.random.default_rng(c.seed + 7).random(c.S)).tolist()


def sense_cfg(c, window="case"):
    level = SC16_LEVEL if c.fmt == "sc16" else 1.0
    return config.make_sense_cfg(c.S, c.tune, c.dwell, c.avg, c.skip, THRESHOLD * level * level,
                                 case_window(c) if window == "case" else window)


def _marked(c, geo, m):
    """The accrued vectors of message m that carry a tone, in the order of their bins: all of them while dwell <= S;
    otherwise one vector per lane first (round (lane + m) mod the lane's vectors; the last round in the last vector's
    lane), then the rest, each class from the dwell's last vector on
    and then from a start that moves with m."""
    f = np.arange(c.dwell)
    if c.dwell <= c.S:
        return f
    lane, rnd = f % geo.stride, f // geo.stride
    per_lane = -(-(c.dwell - lane) // geo.stride)
    cls = np.where(lane == (c.dwell - 1) % geo.stride, per_lane - 1 - rnd, (rnd - lane - m) % per_lane)
    order = np.lexsort((np.where(f == c.dwell - 1, -1, (f + 37 * m) % c.dwell), cls))
    return np.sort(order[:c.S])


def capture(c, sc=None):
    """The capture of a case as float samples (complex64): nmsgs whole messages and a tail of S/2 + 7 samples."""
    sc = sense_cfg(c) if sc is None else sc
    S, per = c.S, c.tune + c.dwell
    level = SC16_LEVEL if c.fmt == "sc16" else 1.0
    rng = np.random.default_rng(c.seed)
    geo = case_geometry(c)
    w = np.array(sc.window[:S], np.float64)
    sigma = level * np.sqrt(NOISE_FLOOR / (2.0 * np.sum(w * w)))
    n = c.nmsgs * per * S + S // 2 + 7
    x = (rng.standard_normal(n, dtype=np.float32) + 1j * rng.standard_normal(n, dtype=np.float32)) * np.float32(sigma)
    t = np.arange(S)
    loud = level * np.sqrt(5.0e-2) / np.sum(w)
    body = x[:c.nmsgs * per * S].reshape(c.nmsgs, per, S)
    body[:, :c.tune, :] += (loud * np.exp(2j * np.pi * (S // 4) * t / S)).astype(np.complex64)
    x[c.nmsgs * per * S:] += np.complex64(loud)
    nmark = min(c.dwell, S)
    gap = (S - nmark) // 2
    shift = 0 if c.window == "default" else 5    # (the default window's main lobe is nine bins wide: neighbours in
    j = np.arange(nmark)                           # bin stay neighbours in power, and the run of bins never wraps)
    for m0 in range(0, c.nmsgs, 4096):
        ms = np.arange(m0, min(c.nmsgs, m0 + 4096))
        marked = np.stack([_marked(c, geo, m) for m in ms]) if c.dwell > S else np.broadcast_to(j, (len(ms), nmark))
        bins = (gap + j[None, :] + shift * ms[:, None]) % S
        # (a lone tone per message takes its place on the scale by chance)
        place = j / (nmark - 1) if nmark > 1 else rng.random((len(ms), 1))
        power = 2.0e-5 * 25.0 ** place * rng.uniform(0.95, 1.05, (len(ms), nmark))
        amp = level * np.sqrt(power) / np.sum(w) * np.exp(2j * np.pi * rng.random((len(ms), nmark)))
        tone = amp[:, :, None] * np.exp(2j * np.pi * bins[:, :, None] * t[None, None, :] / S)
        body[ms[:, None], c.tune + marked, :] += tone.astype(np.complex64)
    return np.ascontiguousarray(x, np.complex64)


_BUILT, _REF = {}, {}


def built(c):
    """(sc, x, xf): the configuration, what the engine is handed (complex64, or int16 (n, 2) for an sc16 case) and the
    float samples those are (what the oracle and the model are handed)."""
    if c.id not in _BUILT:
        sc = sense_cfg(c)
        x = capture(c, sc)
        if c.fmt == "sc16":
            x = iqio.to_sc16(x)
            xf = iqio.from_sc16(x, c.rx_scale)
        else:
            xf = x
        x.setflags(write=False)
        xf.setflags(write=False)
        _BUILT[c.id] = (sc, x, xf)
    return _BUILT[c.id]


def _frozen(r):
    for k in ("msgs", "mean", "bits"):
        r[k].setflags(write=False)
    return r


def reference(orc, c):
    """(sc, x, ref): ref = the oracle's result on the case's float samples."""
    sc, x, xf = built(c)
    if c.id not in _REF:
        _REF[c.id] = _frozen(orc.sense(sc, xf))
    return sc, x, _REF[c.id]


# ---- what a round and a lane decide ----------------------------------------------------------------------------------------
def sole_winners(pw):
    """pw [message][vector][bin] -> winner [message][bin]: the vector that alone holds the bin's maximum after rounding
    to float32, -1 where two tie.  Without that vector the message's float32 body differs at that bin."""
    p32 = pw.astype(np.float32)
    mx = p32.max(axis=1, keepdims=True)
    hit = p32 == mx
    return np.where(hit.sum(axis=1) == 1, hit.argmax(axis=1), -1)


def decides(winner, groups, ngroups):
    """groups[vector] = the round (or lane) of each vector -> [message][group]: True where one of the group's vectors is
    a bin's sole winner, i.e. where the message would differ with the group's vectors removed."""
    out = np.zeros((winner.shape[0], ngroups), bool)
    m, b = np.nonzero(winner >= 0)
    out[m, groups[winner[m, b]]] = True
    return out
