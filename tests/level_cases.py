"""Captures at input levels the rest of the suite never feeds the receiver, shared by test_level_cases_host.py (what the
oracle does with them, and that each reaches the constant it is for) and test_gpu_levels.py (engine against oracle).

Every other receive test uses what orc.tx gives at tx_amplitude = 0.25: rms 0.15 .. 0.2, peaks 0.5 .. 0.9.  The
synchroniser is not scale-free: its window sums are Q23.40 fixed point, LSB 2^-40, each term clamped to +-511
(csrc/common.h q40_clamped, oracle q40), M is clamped to 1024, and a NaN term becomes -511 (DESIGN.md section 2,
"Input level").  The captures here are the loopback captures of three small geometries and one N = 4096 row

  * multiplied by a power of two -- every float32 operation in front of the fixed point then scales exactly, so whatever
    changes with the level comes from the absolute constants and nothing else;
  * as two bursts 2^-k apart in one capture, in both orders;
  * quantised to 16 bits at rms ~ 10 counts;
  * with a single sample replaced by NaN, Inf, (-Inf, NaN) or 3e38.

No GPU and no engine here; the oracle comes in as the `orc` fixture.  Results are computed once and are read-only."""
import collections

import numpy as np

from helpers import loopback_stream, make_cfg, make_payloads
from ofdm_uhd_amd import _abi, iqio

Geom = collections.namedtuple("Geom", "mod N occ CP plen npkt")
GEOMS = {
    "qpsk-512": Geom("qpsk", 512, 200, 128, 300, 4),
    "qam16-256": Geom("qam16", 256, 120, 64, 200, 4),
    "bpsk-64": Geom("bpsk", 64, 48, 16, 60, 4),
    "qam64-4096": Geom("qam64", 4096, 2400, 1024, 200, 2),     # the 2048-term window, for the clamp
}
SMALL = ("qpsk-512", "qam16-256", "bpsk-64")
SNR_DB, CFO_BINS = 30.0, 0.05
Q40_CLAMP = 511.0         # csrc/common.h q40_clamped, oracle q40

# -140 / -120: subnormal input and products.  -70, -24: every term below half an LSB.  -18 .. +8: the edges of the working
# window.  +14: every term at the clamp.  +64: the float32 window sums overflow, single terms stay finite.  +70, +110:
# |y|^2 is Inf and the correlator's products give Inf - Inf = NaN terms.  +125: the channel filter's transform overflows
# and makes NaN from finite input (at +110 it does not yet: 2^110 times the transform's gain stays below 2^128).
EXPONENTS = (-140, -120, -70, -24, -18, -16, -12, 6, 7, 8, 14, 64, 70, 110, 125)
EXPONENTS_4096 = (0, 7, 14, 64)
# the oracle's working window in powers of two of the nominal level (test_level_cases_host.py keeps these true)
WINDOW = (-14, 7)            # every transmitted payload comes back CRC-ok, at every exponent and geometry (also at -16)
SAME_FLAGS = (-11, 6)        # the timing flags are those of e = 0
UNIFORM = [(g, e) for g in SMALL for e in EXPONENTS] + [("qam64-4096", e) for e in EXPONENTS_4096]
UNIFORM_IDS = ["%s-e%+d" % c for c in UNIFORM]

STEP_K = (6, 13)
STEPS = [(k, order) for k in STEP_K for order in ("strong-weak", "weak-strong")]
STEP_IDS = ["k%d-%s" % s for s in STEPS]

NONFINITE = collections.OrderedDict([
    ("nan", complex(np.nan, 0.0)),
    ("inf", complex(np.inf, 0.0)),
    ("minf-nan", complex(-np.inf, np.nan)),
    ("3e38", complex(3e38, 0.0)),
])
POSITIONS = ("lead-in", "data-symbol", "before-flag")
POISON = [(v, p) for v in NONFINITE for p in POSITIONS]
POISON_IDS = ["%s-%s" % c for c in POISON]

RX_TAPS = (_abi.TAP_RX_CHAN_FILT, _abi.TAP_RX_METRIC, _abi.TAP_RX_PRESEL, _abi.TAP_RX_FFT, _abi.TAP_RX_ACQ,
           _abi.TAP_RX_SINK, _abi.TAP_RX_PACKETS)       # = test_gpu_parity.RX_TAPS
_MASK = sum(1 << t for t in RX_TAPS)

_CFG, _BASE, _REF = {}, {}, {}


def cfg_of(geom):
    if geom not in _CFG:
        g = GEOMS[geom]
        _CFG[geom] = make_cfg(g.mod, g.N, g.occ, g.CP)
    return _CFG[geom]


def payloads(geom):
    g = GEOMS[geom]
    return make_payloads(g.npkt, g.plen)


def base_capture(orc, geom):
    """helpers.loopback_stream at its default seeds: 30 dB, 0.05 bins."""
    if geom not in _BASE:
        x = loopback_stream(orc, cfg_of(geom), payloads(geom), snr_db=SNR_DB, cfo_bins=CFO_BINS)
        x.setflags(write=False)
        _BASE[geom] = x
    return _BASE[geom]


def scaled(x, e):
    """x * 2^e as complex64: the product in float64 (exact: range to 2^+-1023), rounded once.  A power of two only
    shifts the exponent, so the rounding does something only where the result is subnormal or overflows."""
    with np.errstate(over="ignore", under="ignore"):
        y = (np.asarray(x).astype(np.complex128) * 2.0 ** e).astype(np.complex64)
    return y


def _ref(orc, key, geom, make):
    if key not in _REF:
        x = make()
        x.setflags(write=False)
        cfg = cfg_of(geom)
        _REF[key] = (cfg, x, orc.rx(cfg, iqio.from_sc16(x) if x.dtype == np.int16 else x, _MASK))
    return _REF[key]


def uniform(orc, geom, e):
    """(cfg, x, ro): the geometry's capture times 2^e and the oracle's result on it (taps of _check_rx)."""
    return _ref(orc, ("uniform", geom, e), geom, lambda: scaled(base_capture(orc, geom), e))


def ok_payloads(ro):
    return [p for ok, p in ro.packets if ok]


# ---- two bursts at different levels ------------------------------------------------------------------------------------
STEP_GEOM = "qpsk-512"
STEP_NPKT = 3


def step_capture(orc, k, order):
    """Two bursts of three qpsk-512 packets each, 2N samples of silence on either side of each: the strong one (packets
    0 .. 2) at the nominal level, the weak one (packets 3 .. 5) times 2^-k, in the given order; then the channel over the
    whole capture, its noise 30 dB under the weak burst."""
    cfg = cfg_of(STEP_GEOM)
    N = cfg.fft_length
    pay = make_payloads(2 * STEP_NPKT, GEOMS[STEP_GEOM].plen)
    strong = orc.tx(cfg, pay[:STEP_NPKT], lead=2 * N, tail=2 * N)
    weak = scaled(orc.tx(cfg, pay[STEP_NPKT:], lead=2 * N, tail=2 * N), -k)
    psig = float(np.mean(np.abs(weak[2 * N:-2 * N].astype(np.complex128)) ** 2))
    x = np.concatenate([strong, weak] if order == "strong-weak" else [weak, strong])
    x = np.ascontiguousarray(x, np.complex64)
    orc.channel(x, sigma=float(np.sqrt(psig / 10 ** (SNR_DB / 10.0))), cfo=CFO_BINS * 2 * np.pi / N)
    return x, pay


def step(orc, k, order):
    """(cfg, x, ro, payloads)."""
    pay = make_payloads(2 * STEP_NPKT, GEOMS[STEP_GEOM].plen)
    return _ref(orc, ("step", k, order), STEP_GEOM, lambda: step_capture(orc, k, order)[0]) + (pay,)


# ---- a 16-bit capture at a low level -----------------------------------------------------------------------------------
SC16_E = -9


def sc16(orc):
    """(cfg, q, ro): the qpsk capture at 2^-9 through iqio.to_sc16 at the default scale (rms ~ 10 counts); the oracle's
    result on iqio.from_sc16(q)."""
    return _ref(orc, ("sc16",), "qpsk-512", lambda: iqio.to_sc16(scaled(base_capture(orc, "qpsk-512"), SC16_E)))


# ---- one non-finite sample ---------------------------------------------------------------------------------------------
def symbols_per_packet(orc, geom):
    cfg, g = cfg_of(geom), GEOMS[geom]
    return len(orc.tx(cfg, payloads(geom)[:1])) // (g.N + g.CP)


def poison_index(orc, position):
    """Where the sample goes in the qpsk capture (lead-in 2N = 1024 samples, packets back to back behind it)."""
    g = GEOMS["qpsk-512"]
    sym = g.N + g.CP
    if position == "lead-in":
        return 100
    if position == "data-symbol":            # the middle of packet 1's third data symbol (symbol 0 is the preamble)
        return 2 * g.N + symbols_per_packet(orc, "qpsk-512") * sym + 3 * sym + g.CP + g.N // 2
    flags = uniform(orc, "qpsk-512", 0)[2].tap(_abi.TAP_RX_PEAKS).tolist()
    assert len(flags) >= g.npkt              # (one per packet, in order; the capture's tail raises one more)
    return int(flags[2]) - 200               # 200 samples before packet 2's flag


def poisoned(orc, value, position):
    """(cfg, x, ro, index)."""
    i = poison_index(orc, position)

    def make():
        x = base_capture(orc, "qpsk-512").copy()
        x[i] = np.complex64(NONFINITE[value])
        return x
    return _ref(orc, ("poison", value, position), "qpsk-512", make) + (i,)


def filter_blocks(cfg, i):
    """The overlap-save blocks of the channel filter whose input window holds sample i, as (first, last) output samples:
    block b transforms x[b*B - (ntaps-1) .. b*B + B) and produces y[b*B .. b*B + B)."""
    nt = int(cfg.ntaps)
    p2 = 1
    while p2 < nt:
        p2 <<= 1
    F = max(64, 2 * p2)
    B = F - nt + 1
    return [(b * B, b * B + B - 1) for b in range(i // B, (i + nt - 1) // B + 1)]


# ---- counts on the oracle's input and taps -----------------------------------------------------------------------------
def n_clamped(x):
    """Samples whose energy term |x|^2 (float32, as the metric forms it) takes the +-511 clamp."""
    with np.errstate(over="ignore", invalid="ignore"):
        e = x.real * x.real + x.imag * x.imag
    return int(np.count_nonzero(e > np.float32(Q40_CLAMP)))


def n_subnormal(x):
    """float32 parts that are subnormal (non-zero, below 2^-126)."""
    p = np.abs(np.ascontiguousarray(x).view(np.float32))
    return int(np.count_nonzero((p > 0) & (p < np.float32(2.0 ** -126))))


def n_nonfinite(x):
    return int(np.count_nonzero(~np.isfinite(np.ascontiguousarray(x).view(np.float32).reshape(-1, 2)).all(axis=1)))


# ---- the normative metric, restated --------------------------------------------------------------------------------------


def _q40(v):
    """llrint(clamp(v) * 2^40) of float32 terms: fmax / fmin (a NaN term becomes -511), round to nearest even."""
    v = np.fmin(np.fmax(v, np.float32(-Q40_CLAMP)), np.float32(Q40_CLAMP))
    return np.rint(v.astype(np.float64) * 2.0 ** 40).astype(np.int64)


def _window(q, w):
    """Sums of the w newest terms.  (The running total wraps in int64 on a long clamped capture; the difference of two
    totals is still the window's sum, which fits: 2048 * 511 * 2^40 < 2^60.)"""
    cs = np.concatenate([np.zeros(1, np.int64), np.cumsum(q, dtype=np.int64)])
    lo = np.maximum(np.arange(len(q)) + 1 - w, 0)
    return cs[1:] - cs[lo]


def q40_metric(cfg, y):
    """u = mean of M over CP samples - 1 as DESIGN.md section 2 defines it, from the filtered stream y: the terms in
    float32 (one rounding per operation), clamped to +-511 and summed in Q23.40, M = |P|^2 / R^2 (0 where R^2 = 0, 1024
    where it is not <= 1024), its mean in Q23.40 too.  NumPy on whole arrays: no order of evaluation to get wrong."""
    F = np.float32
    D, CP = cfg.fft_length // 2, cfg.cp_length
    y = np.asarray(y, np.complex64)
    ar, ai = y.real.copy(), y.imag.copy()
    dr, di = np.zeros_like(ar), np.zeros_like(ai)
    dr[D:], di[D:] = ar[:-D], ai[:-D]
    with np.errstate(all="ignore"):
        cre = ar * dr + ai * di
        cim = ai * dr - ar * di
        en = ar * ar + ai * ai
        pre = (_window(_q40(cre), D).astype(np.float64) * 2.0 ** -40).astype(F)
        pim = (_window(_q40(cim), D).astype(np.float64) * 2.0 ** -40).astype(F)
        r = (_window(_q40(en), D).astype(np.float64) * 2.0 ** -40).astype(F)
        num, den = pre * pre + pim * pim, r * r
        m = np.where(den > 0, num / np.where(den > 0, den, F(1)), F(0)).astype(F)
        m = np.where(m <= F(1024), m, F(1024)).astype(F)
    sm = _window(np.rint(m.astype(np.float64) * 2.0 ** 40).astype(np.int64), CP)
    mbar = (sm.astype(np.float64) * 2.0 ** -40 * float(F(1.0 / CP))).astype(F)
    return mbar + F(-1.0)
