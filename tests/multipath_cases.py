"""Shared by test_multipath_host.py and test_gpu_multipath.py: the float64 model of the propagation channel stage (the
definition in include/ofdm_hip.h; rotation and noise are chan_cases.model, so the noise word of index n is the existing
definition), a NumPy float32 emulation of the kernel's arithmetic with the hooks the mutated copies go through, the
error bound both are held to, and the profiles both files run.

Bound per output:  |out - y64| <= (P + J + 16) * 2^-24 * S[n] + 1e-4 * sigma  with
S[n] = sum_p |g_p| |x[n - d_p]| + sum_j a_j + |add[n]|: P + J float32 additions in any order, 16 more roundings for the
phasor products, the carrier rotation and the final additions, and the project's accepted gap between the hardware's
log2 / sqrt / sin / cos and libm (chan_cases.engine_bound)."""
import collections

import numpy as np

import chan_cases
from ofdm_uhd_amd import multipath
from stage_harness import AMP, EPS, SCALE

TILE = 1024                       # outputs of one workgroup (csrc/multipath.h: MP_TILE)
MAX_INDEX = 1 << 53
TWO64 = 18446744073709551616.0

Profile = collections.namedtuple("Profile", "name paths tones sigma cfo seed stream_id")


def _dense16():
    rng = np.random.default_rng(1601)
    delays = np.concatenate([[0, 1023], 1 + rng.choice(1022, 14, replace=False)])
    rng.shuffle(delays)                                   # the largest delay is not the last path
    g = (rng.standard_normal(16) + 1j * rng.standard_normal(16)) * 0.25
    return [(int(d), complex(np.complex64(c))) for d, c in zip(delays, g)]


def _everything():
    f = {1: 1e-4, 5: -3e-3, 9: 0.5, 14: 0.0371}
    return [(d, g, f[p]) if p in f else (d, g) for p, (d, g) in enumerate(_dense16())]


_TONES4 = [(0.05, 0.0), (0.03, 0.5), (0.04, -0.5, 0.3), (0.02, 0.1234)]

PROFILES = collections.OrderedDict((p.name, p) for p in (
    Profile("unit", [(0, 1.0)], [], 0.0, 0.0, 0xC0FFEE, 0),
    Profile("two_ray", [(0, 1.0), (4, 0.5 * np.exp(0.7j))], [], 0.0, 0.0, 0xC0FFEE, 0),
    Profile("dense16", _dense16(), [], 0.0, 0.0, 0xC0FFEE, 0),
    Profile("twins", [(7, 0.6 + 0.2j), (7, -0.3 + 0.5j)], [], 0.0, 0.0, 0xC0FFEE, 0),
    Profile("late_only", [(1023, 0.8 - 0.3j)], [], 0.0, 0.0, 0xC0FFEE, 0),
    Profile("doppler4", [(0, 1.0, 0.0), (3, 0.5j, 1e-4), (11, -0.4 + 0.1j, -3e-3), (40, 0.3, 0.5)], [], 0.0, 0.0, 0xC0FFEE, 0),
    Profile("tones4", [(0, 1.0)], _TONES4, 0.0, 0.0, 0xC0FFEE, 0),
    Profile("everything", _everything(), _TONES4, 0.01, 0.003, chan_cases.BIG_SEED, 3),
))
NAMES = list(PROFILES)


def cfg_of(name, **kw):
    p = PROFILES[name]
    args = dict(paths=p.paths, tones=p.tones, sigma=p.sigma, cfo=p.cfo, seed=p.seed, stream_id=p.stream_id)
    args.update(kw)
    return multipath.multipath_cfg(**args)


def dmax_of(name):
    return max(path[0] for path in PROFILES[name].paths)


def stream(n, seed=1):
    """A stream at stage_harness.AMP: the model alone keeps a 16-bit store inside its range."""
    rng = np.random.default_rng(seed)
    return (AMP * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)


def turns(cycles):
    """frac(cycles) in units of 2^-64 turn, truncated, 0 where frac rounds up to 1 (engine_stage.inc: ddc_turns)"""
    t = float(cycles) - np.floor(float(cycles))
    if not t < 1.0:
        t = 0.0
    return int(t * TWO64)


def _phase(n, step, start=0):
    """(start + n step) mod 2^64 as uint64: the products wrap as the kernel's do"""
    with np.errstate(over="ignore"):
        return (np.uint64(start) + n * np.uint64(step)).astype(np.uint64)


def _delayed(x, d, drop_before=None):
    """x[n - d] for every n of the stream, zero before its start (or before the sample index drop_before for the outputs
    from there on: a chunk edge that dropped its history)"""
    y = np.zeros(len(x), x.dtype)
    y[d:] = x[:len(x) - d] if d else x
    if drop_before is not None:
        n = np.arange(len(x))
        y[(n >= drop_before) & (n - d < drop_before)] = 0
    return y


def model(x, cfg, first, add=None):
    """(y64, S): the definition in float64 on a stream whose first sample has the absolute index ``first``."""
    x = np.asarray(x, np.complex64)
    n = chan_cases.indices(len(x), first)
    v = np.zeros(len(x), np.complex128)
    S = np.zeros(len(x))
    for d, g, f in multipath.paths_of(cfg):
        D = turns(f)
        c = g * (np.exp(2j * np.pi * (_phase(n, D).astype(np.float64) / TWO64)) if D else 1.0)
        xd = _delayed(x, d).astype(np.complex128)
        v += c * xd
        S += abs(g) * np.abs(xd)
    for a, f, ph in multipath.tones_of(cfg):
        v += a * np.exp(2j * np.pi * (_phase(n, turns(f), turns(ph)).astype(np.float64) / TWO64))
        S += a
    y, _ = chan_cases.model(v, cfg.sigma, cfg.cfo, cfg.seed, cfg.stream_id, first)
    if add is not None:
        y = y + np.asarray(add).astype(np.complex128)
        S = S + np.abs(np.asarray(add).astype(np.complex128))
    return y, S


def bound(cfg, S):
    return (cfg.npaths + cfg.ntones + 16) * EPS * S + 1e-4 * float(cfg.sigma)


# ---- the float32 emulation ---------------------------------------------------------------------------------------------
def _c32(re, im):
    out = np.empty(len(re), np.complex64)
    out.real, out.imag = re, im
    return out


def cmul32(a, b):
    """the gr_complex product in float32: two products and one addition per part, separately rounded"""
    a, b = np.asarray(a, np.complex64), np.asarray(b, np.complex64)
    return _c32(a.real * b.real - a.imag * b.imag, a.real * b.imag + a.imag * b.real)


def cadd32(a, b):
    return _c32(a.real + b.real, a.imag + b.imag)


def phasor32(ph):
    """complex64(expj(2 pi ph / 2^64)) at the float64 angle (int64)ph * 2 pi / 2^64, rounded once"""
    r = ph.astype(np.int64).astype(np.float64) * 3.4061215800865545e-19
    return _c32(np.cos(r).astype(np.float32), np.sin(r).astype(np.float32))


def chan32(x, sigma, cfo, seed, stream_id, first, word_xor=0):
    """common.h's channel_apply in float32, libm in the hardware transcendentals' place"""
    f32 = np.float32
    sigma, cfo = f32(sigma), f32(cfo)
    idx = chan_cases.indices(len(x), first)
    y = np.asarray(x, np.complex64)
    if cfo != 0:
        ph = float(cfo) * idx.astype(np.float64)
        ph = ph - 2.0 * np.pi * np.floor(ph / (2.0 * np.pi) + 0.5)
        y = cmul32(y, _c32(np.cos(ph).astype(f32), np.sin(ph).astype(f32)))
    if sigma > 0:
        w = chan_cases.words(seed, stream_id, idx ^ np.uint64(word_xor))
        inv16 = f32(1.0 / 65536.0)
        u1 = ((w >> np.uint64(16)).astype(f32) + f32(0.5)) * inv16
        u2 = ((w & np.uint64(0xFFFF)).astype(f32) + f32(0.5)) * inv16
        rad = np.sqrt(f32(-1.3862943611198906) * np.log2(u1).astype(f32)).astype(f32)
        ang = 2.0 * np.pi * u2.astype(np.float64)
        sn, cs = np.sin(ang).astype(f32), np.cos(ang).astype(f32)
        s = sigma * f32(0.70710678118654752440)
        y = _c32(y.real + s * (rad * cs), y.imag + s * (rad * sn))
    return y


def emulate(x, cfg, first, add=None, delay_off=None, doppler_at=0, word_xor=0, conj_gain=False, tone_phase=True,
            drop_history_at=None):
    """The kernel's arithmetic in NumPy float32.  The keywords are the mutations test_multipath_host.py proves the bound
    can tell apart: ``delay_off`` = (path, samples), ``doppler_at`` = what is added to n in the Doppler phasors,
    ``word_xor`` = what the noise word's index is xor-ed with, ``conj_gain``, ``tone_phase`` False = phases ignored,
    ``drop_history_at`` = a sample index at which a chunk edge forgets the samples before it."""
    x = np.asarray(x, np.complex64)
    n = chan_cases.indices(len(x), first)
    v = np.zeros(len(x), np.complex64)
    for p, (d, g, f) in enumerate(multipath.paths_of(cfg)):
        if delay_off is not None and delay_off[0] == p:
            d += delay_off[1]
        c = np.full(len(x), np.conj(g) if conj_gain else g, np.complex64)
        D = turns(f)
        if D:
            c = cmul32(c, phasor32(_phase(n + np.uint64(doppler_at), D)))
        v = cadd32(v, cmul32(c, _delayed(x, d, drop_history_at)))
    if cfg.ntones:
        t = np.zeros(len(x), np.complex64)
        for a, f, ph in multipath.tones_of(cfg):
            r = phasor32(_phase(n, turns(f), turns(ph) if tone_phase else 0))
            t = cadd32(t, _c32(np.float32(a) * r.real, np.float32(a) * r.imag))
        v = cadd32(v, t)
    y = chan32(v, cfg.sigma, cfg.cfo, cfg.seed, cfg.stream_id, first, word_xor)
    if add is not None:
        y = cadd32(y, np.asarray(add, np.complex64))
    return y


def ratio(y, y64, b):
    """worst error / bound of complex64 outputs"""
    return float(np.max(np.abs(np.asarray(y).astype(np.complex128) - y64) / np.maximum(b, 1e-300)))


def check(y, x, cfg, first, fmt, what, add=None):
    """The stage's output against the model within the bound; 16-bit output: 0.5 / scale + bound per part wherever
    nothing clamps, at least 90 % of the samples (stage_harness.check_tx_model).  Prints and returns the worst
    error / bound."""
    y64, S = model(x, cfg, first, add)
    b = bound(cfg, S)
    assert len(y) == len(y64), what
    if fmt == "sc16":
        assert y.dtype == np.int16 and y.shape == (len(x), 2), what
        d = (y[:, 0].astype(np.float64) + 1j * y[:, 1].astype(np.float64)) / SCALE - y64
        free = (np.abs(y64.real) * SCALE < 32767 - 1) & (np.abs(y64.imag) * SCALE < 32767 - 1)
        assert np.count_nonzero(free) > 0.9 * len(y), what
        err, b = np.maximum(np.abs(d.real), np.abs(d.imag))[free], (0.5 / SCALE + b)[free]
    else:
        assert y.dtype == np.complex64, what
        err = np.abs(y.astype(np.complex128) - y64)
    worst = float(np.max(err / np.maximum(b, 1e-300))) if len(err) else 0.0
    print("%s: %d outputs, worst error / bound = %.3g" % (what, len(y), worst))
    assert np.all(err <= b), "%s: worst error / bound = %.3g" % (what, worst)
    return worst
