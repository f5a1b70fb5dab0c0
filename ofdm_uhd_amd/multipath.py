"""Propagation channel between the transmitter and the receiver: multipath, Doppler, tones, carrier offset and noise.

The reference has a radio pair and the air between ``usrp_transmit_path`` and ``usrp_receive_path``; with files and
arrays in the radios' place the air is this stage, run on the GPU by ``Engine.multipath`` (csrc/multipath.h): P delayed
paths, each with a complex gain and a Doppler shift, J continuous tones (a primary user for the spectrum sensor), then
the flat channel's carrier rotation and noise (``Engine.channel``).  This module holds the host side: the configuration
struct, a few profile helpers and the ``channel`` object that streams through the stage.

Delays are in samples, frequencies in cycles per sample, phases in cycles, ``cfo`` in radians per sample.
"""
import math
import re

import numpy as np

from . import _abi, iqio

MAX_PATHS = _abi.OFDM_MULTIPATH_MAX_PATHS
MAX_TONES = _abi.OFDM_MULTIPATH_MAX_TONES
MAX_DELAY = _abi.OFDM_MULTIPATH_MAX_DELAY


def _in_half(v, what):
    v = float(v)
    if not abs(v) <= 0.5:           # (NaN fails the comparison)
        raise ValueError("%s must be in [-0.5, 0.5] cycles per sample" % what)
    return v


def multipath_cfg(paths=((0, 1.0),), tones=(), sigma=0.0, cfo=0.0, seed=0xC0FFEE, stream_id=0, out_format="fc32",
                  out_scale=None):
    """ofdm_multipath_cfg for Engine.set_multipath.  ``paths``: 1 to MAX_PATHS tuples (delay, gain[, doppler]), delay an
    integer in [0, MAX_DELAY], gain a finite complex number, doppler in [-0.5, 0.5]; ``tones``: up to MAX_TONES tuples
    (amp, freq[, phase]), amp finite and >= 0, freq in [-0.5, 0.5], phase in cycles; ``sigma`` >= 0 and ``cfo`` are
    the flat channel's (Engine.channel); ``out_format`` is "fc32" or "sc16" (``out_scale`` None: 2^15).  Raises
    ValueError for everything the library refuses."""
    paths, tones = list(paths), list(tones)
    if not 1 <= len(paths) <= MAX_PATHS:
        raise ValueError("multipath_cfg takes 1 to %d paths" % MAX_PATHS)
    if len(tones) > MAX_TONES:
        raise ValueError("multipath_cfg takes at most %d tones" % MAX_TONES)
    cfg = _abi.ofdm_multipath_cfg()
    cfg.struct_size = _abi.C.sizeof(cfg)
    cfg.npaths, cfg.ntones = len(paths), len(tones)
    for p, path in enumerate(paths):
        if not 2 <= len(path) <= 3:
            raise ValueError("a path is (delay, gain) or (delay, gain, doppler)")
        delay, gain = path[0], complex(path[1])
        if delay != int(delay) or not 0 <= int(delay) <= MAX_DELAY:
            raise ValueError("a path's delay must be an integer in [0, %d] samples" % MAX_DELAY)
        gain = np.complex64(gain)
        if not (np.isfinite(gain.real) and np.isfinite(gain.imag)):
            raise ValueError("a path's gain must be finite")
        cfg.delay[p] = int(delay)
        cfg.gain[p].re, cfg.gain[p].im = float(gain.real), float(gain.imag)
        cfg.doppler[p] = _in_half(path[2] if len(path) == 3 else 0.0, "a path's doppler")
    for j, tone in enumerate(tones):
        if not 2 <= len(tone) <= 3:
            raise ValueError("a tone is (amp, freq) or (amp, freq, phase)")
        amp = float(np.float32(tone[0]))
        if not (np.isfinite(amp) and amp >= 0.0):
            raise ValueError("a tone's amplitude must be finite and not negative")
        phase = float(tone[2]) if len(tone) == 3 else 0.0
        if not np.isfinite(phase):
            raise ValueError("a tone's phase must be finite")
        cfg.tone_amp[j] = amp
        cfg.tone_freq[j] = _in_half(tone[1], "a tone's frequency")
        cfg.tone_phase[j] = phase
    sigma, cfo = float(np.float32(sigma)), float(np.float32(cfo))
    if not (np.isfinite(sigma) and sigma >= 0.0):
        raise ValueError("sigma must be finite and not negative")
    if not np.isfinite(cfo):
        raise ValueError("cfo must be finite")
    cfg.sigma, cfg.cfo = sigma, cfo
    cfg.seed, cfg.stream_id = int(seed), int(stream_id)
    cfg.out_format = iqio.FORMATS.index(iqio.check_format(out_format))
    cfg.out_scale = 0.0 if out_scale is None else iqio.check_scale(out_scale, iqio.TX_SCALE)
    return cfg


def paths_of(cfg):
    """[(delay, gain, doppler)] of a configuration"""
    return [(int(cfg.delay[p]), complex(cfg.gain[p].re, cfg.gain[p].im), float(cfg.doppler[p])) for p in range(cfg.npaths)]


def tones_of(cfg):
    """[(amp, freq, phase)] of a configuration"""
    return [(float(cfg.tone_amp[j]), float(cfg.tone_freq[j]), float(cfg.tone_phase[j])) for j in range(cfg.ntones)]


def max_delay(cfg):
    return max(d for d, _, _ in paths_of(cfg))


def sigma_for_snr(snr_db, signal_power):
    """The sigma at which noise of power sigma^2 lies ``snr_db`` below ``signal_power`` (mean |x|^2)."""
    signal_power = float(signal_power)
    if not (np.isfinite(signal_power) and signal_power >= 0.0) or not np.isfinite(float(snr_db)):
        raise ValueError("sigma_for_snr takes a finite snr and a finite signal power >= 0")
    return math.sqrt(signal_power / 10.0 ** (float(snr_db) / 10.0))


def frequency_response(cfg, N):
    """H[k] = sum_p g_p exp(-2j pi k d_p / N), k in [0, N), of a static profile (float64; bin k in FFT order).
    ValueError for a profile with a Doppler path: it has no time-invariant response."""
    k = np.arange(int(N), dtype=np.float64)
    H = np.zeros(int(N), np.complex128)
    for d, g, f in paths_of(cfg):
        if f != 0.0:
            raise ValueError("frequency_response takes a static profile (every doppler 0)")
        H += g * np.exp(-2j * np.pi * k * (d % int(N)) / int(N))
    return H


def exponential_profile(rng, npaths, rms_delay):
    """``npaths`` paths [(delay, gain)] with an exponential power-delay profile of the given RMS delay spread in
    samples: delay 0 and npaths - 1 further distinct delays drawn below 6 * rms_delay (at most MAX_DELAY), Rayleigh
    gains of mean power exp(-delay / rms_delay), the whole normalised to unit power."""
    npaths = int(npaths)
    if not 1 <= npaths <= MAX_PATHS:
        raise ValueError("exponential_profile takes 1 to %d paths" % MAX_PATHS)
    if not (np.isfinite(rms_delay) and rms_delay > 0):
        raise ValueError("rms_delay must be finite and positive")
    span = min(max(int(math.ceil(6.0 * rms_delay)), npaths - 1), MAX_DELAY)
    delays = np.concatenate([[0], 1 + np.sort(rng.choice(span, npaths - 1, replace=False))]).astype(int)
    g = (rng.standard_normal(npaths) + 1j * rng.standard_normal(npaths)) * np.sqrt(0.5 * np.exp(-delays / float(rms_delay)))
    g = g / np.sqrt(np.sum(np.abs(g) ** 2))
    return [(int(d), complex(c)) for d, c in zip(delays, g)]


def _number(s, what):
    try:
        return complex(s.replace("i", "j")) if ("j" in s or "i" in s) else float(s)
    except ValueError:
        raise ValueError("%s: %r is not a number" % (what, s))


def parse(spec):
    """Paths from the command line: "delay:gain[@doppler]" separated by ";", e.g. "0:1;4:0.35+0.35j;9:0.1@1e-4"."""
    out = []
    for item in [s.strip() for s in str(spec).split(";") if s.strip()]:
        m = re.match(r"^(\d+):([^@]+)(?:@(.+))?$", item)
        if not m:
            raise ValueError("a path is delay:gain[@doppler], not %r" % item)
        gain = complex(_number(m.group(2).strip(), "gain"))
        out.append((int(m.group(1)), gain) + ((float(_number(m.group(3).strip(), "doppler").real),) if m.group(3) else ()))
    if not out:
        raise ValueError("no path in %r" % (spec,))
    return out


def parse_tones(spec):
    """Tones from the command line: "amp:freq[@phase]" separated by ";", e.g. "0.01:0.125;0.02:-0.3@0.25"."""
    out = []
    for item in [s.strip() for s in str(spec).split(";") if s.strip()]:
        m = re.match(r"^([^:@]+):([^@]+)(?:@(.+))?$", item)
        if not m:
            raise ValueError("a tone is amp:freq[@phase], not %r" % item)
        vals = [float(_number(g.strip(), "tone").real) for g in m.groups() if g is not None]
        out.append(tuple(vals))
    return out


def format_paths(paths):
    """The inverse of parse (repr keeps every digit)."""
    items = []
    for path in paths:
        g = complex(path[1])
        s = "%d:%s" % (int(path[0]), repr(g.real) if g.imag == 0 else repr(g).strip("()"))
        if len(path) == 3 and path[2] != 0.0:
            s += "@%r" % float(path[2])
        items.append(s)
    return ";".join(items)


class channel(object):
    """A stream through the stage on an Engine of its own (default options).  ``work(iq)`` is one whole stream, its
    echoes' tail included: len(iq) + Dmax samples.  ``feed(chunk)`` returns as many samples as it is given and
    ``flush()`` pushes Dmax zeros, so that the tail comes out, and starts the stream afresh: the concatenation equals
    ``work`` on the concatenated chunks, bit for bit.  A stream fed after work() starts afresh."""

    def __init__(self, cfg, device_id=0):
        from . import engine, options
        self.cfg = cfg
        self.dmax = max_delay(cfg)
        self._e = engine.Engine(options.default_options(), device_id=device_id)
        self._e.set_multipath(cfg)

    def engine(self):
        return self._e

    def feed(self, chunk):
        return self._e.multipath(chunk)

    def flush(self):
        out = self._e.multipath(np.zeros(self.dmax, np.complex64))
        self._e.multipath_reset(0)
        return out

    def work(self, iq):
        self._e.multipath_reset(0)
        return np.concatenate([self.feed(iq), self.flush()])

    def close(self):
        if self._e is not None:
            self._e.close()
            self._e = None
