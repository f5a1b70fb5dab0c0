"""Transmit crest-factor reduction: peak windowing in front of a converter.

The modem's output has a peak-to-average power ratio (PAPR) of 10 to 11 dB, and the only thing between it and a 16-bit
converter used to be the clamp of the sc16 store, a hard clip per I and Q part.  The stage ``Engine.cfr`` runs on the
GPU (csrc/cfr.h) pulls every peak above a threshold down to it by a smooth dip of the gain, of the shape of a window,
delays the stream by the window's half-width and counts what it did.  This module holds the host side: the
configuration struct, a window design, the threshold for a PAPR target and the figures derived from the statistics.
"""
import math

import numpy as np

from . import _abi, iqio

MAX_TAPS = _abi.OFDM_CFR_MAX_TAPS
MAX_HALF_WIDTH = (MAX_TAPS - 1) // 2


def design(half_width, kind="hann"):
    """A window of 2 * half_width + 1 float32 values for ``cfr_cfg``: centre exactly 1, symmetric, every value in
    (0, 1], the ends not zero (a Hann or triangular window of 2 * half_width + 3 points without its two zeros; "rect":
    all ones).  half_width = 0 is the polar clip."""
    H = int(half_width)
    if H != half_width or not 0 <= H <= MAX_HALF_WIDTH:
        raise ValueError("half_width must be an integer in [0, %d]" % MAX_HALF_WIDTH)
    k = np.arange(-H, H + 1, dtype=np.float64) / (H + 1.0)
    if kind == "hann":
        w = 0.5 + 0.5 * np.cos(np.pi * k)
    elif kind == "triangular":
        w = 1.0 - np.abs(k)
    elif kind == "rect":
        w = np.ones(2 * H + 1)
    else:
        raise ValueError("window kind must be hann, triangular or rect, not %r" % (kind,))
    w = w.astype(np.float32)
    w[H] = 1.0
    return w


def cfr_cfg(threshold, window=None, out_format="fc32", out_scale=None):
    """ofdm_cfr_cfg for Engine.set_cfr.  ``threshold`` > 0 is the magnitude peaks are pulled down to; ``window`` holds an
    odd number (at most MAX_TAPS) of values in [0, 1] with the centre exactly 1 (None: design(16)); ``out_format`` is
    "fc32" or "sc16" (``out_scale`` None: 2^15).  Raises ValueError for everything the library refuses."""
    thr = float(np.float32(threshold))
    if not (np.isfinite(thr) and thr > 0.0):
        raise ValueError("threshold must be finite and positive")
    w = design(16) if window is None else np.asarray(window, np.float32).reshape(-1)
    if len(w) % 2 == 0 or len(w) > MAX_TAPS:
        raise ValueError("a window has an odd number of values, at most %d" % MAX_TAPS)
    if not np.all((w >= 0.0) & (w <= 1.0)):         # (NaN fails the comparison)
        raise ValueError("a window's values must be in [0, 1]")
    if w[len(w) // 2] != 1.0:
        raise ValueError("a window's centre must be exactly 1")
    cfg = _abi.ofdm_cfr_cfg()
    cfg.struct_size = _abi.C.sizeof(cfg)
    cfg.threshold = thr
    cfg.ntaps = len(w)
    cfg.taps[:len(w)] = [float(v) for v in w]
    cfg.out_format = iqio.FORMATS.index(iqio.check_format(out_format))
    cfg.out_scale = 0.0 if out_scale is None else iqio.check_scale(out_scale, iqio.TX_SCALE)
    return cfg


def window_of(cfg):
    return np.array(cfg.taps[:cfg.ntaps], np.float32)


def half_width(cfg):
    return (int(cfg.ntaps) - 1) // 2


def threshold_for(papr_db, rms):
    """The threshold that lies ``papr_db`` above a stream of root-mean-square magnitude ``rms``."""
    papr_db, rms = float(papr_db), float(rms)
    if not (np.isfinite(papr_db) and np.isfinite(rms) and rms > 0.0):
        raise ValueError("threshold_for takes a finite PAPR and a finite rms > 0")
    return rms * 10.0 ** (papr_db / 20.0)


def modem_rms(options):
    """Root-mean-square magnitude of the modulator's data symbols, from its own scaling: the inverse FFT of
    occupied_tones unit carriers, times 1 / sqrt(fft_length), times the transmit amplitude where the options carry one
    (ofdm_mod itself runs at amplitude 1).  It is the level a PAPR target is set against: preambles (every other
    carrier) and gaps between packets lie below it."""
    amp = getattr(options, "tx_amplitude", None)
    amp = 1.0 if amp is None else float(amp)
    return amp * math.sqrt(float(options.occupied_tones) / float(options.fft_length))


def _db(ratio):
    return 10.0 * math.log10(ratio) if ratio > 0.0 else float("-inf")


def report(stats, rms=None):
    """PAPR and EVM figures of Engine.cfr_stats().  ``rms`` None: the averages are the measured ones, sum / n over
    everything the stage was fed (gaps between packets and the zeros of a flush included).  ``rms`` given: both PAPR
    figures are taken against the power rms^2, the level the threshold was set against, and ``mean_in_db`` /
    ``mean_out_db`` say where the measured averages lie relative to it.  ``evm_db`` is the error the stage itself
    causes, sum_err / sum_in; ``share_over`` / ``share_touched`` the fraction of samples over the threshold / with a
    gain below 1."""
    n = int(stats["n"])
    if n == 0:
        raise ValueError("no samples since the statistics were reset")
    mean_in, mean_out = stats["sum_in"] / n, stats["sum_out"] / n
    ref_in = ref_out = None if rms is None else float(rms) ** 2
    if rms is None:
        ref_in, ref_out = mean_in, mean_out
    out = {
        "papr_in_db": _db(stats["peak_in"] / ref_in) if ref_in > 0.0 else float("nan"),
        "papr_out_db": _db(stats["peak_out"] / ref_out) if ref_out > 0.0 else float("nan"),
        "evm_db": _db(stats["sum_err"] / stats["sum_in"]) if stats["sum_in"] > 0.0 else float("nan"),
        "share_over": stats["n_over"] / float(n),
        "share_touched": stats["n_touched"] / float(n),
    }
    if rms is not None:
        out["mean_in_db"], out["mean_out_db"] = _db(mean_in / ref_in), _db(mean_out / ref_out)
    return out
