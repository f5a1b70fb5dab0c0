"""Wideband receive front end for captures whose rate is no integer multiple of the modem's: tune to one link and
resample by L / M.

A radio answers a rate request with the rate it can make (the reference's wrapper prints "Actual sps for rate",
uhd_interface.py), and recorded captures come at whatever rate the recorder ran at.  GNU Radio's stage for this is
``blks2.rational_resampler_ccf(interpolation, decimation, taps)``; here it is fused with the frequency translation of
ddc.py and run on the GPU by ``Engine.resamp`` (csrc/resamp.h).  This module holds the host side: the low-pass
design, the normative band-pass table, the configuration struct and the output count.

Frequencies are in cycles per INPUT (wideband) sample; the taps live at L times the input rate.
"""
import numpy as np

from . import _abi, ddc, firdes

MAX_TAPS = _abi.OFDM_RESAMP_MAX_TAPS
MAX_RATIO = 64
MAX_LINKS = _abi.OFDM_RESAMP_BANK_MAX_LINKS


def _check_ratio(interpolation, decimation):
    L, M = int(interpolation), int(decimation)
    if not 1 <= L <= MAX_RATIO:
        raise ValueError("interpolation must be in [1, %d]" % MAX_RATIO)
    if not 1 <= M <= MAX_RATIO:
        raise ValueError("decimation must be in [1, %d]" % MAX_RATIO)
    return L, M


def design(interpolation, decimation, occupied_fraction, transition=None):
    """Real low-pass prototype at L times the wideband rate for a link that fills ``occupied_fraction`` of the output
    band (occupied_tones / fft_length): ``firdes.low_pass(L, 1.0, of / (2M) + transition / 2, transition)`` as
    float32, odd length -- ddc.design at R = M with gain L (the zero-stuffing by L takes 1 / L away).

    Frequencies here are in cycles per sample of the L-times grid, on which the output rate is 1 / M and the input
    rate 1 / L.  The signal's edge lies at of / (2M); the first spectrum that folds onto it after decimation begins at
    1/M - of / (2M).  Default transition: half that gap, (1 - of) / (2M), widened where needed so that
    ntaps <= OFDM_RESAMP_MAX_TAPS.  ValueError where of * L > M: the link is then wider than the capture."""
    L, M = _check_ratio(interpolation, decimation)
    of = float(occupied_fraction)
    if not 0.0 < of <= 1.0:
        raise ValueError("occupied_fraction must be in (0, 1]")
    if of * L > M:
        raise ValueError("a link that fills %g of the output band is wider than the capture at L / M = %d / %d" % (of, L, M))
    if transition is None:
        transition = max((1.0 - of) / (2.0 * M), ddc._MIN_TRANSITION)
    transition = float(transition)
    if firdes.compute_ntaps(1.0, transition) > MAX_TAPS:
        raise ValueError("transition %g needs more than %d taps" % (transition, MAX_TAPS))
    cutoff = min(of / (2.0 * M) + 0.5 * transition, 0.5)
    return np.asarray(firdes.low_pass(float(L), 1.0, cutoff, transition, firdes.WIN_HAMMING), np.float32)


def bandpass_taps(taps, fc, interpolation):
    """The normative table c[k] = complex64(h[k] exp(j 2 pi fc k / L)): float32 taps, float64 arithmetic, rounded
    once.  (``Engine.resamp_taps`` returns the table the kernel holds, computed the same way by the library's libm.)"""
    return ddc.bandpass_taps(taps, fc, interpolation)


def count(first, n, interpolation, decimation):
    """Outputs of a call with input indices [first, first + n): every m with first <= floor(m M / L) < first + n,
    ceil((first + n) L / M) - ceil(first L / M)."""
    L, M = int(interpolation), int(decimation)
    return -(-(int(first) + int(n)) * L // M) - -(-int(first) * L // M)


def resamp_cfg(interpolation, decimation, center_freq=0.0, taps=None, occupied_fraction=None, transition=None):
    """ofdm_resamp_cfg for Engine.set_resamp; ``taps=None`` designs them from ``occupied_fraction``."""
    cfg = ddc._cfg_with_taps(_abi.ofdm_resamp_cfg, "resamp_cfg", MAX_TAPS, taps, occupied_fraction,
                             lambda: design(interpolation, decimation, occupied_fraction, transition))
    cfg.interpolation = int(interpolation)
    cfg.decimation = int(decimation)
    cfg.center_freq = float(center_freq)
    return cfg


def bank_cfg(interpolation, decimation, center_freqs, taps=None, occupied_fraction=None, transition=None):
    """ofdm_resamp_bank_cfg for Engine.set_resamp_bank: one ratio and one prototype, one centre frequency per link
    (1 to MAX_LINKS of them, each in [-0.5, 0.5] cycles per wideband sample; equal ones are allowed).  ``taps=None``
    designs the prototype from ``occupied_fraction`` as resamp_cfg does.  ValueError for a ratio outside 1..64, with
    given taps too."""
    L, M = _check_ratio(interpolation, decimation)
    cfg = ddc._bank_cfg_with_taps(_abi.ofdm_resamp_bank_cfg, "resampler bank", MAX_LINKS, center_freqs, MAX_TAPS, taps,
                                  occupied_fraction,
                                  lambda: design(interpolation, decimation, occupied_fraction, transition))
    cfg.interpolation = L
    cfg.decimation = M
    return cfg
