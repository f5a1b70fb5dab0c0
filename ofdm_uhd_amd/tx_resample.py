"""Wideband transmit at a rate that is no integer multiple of the modem's: resample by L / M and place the signal at an
offset inside the band.

The receive side reads such bands with resample.py; this is its mirror image and the generalisation of duc.py.  GNU
Radio's stage for it is ``blks2.rational_resampler_ccf(interpolation, decimation, taps)`` in front of the radio's
``set_center_freq``; here the two are one pass on the GPU, ``Engine.tx_resamp`` (csrc/tx_resamp.h), which can add its
output onto a band that already holds other links and can store 16-bit IQ.  This module holds the host side: the
low-pass design, the output count, the phase step and the configuration struct.

Frequencies are in cycles per OUTPUT (wideband) sample; the taps live at L times the input rate.
"""
import math

import numpy as np

from . import _abi, ddc, duc, firdes, iqio, resample

MAX_TAPS = _abi.OFDM_TX_RESAMP_MAX_TAPS
MAX_RATIO = resample.MAX_RATIO


_check_ratio = resample._check_ratio   # the two resamplers take the same ratios and count their outputs alike
count = resample.count


def design(interpolation, decimation, occupied_fraction, transition=None):
    """Real low-pass prototype at L times the narrowband rate for a link that fills ``occupied_fraction`` of the
    modem's band (occupied_tones / fft_length): ``firdes.low_pass(L, 1.0, e + transition / 2, transition)`` as
    float32, odd length.

    Frequencies here are in cycles per sample of the L-times grid, on which the input rate is 1 / L and the output
    rate 1 / M.  The signal's edge lies at e = of / (2L).  Zero stuffing puts its first image at 1/L - e; taking every
    M-th sample folds whatever lies beyond 1/M - e onto it.  Default transition: half the gap to the nearer of the two,
    (min(1/L, 1/M) - 2e) / 2, widened where needed so that ntaps <= OFDM_TX_RESAMP_MAX_TAPS.  ValueError where
    of * M > L: the link is then wider than the band.  The gain L restores unit pass-band gain after zero stuffing.

    For M <= L the output rate does not bind and the result is duc.design(L, of) itself, bit for bit (that one rounds
    the unit-gain prototype to float32 before it applies the gain)."""
    L, M = _check_ratio(interpolation, decimation)
    of = float(occupied_fraction)
    if not 0.0 < of <= 1.0:
        raise ValueError("occupied_fraction must be in (0, 1]")
    if of * M > L:
        raise ValueError("a link that fills %g of the modem's band is wider than the band at L / M = %d / %d" % (of, L, M))
    if M <= L:
        return duc.design(L, of, transition)
    e = of / (2.0 * L)
    if transition is None:
        transition = max(0.5 * (min(1.0 / L, 1.0 / M) - 2.0 * e), ddc._MIN_TRANSITION)
    transition = float(transition)
    if firdes.compute_ntaps(1.0, transition) > MAX_TAPS:
        raise ValueError("transition %g needs more than %d taps" % (transition, MAX_TAPS))
    cutoff = min(e + 0.5 * transition, 0.5)
    return np.asarray(firdes.low_pass(float(L), 1.0, cutoff, transition, firdes.WIN_HAMMING), np.float32)


def phase_step(center_freq):
    """D of the definition: frac(fc) in units of 2^-64 turn, truncated; a fraction that rounds up to 1 is 0."""
    t = float(center_freq)
    t -= math.floor(t)
    return int(t * 2.0 ** 64) if t < 1.0 else 0


def history(ntaps, interpolation):
    """Q of the definition: the inputs before the current one that an output can reach."""
    return (int(ntaps) - 1) // int(interpolation)


def tx_resamp_cfg(interpolation, decimation, center_freq=0.0, taps=None, occupied_fraction=None, transition=None,
                  out_format="fc32", out_scale=None):
    """ofdm_tx_resamp_cfg for Engine.set_tx_resamp; ``taps=None`` designs them from ``occupied_fraction``.
    ``out_format`` is "fc32" or "sc16" (``out_scale`` None: 2^15)."""
    cfg = ddc._cfg_with_taps(_abi.ofdm_tx_resamp_cfg, "tx_resamp_cfg", MAX_TAPS, taps, occupied_fraction,
                             lambda: design(interpolation, decimation, occupied_fraction, transition))
    cfg.interpolation = int(interpolation)
    cfg.decimation = int(decimation)
    cfg.out_format = iqio.FORMATS.index(iqio.check_format(out_format))
    cfg.center_freq = float(center_freq)
    cfg.out_scale = 0.0 if out_scale is None else iqio.check_scale(out_scale, iqio.TX_SCALE)
    return cfg
