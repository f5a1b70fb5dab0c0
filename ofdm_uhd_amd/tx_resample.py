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

from . import _abi, ddc, duc, firdes, resample

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
    return ddc._set_out_format(cfg, out_format, out_scale, center_freq)


MAX_LINKS = _abi.OFDM_TX_RESAMP_BANK_MAX_LINKS


def bank_phase_steps(center_freq, interpolation, decimation):
    """(G, E, D) of the bank's definition, each in units of 2^-64 turn: G = turns(fc / M), the phase per step of the
    L-times grid (fc / M is ONE double division, the one the table c[k] = h[k] exp(j 2 pi fc k / M) makes),
    E = L G mod 2^64 per input and D = M G mod 2^64 per output.  With n M = k + m L, k G + m E = n D modulo 2^64."""
    L, M = _check_ratio(interpolation, decimation)
    G = phase_step(float(center_freq) / float(M))
    return G, (L * G) & (2 ** 64 - 1), (M * G) & (2 ** 64 - 1)


def bank_cfg(interpolation, decimation, center_freqs, taps=None, occupied_fraction=None, transition=None,
             out_format="fc32", out_scale=None):
    """ofdm_tx_resamp_bank_cfg for Engine.set_tx_resamp_bank: one ratio and one prototype, one centre frequency per
    link (1 to MAX_LINKS of them, each in [-0.5, 0.5] cycles per wideband sample; equal ones are allowed), row i of
    Engine.tx_resamp_bank's input at center_freqs[i].  ``taps=None`` designs the prototype from ``occupied_fraction``
    as tx_resamp_cfg does; ``out_format`` / ``out_scale`` are tx_resamp_cfg's.  ValueError for a ratio outside 1..64,
    with given taps too."""
    L, M = _check_ratio(interpolation, decimation)
    cfg = ddc._bank_cfg_with_taps(_abi.ofdm_tx_resamp_bank_cfg, "transmit resampler bank", MAX_LINKS, center_freqs,
                                  MAX_TAPS, taps, occupied_fraction,
                                  lambda: design(interpolation, decimation, occupied_fraction, transition), finite=True)
    cfg.interpolation = L
    cfg.decimation = M
    return ddc._set_out_format(cfg, out_format, out_scale)
