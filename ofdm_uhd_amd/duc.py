"""Wideband transmit: place this modem's signal at an offset inside a band L times as wide.

The reference leaves this to its radio (``sink.set_interp`` / ``set_center_freq`` in usrp_transmit_path.py,
``generic_usrp.set_interp``, the two-channel transmitter of dual_channel/dual_channel.py); with files and arrays in
the radio's place the stage is a polyphase interpolating FIR followed by a frequency shift, run on the GPU by
``Engine.duc`` (csrc/duc.h) -- the mirror image of ddc.py.  This module holds the host side: the low-pass design and
the configuration struct.

Frequencies are in cycles per OUTPUT (wideband) sample.
"""
import numpy as np

from . import _abi, ddc

MAX_TAPS = _abi.OFDM_DUC_MAX_TAPS
MAX_INTERP = 64
MAX_LINKS = _abi.OFDM_DUC_BANK_MAX_LINKS


def design(interpolation, occupied_fraction, transition=None):
    """Real low-pass prototype at the wideband rate for a link that fills ``occupied_fraction`` of the modem's band
    (occupied_tones / fft_length): ``L * ddc.design(L, ...)`` as float32, odd length.

    The image geometry is the decimator's alias geometry: the signal's edge lies at occupied_fraction / (2L), the first
    image that zero stuffing creates begins at 1/L - occupied_fraction / (2L).  The factor L restores unit pass-band
    gain after zero stuffing (each polyphase branch sums to about 1)."""
    L = int(interpolation)
    if not 1 <= L <= MAX_INTERP:
        raise ValueError("interpolation must be in [1, %d]" % MAX_INTERP)
    return (np.float32(L) * ddc.design(L, occupied_fraction, transition)).astype(np.float32)


def duc_cfg(interpolation, center_freq, taps=None, occupied_fraction=None, transition=None, out_format="fc32",
            out_scale=None):
    """ofdm_duc_cfg for Engine.set_duc; ``taps=None`` designs them from ``occupied_fraction``.  ``out_format`` is
    "fc32" or "sc16" (``out_scale`` None: 2^15)."""
    cfg = ddc._cfg_with_taps(_abi.ofdm_duc_cfg, "duc_cfg", MAX_TAPS, taps, occupied_fraction,
                             lambda: design(interpolation, occupied_fraction, transition))
    cfg.interpolation = int(interpolation)
    return ddc._set_out_format(cfg, out_format, out_scale, center_freq)


def bank_cfg(interpolation, center_freqs, taps=None, occupied_fraction=None, transition=None, out_format="fc32",
             out_scale=None):
    """ofdm_duc_bank_cfg for Engine.set_duc_bank: one interpolation and one prototype, one centre frequency per link
    (1 to MAX_LINKS of them, each in [-0.5, 0.5] cycles per wideband sample; equal ones are allowed), row i of
    Engine.duc_bank's input at center_freqs[i].  ``taps=None`` designs the prototype from ``occupied_fraction`` as
    duc_cfg does; ``out_format`` / ``out_scale`` are duc_cfg's."""
    cfg = ddc._bank_cfg_with_taps(_abi.ofdm_duc_bank_cfg, "DUC bank", MAX_LINKS, center_freqs, MAX_TAPS, taps,
                                  occupied_fraction, lambda: design(interpolation, occupied_fraction, transition),
                                  finite=True)
    cfg.interpolation = int(interpolation)
    if not 1 <= cfg.interpolation <= MAX_INTERP:
        raise ValueError("interpolation must be in [1, %d]" % MAX_INTERP)
    return ddc._set_out_format(cfg, out_format, out_scale)
