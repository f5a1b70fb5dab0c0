"""Wideband receive front end: tune to one link of a wider capture and decimate to the modem's rate.

The reference leaves this to its radio (``usrp2.source_32fc.set_decim`` / ``set_center_freq`` in
usrp_receive_path.py, predictive_sense.py, dual_channel/dual_channel.py); with files and arrays in the
radio's place the stage is GNU Radio's ``gr.freq_xlating_fir_filter_ccf(decimation, taps, center_freq,
sampling_freq)``, run on the GPU by ``Engine.ddc`` (csrc/ddc.h).  This module holds the host side: the
low-pass design, the normative band-pass table and the configuration struct.

Frequencies are in cycles per INPUT (wideband) sample.
"""
import ctypes as C

import numpy as np

from . import _abi, firdes, iqio

MAX_TAPS = _abi.OFDM_DDC_MAX_TAPS
MAX_DECIM = 64
MAX_LINKS = _abi.OFDM_DDC_BANK_MAX_LINKS
# narrowest transition gr.firdes.low_pass turns into at most MAX_TAPS taps: int(53 / (22 w)) forced odd <= 1023
_MIN_TRANSITION = 53.0 / (22.0 * (MAX_TAPS - 0.5))


def design(decimation, occupied_fraction, transition=None):
    """Real low-pass prototype at the wideband rate for a link that fills ``occupied_fraction`` of the band that
    remains after decimation (occupied_tones / fft_length): ``firdes.low_pass`` taps as float32, odd length.

    The signal's edge lies at occupied_fraction / (2R); the first spectrum that folds onto it after decimation begins
    at 1/R - occupied_fraction / (2R).  Default transition: half that gap, (1 - occupied_fraction) / (2R), widened
    where needed so that ntaps <= OFDM_DDC_MAX_TAPS.  The pass-band edge handed to low_pass (its 6 dB point) is the
    signal's edge plus half the transition."""
    R = int(decimation)
    if not 1 <= R <= MAX_DECIM:
        raise ValueError("decimation must be in [1, %d]" % MAX_DECIM)
    of = float(occupied_fraction)
    if not 0.0 < of <= 1.0:
        raise ValueError("occupied_fraction must be in (0, 1]")
    if transition is None:
        transition = max((1.0 - of) / (2.0 * R), _MIN_TRANSITION)
    transition = float(transition)
    if firdes.compute_ntaps(1.0, transition) > MAX_TAPS:
        raise ValueError("transition %g needs more than %d taps" % (transition, MAX_TAPS))
    cutoff = min(of / (2.0 * R) + 0.5 * transition, 0.5)
    return np.asarray(firdes.low_pass(1.0, 1.0, cutoff, transition, firdes.WIN_HAMMING), np.float32)


def bandpass_taps(taps, fc, interpolation=1):
    """The normative table c[k] = complex64(h[k] exp(j 2 pi fc k / L)): float32 taps, float64 arithmetic, rounded
    once; L = 1 for the DDC and the bank (the division is then exact).  (``Engine.ddc_taps`` / ``resamp_taps`` return
    the table the kernel holds, computed the same way by the library's libm.)"""
    h = np.asarray(taps, np.float32).astype(np.float64)
    k = np.arange(len(h), dtype=np.float64)
    a = 2.0 * np.pi * float(fc) * k / float(int(interpolation))
    return (h * np.cos(a) + 1j * (h * np.sin(a))).astype(np.complex64)


def _cfg_with_taps(struct, who, max_taps, taps, occupied_fraction, design_taps, finite=False):
    """A zeroed ``struct`` (one of the ten stages' configurations) with struct_size, ntaps and taps filled in: the
    given taps as float32 or, with ``taps=None``, what ``design_taps()`` makes of ``occupied_fraction``.  ``finite``:
    the builder refuses taps that are not finite itself (the others leave that to the library)."""
    if taps is None:
        if occupied_fraction is None:
            raise ValueError("%s needs taps or occupied_fraction" % who)
        taps = design_taps()
    taps = np.ascontiguousarray(taps, np.float32).reshape(-1)
    if not 1 <= len(taps) <= max_taps:
        raise ValueError("ntaps must be in [1, %d]" % max_taps)
    if finite and not np.all(np.isfinite(taps)):
        raise ValueError("taps must be finite")
    cfg = struct()
    cfg.struct_size = C.sizeof(struct)
    cfg.ntaps = len(taps)
    C.memmove(cfg.taps, taps.ctypes.data, 4 * len(taps))
    return cfg


def _bank_cfg_with_taps(struct, bank, max_links, center_freqs, max_taps, taps, occupied_fraction, design_taps,
                        finite=False):
    """_cfg_with_taps for the four banks of links at arbitrary centre frequencies (``bank`` names the stage in the
    message): the list is normalised and checked first, against ``max_links`` and [-0.5, 0.5], and fills nlinks and
    center_freq[]."""
    fcs = [float(f) for f in np.asarray(center_freqs, np.float64).reshape(-1)]
    if not 1 <= len(fcs) <= max_links:
        raise ValueError("a %s has 1 to %d links" % (bank, max_links))
    if not all(abs(f) <= 0.5 for f in fcs):
        raise ValueError("center_freqs must lie in [-0.5, 0.5] cycles per sample")
    cfg = _cfg_with_taps(struct, "bank_cfg", max_taps, taps, occupied_fraction, design_taps, finite)
    cfg.nlinks = len(fcs)
    for i, f in enumerate(fcs):
        cfg.center_freq[i] = f
    return cfg


_NO_FC = object()


def _set_out_format(cfg, out_format, out_scale, center_freq=_NO_FC):
    """out_format ("fc32" or "sc16") and out_scale (None: the library's 2^15) of a transmit stage's configuration.
    The single stages hand their ``center_freq`` in as well: it is converted between the two checks, as ever."""
    cfg.out_format = iqio.FORMATS.index(iqio.check_format(out_format))
    if center_freq is not _NO_FC:
        cfg.center_freq = float(center_freq)
    cfg.out_scale = 0.0 if out_scale is None else iqio.check_scale(out_scale, iqio.TX_SCALE)
    return cfg


def ddc_cfg(decimation, center_freq, taps=None, occupied_fraction=None, transition=None):
    """ofdm_ddc_cfg for Engine.set_ddc; ``taps=None`` designs them from ``occupied_fraction``."""
    cfg = _cfg_with_taps(_abi.ofdm_ddc_cfg, "ddc_cfg", MAX_TAPS, taps, occupied_fraction,
                         lambda: design(decimation, occupied_fraction, transition))
    cfg.decimation = int(decimation)
    cfg.center_freq = float(center_freq)
    return cfg


def bank_cfg(decimation, center_freqs, taps=None, occupied_fraction=None, transition=None):
    """ofdm_ddc_bank_cfg for Engine.set_ddc_bank: one decimation and one prototype, one centre frequency per link
    (1 to MAX_LINKS of them, each in [-0.5, 0.5] cycles per wideband sample; equal ones are allowed).  ``taps=None``
    designs the prototype from ``occupied_fraction`` as ddc_cfg does."""
    cfg = _bank_cfg_with_taps(_abi.ofdm_ddc_bank_cfg, "DDC bank", MAX_LINKS, center_freqs, MAX_TAPS, taps,
                              occupied_fraction, lambda: design(decimation, occupied_fraction, transition))
    cfg.decimation = int(decimation)
    return cfg
