"""Wideband receive for links on a uniform grid: the polyphase-FFT channeliser.

Where every link of a capture sits at a centre frequency c/M (cycles per wideband sample) and is decimated by M -- a
radio that watches every slot of a band and hops between them (dual_channel/dual_channel.py tunes one radio channel
per link; the sensing apps step through the band) -- the K filters of the DDC bank collapse into one real-tap polyphase
filter and an M-point transform per output index.  ``Engine.pfb`` (csrc/pfb.h) runs it on the GPU; this module holds
the host side: the prototype design and the configuration struct.  The transmit mirror, the synthesis bank
(``Engine.pfb_synth``, csrc/pfb_synth.h: K narrowband streams into one band in one pass), has its design and
configuration here too.

Channel c in [0, M) sits at c/M; c >= M/2 is the negative frequency (c - M)/M.
"""
import numpy as np

from . import _abi, ddc, duc

MAX_CHANNELS = _abi.OFDM_PFB_MAX_CHANNELS
MAX_TAPS = _abi.OFDM_PFB_MAX_TAPS
CHANNEL_COUNTS = (2, 4, 8, 16, 32, 64)


def design(nchannels, occupied_fraction, transition=None):
    """Real low-pass prototype at the wideband rate for links that fill ``occupied_fraction`` of one channel:
    ``ddc.design`` at decimation M (the alias geometry of a critically sampled channeliser is the DDC's at R = M)."""
    return ddc.design(nchannels, occupied_fraction, transition)


def pfb_cfg(nchannels, channels=None, taps=None, occupied_fraction=None, transition=None):
    """ofdm_pfb_cfg for Engine.set_pfb: M = ``nchannels`` (2, 4, ..., 64) channels, of which ``channels`` are kept, in
    that order (None: all M in order; 1 to M entries, repeats allowed).  A channel may be given signed, in
    [-M/2, M/2): it is taken mod M.  ``taps=None`` designs the prototype from ``occupied_fraction``."""
    M = int(nchannels)
    if M not in CHANNEL_COUNTS or M != nchannels:
        raise ValueError("nchannels must be one of %s" % (CHANNEL_COUNTS,))
    if channels is None:
        channels = range(M)
    chans = [int(c) for c in np.asarray(list(channels)).reshape(-1)]
    if not 1 <= len(chans) <= M:
        raise ValueError("a channeliser keeps 1 to nchannels channels")
    if not all(-(M // 2) <= c < M for c in chans):
        raise ValueError("channels must lie in [-M/2, M)")
    cfg = ddc._cfg_with_taps(_abi.ofdm_pfb_cfg, "pfb_cfg", MAX_TAPS, taps, occupied_fraction,
                             lambda: design(M, occupied_fraction, transition), finite=True)
    cfg.nchannels = M
    cfg.nsel = len(chans)
    for i, c in enumerate(chans):
        cfg.channel[i] = c % M
    return cfg


def synth_design(nchannels, occupied_fraction, transition=None):
    """Real low-pass prototype at the wideband rate for the synthesis bank: ``duc.design`` at interpolation M (the
    image geometry of a critically sampled bank is the DUC's at L = M; gain M in the pass band)."""
    return duc.design(nchannels, occupied_fraction, transition)


def synth_cfg(nchannels, channels, taps=None, occupied_fraction=None, transition=None, out_format="fc32",
              out_scale=None):
    """ofdm_pfb_synth_cfg for Engine.set_pfb_synth: M = ``nchannels`` (2, 4, ..., 64) channels, of which ``channels``
    carry a link, row i of Engine.pfb_synth's input on channels[i] (None: all M in order; 1 to M entries, all
    different).  A channel may be given signed, in [-M/2, M/2): it is taken mod M.  ``taps=None`` designs the prototype
    from ``occupied_fraction``.  ``out_format`` is "fc32" or "sc16" (``out_scale`` None: 2^15)."""
    M = int(nchannels)
    if M not in CHANNEL_COUNTS or M != nchannels:
        raise ValueError("nchannels must be one of %s" % (CHANNEL_COUNTS,))
    if channels is None:
        channels = range(M)
    chans = [int(c) for c in np.asarray(list(channels)).reshape(-1)]
    if not 1 <= len(chans) <= M:
        raise ValueError("a synthesis bank carries 1 to nchannels channels")
    if not all(-(M // 2) <= c < M for c in chans):
        raise ValueError("channels must lie in [-M/2, M)")
    chans = [c % M for c in chans]
    if len(set(chans)) != len(chans):
        raise ValueError("a synthesis bank's channels must all be different (mod nchannels)")
    cfg = ddc._cfg_with_taps(_abi.ofdm_pfb_synth_cfg, "synth_cfg", MAX_TAPS, taps, occupied_fraction,
                             lambda: synth_design(M, occupied_fraction, transition), finite=True)
    cfg.nchannels = M
    cfg.nsel = len(chans)
    for i, c in enumerate(chans):
        cfg.channel[i] = c
    return ddc._set_out_format(cfg, out_format, out_scale)
