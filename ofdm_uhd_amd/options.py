"""Option objects with the reference's attribute names and defaults.

The reference gathers its flags with optparse + GNU Radio's ``eng_option``; each
layer contributes an ``add_options(normal, expert)`` static method
(ofdm.py:150-163,263-276; transmit_path.py:72-79; receive_path.py:45-48;
benchmark_ofdm_tx.py:62-70; benchmark_ofdm_rx.py:62-69).  ``default_options``
gives the same attribute set without a command line.
"""
import optparse


def _eng_float(option, opt, value):
    """GNU Radio eng_notation: 1k, 2.5M, 10m ... (eng_option's ``eng_float``)."""
    scale = {'T': 1e12, 'G': 1e9, 'M': 1e6, 'k': 1e3, 'm': 1e-3, 'u': 1e-6, 'n': 1e-9, 'p': 1e-12}
    try:
        if value and value[-1] in scale:
            return float(value[:-1]) * scale[value[-1]]
        return float(value)
    except ValueError:
        raise optparse.OptionValueError("option %s: invalid engineering notation value: %r" % (opt, value))


def _intx(option, opt, value):
    try:
        return int(value, 0)
    except ValueError:
        raise optparse.OptionValueError("option %s: invalid integer value: %r" % (opt, value))


class eng_option(optparse.Option):
    TYPES = optparse.Option.TYPES + ("eng_float", "intx")
    TYPE_CHECKER = dict(optparse.Option.TYPE_CHECKER)
    TYPE_CHECKER["eng_float"] = _eng_float
    TYPE_CHECKER["intx"] = _intx


def add_resamp_options(parser):
    """--resamp-interp / --resamp-decim / --resamp-freq: the source is a wideband capture at decim / interp times the
    modem's rate (no integer multiple needed); resample.py, Engine.resamp."""
    parser.add_option("", "--resamp-interp", type="intx", default=0,
                      help="with --resamp-decim: the capture runs at decim / interp times the modem's rate; tune and "
                           "resample it on the GPU first (0 = off) [default=%default]")
    parser.add_option("", "--resamp-decim", type="intx", default=0,
                      help="decimation of the rational-rate front end, 1..64 (0 = off) [default=%default]")
    parser.add_option("", "--resamp-freq", type="eng_float", default=0.0,
                      help="with --resamp-interp / --resamp-decim: centre of the link in the capture, cycles per "
                           "sample in [-0.5, 0.5] [default=%default]")


def resamp_from_options(options):
    """dict(interpolation=, decimation=, center_freq=) from --resamp-*, None where the flags are unset or 0; one of
    the two ratios alone means the other is 1."""
    L, M = getattr(options, "resamp_interp", None), getattr(options, "resamp_decim", None)
    if not L and not M:
        return None
    return dict(interpolation=int(L or 1), decimation=int(M or 1),
                center_freq=float(getattr(options, "resamp_freq", 0.0) or 0.0))


def add_tx_resamp_options(parser):
    """--tx-resamp-interp / --tx-resamp-decim / --tx-resamp-freq: the sink is a wideband band at interp / decim times
    the modem's rate (no integer multiple needed); tx_resample.py, Engine.tx_resamp."""
    parser.add_option("", "--tx-resamp-interp", type="intx", default=0,
                      help="with --tx-resamp-decim: write a wideband IQ file at interp / decim times the modem's rate; "
                           "resample and shift the signal on the GPU (0 = off) [default=%default]")
    parser.add_option("", "--tx-resamp-decim", type="intx", default=0,
                      help="decimation of the rational-rate transmit stage, 1..64 (0 = off) [default=%default]")
    parser.add_option("", "--tx-resamp-freq", type="eng_float", default=0.0,
                      help="with --tx-resamp-interp / --tx-resamp-decim: centre of the link in the wideband file, "
                           "cycles per sample in [-0.5, 0.5] [default=%default]")


def tx_resamp_from_options(options):
    """dict(interpolation=, decimation=, center_freq=) from --tx-resamp-*, None where the flags are unset or 0; one of
    the two ratios alone means the other is 1."""
    L, M = getattr(options, "tx_resamp_interp", None), getattr(options, "tx_resamp_decim", None)
    if not L and not M:
        return None
    return dict(interpolation=int(L or 1), decimation=int(M or 1),
                center_freq=float(getattr(options, "tx_resamp_freq", 0.0) or 0.0))


def psd_from_options(options):
    """dict(nfft=, hop=[, spacing=]) from --psd "NFFT[,HOP]" and --psd-spacing, None where --psd is unset; ValueError
    for anything that is not one or two integers."""
    text = getattr(options, "psd", None)
    if not text:
        return None
    parts = str(text).split(",")
    if len(parts) not in (1, 2):
        raise ValueError("--psd takes NFFT or NFFT,HOP")
    nfft = int(parts[0])
    out = dict(nfft=nfft, hop=int(parts[1]) if len(parts) == 2 else None)
    spacing = getattr(options, "psd_spacing", None)
    if spacing is not None:
        out["spacing"] = float(spacing)
    return out


def default_options(**overrides):
    """An options object carrying every hot-path flag at the reference's default."""
    v = optparse.Values()
    v.modulation = "bpsk"        # ofdm.py:154
    v.fft_length = 512           # ofdm.py:156
    v.occupied_tones = 200       # ofdm.py:158
    v.cp_length = 128            # ofdm.py:160
    v.tx_amplitude = 0.250       # transmit_path.py:73
    v.samples_per_symbol = 2     # transmit_path.py:75
    v.verbose = False
    v.log = False
    v.snr = 30                   # benchmark_ofdm_rx.py:64
    v.size = 1024                # benchmark_ofdm_tx.py:64
    v.megabytes = 1.0            # benchmark_ofdm_tx.py:65
    v.discontinuous = False
    v.from_file = None
    for k, val in overrides.items():
        setattr(v, k, val)
    return v
