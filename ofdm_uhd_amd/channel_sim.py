#!/usr/bin/env python3
"""channel_sim: IQ file -> propagation channel on the GPU -> IQ file.

Sits between benchmark_ofdm_tx (``--to-file tx.dat``) and benchmark_ofdm_rx (``--from-file rx.dat``) exactly where
the reference has the air between its two radios: delayed paths with complex gains and Doppler shifts, continuous
tones, a carrier offset and noise (multipath.py, Engine.multipath).  The output is the input's length plus the longest
delay: the echoes' tail comes out.  ``--chunk-samples`` streams the file through the stage; the output is the same
bits whatever the chunking.
"""
import sys
from optparse import OptionParser

import numpy as np

from . import dpd, iqio, multipath, options as _options


def make_parser():
    parser = OptionParser(option_class=_options.eng_option, conflict_handler="resolve")
    parser.add_option("", "--from-file", default="ofdm_tx.dat", help="IQ file to send through the channel [default=%default]")
    parser.add_option("", "--to-file", default="ofdm_rx.dat", help="write the received IQ here [default=%default]")
    parser.add_option("", "--paths", default="0:1",
                      help="paths as delay:gain[@doppler] separated by ';' -- delay in samples (0..1023), gain a complex "
                           "number, doppler in cycles per sample -- e.g. \"0:1;4:0.35+0.35j;9:0.1@1e-4\" [default=%default]")
    parser.add_option("", "--pa", default=None, metavar="example|FILE.npy",
                      help="a power amplifier in front of the paths, on the GPU: the memory-polynomial model whose table of "
                           "shape (memory, orders) this .npy file holds, or the built-in example (dpd.example_pa); its "
                           "gain and peak expansion are printed at the end [default=off]")
    parser.add_option("", "--tones", default="",
                      help="continuous tones as amp:freq[@phase] separated by ';' -- freq in cycles per sample "
                           "[-0.5, 0.5], phase in cycles -- e.g. \"0.01:0.15625\" [default=none]")
    parser.add_option("", "--snr", type="eng_float", default=None,
                      help="add noise this many dB below the signal, whose power is measured over the input file's "
                           "NON-ZERO samples (the silence around the packets does not count) [default=no noise]")
    parser.add_option("", "--cfo-bins", type="eng_float", default=0.0,
                      help="carrier offset in subcarrier spacings of --fft-length [default=%default]")
    parser.add_option("", "--fft-length", type="intx", default=512,
                      help="only turns --cfo-bins into radians per sample: 2 pi bins / fft-length [default=%default]")
    parser.add_option("", "--iq-format", type="choice", choices=list(iqio.FORMATS), default="fc32",
                      help="sample format of both files: fc32 (interleaved float32) or sc16 (interleaved int16) "
                           "[default=%default]")
    parser.add_option("", "--iq-scale", type="eng_float", default=None,
                      help="with sc16: full scale of both files (int16 = rint(sample * scale), saturating) [default=2^15]")
    parser.add_option("", "--chunk-samples", type="eng_float", default=0,
                      help="stream the file through the channel in chunks of this many samples (0 = one call on the "
                           "whole file) [default=%default]")
    parser.add_option("", "--seed", type="intx", default=0xC0FFEE, help="seed of the noise [default=%default]")
    return parser


def _complex(piece, fmt, scale):
    return iqio.from_sc16(piece, 1.0 / scale) if fmt == "sc16" else piece


POWER_CHUNK = 1 << 20     # the power is summed in pieces of this size whatever --chunk-samples: one sigma per file


def signal_power(source, fmt, scale):
    """Mean |x|^2 over the file's non-zero samples (0.0 for a file of zeros)."""
    total, count = 0.0, 0
    for piece in source.read_chunks(POWER_CHUNK):
        x = _complex(piece, fmt, scale).astype(np.complex128)
        p = x.real * x.real + x.imag * x.imag
        total += float(np.sum(p))
        count += int(np.count_nonzero(p))
    return total / count if count else 0.0


def main(argv=None):
    parser = make_parser()
    (options, args) = parser.parse_args(argv)
    if len(args) != 0:
        parser.print_help(sys.stderr)
        sys.exit(1)
    chunk = int(options.chunk_samples)
    if chunk < 0:
        parser.error("--chunk-samples must not be negative")
    if int(options.fft_length) < 1:
        parser.error("--fft-length must be positive")
    try:
        scale = iqio.check_scale(options.iq_scale, iqio.TX_SCALE)
        paths, tones = multipath.parse(options.paths), multipath.parse_tones(options.tones)
        cfo = float(options.cfo_bins) * 2.0 * np.pi / int(options.fft_length)
        multipath.multipath_cfg(paths=paths, tones=tones, cfo=cfo)           # refused before a file is touched
    except ValueError as e:
        parser.error("--paths / --tones / --cfo-bins / --iq-scale: %s" % e)
    pa = None
    if options.pa is not None:
        try:
            pa = dpd.mempoly_cfg(dpd.example_pa() if options.pa == "example" else dpd.load_coef(options.pa))
        except (OSError, ValueError) as e:
            parser.error("--pa: %s" % e)
    source = iqio.file_source(options.from_file, fmt=options.iq_format)
    sigma = 0.0
    if options.snr is not None:
        sigma = multipath.sigma_for_snr(float(options.snr), signal_power(source, options.iq_format, scale))
    cfg = multipath.multipath_cfg(paths=paths, tones=tones, sigma=sigma, cfo=cfo, seed=int(options.seed),
                                  out_format=options.iq_format, out_scale=scale)
    sink = iqio.file_sink(options.to_file, fmt=options.iq_format)
    ch = None
    nout = 0
    try:
        ch = multipath.channel(cfg)
        amplify = (lambda x: x) if pa is None else ch.engine().pa
        if pa is not None:
            ch.engine().set_pa(pa)
        if chunk:
            for piece in source.read_chunks(chunk):
                y = ch.feed(amplify(_complex(piece, options.iq_format, scale)))
                sink.write(y)
                nout += len(y)
            y = ch.flush()
        else:
            y = ch.work(amplify(_complex(source.read_all(), options.iq_format, scale)))
        sink.write(y)
        nout += len(y)
        if pa is not None and ch.engine().pa_stats()["n"]:
            r = dpd.report(ch.engine().pa_stats())
            print("channel_sim: amplifier gain %.2f dB, peak expansion %.2f dB" % (r["gain_db"], r["peak_expansion_db"]))
    finally:
        if ch is not None:
            ch.close()
        sink.close()
    print("channel_sim: %d samples out, %d paths, %d tones, sigma %.6g, cfo %.6g rad/sample" % (
        nout, cfg.npaths, cfg.ntones, cfg.sigma, cfg.cfo))
    return cfg


if __name__ == '__main__':
    try:
        main()
    except KeyboardInterrupt:
        pass
