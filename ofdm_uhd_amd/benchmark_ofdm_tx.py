#!/usr/bin/env python3
"""benchmark_ofdm_tx: packet source -> transmit_path -> IQ file.

Mirror of the reference's benchmark_ofdm_tx.py (:38-126) with the USRP sink swapped
for a file sink (``--to-file``): the first 20 packets carry "This is Garbage data",
then the input file is sent in chunks of ``size - 2`` bytes; every payload is
``!H pktno | !H 0 | data`` (benchmark_ofdm_tx.py:111-117).
"""
import os
import struct
import sys
from optparse import OptionParser

import numpy as np

from . import dpd, iqio, ofdm, options as _options, spectrum, transmit_path


def build_payloads(options, data_source=None):
    """The reference's packet loop (benchmark_ofdm_tx.py:97-124) as a generator."""
    nbytes = int(10e6 * options.megabytes)   # sic: 1 "megabyte" = 10e6 bytes (:97)
    n = 0
    pktno = 0
    pkt_size = int(options.size)
    preamble = 0
    while n < nbytes:
        if pktno < 20:
            data = b"This is Garbage data"
        else:
            data = data_source.read(pkt_size - 2) if data_source is not None else b''
            if data == b'':
                break
        payload = struct.pack('!H', pktno & 0xffff) + struct.pack('!H', preamble & 0xffff) + data
        yield payload
        n += len(payload)
        pktno += 1


def make_parser():
    parser = OptionParser(option_class=_options.eng_option, conflict_handler="resolve")
    expert_grp = parser.add_option_group("Expert")
    parser.add_option("-s", "--size", type="eng_float", default=1024, help="set packet size [default=%default]")
    parser.add_option("-M", "--megabytes", type="eng_float", default=1.0,
                      help="set megabytes to transmit [default=%default]")
    parser.add_option("", "--discontinuous", action="store_true", default=False, help="enable discontinuous mode")
    parser.add_option("", "--from-file", default=None, help="use file for packet contents")
    parser.add_option("", "--to-file", default="ofdm_tx.dat", help="write the modulated IQ here [default=%default]")
    parser.add_option("", "--iq-format", type="choice", choices=list(iqio.FORMATS), default="fc32",
                      help="sample format of the IQ file: fc32 (interleaved float32) or sc16 (interleaved int16, the "
                           "format of rx_samples_to_file and most capture tools) [default=%default]")
    parser.add_option("", "--iq-scale", type="eng_float", default=None,
                      help="with sc16: full scale (int16 = rint(sample * scale), saturating) [default=2^15]")
    parser.add_option("", "--duc-interp", type="intx", default=0,
                      help="write a wideband IQ file at this multiple of the modem's rate: interpolate and shift the "
                           "signal on the GPU (the radio's set_interp; 0 = off) [default=%default]")
    parser.add_option("", "--duc-freq", type="eng_float", default=0.0,
                      help="with --duc-interp: centre of the link in the wideband file, cycles per sample in "
                           "[-0.5, 0.5] (the radio's set_center_freq over the file's rate) [default=%default]")
    parser.add_option("", "--cfr-papr", type="eng_float", default=None,
                      help="crest-factor reduction as the last stage, on the GPU: pull every peak down to this many dB "
                           "above the level of the data symbols by a smooth dip of the gain; the figures (PAPR in and "
                           "out, EVM) are printed at the end [default=off]")
    parser.add_option("", "--cfr-half-width", type="intx", default=16,
                      help="with --cfr-papr: half-width of the gain dip in samples, 0 to 511 (0: polar clip); the "
                           "stream comes out this many samples late [default=%default]")
    parser.add_option("", "--dpd", default=None, metavar="FILE.npy",
                      help="digital predistortion as the last stage, behind --cfr-papr, on the GPU: the memory-polynomial "
                           "table of shape (memory, orders) in this .npy file (dpd.train / dpd.fit), which holds for the "
                           "--tx-amplitude and --cfr-papr it was trained at; gain, peak expansion and the share of "
                           "samples above full scale are printed at the end [default=off]")
    parser.add_option("", "--psd", default=None, metavar="NFFT[,HOP]",
                      help="measure the spectrum of what is written, on the GPU: a Welch estimate over segments of NFFT "
                           "samples (a power of two, 64 to 4096) at hop HOP (NFFT / 2); occupied bandwidth and, behind "
                           "--duc-interp / --tx-resamp-*, the adjacent-channel leakage ratio are printed at the end "
                           "[default=off]")
    parser.add_option("", "--psd-spacing", type="eng_float", default=None, metavar="F",
                      help="with --psd: distance of the adjacent channels in cycles per sample of the written stream "
                           "[default=the modem's rate]")
    parser.add_option("", "--psd-out", default=None, metavar="FILE.npy",
                      help="with --psd: save the density in ascending frequency [default=off]")
    parser.add_option("", "--fec", action="store_true", default=False,
                      help="coded link: protect every payload (at most 2040 bytes) with the rate-1/2 K=7 convolutional "
                           "code and interleaver, encoded on the GPU; demodulate with benchmark_ofdm_rx --fec "
                           "[default=%default]")
    parser.add_option("", "--fec-rate", type="choice", choices=("1/2", "2/3", "3/4", "5/6"), default=None,
                      help="coded link at this rate: the K=7 code punctured by the 802.11 patterns (implies --fec; "
                           "demodulate with the same benchmark_ofdm_rx --fec-rate) [default=1/2]")
    parser.add_option("", "--ldpc", action="store_true", default=False,
                      help="coded link with the other inner code, in the place of --fec: protect every payload (at "
                           "most 2012 bytes) with the rate-1/2 QC-LDPC code, encoded on the GPU; demodulate with "
                           "benchmark_ofdm_rx --ldpc or --ldpc-soft [default=%default]")
    parser.add_option("", "--ldpc-rate", type="choice", choices=("1/2", "2/3", "3/4", "5/6"), default=None,
                      help="--ldpc with the QC-LDPC code of this rate (payloads of at most 2012, 2684, 3020 or 3356 bytes; "
                           "demodulate with the same benchmark_ofdm_rx --ldpc-rate) [default=1/2]")
    parser.add_option("", "--rs", action="store_true", default=False,
                      help="outer code: wrap every payload (at most 3564 bytes, 1780 with --fec / --fec-rate, 1752 with --ldpc, "
                           "2328 / 2632 / 2904 with --ldpc-rate 2/3 / 3/4 / 5/6) in a "
                           "Reed-Solomon block, 32 parity bytes per 223, encoded on the GPU ahead of the inner code; "
                           "demodulate with benchmark_ofdm_rx --rs [default=%default]")
    parser.add_option("", "--sig", action="store_true", default=False,
                      help="self-describing coded link: every block goes out behind a 12-byte signal field that names "
                           "its coding -- the one --fec / --fec-rate / --ldpc / --ldpc-rate / --rs choose, none of them: "
                           "uncoded -- so benchmark_ofdm_rx --sig needs no coding flags; the largest payloads shrink by "
                           "up to 12 bytes [default=%default]")
    _options.add_tx_resamp_options(parser)
    parser.add_option("", "--tx-resamp-freqs", default=None,
                      help="with --tx-resamp-interp / --tx-resamp-decim, instead of --tx-resamp-freq: comma-separated "
                           "centres of ALL links of the band; every link carries the packet stream and they are placed "
                           "on the band in one pass on the GPU (ofdm_mod_resamp_bank) [default=off]")
    transmit_path.transmit_path.add_options(parser, expert_grp)
    ofdm.ofdm_mod.add_options(parser, expert_grp)
    return parser


BANK_BATCH = 16   # packets per link between two flushes of the bank


def _main_tx_resamp_bank(parser, options):
    """--tx-resamp-freqs: the packet stream on every link of one ofdm_mod_resamp_bank, the band to --to-file; returns
    the packets sent per link."""
    if options.duc_interp or options.duc_freq:
        parser.error("--tx-resamp-freqs does not combine with --duc-interp or --duc-freq")
    if options.fec or options.rs or options.ldpc or options.sig:
        parser.error("--tx-resamp-freqs does not combine with --fec, --ldpc, --rs or --sig")
    if options.cfr_papr is not None:
        parser.error("--tx-resamp-freqs does not combine with --cfr-papr")
    if options.dpd is not None:
        parser.error("--tx-resamp-freqs does not combine with --dpd")
    if options.psd is not None:
        parser.error("--tx-resamp-freqs does not combine with --psd")
    if options.tx_resamp_freq:
        parser.error("--tx-resamp-freqs and --tx-resamp-freq are mutually exclusive")
    if not options.tx_resamp_interp and not options.tx_resamp_decim:
        parser.error("--tx-resamp-freqs needs --tx-resamp-interp / --tx-resamp-decim")
    try:
        freqs = [float(f) for f in options.tx_resamp_freqs.split(",")]
    except ValueError:
        parser.error("--tx-resamp-freqs takes comma-separated numbers")
    L, M = int(options.tx_resamp_interp or 1), int(options.tx_resamp_decim or 1)  # (one of the two alone: the other is 1)
    try:
        bank = ofdm.ofdm_mod_resamp_bank(options, freqs, L, M, iq_format=options.iq_format, iq_scale=options.iq_scale)
    except ValueError as e:
        parser.error("--tx-resamp-freqs: %s" % e)
    src = open(options.from_file, 'rb') if options.from_file is not None else None
    if src is not None:
        print(os.path.getsize(options.from_file))
    sink = iqio.file_sink(options.to_file, fmt=options.iq_format)
    try:
        for m in bank.links():
            m.engine().set_tx_amplitude(min(max(options.tx_amplitude, 0.0), 1))
        npk = 0
        for payload in build_payloads(options, src):
            for i in range(len(freqs)):
                bank.send_pkt(i, payload)
            sys.stderr.write('.')
            npk += 1
            if npk % BANK_BATCH == 0:
                sink.write(bank.flush())
        iq = bank.flush(end=True)
        if iq is not None:
            sink.write(iq)
        symbols = sum(m.symbols_sent for m in bank.links())
    finally:
        sink.close()
        bank.close()
    sys.stderr.write("\n%d packets on each of %d links, %d symbols -> %s\n" % (npk, len(freqs), symbols, options.to_file))
    return npk


def main(argv=None):
    parser = make_parser()
    (options, args) = parser.parse_args(argv)
    if len(args) != 0:
        parser.print_help()
        sys.exit(1)
    if options.fec_rate:
        options.fec = dict(rate=options.fec_rate)   # (what transmit_path hands to ofdm_mod(fec=))
    if options.ldpc_rate:
        options.ldpc = dict(rate=options.ldpc_rate)   # (what transmit_path hands to ofdm_mod(ldpc=))
    if options.ldpc and options.fec:
        parser.error("--ldpc / --ldpc-rate take the place of --fec / --fec-rate: a link has one inner code")
    if options.tx_resamp_freqs is not None:
        return _main_tx_resamp_bank(parser, options)

    src = open(options.from_file, 'rb') if options.from_file is not None else None
    if src is not None:
        print(os.path.getsize(options.from_file))

    dpd_stage = None
    if options.dpd is not None:
        try:
            # the converter's full scale in the stream's units: 1, or what --iq-scale maps onto 2^15
            full = 32768.0 / options.iq_scale if options.iq_format == "sc16" and options.iq_scale else 1.0
            dpd_stage = dict(coef=dpd.load_coef(options.dpd), limit=full)
        except (OSError, ValueError) as e:
            parser.error("--dpd: %s" % e)
    if (options.psd_spacing is not None or options.psd_out) and options.psd is None:
        parser.error("--psd-spacing / --psd-out need --psd")
    try:
        psd_stage = _options.psd_from_options(options)
        if psd_stage is not None:
            spectrum.psd_cfg(psd_stage["nfft"], psd_stage["hop"])
    except ValueError as e:
        parser.error("--psd: %s" % e)
    try:
        txpath = transmit_path.transmit_path(options, dpd=dpd_stage, spectrum=psd_stage)
    except ValueError as e:
        if options.cfr_papr is None:
            raise
        parser.error("--cfr-papr / --cfr-half-width: %s" % e)
    sink = iqio.file_sink(options.to_file, fmt=options.iq_format)   # (transmit_path takes the format, --fec, --rs and --duc-interp / --duc-freq, --tx-resamp-* from the options)
    txpath.connect(sink)
    npk = 0
    for payload in build_payloads(options, src):
        txpath.send_pkt(payload)
        sys.stderr.write('.')
        npk += 1
    txpath.send_pkt(eof=True)
    sink.close()
    sys.stderr.write("\n%d packets, %d symbols -> %s\n" % (npk, txpath.ofdm_tx.symbols_sent, options.to_file))
    r = txpath.ofdm_tx.last_cfr
    if r is not None:
        sys.stderr.write("cfr: PAPR %.2f -> %.2f dB, EVM %.1f dB, %.3g of the samples over the threshold, %.3g touched\n" % (
            r["papr_in_db"], r["papr_out_db"], r["evm_db"], r["share_over"], r["share_touched"]))
    r = txpath.ofdm_tx.last_dpd
    if r is not None:
        sys.stderr.write("dpd: gain %.2f dB, peak expansion %.2f dB, %.3g of the samples above full scale\n" % (
            r["gain_db"], r["peak_expansion_db"], r["share_over"]))
    r = txpath.ofdm_tx.last_spectrum
    if r is not None:
        aclr = "" if r.get("aclr_db") is None else ", ACLR lower %.2f / upper %.2f dB" % r["aclr_db"]
        sys.stderr.write("psd: %d segments of %d, power %.4g, occupied bandwidth (99 %%) %.5f%s\n" % (
            r["nseg"], r["nfft"], r["power"], r["obw"], aclr))
        if options.psd_out:
            np.save(options.psd_out, spectrum.ascending(r["density"]))
    return npk


if __name__ == '__main__':
    try:
        main()
    except KeyboardInterrupt:
        pass
