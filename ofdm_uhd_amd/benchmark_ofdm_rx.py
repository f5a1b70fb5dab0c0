#!/usr/bin/env python3
"""benchmark_ofdm_rx: IQ file -> receive_path -> packet accounting.

Mirror of the reference's benchmark_ofdm_rx.py (:35-87) with the USRP source swapped
for a file source (``--from-file``).  ``rx_callback`` is the reference's: payload[2:4]
must be 0, payload[0:2] is the packet number, packets above 19 are written to the
output file, ``n_rcvd`` / ``n_right`` are counted and printed (:50-61).
"""
import struct
import sys
from optparse import OptionParser

from . import config, iqio, ofdm, options as _options, receive_path


class rx_accounting(object):
    def __init__(self, packet_file=None, verbose=True):
        self.n_rcvd = 0
        self.n_right = 0
        self.packet_file = packet_file
        self.verbose = verbose

    def rx_callback(self, ok, payload, quality=None):
        if len(payload) < 4:
            return  # the reference would raise struct.error on a short payload
        (preamble,) = struct.unpack('!H', payload[2:4])
        if preamble == 0:
            self.n_rcvd += 1
            (pktno,) = struct.unpack('!H', payload[0:2])
            if pktno > 19 and self.packet_file is not None:
                self.packet_file.write(payload[4:])
            if ok:
                self.n_right += 1
            if self.verbose:
                line = "ok: %r \t pktno: %d \t n_rcvd: %d \t n_right: %d" % (ok, pktno, self.n_rcvd, self.n_right)
                if quality is not None:   # --link-quality
                    line += " \t snr_pre: %.1f \t snr_dd: %.1f \t cfo: %+.3f" % (
                        quality["snr_preamble_db"], quality["snr_decision_db"], quality["cfo_bins"])
                print(line)


def _rs_erasures(option, opt, value, parser):
    """--rs-erasures [M]: takes the next argument where it is a number."""
    m = 28
    if parser.rargs and parser.rargs[0].isdigit():
        m = int(parser.rargs.pop(0))
    if m > 32:
        parser.error("--rs-erasures takes at most 32")
    setattr(parser.values, option.dest, m)


def make_parser():
    parser = OptionParser(option_class=_options.eng_option, conflict_handler="resolve")
    expert_grp = parser.add_option_group("Expert")
    parser.add_option("", "--snr", type="eng_float", default=30, help="set the SNR of the channel in dB [default=%default]")
    parser.add_option("", "--from-file", default="ofdm_tx.dat", help="IQ file to demodulate [default=%default]")
    parser.add_option("", "--to-file", default="rx1.txt", help="write received file contents here [default=%default]")
    parser.add_option("", "--chunk-samples", type="eng_float", default=0,
                      help="stream the capture through the demodulator in chunks of this many samples "
                           "(0 = one call on the whole file) [default=%default]")
    parser.add_option("", "--link-quality", action="store_true", default=False,
                      help="append the packet's link quality (preamble SNR, decision SNR in dB, carrier offset in "
                           "subcarrier spacings) to each packet line [default=%default]")
    parser.add_option("", "--iq-format", type="choice", choices=list(iqio.FORMATS), default="fc32",
                      help="sample format of the IQ file: fc32 (interleaved float32) or sc16 (interleaved int16, the "
                           "format of rx_samples_to_file and most capture tools) [default=%default]")
    parser.add_option("", "--iq-scale", type="eng_float", default=None,
                      help="with sc16: value of one LSB (sample = int16 * scale) [default=2^-15]")
    parser.add_option("", "--ddc-decim", type="intx", default=0,
                      help="the IQ file is a wideband capture at this multiple of the modem's rate: tune and decimate "
                           "it on the GPU first (the radio's set_decim; 0 = off) [default=%default]")
    parser.add_option("", "--ddc-freq", type="eng_float", default=None,
                      help="with --ddc-decim: centre of the link in the capture, cycles per sample in [-0.5, 0.5] "
                           "(the radio's set_center_freq over the capture's rate) [default=0.0]")
    parser.add_option("", "--ddc-freqs", default=None,
                      help="with --ddc-decim, instead of --ddc-freq: comma-separated centres of ALL links in the capture; "
                           "they are extracted in one pass on the GPU (ofdm_demod_bank), one account per link, and "
                           "--to-file gets .linkN appended [default=off]")
    parser.add_option("", "--fec", action="store_true", default=False,
                      help="coded link: the file was written by benchmark_ofdm_tx --fec; every delivered packet, the "
                           "CRC-failed ones included, goes through the Viterbi decoder on the GPU and is accounted by "
                           "the CRC inside the code [default=%default]")
    parser.add_option("", "--fec-soft", action="store_true", default=False,
                      help="--fec with soft decisions: the receiver hands the decoder one reliability per coded bit, "
                           "weighted by each carrier's channel gain, where --fec hands it the sliced bytes "
                           "[default=%default]")
    parser.add_option("", "--fec-rate", type="choice", choices=("1/2", "2/3", "3/4", "5/6"), default=None,
                      help="coded link at this rate, as benchmark_ofdm_tx --fec-rate wrote it (implies --fec; works "
                           "with --fec-soft) [default=1/2]")
    parser.add_option("", "--ldpc", action="store_true", default=False,
                      help="coded link with the other inner code: the file was written by benchmark_ofdm_tx --ldpc; "
                           "every delivered packet, the CRC-failed ones included, goes through the min-sum decoder on "
                           "the GPU and is accounted by the CRC inside the code [default=%default]")
    parser.add_option("", "--ldpc-soft", action="store_true", default=False,
                      help="--ldpc with soft decisions: the decoder takes the soft demapper's value of every coded bit "
                           "where --ldpc takes the sliced bytes [default=%default]")
    parser.add_option("", "--ldpc-rate", type="choice", choices=("1/2", "2/3", "3/4", "5/6"), default=None,
                      help="the QC-LDPC code of this rate, as benchmark_ofdm_tx --ldpc-rate wrote it (implies --ldpc; works "
                           "with --ldpc-soft) [default=1/2]")
    parser.add_option("", "--rs", action="store_true", default=False,
                      help="outer code: the file was written by benchmark_ofdm_tx --rs; every delivered packet goes "
                           "through the Reed-Solomon decoder on the GPU, behind the inner decoder where --fec, "
                           "--fec-rate, --fec-soft, --ldpc or --ldpc-soft is given, and is accounted by the CRC inside the RS block "
                           "[default=%default]")
    parser.add_option("", "--rs-erasures", action="callback", callback=_rs_erasures, dest="rs_erasures", default=None,
                      help="--rs, decoding with reliabilities: --rs-erasures [M] erases the weakest symbols, at most M "
                           "(0 .. 32, 28 if not given), of every codeword that fails, chosen by the soft demapper's "
                           "values; for an RS link without an inner code (not with --fec, --fec-rate or --fec-soft); "
                           "with --ldpc, --ldpc-rate or --ldpc-soft the symbols are chosen by the min-sum decoder's own "
                           "byte reliabilities "
                           "[default=off]")
    parser.add_option("", "--sig", action="store_true", default=False,
                      help="self-describing coded link: the file was written by benchmark_ofdm_tx --sig; the signal "
                           "field in front of every block names its coding, its fields are decoded on the GPU and every "
                           "packet goes through the decoders its field names -- no coding flag goes with it "
                           "[default=%default]")
    parser.add_option("", "--sig-soft", action="store_true", default=False,
                      help="--sig with soft decisions: field and bodies are decoded from the soft demapper's values "
                           "[default=%default]")
    _options.add_resamp_options(parser)
    parser.add_option("", "--resamp-freqs", default=None,
                      help="with --resamp-interp / --resamp-decim, instead of --resamp-freq: comma-separated centres of "
                           "ALL links in the capture; they are extracted in one pass on the GPU "
                           "(ofdm_demod_resamp_bank), one account per link, and --to-file gets .linkN appended "
                           "[default=off]")
    parser.add_option("", "--csi-report", default=None,
                      help="write the per-carrier channel report over the CRC-ok packets to this file: one line per "
                           "occupied carrier (index, FFT bin, preamble SNR, decision SNR, gain in dB) [default=off]")
    parser.add_option("", "--suggest-map", type="eng_float", default=None,
                      help="print the hex carrier map of the carriers whose SNR reaches this many dB [default=off]")
    receive_path.receive_path.add_options(parser, expert_grp)
    ofdm.ofdm_demod.add_options(parser, expert_grp)
    return parser


def _run_links(options, freqs, make_bank):
    """Every link of the wideband file through ``make_bank(callback)``, an ofdm_demod_bank or one of its kin: one
    account and one ``--to-file``.linkN per link; returns the accounts."""
    files = [open("%s.link%d" % (options.to_file, i), "wb") for i in range(len(freqs))]
    accts = [rx_accounting(f) for f in files]
    bank = None
    try:
        bank = make_bank(lambda link, ok, payload: accts[link].rx_callback(ok, payload))
        source = iqio.file_source(options.from_file, fmt=options.iq_format)
        if int(options.chunk_samples):
            for piece in source.read_chunks(int(options.chunk_samples)):
                bank.feed(piece)
            bank.flush()
        else:
            bank.work(source.read_all())
    finally:
        if bank is not None:
            bank.close()
        for f in files:
            f.close()
    return accts


def _main_bank(parser, options):
    """--ddc-freqs: every link of the wideband file through one ofdm_demod_bank; returns the per-link accounts."""
    if options.ddc_freq is not None:
        parser.error("--ddc-freqs and --ddc-freq are mutually exclusive")
    if not options.ddc_decim:
        parser.error("--ddc-freqs needs --ddc-decim")
    if options.link_quality or options.csi_report is not None or options.suggest_map is not None:
        parser.error("--ddc-freqs does not combine with --link-quality, --csi-report or --suggest-map")
    try:
        freqs = [float(f) for f in options.ddc_freqs.split(",")]
    except ValueError:
        parser.error("--ddc-freqs takes comma-separated numbers")
    return _run_links(options, freqs, lambda cb: ofdm.ofdm_demod_bank(
        options, freqs, int(options.ddc_decim), iq_format=options.iq_format, iq_scale=options.iq_scale, callback=cb))


def _main_resamp_bank(parser, options):
    """--resamp-freqs: every link of the wideband file through one ofdm_demod_resamp_bank; returns the per-link
    accounts."""
    if options.ddc_decim or options.ddc_freq is not None or options.ddc_freqs is not None:
        parser.error("--resamp-freqs does not combine with --ddc-decim, --ddc-freq or --ddc-freqs")
    if options.resamp_freq:
        parser.error("--resamp-freqs and --resamp-freq are mutually exclusive")
    if not options.resamp_interp and not options.resamp_decim:
        parser.error("--resamp-freqs needs --resamp-interp / --resamp-decim")
    if options.link_quality or options.csi_report is not None or options.suggest_map is not None:
        parser.error("--resamp-freqs does not combine with --link-quality, --csi-report or --suggest-map")
    try:
        freqs = [float(f) for f in options.resamp_freqs.split(",")]
    except ValueError:
        parser.error("--resamp-freqs takes comma-separated numbers")
    L, M = int(options.resamp_interp or 1), int(options.resamp_decim or 1)  # (one of the two alone: the other is 1)
    return _run_links(options, freqs, lambda cb: ofdm.ofdm_demod_resamp_bank(
        options, freqs, L, M, iq_format=options.iq_format, iq_scale=options.iq_scale, callback=cb))


def main(argv=None):
    parser = make_parser()
    (options, args) = parser.parse_args(argv)
    if len(args) != 0:
        parser.print_help(sys.stderr)
        sys.exit(1)
    if options.sig_soft:
        options.sig = True
    if options.sig and (options.fec or options.fec_soft or options.fec_rate or options.ldpc or options.ldpc_soft or options.ldpc_rate
                        or options.rs or options.rs_erasures is not None):
        parser.error("--sig / --sig-soft take no coding flags: the signal field names every packet's coding")
    if options.sig and (options.resamp_freqs is not None or options.ddc_freqs is not None):
        parser.error("--sig does not combine with --ddc-freqs or --resamp-freqs")
    if options.fec_soft:
        options.fec = True
    if options.fec_rate:
        options.fec = dict(rate=options.fec_rate)   # (what receive_path hands to ofdm_demod(fec=))
    if options.ldpc_soft:
        options.ldpc = True
    if options.ldpc_rate:
        options.ldpc = dict(rate=options.ldpc_rate)   # (what receive_path hands to ofdm_demod(ldpc=))
    if options.ldpc and options.fec:
        parser.error("--ldpc / --ldpc-soft take the place of --fec / --fec-rate / --fec-soft: a link has one inner code")
    if options.rs_erasures is not None:
        if options.fec:
            parser.error("--rs-erasures needs an RS link without an inner code, or --ldpc: not with --fec, --fec-rate or --fec-soft")
        options.rs = True
    if (options.fec or options.rs or options.ldpc) and (options.resamp_freqs is not None or options.ddc_freqs is not None):
        parser.error("--fec, --ldpc and --rs do not combine with --ddc-freqs or --resamp-freqs")
    if options.resamp_freqs is not None:
        return _main_resamp_bank(parser, options)
    if options.ddc_freqs is not None:
        return _main_bank(parser, options)

    packet_file = open(options.to_file, 'wb')
    acct = rx_accounting(packet_file)
    want_csi = options.csi_report is not None or options.suggest_map is not None
    if options.link_quality:
        rxpath = receive_path.receive_path(None, options, quality_callback=acct.rx_callback, csi=want_csi)
    else:
        rxpath = receive_path.receive_path(acct.rx_callback, options, csi=want_csi)
    # (receive_path takes --iq-format / --iq-scale, --fec, --rs, --ddc-decim / --ddc-freq and --resamp-* from the options)
    rxpath.run(iqio.file_source(options.from_file, fmt=options.iq_format), chunk_samples=int(options.chunk_samples))
    packet_file.close()
    if options.csi_report is not None:
        rep = rxpath.ofdm_rx.carrier_report()
        zl = config.zeros_on_left(options.fft_length, options.occupied_tones)
        with open(options.csi_report, "w") as f:
            f.write("# carrier fft_bin snr_preamble_db snr_decision_db gain_db\n")
            for i in range(options.occupied_tones):
                f.write("%d %d %.2f %.2f %.2f\n" % (i, i + zl, rep["snr_preamble_db"][i], rep["snr_decision_db"][i],
                                                     rep["gain_db"][i]))
    if options.suggest_map is not None:
        print("suggested carrier map: %s" % rxpath.ofdm_rx.suggest_carrier_map(float(options.suggest_map)))
    return acct


if __name__ == '__main__':
    try:
        main()
    except KeyboardInterrupt:
        pass
