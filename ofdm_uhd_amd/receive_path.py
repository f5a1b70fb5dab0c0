"""receive_path: hands the sample stream to ofdm_demod (receive_path.py:29-58)."""
import copy

from . import ofdm, options as _options


class receive_path(object):
    def __init__(self, rx_callback, options, device_id=0, quality_callback=None, csi=False, iq_format=None, iq_scale=None,
                 ddc=None, resample=None, fec=None, soft=None, rs=None, ldpc=None, sig=None):
        """``iq_format`` / ``iq_scale``: sample format of the stream (ofdm_demod); None: the options' ``iq_format`` /
        ``iq_scale`` (--iq-format / --iq-scale), "fc32" where they have none.
        ``ddc``: wideband front end of ofdm_demod, ``dict(decimation=, center_freq=, taps=None)``; None: the options'
        ``ddc_decim`` / ``ddc_freq`` (--ddc-decim / --ddc-freq), no front end where ddc_decim is unset or 0 (what the
        reference sets on its radio: set_decim / set_center_freq, usrp_receive_path.py).
        ``resample``: rational-rate front end of ofdm_demod, ``dict(interpolation=, decimation=, center_freq=0.0,
        taps=None)``; None: the options' ``resamp_interp`` / ``resamp_decim`` / ``resamp_freq`` (--resamp-*).
        ``fec``: coded link of ofdm_demod, ``True`` or ``dict(interleave=16, rate="1/2")``; None: the options' ``fec`` (--fec).
        ``soft``: soft-decision receive of ofdm_demod, ``True`` or ``dict(scale=32)``; None: the options' ``fec_soft``
        (--fec-soft), which turns the coded link on as well.
        ``rs``: outer code of ofdm_demod, ``True`` or ``dict(erasures=True, max_erasures=28)``; None: the options' ``rs``
        (--rs), or their ``rs_erasures`` (--rs-erasures [M]), which turns the soft values on as well; on an ``ldpc`` link
        it selects ``source="ldpc"`` instead and leaves ``soft`` as it is.
        ``ldpc``: the other inner code of ofdm_demod, ``True`` or ``dict(max_iters=20, rate="1/2")``; None: the options' ``ldpc``
        (--ldpc, --ldpc-rate), or their ``ldpc_soft`` (--ldpc-soft), which turns the soft values on as well.
        ``sig``: the signal field of ofdm_demod, ``True``; None: the options' ``sig`` (--sig), or their ``sig_soft``
        (--sig-soft), which turns the soft values on as well.  The field names the coding: no coding setting goes with it."""
        options = copy.copy(options)    # make a copy so we can destructively modify
        if sig is None:
            sig = bool(getattr(options, "sig", None) or getattr(options, "sig_soft", None))
        if sig and soft is None and getattr(options, "sig_soft", None):
            soft = True
        if soft is None and getattr(options, "fec_soft", None):
            soft = True
            fec = (getattr(options, "fec", None) or True) if fec is None else fec   # (a dict where --fec-rate set one)
        if fec is None:
            fec = getattr(options, "fec", None) or None
        if soft is None and getattr(options, "ldpc_soft", None):
            soft = True
            ldpc = (getattr(options, "ldpc", None) or True) if ldpc is None else ldpc   # (a dict where --ldpc-rate set one)
        if ldpc is None:
            ldpc = getattr(options, "ldpc", None) or None
        if rs is None and getattr(options, "rs_erasures", None) is not None:
            rs = dict(erasures=True, max_erasures=int(options.rs_erasures))
            if ldpc:
                rs["source"] = "ldpc"           # the min-sum decoder's own reliabilities, hard bytes (--ldpc) or values (--ldpc-soft)
            else:
                soft = True if soft is None else soft
        if rs is None:
            rs = bool(getattr(options, "rs", None))
        if iq_format is None:
            iq_format = getattr(options, "iq_format", None) or "fc32"
        if iq_scale is None:
            iq_scale = getattr(options, "iq_scale", None)

        if ddc is None and getattr(options, "ddc_decim", None):
            ddc = dict(decimation=int(options.ddc_decim), center_freq=float(getattr(options, "ddc_freq", 0.0) or 0.0))

        if resample is None:
            resample = _options.resamp_from_options(options)

        self._verbose = getattr(options, "verbose", False)
        self._log = getattr(options, "log", False)
        self._rx_callback = rx_callback      # this callback is fired when there's a packet available

        self.ofdm_rx = ofdm.ofdm_demod(options, callback=self._rx_callback, device_id=device_id,
                                       quality_callback=quality_callback, csi=csi, iq_format=iq_format, iq_scale=iq_scale,
                                       ddc=ddc, resample=resample, fec=fec, soft=soft, rs=rs, ldpc=ldpc, sig=sig)

        if self._verbose:
            self._print_verbage()

    def work(self, iq):
        return self.ofdm_rx.work(iq)

    def run(self, source, chunk_samples=None):
        """Demodulate a whole source; with ``chunk_samples`` it is streamed through ofdm_demod.feed
        in pieces of that size (same packets, bounded memory)."""
        if not chunk_samples or not hasattr(source, "read_chunks"):
            return self.ofdm_rx.run(source)
        out = []
        for piece in source.read_chunks(int(chunk_samples)):
            out += self.ofdm_rx.feed(piece)
        out += self.ofdm_rx.flush()
        return out

    def feed(self, iq, flush=False):
        """Continuous operation (what the radio source does in the reference): next chunk in,
        packets that became final out; see ofdm_demod.feed."""
        return self.ofdm_rx.feed(iq, flush)

    def flush(self):
        return self.ofdm_rx.flush()

    def add_options(normal, expert):
        normal.add_option("-v", "--verbose", action="store_true", default=False)
        expert.add_option("-S", "--samples-per-symbol", type="int", default=2,
                          help="set samples/symbol [default=%default]")
        expert.add_option("", "--log", action="store_true", default=False,
                          help="Log all parts of flow graph to files (CAUTION: lots of data)")

    add_options = staticmethod(add_options)

    def _print_verbage(self):
        print("\nReceive Path:")
