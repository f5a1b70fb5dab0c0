"""Host-side counterpart of the reference's ``transmit_path`` (transmit_path.py:35-84): an
``ofdm_mod`` plus the output gain.  Same constructor argument, methods and command-line flags;
the gain stage (gr.multiply_const_cc ``amp``) is folded into the modulator kernel's store."""
import copy

from . import dpd as _dpd, ofdm, options as _options

# flag, group, keyword arguments of the reference's option table (transmit_path.py:72-79)
_FLAGS = (
    (("", "--tx-amplitude"), "normal", dict(type="eng_float", default=0.250, metavar="AMPL",
                                            help="digital output amplitude, 0 <= AMPL < 1 [default=%default]")),
    (("-v", "--verbose"), "normal", dict(action="store_true", default=False)),
    (("-S", "--samples-per-symbol"), "expert", dict(type="int", default=2, help="samples per symbol [default=%default]")),
    (("", "--log"), "expert", dict(action="store_true", default=False,
                                   help="dump every probe point of the flow graph to files (large)")),
)


class transmit_path(object):
    def __init__(self, options, device_id=0, apply_carrier_map=False, iq_format=None, iq_scale=None, duc=None,
                 resample=None, fec=None, rs=None, ldpc=None, sig=None, cfr=None, dpd=None, spectrum=None):
        """``apply_carrier_map=True`` re-enables what transmit_path.py:67 has commented out: the map
        given to send_pkt really reaches the mapper (and must reach the receiver's frame sink too).
        ``iq_format`` / ``iq_scale``: sample format of the output (ofdm_mod); None: the options' ``iq_format`` /
        ``iq_scale`` (--iq-format / --iq-scale), "fc32" where they have none.
        ``duc``: wideband transmit stage of ofdm_mod, ``dict(interpolation=, center_freq=, taps=None)``; None: the
        options' ``duc_interp`` / ``duc_freq`` (--duc-interp / --duc-freq), no stage where duc_interp is unset or 0
        (what the reference sets on its radio: set_interp / set_center_freq, usrp_transmit_path.py).
        ``resample``: rational-rate transmit stage of ofdm_mod, ``dict(interpolation=, decimation=, center_freq=0.0,
        taps=None)``; None: the options' ``tx_resamp_interp`` / ``tx_resamp_decim`` / ``tx_resamp_freq``
        (--tx-resamp-*).
        ``fec``: coded link of ofdm_mod, ``True`` or ``dict(interleave=16, rate="1/2")``; None: the options' ``fec`` (--fec).
        ``rs``: outer code of ofdm_mod, ``True``; None: the options' ``rs`` (--rs).
        ``ldpc``: the other inner code of ofdm_mod, ``True`` or ``dict(max_iters=20, rate="1/2")``; None: the options' ``ldpc``
        (--ldpc, --ldpc-rate).
        ``sig``: the signal field of ofdm_mod, ``True``; None: the options' ``sig`` (--sig).  ``fec`` / ``ldpc`` / ``rs``
        then choose the coding that every packet announces.
        ``cfr``: crest-factor reduction of ofdm_mod, ``dict(papr_db=7.0, half_width=16[, threshold=])``, the last stage;
        None: the options' ``cfr_papr`` / ``cfr_half_width`` (--cfr-papr / --cfr-half-width), no stage where cfr_papr
        is unset.  The threshold follows the transmit amplitude.
        ``dpd``: digital predistortion of ofdm_mod, ``dict(coef=table[, limit=])``, behind ``cfr``; None: the table in
        the .npy file the options' ``dpd`` names (--dpd), no stage where it is unset.  The table does not follow the
        transmit amplitude: it holds for the amplitude it was trained at.
        ``spectrum``: spectrum measurement of ofdm_mod, ``dict(nfft=[, hop=][, window=][, spacing=][, mask=])``, which
        reads what the path hands out; None: the options' ``psd`` ("NFFT[,HOP]", --psd) and ``psd_spacing``
        (--psd-spacing), no measurement where psd is unset.  The figures are ``ofdm_tx.last_spectrum``."""
        opts = copy.copy(options)
        if rs is None:
            rs = bool(getattr(opts, "rs", None))
        if fec is None:
            fec = getattr(opts, "fec", None) or None
        if ldpc is None:
            ldpc = getattr(opts, "ldpc", None) or None
        if sig is None:
            sig = bool(getattr(opts, "sig", None))
        if iq_format is None:
            iq_format = getattr(opts, "iq_format", None) or "fc32"
        if iq_scale is None:
            iq_scale = getattr(opts, "iq_scale", None)
        if duc is None and getattr(opts, "duc_interp", None):
            duc = dict(interpolation=int(opts.duc_interp), center_freq=float(getattr(opts, "duc_freq", 0.0) or 0.0))
        if resample is None:
            resample = _options.tx_resamp_from_options(opts)
        if cfr is None and getattr(opts, "cfr_papr", None) is not None:
            hw = getattr(opts, "cfr_half_width", None)
            cfr = dict(papr_db=float(opts.cfr_papr), half_width=16 if hw is None else int(hw))
        if dpd is None and getattr(opts, "dpd", None):
            dpd = dict(coef=_dpd.load_coef(opts.dpd))
        if spectrum is None and getattr(opts, "psd", None):
            spectrum = _options.psd_from_options(opts)
        self._apply_carrier_map = bool(apply_carrier_map)
        self._cfr = cfr is not None
        self._verbose = bool(getattr(opts, "verbose", False))
        self._samples_per_symbol = getattr(opts, "samples_per_symbol", 2)
        self.carrier_map_old = ""
        self.ofdm_tx = ofdm.ofdm_mod(opts, msgq_limit=4, pad_for_usrp=False, device_id=device_id, iq_format=iq_format,
                                     iq_scale=iq_scale, duc=duc, resample=resample, fec=fec, rs=rs, ldpc=ldpc, sig=sig,
                                     cfr=cfr, dpd=dpd, spectrum=spectrum)
        self.set_tx_amplitude(opts.tx_amplitude)
        if self._verbose:
            self._print_verbage()

    # -- wiring ---------------------------------------------------------------------
    def connect(self, sink):
        """Attach the IQ sink (iqio.file_sink / vector_sink ...) that stands in for the radio."""
        self.ofdm_tx.connect(sink)
        return self

    # -- controls -------------------------------------------------------------------
    def set_tx_amplitude(self, ampl):
        """Output gain, clamped to [0, 1] as transmit_path.py:56-62 does."""
        self._tx_amplitude = min(max(ampl, 0.0), 1)
        self.ofdm_tx.engine().set_tx_amplitude(self._tx_amplitude)
        if self._cfr:
            self.ofdm_tx.set_cfr_amplitude(self._tx_amplitude)   # the threshold follows the amplitude

    def send_pkt(self, payload='', eof=False, carrier_map_new="FE7F"):
        """Queue one packet (or end the burst with eof=True).  A changed carrier map is only recorded,
        exactly like the reference, unless the path was built with apply_carrier_map=True."""
        changed = carrier_map_new != self.carrier_map_old
        if changed and self._apply_carrier_map:
            self.ofdm_tx.reset_carrier_map(carrier_map_new)
        if changed:
            self.carrier_map_old = carrier_map_new
        return self.ofdm_tx.send_pkt(payload, eof)

    def flush(self, end=False):
        return self.ofdm_tx.flush(end)

    # -- command line ---------------------------------------------------------------
    @staticmethod
    def add_options(normal, expert):
        for names, group, kw in _FLAGS:
            (normal if group == "normal" else expert).add_option(*names, **kw)

    def _print_verbage(self):
        print("Tx amplitude     %s" % (self._tx_amplitude,))
        print("samples/symbol:  %3d" % (self._samples_per_symbol,))
