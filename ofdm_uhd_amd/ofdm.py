"""ofdm_mod / ofdm_demod: packets in, baseband IQ out -- and back.

Python-3 mirror of the reference's ``ofdm.py`` (ofdm.py:38-305) with the same
constructor arguments, option names, ``send_pkt`` / callback surface and error
behaviour.  Where the reference wires GNU Radio blocks into a flow graph, this
module hands batches to the HIP engine (libofdm_hip.so): ``send_pkt`` queues a
payload, ``send_pkt(eof=True)`` (or ``flush()``) modulates the queued batch in one
GPU call and writes the samples to the connected sink; ``ofdm_demod.work(iq)``
demodulates one contiguous IQ stream and fires ``callback(ok, payload)`` once per
recovered packet, in stream order, on the caller's thread.
"""
import collections
import math
import sys

import numpy as np

from . import cfr as _cfr, config, csi as _csi, ddc as _ddc, dpd as _dpd, duc as _duc, engine, fec as _fec, iqio, ldpc as _ldpc, ofdm_packet_utils, pfb as _pfb, resample as _resample, rs as _rs, sig as _sig, spectrum as _spectrum, tx_resample as _tx_resample  # noqa: F401  (ofdm_packet_utils re-exported like digital.ofdm_packet_utils)
from .config import known_symbols_4512_3  # noqa: F401  (ofdm.py:310-325)


class ofdm_mod(object):
    """
    Modulates an OFDM stream. Based on the options fft_length, occupied_tones, and
    cp_length, this block creates OFDM symbols using a specified modulation option.

    Send packets by calling send_pkt
    """

    def __init__(self, options, msgq_limit=2, pad_for_usrp=True, device_id=0, iq_format="fc32", iq_scale=None, duc=None,
                 resample=None, fec=None, rs=None, ldpc=None, sig=False, cfr=None, dpd=None, spectrum=None):
        """
        @param options: pass modulation options from higher layers (fft length, occupied tones, etc.)
        @param spectrum: spectrum measurement, ``dict(nfft=1024[, hop=][, window=][, spacing=][, mask=])``: the engine's
               Welch estimator (spectrum.py, Engine.psd) reads the stream flush() hands out, behind ``duc`` /
               ``resample`` / ``cfr`` / ``dpd`` and in the format it is handed out in (an sc16 output is measured as the
               16-bit samples a converter gets), and changes nothing.  ``last_spectrum`` holds the figures
               (spectrum.report: density, peak, nseg, obw, aclr_db, mask_margin_db, ...) of the stream flush(end=True)
               ended last, or of the running one.  The channel's centre and width come from the options and the wideband
               stage: occupied_tones / fft_length of the modem's rate around the stage's centre frequency; ``spacing``
               (None: the modem's rate, the raster of the multi-link banks) places the adjacent channels, ``mask`` is
               spectrum.mask_margin_db's.  None: nothing new runs
        @param dpd: digital predistortion, ``dict(coef=table[, limit=])``: the engine's memory-polynomial stage (dpd.py,
               Engine.dpd) with the (M, K) table ``coef`` (dpd.train / dpd.fit) runs last, behind ``cfr`` where both are
               given: CFR, then DPD, then the converter.  The stages in front then emit complex64 and this one does the
               ``iq_format`` store.  ``limit`` is the converter's full scale in the stream's units; the stage counts the
               samples above it and clamps nothing.  No delay: flush(end=True) / send_pkt(eof=True) starts the stage
               afresh, ``last_dpd`` holds the figures (dpd.report) of the stream that ended last, or of the running
               one, and ``set_dpd_coef(coef)`` swaps the table between streams.  A table holds for the transmit
               amplitude and the peak limit it was trained at: train again after changing either, and give ``cfr=``
               with it (an amplifier has no inverse past its compression point).  None: nothing new runs
        @param cfr: crest-factor reduction, ``dict(papr_db=7.0, half_width=16[, threshold=][, kind="hann"])``: the
               engine's peak-windowing stage (cfr.py, Engine.cfr) runs last, behind ``duc`` / ``resample`` where there is
               one; those stages then emit complex64 and this one does the ``iq_format`` store.  Peaks are pulled down to
               ``threshold``, by default ``papr_db`` above cfr.modem_rms(options) times the pass-band gain of the
               wideband stage in front (the level of the data symbols in the stream that enters the stage).  The stream
               comes out ``half_width`` samples late and continues across flush() calls; flush(end=True) /
               send_pkt(eof=True) pushes ``half_width`` zeros so that the tail comes out, and starts the stage afresh.
               ``last_cfr`` holds the figures (cfr.report, against that level) of the stream that ended last, or of
               the running one.  None: nothing new runs
        @param sig: self-describing coded link (sig.py): every block goes out behind a 12-byte signal field that names
               its coding, so the receiving end, ofdm_demod(sig=True), needs no coding setting.  ``fec`` / ``ldpc`` /
               ``rs`` then only choose the default coding; ``send_pkt(payload, coding=...)`` overrides it per packet, and
               one batch may mix codings: flush() groups the queued packets by coding, encodes each group with the calls
               below, puts the fields in front with one Engine.sig_encode over the whole batch, in the packets' order,
               and modulates once.  The largest payloads shrink by up to 12 bytes (sig.max_payload).  False: no field,
               nothing new runs
        @param msgq_limit: maximum number of messages in message queue (kept for API
               compatibility: the reference blocks send_pkt at this depth, ofdm.py:148;
               here packets are batched until flush)
        @param pad_for_usrp: If true, packets are padded such that they end up a multiple of 128 samples
        @param iq_format: "fc32" (complex64 samples) or "sc16": flush() returns, and the sink is written, int16
               arrays of shape (n, 2), quantised on the GPU as iqio.to_sc16 defines it
        @param iq_scale: full scale of the 16-bit samples (None: 2^15)
        @param duc: wideband transmit stage, ``dict(interpolation=, center_freq=, taps=None)`` (center_freq in cycles
               per wideband sample): flush() modulates in float32 and returns, and writes to the sink, the WIDEBAND
               stream in ``iq_format`` -- the engine's stateful interpolate-and-translate stage (duc.py, Engine.duc)
               stores it; the stream continues across flush() calls (a batch's filter tail comes out in front of the
               next batch) until flush(end=True) / send_pkt(eof=True).  ``taps=None``: duc.design for
               occupied_tones / fft_length
        @param resample: the same for a band whose rate is L / M times the modem's, no integer multiple of it:
               ``dict(interpolation=, decimation=, center_freq=0.0, taps=None)``, the engine's rational-rate transmit
               stage (tx_resample.py, Engine.tx_resamp) in the DUC's place; ``taps=None``: tx_resample.design.  Not
               together with ``duc``
        @param fec: coded link: ``True`` or ``dict(interleave=16, rate="1/2")`` (fec.py).  send_pkt then takes up to 2040
               bytes and flush() encodes the batch on the GPU (Engine.fec_encode: payload | CRC-32 through the rate-1/2,
               K = 7 convolutional code and a block interleaver, 2 n + 10 bytes; ``rate`` "2/3", "3/4" or "5/6" punctures
               it to fec.coded_len(n, rate) bytes) ahead of the modulator; the receiving end is ofdm_demod(fec=) with
               the same setting.  None: the payloads go out as they are and nothing new runs
        @param rs: outer code: ``True`` wraps every payload in a Reed-Solomon block (rs.py, Engine.rs_encode: payload |
               CRC-32, 32 parity bytes per 223, byte-interleaved) before the inner code, if any, and the modulator:
               flush() encodes outer, then inner, then modulates.  send_pkt then takes up to 3564 bytes, 1780 with
               ``fec`` or 1752 with ``ldpc`` (2328, 2632, 2904 at its rates 2/3, 3/4, 5/6: the RS block must fit the inner
               code); the receiving end is
               ofdm_demod(rs=True).  None / False: nothing new runs
        @param ldpc: coded link with the other inner code, in the place of ``fec`` (both: ValueError): ``True``,
               ``dict(max_iters=20, rate="1/2")`` or an int (ldpc.py).  send_pkt then takes up to 2012 bytes and flush()
               encodes the batch on the GPU (Engine.ldpc_encode: payload | CRC-32 in rate-1/2 QC-LDPC codewords of 96 info
               and 96 parity bytes, ldpc.coded_len(n) bytes; ``rate`` "2/3", "3/4" or "5/6" takes the code of that rate,
               codewords of 128 / 64, 144 / 48 or 160 / 32 bytes, payloads up to 2684, 3020 or 3356 bytes,
               ldpc.coded_len(n, rate) bytes); the receiving end is ofdm_demod(ldpc=) with the same setting.  None:
               nothing new runs
        """
        if duc is not None and resample is not None:
            raise ValueError("ofdm_mod takes duc= or resample=, not both")
        if sig:
            _sig.coding(fec=fec, ldpc=ldpc, rs=bool(rs))    # (ValueError for what is no coding, before anything is built)
        if dpd is not None:
            if "coef" not in dpd or set(dpd) - {"coef", "limit"}:
                raise ValueError("dpd= takes coef and limit, not %s" % ", ".join(sorted(dpd)))
            _dpd.mempoly_cfg(dpd["coef"], limit=dpd.get("limit"))   # (ValueError for a bad table, before anything is built)
        self._pad_for_usrp = pad_for_usrp
        self._msgq_limit = msgq_limit
        self._modulation = options.modulation
        self._fft_length = options.fft_length
        self._occupied_tones = options.occupied_tones
        self._cp_length = options.cp_length

        # ofdm.py:71-87: preamble = first occupied_tones known symbols, odd bins zeroed
        self._ksfreq = config.make_ksfreq(self._fft_length, self._occupied_tones)
        self._padded_preambles = [config.padded_preamble(self._fft_length, self._occupied_tones)]
        self._rotated_const = config.rotated_constellation(self._modulation)  # ofdm.py:91-101

        # the modulator alone has unit gain after its 1/sqrt(N) (ofdm.py:114); transmit_path sets the amplitude
        cfg_opts = _copy_options(options, tx_amplitude=1.0)
        self._engine = engine.Engine(cfg_opts, pad_for_usrp=pad_for_usrp, device_id=device_id)
        self._duc = None             # the wideband stage in force: "duc" or "tx_resamp" (Engine.<stage>, <stage>_reset, <stage>_cfg)
        self._duc_live = False       # the wideband stream holds samples whose filter tail is still to come
        occ = self._occupied_tones / float(self._fft_length)
        self._cfr = None if cfr is None else dict(cfr)   # with it, the stage in front stores complex64
        self._dpd = None if dpd is None else dict(dpd)   # with it, cfr= too stores complex64
        last_format, last_scale = (iq_format, iq_scale) if dpd is None else ("fc32", None)   # of the stage in front of dpd=
        stage_format, stage_scale = (last_format, last_scale) if cfr is None else ("fc32", None)
        if duc is not None:
            # the 16-bit format, if any, is the wideband side's: the modulator's output (the stage's input) is complex64
            d = dict(duc)
            self._engine.set_duc(_duc.duc_cfg(d.pop("interpolation"), d.pop("center_freq"), taps=d.pop("taps", None),
                                              occupied_fraction=occ,
                                              out_format=iqio.check_format(stage_format), out_scale=stage_scale, **d))
            self._duc = "duc"
        elif resample is not None:
            d = dict(resample)
            self._engine.set_tx_resamp(_tx_resample.tx_resamp_cfg(
                d.pop("interpolation"), d.pop("decimation"), d.pop("center_freq", 0.0), taps=d.pop("taps", None),
                occupied_fraction=occ, out_format=iqio.check_format(stage_format), out_scale=stage_scale, **d))
            self._duc = "tx_resamp"
        elif iqio.check_format(stage_format) != "fc32":
            self._engine.set_tx_iq_format(iq_format, iq_scale)
        self._dpd_live = False       # the stage has seen samples of a stream that has not ended
        self._last_dpd = None
        if self._dpd is not None:
            coef = self._dpd["coef"]
            self._dpd = dict(limit=self._dpd.get("limit"), out_format=iqio.check_format(iq_format), out_scale=iq_scale)
            self.set_dpd_coef(coef)
        self._cfr_live = False       # the stage holds samples that are still to come out
        self._cfr_rms = None         # the level its threshold was set against
        self._last_cfr = None
        if self._cfr is not None:
            d = self._cfr
            gain = 1.0
            if self._duc is not None:
                # pass-band gain of the stage in front: its prototype low-pass at zero frequency, over L
                wide = getattr(self._engine, self._duc + "_cfg")
                gain = abs(float(np.sum(np.array(wide.taps[:wide.ntaps], np.float64)))) / float(wide.interpolation)
            thr = d.pop("threshold", None)
            papr = d.pop("papr_db", 7.0)
            window = _cfr.design(d.pop("half_width", 16), d.pop("kind", "hann"))
            if d:
                raise ValueError("cfr= takes papr_db, half_width, threshold and kind, not %s" % ", ".join(sorted(d)))
            self._cfr = dict(threshold=thr, papr_db=papr, window=window, level=_cfr.modem_rms(cfg_opts) * gain,
                             out_format=iqio.check_format(last_format), out_scale=last_scale)
            self.set_cfr_amplitude(1.0)
        self._spectrum = None        # spectrum=: the channel and what to report of it
        self._spectrum_live = False  # the estimator has seen samples of a stream that has not ended
        self._last_spectrum = None
        if spectrum is not None:
            d = dict(spectrum)
            fmt = iqio.check_format(iq_format)
            in_scale = None if fmt == "fc32" or iq_scale is None else 1.0 / iqio.check_scale(iq_scale, iqio.TX_SCALE)
            pcfg = _spectrum.psd_cfg(d.pop("nfft", 1024), d.pop("hop", None), d.pop("window", "blackmanharris"),
                                     in_format=fmt, in_scale=in_scale)
            center, rate = 0.0, 1.0              # the modem's centre and rate in the stream that is measured
            if self._duc is not None:
                wide = getattr(self._engine, self._duc + "_cfg")
                center = float(wide.center_freq)
                rate = float(getattr(wide, "decimation", 1)) / float(wide.interpolation)
            spacing = d.pop("spacing", None)
            self._spectrum = dict(center=center, bandwidth=occ * rate, spacing=rate if spacing is None else float(spacing),
                                  mask=d.pop("mask", None))
            if d:
                raise ValueError("spectrum= takes nfft, hop, window, spacing and mask, not %s" % ", ".join(sorted(d)))
            self._engine.set_psd(pcfg)
        self._fec = _fec.as_cfg(fec)
        self._ldpc = _ldpc.as_cfg(ldpc)
        if self._fec is not None and self._ldpc is not None:
            raise ValueError("fec= and ldpc= are two inner codes: a link has one of them")
        self._rs = bool(rs)
        # the coding a packet gets without one of its own (sig only), and the codings of the queued packets
        self._sig = _sig.coding(fec=self._fec, ldpc=self._ldpc, rs=self._rs) if sig else None
        self._pending_coding = []
        self._pending = []
        self._sink = None
        self.symbols_sent = 0
        self.packets_sent = 0

        if getattr(options, "verbose", False):
            self._print_verbage()
        if getattr(options, "log", False):
            self._engine.set_taps(engine._abi.TAP_TX_FREQ, engine._abi.TAP_TX_MAPPER, engine._abi.TAP_TX_IFFT)
        self._log = bool(getattr(options, "log", False))
        if self._log:
            # gr.file_sink opens its file when the flow graph is built (truncating it) and appends for the life of
            # the graph (ofdm.py:123-131)
            for name in ("ofdm_mapper_c.dat", "ofdm_preambles.dat", "ofdm_ifft_c.dat", "ofdm_cp_adder_c.dat"):
                open(name, "wb").close()

    # -- wiring -------------------------------------------------------------------
    def connect(self, sink):
        """Attach the object that receives the modulated samples (``write(iq)``)."""
        self._sink = sink
        return self

    def engine(self):
        return self._engine

    def set_cfr_amplitude(self, ampl):
        """Tell the crest-factor reduction stage (cfr=) the transmit amplitude of the engine (transmit_path does, with
        every set_tx_amplitude): the level its threshold is ``papr_db`` above follows it.  Starts the stage afresh."""
        if self._cfr is None:
            return
        c = self._cfr
        self._cfr_rms = c["level"] * float(ampl)
        thr = c["threshold"] if c["threshold"] is not None else _cfr.threshold_for(c["papr_db"], self._cfr_rms)
        self._engine.set_cfr(_cfr.cfr_cfg(thr, c["window"], out_format=c["out_format"], out_scale=c["out_scale"]))
        self._cfr_live = False

    @property
    def last_cfr(self):
        """cfr.report of the crest-factor reduction stage (cfr=), against the level its threshold was set against: of
        the stream flush(end=True) ended last, or of the running one.  None without the stage or before any sample."""
        if self._cfr is not None and self._cfr_live:
            return _cfr.report(self._engine.cfr_stats(), self._cfr_rms)
        return self._last_cfr

    def set_dpd_coef(self, coef):
        """Another predistorter table (dpd=), between streams: the stage starts afresh.  The table holds for the
        transmit amplitude and peak limit it was trained at."""
        if self._dpd is None:
            raise ValueError("set_dpd_coef() needs ofdm_mod(dpd=)")
        self._engine.set_dpd(_dpd.mempoly_cfg(coef, **self._dpd))
        self._dpd_live = False

    @property
    def last_dpd(self):
        """dpd.report of the predistorter (dpd=): of the stream flush(end=True) ended last, or of the running one.
        None without the stage or before any sample."""
        if self._dpd is not None and self._dpd_live:
            return _dpd.report(self._engine.dpd_stats())
        return self._last_dpd

    def _spectrum_report(self):
        c = self._spectrum
        read = self._engine.psd_read()
        if read["nseg"] == 0:
            return None
        # (a channel as wide as the stream, or adjacent channels that wrap onto it, have no ACLR: none is reported)
        fits = c["spacing"] >= c["bandwidth"] and c["spacing"] + c["bandwidth"] <= 1.0
        return _spectrum.report(read, self._engine.psd_cfg, c["center"], c["bandwidth"], c["spacing"] if fits else None, c["mask"])

    @property
    def last_spectrum(self):
        """spectrum.report of the spectrum measurement (spectrum=): of the stream flush(end=True) ended last, or of the
        running one.  None without the stage or before a whole segment."""
        if self._spectrum is not None and self._spectrum_live:
            return self._spectrum_report()
        return self._last_spectrum

    # -- packets ------------------------------------------------------------------
    def send_pkt(self, payload='', eof=False, coding=None):
        """
        Send the payload.

        @param payload: data to send
        @type payload: bytes (str is encoded latin-1)
        @param coding: this packet's coding on a link with a signal field (ofdm_mod(sig=True); ValueError without):
               a sig.Coding, a coding word, or a dict of sig.coding's keywords (``fec``, ``ldpc``, ``rs``).  None: the
               link's default
        """
        if eof:
            self.flush(end=True)  # gr.message(1): no more packets (ofdm.py:142)
            return
        if isinstance(payload, str):
            payload = payload.encode("latin-1")
        payload = bytes(payload)
        if coding is not None and self._sig is None:
            raise ValueError("send_pkt(coding=) needs ofdm_mod(sig=True): without a signal field the link has one coding")
        if self._sig is not None:
            cod = self._sig if coding is None else (_sig.coding(**coding) if isinstance(coding, dict) else _sig.coding(coding))
            try:
                self._engine.framed_len(_sig.coded_len(len(payload), cod))   # the block, field included, is what gets framed
            except ValueError:
                raise ValueError("len(payload) must be in [0, %d]" % (_sig.max_payload(cod),))
            self._pending.append(payload)
            self._pending_coding.append(cod)
            return
        # same limit and exception as make_packet (ofdm_packet_utils.py:123-126) -- and, like it, raised HERE for
        # the offending packet only: the padded, whitened body must fit the mask too (whiten(), :84-87)
        if self._rs:
            limit = _rs.MAX_PAYLOAD if self._fec is None else _rs.MAX_PAYLOAD_UNDER_FEC
            if self._ldpc is not None:
                limit = _rs.max_payload_under(_ldpc.max_payload(self._ldpc))   # the RS block must fit the inner code at its rate
            if len(payload) > limit:
                raise ValueError("len(payload) must be in [0, %d]" % (limit,))
            block = _rs.coded_len(len(payload))
            # what gets framed: the RS block, or the inner code's block around it
            if self._ldpc is not None:
                block = _ldpc.coded_len(block, self._ldpc)
            self._engine.framed_len(block if self._fec is None else _fec.coded_len(block, self._fec))
            self._pending.append(payload)
            return
        if self._ldpc is not None:
            if len(payload) > _ldpc.max_payload(self._ldpc):
                raise ValueError("len(payload) must be in [0, %d]" % (_ldpc.max_payload(self._ldpc),))
            self._engine.framed_len(_ldpc.coded_len(len(payload), self._ldpc))   # the coded block (at the link's rate) is what gets framed
            self._pending.append(payload)
            return
        if self._fec is not None:
            if len(payload) > _fec.MAX_PAYLOAD:
                raise ValueError("len(payload) must be in [0, %d]" % (_fec.MAX_PAYLOAD,))
            self._engine.framed_len(_fec.coded_len(len(payload), self._fec))   # the coded block (at the link's rate) is what gets framed
            self._pending.append(payload)
            return
        if len(payload) + 4 > len(ofdm_packet_utils.random_mask_tuple):
            raise ValueError("len(payload) must be in [0, %d]" % (len(ofdm_packet_utils.random_mask_tuple),))
        self._engine.framed_len(len(payload))        # ValueError when the whitening mask is exhausted
        self._pending.append(payload)

    def reset_carrier_map(self, carrier_map_new):
        """digital_ofdm_mapper_bcv.reset_carrier_map of the reference's patched GNU Radio
        (the call transmit_path.py:67 has commented out): packets queued so far go out on the old
        map, later ones on the new one."""
        self.flush()
        self._engine.set_carrier_map(carrier_map_new)

    def flush(self, end=False):
        """Modulate everything queued so far; returns the samples (also written to the sink).  With a wideband stage
        (duc= / resample=) they are the wideband stream's next samples (with resample= possibly none yet); ``end=True`` then appends the filter's tail (Q zero
        narrowband samples pushed through) and starts the stage afresh.  With cfr= the samples went through the
        crest-factor reduction stage last and come out half_width samples late; ``end=True`` pushes that many zeros.
        With dpd= the predistorter runs behind all of them; it has no tail, ``end=True`` starts it afresh.  With
        spectrum= the estimator reads what is returned; ``end=True`` keeps its figures as ``last_spectrum`` and starts it
        afresh."""
        end = end and (self._duc is not None or self._cfr is not None or self._dpd is not None or self._spectrum is not None) and (
            self._duc_live or self._cfr_live or self._dpd_live or self._spectrum_live or bool(self._pending))
        if not self._pending and not end:
            return None
        iq = None
        if self._pending:
            pending, self._pending = self._pending, []   # a failing batch never poisons the queue
            codings, self._pending_coding = self._pending_coding, []
            if self._sig is not None:
                pending = self._encode_sig(pending, codings)
            else:
                if self._rs:
                    pending = self._engine.rs_encode(pending)
                if self._fec is not None:
                    pending = self._engine.fec_encode(pending, self._fec)
                if self._ldpc is not None:
                    pending = self._engine.ldpc_encode(pending, self._ldpc)
            iq = self._engine.tx(pending)
            self.symbols_sent += self._engine.last_stats.get("symbols", 0)
            self.packets_sent += len(pending)
            if self._log:
                self._write_logs(iq)
        if self._duc is not None:
            eng = self._engine
            run = getattr(eng, self._duc)        # Engine.duc / Engine.tx_resamp, looked up per call
            parts = [run(iq)] if iq is not None else []
            self._duc_live = True
            if end:
                cfg = getattr(eng, self._duc + "_cfg")
                parts.append(run(np.zeros((cfg.ntaps - 1) // cfg.interpolation, np.complex64)))
                getattr(eng, self._duc + "_reset")(0)
                self._duc_live = False
            iq = np.concatenate(parts) if len(parts) > 1 else parts[0]
        if self._cfr is not None:
            eng = self._engine
            parts = [eng.cfr(iq)] if iq is not None else []
            self._cfr_live = True
            if end:
                parts.append(eng.cfr(np.zeros(_cfr.half_width(eng.cfr_cfg), np.complex64)))
                self._last_cfr = _cfr.report(eng.cfr_stats(), self._cfr_rms)
                eng.cfr_reset()
                self._cfr_live = False
            iq = np.concatenate(parts) if len(parts) > 1 else parts[0]
        if self._dpd is not None:
            eng = self._engine
            if iq is not None:
                iq = eng.dpd(iq)
                self._dpd_live = True
            if end and self._dpd_live:
                self._last_dpd = _dpd.report(eng.dpd_stats())
                eng.dpd_reset()
                self._dpd_live = False
            if iq is None and self._spectrum is None:   # (the end of a stream whose samples all went out before: the stage has no tail)
                return None
        if self._spectrum is not None:
            eng = self._engine
            if iq is not None:
                eng.psd(iq)
                self._spectrum_live = True
            if end and self._spectrum_live:
                self._last_spectrum = self._spectrum_report()
                eng.psd_reset()
                self._spectrum_live = False
            if iq is None:           # (the end of a stream whose samples all went out before: the estimator has no tail)
                return None
        if self._sink is not None:
            self._sink.write(iq)
        return iq

    def _encode_sig(self, payloads, codings):
        """The blocks of a batch on a link with a signal field: the packets grouped by coding, each group through its
        coding's encoders, the fields put in front of all bodies in one call, in the packets' order."""
        eng = self._engine
        groups = {}
        for i, cod in enumerate(codings):
            groups.setdefault(cod, []).append(i)
        bodies = [None] * len(payloads)
        for cod, idx in groups.items():
            part = [payloads[i] for i in idx]
            if cod.rs:
                part = eng.rs_encode(part)
            if cod.codec == _sig.CODEC_FEC:
                part = eng.fec_encode(part, cod.fec)
            elif cod.codec == _sig.CODEC_LDPC:
                part = eng.ldpc_encode(part, cod.ldpc())
            for i, body in zip(idx, part):
                bodies[i] = body
        return eng.sig_encode(codings, bodies)

    def _write_logs(self, iq):
        # the reference's --log probe points (ofdm.py:123-131)
        A = engine._abi
        iqio.file_sink("ofdm_mapper_c.dat", append=True).write(self._engine.tap(A.TAP_TX_MAPPER).reshape(-1))
        iqio.file_sink("ofdm_preambles.dat", append=True).write(self._engine.tap(A.TAP_TX_FREQ).reshape(-1))
        ifft = self._engine.tap(A.TAP_TX_IFFT)
        iqio.file_sink("ofdm_ifft_c.dat", append=True).write(ifft.reshape(-1))
        # ofdm_cp_adder_c.dat: cp_adder's output, BEFORE the 1/sqrt(N) scale block (ofdm.py:113-114,130)
        cp = self._cp_length
        iqio.file_sink("ofdm_cp_adder_c.dat", append=True).write(np.concatenate([ifft[:, ifft.shape[1] - cp:], ifft], axis=1).reshape(-1))

    def add_options(normal, expert):
        """
        Adds OFDM-specific options to the Options Parser
        """
        normal.add_option("-m", "--modulation", type="string", default="bpsk",
                          help="set modulation type (bpsk, qpsk, 8psk, qam{16,64}) [default=%default]")
        expert.add_option("", "--fft-length", type="intx", default=512,
                          help="set the number of FFT bins [default=%default]")
        expert.add_option("", "--occupied-tones", type="intx", default=200,
                          help="set the number of occupied FFT bins [default=%default]")
        expert.add_option("", "--cp-length", type="intx", default=128,
                          help="set the number of bits in the cyclic prefix [default=%default]")
    # Make a static method to call before instantiation
    add_options = staticmethod(add_options)

    def _print_verbage(self):
        """
        Prints information about the OFDM modulator
        """
        print("\nOFDM Modulator:")
        print("Modulation Type: %s" % (self._modulation))
        print("FFT length:      %3d" % (self._fft_length))
        print("Occupied Tones:  %3d" % (self._occupied_tones))
        print("CP length:       %3d" % (self._cp_length))


class ofdm_demod(object):
    """
    Demodulates a received OFDM stream. Based on the options fft_length, occupied_tones, and
    cp_length, this block performs synchronization, FFT, and demodulation of incoming OFDM
    symbols and passes packets up the a higher layer.

    The input is complex baseband.  When packets are demodulated, they are passed to the
    app via the callback.
    """

    def __init__(self, options, callback=None, device_id=0, quality_callback=None, csi=False, iq_format="fc32",
                 iq_scale=None, ddc=None, resample=None, fec=None, soft=None, rs=None, ldpc=None, sig=False):
        """
        @param options: pass modulation options from higher layers (fft length, occupied tones, etc.)
        @param sig: self-describing coded link, the receiving end of ofdm_mod(sig=True): the first 12 bytes of every
            delivered packet are a signal field that names the coding of the body behind it (sig.py).  The fields of
            all delivered packets are decoded in one call (Engine.rx_sig_decode_soft with ``soft``, on the GPU where
            the values lie; Engine.sig_decode on the bytes without), the packets grouped by the word found, and each
            group's bodies go through that coding's decoders (Engine.fec_decode[_soft] / ldpc_decode[_soft], then
            rs_decode; with ``soft`` on the ``last_soft`` values behind the field).  ``callback(ok, payload)`` and the
            returned list carry the decoded payloads and the last stage's verdict, in packet order; a packet whose word
            is not valid comes back as (False, the body as received).  ``last_sig`` holds (word, margin, sig.Coding or
            None) per packet; ``last_fec``, ``last_ldpc`` and ``last_rs`` keep their shapes, with (stage below's
            verdict, 0) / (0, 0) / (stage below's verdict, 0, 0) for a packet whose coding lacks that stage.  The
            field says the coding, so ``fec=`` and ``rs=True`` are a ValueError, ``ldpc=`` may carry ``max_iters``
            only, and ``rs=dict(erasures=...)`` is a ValueError (not on these links yet)
        @param callback:  function of two args: ok, payload
        @type callback: ok: bool; payload: bytes
        @param quality_callback: optional function of three args: ok, payload, quality -- turns on the per-packet
            link quality (a record of engine.QUALITY_DTYPE: SNR, EVM, carrier offset) and is fired per packet next to
            ``callback``
        @param csi: per-subcarrier channel state: ``last_csi`` holds the rows of the packets the last work() / feed()
            returned, carrier_report() / suggest_carrier_map() aggregate the CRC-ok ones (csi.py)
        @param iq_format: "fc32" (complex64 samples) or "sc16": work / feed / flush take int16 arrays of shape (n, 2)
            (flat 2n accepted) and the GPU converts them as it loads (iqio.from_sc16 defines the arithmetic)
        @param iq_scale: value of one LSB of the 16-bit samples (None: 2^-15)
        @param ddc: wideband front end, ``dict(decimation=, center_freq=, taps=None)`` (center_freq in cycles per
            wideband sample): work / feed / flush then take the WIDEBAND stream (in ``iq_format``), the engine's
            stateful tune-and-decimate stage (ddc.py, Engine.ddc) turns it into the complex64 stream at the modem's
            rate and the paths below run on that, unchanged.  ``taps=None``: ddc.design for occupied_tones / fft_length
        @param resample: the same for a capture whose rate is M / L times the modem's, no integer multiple of it:
            ``dict(interpolation=, decimation=, center_freq=0.0, taps=None)``, the engine's rational-rate stage
            (resample.py, Engine.resamp) in the DDC's place; ``taps=None``: resample.design.  Not together with ``ddc``
        @param fec: coded link, as for ofdm_mod: every packet work() / feed() delivers, the CRC-failed ones included, is
            decoded in one batch (Engine.fec_decode) before the callbacks fire.  ``callback(ok, payload)`` and the
            returned list then carry the decoded payload and the verdict of the CRC inside the code; ``last_fec`` holds
            (outer_ok, corrected) per packet -- what the packet CRC said and how many coded bits the decoder changed;
            ``n_ok`` counts decoded verdicts.  Link quality and channel state describe the packets as received
        @param soft: soft-decision receive, ``True`` or ``dict(scale=32)`` (Engine.set_rx_soft): ``last_soft`` holds one
            int8 array per packet the last work() / feed() / flush() returned, 8 values per payload byte.  With ``fec``
            set as well the decoder takes those values on the GPU (Engine.rx_fec_decode_soft) in place of the hard
            bytes; ``last_fec`` keeps its meaning.  Without ``fec`` it only fills ``last_soft``
        @param rs: outer code, as for ofdm_mod: the Reed-Solomon decoder (Engine.rs_decode) runs on every delivered
            packet whatever its CRC said -- behind the inner decoder where ``fec`` is set, hard decisions and ``soft``
            alike.  ``callback(ok, payload)`` and the returned list then carry the corrected payload and the verdict of
            the CRC inside the RS block; ``last_rs`` holds (inner_ok, corrected, failed) per packet -- what the stage
            below said (the inner code's CRC with ``fec``, the packet CRC without), the symbols changed and the
            codewords that could not be decoded; ``last_fec`` keeps its meaning; ``n_ok`` counts outer verdicts.
            ``dict(erasures=True, max_erasures=28)`` decodes with reliabilities (Engine.rs_decode_rel): a codeword that
            fails is tried once more with its weakest symbols, ``max_erasures`` at the most, erased; the reliabilities
            come from ``last_soft`` (Engine.rs_rel_from_soft), so without ``source`` it needs ``soft`` and no ``fec``
            (ValueError).  ``dict(erasures=True, source="fec", max_erasures=28)`` is the same on a concatenated link:
            it needs ``fec``, with or without ``soft``; the inner decoder is then the soft-output one
            (Engine.rx_fec_decode_soft_rel with ``soft``, Engine.fec_decode_rel on the hard bytes without), which
            returns the same payloads and one reliability per decoded byte, and those go to Engine.rs_decode_rel;
            ``last_fec_rel`` holds them, one uint8 array per packet.  ``source="ldpc"`` is the same above ``ldpc`` (below); any other ``source`` is a
            ValueError.  ``last_rs``
            keeps its three fields, ``last_rs_second`` holds the codewords per packet that the second pass decoded
        @param ldpc: coded link with the other inner code, as for ofdm_mod and at the same rate (without ``sig`` no field on the air names
            it), in the place of ``fec`` (both: ValueError):
            every delivered packet goes through the min-sum decoder in one batch (Engine.ldpc_decode on the hard bytes;
            with ``soft`` Engine.rx_ldpc_decode_soft on the values, on the GPU).  ``last_fec`` keeps its shape,
            (outer_ok, corrected) per packet; ``last_ldpc`` holds (iters, cw_failed) per packet.  ``rs=True`` works above
            it as above ``fec``.  ``rs=dict(erasures=True, source="ldpc", max_erasures=28)`` is the concatenated link with
            reliabilities: it needs ``ldpc`` and no ``fec``; the decoder is then k_ldpc_decode_rel
            (Engine.rx_ldpc_decode_soft_rel with ``soft``, Engine.ldpc_decode_rel on the hard bytes without), which returns
            the same payloads and one reliability per decoded byte (min(127, the byte's smallest final |P|), plus 128
            where its codeword met all checks), and those go to Engine.rs_decode_rel as they are; ``last_ldpc_rel``
            holds them, one uint8 array per packet.  ``rs=dict(erasures=True, ...)`` with ``ldpc`` and any other
            ``source``, or none, is a ValueError
        """
        if ddc is not None and resample is not None:
            raise ValueError("ofdm_demod takes ddc= or resample=, not both")
        self._sig = bool(sig)
        self._sig_iters = None       # the LDPC decoder's max_iters on a link with a signal field (None: the default)
        self.last_sig = []           # (word, margin, Coding or None) of the packets the last work() / feed() returned (sig only)
        if self._sig:
            if fec is not None and fec is not False:
                raise ValueError("ofdm_demod(sig=True) takes no fec=: the signal field names the coding")
            if isinstance(rs, dict) and rs.get("erasures"):
                raise ValueError("ofdm_demod(sig=True) does not decode with erasures yet: rs=dict(erasures=...) needs a "
                                 "link whose coding both ends set")
            if rs:
                raise ValueError("ofdm_demod(sig=True) takes no rs=: the signal field says whether the outer code is there")
            if ldpc is not None and ldpc is not False and ldpc is not True:
                if isinstance(ldpc, dict):
                    if set(ldpc) - {"max_iters"}:
                        raise ValueError("ofdm_demod(sig=True): ldpc= may carry max_iters only, the signal field names the rate")
                    ldpc = ldpc.get("max_iters")
                elif isinstance(ldpc, bool) or not isinstance(ldpc, int):
                    raise ValueError("ofdm_demod(sig=True): ldpc= may carry max_iters only, the signal field names the rate")
                if ldpc is not None:
                    self._sig_iters = _ldpc.ldpc_cfg(max_iters=ldpc).max_iters
            fec = rs = ldpc = None
        self._modulation = options.modulation
        self._fft_length = options.fft_length
        self._occupied_tones = options.occupied_tones
        self._cp_length = options.cp_length
        self._snr = getattr(options, "snr", 30)
        self._callback = callback
        self._quality_callback = quality_callback
        self._fec = _fec.as_cfg(fec)
        self._ldpc = _ldpc.as_cfg(ldpc)
        if self._fec is not None and self._ldpc is not None:
            raise ValueError("fec= and ldpc= are two inner codes: a link has one of them")
        if self._ldpc is not None and isinstance(rs, dict) and rs.get("erasures") and rs.get("source") != "ldpc":
            raise ValueError("rs=dict(erasures=True) does not combine with ldpc=: this decoder produces no byte "
                             "reliabilities yet")
        self.last_fec = []           # (outer_ok, corrected) of the packets the last work() / feed() returned (fec / ldpc)
        self.last_ldpc = []          # (iters, cw_failed) of the packets the last work() / feed() returned (ldpc only)
        self._soft = None if (soft is None or soft is False) else soft
        self.last_soft = []          # int8 values of the packets the last work() / feed() returned (soft only)
        self._rs = bool(rs)
        self.last_rs = []            # (inner_ok, corrected, failed) of the packets the last work() / feed() returned (rs only)
        self._rs_rel = None          # ofdm_rs_rel_cfg: decode with reliabilities from last_soft
        self.last_rs_second = []     # codewords per packet the second pass decoded (rs=dict(erasures=True) only)
        self._rs_rel_fec = False     # the reliabilities are the inner decoder's (source="fec"), not the soft demapper's
        self.last_fec_rel = []       # uint8 reliabilities per decoded byte of the packets (source="fec" only)
        self._rs_rel_ldpc = False    # the reliabilities are the min-sum decoder's (source="ldpc")
        self.last_ldpc_rel = []      # uint8 reliabilities per decoded byte of the packets (source="ldpc" only)
        if isinstance(rs, dict):
            opts = dict(rs)
            erasures = bool(opts.pop("erasures", False))
            if not erasures and opts:
                raise ValueError("rs: %s need(s) erasures=True" % ", ".join(sorted(opts)))
            if erasures:
                source = opts.pop("source", None)
                if source is None:
                    if self._soft is None or self._fec is not None:
                        raise ValueError("rs=dict(erasures=True) needs soft= and no fec=: the reliabilities are the soft "
                                         "demapper's; behind the inner decoder ask for its own with source=\"fec\"")
                elif source == "ldpc":
                    if self._fec is not None:
                        raise ValueError("rs=dict(erasures=True, source=\"ldpc\") does not combine with fec=: that decoder's "
                                         "reliabilities are source=\"fec\"")
                    if self._ldpc is None:
                        raise ValueError("rs=dict(erasures=True, source=\"ldpc\") needs ldpc=: the reliabilities are the "
                                         "min-sum decoder's")
                elif source != "fec":
                    raise ValueError("rs: source must be \"fec\" (the inner decoder's reliabilities) or left out "
                                     "(the soft demapper's)")
                elif self._fec is None:
                    raise ValueError("rs=dict(erasures=True, source=\"fec\") needs fec=: the reliabilities are the "
                                     "inner decoder's")
                self._rs_rel_fec = source == "fec"
                self._rs_rel_ldpc = source == "ldpc"
                self._rs_rel = _rs.rs_cfg(**opts)
            self._rs = True

        self._ksfreq = config.make_ksfreq(self._fft_length, self._occupied_tones)  # ofdm.py:210-215
        self._rotated_const = config.rotated_constellation(self._modulation)       # ofdm.py:225-236
        self._engine = engine.Engine(options, device_id=device_id)
        self._ddc = None             # (format, scale, stage) of the wideband front end: stage is "ddc" or "resamp"
        if ddc is not None or resample is not None:
            # the 16-bit format, if any, is the wideband side's: the stage's output (the receiver's input) is complex64
            fmt, scale = iqio.check_format(iq_format), iqio.check_scale(iq_scale, iqio.RX_SCALE)
            occ = self._occupied_tones / float(self._fft_length)
            if ddc is not None:
                d = dict(ddc)
                self._engine.set_ddc(_ddc.ddc_cfg(d.pop("decimation"), d.pop("center_freq"), taps=d.pop("taps", None),
                                                  occupied_fraction=occ, **d))
                self._ddc = (fmt, scale, "ddc")
            else:
                d = dict(resample)
                self._engine.set_resamp(_resample.resamp_cfg(d.pop("interpolation"), d.pop("decimation"),
                                                             d.pop("center_freq", 0.0), taps=d.pop("taps", None),
                                                             occupied_fraction=occ, **d))
                self._ddc = (fmt, scale, "resamp")
        elif iqio.check_format(iq_format) != "fc32":
            self._engine.set_rx_iq_format(iq_format, iq_scale)
        if quality_callback is not None:
            self._engine.set_rx_quality(True)
        # link-quality records of the packets the last work() / feed() returned (quality_callback only)
        self.last_quality = np.zeros(0, engine.QUALITY_DTYPE)
        self.reset_coding_history()  # preamble SNR of the packets delivered with ok set (suggest_coding)
        # channel-state rows of the packets the last work() / feed() returned (csi only), and their running sums
        self._csi = bool(csi)
        if self._csi:
            self._engine.set_rx_csi(True)
        self.last_csi = self._csi_rows(None, [])
        self.reset_carrier_report()
        if self._soft is not None:
            self._engine.set_rx_soft(self._soft)
        self._log = bool(getattr(options, "log", False))
        if self._log:
            self._engine.set_taps(engine._abi.TAP_RX_FFT, engine._abi.TAP_RX_ACQ, engine._abi.TAP_RX_SINK,
                                  engine._abi.TAP_RX_SAMPLER, engine._abi.TAP_RX_SIGMIX, engine._abi.TAP_RX_NCO)
            # file sinks: opened (truncated) with the graph, appended to for its life (ofdm_receiver.py~:144-152,
            # ofdm.py:253-254)
            for name in self._LOG_FILES.values():
                open(name, "wb").close()
        self._log_samples = 0        # samples of the capture the per-sample probe files already hold
        self.n_packets = 0
        self.n_ok = 0
        self._streaming = False      # feed() has data or history pending
        self.reset_stream()
        if getattr(options, "verbose", False):
            self._print_verbage()

    def engine(self):
        return self._engine

    def _tune(self, iq, restart=False):
        """The wideband front end, where one is configured: the next wideband samples in, the narrowband samples they
        complete out (``restart``: the samples begin a new stream)."""
        if self._ddc is None:
            return iq
        eng = self._engine
        fmt, scale, stage = self._ddc
        if restart:
            getattr(eng, stage + "_reset")(0)
        if len(iq) == 0:
            return np.zeros(0, np.complex64)
        run = getattr(eng, stage)        # Engine.ddc / Engine.resamp, looked up per call
        if fmt == "fc32":
            return run(iq)
        eng.set_rx_iq_format(fmt, scale)
        try:
            return run(iq)
        finally:
            eng.set_rx_iq_format("fc32")

    def work(self, iq):
        """Demodulate one contiguous IQ stream; fires the callback per packet and returns the
        list of (ok, payload)."""
        if self._streaming:
            self.reset_stream()  # a one-shot call ends any chunked stream (and drops its carried history)
        iq = self._tune(iq, restart=True)
        pkts = self._engine.rx(iq)
        if self._quality_callback is not None:
            self.last_quality = self._engine.rx_quality()
        if self._csi:
            self.last_csi = self._engine.rx_csi()
            self._csi_accumulate(pkts)
        if self._log:
            self._write_logs()
        if self._soft is not None:
            self.last_soft = self._engine.rx_soft()
        pkts = self._decode(pkts)
        self._deliver(pkts)
        return pkts

    def _decode(self, pkts, sel=None):
        """The coded link's receiving end: the delivered packets' bytes, whatever their CRC said, through the decoder
        (``soft``: their soft values, on the GPU where the last rx() left them; ``sel`` picks the delivered ones among
        that call's packets)."""
        if self._sig:
            return self._decode_sig(pkts, sel)
        if self._fec is not None:
            pkts = self._decode_inner(pkts, sel)
        elif self._ldpc is not None:
            pkts = self._decode_ldpc(pkts, sel)
        if self._rs_rel is not None:
            # (last_soft holds the delivered packets' values, in their order)
            if self._rs_rel_fec:
                rel = self.last_fec_rel
            elif self._rs_rel_ldpc:
                rel = self.last_ldpc_rel
            else:
                rel = self._engine.rs_rel_from_soft(self.last_soft) if pkts else []
            dec = self._engine.rs_decode_rel([p for _, p in pkts], rel, self._rs_rel) if pkts else []
            self.last_rs_second = [s for _, _, _, _, s in dec]
            dec = [d[:4] for d in dec]
            self.last_rs = [(bool(ok), c, f) for (ok, _), (_, _, c, f) in zip(pkts, dec)]
            pkts = [(ok, p) for ok, p, _, _ in dec]
        elif self._rs:
            dec = self._engine.rs_decode([p for _, p in pkts]) if pkts else []
            self.last_rs = [(bool(ok), c, f) for (ok, _), (_, _, c, f) in zip(pkts, dec)]
            pkts = [(ok, p) for ok, p, _, _ in dec]
        return pkts

    def _decode_inner(self, pkts, sel=None):
        if self._rs_rel_fec:
            if self._soft is not None:
                dec = self._engine.rx_fec_decode_soft_rel(self._fec) if pkts else []
                if sel is not None:
                    dec = [dec[i] for i in sel]
            else:
                dec = self._engine.fec_decode_rel([p for _, p in pkts], self._fec) if pkts else []
            self.last_fec_rel = [r for _, _, _, r in dec]
            dec = [d[:3] for d in dec]
        elif self._soft is not None:
            dec = self._engine.rx_fec_decode_soft(self._fec) if pkts else []
            if sel is not None:
                dec = [dec[i] for i in sel]
        else:
            dec = self._engine.fec_decode([p for _, p in pkts], self._fec) if pkts else []
        self.last_fec = [(bool(ok), c) for (ok, _), (_, _, c) in zip(pkts, dec)]
        return [(ok, p) for ok, p, _ in dec]

    def _decode_ldpc(self, pkts, sel=None):
        eng = self._engine
        if self._soft is not None:
            dec = (eng.rx_ldpc_decode_soft_rel if self._rs_rel_ldpc else eng.rx_ldpc_decode_soft)(self._ldpc) if pkts else []
            if sel is not None:
                dec = [dec[i] for i in sel]
        else:
            dec = (eng.ldpc_decode_rel if self._rs_rel_ldpc else eng.ldpc_decode)([p for _, p in pkts], self._ldpc) if pkts else []
        if self._rs_rel_ldpc:
            self.last_ldpc_rel = [d[5] for d in dec]
        self.last_fec = [(bool(ok), d[2]) for (ok, _), d in zip(pkts, dec)]
        self.last_ldpc = [(d[3], d[4]) for d in dec]
        return [(d[0], d[1]) for d in dec]

    def _decode_sig(self, pkts, sel=None):
        """The receiving end of a link with a signal field: every packet's field in one call, the packets grouped by
        the word found, each group through its coding's decoders, the results back in packet order."""
        eng = self._engine
        soft = self._soft is not None
        if soft:
            found = eng.rx_sig_decode_soft() if pkts else []
            if sel is not None:
                found = [found[i] for i in sel]
        else:
            found = eng.sig_decode([p for _, p in pkts]) if pkts else []
        self.last_sig = [(w, m, _sig.coding(w) if _sig.word_valid(w) else None) for w, m in found]
        FB = _sig.FIELD_BYTES
        out = [(False, p[FB:]) for _, p in pkts]                   # what a packet without a valid word comes back as
        self.last_fec = [(bool(ok), 0) for ok, _ in pkts]
        self.last_ldpc = [(0, 0)] * len(pkts)
        self.last_rs = [(bool(ok), 0, 0) for ok, _ in pkts]
        groups = {}
        for i, (_, _, cod) in enumerate(self.last_sig):
            if cod is not None:
                groups.setdefault(cod, []).append(i)
        for cod, idx in groups.items():
            cur = [(bool(pkts[i][0]), pkts[i][1][FB:]) for i in idx]      # (verdict of the stage below, bytes)
            if cod.codec != _sig.CODEC_NONE:
                # (last_soft holds the delivered packets' values, in their order: 8 per byte, the field's first)
                args = ([self.last_soft[i][8 * FB:] for i in idx],) if soft else ([p for _, p in cur],)
                if cod.codec == _sig.CODEC_FEC:
                    dec = (eng.fec_decode_soft if soft else eng.fec_decode)(*args, cod.fec)
                else:
                    dec = (eng.ldpc_decode_soft if soft else eng.ldpc_decode)(*args, cod.ldpc(self._sig_iters))
                    for i, d in zip(idx, dec):
                        self.last_ldpc[i] = (d[3], d[4])
                for i, (below, _), d in zip(idx, cur, dec):
                    self.last_fec[i] = (below, d[2])
                cur = [(d[0], d[1]) for d in dec]
            if cod.rs:
                dec = eng.rs_decode([p for _, p in cur])
                for i, (below, _), d in zip(idx, cur, dec):
                    self.last_rs[i] = (bool(below), d[2], d[3])
                cur = [(d[0], d[1]) for d in dec]
            for i, r in zip(idx, cur):
                out[i] = r
        return out

    def suggest_coding(self, table=None, margin_db=1.0):
        """The coding the link could carry now (sig.suggest_coding): the least redundant coding of ``table`` -- an
        ordered list of (min_snr_db, coding), None: sig.default_table() -- whose threshold plus ``margin_db`` the
        median preamble SNR of the packets delivered with ok set since construction or reset_coding_history() clears;
        None while there is no such packet.  For the transmitter's ``send_pkt(coding=)``.  Needs link quality
        (``quality_callback``): ValueError without."""
        if self._quality_callback is None:
            raise ValueError("suggest_coding() needs link quality: ofdm_demod(..., quality_callback=)")
        return _sig.suggest_coding(self._snr_history, table, margin_db)

    def reset_coding_history(self):
        """Starts the SNR history behind suggest_coding() afresh (it holds the last 65536 packets at the most)."""
        self._snr_history = collections.deque(maxlen=65536)

    def _deliver(self, pkts):
        for i, (ok, payload) in enumerate(pkts):
            self.n_packets += 1
            if ok:
                self.n_ok += 1
                if self._quality_callback is not None:
                    self._snr_history.append(float(self.last_quality[i]["snr_preamble_db"]))
            if self._callback:
                self._callback(ok, payload)  # _queue_watcher_thread.run (ofdm.py:300-305)
            if self._quality_callback is not None:
                self._quality_callback(ok, payload, self.last_quality[i])

    def run(self, source):
        return self.work(source.read_all())

    # -- continuous operation: the flow graph never stops, captures arrive in chunks ------------------
    #
    # The engine demodulates one contiguous array per call and starts every call like the flow graph
    # starts (zero filter / correlator history, detector average 0, NCO phase 0).  feed() stitches
    # chunks so that the packets equal those of ONE call on the whole capture:
    #   * each call sees [carried tail | new chunk]; the tail starts on the sync kernel's tile grid and
    #     reaches back far enough (the detector average looks back 34 tiles; the first tiles of a call
    #     lack correlator history; a packet begun before the horizon can swallow later frames) for
    #     everything after the previous horizon to be detected exactly as in the uncut stream;
    #   * packets whose preamble flag lies beyond `horizon` = end of data minus one maximum-length
    #     packet are held back (their symbols may continue in the next chunk) and come out of the next
    #     call; packets at or before the previous horizon were delivered already and are skipped;
    #   * the NCO continues from the last final flag (phase and step carried over).
    def _stream_geometry(self):
        cfg = self._engine.cfg
        N, CP = cfg.fft_length, cfg.cp_length
        L = N + CP
        T = 2048                                         # SYNC_TILE of csrc/rx_sync.h
        nbits = max(1, int(math.ceil(math.log(cfg.arity, 2))))
        ncar = len(config.carrier_map(cfg.occupied_tones, cfg.occupied_tones, cfg.carrier_map.decode("ascii") or "FE7F"))
        sym_max = int(math.ceil(8.0 * (4 + 4095 + 17) / (ncar * nbits))) + 1
        span = (sym_max + 3) * L + 2 * T + int(cfg.ntaps)
        lookback = (34 + 3 + (L + T - 1) // T) * T
        return T, span, lookback

    def _no_samples(self):
        return np.zeros((0, 2), np.int16) if self._engine.rx_iq_format == "sc16" else np.zeros(0, np.complex64)

    def reset_stream(self):
        self._s_tail = self._no_samples()          # samples carried into the next call (in the receive format)
        self._s_abs = 0                            # absolute index of _s_tail[0]
        self._s_final = -1                         # every flag <= this absolute index has been dealt with
        # settled flags still of interest: (abs flag, phase in 2^-64 turn, step, swallowed); before any flag
        # the NCO idles at phase 0
        self._s_hist = [(0, 0, 0.0, 0)]
        self._s_sym = None                         # (abs flag, symbol ordinal) of the last final flag (link quality)
        self._engine.set_flag_history(None)
        self._engine.set_origin(0)
        if self._ddc is not None:
            getattr(self._engine, self._ddc[2] + "_reset")(0)
        self._streaming = False
        self._log_samples = 0

    def stream_position(self):
        """Where the chunked stream stands, read-only: (absolute index of the first carried sample, samples carried,
        last absolute index up to which every flag is final).  The next feed() demodulates the carried samples plus its
        chunk; flag f of that call (engine().rx_nco_state()) is sample ``first carried + f`` of the stream."""
        return self._s_abs, len(self._s_tail), self._s_final

    def _stream_symbol(self, p):
        """Ordinal, among the sampled symbols of the whole capture, of the preamble of the next final flag p (absolute):
        the sampler's bookkeeping (k_frames) restated over the final flags -- the frame of the flag before takes
        min(timeout + 1, (p - q - 2) // L) data symbols plus its preamble, if it was accepted (q >= N)."""
        cfg = self._engine.cfg
        N, L = cfg.fft_length, cfg.fft_length + cfg.cp_length
        ordinal = 0
        if self._s_sym is not None:
            q, oq = self._s_sym
            ordinal = oq
            if q >= N:
                ordinal += 1 + (min(cfg.sampler_timeout + 1, (p - q - 2) // L) if p >= q + 2 else 0)
        self._s_sym = (p, ordinal)
        return ordinal

    def feed(self, iq, flush=False):
        """Demodulate the next chunk of a continuous capture; returns the packets that became final.
        ``flush=True`` (or flush()) ends the stream: everything still held back is delivered."""
        if self._engine.cfg.sync_mode != engine._abi.SYNC_PN:
            raise ValueError("feed() needs SYNC 'pn': ofdm_sync_fixed's flags are positions in the whole capture")
        # (the first chunk of a stream starts the front end afresh too: a work() before it leaves its capture's end there)
        iq = self._tune(iq, restart=not self._streaming)
        self._streaming = True
        T, span, lookback = self._stream_geometry()
        iq = self._engine._rx_samples(iq)
        buf = np.concatenate([self._s_tail, iq]) if len(self._s_tail) else iq
        base = self._s_abs
        total = base + len(buf)
        horizon = total if flush else total - span           # flags <= horizon are final after this call
        prev_final = self._s_final
        ran = False
        out = []
        qual = []
        sel, rows = [], None    # packets of this call that are delivered now (rows of its channel state)
        soft = []
        if len(buf) and horizon > self._s_final:
            eng = self._engine
            # the settled past: flags inside this buffer keep their known steps (whatever the call re-detects
            # in its unsettled overlap is dropped); the last one before the buffer is the NCO's predecessor
            inside = [f for f in self._s_hist if f[0] >= max(base, 1)]
            before = [f for f in self._s_hist if f[0] < max(base, 1)]
            pred = before[-1] if before else (0, 0, 0.0, 0)
            eng.set_flag_history([f[0] - base for f in inside], [f[2] for f in inside], [f[3] for f in inside],
                                 trust_after=self._s_final - base, pred=(pred[0] - base, pred[1], pred[2]))
            eng.set_origin(base)
            pkts = eng.rx(buf)
            ran = True
            pos = eng.rx_packet_pos().astype(np.int64) + base
            fl, phi, st, sw = eng.rx_nco_state()
            fl = fl.astype(np.int64) + base
            first_sym = {}
            for j in np.flatnonzero((fl > self._s_final) & (fl <= horizon)):
                self._s_hist.append((int(fl[j]), int(phi[j]), float(st[j]), int(sw[j])))
                first_sym[int(fl[j])] = self._stream_symbol(int(fl[j]))
            recs = eng.rx_quality() if self._quality_callback is not None else None
            rows = eng.rx_csi() if self._csi else None
            soft = eng.rx_soft() if self._soft is not None else []
            for i, ((ok, payload), p) in enumerate(zip(pkts, pos)):
                if self._s_final < p <= horizon:
                    out.append((ok, payload))
                    sel.append(i)
                    if recs is not None:
                        # the record as one call on the whole capture gives it: flag and symbol ordinal in the capture
                        r = recs[i].copy()
                        r["flag"] = p
                        r["first_symbol"] = first_sym[int(p)]
                        qual.append(r)
            self._s_final = max(self._s_final, horizon)
        if self._log and ran:
            self._write_logs(base=base, prev_final=prev_final, horizon=horizon, end=total if flush else None)
        if flush:
            self.reset_stream()
        else:
            # carry: one maximum packet (a packet that began before the horizon may swallow frames after
            # it) plus the detector's look-back before the horizon, on the tile grid of the absolute stream
            start = max(base, ((horizon - lookback - span) // T) * T) if horizon > 0 else base
            self._s_tail = buf[start - base:].copy()
            self._s_abs = start
            # history: the flags of the carried part and the last one before it
            keep = [f for f in self._s_hist if f[0] >= max(start, 1)]
            older = [f for f in self._s_hist if f[0] < max(start, 1)]
            self._s_hist = older[-1:] + keep
        if self._quality_callback is not None:
            self.last_quality = np.array(qual, engine.QUALITY_DTYPE)
        if self._csi:
            self.last_csi = self._csi_rows(rows, sel)
            self._csi_accumulate(out)
        if self._soft is not None:
            self.last_soft = [soft[i] for i in sel]
        out = self._decode(out, sel)
        self._deliver(out)
        return out

    # -- per-subcarrier channel state (csi=True) ------------------------------------------------------------------
    def _csi_rows(self, rows, sel):
        occ = int(self._engine.cfg.occupied_tones)
        if rows is None:
            return {"eq": np.zeros((0, occ), np.complex64),
                    **{k: np.zeros((0, occ), np.float32) for k in ("pre_power", "err", "ref")}}
        return {k: v[np.asarray(sel, np.int64)] for k, v in rows.items()}

    def _csi_accumulate(self, pkts):
        """Adds the CRC-ok packets of last_csi to the running per-carrier sums, one packet after the other in delivery
        order (float64): a chunked stream sums exactly what one call on the whole capture sums."""
        acc = self._csi_acc
        for i, (ok, _) in enumerate(pkts):
            if not ok:
                continue
            acc["npkt"] += 1
            for k in ("pre_power", "err", "ref"):
                acc[k] += self.last_csi[k][i].astype(np.float64)
            eq = self.last_csi["eq"][i].astype(np.complex128)
            m = eq.real ** 2 + eq.imag ** 2
            good = np.isfinite(eq.real) & np.isfinite(eq.imag) & (m != 0)
            acc["inv_gain"][good] += 1.0 / m[good]
            acc["ninv"][good] += 1

    def reset_carrier_report(self):
        """Starts the per-carrier sums behind carrier_report() afresh."""
        occ = int(self._engine.cfg.occupied_tones)
        self._csi_acc = {"npkt": 0, "ninv": np.zeros(occ, np.uint32),
                         **{k: np.zeros(occ, np.float64) for k in ("pre_power", "err", "ref", "inv_gain")}}

    def carrier_report(self):
        """Per-carrier SNR (preamble, decision) and gain in dB over the CRC-ok packets delivered since construction or
        reset_carrier_report() (csi.carrier_report; needs csi=True)."""
        if not self._csi:
            raise ValueError("carrier_report() needs ofdm_demod(..., csi=True)")
        return _csi.carrier_report(self._csi_acc, self._engine.cfg)

    def suggest_carrier_map(self, min_snr_db, respect_current=True):
        """Hex carrier map of the carriers whose SNR reaches min_snr_db (csi.suggest_carrier_map): for
        reset_carrier_map() here and the transmitter's set_carrier_map()."""
        return _csi.suggest_carrier_map(self.carrier_report(), self._engine.cfg, min_snr_db, respect_current)

    def flush(self):
        return self.feed(self._no_samples(), flush=True)

    def reset_carrier_map(self, carrier_map_new):
        """The frame sink's side of reset_carrier_map: streams demodulated from now on are
        de-mapped with the new data-carrier set."""
        self._engine.set_carrier_map(carrier_map_new)

    def last_stats(self):
        return dict(self._engine.last_stats)

    _LOG_FILES = {"chan_filt": "ofdm_receiver-chan_filt_c.dat", "fft": "ofdm_receiver-fft_out_c.dat",
                  "acq": "ofdm_receiver-frame_acq_c.dat", "sampler": "ofdm_receiver-sampler_c.dat",
                  "sigmix": "ofdm_receiver-sigmix_c.dat", "nco": "ofdm_receiver-nco_c.dat", "sink": "ofdm_frame_sink_c.dat"}

    def _write_logs(self, base=None, prev_final=None, horizon=None, end=None):
        """The reference's --log probe files (ofdm_receiver.py~:144-152, ofdm.py:253-254): appended to for the life of
        the receiver, like its gr.file_sink blocks.  A one-shot work() appends the whole call.  In a chunked stream
        (feed) every call re-processes a carried tail: only what became FINAL in this call is appended -- per-sample
        probes from the last sample written up to the horizon (the NCO behind it still waits for its flags), symbol
        rows of the frames whose flag lies in (previous horizon, horizon] -- so that the files of a chunked run equal
        those of one call on the whole capture."""
        A = engine._abi
        e = self._engine
        F = self._LOG_FILES

        def app(key, arr):
            iqio.file_sink(F[key], append=True).write(np.ascontiguousarray(arr).reshape(-1))

        y, sm, nco = e.tap(A.TAP_RX_CHAN_FILT), e.tap(A.TAP_RX_SIGMIX), e.tap(A.TAP_RX_NCO)
        fft, acq, samp, sink = e.tap(A.TAP_RX_FFT), e.tap(A.TAP_RX_ACQ), e.tap(A.TAP_RX_SAMPLER), e.tap(A.TAP_RX_SINK)
        if base is None:                      # one-shot
            if not len(sm):                   # (no flag at all: the NCO idles at phase 0, sigmix = chan_filt)
                sm, nco = y, np.ones(len(y), np.complex64)
            for key, arr in (("chan_filt", y), ("sigmix", sm), ("nco", nco), ("fft", fft), ("acq", acq),
                             ("sampler", samp), ("sink", sink)):
                app(key, arr)
            return
        # per-sample probes: absolute samples [log_samples, stop)
        stop = end if end is not None else max(horizon, self._log_samples)
        lo, hi = self._log_samples - base, stop - base
        if hi > lo >= 0:
            app("chan_filt", y[lo:hi])
            # (a call that raised no flag at all computes no NCO: phase 0 throughout, sigmix = chan_filt)
            app("sigmix", sm[lo:hi] if len(sm) else y[lo:hi])
            app("nco", nco[lo:hi] if len(nco) else np.ones(hi - lo, np.complex64))
            self._log_samples = stop
        # symbol rows: frame f of this call holds K[f] + 1 consecutive rows
        fr = e.tap(A.TAP_RX_FRAMES)
        if len(fr):
            rows = np.concatenate([[0], np.cumsum(fr[:, 1].astype(np.int64) + 1)])
            dem = e.tap(A.TAP_RX_DEMAPPED).astype(bool)
            sink_row = np.cumsum(dem) - 1         # row of RX_SINK a demapped symbol went to
            for f in range(len(fr)):
                p = int(fr[f, 0]) + base
                if prev_final < p <= horizon:
                    r0, r1 = int(rows[f]), int(rows[f + 1])
                    app("fft", fft[r0:r1])
                    app("acq", acq[r0:r1])
                    app("sampler", samp[r0:r1])
                    sel = sink_row[r0:r1][dem[r0:r1]]
                    if len(sel):
                        app("sink", sink[sel])

    def add_options(normal, expert):
        """
        Adds OFDM-specific options to the Options Parser
        """
        normal.add_option("-m", "--modulation", type="string", default="bpsk",
                          help="set modulation type (bpsk or qpsk) [default=%default]")
        expert.add_option("", "--fft-length", type="intx", default=512,
                          help="set the number of FFT bins [default=%default]")
        expert.add_option("", "--occupied-tones", type="intx", default=200,
                          help="set the number of occupied FFT bins [default=%default]")
        expert.add_option("", "--cp-length", type="intx", default=128,
                          help="set the number of bits in the cyclic prefix [default=%default]")
    # Make a static method to call before instantiation
    add_options = staticmethod(add_options)

    def _print_verbage(self):
        """
        Prints information about the OFDM demodulator
        """
        print("\nOFDM Demodulator:")
        print("Modulation Type: %s" % (self._modulation))
        print("FFT length:      %3d" % (self._fft_length))
        print("Occupied Tones:  %3d" % (self._occupied_tones))
        print("CP length:       %3d" % (self._cp_length))


def _copy_options(options, **overrides):
    import copy
    o = copy.copy(options)
    for k, v in overrides.items():
        setattr(o, k, v)
    return o


class _ofdm_mod_links(object):
    """What ofdm_mod_channelizer, ofdm_mod_bank and ofdm_mod_resamp_bank share: K plain ofdm_mod produce the narrowband streams and one engine
    owns the stage that places them on the band in one pass.  A subclass checks its arguments, builds the stage's
    configuration and hands both to _open(); ``_stage`` names the engine's stage (Engine.<stage>, <stage>_reset,
    <stage>_cfg) and _history() gives its Q."""

    _stage = None

    def _open(self, opts, configure, device_id):
        self._links = []
        self._live = False       # the band holds samples whose filter tail is still to come
        self._engine = engine.Engine(opts[0], device_id=device_id)
        try:
            configure(self._engine)
            for o in opts:
                self._links.append(ofdm_mod(o, device_id=device_id))
        except Exception:
            self.close()
            raise

    def _history(self, cfg):
        raise NotImplementedError

    def engine(self):
        """The engine that owns the stage."""
        return self._engine

    def links(self):
        """The K per-link modulators, in the order of the list."""
        return list(self._links)

    def send_pkt(self, position, payload=''):
        """Queue ``payload`` on the link at ``position`` of the list (ofdm_mod.send_pkt's checks)."""
        self._links[position].send_pkt(payload)

    def flush(self, end=False):
        """Modulate everything queued on every link and return the band's next samples.  The shorter streams are padded
        with zeros to the longest one's length; the zeros are part of those streams.  The band continues across
        flush() calls (a batch's filter tail comes out in front of the next batch); ``end=True`` appends the tail (Q
        zero columns pushed through) and starts the bank afresh.  None when there is nothing to send.  Every link is
        modulated before the band moves: if one link's batch fails, the batch is dropped on ALL links (as ofdm_mod
        drops a failing batch) and the bank has not run, so the links stay in step."""
        pending = any(m._pending for m in self._links)
        end = end and (self._live or pending)
        if not pending and not end:
            return None
        eng = self._engine
        run = getattr(eng, self._stage)
        cfg = getattr(eng, self._stage + "_cfg")
        parts = []
        if pending:
            try:
                iqs = [m.flush() for m in self._links]
            except Exception:
                for m in self._links:
                    del m._pending[:]
                raise
            n = max(len(iq) for iq in iqs if iq is not None)
            x = np.zeros((len(iqs), n), np.complex64)
            for i, iq in enumerate(iqs):
                if iq is not None:
                    x[i, :len(iq)] = iq
            parts.append(run(x))
            self._live = True
        if end:
            parts.append(run(np.zeros((len(self._links), self._history(cfg)), np.complex64)))
            getattr(eng, self._stage + "_reset")(0)
            self._live = False
        return np.concatenate(parts) if len(parts) > 1 else parts[0]

    def close(self):
        """Closes the bank's engine and the K link engines."""
        for m in self._links:
            m.engine().close()
        self._engine.close()


class ofdm_mod_channelizer(_ofdm_mod_links):
    """
    Modulates links onto a uniform grid of one wideband band: M channels at centre frequencies c/M cycles per wideband
    sample, each interpolated by M (the transmit mirror of ofdm_demod_channelizer, which takes such a band apart).

    K plain ofdm_mod produce the narrowband streams; one engine owns the polyphase-FFT synthesis bank
    (Engine.pfb_synth: one real-tap filter and one M-point transform place all K links in one pass over the band,
    where Engine.duc(iq, add=band) needs one pass per link).
    """

    _stage = "pfb_synth"

    def __init__(self, options, nchannels, channels=None, taps=None, iq_format="fc32", iq_scale=None, device_id=0):
        """
        @param options: one options object for all links, or a list of K for links that differ in modulation
        @param nchannels: M, one of 2, 4, 8, 16, 32, 64: the grid and the interpolation
        @param channels: the K channels that carry a link, in [0, M) or signed in [-M/2, M/2), all different; None:
            all M in order
        @param taps: the shared prototype; None: pfb.synth_design for the largest occupied_tones / fft_length
        @param iq_format, iq_scale: format of the WIDEBAND samples flush() returns, as for ofdm_mod(duc=)
        """
        # every argument is checked before the first engine exists
        channels = None if channels is None else list(channels)
        K = int(nchannels) if channels is None else len(channels)
        if isinstance(options, (list, tuple)):
            opts = list(options)
            if len(opts) != K:
                raise ValueError("ofdm_mod_channelizer needs one options object, or one per channel")
        else:
            opts = [options] * K
        occ = max([o.occupied_tones / float(o.fft_length) for o in opts] or [1.0])
        cfg = _pfb.synth_cfg(nchannels, channels, taps=taps, occupied_fraction=occ,
                             out_format=iqio.check_format(iq_format), out_scale=iq_scale)   # ValueError: M, K, channels, taps
        self._open(opts, lambda e: e.set_pfb_synth(cfg), device_id)

    def _history(self, cfg):
        return (cfg.ntaps - 1) // cfg.nchannels


class ofdm_mod_bank(_ofdm_mod_links):
    """
    Modulates links onto one wideband band at arbitrary centre frequencies: K links that share the interpolation and
    the low-pass prototype and differ in their centre frequency (the transmit counterpart of ofdm_demod_bank, which
    takes such a band apart; ofdm_mod_channelizer is the cheaper way where the links sit on the c/M grid).

    K plain ofdm_mod produce the narrowband streams; one engine owns the DUC bank (Engine.duc_bank: all K links in one
    pass over the band, where Engine.duc(iq, add=band) needs one pass per link).
    """

    _stage = "duc_bank"

    def __init__(self, options, center_freqs, interpolation, taps=None, iq_format="fc32", iq_scale=None, device_id=0):
        """
        @param options: one options object for all links, or a list of K for links that differ in modulation
        @param center_freqs: K centre frequencies, cycles per wideband sample, each in [-0.5, 0.5]
        @param interpolation: wideband rate over the modem's rate, 1..64
        @param taps: the shared prototype; None: duc.design for the largest occupied_tones / fft_length of the links
        @param iq_format, iq_scale: format of the WIDEBAND samples flush() returns, as for ofdm_mod(duc=)
        """
        # every argument is checked before the first engine exists
        fcs = [float(f) for f in np.asarray(center_freqs, np.float64).reshape(-1)]
        if isinstance(options, (list, tuple)):
            opts = list(options)
            if len(opts) != len(fcs):
                raise ValueError("ofdm_mod_bank needs one options object, or one per centre frequency")
        else:
            opts = [options] * len(fcs)
        occ = max([o.occupied_tones / float(o.fft_length) for o in opts] or [1.0])
        cfg = _duc.bank_cfg(interpolation, fcs, taps=taps, occupied_fraction=occ,
                            out_format=iqio.check_format(iq_format), out_scale=iq_scale)   # ValueError: K, fc, L, taps
        self._open(opts, lambda e: e.set_duc_bank(cfg), device_id)

    def _history(self, cfg):
        return (cfg.ntaps - 1) // cfg.interpolation


class ofdm_mod_resamp_bank(_ofdm_mod_links):
    """
    Modulates links onto one wideband band whose rate is no integer multiple of the modem's: K links that share the
    ratio L / M and the low-pass prototype and differ in their centre frequency (the transmit counterpart of
    ofdm_demod_resamp_bank, which takes such a band apart at the mirror ratio M / L).

    K plain ofdm_mod produce the narrowband streams; one engine owns the transmit resampler bank
    (Engine.tx_resamp_bank: all K links in one pass over the band, where Engine.tx_resamp(iq, add=band) needs one pass
    per link).
    """

    _stage = "tx_resamp_bank"

    def __init__(self, options, center_freqs, interpolation, decimation, taps=None, iq_format="fc32", iq_scale=None,
                 device_id=0):
        """
        @param options: one options object for all links, or a list of K for links that differ in modulation
        @param center_freqs: K centre frequencies, cycles per wideband sample, each in [-0.5, 0.5]
        @param interpolation, decimation: L and M, each 1..64: the wideband rate is L / M times the modem's
        @param taps: the shared prototype; None: tx_resample.design for the largest occupied_tones / fft_length of the links
        @param iq_format, iq_scale: format of the WIDEBAND samples flush() returns, as for ofdm_mod(duc=)
        """
        # every argument is checked before the first engine exists
        fcs = [float(f) for f in np.asarray(center_freqs, np.float64).reshape(-1)]
        if isinstance(options, (list, tuple)):
            opts = list(options)
            if len(opts) != len(fcs):
                raise ValueError("ofdm_mod_resamp_bank needs one options object, or one per centre frequency")
        else:
            opts = [options] * len(fcs)
        occ = max([o.occupied_tones / float(o.fft_length) for o in opts] or [1.0])
        cfg = _tx_resample.bank_cfg(interpolation, decimation, fcs, taps=taps, occupied_fraction=occ,
                                    out_format=iqio.check_format(iq_format), out_scale=iq_scale)   # ValueError: K, fc, L, M, taps
        self._open(opts, lambda e: e.set_tx_resamp_bank(cfg), device_id)

    def _history(self, cfg):
        return (cfg.ntaps - 1) // cfg.interpolation


class _ofdm_demod_links(object):
    """What ofdm_demod_bank, ofdm_demod_channelizer and ofdm_demod_resamp_bank share, the receive mirror of
    _ofdm_mod_links: one engine owns the stage that takes the K narrowband streams out of the capture in one pass, and
    each stream goes to a plain ofdm_demod of its own.  A subclass checks its arguments with _check(), builds the
    stage's configuration and hands both to _open(); ``_stage`` names the engine's stage (Engine.<stage>,
    set_<stage>, <stage>_reset)."""

    _stage = None

    def _check(self, options, K, per, callback, position, iq_format, iq_scale):
        """The checks the three classes share, in their order: ``options`` is one object or a list of K (``per``
        names what a list holds one for), ``callback`` a function of (``position``, ok, payload).  Returns the K
        options, the wideband format and scale and the largest occupied fraction."""
        if isinstance(options, (list, tuple)):
            opts = list(options)
            if len(opts) != K:
                raise ValueError("%s needs one options object, or one per %s" % (type(self).__name__, per))
        else:
            opts = [options] * K
        if callback is not None and not callable(callback):
            raise ValueError("callback must be callable: callback(%s, ok, payload)" % position)
        fmt, scale = iqio.check_format(iq_format), iqio.check_scale(iq_scale, iqio.RX_SCALE)
        occ = max([o.occupied_tones / float(o.fft_length) for o in opts] or [1.0])
        return opts, fmt, scale, occ

    def _open(self, opts, cfg, callback, fmt, scale, device_id):
        self._callback = callback
        self._links = []
        self._engine = engine.Engine(opts[0], device_id=device_id)
        try:
            if fmt != "fc32":
                self._engine.set_rx_iq_format(fmt, scale)
            getattr(self._engine, "set_" + self._stage)(cfg)
            for i, o in enumerate(opts):
                cb = (lambda ok, payload, link=i: self._callback(link, ok, payload)) if callback is not None else None
                self._links.append(ofdm_demod(o, callback=cb, device_id=device_id))
        except Exception:
            self.close()
            raise
        self._streaming = False

    def engine(self):
        """The engine that owns the bank."""
        return self._engine

    def links(self):
        """The K per-link demodulators, in the order of the centre frequencies."""
        return list(self._links)

    def _tune(self, iq, restart):
        eng = self._engine
        if restart:
            getattr(eng, self._stage + "_reset")(0)
        if len(iq) == 0:
            return np.zeros((len(self._links), 0), np.complex64)
        return getattr(eng, self._stage)(iq)

    def work(self, iq):
        """Demodulate one contiguous wideband stream: a list of K packet lists."""
        self._streaming = False
        y = self._tune(iq, restart=True)
        return [d.work(y[i]) for i, d in enumerate(self._links)]

    def feed(self, iq, flush=False):
        """The next chunk of a continuous wideband capture: per link, the packets that became final."""
        y = self._tune(iq, restart=not self._streaming)
        self._streaming = not flush
        return [d.feed(y[i], flush) for i, d in enumerate(self._links)]

    def flush(self):
        return self.feed(np.zeros((0, 2), np.int16) if self._engine.rx_iq_format == "sc16" else np.zeros(0, np.complex64),
                         flush=True)

    def close(self):
        """Closes the bank's engine and the K link engines."""
        for d in self._links:
            d.engine().close()
        self._engine.close()


class ofdm_demod_bank(_ofdm_demod_links):
    """
    Demodulates every link of one wideband capture: K links that share the decimation and the low-pass prototype and
    differ in their centre frequency (the receive-side counterpart of adding links onto one band with Engine.duc).

    One engine owns the DDC bank (Engine.ddc_bank: all K narrowband streams from one pass over the wideband samples);
    each stream goes to a plain ofdm_demod of its own.  Link i returns what ofdm_demod(options_i, ddc=dict(decimation=,
    center_freq=center_freqs[i], taps=)) returns on the same samples.
    """

    _stage = "ddc_bank"

    def __init__(self, options, center_freqs, decimation, taps=None, callback=None, iq_format="fc32", iq_scale=None,
                 device_id=0):
        """
        @param options: one options object for all links, or a list of K for links that differ in modulation
        @param center_freqs: K centre frequencies, cycles per wideband sample, each in [-0.5, 0.5]
        @param decimation: wideband rate over the modem's rate, 1..64
        @param taps: the shared prototype; None: ddc.design for the largest occupied_tones / fft_length of the links
        @param callback: function of three args: link, ok, payload -- per call fired for link 0's packets, then link
            1's, and so on
        @param iq_format, iq_scale: format of the WIDEBAND samples, as for ofdm_demod
        """
        # every argument is checked before the first engine exists
        fcs = [float(f) for f in np.asarray(center_freqs, np.float64).reshape(-1)]
        opts, fmt, scale, occ = self._check(options, len(fcs), "centre frequency", callback, "link", iq_format, iq_scale)
        cfg = _ddc.bank_cfg(decimation, fcs, taps=taps, occupied_fraction=occ)   # ValueError: K, frequencies, R, taps
        self._open(opts, cfg, callback, fmt, scale, device_id)


class ofdm_demod_channelizer(ofdm_demod_bank):
    """
    Demodulates links that sit on a uniform grid of one wideband capture: M channels at centre frequencies c/M cycles
    per wideband sample, each decimated by M (a radio that watches every slot of a band).  ofdm_demod_bank with the
    polyphase-FFT channeliser (Engine.pfb) in the DDC bank's place: one real-tap filter and one M-point transform serve
    all channels, up to 64 of them.  work, feed, flush, links and close are the bank's.
    """

    _stage = "pfb"

    def __init__(self, options, nchannels, channels=None, taps=None, callback=None, iq_format="fc32", iq_scale=None,
                 device_id=0):
        """
        @param options: one options object for all kept channels, or a list of K for links that differ in modulation
        @param nchannels: M, one of 2, 4, 8, 16, 32, 64: the grid and the decimation
        @param channels: the K channels to demodulate, in [0, M) or signed in [-M/2, M/2); None: all M in order
        @param taps: the shared prototype; None: pfb.design for the largest occupied_tones / fft_length of the links
        @param callback: function of three args: channel_position, ok, payload -- per call fired for position 0's
            packets, then position 1's, and so on
        @param iq_format, iq_scale: format of the WIDEBAND samples, as for ofdm_demod
        """
        # every argument is checked before the first engine exists
        channels = None if channels is None else list(channels)
        K = int(nchannels) if channels is None else len(channels)
        opts, fmt, scale, occ = self._check(options, K, "kept channel", callback, "channel_position", iq_format, iq_scale)
        cfg = _pfb.pfb_cfg(nchannels, channels, taps=taps, occupied_fraction=occ)   # ValueError: M, K, channels, taps
        self._open(opts, cfg, callback, fmt, scale, device_id)


class ofdm_demod_resamp_bank(ofdm_demod_bank):
    """
    Demodulates every link of one wideband capture whose rate is M / L times the modem's, no integer multiple of it
    (a recorder's 25 MS/s file that holds several 10 MS/s links): K links that share the ratio and the low-pass
    prototype and differ in their centre frequency.  ofdm_demod_bank with the resampler bank (Engine.resamp_bank) in
    the DDC bank's place: link i returns what ofdm_demod(options_i, resample=dict(interpolation=, decimation=,
    center_freq=center_freqs[i], taps=)) returns on the same samples.  work, feed, flush, links and close are the
    bank's.
    """

    _stage = "resamp_bank"

    def __init__(self, options, center_freqs, interpolation, decimation, taps=None, callback=None, iq_format="fc32",
                 iq_scale=None, device_id=0):
        """
        @param options: one options object for all links, or a list of K for links that differ in modulation
        @param center_freqs: K centre frequencies, cycles per wideband sample, each in [-0.5, 0.5]
        @param interpolation, decimation: L and M, 1..64 each: the modem's rate is L / M times the capture's
        @param taps: the shared prototype at L times the wideband rate; None: resample.design for the largest
            occupied_tones / fft_length of the links
        @param callback: function of three args: link, ok, payload -- per call fired for link 0's packets, then link
            1's, and so on
        @param iq_format, iq_scale: format of the WIDEBAND samples, as for ofdm_demod
        """
        # every argument is checked before the first engine exists
        fcs = [float(f) for f in np.asarray(center_freqs, np.float64).reshape(-1)]
        opts, fmt, scale, occ = self._check(options, len(fcs), "centre frequency", callback, "link", iq_format, iq_scale)
        # ValueError: K, frequencies, L, M, taps
        cfg = _resample.bank_cfg(interpolation, decimation, fcs, taps=taps, occupied_fraction=occ)
        self._open(opts, cfg, callback, fmt, scale, device_id)
