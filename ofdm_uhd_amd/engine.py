"""Thin Python wrapper over the C ABI of libofdm_hip.so (include/ofdm_hip.h).

``Engine`` owns one ``ofdm_handle`` (one GPU, one HIP stream).  In host mode it
takes / returns NumPy arrays; in device mode (``device_ptrs=True``) the bulk
arguments are raw device pointers (e.g. ``torch.Tensor.data_ptr()``), which is
what bench.py uses so that nothing crosses PCIe inside the timed region.

IQ samples are complex64 unless a direction was switched to 16-bit IQ
(``set_rx_iq_format("sc16")`` / ``set_tx_iq_format("sc16")``): then they are
``int16`` arrays of shape ``(n, 2)`` (iqio.to_sc16 / from_sc16 define the
conversion), and a device pointer points to int16 pairs.

There is no CPU implementation behind this class: if the library is missing,
importing fails loudly (see _abi.load).
"""
import ctypes as C
import importlib

import numpy as np

from . import _abi, config, iqio


def _quality_dtype():
    st = _abi.ofdm_pkt_quality
    conv = {C.c_uint64: np.uint64, C.c_uint32: np.uint32, C.c_int32: np.int32, C.c_float: np.float32}
    return np.dtype({"names": [f for f, _ in st._fields_],
                     "formats": [conv[t] for _, t in st._fields_],
                     "offsets": [getattr(st, f).offset for f, _ in st._fields_],
                     "itemsize": C.sizeof(st)})


# one ofdm_pkt_quality record (include/ofdm_hip.h) as a NumPy structured dtype
QUALITY_DTYPE = _quality_dtype()


class EngineError(RuntimeError):
    def __init__(self, code, msg):
        RuntimeError.__init__(self, "libofdm_hip: %s (code %d)" % (msg, code))
        self.code = code


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


# the slots of the memory-polynomial stage by the names Engine gives them
_MEMPOLY_SLOT = {"dpd": _abi.OFDM_MEMPOLY_DPD, "pa": _abi.OFDM_MEMPOLY_PA}


def _u32(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def _u64(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint64))


def pack_payloads(payloads):
    """list of bytes -> (blob uint8, offsets uint64, lengths uint32)"""
    lens = np.array([len(p) for p in payloads], np.uint32)
    offs = np.zeros(max(len(payloads), 1), np.uint64)
    if len(payloads) > 1:
        offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    blob = np.frombuffer(b"".join(bytes(p) for p in payloads), np.uint8)
    if blob.size == 0:
        blob = np.zeros(1, np.uint8)
    return np.ascontiguousarray(blob), offs[:len(payloads)] if len(payloads) else offs[:0], lens


def _pack_values(values, strict=False):
    """list of int8 arrays, 8 values per coded byte -> (blob int8, offsets uint64 in values, lengths uint32 in bytes): what
    the ``*_soft`` calls take.  The blob ends in 8 zero values of padding, so that no offset points past it.  A length
    that is no multiple of 8 is handed on as the length 1, which is no block to any decoder; with ``strict`` (the outer
    code's reliabilities, which have no such answer) it raises ValueError."""
    vals = [np.ascontiguousarray(v, np.int8).reshape(-1) for v in values]
    if strict and any(len(v) % 8 for v in vals):
        raise ValueError("rs: 8 values per byte")
    lens = np.array([len(v) // 8 if len(v) % 8 == 0 else 1 for v in vals], np.uint32)
    offs = np.zeros(max(len(vals), 1), np.uint64)
    if len(vals) > 1:
        offs[1:] = np.cumsum([len(v) for v in vals[:-1]], dtype=np.uint64)
    return np.concatenate(vals + [np.zeros(8, np.int8)]), offs[:len(vals)], lens


class Engine(object):
    def __init__(self, options=None, cfg=None, pad_for_usrp=False, device_ptrs=False, device_id=0, **cfg_kw):
        self._lib = _abi.load()
        if cfg is None:
            cfg = config.make_cfg(options, pad_for_usrp=pad_for_usrp, device_ptrs=device_ptrs,
                                  device_id=device_id, **cfg_kw)
        self.cfg = cfg
        self.device_ptrs = bool(cfg.flags & _abi.OFDM_F_DEVICE_PTRS)
        self._h = C.c_void_p(None)
        rc = self._lib.ofdm_create(C.byref(cfg), C.byref(self._h))
        if rc != _abi.OFDM_OK:
            msg = self._lib.ofdm_last_error(None)
            self._h = C.c_void_p(None)
            if rc == _abi.OFDM_E_INVAL:
                raise ValueError((msg or b"").decode())
            raise EngineError(rc, (msg or b"").decode())
        self.N = cfg.fft_length
        self.CP = cfg.cp_length
        self.L = self.N + self.CP
        self.occ = cfg.occupied_tones
        self.last_stats = {}
        self._rx_sense_cfg = None
        self.ddc_cfg = None     # the wideband front end's configuration in force (set_ddc), None without one
        self.ddc_bank_cfg = None  # the DDC bank's configuration in force (set_ddc_bank), None without one
        self.resamp_cfg = None  # the rational-rate front end's configuration in force (set_resamp), None without one
        self.resamp_bank_cfg = None  # the resampler bank's configuration in force (set_resamp_bank), None without one
        self.duc_cfg = None     # the wideband transmit stage's configuration in force (set_duc), None without one
        self.tx_resamp_cfg = None  # the rational-rate transmit stage's configuration in force (set_tx_resamp), None without one
        self.pfb_cfg = None     # the channeliser's configuration in force (set_pfb), None without one
        self.pfb_synth_cfg = None  # the synthesis bank's configuration in force (set_pfb_synth), None without one
        self.duc_bank_cfg = None  # the DUC bank's configuration in force (set_duc_bank), None without one
        self.tx_resamp_bank_cfg = None  # the transmit resampler bank's configuration in force (set_tx_resamp_bank), None without one
        self.multipath_cfg = None  # the propagation channel's configuration in force (set_multipath), None without one
        self.cfr_cfg = None  # the crest-factor reduction stage's configuration in force (set_cfr), None without one
        self.dpd_cfg = None  # the predistorter's configuration in force (set_dpd), None without one
        self.pa_cfg = None   # the amplifier model's configuration in force (set_pa), None without one
        self.psd_cfg = None  # the spectrum stage's configuration in force (set_psd), None without one
        self.rx_iq_format = self.tx_iq_format = "fc32"
        self.rx_iq_scale, self.tx_iq_scale = iqio.RX_SCALE, iqio.TX_SCALE

    # -- plumbing ---------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.ofdm_destroy(self._h)
            self._h = C.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc == _abi.OFDM_OK:
            return
        msg = (self._lib.ofdm_last_error(self._h) or b"").decode()
        if rc == _abi.OFDM_E_INVAL:
            raise ValueError(msg)
        raise EngineError(rc, msg)

    def set_stream(self, hip_stream_ptr):
        self._check(self._lib.ofdm_set_stream(self._h, C.c_void_p(hip_stream_ptr)))

    def set_tx_amplitude(self, ampl):
        self._check(self._lib.ofdm_set_tx_amplitude(self._h, float(ampl)))

    def set_carrier_map(self, carriers="FE7F"):
        """reset_carrier_map of the reference's patched mapper (transmit_path.py:67): swap the data
        carrier map of BOTH directions of this engine, e.g. to hex_conv's output clipped to
        occupied_tones/4 digits (sensing_and_tramsmitting.py:470)."""
        self._check(self._lib.ofdm_set_carrier_map(self._h, (carriers or "").encode("ascii")))
        self.cfg.carrier_map = (carriers or "").encode("ascii")   # the host copy follows the handle (stream geometry)

    def set_channel(self, sigma=0.0, cfo=0.0, seed=0xC0FFEE, stream_id=0, lead=0, tail=0, enable=True):
        if not enable:
            self._check(self._lib.ofdm_set_channel(self._h, None))
            return
        ch = _abi.ofdm_chan(sigma=sigma, cfo=cfo, seed=seed, stream_id=stream_id, lead_samples=lead,
                            tail_samples=tail)
        self._check(self._lib.ofdm_set_channel(self._h, C.byref(ch)))

    def set_rx_iq_format(self, fmt="fc32", scale=None):
        """Sample format of what rx / rx_submit_device / rx_device / sense are handed from now on: "fc32"
        (complex64) or "sc16" (int16 (n, 2); sample = int16 * scale, default 2^-15)."""
        scale = iqio.check_scale(scale, iqio.RX_SCALE)
        self._check(self._lib.ofdm_set_rx_iq_format(self._h, iqio.FORMATS.index(iqio.check_format(fmt)), scale))
        self.rx_iq_format, self.rx_iq_scale = fmt, scale

    def set_tx_iq_format(self, fmt="fc32", scale=None):
        """Sample format of what tx / tx_device produce from now on: "fc32" or "sc16" (int16 (n, 2) =
        clamp(rint(sample * scale)), default scale 2^15)."""
        scale = iqio.check_scale(scale, iqio.TX_SCALE)
        self._check(self._lib.ofdm_set_tx_iq_format(self._h, iqio.FORMATS.index(iqio.check_format(fmt)), scale))
        self.tx_iq_format, self.tx_iq_scale = fmt, scale

    def _rx_samples(self, iq):
        """A host array in the receive format, contiguous; a dtype of the other format is refused, never reinterpreted."""
        if self.rx_iq_format == "sc16":
            return iqio.as_sc16(iq)
        if np.asarray(iq).dtype == np.int16:
            raise ValueError("int16 samples handed to an engine in fc32 mode (set_rx_iq_format(\"sc16\") first)")
        return np.ascontiguousarray(iq, np.complex64)

    def set_taps(self, *taps):
        mask = 0
        for t in taps:
            mask |= 1 << t
        self._check(self._lib.ofdm_set_taps(self._h, mask))

    def prof_enable(self, on=True):
        self._check(self._lib.ofdm_prof_enable(self._h, 1 if on else 0))

    def prof_reset(self):
        self._check(self._lib.ofdm_prof_reset(self._h))

    def prof(self):
        out = {}
        for k in range(_abi.K_COUNT):
            ms = C.c_double(0)
            n = C.c_uint64(0)
            self._check(self._lib.ofdm_prof_get(self._h, k, C.byref(ms), C.byref(n)))
            out[self._lib.ofdm_kernel_name(k).decode()] = (ms.value, n.value)
        return out

    # -- framing ----------------------------------------------------------------
    def framed_len(self, payload_len):
        n = C.c_uint32(0)
        self._check(self._lib.ofdm_framed_len(self._h, int(payload_len), C.byref(n)))
        return n.value

    def make_packets(self, payloads):
        """Batched make_packet; host mode only.  Returns list of bytes."""
        assert not self.device_ptrs
        blob, offs, lens = pack_payloads(payloads)
        total = 0
        for ln in lens:
            total += self.framed_len(int(ln))
        out = np.zeros(max(total, 1), np.uint8)
        foff = np.zeros(len(payloads) + 1, np.uint64)
        self._check(self._lib.ofdm_make_packets(self._h, _ptr(blob), offs.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                lens.ctypes.data_as(C.POINTER(C.c_uint32)), len(payloads), _ptr(out),
                                                len(out), foff.ctypes.data_as(C.POINTER(C.c_uint64))))
        return [out[int(foff[i]):int(foff[i + 1])].tobytes() for i in range(len(payloads))]

    # -- TX ----------------------------------------------------------------------
    def tx_frame_count(self, lens):
        lens = np.ascontiguousarray(lens, np.uint32)
        nsym = C.c_uint64(0)
        nsamp = C.c_uint64(0)
        self._check(self._lib.ofdm_tx_frame_count(self._h, lens.ctypes.data_as(C.POINTER(C.c_uint32)), len(lens),
                                                  C.byref(nsym), C.byref(nsamp)))
        return nsym.value, nsamp.value

    def tx(self, payloads):
        """Host mode: list of payload bytes -> IQ in the transmit format (incl. channel lead/tail if set)."""
        assert not self.device_ptrs
        blob, offs, lens = pack_payloads(payloads)
        _, nsamp = self.tx_frame_count(lens)
        iq = np.zeros((max(nsamp, 1), 2), np.int16) if self.tx_iq_format == "sc16" else np.zeros(max(nsamp, 1), np.complex64)
        ns = C.c_uint64(0)
        st = _abi.ofdm_stats()
        self._check(self._lib.ofdm_tx(self._h, _ptr(blob), offs.ctypes.data_as(C.POINTER(C.c_uint64)),
                                      lens.ctypes.data_as(C.POINTER(C.c_uint32)), len(payloads), _ptr(iq), len(iq),
                                      C.byref(ns), C.byref(st)))
        self.last_stats = st.as_dict()
        return iq[:ns.value]

    def wait(self):
        """Block until everything queued on the handle's stream (tx_device(wait=False)) is done."""
        self._check(self._lib.ofdm_wait(self._h))

    def tx_device(self, payload_ptr, offs, lens, iq_ptr, iq_cap, wait=True):
        """Device mode: payload bytes and IQ are device pointers; offs/lens are NumPy host arrays.
        ``wait=False`` only queues the work (ofdm_tx_async): a following rx_device() on the same engine
        is ordered behind it on the stream, so a TX -> RX loopback needs no host round trip in between."""
        assert self.device_ptrs
        ns = C.c_uint64(0)
        st = _abi.ofdm_stats()
        fn = self._lib.ofdm_tx if wait else self._lib.ofdm_tx_async
        self._check(fn(self._h, C.c_void_p(payload_ptr), offs.ctypes.data_as(C.POINTER(C.c_uint64)),
                                      lens.ctypes.data_as(C.POINTER(C.c_uint32)), len(lens), C.c_void_p(iq_ptr),
                                      int(iq_cap), C.byref(ns), C.byref(st)))
        self.last_stats = st.as_dict()
        return ns.value

    def channel(self, iq, sigma=0.0, cfo=0.0, seed=0xC0FFEE, stream_id=0, index0=0):
        """Host mode: returns a new array with the synthetic channel applied."""
        assert not self.device_ptrs
        if np.asarray(iq).dtype == np.int16:
            raise ValueError("channel() works on complex64 samples only (ofdm_channel is float32 whatever the IQ formats)")
        out = np.ascontiguousarray(iq, np.complex64).copy()
        ch = _abi.ofdm_chan(sigma=sigma, cfo=cfo, seed=seed, stream_id=stream_id, lead_samples=0, tail_samples=0)
        self._check(self._lib.ofdm_channel(self._h, _ptr(out), len(out), C.byref(ch), index0))
        return out

    # -- RX ----------------------------------------------------------------------
    def rx(self, iq, max_pkts=None, payload_cap=None):
        """Host mode: IQ in the receive format -> list of (ok, payload) in stream order, exactly the pairs the
        reference hands to its rx callback (ofdm.py:300-305)."""
        assert not self.device_ptrs
        iq = self._rx_samples(iq)
        if max_pkts is None:
            max_pkts = len(iq) // self.L + 16
        if payload_cap is None:
            payload_cap = max_pkts * 64 + len(iq)  # bits never exceed 8 per sample
        pay = np.zeros(max(payload_cap, 1), np.uint8)
        off = np.zeros(max_pkts + 1, np.uint64)
        ln = np.zeros(max(max_pkts, 1), np.uint32)
        ok = np.zeros(max(max_pkts, 1), np.uint8)
        npk = C.c_int(0)
        st = _abi.ofdm_stats()
        rc = self._lib.ofdm_rx(self._h, _ptr(iq) if len(iq) else None, len(iq), _ptr(pay), len(pay),
                               off.ctypes.data_as(C.POINTER(C.c_uint64)), ln.ctypes.data_as(C.POINTER(C.c_uint32)),
                               ok.ctypes.data_as(C.POINTER(C.c_uint8)), max_pkts, C.byref(npk), C.byref(st))
        self.last_stats = st.as_dict()
        self._check(rc)
        return [(bool(ok[i]), pay[int(off[i]):int(off[i]) + int(ln[i])].tobytes()) for i in range(npk.value)]

    def snr(self):
        """digital_ofdm_frame_acquisition.snr() (digital_swig.py:4231-4239): GNU Radio 3.6.0 never updates the estimate
        it initialises to 0."""
        v = C.c_float(-1.0)
        self._check(self._lib.ofdm_rx_snr(self._h, C.byref(v)))
        return float(v.value)

    def set_rx_quality(self, on=True):
        """Per-packet link quality (SNR, EVM, carrier offset) for the following rx() / rx_device() calls."""
        self._check(self._lib.ofdm_set_rx_quality(self._h, 1 if on else 0))

    def rx_quality(self):
        """Link quality of the packets the last rx() / rx_device() call returned, one record per packet in the same
        order: a NumPy structured array of QUALITY_DTYPE (the fields of ofdm_pkt_quality).  ValueError if that call
        ran without set_rx_quality(True)."""
        n = C.c_int(0)
        self._check(self._lib.ofdm_rx_quality(self._h, None, 0, C.byref(n)))
        out = np.zeros(max(n.value, 1), QUALITY_DTYPE)
        if n.value:
            self._check(self._lib.ofdm_rx_quality(self._h, _ptr(out), n.value, C.byref(n)))
        return out[:n.value]

    def set_rx_csi(self, on=True):
        """Per-subcarrier channel state (equaliser, preamble power, decision error / reference energy per carrier) for
        the following rx() / rx_device() calls."""
        self._check(self._lib.ofdm_set_rx_csi(self._h, 1 if on else 0))

    def rx_csi(self, first=0, count=None):
        """Channel-state rows of the packets the last rx() / rx_device() call returned, in the same order, packets
        [first, first + count) (count None: to the end): a dict of ``eq`` complex64 and ``pre_power``, ``err``,
        ``ref`` float32, each [count, occupied_tones] (definitions: include/ofdm_hip.h).  ValueError if that call ran
        without set_rx_csi(True) or the range lies outside its packets."""
        n = C.c_int(0)
        self._check(self._lib.ofdm_rx_csi(self._h, 0, 0, None, None, None, None, C.byref(n)))
        count = max(n.value - int(first), 0) if count is None else int(count)
        occ = int(self.cfg.occupied_tones)
        out = {"eq": np.zeros((count, occ), np.complex64)}
        for k in ("pre_power", "err", "ref"):
            out[k] = np.zeros((count, occ), np.float32)
        if count:
            self._check(self._lib.ofdm_rx_csi(self._h, int(first), count, _ptr(out["eq"]), _ptr(out["pre_power"]),
                                              _ptr(out["err"]), _ptr(out["ref"]), C.byref(n)))
        return out

    def rx_csi_summary(self, crc_ok_only=True):
        """Per-carrier float64 sums over the last call's packets (the CRC-ok ones only by default), reduced on the
        device in a fixed order: ``npkt``, ``pre_power``, ``err``, ``ref``, ``inv_gain`` (sum |1/eq|^2 over the finite
        non-zero eq) and ``ninv`` (their count, uint32).  csi.carrier_report turns it into per-carrier dB figures."""
        occ = int(self.cfg.occupied_tones)
        out = {k: np.zeros(occ, np.float64) for k in ("pre_power", "err", "ref", "inv_gain")}
        out["ninv"] = np.zeros(occ, np.uint32)
        npk = C.c_uint32(0)
        self._check(self._lib.ofdm_rx_csi_summary(self._h, 1 if crc_ok_only else 0, C.byref(npk), _ptr(out["pre_power"]),
                                                  _ptr(out["err"]), _ptr(out["ref"]), _ptr(out["inv_gain"]),
                                                  _ptr(out["ninv"])))
        out["npkt"] = int(npk.value)
        return out

    def rx_submit_device(self, iq_ptr, nsamples):
        """Queue the receiver's input stage for this buffer and return at once (ofdm_rx_submit): a tx_device(...,
        wait=False) issued next is held back only until that stage has read the buffer, and runs beside the
        rx_device() call that follows with the same arguments."""
        assert self.device_ptrs
        self._check(self._lib.ofdm_rx_submit(self._h, C.c_void_p(iq_ptr), int(nsamples)))

    def rx_device(self, iq_ptr, nsamples, payload_ptr, payload_cap, max_pkts):
        """Device mode.  Returns (npkt, off, len, ok) with NumPy metadata arrays."""
        assert self.device_ptrs
        off = np.zeros(max_pkts + 1, np.uint64)
        ln = np.zeros(max(max_pkts, 1), np.uint32)
        ok = np.zeros(max(max_pkts, 1), np.uint8)
        npk = C.c_int(0)
        st = _abi.ofdm_stats()
        rc = self._lib.ofdm_rx(self._h, C.c_void_p(iq_ptr), int(nsamples), C.c_void_p(payload_ptr), int(payload_cap),
                               off.ctypes.data_as(C.POINTER(C.c_uint64)), ln.ctypes.data_as(C.POINTER(C.c_uint32)),
                               ok.ctypes.data_as(C.POINTER(C.c_uint8)), int(max_pkts), C.byref(npk), C.byref(st))
        self.last_stats = st.as_dict()
        self._check(rc)
        n = npk.value
        return n, off[:n + 1], ln[:n], ok[:n]

    # -- the ten wideband stream stages: one body per kind of call, the stage's name picks the ofdm_* symbols --------
    def _stage_set(self, name, maker, cfg, kw):
        """ofdm_set_<name>: ``cfg`` or, from keywords, what ``maker`` ("module.function" of this package) builds."""
        if cfg is None and kw:
            mod, fn = maker.split(".")
            cfg = getattr(importlib.import_module("." + mod, __package__), fn)(**kw)
        self._check(getattr(self._lib, "ofdm_set_" + name)(self._h, C.byref(cfg) if cfg is not None else None))
        setattr(self, name + "_cfg", cfg)

    def _stage_reset(self, name, first):
        self._check(getattr(self._lib, "ofdm_%s_reset" % name)(self._h, int(first)))

    def _stage_count(self, name, nin):
        n = C.c_uint64(0)
        self._check(getattr(self._lib, "ofdm_%s_count" % name)(self._h, int(nin), C.byref(n)))
        return n.value

    def _stage_taps(self, name, *link):
        fn = getattr(self._lib, "ofdm_%s_taps" % name)
        n = C.c_int(0)
        self._check(fn(self._h, *(link + (None, 0, C.byref(n)))))
        out = np.zeros(n.value, np.complex64)
        self._check(fn(self._h, *(link + (_ptr(out), n.value, C.byref(n)))))
        return out

    def _stage_last_ms(self, name):
        ms = C.c_double(0)
        self._check(getattr(self._lib, "ofdm_%s_last_ms" % name)(self._h, C.byref(ms)))
        return ms.value

    def _stage_call(self, name, *args):
        """ofdm_<name>(handle, args..., &nout) -> nout"""
        n = C.c_uint64(0)
        self._check(getattr(self._lib, "ofdm_" + name)(self._h, *(args + (C.byref(n),))))
        return n.value

    def _stage_device(self, name, *args):
        assert self.device_ptrs
        return self._stage_call(name, *args)

    def _rx_stage(self, name, iq):
        """Host mode of a receive stage with one output run: ddc() and resamp()."""
        assert not self.device_ptrs
        iq = self._rx_samples(iq)
        out = np.zeros(max(self._stage_count(name, len(iq)), 1), np.complex64)
        return out[:self._stage_call(name, _ptr(iq) if len(iq) else None, len(iq), _ptr(out), len(out))]

    def _tx_stage(self, name, iq, add, count, add_size):
        """Host mode of a transmit stage, duc() and tx_resamp(): ``count`` gives the outputs of len(iq) inputs."""
        assert not self.device_ptrs
        cfg = getattr(self, name + "_cfg")
        if cfg is None:
            raise ValueError("%s() without set_%s()" % (name, name))
        if np.asarray(iq).dtype == np.int16:
            raise ValueError("%s() takes complex64 samples (its 16-bit side is the output)" % name)
        iq = np.ascontiguousarray(iq, np.complex64).reshape(-1)
        no = count(len(iq))
        if add is not None:
            add = np.ascontiguousarray(add, np.complex64).reshape(-1)
            if len(add) != no:
                raise ValueError("add must hold %s samples" % add_size)
        sc16 = cfg.out_format == _abi.OFDM_IQ_SC16
        out = np.zeros((max(no, 1), 2), np.int16) if sc16 else np.zeros(max(no, 1), np.complex64)
        return out[:self._stage_call(name, _ptr(iq) if len(iq) else None, len(iq),
                                     _ptr(add) if add is not None and no else None, _ptr(out), len(out))]

    def _tx_bank_stage(self, name, x, add, rows, factor, shape, add_size):
        """Host mode of a transmit bank, pfb_synth(), duc_bank() and tx_resamp_bank(): ``x`` is complex64 of shape
        (rows, nin) and gives nin * factor outputs (``factor`` a field of the configuration) or factor(nin) of them
        (a callable: the stage's count); ``shape`` and ``add_size`` name the two in the error messages."""
        assert not self.device_ptrs
        cfg = getattr(self, name + "_cfg")
        if cfg is None:
            raise ValueError("%s() without set_%s()" % (name, name))
        if np.asarray(x).dtype == np.int16:
            raise ValueError("%s() takes complex64 samples (its 16-bit side is the output)" % name)
        x = np.ascontiguousarray(x, np.complex64)
        K = int(getattr(cfg, rows))
        if x.ndim == 1 and K == 1:
            x = x.reshape(1, -1)
        if x.ndim != 2 or x.shape[0] != K:
            raise ValueError("%s() takes complex64 of shape %s" % (name, shape))
        nin = x.shape[1]
        no = factor(nin) if callable(factor) else nin * int(getattr(cfg, factor))
        if add is not None:
            add = np.ascontiguousarray(add, np.complex64).reshape(-1)
            if len(add) != no:
                raise ValueError("add must hold %s samples" % add_size)
        sc16 = cfg.out_format == _abi.OFDM_IQ_SC16
        out = np.zeros((max(no, 1), 2), np.int16) if sc16 else np.zeros(max(no, 1), np.complex64)
        return out[:self._stage_call(name, _ptr(x) if nin else None, nin, nin,
                                     _ptr(add) if add is not None and no else None, _ptr(out), len(out))]

    # -- wideband front end (tune and decimate ahead of rx) ---------------------------------
    def set_ddc(self, cfg=None, **kw):
        """Configure the front end (usrp2.source_32fc.set_decim + set_center_freq; gr.freq_xlating_fir_filter_ccf):
        an ``ofdm_ddc_cfg`` (ddc.ddc_cfg) or its keywords (decimation=, center_freq=, taps= / occupied_fraction=).
        ``set_ddc(None)`` with no keywords removes it.  Resets the stream state."""
        self._stage_set("ddc", "ddc.ddc_cfg", cfg, kw)

    def ddc_reset(self, first_sample_index=0):
        """Start a new wideband stream whose first sample has this absolute index; the filter history is zero."""
        self._stage_reset("ddc", first_sample_index)

    def ddc_count(self, nin):
        """Outputs the next ddc() call of ``nin`` samples produces, from the current stream state."""
        return self._stage_count("ddc", nin)

    def ddc(self, iq):
        """Host mode: the next samples of the wideband stream (in the receive IQ format) -> the narrowband complex64
        samples they complete (possibly none).  Stateful: any segmentation of a stream gives the same bits."""
        return self._rx_stage("ddc", iq)

    def ddc_device(self, iq_ptr, nin, out_ptr, out_cap):
        """Device mode: both buffers are device pointers; ``out_ptr`` can go straight to rx_device / rx_submit_device
        (same stream).  Returns the number of outputs written."""
        return self._stage_device("ddc", C.c_void_p(iq_ptr), int(nin), C.c_void_p(out_ptr), int(out_cap))

    def ddc_taps(self):
        """The band-pass table c[k] the kernel multiplies with (complex64)."""
        return self._stage_taps("ddc")

    def ddc_last_ms(self):
        """HIP-event time of k_ddc in the last ddc() / ddc_device() (needs prof_enable())."""
        return self._stage_last_ms("ddc")

    # -- rational-rate front end (tune and resample by L / M ahead of rx) ----------------------
    def set_resamp(self, cfg=None, **kw):
        """Configure the resampler (blks2.rational_resampler_ccf behind a tuner): an ``ofdm_resamp_cfg``
        (resample.resamp_cfg) or its keywords (interpolation=, decimation=, center_freq=, taps= / occupied_fraction=).
        ``set_resamp(None)`` with no keywords removes it.  Resets the stream state; the DDC and the bank keep theirs."""
        self._stage_set("resamp", "resample.resamp_cfg", cfg, kw)

    def resamp_reset(self, first_sample_index=0):
        """Start a new wideband stream whose first sample has this absolute index; the filter history is zero."""
        self._stage_reset("resamp", first_sample_index)

    def resamp_count(self, nin):
        """Outputs the next resamp() call of ``nin`` samples produces, from the current stream state."""
        return self._stage_count("resamp", nin)

    def resamp(self, iq):
        """Host mode: the next samples of the wideband stream (in the receive IQ format) -> the complex64 samples at
        L / M times their rate that they complete (possibly none).  Stateful: any segmentation gives the same bits."""
        return self._rx_stage("resamp", iq)

    def resamp_device(self, iq_ptr, nin, out_ptr, out_cap):
        """Device mode: both buffers are device pointers; ``out_ptr`` can go straight to rx_device / rx_submit_device
        (same stream).  Returns the number of outputs written."""
        return self._stage_device("resamp", C.c_void_p(iq_ptr), int(nin), C.c_void_p(out_ptr), int(out_cap))

    def resamp_taps(self):
        """The band-pass table c[k] the kernel multiplies with (complex64)."""
        return self._stage_taps("resamp")

    def resamp_last_ms(self):
        """HIP-event time of k_resamp in the last resamp() / resamp_device() (needs prof_enable())."""
        return self._stage_last_ms("resamp")

    # -- resampler bank: every link of a capture at a rational rate in one pass ----------------
    def set_resamp_bank(self, cfg=None, **kw):
        """Configure the bank: an ``ofdm_resamp_bank_cfg`` (resample.bank_cfg) or its keywords (interpolation=,
        decimation=, center_freqs=, taps= / occupied_fraction=).  ``set_resamp_bank(None)`` with no keywords removes
        it.  Resets the bank's stream state; the single resampler (set_resamp) is a separate stage and keeps its own."""
        self._stage_set("resamp_bank", "resample.bank_cfg", cfg, kw)

    def resamp_bank_reset(self, first_sample_index=0):
        """Start a new wideband stream whose first sample has this absolute index; the filter history is zero."""
        self._stage_reset("resamp_bank", first_sample_index)

    def resamp_bank_count(self, nin):
        """Outputs PER LINK the next resamp_bank() call of ``nin`` samples produces, from the current stream state."""
        return self._stage_count("resamp_bank", nin)

    def resamp_bank(self, iq):
        """Host mode: the next samples of the wideband stream (in the receive IQ format) -> complex64 of shape
        (K, nout): row i is what resamp() gives for link i's frequency.  Stateful like resamp()."""
        assert not self.device_ptrs
        if self.resamp_bank_cfg is None:
            raise ValueError("resamp_bank() without set_resamp_bank()")
        iq = self._rx_samples(iq)
        K = int(self.resamp_bank_cfg.nlinks)
        cap = max(self.resamp_bank_count(len(iq)), 1)
        out = np.zeros((K, cap), np.complex64)
        return out[:, :self._stage_call("resamp_bank", _ptr(iq) if len(iq) else None, len(iq), _ptr(out), cap, cap)]

    def resamp_bank_device(self, iq_ptr, nin, out_ptr, link_stride, out_cap):
        """Device mode: both buffers are device pointers; link i's run begins ``link_stride`` samples after link
        i - 1's and can go straight to rx_device / rx_submit_device.  Returns the number of outputs per link."""
        return self._stage_device("resamp_bank", C.c_void_p(iq_ptr), int(nin), C.c_void_p(out_ptr), int(link_stride),
                                  int(out_cap))

    def resamp_bank_taps(self, link):
        """The band-pass table of one link as the kernel multiplies with it (complex64)."""
        return self._stage_taps("resamp_bank", int(link))

    def resamp_bank_last_ms(self):
        """HIP-event time of k_resamp_bank in the last resamp_bank() / resamp_bank_device() (needs prof_enable())."""
        return self._stage_last_ms("resamp_bank")

    # -- DDC bank: every link of a wideband capture in one pass ------------------------------
    def set_ddc_bank(self, cfg=None, **kw):
        """Configure the bank: an ``ofdm_ddc_bank_cfg`` (ddc.bank_cfg) or its keywords (decimation=, center_freqs=,
        taps= / occupied_fraction=).  ``set_ddc_bank(None)`` with no keywords removes it.  Resets the bank's stream
        state; the single front end (set_ddc) is a separate stage and keeps its own."""
        self._stage_set("ddc_bank", "ddc.bank_cfg", cfg, kw)

    def ddc_bank_reset(self, first_sample_index=0):
        """Start a new wideband stream whose first sample has this absolute index; the filter history is zero."""
        self._stage_reset("ddc_bank", first_sample_index)

    def ddc_bank_count(self, nin):
        """Outputs PER LINK the next ddc_bank() call of ``nin`` samples produces, from the current stream state."""
        return self._stage_count("ddc_bank", nin)

    def ddc_bank(self, iq):
        """Host mode: the next samples of the wideband stream (in the receive IQ format) -> complex64 of shape
        (K, nout): row i is what ddc() gives for link i's frequency.  Stateful like ddc()."""
        assert not self.device_ptrs
        if self.ddc_bank_cfg is None:
            raise ValueError("ddc_bank() without set_ddc_bank()")
        iq = self._rx_samples(iq)
        K = int(self.ddc_bank_cfg.nlinks)
        cap = max(self.ddc_bank_count(len(iq)), 1)
        out = np.zeros((K, cap), np.complex64)
        return out[:, :self._stage_call("ddc_bank", _ptr(iq) if len(iq) else None, len(iq), _ptr(out), cap, cap)]

    def ddc_bank_device(self, iq_ptr, nin, out_ptr, link_stride, out_cap):
        """Device mode: both buffers are device pointers; link i's run begins ``link_stride`` samples after link
        i - 1's and can go straight to rx_device / rx_submit_device.  Returns the number of outputs per link."""
        return self._stage_device("ddc_bank", C.c_void_p(iq_ptr), int(nin), C.c_void_p(out_ptr), int(link_stride),
                                  int(out_cap))

    def ddc_bank_taps(self, link):
        """The band-pass table of one link as the kernel multiplies with it (complex64)."""
        return self._stage_taps("ddc_bank", int(link))

    def ddc_bank_last_ms(self):
        """HIP-event time of k_ddc_bank in the last ddc_bank() / ddc_bank_device() (needs prof_enable())."""
        return self._stage_last_ms("ddc_bank")

    # -- polyphase-FFT channeliser: every link of a capture whose links sit on the k/M grid ------------
    def set_pfb(self, cfg=None, **kw):
        """Configure the channeliser: an ``ofdm_pfb_cfg`` (pfb.pfb_cfg) or its keywords (nchannels=, channels=,
        taps= / occupied_fraction=).  ``set_pfb(None)`` with no keywords removes it.  Resets the channeliser's stream
        state; every other stage keeps its own."""
        self._stage_set("pfb", "pfb.pfb_cfg", cfg, kw)

    def pfb_reset(self, first_sample_index=0):
        """Start a new wideband stream whose first sample has this absolute index; the filter history is zero."""
        self._stage_reset("pfb", first_sample_index)

    def pfb_count(self, nin):
        """Outputs PER CHANNEL the next pfb() call of ``nin`` samples produces, from the current stream state."""
        return self._stage_count("pfb", nin)

    def pfb(self, iq):
        """Host mode: the next samples of the wideband stream (in the receive IQ format) -> complex64 of shape
        (K, nout): row i is selected channel i, the link at channels[i] / M decimated by M.  Stateful like ddc()."""
        assert not self.device_ptrs
        if self.pfb_cfg is None:
            raise ValueError("pfb() without set_pfb()")
        iq = self._rx_samples(iq)
        K = int(self.pfb_cfg.nsel)
        cap = max(self.pfb_count(len(iq)), 1)
        out = np.zeros((K, cap), np.complex64)
        return out[:, :self._stage_call("pfb", _ptr(iq) if len(iq) else None, len(iq), _ptr(out), cap, cap)]

    def pfb_device(self, iq_ptr, nin, out_ptr, chan_stride, out_cap):
        """Device mode: both buffers are device pointers; selected channel i's run begins ``chan_stride`` samples
        after channel i - 1's and can go straight to rx_device / rx_submit_device.  Returns the outputs per channel."""
        return self._stage_device("pfb", C.c_void_p(iq_ptr), int(nin), C.c_void_p(out_ptr), int(chan_stride),
                                  int(out_cap))

    def pfb_last_ms(self):
        """HIP-event time of k_pfb in the last pfb() / pfb_device() (needs prof_enable())."""
        return self._stage_last_ms("pfb")

    # -- polyphase-FFT synthesis bank: every link of a band on the c/M grid in one pass over it ------------
    def set_pfb_synth(self, cfg=None, **kw):
        """Configure the synthesis bank: an ``ofdm_pfb_synth_cfg`` (pfb.synth_cfg) or its keywords (nchannels=,
        channels=, taps= / occupied_fraction=, out_format=, out_scale=).  ``set_pfb_synth(None)`` with no keywords
        removes it.  Resets the bank's stream state; every other stage keeps its own."""
        self._stage_set("pfb_synth", "pfb.synth_cfg", cfg, kw)

    def pfb_synth_reset(self, first=0):
        """Start new narrowband streams whose first samples have this absolute index (outputs begin at M * first);
        the filter history is zero."""
        self._stage_reset("pfb_synth", first)

    def pfb_synth(self, x, add=None):
        """Host mode: the next samples of the K narrowband streams, complex64 of shape (K, nin), row i on channel
        channels[i] -> nin * M samples of the band (complex64, or int16 of shape (n, 2) with out_format "sc16"), added
        onto the complex64 band ``add`` where one is given.  Stateful: any segmentation gives the same bits."""
        return self._tx_bank_stage("pfb_synth", x, add, "nsel", "nchannels", "(nsel, nin)", "nin * nchannels")

    def pfb_synth_device(self, iq_ptr, chan_stride, nin, out_ptr, out_cap, add_ptr=None):
        """Device mode: all buffers are device pointers; selected channel i's ``nin`` inputs begin ``chan_stride``
        samples after channel i - 1's (what pfb_device writes; what tx_device(wait=False) is filling, same handle),
        ``add_ptr`` may be ``out_ptr`` itself for complex64 output.  Returns the number of outputs written."""
        return self._stage_device("pfb_synth", C.c_void_p(iq_ptr), int(chan_stride), int(nin),
                                  C.c_void_p(add_ptr) if add_ptr else None, C.c_void_p(out_ptr), int(out_cap))

    def pfb_synth_last_ms(self):
        """HIP-event time of k_pfb_synth in the last pfb_synth() / pfb_synth_device() (needs prof_enable())."""
        return self._stage_last_ms("pfb_synth")

    # -- wideband transmit (interpolate and translate behind tx) -------------------------------
    def set_duc(self, cfg=None, **kw):
        """Configure the transmit stage (sink.set_interp + set_center_freq): an ``ofdm_duc_cfg`` (duc.duc_cfg) or its
        keywords (interpolation=, center_freq=, taps= / occupied_fraction=, out_format=, out_scale=).
        ``set_duc(None)`` with no keywords removes it.  Resets the stream state."""
        self._stage_set("duc", "duc.duc_cfg", cfg, kw)

    def duc_reset(self, first=0):
        """Start a new narrowband stream whose first sample has this absolute index (outputs begin at L * first); the
        filter history is zero."""
        self._stage_reset("duc", first)

    def duc(self, iq, add=None):
        """Host mode: the next complex64 samples of the narrowband stream -> len(iq) * L wideband samples (complex64,
        or int16 of shape (n, 2) with out_format "sc16"), added onto the complex64 band ``add`` where one is given.
        Stateful: any segmentation of a stream gives the same bits."""
        return self._tx_stage("duc", iq, add, lambda n: n * int(self.duc_cfg.interpolation), "len(iq) * interpolation")

    def duc_device(self, iq_ptr, nin, out_ptr, out_cap, add_ptr=None):
        """Device mode: all buffers are device pointers; ``iq_ptr`` can be what tx_device(wait=False) is filling (same
        handle), ``add_ptr`` may be ``out_ptr`` itself for complex64 output.  Returns the number of outputs written."""
        return self._stage_device("duc", C.c_void_p(iq_ptr), int(nin), C.c_void_p(add_ptr) if add_ptr else None,
                                  C.c_void_p(out_ptr), int(out_cap))

    def duc_last_ms(self):
        """HIP-event time of k_duc in the last duc() / duc_device() (needs prof_enable())."""
        return self._stage_last_ms("duc")

    # -- DUC bank: every link of a band at arbitrary centre frequencies in one pass over it ------------
    def set_duc_bank(self, cfg=None, **kw):
        """Configure the bank: an ``ofdm_duc_bank_cfg`` (duc.bank_cfg) or its keywords (interpolation=, center_freqs=,
        taps= / occupied_fraction=, out_format=, out_scale=).  ``set_duc_bank(None)`` with no keywords removes it.
        Resets the bank's stream state; the single stage (set_duc) is a separate one and keeps its own."""
        self._stage_set("duc_bank", "duc.bank_cfg", cfg, kw)

    def duc_bank_reset(self, first=0):
        """Start new narrowband streams whose first samples have this absolute index (outputs begin at L * first);
        the filter history is zero."""
        self._stage_reset("duc_bank", first)

    def duc_bank(self, x, add=None):
        """Host mode: the next samples of the K narrowband streams, complex64 of shape (K, nin), row i at
        center_freqs[i] -> nin * L samples of the band (complex64, or int16 of shape (n, 2) with out_format "sc16"),
        added onto the complex64 band ``add`` where one is given.  Stateful: any segmentation gives the same bits."""
        return self._tx_bank_stage("duc_bank", x, add, "nlinks", "interpolation", "(nlinks, nin)", "nin * interpolation")

    def duc_bank_device(self, iq_ptr, link_stride, nin, out_ptr, out_cap, add_ptr=None):
        """Device mode: all buffers are device pointers; link i's ``nin`` inputs begin ``link_stride`` samples after
        link i - 1's (what tx_device(wait=False) is filling, same handle), ``add_ptr`` may be ``out_ptr`` itself for
        complex64 output.  Returns the number of outputs written."""
        return self._stage_device("duc_bank", C.c_void_p(iq_ptr), int(link_stride), int(nin),
                                  C.c_void_p(add_ptr) if add_ptr else None, C.c_void_p(out_ptr), int(out_cap))

    def duc_bank_taps(self, link):
        """The band-pass table of one link as the kernel multiplies with it (complex64)."""
        return self._stage_taps("duc_bank", int(link))

    def duc_bank_last_ms(self):
        """HIP-event time of k_duc_bank in the last duc_bank() / duc_bank_device() (needs prof_enable())."""
        return self._stage_last_ms("duc_bank")

    # -- rational-rate transmit (resample by L / M and translate behind tx) ---------------------
    def set_tx_resamp(self, cfg=None, **kw):
        """Configure the rational-rate transmit stage (blks2.rational_resampler_ccf + set_center_freq): an
        ``ofdm_tx_resamp_cfg`` (tx_resample.tx_resamp_cfg) or its keywords (interpolation=, decimation=, center_freq=,
        taps= / occupied_fraction=, out_format=, out_scale=).  ``set_tx_resamp(None)`` with no keywords removes it.
        Resets the stream state; the DUC keeps its own."""
        self._stage_set("tx_resamp", "tx_resample.tx_resamp_cfg", cfg, kw)

    def tx_resamp_reset(self, first=0):
        """Start a new narrowband stream whose first sample has this absolute index; the filter history is zero."""
        self._stage_reset("tx_resamp", first)

    def tx_resamp_count(self, nin):
        """Outputs the next tx_resamp() call of ``nin`` samples produces, from the current stream state."""
        return self._stage_count("tx_resamp", nin)

    def tx_resamp(self, iq, add=None):
        """Host mode: the next complex64 samples of the narrowband stream -> the wideband samples at L / M times their
        rate that they complete (possibly none; complex64, or int16 of shape (n, 2) with out_format "sc16"), added
        onto the complex64 band ``add`` where one is given.  Stateful: any segmentation gives the same bits."""
        return self._tx_stage("tx_resamp", iq, add, self.tx_resamp_count, "tx_resamp_count(len(iq))")

    def tx_resamp_device(self, iq_ptr, nin, out_ptr, out_cap, add_ptr=None):
        """Device mode: all buffers are device pointers; ``iq_ptr`` can be what tx_device(wait=False) is filling (same
        handle), ``add_ptr`` may be ``out_ptr`` itself for complex64 output.  Returns the number of outputs written."""
        return self._stage_device("tx_resamp", C.c_void_p(iq_ptr), int(nin), C.c_void_p(add_ptr) if add_ptr else None,
                                  C.c_void_p(out_ptr), int(out_cap))

    def tx_resamp_last_ms(self):
        """HIP-event time of k_tx_resamp in the last tx_resamp() / tx_resamp_device() (needs prof_enable())."""
        return self._stage_last_ms("tx_resamp")

    # -- transmit resampler bank: every link of a band at a rational rate in one pass over it ------------
    def set_tx_resamp_bank(self, cfg=None, **kw):
        """Configure the bank: an ``ofdm_tx_resamp_bank_cfg`` (tx_resample.bank_cfg) or its keywords (interpolation=,
        decimation=, center_freqs=, taps= / occupied_fraction=, out_format=, out_scale=).
        ``set_tx_resamp_bank(None)`` with no keywords removes it.  Resets the bank's stream state; the single stage
        (set_tx_resamp) is a separate one and keeps its own."""
        self._stage_set("tx_resamp_bank", "tx_resample.bank_cfg", cfg, kw)

    def tx_resamp_bank_reset(self, first=0):
        """Start new narrowband streams whose first samples have this absolute index; the filter history is zero."""
        self._stage_reset("tx_resamp_bank", first)

    def tx_resamp_bank_count(self, nin):
        """Outputs the next tx_resamp_bank() call of ``nin`` samples per link produces, from the current stream state."""
        return self._stage_count("tx_resamp_bank", nin)

    def tx_resamp_bank(self, x, add=None):
        """Host mode: the next samples of the K narrowband streams, complex64 of shape (K, nin), row i at
        center_freqs[i] -> the samples of the band at L / M times their rate that they complete (possibly none;
        complex64, or int16 of shape (n, 2) with out_format "sc16"), added onto the complex64 band ``add`` where one
        is given.  Stateful: any segmentation gives the same bits."""
        return self._tx_bank_stage("tx_resamp_bank", x, add, "nlinks", self.tx_resamp_bank_count, "(nlinks, nin)",
                                   "tx_resamp_bank_count(nin)")

    def tx_resamp_bank_device(self, iq_ptr, link_stride, nin, out_ptr, out_cap, add_ptr=None):
        """Device mode: all buffers are device pointers; link i's ``nin`` inputs begin ``link_stride`` samples after
        link i - 1's (what tx_device(wait=False) is filling, same handle), ``add_ptr`` may be ``out_ptr`` itself for
        complex64 output.  Returns the number of outputs written."""
        return self._stage_device("tx_resamp_bank", C.c_void_p(iq_ptr), int(link_stride), int(nin),
                                  C.c_void_p(add_ptr) if add_ptr else None, C.c_void_p(out_ptr), int(out_cap))

    def tx_resamp_bank_taps(self, link):
        """The band-pass table of one link as the kernel multiplies with it (complex64)."""
        return self._stage_taps("tx_resamp_bank", int(link))

    def tx_resamp_bank_last_ms(self):
        """HIP-event time of k_tx_resamp_bank in the last tx_resamp_bank() / tx_resamp_bank_device() (needs
        prof_enable())."""
        return self._stage_last_ms("tx_resamp_bank")

    # -- chunked streams --------------------------------------------------------------
    # -- propagation channel (multipath, Doppler, tones, carrier offset and noise between tx and rx) ---------------
    def set_multipath(self, cfg=None, **kw):
        """Configure the propagation channel stage: an ``ofdm_multipath_cfg`` (multipath.multipath_cfg) or its keywords
        (paths=, tones=, sigma=, cfo=, seed=, stream_id=, out_format=, out_scale=).  ``set_multipath(None)`` with no
        keywords removes it.  Resets the stream state."""
        self._stage_set("multipath", "multipath.multipath_cfg", cfg, kw)

    def multipath_reset(self, first=0):
        """Start a new stream whose first sample has this absolute index (at most 2^53); the echo history is zero."""
        self._stage_reset("multipath", first)

    def multipath(self, iq, add=None):
        """Host mode: the next complex64 samples of the stream -> as many received samples (complex64, or int16 of
        shape (n, 2) with out_format "sc16"), added onto the complex64 band ``add`` where one is given.  Stateful: any
        segmentation of a stream gives the same bits."""
        return self._tx_stage("multipath", iq, add, lambda n: n, "len(iq)")

    def multipath_device(self, iq_ptr, nin, out_ptr, out_cap, add_ptr=None):
        """Device mode: all buffers are device pointers; ``iq_ptr`` can be what tx_device(wait=False) is filling (same
        handle) and must not overlap ``out_ptr``; ``add_ptr`` may be ``out_ptr`` itself for complex64 output.  Returns
        the number of outputs written."""
        return self._stage_device("multipath", C.c_void_p(iq_ptr), int(nin), C.c_void_p(add_ptr) if add_ptr else None,
                                  C.c_void_p(out_ptr), int(out_cap))

    def multipath_last_ms(self):
        """HIP-event time of k_multipath in the last multipath() / multipath_device() (needs prof_enable())."""
        return self._stage_last_ms("multipath")

    # -- transmit crest-factor reduction (peak windowing, the last stage in front of a converter) -------------------
    def set_cfr(self, cfg=None, **kw):
        """Configure the crest-factor reduction stage: an ``ofdm_cfr_cfg`` (cfr.cfr_cfg) or its keywords (threshold=,
        window=, out_format=, out_scale=).  ``set_cfr(None)`` with no keywords removes it.  Resets the stream state
        and the statistics."""
        self._stage_set("cfr", "cfr.cfr_cfg", cfg, kw)

    def cfr_reset(self):
        """Start a new stream: the history and the statistics are zero."""
        self._check(self._lib.ofdm_cfr_reset(self._h))

    def cfr(self, iq):
        """Host mode: the next complex64 samples of the stream -> as many samples (complex64, or int16 of shape (n, 2)
        with out_format "sc16"), delayed by the window's half-width, every peak above the threshold pulled down to it.
        Stateful: any segmentation of a stream gives the same bits."""
        assert not self.device_ptrs
        if self.cfr_cfg is None:
            raise ValueError("cfr() without set_cfr()")
        if np.asarray(iq).dtype == np.int16:
            raise ValueError("cfr() takes complex64 samples (its 16-bit side is the output)")
        iq = np.ascontiguousarray(iq, np.complex64).reshape(-1)
        n = len(iq)
        sc16 = self.cfr_cfg.out_format == _abi.OFDM_IQ_SC16
        out = np.zeros((max(n, 1), 2), np.int16) if sc16 else np.zeros(max(n, 1), np.complex64)
        return out[:self._stage_call("cfr", _ptr(iq) if n else None, n, _ptr(out), len(out))]

    def cfr_device(self, iq_ptr, nin, out_ptr, out_cap):
        """Device mode: both buffers are device pointers and must not overlap.  Returns the number of outputs written."""
        return self._stage_device("cfr", C.c_void_p(iq_ptr), int(nin), C.c_void_p(out_ptr), int(out_cap))

    def cfr_stats(self):
        """The statistics since set_cfr() / cfr_reset() as a dict: n, n_over, n_touched, peak_in, peak_out, sum_in,
        sum_out, sum_err (ofdm_cfr_stats; cfr.report turns them into PAPR and EVM figures)."""
        st = _abi.ofdm_cfr_stats()
        self._check(self._lib.ofdm_cfr_stats(self._h, C.byref(st)))
        return st.as_dict()

    def cfr_last_ms(self):
        """HIP-event time of k_cfr and its reduction in the last cfr() / cfr_device() (needs prof_enable())."""
        return self._stage_last_ms("cfr")

    # -- memory polynomial: the predistorter (slot dpd, transmit side) and the amplifier model (slot pa, air side) -----
    # one implementation, two instances (csrc/mempoly.h): ``name`` is "dpd" or "pa"
    def _mempoly_set(self, name, cfg, kw):
        if cfg is None and kw:
            cfg = importlib.import_module(".dpd", __package__).mempoly_cfg(**kw)
        self._check(self._lib.ofdm_set_mempoly(self._h, _MEMPOLY_SLOT[name], C.byref(cfg) if cfg is not None else None))
        setattr(self, name + "_cfg", cfg)

    def _mempoly(self, name, iq):
        assert not self.device_ptrs
        cfg = getattr(self, name + "_cfg")
        if cfg is None:
            raise ValueError("%s() without set_%s()" % (name, name))
        if np.asarray(iq).dtype == np.int16:
            raise ValueError("%s() takes complex64 samples (its 16-bit side is the output)" % name)
        iq = np.ascontiguousarray(iq, np.complex64).reshape(-1)
        n = len(iq)
        sc16 = cfg.out_format == _abi.OFDM_IQ_SC16
        out = np.zeros((max(n, 1), 2), np.int16) if sc16 else np.zeros(max(n, 1), np.complex64)
        return out[:self._stage_call("mempoly", _MEMPOLY_SLOT[name], _ptr(iq) if n else None, n, _ptr(out), len(out))]

    def _mempoly_stats(self, name):
        st = _abi.ofdm_mempoly_stats()
        self._check(self._lib.ofdm_mempoly_stats(self._h, _MEMPOLY_SLOT[name], C.byref(st)))
        return st.as_dict()

    def _mempoly_last_ms(self, name):
        ms = C.c_double(0)
        self._check(self._lib.ofdm_mempoly_last_ms(self._h, _MEMPOLY_SLOT[name], C.byref(ms)))
        return ms.value

    def set_dpd(self, cfg=None, **kw):
        """Configure the predistorter: an ``ofdm_mempoly_cfg`` (dpd.mempoly_cfg) or its keywords (coef=, out_format=,
        out_scale=, limit=).  ``set_dpd(None)`` with no keywords removes it.  Resets the slot's stream state and
        statistics; the amplifier model (set_pa) is a separate instance and keeps its own."""
        self._mempoly_set("dpd", cfg, kw)

    def dpd_reset(self):
        """Start a new stream: the history and the statistics are zero."""
        self._check(self._lib.ofdm_mempoly_reset(self._h, _abi.OFDM_MEMPOLY_DPD))

    def dpd(self, iq):
        """Host mode: the next complex64 samples of the stream -> as many predistorted samples (complex64, or int16 of
        shape (n, 2) with out_format "sc16"), no delay.  Stateful: any segmentation of a stream gives the same bits."""
        return self._mempoly("dpd", iq)

    def dpd_device(self, iq_ptr, nin, out_ptr, out_cap):
        """Device mode: both buffers are device pointers and must not overlap.  Returns the number of outputs written."""
        return self._stage_device("mempoly", _abi.OFDM_MEMPOLY_DPD, C.c_void_p(iq_ptr), int(nin), C.c_void_p(out_ptr), int(out_cap))

    def dpd_stats(self):
        """The statistics since set_dpd() / dpd_reset() as a dict: n, n_over, peak_in, peak_out, sum_in, sum_out
        (ofdm_mempoly_stats; dpd.report turns them into gain, peak expansion and the share over the limit)."""
        return self._mempoly_stats("dpd")

    def dpd_last_ms(self):
        """HIP-event time of k_mempoly and its reduction in the last dpd() / dpd_device() (needs prof_enable())."""
        return self._mempoly_last_ms("dpd")

    def set_pa(self, cfg=None, **kw):
        """Configure the amplifier model, the same stage in the other slot: as set_dpd."""
        self._mempoly_set("pa", cfg, kw)

    def pa_reset(self):
        """Start a new stream: the history and the statistics are zero."""
        self._check(self._lib.ofdm_mempoly_reset(self._h, _abi.OFDM_MEMPOLY_PA))

    def pa(self, iq):
        """Host mode: the next complex64 samples of the stream -> as many samples behind the amplifier: as dpd()."""
        return self._mempoly("pa", iq)

    def pa_device(self, iq_ptr, nin, out_ptr, out_cap):
        """Device mode: as dpd_device()."""
        return self._stage_device("mempoly", _abi.OFDM_MEMPOLY_PA, C.c_void_p(iq_ptr), int(nin), C.c_void_p(out_ptr), int(out_cap))

    def pa_stats(self):
        """The statistics since set_pa() / pa_reset(): as dpd_stats()."""
        return self._mempoly_stats("pa")

    def pa_last_ms(self):
        """HIP-event time of k_mempoly and its reduction in the last pa() / pa_device() (needs prof_enable())."""
        return self._mempoly_last_ms("pa")

    # -- spectrum measurement: a Welch estimator over any stream (csrc/psd.h; figures: spectrum.py) --------------------
    def set_psd(self, cfg=None, **kw):
        """Configure the spectrum stage: an ``ofdm_psd_cfg`` (spectrum.psd_cfg) or its keywords (nfft=, hop=, window=,
        in_format=, in_scale=).  ``set_psd(None)`` with no keywords removes it.  Resets the stream state and the
        accumulators."""
        self._stage_set("psd", "spectrum.psd_cfg", cfg, kw)

    def psd_reset(self):
        """Start a new stream: nothing pending, the accumulators zero."""
        self._check(self._lib.ofdm_psd_reset(self._h))

    def psd_count(self, nin):
        """Segments the next call of ``nin`` samples would complete."""
        return self._stage_count("psd", nin)

    def _psd_samples(self, iq):
        if self.psd_cfg is None:
            raise ValueError("psd() without set_psd()")
        if self.psd_cfg.in_format == _abi.OFDM_IQ_SC16:
            return iqio.as_sc16(iq)
        if np.asarray(iq).dtype == np.int16:
            raise ValueError("int16 samples handed to a spectrum stage in fc32 mode (in_format=\"sc16\")")
        return np.ascontiguousarray(iq, np.complex64).reshape(-1)

    def psd(self, iq, rows=False):
        """Host mode: the next samples of the stream (complex64, or int16 of shape (n, 2) with in_format "sc16") into
        the estimator.  Returns the number of segments the call completed, or with ``rows=True`` their float32 power
        spectra, shape (segments, nfft), FFT order.  Stateful: any segmentation of a stream gives the same rows."""
        assert not self.device_ptrs
        iq = self._psd_samples(iq)
        n = len(iq)
        if not rows:
            return self._stage_call("psd", _ptr(iq) if n else None, n, None, 0)
        nfft = int(self.psd_cfg.nfft)
        out = np.zeros((max(self.psd_count(n), 1), nfft), np.float32)
        return out[:self._stage_call("psd", _ptr(iq) if n else None, n, _ptr(out), len(out))]

    def psd_device(self, iq_ptr, nin, rows_ptr=None, rows_cap=0):
        """Device mode: ``iq_ptr`` is a device pointer in the configured input format, ``rows_ptr`` None or a device
        buffer of ``rows_cap`` rows of nfft float32 that must not overlap the input.  Returns the segments completed."""
        return self._stage_device("psd", C.c_void_p(iq_ptr), int(nin), C.c_void_p(rows_ptr) if rows_ptr else None, int(rows_cap))

    def psd_read(self):
        """The accumulators since set_psd() / psd_reset() as a dict: ``sum`` (float64, nfft), ``peak`` (float32, nfft),
        both in FFT order, and ``nseg`` (spectrum.report turns them into density, ACLR, occupied bandwidth and mask
        margin).  In device mode the two arrays are read through the library's own staging: pass device buffers to
        psd_read_device instead."""
        if self.psd_cfg is None:
            raise ValueError("psd_read() without set_psd()")
        assert not self.device_ptrs
        nfft = int(self.psd_cfg.nfft)
        s, p, n = np.zeros(nfft, np.float64), np.zeros(nfft, np.float32), C.c_uint64(0)
        self._check(self._lib.ofdm_psd_read(self._h, _ptr(s), _ptr(p), C.byref(n)))
        return {"sum": s, "peak": p, "nseg": n.value}

    def psd_read_device(self, sum_ptr=None, peak_ptr=None):
        """Device mode: the sums (nfft float64) and maxima (nfft float32) into device buffers; returns ``nseg``."""
        assert self.device_ptrs
        n = C.c_uint64(0)
        self._check(self._lib.ofdm_psd_read(self._h, C.c_void_p(sum_ptr) if sum_ptr else None,
                                            C.c_void_p(peak_ptr) if peak_ptr else None, C.byref(n)))
        return n.value

    def psd_last_ms(self):
        """HIP-event time of k_psd and k_psd_reduce in the last psd() / psd_device() (needs prof_enable())."""
        return self._stage_last_ms("psd")

    # -- coded links: the two call shapes every codec shares (the counterpart of csrc/engine_codec.inc) ----------------
    # ``head`` is what a call takes ahead of its batch: () or (C.byref(cfg),).
    def _codec_encode(self, fn, head, in_ptr, offs, lens, out_ptr, out_cap):
        """fn(handle, *head, in, offs, lens, nblk, out, cap, block offsets) -> the nblk + 1 block offsets (uint64)."""
        coff = np.zeros(len(lens) + 1, np.uint64)
        self._check(fn(self._h, *head, in_ptr, _u64(offs), _u32(lens), len(lens), out_ptr, int(out_cap), _u64(coff)))
        return coff

    def _codec_encode_host(self, fn, head, payloads, room):
        """Host mode of an encode call: list of payloads -> list of blocks, in ``room(lens)`` bytes at the most."""
        assert not self.device_ptrs
        blob, offs, lens = pack_payloads(payloads)
        out = np.zeros(max(int(room(lens.astype(np.int64))), 1), np.uint8)
        coff = self._codec_encode(fn, head, _ptr(blob), offs, lens, _ptr(out), len(out))
        return [out[int(coff[i]):int(coff[i + 1])].tobytes() for i in range(len(payloads))]

    def _codec_decode(self, fn, head, n, out_ptr, out_cap, extra=(), tail=()):
        """fn(handle, *head, out, cap, payload offsets, ok, corrected, *extra, *tail) over n blocks: ``head`` ends with
        the batch (_batch()) where the call takes one, ``extra`` names the dtypes of the per-block outputs after
        ``corrected``, ``tail`` is what follows them.  Returns (payload offsets uint64[n + 1], ok uint8[n],
        corrected uint32[n], one array[n] per ``extra``) as host arrays."""
        poff = np.zeros(n + 1, np.uint64)
        cols = [np.zeros(max(n, 1), dt) for dt in (np.uint8, np.uint32) + tuple(extra)]
        self._check(fn(self._h, *head, out_ptr, int(out_cap), _u64(poff), *[_u32(c) if c.dtype == np.uint32 else _ptr(c) for c in cols],
                       *tail))
        return (poff,) + tuple(c[:n] for c in cols)

    @staticmethod
    def _batch(in_ptr, offs, lens, *more):
        """The batch of a decode call as it follows ``head``: (in, offs, lens, nblk) and what a codec puts behind them."""
        return (in_ptr, _u64(offs), _u32(lens), len(lens)) + more

    def _rx_batch(self, n):
        """What an rx_*_decode_soft call takes in a batch's place, behind its outputs: (max_pkts, &n)."""
        return (n, C.byref(C.c_int(0)))

    @staticmethod
    def _codec_results(out, poff, ok, *cols):
        """(ok, payload, one int per column) per block, out of what _codec_decode returned."""
        return [(bool(ok[i]), out[int(poff[i]):int(poff[i + 1])].tobytes()) + tuple(int(c[i]) for c in cols) for i in range(len(ok))]

    # -- coded links (convolutional encoder and Viterbi decoder over the payloads) ---------------------------------
    def _fec_cfg(self, fec):
        from . import fec as _fec
        cfg = _fec.as_cfg(True if fec is None else fec)
        if cfg is None:
            raise ValueError("fec=False names no code")
        return cfg

    @staticmethod
    def _fec_payload_room(cfg, lens):
        """Bytes that hold the payloads of blocks of these lengths: half a block at rate 1/2, under a whole one at the
        punctured rates."""
        total = int(np.asarray(lens).astype(np.int64).sum())
        return max(total if cfg.rate else total // 2, 1)

    def fec_encode(self, payloads, fec=None):
        """Host mode: list of payloads (0 .. 2040 bytes each) -> list of coded blocks (2 n + 10 bytes each), the
        payloads tx() then takes.  ``fec``: None / True (16 interleaver columns), a column count, a dict of
        fec.fec_cfg's keywords or an ``ofdm_fec_cfg``."""
        return self._codec_encode_host(self._lib.ofdm_fec_encode, (C.byref(self._fec_cfg(fec)),), payloads,
                                       lambda lens: 2 * lens.sum() + 10 * len(lens))   # (covers every rate)

    def fec_encode_device(self, payload_ptr, offs, lens, coded_ptr, coded_cap, fec=None):
        """Device mode: payload bytes and coded blocks are device pointers; offs / lens are NumPy host arrays.
        Returns the nblk + 1 block offsets (uint64)."""
        assert self.device_ptrs
        return self._codec_encode(self._lib.ofdm_fec_encode, (C.byref(self._fec_cfg(fec)),), C.c_void_p(payload_ptr), offs, lens,
                                  C.c_void_p(coded_ptr), coded_cap)

    def _fec_decode_host(self, fn, fec, packed, rel):
        """Host mode of the four fec decode calls: ``packed`` is pack_payloads' or _pack_values' (blob, offs, lens)."""
        assert not self.device_ptrs
        cfg = self._fec_cfg(fec)
        blob, offs, lens = packed
        out = np.zeros(self._fec_payload_room(cfg, lens), np.uint8)
        head = (C.byref(cfg),) + self._batch(_ptr(blob), offs, lens)
        if not rel:
            return self._codec_results(out, *self._codec_decode(fn, head, len(lens), _ptr(out), len(out)))
        q = np.zeros(len(out), np.uint8)
        return self._fec_rel_results(out, q, *self._codec_decode(fn, head, len(lens), _ptr(out), len(out), tail=(_ptr(q), len(q))))

    def fec_decode(self, blocks, fec=None):
        """Host mode: list of received blocks (hard bytes of any length, e.g. the payloads rx() delivered whatever
        their CRC said) -> list of (ok, payload, corrected): the decoded payload, whether its inner CRC matches, and
        the number of coded bits the decoder changed.  A length that is no block gives (False, b"", 0)."""
        return self._fec_decode_host(self._lib.ofdm_fec_decode, fec, pack_payloads(blocks), False)

    def fec_decode_soft(self, values, fec=None):
        """Host mode: list of int8 arrays, one value per transmitted bit (v > 0 means 1, 0 is an erasure, -128 reads
        as -127), 8 per coded byte -> list of (ok, payload, corrected) as fec_decode.  An array whose length is no
        multiple of 8, or no block's, gives (False, b"", 0)."""
        return self._fec_decode_host(self._lib.ofdm_fec_decode_soft, fec, _pack_values(values), False)

    def fec_decode_device(self, in_ptr, offs, lens, payload_ptr, payload_cap, fec=None, soft=False):
        """Device mode: the blocks (hard bytes, or int8 values with ``soft``: 8 per coded byte, offsets in values) and
        the payloads are device pointers; offs / lens (coded bytes) are NumPy host arrays.  Returns (payload offsets
        uint64[nblk + 1], ok uint8[nblk], corrected uint32[nblk]) as host arrays."""
        assert self.device_ptrs
        fn = self._lib.ofdm_fec_decode_soft if soft else self._lib.ofdm_fec_decode
        head = (C.byref(self._fec_cfg(fec)),) + self._batch(C.c_void_p(in_ptr), offs, lens)
        return self._codec_decode(fn, head, len(lens), C.c_void_p(payload_ptr), payload_cap)

    def fec_last_ms(self):
        """HIP-event time of k_fec_encode / k_fec_decode (k_fec_decode_rel after a ``*_rel`` call) in the last fec call
        (needs prof_enable())."""
        return self._stage_last_ms("fec")

    # -- coded links, reliabilities out (the soft-output Viterbi decoder: one reliability byte per payload byte) --------
    @staticmethod
    def _fec_rel_results(out, rel, poff, ok, corr):
        return [r + (rel[int(poff[i]):int(poff[i + 1])].copy(),) for i, r in enumerate(Engine._codec_results(out, poff, ok, corr))]

    def fec_decode_rel(self, blocks, fec=None):
        """Host mode: fec_decode() with reliabilities -> list of (ok, payload, corrected, rel): fec_decode()'s three
        fields, and ``rel`` a uint8 array of len(payload): 0 where a path as good as the decoded one disagrees in the
        byte, 255 "never erase" -- what rs_decode_rel() takes.  A length that is no block gives (False, b"", 0, [])."""
        return self._fec_decode_host(self._lib.ofdm_fec_decode_rel, fec, pack_payloads(blocks), True)

    def fec_decode_soft_rel(self, values, fec=None):
        """Host mode: fec_decode_soft() with reliabilities -> list of (ok, payload, corrected, rel) as fec_decode_rel."""
        return self._fec_decode_host(self._lib.ofdm_fec_decode_soft_rel, fec, _pack_values(values), True)

    def fec_decode_rel_device(self, in_ptr, offs, lens, payload_ptr, payload_cap, rel_ptr, rel_cap, fec=None, soft=False):
        """Device mode: fec_decode_device() with the reliabilities written to the device buffer ``rel_ptr`` at the
        payloads' offsets: (payload_ptr, rel_ptr, the returned offsets) are what rs_decode_rel_device() takes as blocks,
        reliabilities and offsets, with ``rel_offs=None``.  Returns (payload offsets, ok, corrected) as host arrays."""
        assert self.device_ptrs
        fn = self._lib.ofdm_fec_decode_soft_rel if soft else self._lib.ofdm_fec_decode_rel
        head = (C.byref(self._fec_cfg(fec)),) + self._batch(C.c_void_p(in_ptr), offs, lens)
        return self._codec_decode(fn, head, len(lens), C.c_void_p(payload_ptr), payload_cap, tail=(C.c_void_p(rel_ptr), int(rel_cap)))

    def fec_punct_last_ms(self):
        """HIP-event time of k_fec_puncture / k_fec_depuncture alone in the last fec call, which ran at a punctured
        rate (needs prof_enable())."""
        return self._stage_last_ms("fec_punct")

    # -- outer code (Reed-Solomon over the payloads, above the coded links) -------------------------------------------
    def rs_encode(self, payloads):
        """Host mode: list of payloads (0 .. 3564 bytes each) -> list of RS blocks (rs.coded_len(n) bytes each), the
        payloads fec_encode() or tx() then takes."""
        return self._codec_encode_host(self._lib.ofdm_rs_encode, (), payloads,
                                       lambda lens: (lens + 4 + 32 * ((lens + 4 + 222) // 223)).sum())

    def rs_encode_device(self, payload_ptr, offs, lens, coded_ptr, coded_cap):
        """Device mode: payload bytes and RS blocks are device pointers; offs / lens are NumPy host arrays.  Returns
        the nblk + 1 block offsets (uint64), which fec_encode_device() takes as its payload offsets."""
        assert self.device_ptrs
        return self._codec_encode(self._lib.ofdm_rs_encode, (), C.c_void_p(payload_ptr), offs, lens, C.c_void_p(coded_ptr), coded_cap)

    def rs_decode(self, blocks):
        """Host mode: list of received RS blocks (bytes of any length, e.g. what fec_decode() returned whatever its
        CRC said) -> list of (ok, payload, corrected, failed): the corrected payload, whether its CRC matches, the
        symbols changed and the codewords that could not be decoded.  A length that is no block gives
        (False, b"", 0, 0)."""
        assert not self.device_ptrs
        blob, offs, lens = pack_payloads(blocks)
        out = np.zeros(max(int(lens.astype(np.int64).sum()), 1), np.uint8)
        return self._codec_results(out, *self._codec_decode(self._lib.ofdm_rs_decode, self._batch(_ptr(blob), offs, lens), len(lens),
                                                            _ptr(out), len(out), extra=(np.uint32,)))

    def rs_decode_device(self, in_ptr, offs, lens, payload_ptr, payload_cap):
        """Device mode: the blocks and the payloads are device pointers (the blocks can be what fec_decode_device()
        wrote, with its payload offsets); offs / lens are NumPy host arrays.  Returns (payload offsets uint64[nblk + 1],
        ok uint8[nblk], corrected uint32[nblk], failed uint32[nblk]) as host arrays."""
        assert self.device_ptrs
        return self._codec_decode(self._lib.ofdm_rs_decode, self._batch(C.c_void_p(in_ptr), offs, lens), len(lens),
                                  C.c_void_p(payload_ptr), payload_cap, extra=(np.uint32,))

    def rs_last_ms(self):
        """HIP-event time of k_rs_encode / k_rs_decode in the last rs call (needs prof_enable())."""
        return self._stage_last_ms("rs")

    # -- outer code, decoding with reliabilities (errors-and-erasures, the erased symbols chosen per codeword) ---------
    def rs_rel_from_soft(self, values):
        """Host mode: list of int8 arrays, 8 values per byte (what rx_soft() returns for the packets of an RS link
        without an inner code) -> list of uint8 arrays, one reliability per byte (rs.rel_from_values on the GPU)."""
        assert not self.device_ptrs
        blob, offs, lens = _pack_values(values, strict=True)
        out = np.zeros(max(int(lens.astype(np.int64).sum()), 1), np.uint8)
        roff = self._codec_encode(self._lib.ofdm_rs_rel_from_soft, (), _ptr(blob), offs, lens, _ptr(out), len(out))
        return [out[int(roff[i]):int(roff[i + 1])].copy() for i in range(len(lens))]

    def rs_rel_from_soft_device(self, soft_ptr, offs, lens, rel_ptr, rel_cap):
        """Device mode: the values (e.g. what rx_soft_device() wrote, with its offsets; lens in bytes = values / 8) and
        the reliabilities are device pointers; offs / lens are NumPy host arrays.  Returns the nblk + 1 reliability
        offsets (uint64), which rs_decode_rel_device() takes as ``rel_offs``."""
        assert self.device_ptrs
        return self._codec_encode(self._lib.ofdm_rs_rel_from_soft, (), C.c_void_p(soft_ptr), offs, lens, C.c_void_p(rel_ptr), rel_cap)

    def _rs_decode_rel(self, cfg, in_ptr, offs, lens, rel_ptr, rel_offs, out_ptr, out_cap):
        head = (C.byref(cfg),) + self._batch(in_ptr, offs, lens, rel_ptr, None if rel_offs is None else _u64(rel_offs))
        return self._codec_decode(self._lib.ofdm_rs_decode_rel, head, len(lens), out_ptr, out_cap, extra=(np.uint32, np.uint32))

    def rs_decode_rel(self, blocks, rel, rs=None):
        """Host mode: rs_decode() with reliabilities: ``rel`` holds one uint8 array (or bytes) per block, one value per
        byte of it, 0 the least reliable, 255 never erased; None decodes without.  ``rs``: None / True (at most 28
        erasures per codeword), a dict of rs.rs_cfg's keywords or an ``ofdm_rs_rel_cfg``.  Returns a list of
        (ok, payload, corrected, failed, second): as rs_decode(), and the codewords the second pass decoded."""
        assert not self.device_ptrs
        from . import rs as _rs
        cfg = _rs.as_cfg(rs)
        blob, offs, lens = pack_payloads(blocks)
        rblob = None
        if rel is not None:
            rel = [np.frombuffer(bytes(r), np.uint8) if isinstance(r, (bytes, bytearray)) else np.ascontiguousarray(r, np.uint8).reshape(-1)
                   for r in rel]
            if [len(r) for r in rel] != [len(b) for b in blocks]:
                raise ValueError("rs: one reliability per byte of every block")
            rblob = np.concatenate(rel + [np.zeros(1, np.uint8)])     # laid out like the blocks: rel_off = coded_off
        out = np.zeros(max(int(lens.astype(np.int64).sum()), 1), np.uint8)
        return self._codec_results(out, *self._rs_decode_rel(cfg, _ptr(blob), offs, lens, None if rblob is None else _ptr(rblob), None,
                                                             _ptr(out), len(out)))

    def rs_decode_rel_device(self, in_ptr, offs, lens, rel_ptr, rel_offs, payload_ptr, payload_cap, rs=None):
        """Device mode: blocks, reliabilities (``rel_ptr`` 0 / None: none; ``rel_offs`` None: at the blocks' offsets)
        and payloads are device pointers; offs / lens / rel_offs are NumPy host arrays.  Returns (payload offsets
        uint64[nblk + 1], ok uint8[nblk], corrected, failed, second uint32[nblk]) as host arrays."""
        assert self.device_ptrs
        from . import rs as _rs
        return self._rs_decode_rel(_rs.as_cfg(rs), C.c_void_p(in_ptr), offs, lens, C.c_void_p(rel_ptr) if rel_ptr else None, rel_offs,
                                   C.c_void_p(payload_ptr), payload_cap)

    def rs_rel_last_ms(self):
        """HIP-event time of k_rs_rel_soft in the last rs_rel_from_soft call (needs prof_enable())."""
        return self._stage_last_ms("rs_rel")

    # -- soft-decision receive: per-bit reliabilities of the delivered packets, decoded where they lie ---------------
    def set_rx_soft(self, soft=True):
        """Soft values for the following rx() / rx_device() calls: ``True`` (scale 32), ``dict(scale=)`` or a number
        (the scale); ``None`` / ``False`` turns them off and frees their buffer."""
        if soft is None or soft is False:
            self._check(self._lib.ofdm_set_rx_soft(self._h, None))
            return
        if isinstance(soft, dict):
            unknown = set(soft) - {"scale"}
            if unknown:
                raise ValueError("unknown soft option(s): %s" % ", ".join(sorted(unknown)))
            scale = soft.get("scale", 32.0)
        else:
            scale = 32.0 if soft is True else soft
        cfg = _abi.ofdm_soft_cfg(struct_size=C.sizeof(_abi.ofdm_soft_cfg), scale=float(scale))
        self._check(self._lib.ofdm_set_rx_soft(self._h, C.byref(cfg)))

    def _rx_soft_offsets(self):
        n = C.c_int(0)
        self._check(self._lib.ofdm_rx_soft(self._h, None, 0, None, C.byref(n)))
        off = np.zeros(n.value + 1, np.uint64)
        self._check(self._lib.ofdm_rx_soft(self._h, None, 0, _u64(off), C.byref(n)))
        return n.value, off

    def rx_soft(self):
        """Host mode: the soft values of the packets the last rx() returned, in the same order: a list of int8 arrays,
        8 * len(payload) values each, MSB first (v > 0: the bit is 1; 0: an erasure).  ValueError if that call ran
        without set_rx_soft()."""
        assert not self.device_ptrs
        n, off = self._rx_soft_offsets()
        vals = np.zeros(max(int(off[n]), 1), np.int8)
        if off[n]:
            self._check(self._lib.ofdm_rx_soft(self._h, _ptr(vals), len(vals), None, C.byref(C.c_int(0))))
        return [vals[int(off[i]):int(off[i + 1])].copy() for i in range(n)]

    def rx_soft_device(self, out_ptr, cap):
        """Device mode: copies the last call's values to the device buffer ``out_ptr`` (``cap`` values); returns the
        n + 1 value offsets (uint64, host)."""
        assert self.device_ptrs
        n, off = self._rx_soft_offsets()
        self._check(self._lib.ofdm_rx_soft(self._h, C.c_void_p(out_ptr), int(cap), None, C.byref(C.c_int(0))))
        return off

    def rx_fec_decode_soft(self, fec=None):
        """Host mode: the packets the last rx() returned, decoded from the handle's own soft values (they never visit
        the host) -> list of (ok, payload, corrected) as fec_decode_soft.  Needs set_rx_soft() before that rx()."""
        assert not self.device_ptrs
        n, off = self._rx_soft_offsets()
        cfg = self._fec_cfg(fec)
        out = np.zeros(self._fec_payload_room(cfg, [int(off[n]) // 8]), np.uint8)
        return self._codec_results(out, *self._codec_decode(self._lib.ofdm_rx_fec_decode_soft, (C.byref(cfg),), n, _ptr(out), len(out),
                                                            tail=self._rx_batch(n)))

    def rx_fec_decode_soft_device(self, payload_ptr, payload_cap, fec=None):
        """Device mode: the same into the device buffer ``payload_ptr``; returns (payload offsets uint64[n + 1],
        ok uint8[n], corrected uint32[n]) as host arrays."""
        assert self.device_ptrs
        n, _ = self._rx_soft_offsets()
        return self._codec_decode(self._lib.ofdm_rx_fec_decode_soft, (C.byref(self._fec_cfg(fec)),), n, C.c_void_p(payload_ptr),
                                  payload_cap, tail=self._rx_batch(n))

    def rx_fec_decode_soft_rel(self, fec=None):
        """Host mode: rx_fec_decode_soft() with reliabilities -> list of (ok, payload, corrected, rel) as
        fec_decode_rel."""
        assert not self.device_ptrs
        n, off = self._rx_soft_offsets()
        cfg = self._fec_cfg(fec)
        out = np.zeros(self._fec_payload_room(cfg, [int(off[n]) // 8]), np.uint8)
        rel = np.zeros(len(out), np.uint8)
        return self._fec_rel_results(out, rel, *self._codec_decode(self._lib.ofdm_rx_fec_decode_soft_rel, (C.byref(cfg),), n, _ptr(out),
                                                                   len(out), tail=(_ptr(rel), len(rel)) + self._rx_batch(n)))

    def rx_fec_decode_soft_rel_device(self, payload_ptr, payload_cap, rel_ptr, rel_cap, fec=None):
        """Device mode: the same into the device buffers ``payload_ptr`` and ``rel_ptr``; returns (payload offsets
        uint64[n + 1], ok uint8[n], corrected uint32[n]) as host arrays."""
        assert self.device_ptrs
        n, _ = self._rx_soft_offsets()
        return self._codec_decode(self._lib.ofdm_rx_fec_decode_soft_rel, (C.byref(self._fec_cfg(fec)),), n, C.c_void_p(payload_ptr),
                                  payload_cap, tail=(C.c_void_p(rel_ptr), int(rel_cap)) + self._rx_batch(n))

    def rx_soft_last_ms(self):
        """HIP-event time of k_soft_demap in the last rx() / rx_device() (needs prof_enable())."""
        return self._stage_last_ms("rx_soft")

    # -- coded links, the second inner code (QC-LDPC encoder and layered min-sum decoder over the payloads) -----------
    _LDPC_EXTRA = (np.uint8, np.uint32)   # iters, cw_failed

    def _ldpc_cfg(self, ldpc):
        from . import ldpc as _ldpc
        cfg = _ldpc.as_cfg(True if ldpc is None else ldpc)
        if cfg is None:
            raise ValueError("ldpc=False names no code")
        return cfg

    def ldpc_encode(self, payloads, ldpc=None):
        """Host mode: list of payloads (0 .. ldpc.max_payload(rate) bytes each) -> list of coded blocks
        (ldpc.coded_len(n, rate) bytes each), the payloads tx() then takes.  ``ldpc``: None / True, max_iters, a dict of
        ldpc.ldpc_cfg's keywords or an ``ofdm_ldpc_cfg`` (the encoder takes its rate and only checks the rest)."""
        # n + 4 + PB ceil((n + 4) / KI) <= 2 n + 104 at every rate (PB <= KI, PB <= 96)
        return self._codec_encode_host(self._lib.ofdm_ldpc_encode, (C.byref(self._ldpc_cfg(ldpc)),), payloads,
                                       lambda lens: 2 * lens.sum() + 104 * len(lens))

    def ldpc_encode_device(self, payload_ptr, offs, lens, coded_ptr, coded_cap, ldpc=None):
        """Device mode: payload bytes and coded blocks are device pointers; offs / lens are NumPy host arrays.
        Returns the nblk + 1 block offsets (uint64)."""
        assert self.device_ptrs
        return self._codec_encode(self._lib.ofdm_ldpc_encode, (C.byref(self._ldpc_cfg(ldpc)),), C.c_void_p(payload_ptr), offs, lens,
                                  C.c_void_p(coded_ptr), coded_cap)

    def _ldpc_decode(self, fn, ldpc, in_ptr, offs, lens, out_ptr, out_cap):
        head = (C.byref(self._ldpc_cfg(ldpc)),) + self._batch(in_ptr, offs, lens)
        return self._codec_decode(fn, head, len(lens), out_ptr, out_cap, extra=self._LDPC_EXTRA)

    def _ldpc_decode_host(self, fn, ldpc, packed):
        assert not self.device_ptrs
        blob, offs, lens = packed
        out = np.zeros(max(int(lens.astype(np.int64).sum()), 1), np.uint8)      # a payload is shorter than its block
        return self._codec_results(out, *self._ldpc_decode(fn, ldpc, _ptr(blob), offs, lens, _ptr(out), len(out)))

    def ldpc_decode(self, blocks, ldpc=None):
        """Host mode: list of received blocks (hard bytes of any length, e.g. the payloads rx() delivered whatever
        their CRC said) -> list of (ok, payload, corrected, iters, cw_failed): the decoded payload, whether its inner
        CRC matches, the sent bits the decoder changed, the most iterations one of the block's codewords took and
        the codewords that never met all checks.  A length that is no block gives (False, b"", 0, 0, 0)."""
        return self._ldpc_decode_host(self._lib.ofdm_ldpc_decode, ldpc, pack_payloads(blocks))

    def ldpc_decode_soft(self, values, ldpc=None):
        """Host mode: list of int8 arrays, one value per sent bit (v > 0 means 1, 0 is an erasure, -128 reads as
        -127), 8 per coded byte -> list of (ok, payload, corrected, iters, cw_failed) as ldpc_decode.  An array whose
        length is no multiple of 8, or no block's, gives (False, b"", 0, 0, 0)."""
        return self._ldpc_decode_host(self._lib.ofdm_ldpc_decode_soft, ldpc, _pack_values(values))

    def ldpc_decode_device(self, in_ptr, offs, lens, payload_ptr, payload_cap, ldpc=None, soft=False):
        """Device mode: the blocks (hard bytes, or int8 values with ``soft``: 8 per coded byte, offsets in values) and
        the payloads are device pointers; offs / lens (coded bytes) are NumPy host arrays.  Returns (payload offsets
        uint64[nblk + 1], ok uint8[nblk], corrected uint32[nblk], iters uint8[nblk], cw_failed uint32[nblk]) as host
        arrays."""
        assert self.device_ptrs
        fn = self._lib.ofdm_ldpc_decode_soft if soft else self._lib.ofdm_ldpc_decode
        return self._ldpc_decode(fn, ldpc, C.c_void_p(in_ptr), offs, lens, C.c_void_p(payload_ptr), payload_cap)

    def _rx_ldpc_decode_soft(self, ldpc, out_ptr, out_cap, n):
        return self._codec_decode(self._lib.ofdm_rx_ldpc_decode_soft, (C.byref(self._ldpc_cfg(ldpc)),), n, out_ptr, out_cap,
                                  extra=self._LDPC_EXTRA, tail=self._rx_batch(n))

    def rx_ldpc_decode_soft(self, ldpc=None):
        """Host mode: the packets the last rx() returned, decoded from the handle's own soft values (they never visit
        the host) -> list of (ok, payload, corrected, iters, cw_failed) as ldpc_decode_soft.  Needs set_rx_soft()
        before that rx()."""
        assert not self.device_ptrs
        n, off = self._rx_soft_offsets()
        out = np.zeros(max(int(off[n]) // 8, 1), np.uint8)                      # 8 values per coded byte
        return self._codec_results(out, *self._rx_ldpc_decode_soft(ldpc, _ptr(out), len(out), n))

    def rx_ldpc_decode_soft_device(self, payload_ptr, payload_cap, ldpc=None):
        """Device mode: the same into the device buffer ``payload_ptr``; returns the host arrays of
        ldpc_decode_device."""
        assert self.device_ptrs
        n, _ = self._rx_soft_offsets()
        return self._rx_ldpc_decode_soft(ldpc, C.c_void_p(payload_ptr), payload_cap, n)

    def ldpc_last_ms(self):
        """HIP-event time of k_ldpc_encode / k_ldpc_decode (k_ldpc_decode_rel after a ``*_rel`` call) in the last ldpc
        call (needs prof_enable())."""
        return self._stage_last_ms("ldpc")

    # -- LDPC coded links, reliabilities out (one byte per payload byte from the min-sum decoder's final values) --------
    @staticmethod
    def _ldpc_rel_results(out, rel, poff, ok, *cols):
        return [r + (rel[int(poff[i]):int(poff[i + 1])].copy(),) for i, r in enumerate(Engine._codec_results(out, poff, ok, *cols))]

    def _ldpc_decode_rel_host(self, fn, ldpc, packed):
        assert not self.device_ptrs
        blob, offs, lens = packed
        out = np.zeros(max(int(lens.astype(np.int64).sum()), 1), np.uint8)      # a payload is shorter than its block
        rel = np.zeros(len(out), np.uint8)
        head = (C.byref(self._ldpc_cfg(ldpc)),) + self._batch(_ptr(blob), offs, lens)
        return self._ldpc_rel_results(out, rel, *self._codec_decode(fn, head, len(lens), _ptr(out), len(out), extra=self._LDPC_EXTRA,
                                                                    tail=(_ptr(rel), len(rel))))

    def ldpc_decode_rel(self, blocks, ldpc=None):
        """Host mode: ldpc_decode() with reliabilities -> list of (ok, payload, corrected, iters, cw_failed, rel):
        ldpc_decode()'s five fields, and ``rel`` a uint8 array of len(payload): min(127, the smallest final |P| of the
        byte's eight bits), plus 128 where the byte's codeword met all checks; 255 is "never erase" -- what
        rs_decode_rel() takes.  A length that is no block gives (False, b"", 0, 0, 0, [])."""
        return self._ldpc_decode_rel_host(self._lib.ofdm_ldpc_decode_rel, ldpc, pack_payloads(blocks))

    def ldpc_decode_soft_rel(self, values, ldpc=None):
        """Host mode: ldpc_decode_soft() with reliabilities -> list of (ok, payload, corrected, iters, cw_failed, rel) as
        ldpc_decode_rel."""
        return self._ldpc_decode_rel_host(self._lib.ofdm_ldpc_decode_soft_rel, ldpc, _pack_values(values))

    def ldpc_decode_rel_device(self, in_ptr, offs, lens, payload_ptr, payload_cap, rel_ptr, rel_cap, ldpc=None, soft=False):
        """Device mode: ldpc_decode_device() with the reliabilities written to the device buffer ``rel_ptr`` at the
        payloads' offsets: (payload_ptr, rel_ptr, the returned offsets) are what rs_decode_rel_device() takes as blocks,
        reliabilities and offsets, with ``rel_offs=None``.  Returns the host arrays of ldpc_decode_device."""
        assert self.device_ptrs
        fn = self._lib.ofdm_ldpc_decode_soft_rel if soft else self._lib.ofdm_ldpc_decode_rel
        head = (C.byref(self._ldpc_cfg(ldpc)),) + self._batch(C.c_void_p(in_ptr), offs, lens)
        return self._codec_decode(fn, head, len(lens), C.c_void_p(payload_ptr), payload_cap, extra=self._LDPC_EXTRA,
                                  tail=(C.c_void_p(rel_ptr), int(rel_cap)))

    def _rx_ldpc_decode_soft_rel(self, ldpc, out_ptr, out_cap, rel_ptr, rel_cap, n):
        return self._codec_decode(self._lib.ofdm_rx_ldpc_decode_soft_rel, (C.byref(self._ldpc_cfg(ldpc)),), n, out_ptr, out_cap,
                                  extra=self._LDPC_EXTRA, tail=(rel_ptr, int(rel_cap)) + self._rx_batch(n))

    def rx_ldpc_decode_soft_rel(self, ldpc=None):
        """Host mode: rx_ldpc_decode_soft() with reliabilities -> list of (ok, payload, corrected, iters, cw_failed, rel)
        as ldpc_decode_rel."""
        assert not self.device_ptrs
        n, off = self._rx_soft_offsets()
        out = np.zeros(max(int(off[n]) // 8, 1), np.uint8)                      # 8 values per coded byte
        rel = np.zeros(len(out), np.uint8)
        return self._ldpc_rel_results(out, rel, *self._rx_ldpc_decode_soft_rel(ldpc, _ptr(out), len(out), _ptr(rel), len(rel), n))

    def rx_ldpc_decode_soft_rel_device(self, payload_ptr, payload_cap, rel_ptr, rel_cap, ldpc=None):
        """Device mode: the same into the device buffers ``payload_ptr`` and ``rel_ptr``; returns the host arrays of
        ldpc_decode_device."""
        assert self.device_ptrs
        n, _ = self._rx_soft_offsets()
        return self._rx_ldpc_decode_soft_rel(ldpc, C.c_void_p(payload_ptr), payload_cap, C.c_void_p(rel_ptr), rel_cap, n)

    # -- coded links: the signal field (12 bytes in front of a block that name its coding; sig.py) ----------------------
    @staticmethod
    def _sig_words(words):
        from . import sig as _sig
        return np.ascontiguousarray([w.word if isinstance(w, _sig.Coding) else int(w) for w in words], np.uint16)

    def sig_encode(self, words, bodies):
        """Host mode: one coding word (or sig.Coding) and one body (bytes, e.g. what fec_encode() returned) per block
        -> list of blocks, the 12-byte field in front of each body: the payloads tx() then takes.  ValueError for a
        word that is not valid."""
        assert not self.device_ptrs
        words = self._sig_words(words)
        if len(words) != len(bodies):
            raise ValueError("sig: one word per body")
        return self._codec_encode_host(self._lib.ofdm_sig_encode, (words.ctypes.data_as(C.POINTER(C.c_uint16)),), bodies,
                                       lambda lens: lens.sum() + 12 * len(lens))

    def sig_encode_device(self, words, body_ptr, offs, lens, out_ptr, out_cap):
        """Device mode: bodies and blocks are device pointers; words / offs / lens are host arrays.  Returns the
        nblk + 1 block offsets (uint64)."""
        assert self.device_ptrs
        words = self._sig_words(words)
        if len(words) != len(lens):
            raise ValueError("sig: one word per body")
        return self._codec_encode(self._lib.ofdm_sig_encode, (words.ctypes.data_as(C.POINTER(C.c_uint16)),), C.c_void_p(body_ptr), offs,
                                  lens, C.c_void_p(out_ptr), out_cap)

    def _sig_decode(self, fn, head, n, tail=()):
        """fn(handle, *head, word, margin, *tail) over n packets -> (word uint16[n], margin uint16[n])."""
        word, margin = np.zeros(max(n, 1), np.uint16), np.zeros(max(n, 1), np.uint16)
        u16p = C.POINTER(C.c_uint16)
        self._check(fn(self._h, *head, word.ctypes.data_as(u16p), margin.ctypes.data_as(u16p), *tail))
        return word[:n], margin[:n]

    @staticmethod
    def _sig_results(word, margin):
        return [(int(w), int(m)) for w, m in zip(word, margin)]

    def sig_decode(self, blocks):
        """Host mode: list of received blocks (hard bytes of any length, e.g. the payloads rx() delivered whatever
        their CRC said) -> list of (word, margin): the most likely coding word of each block's field -- valid or not,
        sig.word_valid() tells -- and how far its metric lies above the next word's (0 .. 24384; 0: a tie).  A block
        under 12 bytes gives (0xFFFF, 0)."""
        assert not self.device_ptrs
        blob, offs, lens = pack_payloads(blocks)
        return self._sig_results(*self._sig_decode(self._lib.ofdm_sig_decode, self._batch(_ptr(blob), offs, lens), len(lens)))

    def sig_decode_soft(self, values):
        """Host mode: list of int8 arrays, one value per bit (v > 0 means 1, 0 is an erasure, -128 reads as -127), 8 per
        byte of the block -> list of (word, margin) as sig_decode.  An array under 96 values, or whose length is no
        multiple of 8, gives (0xFFFF, 0)."""
        assert not self.device_ptrs
        blob, offs, lens = _pack_values(values)
        return self._sig_results(*self._sig_decode(self._lib.ofdm_sig_decode_soft, self._batch(_ptr(blob), offs, lens), len(lens)))

    def sig_decode_device(self, in_ptr, offs, lens, soft=False):
        """Device mode: the blocks (hard bytes, or int8 values with ``soft``: 8 per byte, offsets in values) are a
        device pointer; offs / lens (bytes) are NumPy host arrays.  Returns (word uint16[nblk], margin uint16[nblk])
        as host arrays."""
        assert self.device_ptrs
        fn = self._lib.ofdm_sig_decode_soft if soft else self._lib.ofdm_sig_decode
        return self._sig_decode(fn, self._batch(C.c_void_p(in_ptr), offs, lens), len(lens))

    def rx_sig_decode_soft(self):
        """Host mode: the fields of the packets the last rx() returned, decoded from the handle's own soft values (they
        never visit the host) -> list of (word, margin) as sig_decode_soft.  Needs set_rx_soft() before that rx()."""
        assert not self.device_ptrs
        n, _ = self._rx_soft_offsets()
        return self._sig_results(*self._sig_decode(self._lib.ofdm_rx_sig_decode_soft, (), n, tail=self._rx_batch(n)))

    def rx_sig_decode_soft_device(self):
        """Device mode: the same; returns the host arrays of sig_decode_device."""
        assert self.device_ptrs
        n, _ = self._rx_soft_offsets()
        return self._sig_decode(self._lib.ofdm_rx_sig_decode_soft, (), n, tail=self._rx_batch(n))

    def sig_last_ms(self):
        """HIP-event time of k_sig_encode / k_sig_decode in the last sig call (needs prof_enable())."""
        return self._stage_last_ms("sig")

    def rx_packet_pos(self):
        """Flag sample (relative to the last rx() call's IQ) of every packet it delivered."""
        n = C.c_int(0)
        self._check(self._lib.ofdm_rx_packet_pos(self._h, None, 0, C.byref(n)))
        pos = np.zeros(max(n.value, 1), np.uint64)
        if n.value:
            self._check(self._lib.ofdm_rx_packet_pos(self._h, _ptr(pos), n.value, C.byref(n)))
        return pos[:n.value]

    def rx_nco_state(self):
        """(flags uint64, phase uint64 in 2^-64 turn, step float64, swallowed uint8) of the last rx() call."""
        n = C.c_int(0)
        self._check(self._lib.ofdm_rx_nco_state(self._h, None, None, None, None, 0, C.byref(n)))
        k = n.value
        fl, phi = np.zeros(max(k, 1), np.uint64), np.zeros(max(k, 1), np.uint64)
        st, sw = np.zeros(max(k, 1), np.float64), np.zeros(max(k, 1), np.uint8)
        if k:
            self._check(self._lib.ofdm_rx_nco_state(self._h, _ptr(fl), _ptr(phi), _ptr(st), _ptr(sw), k, C.byref(n)))
        return fl[:k], phi[:k], st[:k], sw[:k]

    def set_origin(self, first_sample_index=0):
        """Index, in its capture, of the first sample of the following rx() calls: keeps the channel
        filter's block grid where one call on the whole capture would have it."""
        self._check(self._lib.ofdm_rx_set_origin(self._h, int(first_sample_index)))

    def set_flag_history(self, flags=None, steps=None, swallowed=None, trust_after=-1, pred=(0, 0, 0.0)):
        """The settled past for the following rx() calls (flags=None switches it off): ``flags`` /
        ``steps`` / ``swallowed`` replace what a call detects up to ``trust_after``; ``pred`` = (flag,
        phase, step) of the flag before them (may lie before the call's first sample)."""
        if flags is None:
            self._check(self._lib.ofdm_rx_set_flag_history(self._h, 0, 0, None, None, None, 0, 0, 0, 0.0))
            return
        fl = np.ascontiguousarray(flags, np.int64)
        st = np.ascontiguousarray(steps, np.float64)
        sw = np.ascontiguousarray(swallowed, np.uint8)
        k = len(fl)
        self._check(self._lib.ofdm_rx_set_flag_history(self._h, 1, k, _ptr(fl) if k else None, _ptr(st) if k else None,
                                                       _ptr(sw) if k else None, int(trust_after), int(pred[0]),
                                                       int(pred[1]), float(pred[2])))

    # -- spectrum sensing ----------------------------------------------------------
    def _sense_outputs(self, sc, nm, nd):
        S = sc.fft_size
        return (np.zeros((max(nm, 1), S), np.float32), np.zeros((max(nd, 1), S), np.float64),
                np.zeros((max(nd, 1), S), np.uint8), np.zeros((max(nd, 1), S // 4), np.uint8))

    @staticmethod
    def _sense_pack(msgs, mean, bits, hexs, nm, nd):
        return {"msgs": msgs[:nm], "mean": mean[:nd], "bits": bits[:nd],
                "hex": [hexs[d].tobytes().decode("ascii") for d in range(nd)]}

    def sense_count(self, sc, nsamples):
        nm, nd = C.c_uint64(0), C.c_uint64(0)
        self._check(self._lib.ofdm_sense_count(C.byref(sc), int(nsamples), C.byref(nm), C.byref(nd)))
        return nm.value, nd.value

    def sense(self, sc, iq, nsamples=None):
        """The `sensor` flowgraph + sense_loop of predictive_sense.py over one IQ stream.
        Returns {"msgs": float32[nmsgs][fft] (bin_statistics_f message bodies, FFT order),
        "mean": float64[ndec][fft], "bits": uint8[ndec][fft] (both ascending frequency),
        "hex": [str]} -- one hex carrier map per decision, as hex_conv returns it."""
        if self.device_ptrs:
            ptr, n = C.c_void_p(int(iq)), int(nsamples)
        else:
            iq = self._rx_samples(iq)
            ptr, n = (_ptr(iq) if len(iq) else None), len(iq)
        nm, nd = self.sense_count(sc, n)
        msgs, mean, bits, hexs = self._sense_outputs(sc, nm, nd)
        onm, ond = C.c_uint64(0), C.c_uint64(0)
        self._check(self._lib.ofdm_sense(self._h, C.byref(sc), ptr, n, _ptr(msgs), max(nm, 1), _ptr(mean), _ptr(bits),
                                         _ptr(hexs), max(nd, 1), C.byref(onm), C.byref(ond)))
        return self._sense_pack(msgs, mean, bits, hexs, onm.value, ond.value)

    def sense_decide(self, sc, msgs):
        """sense_loop alone over message bodies [nmsgs][fft_size] (e.g. from a real msg_queue)."""
        msgs = np.ascontiguousarray(msgs, np.float32)
        nm = msgs.shape[0]
        nd = nm // (sc.avg_msgs + sc.skip_msgs)
        _, mean, bits, hexs = self._sense_outputs(sc, 0, nd)
        ond = C.c_uint64(0)
        self._check(self._lib.ofdm_sense_decide(self._h, C.byref(sc), _ptr(msgs), nm, _ptr(mean), _ptr(bits),
                                                _ptr(hexs), max(nd, 1), C.byref(ond)))
        r = self._sense_pack(msgs, mean, bits, hexs, nm, ond.value)
        del r["msgs"]
        return r

    def set_rx_sense(self, sc):
        """Fuse the sensor into every following rx()/rx_device() call (None switches it off)."""
        self._rx_sense_cfg = sc
        self._check(self._lib.ofdm_set_rx_sense(self._h, C.byref(sc) if sc is not None else None))

    def rx_sense_result(self, nsamples, want_msgs=True, want_mean=True):
        """Outcome of the sensing run fused into the last rx()/rx_device() call.  The message
        bodies and the means are large for long streams: leave them on the device with
        want_msgs/want_mean=False when only the decisions are needed."""
        sc = self._rx_sense_cfg
        if sc is None:
            raise ValueError("set_rx_sense() has not been called")
        nm, nd = self.sense_count(sc, nsamples)
        msgs, mean, bits, hexs = self._sense_outputs(sc, nm if want_msgs else 0, nd)
        onm, ond = C.c_uint64(0), C.c_uint64(0)
        self._check(self._lib.ofdm_rx_sense_result(self._h, _ptr(msgs) if want_msgs else None, max(nm, 1),
                                                   _ptr(mean) if want_mean else None, _ptr(bits), _ptr(hexs),
                                                   max(nd, 1), C.byref(onm), C.byref(ond)))
        r = self._sense_pack(msgs, mean, bits, hexs, onm.value if want_msgs else 0, ond.value)
        if not want_msgs:
            del r["msgs"]
        if not want_mean:
            del r["mean"]
        return r

    def sense_device_msgs(self):
        """(device pointer, nmsgs, fft_size) of the last run's message bodies, for an in-place
        cross-GPU max-reduce (parallel.allreduce_sensed); follow with sense_redecide()."""
        p, nm, S = C.c_void_p(None), C.c_uint64(0), C.c_uint32(0)
        self._check(self._lib.ofdm_sense_device_msgs(self._h, C.byref(p), C.byref(nm), C.byref(S)))
        return (p.value or 0), nm.value, S.value

    def sense_redecide(self, sc=None):
        sc = self._rx_sense_cfg if sc is None else sc
        self._check(self._lib.ofdm_sense_redecide(self._h, C.byref(sc)))

    # -- taps ---------------------------------------------------------------------
    _TAP_DTYPES = {
        _abi.TAP_TX_PACKETS: np.uint8, _abi.TAP_TX_FREQ: np.complex64, _abi.TAP_RX_CHAN_FILT: np.complex64,
        _abi.TAP_RX_METRIC: np.float32, _abi.TAP_RX_PEAKS: np.uint64, _abi.TAP_RX_ANGLES: np.float32,
        _abi.TAP_RX_FRAMES: np.uint64, _abi.TAP_RX_FFT: np.complex64, _abi.TAP_RX_ACQ: np.complex64,
        _abi.TAP_RX_SINK: np.complex64, _abi.TAP_RX_PACKETS: np.uint8, _abi.TAP_TX_MAPPER: np.complex64,
        _abi.TAP_TX_IFFT: np.complex64, _abi.TAP_RX_SAMPLER: np.complex64, _abi.TAP_RX_SIGMIX: np.complex64,
        _abi.TAP_RX_NCO: np.complex64, _abi.TAP_RX_PRESEL: np.float32, _abi.TAP_RX_DEMAPPED: np.uint8,
        _abi.TAP_RX_RUN_AVG: np.float64,
    }

    def tap(self, tap):
        nb = C.c_uint64(0)
        self._check(self._lib.ofdm_tap(self._h, tap, None, 0, C.byref(nb)))
        dt = np.dtype(self._TAP_DTYPES[tap])
        out = np.zeros(nb.value // dt.itemsize, dt)
        if nb.value:
            self._check(self._lib.ofdm_tap(self._h, tap, _ptr(out), nb.value, C.byref(nb)))
        if tap in (_abi.TAP_RX_FRAMES, _abi.TAP_RX_RUN_AVG):
            out = out.reshape(-1, 2)
        elif tap in (_abi.TAP_TX_FREQ, _abi.TAP_RX_FFT, _abi.TAP_TX_MAPPER, _abi.TAP_TX_IFFT, _abi.TAP_RX_SAMPLER):
            out = out.reshape(-1, self.N)
        elif tap in (_abi.TAP_RX_ACQ, _abi.TAP_RX_SINK):
            out = out.reshape(-1, self.occ)
        return out


def device_count():
    return _abi.load().ofdm_device_count()
