"""ctypes view of include/ofdm_hip.h and the loader for libofdm_hip.so.

The library is the product: there is no Python/NumPy fallback.  Loading fails
loudly if the shared object has not been built (``python -c "import
__graft_entry__ as g; g.build()"`` or ``make -C ofdm_uhd_amd/csrc``).
"""
import ctypes as C
import os

OFDM_ABI_VERSION = 6
OFDM_MAX_FFT = 4096
OFDM_MAX_TAPS = 512
OFDM_MAX_ARITY = 256
OFDM_MASK_LEN = 4096
OFDM_MAX_PKT_LEN = 4096
OFDM_MAX_CARRIER_HEX = 1024
OFDM_DDC_MAX_TAPS = 1024
OFDM_DDC_BANK_MAX_LINKS = 8
OFDM_RESAMP_MAX_TAPS = 1024
OFDM_RESAMP_BANK_MAX_LINKS = 8
OFDM_DUC_MAX_TAPS = 1024
OFDM_DUC_BANK_MAX_LINKS = 8
OFDM_TX_RESAMP_MAX_TAPS = 1024
OFDM_TX_RESAMP_BANK_MAX_LINKS = 8
OFDM_PFB_MAX_CHANNELS = 64
OFDM_PFB_MAX_TAPS = 1024
OFDM_MULTIPATH_MAX_PATHS = 16
OFDM_MULTIPATH_MAX_TONES = 4
OFDM_MULTIPATH_MAX_DELAY = 1023
OFDM_CFR_MAX_TAPS = 1023
OFDM_MEMPOLY_MAX_MEMORY = 8
OFDM_MEMPOLY_MAX_ORDERS = 5
OFDM_MEMPOLY_DPD, OFDM_MEMPOLY_PA = 0, 1     # the two slots of ofdm_set_mempoly
OFDM_MEMPOLY_SLOTS = 2
OFDM_PSD_MAX_FFT = 4096
OFDM_FEC_MAX_PAYLOAD = 2040
OFDM_FEC_MAX_CODED = 4090
OFDM_FEC_RATE_1_2, OFDM_FEC_RATE_2_3, OFDM_FEC_RATE_3_4, OFDM_FEC_RATE_5_6 = 0, 1, 2, 3
OFDM_LDPC_MAX_PAYLOAD = 2012
OFDM_LDPC_MAX_CODED = 4032
OFDM_LDPC_RATE_1_2, OFDM_LDPC_RATE_2_3, OFDM_LDPC_RATE_3_4, OFDM_LDPC_RATE_5_6 = 0, 1, 2, 3
OFDM_SIG_FIELD_BYTES = 12
OFDM_SIG_CODEC_NONE, OFDM_SIG_CODEC_FEC, OFDM_SIG_CODEC_LDPC = 0, 1, 2
OFDM_SIG_NO_WORD = 0xFFFF
OFDM_RS_PARITY = 32
OFDM_RS_MAX_PAYLOAD = 3564
OFDM_RS_MAX_CODED = 4080

OFDM_OK = 0
OFDM_E_INVAL = -1
OFDM_E_NOMEM = -2
OFDM_E_CAPACITY = -3
OFDM_E_HIP = -4
OFDM_E_OVERFLOW = -5

OFDM_F_DEVICE_PTRS = 1 << 0
OFDM_F_PAD_FOR_USRP = 1 << 1

(TAP_TX_PACKETS, TAP_TX_FREQ, TAP_RX_CHAN_FILT, TAP_RX_METRIC, TAP_RX_PEAKS, TAP_RX_ANGLES,
 TAP_RX_FRAMES, TAP_RX_FFT, TAP_RX_ACQ, TAP_RX_SINK, TAP_RX_PACKETS, TAP_TX_MAPPER, TAP_TX_IFFT, TAP_RX_SAMPLER,
 TAP_RX_SIGMIX, TAP_RX_NCO, TAP_RX_PRESEL, TAP_RX_DEMAPPED, TAP_RX_RUN_AVG, TAP_COUNT) = range(20)
SYNC_PN, SYNC_FIXED = 0, 1
OFDM_IQ_FC32, OFDM_IQ_SC16 = 0, 1

(K_FRAME, K_TX, K_CHAN, K_SYNC, K_PEAK, K_DEMOD, K_DEFRAME, K_SENSE, K_FILTER, K_EXACT, K_FRONT, K_COUNT) = range(12)
OFDM_SENSE_MAX_FFT = 4096


class ofdm_c32(C.Structure):
    _fields_ = [("re", C.c_float), ("im", C.c_float)]


class ofdm_sc16(C.Structure):
    _fields_ = [("re", C.c_int16), ("im", C.c_int16)]


class ofdm_cfg(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("device_id", C.c_int32),
        ("flags", C.c_uint32),
        ("fft_length", C.c_uint32),
        ("occupied_tones", C.c_uint32),
        ("cp_length", C.c_uint32),
        ("arity", C.c_uint32),
        ("constellation", ofdm_c32 * OFDM_MAX_ARITY),
        ("known_symbol", ofdm_c32 * OFDM_MAX_FFT),
        ("tx_amplitude", C.c_float),
        ("phase_gain", C.c_float),
        ("freq_gain", C.c_float),
        ("eq_gain", C.c_float),
        ("max_fft_shift_len", C.c_uint32),
        ("sampler_timeout", C.c_uint32),
        ("peak_rise", C.c_float),
        ("peak_fall", C.c_float),
        ("peak_alpha", C.c_float),
        ("ntaps", C.c_uint32),
        ("taps", C.c_float * OFDM_MAX_TAPS),
        ("whitening_mask", C.c_uint8 * OFDM_MASK_LEN),
        ("whitener_offset", C.c_uint32),
        ("pad_seed", C.c_uint64),
        ("carrier_map", C.c_char * (OFDM_MAX_CARRIER_HEX + 8)),
        ("sync_mode", C.c_uint32),
        ("fixed_nsymbols", C.c_uint32),
        ("fixed_freq_offset", C.c_float),
        ("reserved0", C.c_uint32),
    ]


class ofdm_chan(C.Structure):
    _fields_ = [
        ("sigma", C.c_float),
        ("cfo", C.c_float),
        ("seed", C.c_uint64),
        ("stream_id", C.c_uint64),
        ("lead_samples", C.c_uint64),
        ("tail_samples", C.c_uint64),
    ]


class ofdm_stats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in (
        "symbols", "samples", "peaks", "frames", "headers_ok", "packets", "crc_ok",
        "chained_frames", "overflow")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class ofdm_sense_cfg(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("fft_size", C.c_uint32),
        ("tune_delay", C.c_uint32),
        ("dwell_delay", C.c_uint32),
        ("avg_msgs", C.c_uint32),
        ("skip_msgs", C.c_uint32),
        ("threshold", C.c_double),
        ("window", C.c_float * OFDM_SENSE_MAX_FFT),
    ]


class ofdm_pkt_quality(C.Structure):
    _fields_ = [
        ("flag", C.c_uint64),
        ("first_symbol", C.c_uint32),
        ("nsym", C.c_uint32),
        ("ncarriers", C.c_uint32),
        ("coarse", C.c_int32),
        ("cfo_bins", C.c_float),
        ("pilot_power", C.c_float),
        ("null_power", C.c_float),
        ("err_energy", C.c_float),
        ("ref_energy", C.c_float),
        ("snr_preamble_db", C.c_float),
        ("snr_decision_db", C.c_float),
    ]


class ofdm_ddc_cfg(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("decimation", C.c_uint32),
        ("ntaps", C.c_uint32),
        ("reserved", C.c_uint32),
        ("center_freq", C.c_double),
        ("taps", C.c_float * OFDM_DDC_MAX_TAPS),
    ]


class ofdm_ddc_bank_cfg(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("decimation", C.c_uint32),
        ("ntaps", C.c_uint32),
        ("nlinks", C.c_uint32),
        ("center_freq", C.c_double * OFDM_DDC_BANK_MAX_LINKS),
        ("taps", C.c_float * OFDM_DDC_MAX_TAPS),
    ]


class ofdm_pfb_cfg(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("nchannels", C.c_uint32),
        ("ntaps", C.c_uint32),
        ("nsel", C.c_uint32),
        ("channel", C.c_uint8 * OFDM_PFB_MAX_CHANNELS),
        ("taps", C.c_float * OFDM_PFB_MAX_TAPS),
    ]


class ofdm_pfb_synth_cfg(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("nchannels", C.c_uint32),
        ("ntaps", C.c_uint32),
        ("nsel", C.c_uint32),
        ("out_format", C.c_uint32),
        ("out_scale", C.c_float),
        ("channel", C.c_uint8 * OFDM_PFB_MAX_CHANNELS),
        ("taps", C.c_float * OFDM_PFB_MAX_TAPS),
    ]


class ofdm_duc_cfg(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("interpolation", C.c_uint32),
        ("ntaps", C.c_uint32),
        ("out_format", C.c_uint32),
        ("center_freq", C.c_double),
        ("out_scale", C.c_float),
        ("reserved", C.c_uint32),
        ("taps", C.c_float * OFDM_DUC_MAX_TAPS),
    ]


class ofdm_duc_bank_cfg(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("interpolation", C.c_uint32),
        ("ntaps", C.c_uint32),
        ("nlinks", C.c_uint32),
        ("out_format", C.c_uint32),
        ("out_scale", C.c_float),
        ("center_freq", C.c_double * OFDM_DUC_BANK_MAX_LINKS),
        ("taps", C.c_float * OFDM_DUC_MAX_TAPS),
    ]


class ofdm_resamp_cfg(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("interpolation", C.c_uint32),
        ("decimation", C.c_uint32),
        ("ntaps", C.c_uint32),
        ("center_freq", C.c_double),
        ("taps", C.c_float * OFDM_RESAMP_MAX_TAPS),
    ]


class ofdm_resamp_bank_cfg(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("interpolation", C.c_uint32),
        ("decimation", C.c_uint32),
        ("ntaps", C.c_uint32),
        ("nlinks", C.c_uint32),
        ("center_freq", C.c_double * OFDM_RESAMP_BANK_MAX_LINKS),
        ("taps", C.c_float * OFDM_RESAMP_MAX_TAPS),
    ]


class ofdm_tx_resamp_cfg(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("interpolation", C.c_uint32),
        ("decimation", C.c_uint32),
        ("ntaps", C.c_uint32),
        ("out_format", C.c_uint32),
        ("center_freq", C.c_double),
        ("out_scale", C.c_float),
        ("reserved", C.c_uint32),
        ("taps", C.c_float * OFDM_TX_RESAMP_MAX_TAPS),
    ]


class ofdm_tx_resamp_bank_cfg(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("interpolation", C.c_uint32),
        ("decimation", C.c_uint32),
        ("ntaps", C.c_uint32),
        ("nlinks", C.c_uint32),
        ("out_format", C.c_uint32),
        ("out_scale", C.c_float),
        ("center_freq", C.c_double * OFDM_TX_RESAMP_BANK_MAX_LINKS),
        ("taps", C.c_float * OFDM_TX_RESAMP_MAX_TAPS),
    ]


class ofdm_multipath_cfg(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("npaths", C.c_uint32),
        ("ntones", C.c_uint32),
        ("out_format", C.c_uint32),
        ("out_scale", C.c_float),
        ("sigma", C.c_float),
        ("cfo", C.c_float),
        ("seed", C.c_uint64),
        ("stream_id", C.c_uint64),
        ("delay", C.c_uint32 * OFDM_MULTIPATH_MAX_PATHS),
        ("gain", ofdm_c32 * OFDM_MULTIPATH_MAX_PATHS),
        ("doppler", C.c_double * OFDM_MULTIPATH_MAX_PATHS),
        ("tone_amp", C.c_float * OFDM_MULTIPATH_MAX_TONES),
        ("tone_freq", C.c_double * OFDM_MULTIPATH_MAX_TONES),
        ("tone_phase", C.c_double * OFDM_MULTIPATH_MAX_TONES),
    ]


class ofdm_cfr_cfg(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("threshold", C.c_float),
        ("ntaps", C.c_uint32),
        ("out_format", C.c_uint32),
        ("out_scale", C.c_float),
        ("taps", C.c_float * OFDM_CFR_MAX_TAPS),
    ]


class ofdm_cfr_stats(C.Structure):        # the header's ``struct ofdm_cfr_stats`` (a tag: the name is the function's)
    _fields_ = [
        ("n", C.c_uint64),
        ("n_over", C.c_uint64),
        ("n_touched", C.c_uint64),
        ("peak_in", C.c_float),
        ("peak_out", C.c_float),
        ("sum_in", C.c_double),
        ("sum_out", C.c_double),
        ("sum_err", C.c_double),
    ]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class ofdm_mempoly_cfg(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("memory", C.c_uint32),
        ("orders", C.c_uint32),
        ("out_format", C.c_uint32),
        ("out_scale", C.c_float),
        ("limit", C.c_float),
        ("coef", ofdm_c32 * (OFDM_MEMPOLY_MAX_MEMORY * OFDM_MEMPOLY_MAX_ORDERS)),
    ]


class ofdm_mempoly_stats(C.Structure):    # the header's ``struct ofdm_mempoly_stats`` (a tag: the name is the function's)
    _fields_ = [
        ("n", C.c_uint64),
        ("n_over", C.c_uint64),
        ("peak_in", C.c_float),
        ("peak_out", C.c_float),
        ("sum_in", C.c_double),
        ("sum_out", C.c_double),
    ]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class ofdm_psd_cfg(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("nfft", C.c_uint32),
        ("hop", C.c_uint32),
        ("in_format", C.c_uint32),
        ("in_scale", C.c_float),
        ("taps", C.c_float * OFDM_PSD_MAX_FFT),
    ]


class ofdm_fec_cfg(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("interleave_cols", C.c_uint32),
        ("rate", C.c_uint32),
        ("reserved", C.c_uint32 * 5),
    ]


class ofdm_soft_cfg(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("scale", C.c_float),
    ]


class ofdm_rs_rel_cfg(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("max_erasures", C.c_uint32),
        ("reserved", C.c_uint32 * 6),
    ]


class _ofdm_ldpc_cfg_tail(C.Union):       # the header's anonymous union: the rate is the word that is reserved[0]
    _fields_ = [
        ("reserved", C.c_uint32 * 6),
        ("rate", C.c_uint32),
    ]


class ofdm_ldpc_cfg(C.Structure):
    _anonymous_ = ("_tail",)
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("max_iters", C.c_uint32),
        ("_tail", _ofdm_ldpc_cfg_tail),
    ]


# every symbol include/ofdm_hip.h declares (tests check the .so exports all of them)
EXPORTS = (
    "ofdm_abi_version", "ofdm_device_count", "ofdm_create", "ofdm_destroy", "ofdm_last_error",
    "ofdm_set_stream", "ofdm_set_tx_amplitude", "ofdm_set_carrier_map", "ofdm_set_channel", "ofdm_framed_len",
    "ofdm_make_packets", "ofdm_tx_frame_count", "ofdm_tx", "ofdm_tx_async", "ofdm_wait", "ofdm_channel", "ofdm_rx",
    "ofdm_set_taps", "ofdm_tap", "ofdm_prof_enable", "ofdm_prof_reset", "ofdm_prof_get",
    "ofdm_kernel_name", "ofdm_sense_count", "ofdm_sense", "ofdm_sense_decide", "ofdm_set_rx_sense",
    "ofdm_rx_sense_result", "ofdm_sense_device_msgs", "ofdm_sense_redecide",
    "ofdm_rx_packet_pos", "ofdm_rx_nco_state", "ofdm_rx_set_flag_history", "ofdm_rx_set_origin", "ofdm_rx_submit", "ofdm_rx_snr",
    "ofdm_set_rx_quality", "ofdm_rx_quality", "ofdm_set_rx_csi", "ofdm_rx_csi", "ofdm_rx_csi_summary",
    "ofdm_set_rx_iq_format", "ofdm_set_tx_iq_format",
    "ofdm_set_ddc", "ofdm_ddc_reset", "ofdm_ddc_count", "ofdm_ddc", "ofdm_ddc_taps", "ofdm_ddc_last_ms",
    "ofdm_set_duc", "ofdm_duc_reset", "ofdm_duc", "ofdm_duc_last_ms",
    "ofdm_set_ddc_bank", "ofdm_ddc_bank_reset", "ofdm_ddc_bank_count", "ofdm_ddc_bank", "ofdm_ddc_bank_taps",
    "ofdm_ddc_bank_last_ms",
    "ofdm_set_resamp", "ofdm_resamp_reset", "ofdm_resamp_count", "ofdm_resamp", "ofdm_resamp_taps", "ofdm_resamp_last_ms",
    "ofdm_set_resamp_bank", "ofdm_resamp_bank_reset", "ofdm_resamp_bank_count", "ofdm_resamp_bank", "ofdm_resamp_bank_taps",
    "ofdm_resamp_bank_last_ms",
    "ofdm_set_tx_resamp", "ofdm_tx_resamp_reset", "ofdm_tx_resamp_count", "ofdm_tx_resamp", "ofdm_tx_resamp_last_ms",
    "ofdm_set_pfb", "ofdm_pfb_reset", "ofdm_pfb_count", "ofdm_pfb", "ofdm_pfb_last_ms",
    "ofdm_set_pfb_synth", "ofdm_pfb_synth_reset", "ofdm_pfb_synth", "ofdm_pfb_synth_last_ms",
    "ofdm_set_duc_bank", "ofdm_duc_bank_reset", "ofdm_duc_bank", "ofdm_duc_bank_taps", "ofdm_duc_bank_last_ms",
    "ofdm_set_tx_resamp_bank", "ofdm_tx_resamp_bank_reset", "ofdm_tx_resamp_bank_count", "ofdm_tx_resamp_bank",
    "ofdm_tx_resamp_bank_taps", "ofdm_tx_resamp_bank_last_ms",
    "ofdm_set_multipath", "ofdm_multipath_reset", "ofdm_multipath", "ofdm_multipath_last_ms",
    "ofdm_set_cfr", "ofdm_cfr_reset", "ofdm_cfr", "ofdm_cfr_stats", "ofdm_cfr_last_ms",
    "ofdm_set_mempoly", "ofdm_mempoly_reset", "ofdm_mempoly", "ofdm_mempoly_stats", "ofdm_mempoly_last_ms",
    "ofdm_set_psd", "ofdm_psd_reset", "ofdm_psd_count", "ofdm_psd", "ofdm_psd_read", "ofdm_psd_last_ms",
    "ofdm_fec_coded_len", "ofdm_fec_payload_len", "ofdm_fec_encode", "ofdm_fec_decode", "ofdm_fec_decode_soft",
    "ofdm_fec_last_ms", "ofdm_fec_coded_len_rate", "ofdm_fec_payload_len_rate", "ofdm_fec_punct_last_ms",
    "ofdm_set_rx_soft", "ofdm_rx_soft", "ofdm_rx_fec_decode_soft", "ofdm_rx_soft_last_ms",
    "ofdm_fec_decode_rel", "ofdm_fec_decode_soft_rel", "ofdm_rx_fec_decode_soft_rel",
    "ofdm_rs_coded_len", "ofdm_rs_payload_len", "ofdm_rs_encode", "ofdm_rs_decode", "ofdm_rs_last_ms",
    "ofdm_rs_decode_rel", "ofdm_rs_rel_from_soft", "ofdm_rs_rel_last_ms",
    "ofdm_ldpc_coded_len", "ofdm_ldpc_payload_len", "ofdm_ldpc_encode", "ofdm_ldpc_decode", "ofdm_ldpc_decode_soft",
    "ofdm_rx_ldpc_decode_soft", "ofdm_ldpc_last_ms", "ofdm_ldpc_coded_len_rate", "ofdm_ldpc_payload_len_rate",
    "ofdm_ldpc_decode_rel", "ofdm_ldpc_decode_soft_rel", "ofdm_rx_ldpc_decode_soft_rel",
    "ofdm_sig_word", "ofdm_sig_word_fields", "ofdm_sig_word_valid", "ofdm_sig_encode", "ofdm_sig_decode",
    "ofdm_sig_decode_soft", "ofdm_rx_sig_decode_soft", "ofdm_sig_last_ms",
)

_LIB = None
# OFDM_HIP_LIB selects another build of the same library (e.g. the -DSYNC_STAMPS diagnostic build)
LIB_PATH = os.environ.get("OFDM_HIP_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc",
                                                         "libofdm_hip.so")


def _declare(lib):
    vp, u8p, u32p, u64p = C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    H = C.c_void_p
    lib.ofdm_abi_version.restype = C.c_int
    lib.ofdm_device_count.restype = C.c_int
    lib.ofdm_create.argtypes = [C.POINTER(ofdm_cfg), C.POINTER(H)]
    lib.ofdm_destroy.argtypes = [H]
    lib.ofdm_destroy.restype = None
    lib.ofdm_last_error.argtypes = [H]
    lib.ofdm_last_error.restype = C.c_char_p
    lib.ofdm_set_stream.argtypes = [H, vp]
    lib.ofdm_set_tx_amplitude.argtypes = [H, C.c_float]
    lib.ofdm_set_carrier_map.argtypes = [H, C.c_char_p]
    lib.ofdm_set_channel.argtypes = [H, C.POINTER(ofdm_chan)]
    lib.ofdm_framed_len.argtypes = [H, C.c_uint32, u32p]
    lib.ofdm_make_packets.argtypes = [H, u8p, u64p, u32p, C.c_int, u8p, C.c_uint64, u64p]
    lib.ofdm_tx_frame_count.argtypes = [H, u32p, C.c_int, u64p, u64p]
    lib.ofdm_tx.argtypes = [H, u8p, u64p, u32p, C.c_int, vp, C.c_uint64, u64p, C.POINTER(ofdm_stats)]
    lib.ofdm_tx_async.argtypes = lib.ofdm_tx.argtypes
    lib.ofdm_wait.argtypes = [H]
    lib.ofdm_channel.argtypes = [H, vp, C.c_uint64, C.POINTER(ofdm_chan), C.c_uint64]
    lib.ofdm_rx.argtypes = [H, vp, C.c_uint64, u8p, C.c_uint64, u64p, u32p, C.POINTER(C.c_uint8),
                            C.c_int, C.POINTER(C.c_int), C.POINTER(ofdm_stats)]
    lib.ofdm_set_rx_iq_format.argtypes = [H, C.c_int, C.c_float]
    lib.ofdm_set_tx_iq_format.argtypes = [H, C.c_int, C.c_float]
    lib.ofdm_set_ddc.argtypes = [H, C.POINTER(ofdm_ddc_cfg)]
    lib.ofdm_ddc_reset.argtypes = [H, C.c_uint64]
    lib.ofdm_ddc_count.argtypes = [H, C.c_uint64, u64p]
    lib.ofdm_ddc.argtypes = [H, vp, C.c_uint64, vp, C.c_uint64, u64p]
    lib.ofdm_ddc_taps.argtypes = [H, vp, C.c_int, C.POINTER(C.c_int)]
    lib.ofdm_ddc_last_ms.argtypes = [H, C.POINTER(C.c_double)]
    lib.ofdm_set_ddc_bank.argtypes = [H, C.POINTER(ofdm_ddc_bank_cfg)]
    lib.ofdm_ddc_bank_reset.argtypes = [H, C.c_uint64]
    lib.ofdm_ddc_bank_count.argtypes = [H, C.c_uint64, u64p]
    lib.ofdm_ddc_bank.argtypes = [H, vp, C.c_uint64, vp, C.c_uint64, C.c_uint64, u64p]
    lib.ofdm_ddc_bank_taps.argtypes = [H, C.c_int, vp, C.c_int, C.POINTER(C.c_int)]
    lib.ofdm_ddc_bank_last_ms.argtypes = [H, C.POINTER(C.c_double)]
    lib.ofdm_set_pfb.argtypes = [H, C.POINTER(ofdm_pfb_cfg)]
    lib.ofdm_pfb_reset.argtypes = [H, C.c_uint64]
    lib.ofdm_pfb_count.argtypes = [H, C.c_uint64, u64p]
    lib.ofdm_pfb.argtypes = [H, vp, C.c_uint64, vp, C.c_uint64, C.c_uint64, u64p]
    lib.ofdm_pfb_last_ms.argtypes = [H, C.POINTER(C.c_double)]
    lib.ofdm_set_pfb_synth.argtypes = [H, C.POINTER(ofdm_pfb_synth_cfg)]
    lib.ofdm_pfb_synth_reset.argtypes = [H, C.c_uint64]
    lib.ofdm_pfb_synth.argtypes = [H, vp, C.c_uint64, C.c_uint64, vp, vp, C.c_uint64, u64p]
    lib.ofdm_pfb_synth_last_ms.argtypes = [H, C.POINTER(C.c_double)]
    lib.ofdm_set_resamp.argtypes = [H, C.POINTER(ofdm_resamp_cfg)]
    lib.ofdm_resamp_reset.argtypes = [H, C.c_uint64]
    lib.ofdm_resamp_count.argtypes = [H, C.c_uint64, u64p]
    lib.ofdm_resamp.argtypes = [H, vp, C.c_uint64, vp, C.c_uint64, u64p]
    lib.ofdm_resamp_taps.argtypes = [H, vp, C.c_int, C.POINTER(C.c_int)]
    lib.ofdm_resamp_last_ms.argtypes = [H, C.POINTER(C.c_double)]
    lib.ofdm_set_resamp_bank.argtypes = [H, C.POINTER(ofdm_resamp_bank_cfg)]
    lib.ofdm_resamp_bank_reset.argtypes = [H, C.c_uint64]
    lib.ofdm_resamp_bank_count.argtypes = [H, C.c_uint64, u64p]
    lib.ofdm_resamp_bank.argtypes = [H, vp, C.c_uint64, vp, C.c_uint64, C.c_uint64, u64p]
    lib.ofdm_resamp_bank_taps.argtypes = [H, C.c_int, vp, C.c_int, C.POINTER(C.c_int)]
    lib.ofdm_resamp_bank_last_ms.argtypes = [H, C.POINTER(C.c_double)]
    lib.ofdm_set_duc.argtypes = [H, C.POINTER(ofdm_duc_cfg)]
    lib.ofdm_duc_reset.argtypes = [H, C.c_uint64]
    lib.ofdm_duc.argtypes = [H, vp, C.c_uint64, vp, vp, C.c_uint64, u64p]
    lib.ofdm_duc_last_ms.argtypes = [H, C.POINTER(C.c_double)]
    lib.ofdm_set_duc_bank.argtypes = [H, C.POINTER(ofdm_duc_bank_cfg)]
    lib.ofdm_duc_bank_reset.argtypes = [H, C.c_uint64]
    lib.ofdm_duc_bank.argtypes = [H, vp, C.c_uint64, C.c_uint64, vp, vp, C.c_uint64, u64p]
    lib.ofdm_duc_bank_taps.argtypes = [H, C.c_int, vp, C.c_int, C.POINTER(C.c_int)]
    lib.ofdm_duc_bank_last_ms.argtypes = [H, C.POINTER(C.c_double)]
    lib.ofdm_set_tx_resamp.argtypes = [H, C.POINTER(ofdm_tx_resamp_cfg)]
    lib.ofdm_tx_resamp_reset.argtypes = [H, C.c_uint64]
    lib.ofdm_tx_resamp_count.argtypes = [H, C.c_uint64, u64p]
    lib.ofdm_tx_resamp.argtypes = [H, vp, C.c_uint64, vp, vp, C.c_uint64, u64p]
    lib.ofdm_tx_resamp_last_ms.argtypes = [H, C.POINTER(C.c_double)]
    lib.ofdm_set_tx_resamp_bank.argtypes = [H, C.POINTER(ofdm_tx_resamp_bank_cfg)]
    lib.ofdm_tx_resamp_bank_reset.argtypes = [H, C.c_uint64]
    lib.ofdm_tx_resamp_bank_count.argtypes = [H, C.c_uint64, u64p]
    lib.ofdm_tx_resamp_bank.argtypes = [H, vp, C.c_uint64, C.c_uint64, vp, vp, C.c_uint64, u64p]
    lib.ofdm_tx_resamp_bank_taps.argtypes = [H, C.c_int, vp, C.c_int, C.POINTER(C.c_int)]
    lib.ofdm_tx_resamp_bank_last_ms.argtypes = [H, C.POINTER(C.c_double)]
    lib.ofdm_set_multipath.argtypes = [H, C.POINTER(ofdm_multipath_cfg)]
    lib.ofdm_multipath_reset.argtypes = [H, C.c_uint64]
    lib.ofdm_multipath.argtypes = [H, vp, C.c_uint64, vp, vp, C.c_uint64, u64p]
    lib.ofdm_multipath_last_ms.argtypes = [H, C.POINTER(C.c_double)]
    lib.ofdm_set_cfr.argtypes = [H, C.POINTER(ofdm_cfr_cfg)]
    lib.ofdm_cfr_reset.argtypes = [H]
    lib.ofdm_cfr.argtypes = [H, vp, C.c_uint64, vp, C.c_uint64, u64p]
    lib.ofdm_cfr_stats.argtypes = [H, C.POINTER(ofdm_cfr_stats)]
    lib.ofdm_cfr_last_ms.argtypes = [H, C.POINTER(C.c_double)]
    lib.ofdm_set_psd.argtypes = [H, C.POINTER(ofdm_psd_cfg)]
    lib.ofdm_psd_reset.argtypes = [H]
    lib.ofdm_psd_count.argtypes = [H, C.c_uint64, u64p]
    lib.ofdm_psd.argtypes = [H, vp, C.c_uint64, vp, C.c_uint64, u64p]
    lib.ofdm_psd_read.argtypes = [H, vp, vp, u64p]
    lib.ofdm_psd_last_ms.argtypes = [H, C.POINTER(C.c_double)]
    lib.ofdm_set_mempoly.argtypes = [H, C.c_uint32, C.POINTER(ofdm_mempoly_cfg)]
    lib.ofdm_mempoly_reset.argtypes = [H, C.c_uint32]
    lib.ofdm_mempoly.argtypes = [H, C.c_uint32, vp, C.c_uint64, vp, C.c_uint64, u64p]
    lib.ofdm_mempoly_stats.argtypes = [H, C.c_uint32, C.POINTER(ofdm_mempoly_stats)]
    lib.ofdm_mempoly_last_ms.argtypes = [H, C.c_uint32, C.POINTER(C.c_double)]
    FC = C.POINTER(ofdm_fec_cfg)
    lib.ofdm_fec_coded_len.argtypes = [C.c_uint32, u32p]
    lib.ofdm_fec_payload_len.argtypes = [C.c_uint32, u32p]
    lib.ofdm_fec_encode.argtypes = [H, FC, u8p, u64p, u32p, C.c_int, u8p, C.c_uint64, u64p]
    lib.ofdm_fec_decode.argtypes = [H, FC, u8p, u64p, u32p, C.c_int, u8p, C.c_uint64, u64p, vp, u32p]
    lib.ofdm_fec_decode_soft.argtypes = lib.ofdm_fec_decode.argtypes
    lib.ofdm_fec_last_ms.argtypes = [H, C.POINTER(C.c_double)]
    lib.ofdm_fec_coded_len_rate.argtypes = [C.c_uint32, C.c_uint32, u32p]
    lib.ofdm_fec_payload_len_rate.argtypes = [C.c_uint32, C.c_uint32, u32p]
    lib.ofdm_fec_punct_last_ms.argtypes = [H, C.POINTER(C.c_double)]
    lib.ofdm_set_rx_soft.argtypes = [H, C.POINTER(ofdm_soft_cfg)]
    lib.ofdm_rx_soft.argtypes = [H, vp, C.c_uint64, u64p, C.POINTER(C.c_int)]
    lib.ofdm_rx_fec_decode_soft.argtypes = [H, FC, u8p, C.c_uint64, u64p, vp, u32p, C.c_int, C.POINTER(C.c_int)]
    lib.ofdm_rx_soft_last_ms.argtypes = [H, C.POINTER(C.c_double)]
    lib.ofdm_fec_decode_rel.argtypes = lib.ofdm_fec_decode.argtypes + [u8p, C.c_uint64]
    lib.ofdm_fec_decode_soft_rel.argtypes = lib.ofdm_fec_decode_rel.argtypes
    lib.ofdm_rx_fec_decode_soft_rel.argtypes = [H, FC, u8p, C.c_uint64, u64p, vp, u32p, u8p, C.c_uint64, C.c_int, C.POINTER(C.c_int)]
    lib.ofdm_rs_coded_len.argtypes = [C.c_uint32, u32p]
    lib.ofdm_rs_payload_len.argtypes = [C.c_uint32, u32p]
    lib.ofdm_rs_encode.argtypes = [H, u8p, u64p, u32p, C.c_int, u8p, C.c_uint64, u64p]
    lib.ofdm_rs_decode.argtypes = [H, u8p, u64p, u32p, C.c_int, u8p, C.c_uint64, u64p, vp, u32p, u32p]
    lib.ofdm_rs_last_ms.argtypes = [H, C.POINTER(C.c_double)]
    lib.ofdm_rs_decode_rel.argtypes = [H, C.POINTER(ofdm_rs_rel_cfg), u8p, u64p, u32p, C.c_int, u8p, u64p, u8p, C.c_uint64, u64p, vp, u32p,
                                       u32p, u32p]
    lib.ofdm_rs_rel_from_soft.argtypes = [H, vp, u64p, u32p, C.c_int, u8p, C.c_uint64, u64p]
    lib.ofdm_rs_rel_last_ms.argtypes = [H, C.POINTER(C.c_double)]
    LC = C.POINTER(ofdm_ldpc_cfg)
    lib.ofdm_ldpc_coded_len.argtypes = [C.c_uint32, u32p]
    lib.ofdm_ldpc_payload_len.argtypes = [C.c_uint32, u32p]
    lib.ofdm_ldpc_coded_len_rate.argtypes = [C.c_uint32, C.c_uint32, u32p]
    lib.ofdm_ldpc_payload_len_rate.argtypes = [C.c_uint32, C.c_uint32, u32p]
    lib.ofdm_ldpc_encode.argtypes = [H, LC, u8p, u64p, u32p, C.c_int, u8p, C.c_uint64, u64p]
    lib.ofdm_ldpc_decode.argtypes = [H, LC, u8p, u64p, u32p, C.c_int, u8p, C.c_uint64, u64p, vp, u32p, vp, u32p]
    lib.ofdm_ldpc_decode_soft.argtypes = lib.ofdm_ldpc_decode.argtypes
    lib.ofdm_rx_ldpc_decode_soft.argtypes = [H, LC, u8p, C.c_uint64, u64p, vp, u32p, vp, u32p, C.c_int, C.POINTER(C.c_int)]
    lib.ofdm_ldpc_last_ms.argtypes = [H, C.POINTER(C.c_double)]
    lib.ofdm_ldpc_decode_rel.argtypes = lib.ofdm_ldpc_decode.argtypes + [u8p, C.c_uint64]
    lib.ofdm_ldpc_decode_soft_rel.argtypes = lib.ofdm_ldpc_decode_rel.argtypes
    lib.ofdm_rx_ldpc_decode_soft_rel.argtypes = [H, LC, u8p, C.c_uint64, u64p, vp, u32p, vp, u32p, u8p, C.c_uint64, C.c_int,
                                                 C.POINTER(C.c_int)]
    u16p = C.POINTER(C.c_uint16)
    lib.ofdm_sig_word.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, u16p]
    lib.ofdm_sig_word_fields.argtypes = [C.c_uint32, u32p, u32p, u32p, u32p]
    lib.ofdm_sig_word_valid.argtypes = [C.c_uint32]
    lib.ofdm_sig_encode.argtypes = [H, u16p, u8p, u64p, u32p, C.c_int, u8p, C.c_uint64, u64p]
    lib.ofdm_sig_decode.argtypes = [H, u8p, u64p, u32p, C.c_int, u16p, u16p]
    lib.ofdm_sig_decode_soft.argtypes = lib.ofdm_sig_decode.argtypes
    lib.ofdm_rx_sig_decode_soft.argtypes = [H, u16p, u16p, C.c_int, C.POINTER(C.c_int)]
    lib.ofdm_sig_last_ms.argtypes = [H, C.POINTER(C.c_double)]
    lib.ofdm_set_taps.argtypes = [H, C.c_uint32]
    lib.ofdm_tap.argtypes = [H, C.c_int, vp, C.c_uint64, u64p]
    lib.ofdm_prof_enable.argtypes = [H, C.c_int]
    lib.ofdm_prof_reset.argtypes = [H]
    lib.ofdm_prof_get.argtypes = [H, C.c_int, C.POINTER(C.c_double), u64p]
    lib.ofdm_kernel_name.argtypes = [C.c_int]
    lib.ofdm_kernel_name.restype = C.c_char_p
    SC = C.POINTER(ofdm_sense_cfg)
    lib.ofdm_sense_count.argtypes = [SC, C.c_uint64, u64p, u64p]
    lib.ofdm_sense.argtypes = [H, SC, vp, C.c_uint64, vp, C.c_uint64, vp, vp, vp, C.c_uint64, u64p, u64p]
    lib.ofdm_sense_decide.argtypes = [H, SC, vp, C.c_uint64, vp, vp, vp, C.c_uint64, u64p]
    lib.ofdm_set_rx_sense.argtypes = [H, SC]
    lib.ofdm_rx_sense_result.argtypes = [H, vp, C.c_uint64, vp, vp, vp, C.c_uint64, u64p, u64p]
    lib.ofdm_rx_packet_pos.argtypes = [H, vp, C.c_int, C.POINTER(C.c_int)]
    lib.ofdm_rx_nco_state.argtypes = [H, vp, vp, vp, vp, C.c_int, C.POINTER(C.c_int)]
    lib.ofdm_rx_set_origin.argtypes = [H, C.c_uint64]
    lib.ofdm_rx_snr.argtypes = [H, C.POINTER(C.c_float)]
    lib.ofdm_set_rx_quality.argtypes = [H, C.c_int]
    lib.ofdm_rx_quality.argtypes = [H, vp, C.c_int, C.POINTER(C.c_int)]
    lib.ofdm_set_rx_csi.argtypes = [H, C.c_int]
    lib.ofdm_rx_csi.argtypes = [H, C.c_int, C.c_int, vp, vp, vp, vp, C.POINTER(C.c_int)]
    lib.ofdm_rx_csi_summary.argtypes = [H, C.c_int, u32p, vp, vp, vp, vp, vp]
    lib.ofdm_rx_submit.argtypes = [H, C.c_void_p, C.c_uint64]
    lib.ofdm_rx_set_flag_history.argtypes = [H, C.c_int, C.c_int, vp, vp, vp, C.c_int64, C.c_int64, C.c_uint64, C.c_double]
    lib.ofdm_sense_device_msgs.argtypes = [H, C.POINTER(C.c_void_p), u64p, u32p]
    lib.ofdm_sense_redecide.argtypes = [H, SC]
    for name in EXPORTS:
        fn = getattr(lib, name)
        if fn.restype is C.c_int and name not in ("ofdm_abi_version", "ofdm_device_count"):
            pass
    return lib


def _preload_hip_runtime():
    """One HIP runtime per process.  PyTorch-ROCm wheels bundle their own libamdhip64.so (SONAME
    libamdhip64.so.7, the name libofdm_hip.so needs).  If that copy is mapped first the dynamic linker
    hands it to us as well; if /opt/rocm's copy came first, a later ``import torch`` would map a SECOND
    runtime and find "No HIP GPUs".  So when torch is installed, map its runtime before ours --
    without importing torch."""
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.origin:
            return
        cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
        if os.path.exists(cand):
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
    except Exception:
        pass


def load():
    """Load libofdm_hip.so (once).  Raises ImportError if it is missing: the HIP
    engine IS the implementation, nothing falls back to the CPU."""
    global _LIB
    if _LIB is None:
        _preload_hip_runtime()
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "libofdm_hip.so not found at %s -- build it first (__graft_entry__.build() or "
                "`make -C ofdm_uhd_amd/csrc`); there is no CPU fallback" % LIB_PATH)
        lib = C.CDLL(LIB_PATH)
        ver = lib.ofdm_abi_version()
        if ver != OFDM_ABI_VERSION:
            raise ImportError("libofdm_hip.so ABI %d != expected %d" % (ver, OFDM_ABI_VERSION))
        _LIB = _declare(lib)
    return _LIB
