/*
 * ofdm_hip.h -- C ABI of libofdm_hip.so, the MI355X (gfx950) OFDM TX/RX engine.
 *
 * This is the drop-in boundary for the ofdm_mod / ofdm_demod hot path of
 * rubiruchi/ofdm_uhd.  The reference reaches its DSP through SWIG proxies of
 * GNU Radio 3.6 blocks (digital_swig.py); each entry point below names the
 * reference interface it replaces.  Plain C types only: pointers, sizes and
 * one POD configuration struct -- no torch / C++ types.
 *
 * Conventions
 *   - every function returns 0 (OFDM_OK) or a negative OFDM_E_* code; the
 *     message is available from ofdm_last_error().
 *   - bulk data pointers (payload bytes, IQ samples) are DEVICE pointers when
 *     the handle was created with OFDM_F_DEVICE_PTRS, host pointers otherwise.
 *     Small metadata arrays (offsets, lengths, flags, counters) are always
 *     HOST pointers.
 *   - a handle is single-owner (not thread-safe) and bound to one GPU and one
 *     HIP stream.  Calls return after the stream has drained unless stated.
 *   - IQ samples are interleaved float32 (I,Q) = gr_complex, the format of
 *     gr.file_sink(gr.sizeof_gr_complex, ...) (ofdm.py:124-131), unless the handle was
 *     switched to 16-bit IQ (ofdm_sc16: the wire format of a USRP and of most recorded
 *     captures) with ofdm_set_rx_iq_format / ofdm_set_tx_iq_format below.
 */
#ifndef OFDM_HIP_H
#define OFDM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 6 still: the 16-bit IQ entry points (ofdm_set_rx_iq_format / ofdm_set_tx_iq_format) are additions -- no struct,
 * prototype or default behaviour of version 6 changed, a caller built against it runs unchanged.  Consequence:
 * ofdm_abi_version() does not tell whether a library has the two setters; a caller that must run on older builds of
 * version 6 looks the symbols up (dlsym).  The same holds for the wideband front end (ofdm_set_ddc ... ofdm_ddc_last_ms). */
#define OFDM_ABI_VERSION 6

#define OFDM_MAX_FFT 4096
#define OFDM_MAX_CARRIER_HEX 1024 /* hex digits of a carrier map: OFDM_MAX_FFT / 4 */
#define OFDM_MAX_TAPS 512
#define OFDM_MAX_ARITY 256
#define OFDM_MASK_LEN 4096      /* len(random_mask_tuple), ofdm_packet_utils.py:195 */
#define OFDM_MAX_PKT_LEN 4096   /* MAX_PKT_LEN of digital_ofdm_frame_sink */

enum {
  OFDM_OK = 0,
  OFDM_E_INVAL = -1,     /* bad argument / configuration (std::invalid_argument in GR ctors) */
  OFDM_E_NOMEM = -2,
  OFDM_E_CAPACITY = -3,  /* caller-provided output buffer too small */
  OFDM_E_HIP = -4,       /* HIP runtime error */
  OFDM_E_OVERFLOW = -5   /* degenerate input exceeded an internal bound */
};

enum {
  OFDM_F_DEVICE_PTRS = 1u << 0, /* bulk pointers are device pointers */
  OFDM_F_PAD_FOR_USRP = 1u << 1 /* make_packet(pad_for_usrp=True), ofdm.py:45,144 */
};

typedef struct ofdm_c32 {
  float re, im;
} ofdm_c32;

/*
 * Everything ofdm_mod.__init__ / ofdm_demod.__init__ / ofdm_receiver.__init__
 * compute before building their flow graphs (ofdm.py:63-101,204-247,
 * ofdm_receiver.py~:69-98).  The Python host fills it; the engine copies it.
 */
typedef struct ofdm_cfg {
  uint32_t struct_size; /* sizeof(ofdm_cfg), ABI guard */
  int32_t device_id;    /* HIP device ordinal */
  uint32_t flags;       /* OFDM_F_* */

  uint32_t fft_length;     /* options.fft_length      (ofdm.py:64)  power of two, 64..4096 */
  uint32_t occupied_tones; /* options.occupied_tones  (ofdm.py:65)  */
  uint32_t cp_length;      /* options.cp_length       (ofdm.py:66)  */
  uint32_t arity;          /* len(rotated_const)      (ofdm.py:91-92) */

  ofdm_c32 constellation[OFDM_MAX_ARITY]; /* rotated_const (ofdm.py:98-101) */
  ofdm_c32 known_symbol[OFDM_MAX_FFT];    /* ksfreq, occupied_tones entries (ofdm.py:73-77) */

  float tx_amplitude; /* transmit_path._tx_amplitude after the [0,1] clamp (transmit_path.py:56-62) */

  float phase_gain;           /* ofdm_frame_sink phase_gain 0.25 (ofdm.py:238) */
  float freq_gain;            /* ofdm_frame_sink freq_gain  0.25*0.25/4 (ofdm.py:239) */
  float eq_gain;              /* digital_ofdm_frame_sink d_eq_gain 0.05 */
  uint32_t max_fft_shift_len; /* ofdm_frame_acquisition max_fft_shift_len 4 (digital_swig.py:4318-4328) */
  uint32_t sampler_timeout;   /* ofdm_sampler timeout 1000 (digital_swig.py:4719-4724) */

  float peak_rise;  /* gr_peak_detector_fb threshold_factor_rise 0.20 (ofdm_sync_pn) */
  float peak_fall;  /* gr_peak_detector_fb threshold_factor_fall 0.20 */
  float peak_alpha; /* gr_peak_detector_fb alpha 0.001; accepted range (0, 0.005]: above it the Q40 part of the
                     * detector's closed-form average can lose more than 1e-6 at a run start */

  uint32_t ntaps;             /* len(chan_coeffs), odd (ofdm_receiver.py~:71-75) */
  float taps[OFDM_MAX_TAPS];  /* gr.firdes.low_pass(1, 1, bw+tb, tb, WIN_HAMMING) as float32 */

  uint8_t whitening_mask[OFDM_MASK_LEN]; /* random_mask_tuple (ofdm_packet_utils.py:195-452) */
  uint32_t whitener_offset;              /* make_packet whitener_offset, 0..15 (ofdm_packet_utils.py:100) */

  uint64_t pad_seed; /* seed of the counter-based generator that replaces the mapper's rand()%arity fill */
  /* data-carrier map as a hex string, NUL terminated; "" = the mapper's built-in "FE7F"
   * (transmit_path.py:64).  Used identically by the mapper (container fft_length) and the
   * frame sink (container occupied_tones); see ofdm_set_carrier_map. */
  char carrier_map[OFDM_MAX_CARRIER_HEX + 8];

  /* ofdm_receiver's SYNC selector (ofdm_receiver.py~:89-119).  OFDM_SYNC_PN is the reference's hard-wired choice;
   * OFDM_SYNC_FIXED is its "for testing only" branch (:108-119): chan_filt = multiply_const(1.0), a timing flag on
   * the last sample of every fixed_nsymbols-th symbol starting with the first (ofdm_sync_fixed), a constant
   * frequency-offset input to the NCO.  ("ml" and "pnac" need blocks the reference's tree does not hold.) */
  uint32_t sync_mode;
  uint32_t fixed_nsymbols;   /* symbols per packet incl. the preamble (reference: 18) */
  float fixed_freq_offset;   /* reference: 0.0 */
  uint32_t reserved0;
} ofdm_cfg;
enum { OFDM_SYNC_PN = 0, OFDM_SYNC_FIXED = 1 };

/* Synthetic channel fused into the TX store (replaces the UHD sink/source pair
 * usrp_transmit_path.py:66-72 / usrp_receive_path.py:67-73 for loopback). */
typedef struct ofdm_chan {
  float sigma;             /* AWGN: y = x + sigma*(g1 + j g2)/sqrt(2), g ~ N(0,1) */
  float cfo;               /* carrier offset, radians per sample: x[n] *= exp(j*cfo*n) */
  uint64_t seed;           /* Philox-2x32-7: counter = sample index / 2, key = hash(seed, stream_id) */
  uint64_t stream_id;      /* independent noise per stream */
  uint64_t lead_samples;   /* noise-only samples before the first packet */
  uint64_t tail_samples;   /* noise-only samples after the last packet  */
} ofdm_chan;

/* per-call counters; the cross-GPU reduce sums these */
typedef struct ofdm_stats {
  uint64_t symbols;          /* OFDM symbols processed (TX: emitted incl. preambles; RX: demodulated + preambles) */
  uint64_t samples;          /* IQ samples produced / consumed */
  uint64_t peaks;            /* timing flags raised by the peak detector */
  uint64_t frames;           /* preambles accepted by the sampler */
  uint64_t headers_ok;       /* frames whose 2x16-bit header halves matched */
  uint64_t packets;          /* messages the frame sink posted */
  uint64_t crc_ok;           /* packets whose CRC-32 checked */
  uint64_t chained_frames;   /* frames consumed as payload of an earlier unfinished packet */
  uint64_t overflow;         /* non-zero: an internal bound was hit, result incomplete */
} ofdm_stats;

typedef struct ofdm_handle ofdm_handle;

/* --- lifecycle ---------------------------------------------------------- */
int ofdm_abi_version(void);
int ofdm_device_count(void);
/* replaces ofdm_mod.__init__/ofdm_demod.__init__ graph construction (ofdm.py:45-131,186-261) */
int ofdm_create(const ofdm_cfg *cfg, ofdm_handle **out);
void ofdm_destroy(ofdm_handle *h);
const char *ofdm_last_error(const ofdm_handle *h); /* h may be NULL: error of the last failed ofdm_create */
/* run on a caller-owned hipStream_t (e.g. torch's current stream); NULL restores the handle's own stream */
int ofdm_set_stream(ofdm_handle *h, void *hip_stream);
/* transmit_path.set_tx_amplitude (transmit_path.py:56-62); clamps to [0,1] */
int ofdm_set_tx_amplitude(ofdm_handle *h, float ampl);
/* digital_ofdm_mapper_bcv::reset_carrier_map of the reference's patched GNU Radio
 * (transmit_path.py:64-70; the call is commented out at :67, so the stock behaviour is
 * never to change it): rebuilds the mapper's and the frame sink's subcarrier tables from a
 * hex string such as the one hex_conv returns (clipped to occupied_tones/4 digits,
 * sensing_and_tramsmitting.py:470).  NULL or "" restores "FE7F".  OFDM_E_INVAL when the
 * string holds a non-hex digit or allocates more carriers than occupied_tones (the
 * blocks' std::invalid_argument); the previous map then stays in force. */
int ofdm_set_carrier_map(ofdm_handle *h, const char *hex);
/* --- 16-bit IQ at the engine boundary -------------------------------------------------------------------------------
 * Per handle and per direction; OFDM_IQ_FC32 (interleaved float32) is the default and runs exactly what it always ran.
 * With OFDM_IQ_SC16 the `iq` / `iq_out` argument of the calls named below points to ofdm_sc16 (cast it; 4-byte aligned)
 * and nsamples / iq_cap keep counting samples; host or device pointers as the handle was created.
 *   receive   x.re = (float)i.re * scale, same for im: one float32 multiply, int16 -> float32 is exact.  Default
 *             scale 2^-15.  The channel filter, the sensor and (SYNC "fixed") a small expand kernel convert as they
 *             load: the receiver computes bit for bit what it computes from the expanded float array.
 *   transmit  q = clamp(rintf(x * scale), -32768, 32767) per part: one float32 multiply, round half to even, NaN -> 0,
 *             clamped in float before the integer conversion.  Default scale 2^15.  Quantised at the store, after
 *             amplitude and the fused channel (noise and carrier offset are applied in float), the noise-only lead-in
 *             and tail included.
 * Any finite scale > 0 is accepted (a driver's own convention, e.g. 32767); scale is ignored with OFDM_IQ_FC32.  The
 * two defaults are exact powers of two: an sc16 TX -> RX loop returns the quantised grid exactly.
 * OFDM_E_INVAL: unknown format; scale not finite and positive; a change of the receive format while an ofdm_rx_submit
 * is pending; sc16 receive together with the opt-in fused front end (OFDM_FRONT=1, float only).  The calls that take
 * samples return OFDM_E_INVAL for an ofdm_sc16 pointer that is not 4-byte aligned (a sample is moved as one dword).
 * What stays float32: ofdm_channel (in place on a float buffer), every debug tap, the --log probe files. */
typedef struct ofdm_sc16 {
  int16_t re, im;
} ofdm_sc16;
enum { OFDM_IQ_FC32 = 0, OFDM_IQ_SC16 = 1 };
int ofdm_set_rx_iq_format(ofdm_handle *h, int format, float scale); /* ofdm_rx, ofdm_rx_submit, ofdm_sense, fused sensing */
int ofdm_set_tx_iq_format(ofdm_handle *h, int format, float scale); /* ofdm_tx, ofdm_tx_async */
/* channel applied inside ofdm_tx; NULL disables it */
int ofdm_set_channel(ofdm_handle *h, const ofdm_chan *chan);

/* --- packet framing ------------------------------------------------------
 * Batched make_packet / unmake_packet (ofdm_packet_utils.py:99-143,169-191)
 * incl. digital_crc32 (digital_swig.py:3151-3169).  Framed packet k occupies
 * framed[framed_off[k] .. +payload_len[k]+9 (+USRP pad)].                  */
int ofdm_framed_len(const ofdm_handle *h, uint32_t payload_len, uint32_t *framed_len);
int ofdm_make_packets(ofdm_handle *h, const uint8_t *payloads, const uint64_t *payload_off,
                      const uint32_t *payload_len, int npkt, uint8_t *framed, uint64_t framed_cap,
                      uint64_t *framed_off /* npkt+1, host, out */);

/* --- transmit: ofdm_mod.send_pkt ... multiply_const (ofdm.py:106-118,133-148;
 *     transmit_path.py:47-54) ------------------------------------------------
 * payload bytes in -> make_packet -> ofdm_mapper_bcv -> ofdm_insert_preamble
 * -> fft_vcc(inverse, shift) -> ofdm_cyclic_prefixer -> 1/sqrt(N) -> amp
 * [-> channel].  Packet k starts at sample lead + sym_off[k]*(N+CP).         */
int ofdm_tx_frame_count(const ofdm_handle *h, const uint32_t *payload_len, int npkt,
                        uint64_t *nsymbols, uint64_t *nsamples /* incl. channel lead/tail */);
int ofdm_tx(ofdm_handle *h, const uint8_t *payloads, const uint64_t *payload_off,
            const uint32_t *payload_len, int npkt, ofdm_c32 *iq_out, uint64_t iq_cap,
            uint64_t *nsamples, ofdm_stats *stats /* may be NULL */);

/* the same, returning as soon as the work is queued on the handle's stream: the samples are complete after
 * ofdm_wait() -- or for whatever the caller queues behind them on that stream, e.g. ofdm_rx() on the same
 * handle reading iq_out (device-pointer mode: a TX -> RX loopback then has no host round trip in between).
 * The host metadata arrays may be reused at once; in host-pointer mode iq_out must not be read before ofdm_wait.
 * One asynchronous call may be outstanding per handle: ofdm_wait (or any synchronous call on the handle, all
 * of which end with a stream synchronisation) must come before the next ofdm_tx_async. */
int ofdm_tx_async(ofdm_handle *h, const uint8_t *payloads, const uint64_t *payload_off,
                  const uint32_t *payload_len, int npkt, ofdm_c32 *iq_out, uint64_t iq_cap,
                  uint64_t *nsamples, ofdm_stats *stats /* may be NULL */);
int ofdm_wait(ofdm_handle *h);

/* standalone channel on an existing IQ buffer (same generator as the fused one;
 * sample n of the buffer is stream sample index0+n).  Always float32, whatever the handle's IQ formats. */
int ofdm_channel(ofdm_handle *h, ofdm_c32 *iq, uint64_t n, const ofdm_chan *chan, uint64_t index0);

/* --- receive: ofdm_demod (ofdm.py:221-261) = ofdm_receiver (ofdm_receiver.py~:131-142)
 *     + ofdm_frame_sink + _queue_watcher_thread/unmake_packet (ofdm.py:300-305) ---
 * One contiguous IQ stream in; for every message the frame sink would post,
 * in stream order: payload bytes (CRC stripped), length, CRC verdict.  These
 * are exactly the (ok, payload) pairs the reference hands to its callback.  */
int ofdm_rx(ofdm_handle *h, const ofdm_c32 *iq, uint64_t nsamples, uint8_t *payload_out,
            uint64_t payload_cap, uint64_t *payload_off /* max_pkts+1, host */,
            uint32_t *payload_len /* max_pkts, host */, uint8_t *crc_ok /* max_pkts, host */,
            int max_pkts, int *npkt, ofdm_stats *stats /* may be NULL */);

/* digital_ofdm_frame_acquisition::snr() (digital_swig.py:4231-4239, "Return an estimate of the SNR of the channel").
 * In GNU Radio 3.6.0 the block initialises d_snr_est to 0 in its constructor and no code path ever updates it
 * [GR-3.6.0, recalled; the reference never calls it]: the accessor returns that constant, and so does this. */
int ofdm_rx_snr(const ofdm_handle *h, float *snr_est); /* still the stub: per-packet figures come from ofdm_rx_quality */

/* --- link quality: per-packet SNR, EVM and carrier offset (no reference counterpart) -----------------------------
 * Off by default; ofdm_set_rx_quality(h, 1) holds for the following ofdm_rx calls.  A call with it on runs the
 * demodulator's instrumented kernel and one gather kernel more; a call with it off runs exactly what it ran before.
 * Definitions (occ = occupied_tones, zl = (N - occ) / 2, ks = the known preamble symbol over the occupied block):
 *   pilot / null bins  occupied index i in [0, occ) is read at Ysh[i + zl + coarse] of the packet's own preamble
 *                      (FFT output, DC in the middle; 0 outside [0, N), as frame acquisition reads it): a pilot bin
 *                      where ks[i] != 0, a null bin where ks[i] == 0 (every odd absolute bin).  The means divide by
 *                      the two bin counts.
 *   decision energies  every carrier the frame sink demapped for the packet (header symbols included, and a later
 *                      preamble the packet's chain consumed as data): the rows of OFDM_TAP_RX_SINK.  sigrot is the
 *                      slicer's input, decision the constellation point it picked.
 *   cfo_bins           coarse + fine, fine = -step * N / (2 pi) with step the NCO's per-sample phase step at the
 *                      packet's flag (SYNC "fixed": the one fixed_freq_offset gives).  Same sign as
 *                      ofdm_chan.cfo * N / (2 pi).
 * Sums are per-thread sequential, then the demodulator's fixed reduction tree: the records are bit-reproducible. */
typedef struct ofdm_pkt_quality {
  uint64_t flag;          /* flag sample of the packet's preamble (= its ofdm_rx_packet_pos entry)             */
  uint32_t first_symbol;  /* ordinal of that preamble among the call's sampled symbols (row of TAP_RX_FFT)     */
  uint32_t nsym;          /* symbols the frame sink demapped for this packet (rows of TAP_RX_SINK)             */
  uint32_t ncarriers;     /* carriers demapped = nsym * (data carriers of the sink's map)                      */
  int32_t coarse;         /* frame acquisition's integer bin shift                                             */
  float cfo_bins;         /* carrier offset estimate, subcarrier spacings                                      */
  float pilot_power;      /* mean |Y|^2 over the preamble's known (non-zero) carriers, FFT-output units        */
  float null_power;       /* mean |Y|^2 over its zeroed carriers inside the occupied band                      */
  float err_energy;       /* sum over demapped carriers of |sigrot - decision|^2                               */
  float ref_energy;       /* sum over demapped carriers of |decision|^2                                        */
  float snr_preamble_db;  /* 10 log10(max(pilot_power / null_power - 1, 1e-6))                                 */
  float snr_decision_db;  /* 10 log10(ref_energy / max(err_energy, 1e-30)) = -20 log10(EVM_rms)                */
} ofdm_pkt_quality;

int ofdm_set_rx_quality(ofdm_handle *h, int enable); /* off by default; holds for the following ofdm_rx calls */
/* one record per packet of the last ofdm_rx, in the order of its payloads (CRC failures included); out == NULL:
 * size query.  OFDM_E_INVAL if the last call ran without link quality; OFDM_E_CAPACITY (with *n set) if cap < *n. */
int ofdm_rx_quality(ofdm_handle *h, ofdm_pkt_quality *out, int cap, int *n);

/* --- per-subcarrier channel state (CSI) per packet, and its per-carrier summary (no reference counterpart) ---------
 * Off by default; ofdm_set_rx_csi(h, 1) holds for the following ofdm_rx calls.  A call with it on runs the
 * demodulator's CSI instantiation and one gather kernel more; a call with it off runs exactly what it ran before.
 * Independent of link quality.  Notation: occ = occupied_tones, zl = (N - occ + 1) / 2, coarse = frame acquisition's
 * integer bin shift for the packet's preamble, Y[i] = Ysh[i + zl + coarse] of that preamble (FFT output, DC in the
 * middle; 0 outside [0, N)), read exactly where the equaliser and the link-quality sums read it.  Pilot bin: ks[i] != 0;
 * null bin: ks[i] == 0, every odd absolute bin.
 * Per delivered packet (CRC failures included), one row per array, occ entries each, in payload order:
 *   eq         hinv[i] of the packet's OWN preamble, bit for bit what the demodulator multiplies with:
 *              ks[i] / (comp Y[i]) at even i, the mean of the two neighbours at interior odd i, a copy of occ-2 at occ-1
 *              when occ is even (the equaliser works on occupied-index parity, not on ks).  A later preamble the
 *              packet's chain consumes as data re-estimates hinv; the row keeps the first one.  Non-finite values are
 *              stored as computed.
 *   pre_power  |Y[i]|^2 of the packet's own preamble
 *   err        sum over the symbols the frame sink demapped for the packet (those link quality counts), in symbol
 *              order, of |sigrot - decision|^2 on the carrier whose sink-map entry is i (smap[c] == i); 0 where i is
 *              not in the sink's map
 *   ref        the same sum of |decision|^2
 * One thread owns each carrier for the whole chain: every entry is a sequential float32 sum, bit-reproducible.
 * Summary over the last call's packets (all, or the CRC-ok ones), per carrier, float64: npkt, sum pre_power, sum err,
 * sum ref, and sum |1/eq|^2 over the finite non-zero eq with the count of those entries.  Summation order is fixed
 * (chunks of consecutive packets, then the chunks in order; no float atomics): repeated calls give the same bits.
 * Derived report (host side, ofdm_uhd_amd/csi.py):
 *   P[i] = sum pre_power[i] / npkt
 *   Nh[i] = P[i] at a null bin; at a pilot bin the mean of P at the nearest null bin on each side (one at the edge)
 *   Sh[i] = max(P[i] - Nh[i], 0) at a pilot bin; at a null bin the mean of Sh at the neighbouring pilot bins
 *   snr_preamble_db[i] = 10 log10(max(Sh / Nh, 1e-6))   (every occupied carrier, used by the current map or not)
 *   snr_decision_db[i] = 10 log10(sum ref / max(sum err, 1e-30))   (NaN outside the sink's map)
 *   gain_db[i] = 10 log10(mean |1/eq|^2)
 * Rows take about 20 occ bytes of device memory per frame and per packet, allocated only while CSI is on. */
int ofdm_set_rx_csi(ofdm_handle *h, int enable); /* off by default; holds for the following ofdm_rx calls */
/* rows [first, first+count) of the last call's packets, HOST memory, any array may be NULL; *n = packets of that
 * call (count == 0: size query).  OFDM_E_INVAL if that call ran without CSI or first+count > *n. */
int ofdm_rx_csi(ofdm_handle *h, int first, int count, ofdm_c32 *eq, float *pre_power, float *err, float *ref, int *n);
/* per-carrier float64 sums of the definitions above, each array occ entries, HOST memory (any may be NULL) */
int ofdm_rx_csi_summary(ofdm_handle *h, int crc_ok_only, uint32_t *npkt, double *pre_power, double *err, double *ref,
                        double *inv_gain, uint32_t *ninv);

/* --- spectrum sensing: the `sensor` flowgraph + sense_loop + hex_conv
 *     (predictive_sense.py:72-123,150-268; same code in sensing_and_tramsmitting*.py) ---
 * stream_to_vector(fft_size) -> fft_vcc(fft_size, True, window) -> complex_to_mag_squared
 * -> bin_statistics_f(fft_size, msgq, tune, tune_delay, dwell_delay): after every retune
 * tune_delay vectors are discarded, then the per-bin MAX over dwell_delay vectors is
 * posted as one message (float32[fft_size], FFT order).  sense_loop then sums avg_msgs
 * messages in float64 (:168-172), consumes skip_msgs more without using them (the message
 * that reaches the else branch, :174), divides by avg_msgs (:175-176), thresholds
 * (bit = 0 if mean > threshold else 1, :179), swaps the halves into ascending-frequency
 * order (:193-205) and packs nibbles LSB-first into upper-case hex (hex_conv :235-268). */
#define OFDM_SENSE_MAX_FFT 4096
typedef struct ofdm_sense_cfg {
  uint32_t struct_size;    /* = sizeof(ofdm_sense_cfg) */
  uint32_t fft_size;       /* power of two, 64..4096 (-s/--fft-size, default 256) */
  uint32_t tune_delay;     /* vectors dropped per message period (>= 0)           */
  uint32_t dwell_delay;    /* vectors max-held per message (>= 1)                 */
  uint32_t avg_msgs;       /* messages averaged per decision (10)                 */
  uint32_t skip_msgs;      /* messages consumed unused per decision (1)           */
  double threshold;        /* 1e-4 (:179); 1e-3 / 0.2 in the secondary_tx variants */
  float window[OFDM_SENSE_MAX_FFT]; /* fft_vcc window taps (window.blackmanharris) */
} ofdm_sense_cfg;

/* how many messages / decisions a stream of nsamples yields */
int ofdm_sense_count(const ofdm_sense_cfg *sc, uint64_t nsamples, uint64_t *nmsgs, uint64_t *ndecisions);
/* iq follows OFDM_F_DEVICE_PTRS; every output is HOST memory and may be NULL:
 * msgs[nmsgs][fft_size] (bin_statistics_f message bodies, FFT order), then per decision
 * mean_inorder[fft_size] (float64, ascending frequency), bits_inorder[fft_size] (0/1),
 * hex[fft_size/4] (no terminator). */
int ofdm_sense(ofdm_handle *h, const ofdm_sense_cfg *sc, const ofdm_c32 *iq, uint64_t nsamples,
               float *msgs, uint64_t msgs_cap /* messages */, double *mean_inorder, uint8_t *bits_inorder,
               char *hex, uint64_t dec_cap /* decisions */, uint64_t *nmsgs, uint64_t *ndecisions);
/* sense_loop alone (:150-222) over ready-made message bodies msgs[nmsgs][fft_size]
 * (HOST memory, e.g. drained from a real gr.msg_queue): same three decision outputs. */
int ofdm_sense_decide(ofdm_handle *h, const ofdm_sense_cfg *sc, const float *msgs, uint64_t nmsgs,
                      double *mean_inorder, uint8_t *bits_inorder, char *hex, uint64_t dec_cap,
                      uint64_t *ndecisions);
/* fuse the sensor into ofdm_rx (BASELINE config 5): while set, every ofdm_rx call also
 * runs the sensing kernels over the same IQ buffer on a second stream, overlapped with
 * the receiver; fetch the outcome of the last call with ofdm_rx_sense_result (same
 * outputs as ofdm_sense).  sc == NULL switches it off. */
int ofdm_set_rx_sense(ofdm_handle *h, const ofdm_sense_cfg *sc);
int ofdm_rx_sense_result(ofdm_handle *h, float *msgs, uint64_t msgs_cap, double *mean_inorder,
                         uint8_t *bits_inorder, char *hex, uint64_t dec_cap, uint64_t *nmsgs,
                         uint64_t *ndecisions);
/* cooperative sensing across GPUs (BASELINE config 5): the DEVICE address of the message
 * bodies of the last run, float32[nmsgs][fft_size], so that the caller can max-reduce them
 * in place over RCCL (ncclMax; powers are >= 0) ... */
int ofdm_sense_device_msgs(ofdm_handle *h, void **d_msgs, uint64_t *nmsgs, uint32_t *fft_size);
/* ... and re-take the decisions (mean / bits / hex) from the reduced bodies; read them with
 * ofdm_rx_sense_result.  Both calls order themselves after the sensing kernels. */
int ofdm_sense_redecide(ofdm_handle *h, const ofdm_sense_cfg *sc);

/* --- wideband receive: tune and decimate ahead of ofdm_rx (DDC) -------------------------------------------------------
 * Replaces what the reference leaves to its radio (usrp2.source_32fc.set_decim / set_center_freq,
 * usrp_receive_path.py) for captures taken wider than the modem's rate, with several links sharing the band: GNU Radio's
 * gr.freq_xlating_fir_filter_ccf(decimation, taps, center_freq, sampling_freq) with integer-turn phase bookkeeping, so
 * that any chunking of the stream gives the same bits.  A standalone, stateful stage: ofdm_rx and every other entry
 * point run exactly what they ran; with no DDC configured nothing here launches, allocates or copies.
 *   input     wideband samples x[n], n an absolute index counted from the last reset (ofdm_set_ddc, ofdm_ddc_reset);
 *             samples before that reset's first index are zero.  Format: the handle's receive IQ format and scale
 *             (ofdm_set_rx_iq_format), converted as the channel filter converts (one float32 multiply per part).
 *   table     c[k] = complex64(h[k] exp(j 2 pi fc k)), k in [0, ntaps): float64 on the host, rounded once;
 *             ofdm_ddc_taps returns exactly what the kernel multiplies with.
 *   output    m exists for every m >= 0 with m R <= the last input index seen:
 *               v[m] = sum_k c[k] x[m R - k]     float32; the order of the additions is a function of k alone
 *               y[m] = v[m] r[m]                 r[m] = complex64(expj(-2 pi Phi_m / 2^64)), Phi_m = m D mod 2^64,
 *             D = frac(fc R) 2^64 truncated to an integer, 0 where frac rounds up to 1 (the integer-turn convention of the receiver's NCO); expj is
 *             the engine's bit-reproducible float64 evaluation, not the hardware's sin / cos.
 *   state     the last ntaps - 1 converted samples and the absolute index of the next input sample.  A call with
 *             input indices [a, a + n) produces the outputs m with a <= m R < a + n -- possibly none.  A stream fed in
 *             any segmentation gives bit-identical outputs.
 * Pointers are host or device as the handle was created; in device mode iq_out can be handed straight to ofdm_rx /
 * ofdm_rx_submit on the same handle (same stream, no host round trip).  ofdm_ddc returns after the stream drained.
 * OFDM_E_INVAL: bad struct_size, decimation, ntaps, a non-finite tap, |center_freq| > 0.5; ofdm_ddc / ofdm_ddc_reset /
 * ofdm_ddc_count / ofdm_ddc_taps without a configuration; an ofdm_sc16 pointer not 4-byte (float32: 8-byte) aligned.
 * Also OFDM_E_INVAL: a first_sample_index above 2^62, or a call that would take the stream's sample index past 2^63
 * (indices and phases are computed in 64-bit integers that must not wrap).
 * OFDM_E_CAPACITY: out_cap smaller than ofdm_ddc_count says (*nout is set); the stream state is then unchanged. */
#define OFDM_DDC_MAX_TAPS 1024
typedef struct ofdm_ddc_cfg {
  uint32_t struct_size; /* = sizeof(ofdm_ddc_cfg) */
  uint32_t decimation;  /* R, 1..64, any integer (set_decim) */
  uint32_t ntaps;       /* 1..OFDM_DDC_MAX_TAPS */
  uint32_t reserved;
  double center_freq;   /* fc, cycles per INPUT sample, [-0.5, 0.5] (set_center_freq / sampling_freq) */
  float taps[OFDM_DDC_MAX_TAPS]; /* real low-pass prototype at the input rate (gr.firdes.low_pass) */
} ofdm_ddc_cfg;
/* gr.freq_xlating_fir_filter_ccf ctor = usrp2.source_32fc.set_decim + set_center_freq; NULL: none.  Resets the stream
 * state (history zero, next input index 0). */
int ofdm_set_ddc(ofdm_handle *h, const ofdm_ddc_cfg *cfg);
/* a new stream whose first sample has this absolute index (a retune / a gap in the capture): history zero */
int ofdm_ddc_reset(ofdm_handle *h, uint64_t first_sample_index);
/* outputs the NEXT ofdm_ddc call of nin samples produces, from the current state (gr_sync_decimator's fixed ratio,
 * exact for any R and any start) */
int ofdm_ddc_count(const ofdm_handle *h, uint64_t nin, uint64_t *nout);
/* gr.freq_xlating_fir_filter_ccf::work on the next nin samples of the stream */
int ofdm_ddc(ofdm_handle *h, const void *iq_in, uint64_t nin, ofdm_c32 *iq_out, uint64_t out_cap, uint64_t *nout);
/* freq_xlating_fir_filter_ccf's internal band-pass taps: the table the kernel multiplies with (out NULL: size query) */
int ofdm_ddc_taps(const ofdm_handle *h, ofdm_c32 *out, int cap, int *n);
/* HIP-event time of k_ddc in the last ofdm_ddc, which must have run with profiling on (ofdm_prof_enable) and produced
 * output; OFDM_E_INVAL otherwise.  Separate from ofdm_prof_get: the OFDM_K_* table is unchanged. */
int ofdm_ddc_last_ms(const ofdm_handle *h, double *ms);

/* --- wideband receive: every link of a capture in one pass (DDC bank) -------------------------------------------------
 * The receive-side counterpart of adding several links onto one band (ofdm_duc with `add`): one decimation R, one real
 * prototype h[0..ntaps) and K centre frequencies give K narrowband streams from ONE pass over the wideband stream,
 * where K calls of ofdm_ddc read and stage the capture K times (dual_channel/dual_channel.py tunes one radio channel
 * per link).  Additions only: OFDM_ABI_VERSION stays 6 and the OFDM_K_* table is unchanged.
 * Definition.  Link i of the bank is the DDC above with (decimation = R, taps = h, center_freq = fc[i]), bit for bit:
 *   table     c_i[k] = complex64(h[k] exp(j 2 pi fc_i k)), float64 on the host, rounded once (ofdm_ddc_bank_taps);
 *   phase     D_i = frac(fc_i R) 2^64 truncated, 0 where frac rounds up to 1;
 *   input     the handle's receive IQ format and scale, converted as the DDC converts;
 *   output    of a call with input indices [a, a + n): every m with a <= m R < a + n, the same set for every link;
 *   additions tap k = q R + p belongs to chain q mod NG (NG = 1 for R <= 4, 4 otherwise); a chain adds its taps in
 *             ascending k into A += c.re * (x.re, x.im), B += c.im * (x.re, x.im), packed fused multiply-adds begun at
 *             +0; the chains are added in ascending order; v = (A.re - B.im, A.im + B.re);
 *   rotation  y[m] = v[m] r_i[m], the unfused complex product, r_i[m] = complex64(expj(-2 pi (m D_i mod 2^64) / 2^64)).
 * Nothing depends on where a call, a chunk or a tile starts, on K, or on a link's position in the list: link i's
 * stream equals what ofdm_ddc gives for fc_i, under any segmentation.  Equal frequencies are allowed and give equal
 * outputs.
 *   state     the last ntaps - 1 converted samples and the absolute index of the next input sample, shared by all
 *             links and separate from the single DDC's: a handle may have both configured, neither disturbs the other.
 * Pointers are host or device as the handle was created; ordering behind an ofdm_tx_async in flight and the alignment
 * rules are ofdm_ddc's.  Link i's outputs go to the contiguous run iq_out + i * link_stride (samples); out_cap and
 * *nout count outputs PER LINK.  With no bank configured nothing here launches, allocates or copies.
 * OFDM_E_INVAL: as for the DDC (bad struct_size, decimation, ntaps, a non-finite tap, a call without a configuration,
 * misaligned input, first_sample_index above 2^62, a sample index past 2^63), and: nlinks 0 or above
 * OFDM_DDC_BANK_MAX_LINKS, any |center_freq[i]| > 0.5 or NaN, link >= nlinks, link_stride < *nout with nlinks > 1.  A
 * refused configuration leaves the one in force (or none) as it was.
 * OFDM_E_CAPACITY: out_cap smaller than ofdm_ddc_bank_count says (*nout is set); the stream state is then unchanged. */
#define OFDM_DDC_BANK_MAX_LINKS 8
typedef struct ofdm_ddc_bank_cfg {
  uint32_t struct_size; /* = sizeof(ofdm_ddc_bank_cfg) */
  uint32_t decimation;  /* R, 1..64, shared by the links */
  uint32_t ntaps;       /* 1..OFDM_DDC_MAX_TAPS */
  uint32_t nlinks;      /* K, 1..OFDM_DDC_BANK_MAX_LINKS */
  double center_freq[OFDM_DDC_BANK_MAX_LINKS]; /* fc[i], cycles per INPUT sample, [-0.5, 0.5]; the first nlinks count */
  float taps[OFDM_DDC_MAX_TAPS];               /* real low-pass prototype at the input rate, shared by the links */
} ofdm_ddc_bank_cfg;
/* K freq_xlating_fir_filter_ccf ctors on one stream; NULL: none.  Resets the bank's stream state. */
int ofdm_set_ddc_bank(ofdm_handle *h, const ofdm_ddc_bank_cfg *cfg);
/* a new stream whose first sample has this absolute index: history zero */
int ofdm_ddc_bank_reset(ofdm_handle *h, uint64_t first_sample_index);
/* outputs PER LINK the next ofdm_ddc_bank call of nin samples produces, from the current state */
int ofdm_ddc_bank_count(const ofdm_handle *h, uint64_t nin, uint64_t *nout);
/* the next nin samples of the stream through every link: link i at iq_out + i * link_stride, out_cap per link */
int ofdm_ddc_bank(ofdm_handle *h, const void *iq_in, uint64_t nin, ofdm_c32 *iq_out, uint64_t link_stride, uint64_t out_cap,
                  uint64_t *nout);
/* the table of one link as the kernel multiplies with it (out NULL: size query) */
int ofdm_ddc_bank_taps(const ofdm_handle *h, int link, ofdm_c32 *out, int cap, int *n);
/* HIP-event time of k_ddc_bank in the last ofdm_ddc_bank, which must have run with profiling on and produced output;
 * OFDM_E_INVAL otherwise. */
int ofdm_ddc_bank_last_ms(const ofdm_handle *h, double *ms);

/* --- wideband receive: polyphase-FFT channeliser for links on the k/M grid --------------------------------------------
 * Where the links of a capture sit on a uniform grid (dual_channel/dual_channel.py tunes one radio channel per link;
 * the sensing apps step through every slot of a band), link c at centre frequency c/M with decimation M, the DDC's
 * rotation is exactly 1 and the bank's K filters collapse into ONE real-tap polyphase filter followed by an M-point
 * transform per output index: all M channels for 2 ntaps multiply-adds plus O(M log M), and up to 64 of them.  A
 * standalone, stateful stage; additions only: OFDM_ABI_VERSION stays 6, the OFDM_K_* table is unchanged, and with no
 * channeliser configured nothing here launches, allocates or copies.
 * Definition.  M = nchannels, one of 2, 4, 8, 16, 32, 64; h[k], k in [0, ntaps): real float32 taps at the wideband
 * rate (ntaps < M is allowed: a branch without taps is 0); channel c in [0, M) sits at c/M cycles per input sample, so
 * c >= M/2 is the negative frequency (c - M)/M.  x[n]: wideband samples, n an absolute index counted from the last
 * reset (ofdm_set_pfb, ofdm_pfb_reset), zero before that reset's first index; the handle's receive IQ format and
 * scale, converted as the DDC converts.
 *   branches  u_p[m] = sum over q >= 0 with q M + p < ntaps of  h[q M + p] * x[(m - q) M - p],   p = 0..M-1:
 *             float32, ONE chain of packed fused multiply-adds on (re, im), ascending q, begun at +0
 *   table     w[j] = complex64(exp(+2 pi i j / M)), j in [0, M): float64 on the host, rounded once
 *   output    y_c[m] = sum_p u_p[m] w[(c p) mod M], evaluated in float32 by the radix-2 decimation-in-time recursion
 *               D_1(v) = v;   E = D_{n/2}(v[0], v[2], ...),  O = D_{n/2}(v[1], v[3], ...)
 *               t[c] = O[c] w[c M / n]    the unfused complex product; t[0] = O[0] (index 0 is not multiplied)
 *               D_n(v)[c] = E[c] + t[c],  D_n(v)[c + n/2] = E[c] - t[c]        c in [0, n/2)
 *             y[m] = D_M(u_0[m], ..., u_{M-1}[m]).  Schedule: M <= 16 is evaluated whole by one thread per output
 *             index; M = 32 and 64 in two steps of the same recursion -- the M/8 sub-transforms of size 8 (over
 *             p = r + (M/8) k), then the levels n = 16 .. M for the entries with equal c mod 8 -- the same operations
 *             on the same operands.
 *   outputs   the DDC's with R = M: a call with input indices [a, a + n) produces every m with a <= m M < a + n.
 * The bits of y_c[m] are a function of (m, c) and (M, h) alone: not of which channels are selected, their order or
 * number (the whole transform is computed, only selected rows are stored), nor of where a call, a chunk or a tile
 * starts.  A channel may be selected more than once; the rows are then equal.  Mathematically y_c[m] is the DDC bank's
 * link (R = M, h, fc = c/M); the order of the additions, hence the last bits, are this stage's own.
 *   state     the last ntaps - 1 converted samples (two buffers taking turns) and the absolute index of the next input
 *             sample: the channeliser's own, separate from every other stage's.
 * Pointers are host or device as the handle was created; ordering behind an ofdm_tx_async in flight and the alignment
 * rules are ofdm_ddc's.  Selected channel i's outputs go to the contiguous run iq_out + i * chan_stride (samples);
 * out_cap and *nout count outputs PER CHANNEL.  ofdm_pfb returns after the stream drained.
 * OFDM_E_INVAL: bad struct_size, nchannels not in the set, ntaps outside 1..OFDM_PFB_MAX_TAPS, nsel 0 or above
 * nchannels, a channel >= nchannels, a non-finite tap; a call without a configuration; an ofdm_sc16 input not 4-byte
 * (float32 input or iq_out: 8-byte) aligned; chan_stride < *nout with nsel > 1; first_sample_index above 2^62 or a
 * sample index past 2^63; a call too long for one grid (split it).  A refused configuration leaves the one in force
 * (or none) as it was.
 * OFDM_E_CAPACITY: out_cap smaller than ofdm_pfb_count says (*nout is set); the stream state is then unchanged. */
#define OFDM_PFB_MAX_CHANNELS 64
#define OFDM_PFB_MAX_TAPS 1024
typedef struct ofdm_pfb_cfg {
  uint32_t struct_size; /* = sizeof(ofdm_pfb_cfg) */
  uint32_t nchannels;   /* M: 2, 4, 8, 16, 32 or 64; also the decimation */
  uint32_t ntaps;       /* 1..OFDM_PFB_MAX_TAPS */
  uint32_t nsel;        /* K, 1..nchannels */
  uint8_t channel[OFDM_PFB_MAX_CHANNELS]; /* the selected channels, each in [0, nchannels); the first nsel count */
  float taps[OFDM_PFB_MAX_TAPS];          /* real low-pass prototype at the input rate, shared by the channels */
} ofdm_pfb_cfg;
/* one set_center_freq per radio channel of a uniform grid (dual_channel.py; the band scan of the sensing apps); NULL:
 * none.  Resets the channeliser's stream state. */
int ofdm_set_pfb(ofdm_handle *h, const ofdm_pfb_cfg *cfg);
/* a new stream whose first sample has this absolute index (a retune / a gap in the capture): history zero */
int ofdm_pfb_reset(ofdm_handle *h, uint64_t first_sample_index);
/* outputs PER CHANNEL the next ofdm_pfb call of nin samples produces, from the current state */
int ofdm_pfb_count(const ofdm_handle *h, uint64_t nin, uint64_t *nout);
/* the next nin samples of the stream through every channel of the grid (what the per-channel tuners of dual_channel.py
 * deliver, for all slots at once): selected channel i at iq_out + i * chan_stride, out_cap per channel */
int ofdm_pfb(ofdm_handle *h, const void *iq_in, uint64_t nin, ofdm_c32 *iq_out, uint64_t chan_stride, uint64_t out_cap,
             uint64_t *nout);
/* HIP-event time of k_pfb in the last ofdm_pfb, which must have run with profiling on and produced output;
 * OFDM_E_INVAL otherwise.  As ofdm_ddc_last_ms: the OFDM_K_* table is unchanged. */
int ofdm_pfb_last_ms(const ofdm_handle *h, double *ms);

/* --- wideband receive: rational-rate resampler (L / M) with tuning ahead of ofdm_rx -----------------------------------
 * The stages above need a capture whose rate is an integer multiple of the modem's.  Recorded captures often are not
 * (a radio answers a rate request with the rate it can make: "Actual sps for rate", uhd_interface.py): a file taken at
 * 25 MS/s that holds a 10 MS/s link has the ratio 5/2.  GNU Radio's blks2.rational_resampler_ccf(interpolation,
 * decimation, taps) fills that gap; this stage is that resampler fused with the DDC's frequency translation, so one
 * pass over the capture tunes to a link and brings it to the modem's rate for any L / M.  A standalone, stateful stage;
 * additions only: OFDM_ABI_VERSION stays 6, the OFDM_K_* table is unchanged, and with no resampler configured nothing
 * here launches, allocates or copies.
 * Definition.  x[i]: wideband samples, i an absolute index counted from the last reset (ofdm_set_resamp,
 * ofdm_resamp_reset), zero before that reset's first index; the handle's receive IQ format and scale, converted as
 * the DDC converts (one float32 multiply per part).  L = interpolation, M = decimation, any integers in 1..64 (the
 * library does not reduce them); h[k], k in [0, ntaps): real float32 taps at L times the input rate; fc in cycles per
 * INPUT sample.
 *   table     c[k] = complex64(h[k] exp(j 2 pi fc k / L)): float64 on the host, rounded once; ofdm_resamp_taps returns
 *             exactly what the kernel multiplies with.
 *   output n  sits at position n M on the L-times grid:  i_n = floor(n M / L),  p_n = n M mod L
 *               v[n] = sum over q >= 0 with p_n + q L < ntaps of  c[p_n + q L] * x[i_n - q]      float32
 *               y[n] = v[n] r[n]   r[n] = complex64(expj(-2 pi Phi_n / 2^64)),  Phi_n = n D mod 2^64
 *             D = frac(fc M / L) 2^64 truncated, 0 where frac rounds up to 1 (fc * M / L evaluated in float64).
 *   additions A += c.re * (x.re, x.im), B += c.im * (x.re, x.im): packed fused multiply-adds begun at +0;
 *             v = (A.re - B.im, A.im + B.re).  Tap q of an output belongs to chain q mod NG, a chain adds in ascending
 *             q, the chains are added in ascending order.  NG is a function of (L, M) alone: with
 *             KC = 16, 8, 4, 2, 1 for max(L, M) <= 1, 2, 4, 8, 64 it is 4 where L * KC < 4 and 1 otherwise.
 *   rotation  the unfused complex product with the engine's bit-reproducible float64 expj (as in the DDC).
 *   outputs   a call with input indices [a, a + n) produces every output with a <= i_n < a + n:
 *             count = ceil((a + n) L / M) - ceil(a L / M), possibly 0; a phase without a tap gives v = 0.
 *   state     the last (ntaps - 1) / L converted inputs and the absolute index of the next input; separate from the
 *             DDC's and the bank's: a handle may hold all three.
 * Nothing depends on where a call, a chunk or a tile starts: any segmentation of a stream gives bit-identical
 * outputs.  With L = 1 this is the DDC's definition (the summation order, hence the last bits, are this stage's own).
 * The stream's input index must stay at or below 2^56, as a reset value and after a call (i L and n M then fit 64-bit
 * integers); a call or reset that breaks this is refused.
 * Pointers are host or device as the handle was created; ordering behind an ofdm_tx_async in flight and the alignment
 * rules are ofdm_ddc's.  ofdm_resamp returns after the stream drained.
 * OFDM_E_INVAL: bad struct_size, interpolation or decimation outside 1..64, ntaps outside 1..OFDM_RESAMP_MAX_TAPS, a
 * non-finite tap, |center_freq| > 0.5 or NaN; ofdm_resamp / ofdm_resamp_reset / ofdm_resamp_count / ofdm_resamp_taps
 * without a configuration; an ofdm_sc16 pointer not 4-byte (float32: 8-byte) aligned; the index limit above.  A
 * refused configuration leaves the one in force (or none) as it was.
 * OFDM_E_CAPACITY: out_cap smaller than ofdm_resamp_count says (*nout is set); the stream state is then unchanged. */
#define OFDM_RESAMP_MAX_TAPS 1024
typedef struct ofdm_resamp_cfg {
  uint32_t struct_size;   /* = sizeof(ofdm_resamp_cfg) */
  uint32_t interpolation; /* L, 1..64 */
  uint32_t decimation;    /* M, 1..64 */
  uint32_t ntaps;         /* 1..OFDM_RESAMP_MAX_TAPS */
  double center_freq;     /* fc, cycles per INPUT sample, [-0.5, 0.5] */
  float taps[OFDM_RESAMP_MAX_TAPS]; /* real low-pass prototype at L times the input rate, gain L in its pass band */
} ofdm_resamp_cfg;
/* rational_resampler_ccf's ctor behind a tuner; NULL: none.  Resets the stream state (history zero, next input 0). */
int ofdm_set_resamp(ofdm_handle *h, const ofdm_resamp_cfg *cfg);
/* a new stream whose first sample has this absolute index (at most 2^56): history zero */
int ofdm_resamp_reset(ofdm_handle *h, uint64_t first_sample_index);
/* outputs the NEXT ofdm_resamp call of nin samples produces, from the current state */
int ofdm_resamp_count(const ofdm_handle *h, uint64_t nin, uint64_t *nout);
/* the next nin samples of the wideband stream in, the samples at L / M times their rate that they complete out */
int ofdm_resamp(ofdm_handle *h, const void *iq_in, uint64_t nin, ofdm_c32 *iq_out, uint64_t out_cap, uint64_t *nout);
/* the table the kernel multiplies with (out NULL: size query) */
int ofdm_resamp_taps(const ofdm_handle *h, ofdm_c32 *out, int cap, int *n);
/* HIP-event time of k_resamp in the last ofdm_resamp, which must have run with profiling on (ofdm_prof_enable) and
 * produced output; OFDM_E_INVAL otherwise.  As ofdm_ddc_last_ms: the OFDM_K_* table is unchanged. */
int ofdm_resamp_last_ms(const ofdm_handle *h, double *ms);

/* --- wideband receive: every link of a capture in one pass at a rational rate (resampler bank) ------------------------
 * What the DDC bank is to ofdm_ddc, for ofdm_resamp: one ratio L / M, one real prototype h[0..ntaps) and K centre
 * frequencies give K streams at the modem's rate from ONE pass over the wideband stream (a 25 MS/s capture that holds
 * several 10 MS/s links), where K calls of ofdm_resamp read, convert and stage the capture K times.  Additions only:
 * OFDM_ABI_VERSION stays 6 and the OFDM_K_* table is unchanged.
 * Definition.  Link i of the bank is the resampler above with (interpolation = L, decimation = M, taps = h,
 * center_freq = fc[i]), bit for bit:
 *   table     c_i[k] = complex64(h[k] exp(j 2 pi fc_i k / L)), float64 on the host, rounded once
 *             (ofdm_resamp_bank_taps);
 *   phase     D_i = frac(fc_i M / L) 2^64 truncated, 0 where frac rounds up to 1;
 *   input     the handle's receive IQ format and scale, converted as the resampler converts;
 *   output    of a call with input indices [a, a + n): every n with a <= floor(n M / L) < a + n, the same set for every
 *             link;
 *   additions tap q of an output belongs to chain q mod NG, NG the resampler's function of (L, M) alone; a chain adds
 *             its taps in ascending q into A += c.re * (x.re, x.im), B += c.im * (x.re, x.im), packed fused
 *             multiply-adds begun at +0; the chains are added in ascending order; v = (A.re - B.im, A.im + B.re);
 *   rotation  y_i[n] = v_i[n] r_i[n], the unfused complex product,
 *             r_i[n] = complex64(expj(-2 pi (n D_i mod 2^64) / 2^64)).
 * Nothing depends on where a call, a chunk or a tile starts, on K, or on a link's position in the list: link i's
 * stream equals what ofdm_resamp gives for fc_i, under any segmentation.  Equal frequencies are allowed and give equal
 * outputs.
 *   state     the last (ntaps - 1) / L converted samples and the absolute index of the next input sample, shared by
 *             all links and separate from the resampler's, the DDC's, the DDC bank's, the channeliser's and the
 *             transmit stages': a handle may have all of them configured, none disturbs another.
 * Pointers are host or device as the handle was created; ordering behind an ofdm_tx_async in flight and the alignment
 * rules are ofdm_ddc's.  Link i's outputs go to the contiguous run iq_out + i * link_stride (samples); out_cap and
 * *nout count outputs PER LINK.  With no bank configured nothing here launches, allocates or copies.
 * OFDM_E_INVAL: as for the resampler (bad struct_size, interpolation, decimation, ntaps, a non-finite tap, a call
 * without a configuration, misaligned input, a stream index above 2^56), and: nlinks 0 or above
 * OFDM_RESAMP_BANK_MAX_LINKS, any |center_freq[i]| > 0.5 or NaN, link >= nlinks, link_stride < *nout with nlinks > 1.
 * A refused configuration leaves the one in force (or none) as it was.
 * OFDM_E_CAPACITY: out_cap smaller than ofdm_resamp_bank_count says (*nout is set); the stream state is then
 * unchanged. */
#define OFDM_RESAMP_BANK_MAX_LINKS 8
typedef struct ofdm_resamp_bank_cfg {
  uint32_t struct_size;   /* = sizeof(ofdm_resamp_bank_cfg) */
  uint32_t interpolation; /* L, 1..64, shared by the links */
  uint32_t decimation;    /* M, 1..64, shared by the links */
  uint32_t ntaps;         /* 1..OFDM_RESAMP_MAX_TAPS */
  uint32_t nlinks;        /* K, 1..OFDM_RESAMP_BANK_MAX_LINKS */
  double center_freq[OFDM_RESAMP_BANK_MAX_LINKS]; /* fc[i], cycles per INPUT sample, [-0.5, 0.5]; the first nlinks count */
  float taps[OFDM_RESAMP_MAX_TAPS]; /* real low-pass prototype at L times the input rate, shared by the links */
} ofdm_resamp_bank_cfg;
/* K rational_resampler_ccf ctors behind K tuners on one stream; NULL: none.  Resets the bank's stream state. */
int ofdm_set_resamp_bank(ofdm_handle *h, const ofdm_resamp_bank_cfg *cfg);
/* a new stream whose first sample has this absolute index (at most 2^56): history zero */
int ofdm_resamp_bank_reset(ofdm_handle *h, uint64_t first_sample_index);
/* outputs PER LINK the next ofdm_resamp_bank call of nin samples produces, from the current state */
int ofdm_resamp_bank_count(const ofdm_handle *h, uint64_t nin, uint64_t *nout);
/* the next nin samples of the stream through every link: link i at iq_out + i * link_stride, out_cap per link */
int ofdm_resamp_bank(ofdm_handle *h, const void *iq_in, uint64_t nin, ofdm_c32 *iq_out, uint64_t link_stride,
                     uint64_t out_cap, uint64_t *nout);
/* the table of one link as the kernel multiplies with it (out NULL: size query) */
int ofdm_resamp_bank_taps(const ofdm_handle *h, int link, ofdm_c32 *out, int cap, int *n);
/* HIP-event time of k_resamp_bank in the last ofdm_resamp_bank, which must have run with profiling on and produced
 * output; OFDM_E_INVAL otherwise. */
int ofdm_resamp_bank_last_ms(const ofdm_handle *h, double *ms);

/* --- wideband transmit: interpolate and translate (DUC) behind ofdm_tx -------------
 * The mirror image of the stage above.  The reference leaves it to its radio (sink.set_interp / set_center_freq,
 * usrp_transmit_path.py:79-88; generic_usrp.set_interp; the two-channel transmitter of dual_channel/dual_channel.py);
 * with files and arrays in the radio's place it is a stateful polyphase interpolating FIR followed by a frequency
 * shift, which can add its output onto a band that already holds other links and can store 16-bit IQ.
 * Definition.  x[m]: narrowband complex64 samples, m an absolute index counted from the last reset (x is zero before
 * that reset's first index); L = interpolation; h[k], k in [0, ntaps): real float32 taps at the OUTPUT rate; fc in
 * cycles per OUTPUT sample.  For every input index m and phase p in [0, L) the output index is n = m L + p:
 *   v[n] = sum over q >= 0 with p + q L < ntaps of  h[p + q L] * x[m - q]     float32; real tap times complex sample
 *   y[n] = v[n] * r[n]      r[n] = complex64(expj(+2 pi Phi_n / 2^64)),  Phi_n = n D mod 2^64,
 *                           D = frac(fc) * 2^64 truncated, 0 where frac rounds up to 1 (the DDC's convention)
 *   out[n] = store(y[n] + add[n])  when an `add` buffer is given: one float32 addition per part
 *          = store(y[n])           otherwise
 *   additions v[n] is one chain in ascending q, begun at +0, of fused multiply-adds on the (re, im) pair: its value is
 *             a function of n alone.  A phase without a tap (ntaps <= p) gives v[n] = 0.
 *   product   y = v r is the gr_complex product: two products and one addition per part, separately rounded.
 *   phasor    r[n] depends on n and the configuration only; it is the engine's bit-reproducible float64 evaluation of
 *             expj at the phase (int64)Phi_n * 2 pi / 2^64, once per output, rounded to complex64 once -- not the
 *             hardware's sin / cos.
 *   store     complex64, or ofdm_sc16 by the transmit rule: clamp(rintf(part * scale), -32768, 32767), NaN -> 0,
 *             clamped in float.
 *   state     the last Q = (ntaps - 1) / L inputs and the absolute index of the next input.  A call with nin inputs
 *             produces exactly nin * L outputs.  A stream fed in any segmentation gives bit-identical outputs; calls
 *             of 0 inputs and calls shorter than Q are included.
 * Pointers are host or device as the handle was created.  iq_in is always complex64, whatever the handle's transmit
 * format; out_format is the stage's own.  add (may be NULL) is complex64 with nin * L samples and may be iq_out
 * itself when out_format is OFDM_IQ_FC32: each output sample is read before it is written, by the same thread.
 * Like ofdm_ddc, ofdm_duc orders itself behind an ofdm_tx_async still in flight on the transmit stream (in device
 * mode ofdm_tx_async's iq_out can be handed straight to it) and returns after the stream drained.
 * OFDM_E_INVAL: bad struct_size, interpolation, ntaps, out_format or out_scale, a non-finite tap, |center_freq| > 0.5;
 * ofdm_duc / ofdm_duc_reset without a configuration; a float32 pointer not 8-byte (ofdm_sc16: 4-byte) aligned; a
 * first_input_index, or a call, that would take an output index past 2^63.  A refused configuration leaves the one
 * in force (or none) as it was.
 * OFDM_E_CAPACITY: out_cap < nin * L (*nout is set); the stream state is then unchanged. */
#define OFDM_DUC_MAX_TAPS 1024
typedef struct ofdm_duc_cfg {
  uint32_t struct_size;   /* = sizeof(ofdm_duc_cfg) */
  uint32_t interpolation; /* L, 1..64, any integer (set_interp) */
  uint32_t ntaps;         /* 1..OFDM_DUC_MAX_TAPS */
  uint32_t out_format;    /* OFDM_IQ_FC32 | OFDM_IQ_SC16 */
  double center_freq;     /* fc, cycles per OUTPUT sample, [-0.5, 0.5] (set_center_freq / sampling_freq) */
  float out_scale;        /* OFDM_IQ_SC16 only: finite, > 0; 0 = the default 2^15 */
  uint32_t reserved;
  float taps[OFDM_DUC_MAX_TAPS]; /* real low-pass prototype at the output rate, gain L in its pass band */
} ofdm_duc_cfg;
/* sink.set_interp + set_center_freq; NULL: none.  Resets the stream state (history zero, next input index 0). */
int ofdm_set_duc(ofdm_handle *h, const ofdm_duc_cfg *cfg);
/* a new stream whose first input has this absolute index: history zero, outputs begin at index L * first */
int ofdm_duc_reset(ofdm_handle *h, uint64_t first_input_index);
/* the next nin samples of the narrowband stream in, nin * L wideband samples out (added onto `add` where given) */
int ofdm_duc(ofdm_handle *h, const ofdm_c32 *iq_in, uint64_t nin, const ofdm_c32 *add, void *iq_out, uint64_t out_cap,
             uint64_t *nout);
/* HIP-event time of k_duc in the last ofdm_duc, which must have run with profiling on (ofdm_prof_enable) and produced
 * output; OFDM_E_INVAL otherwise.  As ofdm_ddc_last_ms: the OFDM_K_* table is unchanged. */
int ofdm_duc_last_ms(const ofdm_handle *h, double *ms);

/* --- wideband transmit: polyphase-FFT synthesis bank for links on the c/M grid ----------------------------------------
 * The transmit mirror of the channeliser (ofdm_pfb): where the links of a band sit on a uniform grid (the two-channel
 * transmitter of dual_channel/dual_channel.py, one set_center_freq per radio channel), link c at centre frequency c/M
 * with interpolation M, the DUC's rotation is periodic with period M and the K passes of ofdm_duc(..., add = band)
 * collapse into ONE real-tap polyphase filter behind one M-point transform per input index: about 2 ntaps / M
 * multiply-adds and 8 bytes written per output sample, whatever the number of links.  A band built here is what
 * ofdm_pfb takes apart.  A standalone, stateful stage; additions only: OFDM_ABI_VERSION stays 6, the OFDM_K_* table is
 * unchanged, and with no synthesis bank configured nothing here launches, allocates or copies.
 * Definition.  M = nchannels, one of 2, 4, 8, 16, 32, 64, also the interpolation; K = nsel selected channels c_i in
 * [0, M), all different; h[k], k in [0, ntaps): real float32 taps at the OUTPUT rate (ntaps < M is allowed: a phase
 * without a tap gives 0); x_i[m]: selected channel i's narrowband complex64 stream, m an absolute index counted from
 * the last reset (ofdm_set_pfb_synth, ofdm_pfb_synth_reset), zero before that reset's first index.  Channel c sits at
 * c/M cycles per output sample, so c >= M/2 is the negative frequency (c - M)/M.
 *   column    z_c[m] = x_i[m] where c = c_i, (+0, +0) for every channel not selected
 *   table     w[j] = complex64(exp(+2 pi i j / M)), j in [0, M): ofdm_pfb's table, float64 on the host, rounded once
 *   spread    V[m] = D_M(z_0[m], ..., z_{M-1}[m]), V_p[m] = sum_c z_c[m] w[(c p) mod M]: D_M is ofdm_pfb's radix-2
 *             decimation-in-time recursion, the same function with the same schedule (M <= 16 whole; M = 32 and 64 in
 *             the two steps M = 8 * (M/8)), here over the channel index c, giving the phase p.  The WHOLE transform is
 *             evaluated, zeros included.
 *   filter    output n = m M + p, p in [0, M):
 *               v[n] = sum over q >= 0 with q M + p < ntaps of  h[q M + p] * V_p[m - q]
 *             float32, ONE chain of packed fused multiply-adds on (re, im), ascending q, begun at +0
 *   store     out[n] = store(v[n] + add[n]) when an `add` buffer is given (one float32 addition per part), else
 *             store(v[n]); complex64, or ofdm_sc16 by the transmit rule of ofdm_duc (out_format / out_scale are the
 *             stage's own).
 * There is no rotation: it is the transform.  Mathematically out = sum_i ofdm_duc(x_i; L = M, h, fc = c_i / M); the
 * order of the additions, hence the last bits, are this stage's own.  The bits of out[n] are a function of n, of
 * (M, h) and of the M-vector of channel inputs alone: never of the order in which the channels are listed, nor of
 * where a call, a chunk or a tile starts.  With channel 0 alone selected every butterfly adds or subtracts a zero,
 * V_p[m] = x[m] exactly, and the output equals ofdm_duc's at L = M, fc = 0 as numbers (the sign of a zero may differ).
 *   state     the last Q = (ntaps - 1) / M inputs of every selected channel (two buffers taking turns) and the absolute
 *             index of the next input: the bank's own, separate from every other stage's (a handle may hold the
 *             channeliser and the synthesis bank together).  A call with nin input indices per channel produces exactly
 *             nin * M outputs; calls of 0 and calls shorter than Q are included.
 * Selected channel i's nin inputs are the contiguous run iq_in + i * chan_stride (samples): the layout ofdm_pfb
 * writes.  add (may be NULL) is complex64 with nin * M samples and may be iq_out itself when out_format is
 * OFDM_IQ_FC32: each output sample is read before it is written, by the same thread.  Pointers are host or device as
 * the handle was created.  Like ofdm_duc, ofdm_pfb_synth orders itself behind an ofdm_tx_async still in flight and
 * returns after the stream drained.
 * OFDM_E_INVAL: bad struct_size, nchannels not in the set, ntaps outside 1..OFDM_PFB_MAX_TAPS, nsel 0 or above
 * nchannels, a channel >= nchannels, a channel listed twice, a bad out_format or out_scale, a non-finite tap;
 * ofdm_pfb_synth / ofdm_pfb_synth_reset without a configuration; a float32 pointer not 8-byte (ofdm_sc16: 4-byte)
 * aligned; chan_stride < nin with nsel > 1; a first_input_index, or a call, that would take an output index past
 * 2^63; a call too long for one grid (split it).  A refused configuration leaves the one in force (or none) as it was.
 * OFDM_E_CAPACITY: out_cap < nin * M (*nout is set); the stream state is then unchanged. */
typedef struct ofdm_pfb_synth_cfg {
  uint32_t struct_size; /* = sizeof(ofdm_pfb_synth_cfg) */
  uint32_t nchannels;   /* M: 2, 4, 8, 16, 32 or 64; also the interpolation */
  uint32_t ntaps;       /* 1..OFDM_PFB_MAX_TAPS */
  uint32_t nsel;        /* K, 1..nchannels */
  uint32_t out_format;  /* OFDM_IQ_FC32 | OFDM_IQ_SC16 */
  float out_scale;      /* OFDM_IQ_SC16 only: finite, > 0; 0 = the default 2^15 */
  uint8_t channel[OFDM_PFB_MAX_CHANNELS]; /* the selected channels, each in [0, nchannels), all different; the first nsel count */
  float taps[OFDM_PFB_MAX_TAPS];          /* real low-pass prototype at the output rate, gain M in its pass band */
} ofdm_pfb_synth_cfg;
/* one set_center_freq per radio channel of a uniform grid, transmit side; NULL: none.  Resets the stream state
 * (history zero, next input index 0). */
int ofdm_set_pfb_synth(ofdm_handle *h, const ofdm_pfb_synth_cfg *cfg);
/* a new stream whose first input has this absolute index: history zero, outputs begin at index M * first */
int ofdm_pfb_synth_reset(ofdm_handle *h, uint64_t first_input_index);
/* the next nin samples of every selected channel in, the nin * M samples of the band out (added onto `add` where given) */
int ofdm_pfb_synth(ofdm_handle *h, const ofdm_c32 *iq_in, uint64_t chan_stride, uint64_t nin, const ofdm_c32 *add,
                   void *iq_out, uint64_t out_cap, uint64_t *nout);
/* HIP-event time of k_pfb_synth in the last ofdm_pfb_synth, which must have run with profiling on (ofdm_prof_enable)
 * and produced output; OFDM_E_INVAL otherwise.  As ofdm_ddc_last_ms: the OFDM_K_* table is unchanged. */
int ofdm_pfb_synth_last_ms(const ofdm_handle *h, double *ms);

/* --- wideband transmit: every link of a band at arbitrary centre frequencies in one pass (DUC bank) -------------------
 * The transmit counterpart of the DDC bank, and what replaces one ofdm_duc(..., add = band) pass per link (the
 * two-channel transmitter of dual_channel/dual_channel.py; one sink.set_interp + set_center_freq per link,
 * usrp_transmit_path.py:79-88): one interpolation L, one real prototype h[0..ntaps) and K centre frequencies place K
 * narrowband streams on the band in ONE pass.  K passes of the DUC move the band K times through memory and evaluate
 * the float64 phasor r[n] once per OUTPUT and pass; here the shift moves to the input side,
 *   h[k] x[m - q] e^{j 2 pi fc n} = (h[k] e^{j 2 pi fc k}) (x[m - q] e^{j 2 pi fc L (m - q)}),   n = m L + p, k = p + q L,
 * one phasor per INPUT sample and link, and all links add into one accumulator pair before a single store.  The order
 * of the additions, hence the last bits, are this stage's own: it is not bit-identical to K DUC passes.  A standalone,
 * stateful stage; additions only: OFDM_ABI_VERSION stays 6, the OFDM_K_* table is unchanged, and with no bank
 * configured nothing here launches, allocates or copies.
 * Definition.  K = nlinks links, 1..OFDM_DUC_BANK_MAX_LINKS; L = interpolation in [1, 64], shared; h[k], k in
 * [0, ntaps): real float32 taps at the OUTPUT rate, shared; fc_i in [-0.5, 0.5] cycles per OUTPUT sample; x_i[m]:
 * link i's narrowband complex64 stream, m an absolute index counted from the last reset (ofdm_set_duc_bank,
 * ofdm_duc_bank_reset), zero before that reset's first index.
 *   phase     D_i = frac(fc_i) * 2^64 truncated, 0 where frac rounds up to 1 (the DUC's convention);
 *             E_i = (L * D_i) mod 2^64, the advance per INPUT sample.
 *   rotation  xr_i[m] = x_i[m] * r_i[m], r_i[m] = complex64(expj(+2 pi (m E_i mod 2^64) / 2^64)): the engine's
 *             bit-reproducible float64 evaluation of expj at the phase (int64)(m E_i) * 2 pi / 2^64 (the DUC's),
 *             rounded to complex64 once; the product is the gr_complex product: two products and one addition per
 *             part, separately rounded.  A function of the absolute m and the configuration alone.
 *   table     c_i[k] = complex64(h[k] exp(j 2 pi fc_i k)), float64 on the host, rounded once (ofdm_duc_bank_taps):
 *             the DDC bank's table.
 *   sums      for output n = m L + p, p in [0, L): A and B are each ONE chain of packed fused multiply-adds on the
 *             (re, im) pair, begun at +0; the links in ascending i, inside a link q ascending over p + q L < ntaps:
 *               A = fma(re c_i[p + q L], xr_i[m - q], A),   B = fma(im c_i[p + q L], xr_i[m - q], B)
 *             v[n] = (A.re - B.im, A.im + B.re), one float32 operation per part.  A phase without a tap
 *             (ntaps <= p) gives v[n] = 0.  The value depends on n and the configuration (the order of the list
 *             included), never on where a call, a chunk or a tile starts.
 *   store     out[n] = store(v[n] + add[n]) when an `add` buffer is given (one float32 addition per part), else
 *             store(v[n]); complex64, or ofdm_sc16 by the transmit rule of ofdm_duc (out_format / out_scale are the
 *             stage's own, as in ofdm_duc_cfg).
 *   state     the last Q = (ntaps - 1) / L RAW inputs of every link (two buffers taking turns; they are rotated when
 *             they are used, never stored rotated) and the absolute index of the next input: the bank's own, separate
 *             from every other stage's.  A call with nin inputs per link produces exactly nin * L outputs; any
 *             segmentation gives the same bits, calls of 0 inputs and calls shorter than Q included.
 * With K = 1 and fc = 0 the output equals ofdm_duc's at fc = 0, and with K = 1 and h = {1.0} it equals ofdm_duc's at
 * the same fc, as numbers (the sign of a zero may differ): the phasor, the phase convention and the product are the
 * DUC's.  Link i's nin inputs are the contiguous run iq_in + i * link_stride (samples), as in ofdm_pfb_synth.  add
 * (may be NULL) is complex64 with nin * L samples and may be iq_out itself when out_format is OFDM_IQ_FC32: each
 * output sample is read before it is written, by the same thread.  Pointers are host or device as the handle was
 * created.  Like ofdm_duc, ofdm_duc_bank orders itself behind an ofdm_tx_async still in flight and returns after the
 * stream drained.
 * OFDM_E_INVAL: bad struct_size, interpolation, ntaps, nlinks, out_format or out_scale, a non-finite tap, any
 * |center_freq[i]| > 0.5 or NaN; ofdm_duc_bank / ofdm_duc_bank_reset without a configuration; link >= nlinks; a
 * float32 pointer not 8-byte (ofdm_sc16: 4-byte) aligned; link_stride < nin with nlinks > 1; a first_input_index, or
 * a call, that would take an output index past 2^63; a call too long for one grid (split it).  A refused
 * configuration leaves the one in force (or none) as it was.
 * OFDM_E_CAPACITY: out_cap < nin * L (*nout is set); the stream state is then unchanged. */
#define OFDM_DUC_BANK_MAX_LINKS 8
typedef struct ofdm_duc_bank_cfg {
  uint32_t struct_size;   /* = sizeof(ofdm_duc_bank_cfg) */
  uint32_t interpolation; /* L, 1..64, shared by the links */
  uint32_t ntaps;         /* 1..OFDM_DUC_MAX_TAPS */
  uint32_t nlinks;        /* K, 1..OFDM_DUC_BANK_MAX_LINKS */
  uint32_t out_format;    /* OFDM_IQ_FC32 | OFDM_IQ_SC16 */
  float out_scale;        /* OFDM_IQ_SC16 only: finite, > 0; 0 = the default 2^15 */
  double center_freq[OFDM_DUC_BANK_MAX_LINKS]; /* fc[i], cycles per OUTPUT sample, [-0.5, 0.5]; the first nlinks count */
  float taps[OFDM_DUC_MAX_TAPS];               /* real low-pass prototype at the output rate, gain L in its pass band */
} ofdm_duc_bank_cfg;
/* K times sink.set_interp + set_center_freq on one band; NULL: none.  Resets the bank's stream state (history zero,
 * next input index 0). */
int ofdm_set_duc_bank(ofdm_handle *h, const ofdm_duc_bank_cfg *cfg);
/* a new stream whose first input has this absolute index: history zero, outputs begin at index L * first */
int ofdm_duc_bank_reset(ofdm_handle *h, uint64_t first_input_index);
/* the next nin samples of every link in, the nin * L samples of the band out (added onto `add` where given) */
int ofdm_duc_bank(ofdm_handle *h, const ofdm_c32 *iq_in, uint64_t link_stride, uint64_t nin, const ofdm_c32 *add,
                  void *iq_out, uint64_t out_cap, uint64_t *nout);
/* the table of one link as the kernel multiplies with it (out NULL: size query) */
int ofdm_duc_bank_taps(const ofdm_handle *h, int link, ofdm_c32 *out, int cap, int *n);
/* HIP-event time of k_duc_bank in the last ofdm_duc_bank, which must have run with profiling on (ofdm_prof_enable)
 * and produced output; OFDM_E_INVAL otherwise.  As ofdm_ddc_last_ms: the OFDM_K_* table is unchanged. */
int ofdm_duc_bank_last_ms(const ofdm_handle *h, double *ms);

/* --- wideband transmit: rational-rate resampler (L / M) behind ofdm_tx -------------------------------------------------
 * The DUC above needs a band whose rate is an integer multiple of the modem's.  A band at 25 MS/s that is to hold
 * 10 MS/s links has the ratio 5/2: GNU Radio's blks2.rational_resampler_ccf(interpolation, decimation, taps) in front
 * of the radio's set_center_freq fills that gap, and this stage is that resampler followed by the DUC's frequency
 * shift, `add` and 16-bit store -- the transmit-side counterpart of ofdm_resamp.  A standalone, stateful stage;
 * additions only: OFDM_ABI_VERSION stays 6, the OFDM_K_* table is unchanged, and with the stage not configured nothing
 * here launches, allocates or copies.
 * Definition.  x[i]: narrowband complex64 samples, i an absolute index counted from the last reset
 * (ofdm_set_tx_resamp, ofdm_tx_resamp_reset), zero before that reset's first index.  L = interpolation,
 * M = decimation, any integers in 1..64 (the library does not reduce them; either may be the larger); h[k],
 * k in [0, ntaps): real float32 taps at L times the input rate; fc in cycles per OUTPUT sample.
 *   output n  sits at position n M on the L-times grid:  i_n = floor(n M / L),  p_n = n M mod L
 *               v[n] = sum over q >= 0 with p_n + q L < ntaps of  h[p_n + q L] * x[i_n - q]     real tap times complex sample
 *               y[n] = v[n] * r[n]   r[n] = complex64(expj(+2 pi Phi_n / 2^64)),  Phi_n = n D mod 2^64,
 *                                    D = frac(fc) * 2^64 truncated, 0 where frac rounds up to 1 (the DDC's convention)
 *               out[n] = store(y[n] + add[n])  when an `add` buffer is given: one float32 addition per part
 *                      = store(y[n])           otherwise
 *   additions v[n] is ONE chain in ascending q, begun at +0, of fused multiply-adds on the (re, im) pair: its value is
 *             a function of n alone.  A phase without a tap (ntaps <= p_n) gives v[n] = 0.
 *   product   y = v r is the gr_complex product: two products and one addition per part, separately rounded.
 *   phasor    the engine's bit-reproducible float64 evaluation of expj at the phase (int64)Phi_n * 2 pi / 2^64, once
 *             per output, rounded to complex64 once -- not the hardware's sin / cos.
 *   store     complex64, or ofdm_sc16 by the transmit rule: clamp(rintf(part * scale), -32768, 32767), NaN -> 0,
 *             clamped in float.  out_format and out_scale are the stage's own, as in ofdm_duc_cfg.
 *   outputs   a call with input indices [a, a + nin) produces every output with a <= i_n < a + nin:
 *             count = ceil((a + nin) L / M) - ceil(a L / M), possibly 0 when L < M; `add` has that many samples.
 *   state     the last Q = (ntaps - 1) / L inputs and the absolute index of the next input; separate from the DUC's: a
 *             handle may hold both.
 * Nothing depends on where a call, a chunk or a tile starts: any segmentation of a stream gives bit-identical
 * outputs; calls of 0 inputs, calls shorter than Q and calls that produce nothing are included.  With M = 1 this is
 * ofdm_duc's definition, chain and rotation included: the outputs are bit-identical to ofdm_duc's.
 * The stream's input index must stay at or below 2^56, as a reset value and after a call (i L and n M then fit 64-bit
 * integers); a call or reset that breaks this is refused.
 * Pointers are host or device as the handle was created.  iq_in is always complex64, whatever the handle's transmit
 * format.  add (may be NULL) is complex64 and may be iq_out itself when out_format is OFDM_IQ_FC32: each output sample
 * is read before it is written, by the same thread.  Like ofdm_duc, ofdm_tx_resamp orders itself behind an
 * ofdm_tx_async still in flight on the transmit stream and returns after the stream drained.
 * OFDM_E_INVAL: bad struct_size, interpolation or decimation outside 1..64, ntaps outside 1..OFDM_TX_RESAMP_MAX_TAPS,
 * bad out_format or out_scale, a non-finite tap, |center_freq| > 0.5 or NaN; ofdm_tx_resamp / ofdm_tx_resamp_reset /
 * ofdm_tx_resamp_count without a configuration; a float32 pointer not 8-byte (ofdm_sc16: 4-byte) aligned; the index
 * limit above.  A refused configuration leaves the one in force (or none) as it was.
 * OFDM_E_CAPACITY: out_cap smaller than ofdm_tx_resamp_count says (*nout is set); the stream state is then unchanged. */
#define OFDM_TX_RESAMP_MAX_TAPS 1024
typedef struct ofdm_tx_resamp_cfg {
  uint32_t struct_size;   /* = sizeof(ofdm_tx_resamp_cfg) */
  uint32_t interpolation; /* L, 1..64 */
  uint32_t decimation;    /* M, 1..64 */
  uint32_t ntaps;         /* 1..OFDM_TX_RESAMP_MAX_TAPS */
  uint32_t out_format;    /* OFDM_IQ_FC32 | OFDM_IQ_SC16 */
  double center_freq;     /* fc, cycles per OUTPUT sample, [-0.5, 0.5] */
  float out_scale;        /* OFDM_IQ_SC16 only: finite, > 0; 0 = the default 2^15 */
  uint32_t reserved;
  float taps[OFDM_TX_RESAMP_MAX_TAPS]; /* real low-pass prototype at L times the input rate, gain L in its pass band */
} ofdm_tx_resamp_cfg;
/* rational_resampler_ccf's ctor + set_center_freq; NULL: none.  Resets the stream state (history zero, next input 0). */
int ofdm_set_tx_resamp(ofdm_handle *h, const ofdm_tx_resamp_cfg *cfg);
/* a new stream whose first input has this absolute index (at most 2^56): history zero */
int ofdm_tx_resamp_reset(ofdm_handle *h, uint64_t first_input_index);
/* outputs the NEXT ofdm_tx_resamp call of nin samples produces, from the current state */
int ofdm_tx_resamp_count(const ofdm_handle *h, uint64_t nin, uint64_t *nout);
/* the next nin samples of the narrowband stream in, the wideband samples they complete out (added onto `add` where given) */
int ofdm_tx_resamp(ofdm_handle *h, const ofdm_c32 *iq_in, uint64_t nin, const ofdm_c32 *add, void *iq_out, uint64_t out_cap,
                   uint64_t *nout);
/* HIP-event time of k_tx_resamp in the last ofdm_tx_resamp, which must have run with profiling on (ofdm_prof_enable)
 * and produced output; OFDM_E_INVAL otherwise.  As ofdm_ddc_last_ms: the OFDM_K_* table is unchanged. */
int ofdm_tx_resamp_last_ms(const ofdm_handle *h, double *ms);

/* --- wideband transmit: L / M resampler bank, K links onto one band in one pass -------------------------------------
 * What replaces one ofdm_tx_resamp(..., add = band) pass per link (several 10 MS/s links in a 25 MS/s band): one ratio
 * L / M, one real prototype h[0..ntaps) and K centre frequencies place K narrowband streams on the band in ONE pass.
 * K passes of ofdm_tx_resamp evaluate the float64 phasor once per OUTPUT and pass; here the shift moves to the input
 * side, as in the DUC bank: one phasor per INPUT sample and link (M / L per output), and all links add into one
 * accumulator pair before a single store.  The order of the additions, hence the last bits, are this stage's own: it
 * is not bit-identical to K ofdm_tx_resamp passes.  A standalone, stateful stage; additions only: OFDM_ABI_VERSION
 * stays 6, the OFDM_K_* table is unchanged, and with no bank configured nothing here launches, allocates or copies.
 * Definition.  K = nlinks links, 1..OFDM_TX_RESAMP_BANK_MAX_LINKS; L = interpolation and M = decimation, any integers
 * in 1..64, shared (the library does not reduce them); h[k], k in [0, ntaps): real float32 taps at L times the input
 * rate, shared; fc_i in [-0.5, 0.5] cycles per OUTPUT sample; x_i[m]: link i's narrowband complex64 stream, m an
 * absolute index counted from the last reset (ofdm_set_tx_resamp_bank, ofdm_tx_resamp_bank_reset), zero before that
 * reset's first index.  Output n sits at position n M on the L-times grid: i_n = floor(n M / L), p_n = n M mod L, and
 * a call with the inputs [a, a + nin) produces every output with a <= i_n < a + nin, as in ofdm_tx_resamp.
 *   phase     G_i = frac(fc_i / M) * 2^64 truncated, 0 where frac rounds up to 1: the phase per step of the L-times
 *             grid; fc_i / M is ONE double division.  E_i = (L * G_i) mod 2^64 is the advance per INPUT sample,
 *             D_i = (M * G_i) mod 2^64 the advance per OUTPUT sample.  The effective centre frequency is D_i / 2^64
 *             cycles per output sample; it can differ from fc_i by up to about M * 2^-54.
 *   rotation  xr_i[m] = x_i[m] * r_i[m], r_i[m] = complex64(expj(+2 pi (m E_i mod 2^64) / 2^64)): the engine's
 *             bit-reproducible float64 evaluation of expj, rounded to complex64 once; the product is the gr_complex
 *             product: two products and one addition per part, separately rounded.  A function of the absolute m and
 *             the configuration alone.
 *   table     c_i[k] = complex64(h[k] exp(j 2 pi fc_i k / M)), float64 on the host, rounded once
 *             (ofdm_tx_resamp_bank_taps): bit for bit the table ofdm_resamp_bank_taps returns for the mirror ratio
 *             (interpolation = M) with the same (h, fc_i).
 *   sums      for output n, p = p_n: A and B are each ONE chain of packed fused multiply-adds on the (re, im) pair,
 *             begun at +0; the links in ascending i, inside a link q ascending while p + q L < ntaps:
 *               A = fma(re c_i[p + q L], xr_i[i_n - q], A),   B = fma(im c_i[p + q L], xr_i[i_n - q], B)
 *             v[n] = (A.re - B.im, A.im + B.re), one float32 operation per part.  A phase without a tap
 *             (ntaps <= p) gives v[n] = 0.  The input-side shift is exact: n M = (p + q L) + (i_n - q) L, so
 *             k G_i + m E_i = n D_i modulo 2^64 without rounding.  The value depends on n and the configuration (the
 *             order of the list included), never on where a call, a chunk or a tile starts.
 *   store     out[n] = store(v[n] + add[n]) when an `add` buffer is given (one float32 addition per part), else
 *             store(v[n]); complex64, or ofdm_sc16 by the transmit rule of ofdm_tx_resamp (out_format / out_scale are
 *             the stage's own).
 *   state     the last Q = (ntaps - 1) / L RAW inputs of every link (rotated when they are used, never stored rotated)
 *             and the absolute index of the next input: the bank's own, separate from every other stage's.  Any
 *             segmentation gives the same bits; calls of 0 inputs, calls shorter than Q and calls that produce nothing
 *             are included.
 * With K = 1 and fc = 0 the output equals ofdm_tx_resamp's at fc = 0; with K = 1 and h = {1.0} it equals
 * ofdm_tx_resamp's at the same fc wherever frac(fc) 2^64 = M G exactly.  The stream's input index must stay at or
 * below 2^56, as a reset value and after a call.  Link i's nin inputs are the contiguous run iq_in + i * link_stride
 * (samples).  add (may be NULL) is complex64 with as many samples as the call has outputs and may be iq_out itself when
 * out_format is OFDM_IQ_FC32: each output sample is read before it is written, by the same thread.  Pointers are host
 * or device as the handle was created.  Like ofdm_duc_bank, the call orders itself behind an ofdm_tx_async still in
 * flight and returns after the stream drained.
 * OFDM_E_INVAL: bad struct_size, interpolation or decimation outside 1..64, bad ntaps, nlinks, out_format or out_scale,
 * a non-finite tap, any |center_freq[i]| > 0.5 or NaN; ofdm_tx_resamp_bank / _reset / _count / _taps without a
 * configuration; link >= nlinks; a float32 pointer not 8-byte (ofdm_sc16: 4-byte) aligned; link_stride < nin with
 * nlinks > 1; the index limit above; a call too long for one grid (split it).  A refused configuration leaves the one
 * in force (or none) as it was.
 * OFDM_E_CAPACITY: out_cap smaller than ofdm_tx_resamp_bank_count says (*nout is set); the stream state is then
 * unchanged. */
#define OFDM_TX_RESAMP_BANK_MAX_LINKS 8
typedef struct ofdm_tx_resamp_bank_cfg {
  uint32_t struct_size;   /* = sizeof(ofdm_tx_resamp_bank_cfg) */
  uint32_t interpolation; /* L, 1..64, shared by the links */
  uint32_t decimation;    /* M, 1..64, shared by the links */
  uint32_t ntaps;         /* 1..OFDM_TX_RESAMP_MAX_TAPS */
  uint32_t nlinks;        /* K, 1..OFDM_TX_RESAMP_BANK_MAX_LINKS */
  uint32_t out_format;    /* OFDM_IQ_FC32 | OFDM_IQ_SC16 */
  float out_scale;        /* OFDM_IQ_SC16 only: finite, > 0; 0 = the default 2^15 */
  double center_freq[OFDM_TX_RESAMP_BANK_MAX_LINKS]; /* fc[i], cycles per OUTPUT sample, [-0.5, 0.5]; the first nlinks count */
  float taps[OFDM_TX_RESAMP_MAX_TAPS]; /* real low-pass prototype at L times the input rate, gain L in its pass band */
} ofdm_tx_resamp_bank_cfg;
/* K rational_resampler_ccf ctors + set_center_freq on one band; NULL: none.  Resets the bank's stream state (history
 * zero, next input index 0). */
int ofdm_set_tx_resamp_bank(ofdm_handle *h, const ofdm_tx_resamp_bank_cfg *cfg);
/* a new stream whose first input has this absolute index (at most 2^56): history zero */
int ofdm_tx_resamp_bank_reset(ofdm_handle *h, uint64_t first_input_index);
/* outputs the NEXT ofdm_tx_resamp_bank call of nin samples per link produces, from the current state */
int ofdm_tx_resamp_bank_count(const ofdm_handle *h, uint64_t nin, uint64_t *nout);
/* the next nin samples of every link in, the samples of the band they complete out (added onto `add` where given) */
int ofdm_tx_resamp_bank(ofdm_handle *h, const ofdm_c32 *iq_in, uint64_t link_stride, uint64_t nin, const ofdm_c32 *add,
                        void *iq_out, uint64_t out_cap, uint64_t *nout);
/* the table of one link as the kernel multiplies with it (out NULL: size query) */
int ofdm_tx_resamp_bank_taps(const ofdm_handle *h, int link, ofdm_c32 *out, int cap, int *n);
/* HIP-event time of k_tx_resamp_bank in the last ofdm_tx_resamp_bank, which must have run with profiling on
 * (ofdm_prof_enable) and produced output; OFDM_E_INVAL otherwise.  As ofdm_ddc_last_ms: the OFDM_K_* table is unchanged. */
int ofdm_tx_resamp_bank_last_ms(const ofdm_handle *h, double *ms);

/* --- propagation channel: multipath, Doppler, tones, carrier offset and noise between ofdm_tx and ofdm_rx ------------
 * The reference puts a radio pair and the air between its transmitter and its receiver (usrp_transmit_path.py ->
 * usrp_receive_path.py); ofdm_chan above is the flat stand-in for it.  This stage is the frequency-selective and
 * time-varying one: P delayed paths, each with a complex gain and a Doppler shift, J continuous tones (a primary user
 * for the sensor), then ofdm_chan's carrier rotation and noise.  It has the call shape of ofdm_duc at L = 1.
 * Definition.  n is the absolute stream index; x[n] is indexed from the last reset (ofdm_set_multipath,
 * ofdm_multipath_reset) and zero before that reset's first index.
 *   c_p[n] = g_p                                                        where D_p == 0
 *          = g_p * complex64(expj(2 pi ((n D_p) mod 2^64) / 2^64))      otherwise: the gr_complex product
 *   v[n]   = sum over p in [0, P) of c_p[n] * x[n - d_p]                gr_complex products, added in float32 per part
 *                                                                       in ascending p, begun at +0
 *   t[n]   = sum over j in [0, J) of a_j * complex64(expj(2 pi ((Psi_j + n F_j) mod 2^64) / 2^64))
 *                                                                       real times complex; ascending j, begun at +0
 *   z[n]   = channel(v[n] + t[n]) at stream index n: ofdm_chan's definition with (sigma, cfo, seed, stream_id) -- the
 *            rotation by cfo * n where cfo != 0, then the noise word of index n where sigma > 0
 *   out[n] = store(z[n] + add[n])  when an `add` buffer is given: one float32 addition per part
 *          = store(z[n])           otherwise; complex64, or ofdm_sc16 by the transmit rule of ofdm_duc
 *   phases    D_p = frac(doppler_p) * 2^64, F_j = frac(tone_freq_j) * 2^64, Psi_j = frac(tone_phase_j) * 2^64,
 *             truncated, 0 where frac rounds up to 1 (the DDC's convention); the phasors are the engine's
 *             bit-reproducible float64 evaluation of expj at (int64)phase * 2 pi / 2^64, rounded to complex64 once.
 *   state     the last Dmax = max d_p inputs and the absolute index of the next input.  A call with nin inputs
 *             produces exactly nin outputs.  Every term is a function of n alone: a stream fed in any segmentation
 *             gives bit-identical outputs; calls of 0 inputs and calls shorter than Dmax are included.
 * With P = 1, d = 0, g = 1, J = 0 the output equals ofdm_channel's on the same samples at index0 = the stream's first
 * index, as numbers.  The stream index stays at or below 2^53: the rotation's float64 product cfo * n is exact only
 * below it.
 * Pointers are host or device as the handle was created.  iq_in and add are complex64; add (may be NULL) holds nin
 * samples and may be iq_out itself when out_format is OFDM_IQ_FC32.  iq_in must not overlap iq_out: a workgroup reads
 * the inputs of its neighbours' outputs.  Like ofdm_duc, the call orders itself behind an ofdm_tx_async still in
 * flight and returns after the stream drained.
 * OFDM_E_INVAL: bad struct_size, npaths, ntones, out_format or out_scale; a delay above OFDM_MULTIPATH_MAX_DELAY; a
 * non-finite gain; |doppler| or |tone_freq| > 0.5 or NaN; a tone_amp negative or not finite; a non-finite tone_phase;
 * sigma negative or not finite; a non-finite cfo (entries beyond npaths / ntones are not looked at);
 * ofdm_multipath / ofdm_multipath_reset without a configuration; a float32 pointer not 8-byte (ofdm_sc16: 4-byte)
 * aligned; iq_in overlapping iq_out; a first_index above 2^53, or a call that would take the stream past it.  A
 * refused configuration leaves the one in force (or none), stream state included, as it was.
 * OFDM_E_CAPACITY: out_cap < nin (*nout is set); the stream state is then unchanged. */
#define OFDM_MULTIPATH_MAX_PATHS 16
#define OFDM_MULTIPATH_MAX_TONES 4
#define OFDM_MULTIPATH_MAX_DELAY 1023
typedef struct ofdm_multipath_cfg {
  uint32_t struct_size;   /* = sizeof(ofdm_multipath_cfg) */
  uint32_t npaths;        /* P, 1..OFDM_MULTIPATH_MAX_PATHS */
  uint32_t ntones;        /* J, 0..OFDM_MULTIPATH_MAX_TONES */
  uint32_t out_format;    /* OFDM_IQ_FC32 | OFDM_IQ_SC16 */
  float out_scale;        /* OFDM_IQ_SC16 only: finite, > 0; 0 = the default 2^15 */
  float sigma;            /* ofdm_chan.sigma: finite, >= 0 */
  float cfo;              /* ofdm_chan.cfo, radians per sample: finite */
  uint64_t seed;          /* ofdm_chan.seed */
  uint64_t stream_id;     /* ofdm_chan.stream_id */
  uint32_t delay[OFDM_MULTIPATH_MAX_PATHS];   /* d_p in samples, 0..OFDM_MULTIPATH_MAX_DELAY; equal ones are allowed */
  ofdm_c32 gain[OFDM_MULTIPATH_MAX_PATHS];    /* g_p, finite */
  double doppler[OFDM_MULTIPATH_MAX_PATHS];   /* cycles per sample, [-0.5, 0.5] */
  float tone_amp[OFDM_MULTIPATH_MAX_TONES];   /* a_j: finite, >= 0 */
  double tone_freq[OFDM_MULTIPATH_MAX_TONES]; /* cycles per sample, [-0.5, 0.5] */
  double tone_phase[OFDM_MULTIPATH_MAX_TONES]; /* phase at stream index 0, cycles: finite */
} ofdm_multipath_cfg;
/* NULL: none (touches no device memory).  Resets the stream state (history zero, next index 0). */
int ofdm_set_multipath(ofdm_handle *h, const ofdm_multipath_cfg *cfg);
/* a new stream whose first sample has this absolute index (at most 2^53): history zero */
int ofdm_multipath_reset(ofdm_handle *h, uint64_t first_index);
/* the next nin samples of the stream in, nin samples out (added onto `add` where given) */
int ofdm_multipath(ofdm_handle *h, const ofdm_c32 *iq_in, uint64_t nin, const ofdm_c32 *add, void *iq_out, uint64_t out_cap,
                   uint64_t *nout);
/* HIP-event time of k_multipath in the last ofdm_multipath, which must have run with profiling on (ofdm_prof_enable)
 * and produced output; OFDM_E_INVAL otherwise.  As ofdm_ddc_last_ms: the OFDM_K_* table is unchanged. */
int ofdm_multipath_last_ms(const ofdm_handle *h, double *ms);

/* --- transmit crest-factor reduction: peak windowing in front of a converter -----------------------------------------
 * The modem's output has a peak-to-average power ratio of 10 to 11 dB; the clamp of the ofdm_sc16 store is a hard clip
 * per I and Q part.  This stage is the last one of a transmit chain, behind ofdm_tx and ofdm_duc / ofdm_tx_resamp:
 * every peak above a threshold is pulled down to it by a smooth dip of the gain, of the shape of a window the caller
 * supplies, and the stage counts what it did.  It has the call shape of ofdm_multipath without `add`: nin samples in,
 * nin samples out, stateful across calls.
 * Definition.  A = threshold, H = (ntaps - 1) / 2, w[k] = taps[k]; n is the stream index, x[n] indexed from the last
 * reset (ofdm_set_cfr, ofdm_cfr_reset) and zero before it.  All arithmetic is float32, every operation rounded once:
 *   m[n]   = sqrtf(x[n].re * x[n].re + x[n].im * x[n].im)     two products, one addition, one square root
 *   c[n]   = m[n] > A ? 1.0f - A / m[n] : 0.0f                 (a NaN magnitude gives 0; c[n] = 0 for n before the reset)
 *   s[n]   = sum over k in [0, 2H] of w[k] * c[n - k]          product, then addition, in ascending k, begun at +0
 *   b[n]   = fmaxf(0.0f, 1.0f - s[n])
 *   y[n]   = (b[n] * x[n - H].re, b[n] * x[n - H].im)
 *   out[n] = store(y[n])                                       complex64, or ofdm_sc16 by the transmit rule of ofdm_duc
 * The output is the input delayed by H samples.  H = 0 is the polar clip.  Because w[H] = 1, s[n] >= c[n - H] and
 * |y[n]| <= A up to rounding: max |y| <= A (1 + 2^-22) + 2^-24 max |x|.  Every term is a function of the stream alone: a
 * stream fed in any segmentation gives bit-identical outputs; calls of 0 inputs and calls shorter than 2H are included.
 *   state     the last 2H inputs.  A call with nin inputs produces exactly nin outputs; the last H samples of a
 *             stream come out when H more samples (zeros) are pushed behind it.
 * Statistics accumulate from ofdm_set_cfr / ofdm_cfr_reset on, over the inputs (n, n_over, peak_in, sum_in) and the
 * outputs (the others) of the calls since.  m^2 and |y|^2 are the float32 re * re + im * im; a term of sum_err is the
 * float32 (y.re - x.re)^2 + (y.im - x.im)^2 with x = x[n - H]: two differences, two squares, one addition.  Counts and
 * maxima (fmaxf, from 0: a NaN is not counted) do not depend on how the stream was cut; the float64 sums are added per
 * workgroup and then per call in a fixed order, so equal calls give equal sums, and two segmentations differ by the
 * rounding of float64 additions alone.
 * Pointers are host or device as the handle was created.  iq_in is complex64 and must not overlap iq_out: a workgroup
 * reads the inputs of its neighbours' outputs.  Like ofdm_duc, the call orders itself behind an ofdm_tx_async still in
 * flight and returns after the stream drained.  The kernel takes no id in the OFDM_K_* table (ofdm_cfr_last_ms).
 * OFDM_E_INVAL: bad struct_size; a threshold not finite or <= 0; ntaps even, 0 or above OFDM_CFR_MAX_TAPS;
 * taps[H] != 1; a tap outside [0, 1] or NaN; bad out_format or out_scale (entries beyond ntaps are not looked at);
 * ofdm_cfr / ofdm_cfr_reset / ofdm_cfr_stats without a configuration; a float32 pointer not 8-byte (ofdm_sc16:
 * 4-byte) aligned; iq_in overlapping iq_out; a call too long for one grid (2^34 samples: split it).  A refused
 * configuration leaves the one in force (or none), stream state and statistics included, as it was.
 * OFDM_E_CAPACITY: out_cap < nin (*nout is set); the stream state is then unchanged. */
#define OFDM_CFR_MAX_TAPS 1023
typedef struct ofdm_cfr_cfg {
  uint32_t struct_size;   /* = sizeof(ofdm_cfr_cfg) */
  float threshold;        /* A: finite, > 0 */
  uint32_t ntaps;         /* 2H + 1: odd, 1..OFDM_CFR_MAX_TAPS */
  uint32_t out_format;    /* OFDM_IQ_FC32 | OFDM_IQ_SC16 */
  float out_scale;        /* OFDM_IQ_SC16 only: finite, > 0; 0 = the default 2^15 */
  float taps[OFDM_CFR_MAX_TAPS]; /* the window: every value in [0, 1], taps[H] == 1 */
} ofdm_cfr_cfg;
struct ofdm_cfr_stats {   /* (a tag only: ofdm_cfr_stats is the function below) */
  uint64_t n;             /* samples */
  uint64_t n_over;        /* inputs with m > A */
  uint64_t n_touched;     /* outputs with b < 1 */
  float peak_in;          /* max m^2 */
  float peak_out;         /* max |y|^2 */
  double sum_in;          /* sum of m^2 */
  double sum_out;         /* sum of |y|^2 */
  double sum_err;         /* sum of |y[n] - x[n - H]|^2 */
};
/* NULL: none (touches no device memory).  Resets the stream state (history zero) and the statistics. */
int ofdm_set_cfr(ofdm_handle *h, const ofdm_cfr_cfg *cfg);
/* a new stream: history zero, statistics zero */
int ofdm_cfr_reset(ofdm_handle *h);
/* the next nin samples of the stream in, nin samples out */
int ofdm_cfr(ofdm_handle *h, const ofdm_c32 *iq_in, uint64_t nin, void *iq_out, uint64_t out_cap, uint64_t *nout);
/* the statistics since ofdm_set_cfr / ofdm_cfr_reset */
int ofdm_cfr_stats(ofdm_handle *h, struct ofdm_cfr_stats *out);
/* HIP-event time of k_cfr and the reduction of its partials in the last ofdm_cfr, which must have run with profiling
 * on (ofdm_prof_enable) and produced output; OFDM_E_INVAL otherwise.  As ofdm_ddc_last_ms: the OFDM_K_* table is
 * unchanged. */
int ofdm_cfr_last_ms(const ofdm_handle *h, double *ms);

/* --- transmit linearisation: a memory polynomial as predistorter and as power-amplifier model -------------------------
 * Peaks are limited (ofdm_cfr) because a power amplifier follows the converter.  This stage is a memory polynomial over
 * the stream: with one coefficient table it is the usual behavioural model of such an amplifier, with another it is
 * that amplifier's digital predistorter (the table comes from a least-squares fit on the host: dpd.py).  A handle
 * holds two instances, each with its own configuration, history, statistics and timer: slot OFDM_MEMPOLY_DPD, the
 * transmit side (behind ofdm_cfr, in front of the converter), and slot OFDM_MEMPOLY_PA, the air side (in front of
 * ofdm_multipath).  It has the call shape of ofdm_cfr: nin samples in, nin samples out, stateful across calls, no delay.
 * Definition.  M = memory, K = orders (the odd orders 1, 3, .., 2K - 1), a[m][k] = coef[m * OFDM_MEMPOLY_MAX_ORDERS + k];
 * n is the stream index, x[n] indexed from the last reset (ofdm_set_mempoly, ofdm_mempoly_reset) and zero before it.
 * All arithmetic is float32, every operation rounded once, nothing contracted:
 *   p[j]   = x[j].re * x[j].re + x[j].im * x[j].im           two products, one addition
 *   h_m[j] = Horner in p[j], from the top: h = a[m][K-1]; for k = K-2 .. 0:
 *            h = (h.re * p[j] + a[m][k].re, h.im * p[j] + a[m][k].im)       product, then addition: never an fmaf
 *   t_m[n] = h_m[n-m] (x) x[n-m] = (hr * xr - hi * xi, hr * xi + hi * xr)   the gr_complex product of the other stages
 *   y[n]   = t_0[n] + t_1[n] + .. + t_{M-1}[n]               float32 additions per part, ascending m, begun at t_0 (not +0)
 *   out[n] = store(y[n])                                     complex64, or ofdm_sc16 by the transmit rule of ofdm_duc
 * Every term is a function of the stream alone: a stream fed in any segmentation gives bit-identical outputs; calls of
 * 0 inputs and calls shorter than M - 1 are included.  The stage is causal: state is the last M - 1 inputs.
 * Statistics accumulate from ofdm_set_mempoly / ofdm_mempoly_reset on, as ofdm_cfr's do: n; peak_in and sum_in over
 * p[n]; peak_out and sum_out over |y|^2 = y.re * y.re + y.im * y.im (float32); n_over the outputs with |y|^2 above the
 * float32 product limit * limit.  `limit` is the converter's full scale: the stage counts and clamps nothing (a
 * predistorter expands peaks); +inf counts none.  Counts and maxima (fmaxf, from 0) do not depend on how the stream was
 * cut; the float64 sums are added per workgroup and then per call in a fixed order.
 * Pointers are host or device as the handle was created.  iq_in is complex64 and must not overlap iq_out: a workgroup
 * reads the inputs of its neighbour's outputs.  Like ofdm_cfr, the call orders itself behind an ofdm_tx_async still in
 * flight and returns after the stream drained.  The kernel takes no id in the OFDM_K_* table (ofdm_mempoly_last_ms).
 * Additions only: OFDM_ABI_VERSION stays 6, and with no slot configured nothing here launches, allocates or copies.
 * OFDM_E_INVAL: a slot that is neither OFDM_MEMPOLY_DPD nor OFDM_MEMPOLY_PA; bad struct_size; memory outside
 * [1, OFDM_MEMPOLY_MAX_MEMORY]; orders outside [1, OFDM_MEMPOLY_MAX_ORDERS]; a coefficient a[m][k] with m < memory and
 * k < orders that is not finite (the other entries are not looked at); a limit that is NaN or <= 0; bad out_format or
 * out_scale; ofdm_mempoly / ofdm_mempoly_reset / ofdm_mempoly_stats on a slot without a configuration; a float32
 * pointer not 8-byte (ofdm_sc16: 4-byte) aligned; iq_in overlapping iq_out; a call too long for two levels of the
 * statistics' reduction (2^34 samples: split it).  A refused configuration leaves the one in force (or none), stream
 * state and statistics included, as it was; a refused call moves nothing.
 * OFDM_E_CAPACITY: out_cap < nin (*nout is set); the stream state is then unchanged. */
#define OFDM_MEMPOLY_MAX_MEMORY 8
#define OFDM_MEMPOLY_MAX_ORDERS 5
#define OFDM_MEMPOLY_DPD 0u   /* slot: the predistorter, transmit side */
#define OFDM_MEMPOLY_PA 1u    /* slot: the amplifier model, air side */
#define OFDM_MEMPOLY_SLOTS 2
typedef struct ofdm_mempoly_cfg {
  uint32_t struct_size;   /* = sizeof(ofdm_mempoly_cfg) */
  uint32_t memory;        /* M: 1..OFDM_MEMPOLY_MAX_MEMORY */
  uint32_t orders;        /* K: 1..OFDM_MEMPOLY_MAX_ORDERS (polynomial orders 1, 3, .., 2K - 1) */
  uint32_t out_format;    /* OFDM_IQ_FC32 | OFDM_IQ_SC16 */
  float out_scale;        /* OFDM_IQ_SC16 only: finite, > 0; 0 = the default 2^15 */
  float limit;            /* > 0; +inf: n_over stays 0 */
  ofdm_c32 coef[OFDM_MEMPOLY_MAX_MEMORY * OFDM_MEMPOLY_MAX_ORDERS]; /* a[m][k] at [m * OFDM_MEMPOLY_MAX_ORDERS + k] */
} ofdm_mempoly_cfg;
struct ofdm_mempoly_stats {  /* (a tag only: ofdm_mempoly_stats is the function below) */
  uint64_t n;             /* samples */
  uint64_t n_over;        /* outputs with |y|^2 > limit * limit */
  float peak_in;          /* max p */
  float peak_out;         /* max |y|^2 */
  double sum_in;          /* sum of p */
  double sum_out;         /* sum of |y|^2 */
};
/* NULL: none (touches no device memory).  Resets the slot's stream state (history zero) and statistics. */
int ofdm_set_mempoly(ofdm_handle *h, uint32_t slot, const ofdm_mempoly_cfg *cfg);
/* a new stream on the slot: history zero, statistics zero */
int ofdm_mempoly_reset(ofdm_handle *h, uint32_t slot);
/* the next nin samples of the slot's stream in, nin samples out */
int ofdm_mempoly(ofdm_handle *h, uint32_t slot, const ofdm_c32 *iq_in, uint64_t nin, void *iq_out, uint64_t out_cap,
                 uint64_t *nout);
/* the slot's statistics since ofdm_set_mempoly / ofdm_mempoly_reset */
int ofdm_mempoly_stats(ofdm_handle *h, uint32_t slot, struct ofdm_mempoly_stats *out);
/* HIP-event time of k_mempoly and the reduction of its partials in the slot's last ofdm_mempoly, which must have run
 * with profiling on (ofdm_prof_enable) and produced output; OFDM_E_INVAL otherwise.  As ofdm_cfr_last_ms: the OFDM_K_*
 * table is unchanged. */
int ofdm_mempoly_last_ms(const ofdm_handle *h, uint32_t slot, double *ms);

/* --- spectrum measurement: an averaged-periodogram (Welch) estimator over any complex stream --------------------------
 * What ofdm_cfr and ofdm_mempoly exist for is what a transmitter emits outside its channel.  This stage measures it: the
 * power spectrum of a stream, segment by segment, with a float64 average, a max-hold and, where asked for, the
 * per-segment rows (adjacent-channel leakage, occupied bandwidth and mask margins are host-side figures of the average:
 * spectrum.py).  It reads its input and changes nothing.
 * Definition.  F = nfft, S = hop, w[i] = taps[i]; n is the stream index from the last reset (ofdm_set_psd,
 * ofdm_psd_reset).  Input samples are complex64, or ofdm_sc16 converted by the receive rule (float)int16 * in_scale.
 * Segment j covers x[j S .. j S + F); after T samples, T < F ? 0 : (T - F) / S + 1 segments are complete, and a call
 * completes those whose last sample it brought.  State: the samples from the first incomplete segment on, always fewer
 * than F; calls of 0 samples are included.  Per segment, in float32, every operation rounded once:
 *   e[i]   = (x[jS + i].re * w[i], x[jS + i].im * w[i])
 *   X      = fft_F(e)                                         the forward transform of ofdm_sense, same schedule: the
 *                                                             same inputs give the same bits
 *   P_j[k] = X[k].re * X[k].re + X[k].im * X[k].im            two products, one addition
 * P_j is a function of the stream alone: any segmentation of a stream gives bit-identical rows.  Accumulators since the
 * reset: nseg; sum[k], the float64 sum of P_j[k]; peak[k] = max over j of P_j[k], from 0 (order-independent; a NaN is not
 * counted, as in ofdm_sense).  The float64 sums are added per thread, per workgroup and then per call in an order fixed
 * by the call's segment count alone, without float atomics: equal calls give equal sums, and two segmentations differ by
 * the rounding of float64 additions alone (the rule of ofdm_cfr's statistics).  Bins are in FFT order: bin k is the
 * frequency k / F cycles per sample for k < F / 2 and (k - F) / F from there on.
 * Pointers are host or device as the handle was created (nrows and nseg are always host memory).  Like ofdm_cfr, the
 * call orders itself behind an ofdm_tx_async still in flight and returns after the stream drained.  The kernels take no
 * id in the OFDM_K_* table (ofdm_psd_last_ms).  Additions only: OFDM_ABI_VERSION stays 6, and with the stage not
 * configured nothing here launches, allocates or copies.
 * OFDM_E_INVAL: bad struct_size; an nfft that is not a power of two in [64, OFDM_PSD_MAX_FFT]; a hop of 0 or above nfft;
 * a tap among the first nfft that is not finite, or all of them zero (entries beyond nfft are not looked at); bad
 * in_format or in_scale; a complex64 pointer not 8-byte, an ofdm_sc16 or float pointer not 4-byte, a double pointer not
 * 8-byte aligned; rows overlapping iq_in; ofdm_psd / ofdm_psd_reset / ofdm_psd_count / ofdm_psd_read without a
 * configuration; a stream past 2^62 samples; a call that completes more than 2^31 - 1 segments (split it).  A refused
 * configuration leaves the one in force (or none), stream state and accumulators included, as it was; a refused call
 * moves nothing.
 * OFDM_E_CAPACITY: rows given and rows_cap below the call's segment count (*nrows is set); the stream state and the
 * accumulators are then unchanged. */
#define OFDM_PSD_MAX_FFT 4096
typedef struct ofdm_psd_cfg {
  uint32_t struct_size;   /* = sizeof(ofdm_psd_cfg) */
  uint32_t nfft;          /* F: a power of two, 64..OFDM_PSD_MAX_FFT */
  uint32_t hop;           /* S: 1..nfft */
  uint32_t in_format;     /* OFDM_IQ_FC32 | OFDM_IQ_SC16 */
  float in_scale;         /* OFDM_IQ_SC16 only: finite, > 0; 0 = the default 2^-15 */
  float taps[OFDM_PSD_MAX_FFT]; /* the window: the first nfft finite and not all zero */
} ofdm_psd_cfg;
/* NULL: none (touches no device memory).  Resets the stream state and the accumulators. */
int ofdm_set_psd(ofdm_handle *h, const ofdm_psd_cfg *cfg);
/* a new stream: nothing pending, accumulators zero */
int ofdm_psd_reset(ofdm_handle *h);
/* segments the next call of nin samples would complete */
int ofdm_psd_count(ofdm_handle *h, uint64_t nin, uint64_t *nrows);
/* the next nin samples of the stream.  rows: NULL, or room for rows_cap rows of nfft float32, which receive this call's
 * P_j in segment order. */
int ofdm_psd(ofdm_handle *h, const void *iq_in, uint64_t nin, float *rows, uint64_t rows_cap, uint64_t *nrows);
/* the accumulators since ofdm_set_psd / ofdm_psd_reset: nfft sums, nfft maxima, the segment count; each may be NULL */
int ofdm_psd_read(ofdm_handle *h, double *sum, float *peak, uint64_t *nseg);
/* HIP-event time of k_psd and k_psd_reduce in the last ofdm_psd, which must have run with profiling on
 * (ofdm_prof_enable) and completed a segment; OFDM_E_INVAL otherwise.  As ofdm_cfr_last_ms: the OFDM_K_* table is
 * unchanged. */
int ofdm_psd_last_ms(const ofdm_handle *h, double *ms);

/* --- coded links: rate-1/2, K = 7 convolutional code over the payload, Viterbi decoder on the GPU --------------------
 * A forward-error-correcting layer at the payload boundary: ofdm_fec_encode turns payloads into coded blocks that go
 * to ofdm_tx / ofdm_make_packets as payloads; ofdm_fec_decode takes the payloads ofdm_rx delivered (CRC-failed ones
 * included) and returns what was sent.  Additions only: OFDM_ABI_VERSION stays 6, the OFDM_K_* table is unchanged, and
 * without a call to these functions nothing here launches, allocates or copies.  All arithmetic is integer: results
 * are defined bit for bit.
 *
 * Definition.  Info bytes of an n-byte payload (0 <= n <= OFDM_FEC_MAX_PAYLOAD): payload | CRC-32(payload) big-endian
 * (the packet CRC); info bits u[0 .. 8(n+4)) MSB first, six zero tail bits behind them, u[t] = 0 for t < 0;
 * T = 8(n+4) + 6 steps.  Generators 133 / 171 octal:  A[t] = u[t]^u[t-2]^u[t-3]^u[t-5]^u[t-6],
 * B[t] = u[t]^u[t-1]^u[t-2]^u[t-3]^u[t-6];  coded bits c[2t] = A[t], c[2t+1] = B[t], then 4 zero pad bits:
 * 16n + 80 bits = 2n + 10 bytes.  Interleaver with C = interleave_cols columns, R = (16n + 80) / C: sent bit j =
 * c[(j mod R) * C + j / R], packed MSB first (C = 1: identity).
 * Decoder input: one signed value v per sent bit, v > 0 means 1, v = 0 is an erasure, -128 reads as -127; a hard byte
 * is v = +1 / -1 per bit.  The last 4 (deinterleaved) positions are ignored.  Full-sequence maximum-correlation
 * Viterbi: state bit k = u[t-1-k]; start and end in state 0; int32 path metric = sum of (2c-1) * v; a path is
 * replaced only by a strictly larger metric (on a tie the predecessor with u[t-6] = 0 stays); full traceback.
 * Per block: the n payload bytes, ok = 1 when the decoded CRC matches, corrected = positions among the first 2T
 * deinterleaved ones with v != 0 whose sign disagrees with the decoded sequence encoded again.
 * A coded length that is odd, under 10 or over OFDM_FEC_MAX_CODED is no block: ok = 0, no payload bytes,
 * corrected = 0 for that entry, and no error for the batch; nothing of it is read.
 *
 * Pointers as for ofdm_make_packets: the blobs (payloads, coded, soft) are host or device pointers by the handle's
 * mode; the offset, length, ok and corrected arrays are always host memory.  coded_off / payload_off OUT have
 * nblk + 1 entries and are set before the capacity check.  cfg NULL: interleave_cols 16.
 * OFDM_E_INVAL: bad struct_size, interleave_cols not one of 1, 2, 4, 8, 16, a payload longer than
 * OFDM_FEC_MAX_PAYLOAD (encode), a null argument.  OFDM_E_CAPACITY: the output blob is too small.
 * The decision workspace (8 bytes per trellis step and block in flight) belongs to the handle and is bounded; a large
 * batch is decoded in slices.
 *
 * Punctured rates (ofdm_fec_cfg.rate, both ends configured alike).  rate = OFDM_FEC_RATE_1_2 (0) is everything above,
 * unchanged: the same kernels and launches, nothing new allocates or copies.  Any value above OFDM_FEC_RATE_5_6 is
 * OFDM_E_INVAL.  Otherwise the mother coded bits c[0 .. 2T), 2T = 16n + 76 (without the pad), are thinned by the 802.11
 * patterns: bit i is kept when (i mod period) lies in the keep set,
 *   2/3: period 4, keep {0, 1, 2};   3/4: period 6, keep {0, 1, 2, 5};   5/6: period 10, keep {0, 1, 2, 5, 6, 9}.
 * Kept stream p[q] = c[i_q], i_q the q-th kept index in ascending order, K kept bits; the block has P = ceil(K / 8)
 * bytes, p[q] = 0 for K <= q < 8P.  P is strictly increasing in n, so a received length names at most one n; a length
 * P never reaches (or above P(OFDM_FEC_MAX_PAYLOAD)) is no block.  Interleaver of the punctured block: C' = the largest
 * power of two that is <= interleave_cols and divides 8P (8 where interleave_cols is 16 and P is odd, interleave_cols
 * otherwise), R' = 8P / C', sent bit j = p[(j mod R') * C' + j / R'], packed MSB first.
 * Decoding: one signed value v per sent bit of the punctured block; the C' interleaver is undone, mother value
 * d[i_q] = v_q for q < K, every other mother position (punctured ones and the pad) is 0, the values v_q, q >= K, are
 * ignored; then the decoder defined above runs on d, unchanged (corrected counts positions with d != 0 only).
 * All lengths and offsets of coded blocks, in and out, are those of the punctured blocks.  The mother values of the
 * blocks in flight (8 bytes per mother byte) live in a buffer the handle owns, cut into the same slices as the decision
 * workspace. */
#define OFDM_FEC_MAX_PAYLOAD 2040
#define OFDM_FEC_MAX_CODED 4090
#define OFDM_FEC_RATE_1_2 0
#define OFDM_FEC_RATE_2_3 1
#define OFDM_FEC_RATE_3_4 2
#define OFDM_FEC_RATE_5_6 3
typedef struct ofdm_fec_cfg {
  uint32_t struct_size;      /* = sizeof(ofdm_fec_cfg) */
  uint32_t interleave_cols;  /* 1, 2, 4, 8 or 16 */
  uint32_t rate;             /* OFDM_FEC_RATE_*; 0 = rate 1/2, the mother code */
  uint32_t reserved[5];      /* 0 */
} ofdm_fec_cfg;

/* pure host functions, usable without a GPU: 2n + 10, and its inverse (OFDM_E_INVAL for a length that is no block) */
int ofdm_fec_coded_len(uint32_t payload_len, uint32_t *coded_len);
int ofdm_fec_payload_len(uint32_t coded_len, uint32_t *payload_len);
int ofdm_fec_encode(ofdm_handle *h, const ofdm_fec_cfg *cfg, const uint8_t *payloads, const uint64_t *payload_off,
                    const uint32_t *payload_len, int nblk, uint8_t *coded, uint64_t coded_cap, uint64_t *coded_off);
int ofdm_fec_decode(ofdm_handle *h, const ofdm_fec_cfg *cfg, const uint8_t *coded, const uint64_t *coded_off,
                    const uint32_t *coded_len, int nblk, uint8_t *payloads, uint64_t payload_cap, uint64_t *payload_off,
                    uint8_t *ok, uint32_t *corrected);
/* the same from int8 values, 8 per coded byte: block k holds 8 * coded_len[k] values from soft + soft_off[k] */
int ofdm_fec_decode_soft(ofdm_handle *h, const ofdm_fec_cfg *cfg, const int8_t *soft, const uint64_t *soft_off,
                         const uint32_t *coded_len, int nblk, uint8_t *payloads, uint64_t payload_cap,
                         uint64_t *payload_off, uint8_t *ok, uint32_t *corrected);
/* HIP-event time of k_fec_encode / k_fec_decode (all slices) in the last of the three calls above, which must have run
 * with profiling on (ofdm_prof_enable) and launched; OFDM_E_INVAL otherwise.  As ofdm_ddc_last_ms: the OFDM_K_* table
 * is unchanged. */
int ofdm_fec_last_ms(const ofdm_handle *h, double *ms);
/* The two length functions at a rate, usable without a GPU: P(n) and its inverse (OFDM_E_INVAL for a rate above
 * OFDM_FEC_RATE_5_6, a payload above OFDM_FEC_MAX_PAYLOAD, a length that is no block at that rate, a null pointer).
 * With rate 0 they are ofdm_fec_coded_len / ofdm_fec_payload_len. */
int ofdm_fec_coded_len_rate(uint32_t rate, uint32_t payload_len, uint32_t *coded_len);
int ofdm_fec_payload_len_rate(uint32_t rate, uint32_t coded_len, uint32_t *payload_len);
/* HIP-event time of k_fec_puncture / k_fec_depuncture (all slices) alone in the last fec call, which must have run at a
 * punctured rate with profiling on and launched; OFDM_E_INVAL otherwise.  ofdm_fec_last_ms keeps reporting the encoder /
 * decoder: k_fec_decode's slices in a punctured decode; in a punctured encode k_fec_puncture is the encoder, and both
 * functions report it. */
int ofdm_fec_punct_last_ms(const ofdm_handle *h, double *ms);

/* --- soft-decision receive: per-bit reliabilities of the delivered packets (no reference counterpart) -----------------
 * Off by default; ofdm_set_rx_soft(h, &cfg) holds for the following ofdm_rx calls, ofdm_set_rx_soft(h, NULL) turns it
 * off and frees its buffer.  With it on, every packet ofdm_rx delivers (CRC failures included) also gets
 * 8 * payload_len int8 values in a buffer the handle owns, in the order ofdm_fec_decode_soft reads: value 8 m + k
 * belongs to bit 7 - k of payload byte m, v > 0 means the bit is 1, 0 is an erasure, -128 never occurs.
 * ofdm_rx_fec_decode_soft decodes them where they lie.  Additions only: OFDM_ABI_VERSION and the OFDM_K_* table are
 * unchanged, with the option off nothing new launches, allocates or copies, and no existing kernel changes: a call
 * with it on runs the demodulator's tap pass with the sink's rows requested internally, the CSI instantiation for the
 * equaliser rows, and one kernel more (k_soft_demap).  Independent of ofdm_set_taps, ofdm_set_rx_quality and
 * ofdm_set_rx_csi, which keep answering exactly as set (ofdm_tap(OFDM_TAP_RX_SINK) still needs the caller's own mask).
 *
 * Definition.  nmap data carriers per symbol, sink column c at occupied index smap[c]; nbits bits per carrier,
 * constellation cst[j], j < arity; the bit label of point j is j itself.  For one delivered packet: plen payload bytes
 * (message length minus the 4 CRC bytes); s = 0, 1, ... numbers the symbols the frame sink demapped for it (the rows
 * first_symbol + 1 ... first_symbol + nsym of the sampled symbols: the rows OFDM_TAP_RX_SINK holds for the packet);
 * eq is the packet's ofdm_rx_csi row hinv.  All arithmetic is float32, every operation rounded separately.
 *   carrier weight  m_i = eq[i].re^2 + eq[i].im^2;  w_i = 1 / m_i if m_i is finite and > 0, else 0
 *   mean weight     wbar = (sum of w_smap[c] for c = 0 ... nmap-1, one sequential chain in that order) / nmap
 *   gain            g = scale / (wbar * dmin2), dmin2 the smallest |cst[a] - cst[b]|^2 over a != b;
 *                   if wbar is 0 or not finite, every value of the packet is 0
 *   distances       for carrier (s, c) with x the slicer's input there: d_j = |x - cst[j]|^2, the slicer's own expression
 *   bit b < nbits   D0 = min d_j over the points with bit b of j clear, D1 over those with it set (+inf for an empty
 *                   class);  l = (D0 - D1) * (w_smap[c] * g);  v = rint(l) clamped to [-127, 127], NaN gives 0
 *   placement       the sink packs LSB first: stream bit beta = (s * nmap + c) * nbits + b lies in frame byte beta >> 3
 *                   with bit weight e = beta & 7; frame bytes 0-3 are the header; message byte mb = (beta >> 3) - 4 with
 *                   0 <= mb < plen receives the value at index 8 mb + 7 - e, negated where bit e of whitening_mask[mb]
 *                   is 1 (the mask ofdm_rx removes, offset 0).  Nothing is produced for the CRC bytes or beyond.
 * Packets the deframer does not deliver get no values.  Wherever the slicer's input has no two equidistant nearest
 * points with opposite bit b, v != 0 implies (v > 0) == the delivered payload's bit.
 * scale sets the value of a bit at the constellation's decision distance on a carrier of mean weight (default 32).
 *
 * ofdm_rx_soft: the last call's values, `out` a host or device pointer by the handle's mode, cap in values; off (host,
 * may be NULL) receives *n + 1 value offsets, packet k at [off[k], off[k+1]); out == NULL: size query.  OFDM_E_INVAL if
 * that call ran without soft values; OFDM_E_CAPACITY (with *n and off set) if cap < off[*n].
 * ofdm_rx_fec_decode_soft: the last call's packets through ofdm_fec_decode_soft's decoder, the values read from the
 * handle's buffer; payloads by the handle's mode, payload_off (max_pkts + 1), ok and corrected (max_pkts) host arrays.
 * A packet whose length is no block gives ok = 0 and no bytes.  OFDM_E_CAPACITY (with *n set) if max_pkts < *n.
 * ofdm_rx_soft_last_ms: HIP-event time of k_soft_demap in the last ofdm_rx, which must have run with profiling on and
 * launched it; OFDM_E_INVAL otherwise.  As ofdm_fec_last_ms: the OFDM_K_* table is unchanged. */
typedef struct ofdm_soft_cfg {
  uint32_t struct_size; /* = sizeof(ofdm_soft_cfg) */
  float scale;          /* > 0, finite; 32 is the usual choice */
} ofdm_soft_cfg;

int ofdm_set_rx_soft(ofdm_handle *h, const ofdm_soft_cfg *cfg);
int ofdm_rx_soft(ofdm_handle *h, int8_t *out, uint64_t cap, uint64_t *off, int *n);
int ofdm_rx_fec_decode_soft(ofdm_handle *h, const ofdm_fec_cfg *cfg, uint8_t *payloads, uint64_t payload_cap,
                            uint64_t *payload_off, uint8_t *ok, uint32_t *corrected, int max_pkts, int *n);
int ofdm_rx_soft_last_ms(ofdm_handle *h, double *ms);

/* --- coded links, reliabilities out: a soft-output Viterbi decoder for errors-and-erasures decoding of the outer code ----
 * A second inner decoder: ofdm_fec_decode_rel / ofdm_fec_decode_soft_rel / ofdm_rx_fec_decode_soft_rel return exactly what
 * ofdm_fec_decode / ofdm_fec_decode_soft / ofdm_rx_fec_decode_soft return for the same input, and one reliability byte per
 * decoded payload byte in the format ofdm_rs_decode_rel takes.  Additions only: OFDM_ABI_VERSION stays 6, the OFDM_K_*
 * table is unchanged, k_fec_decode, its launches and its workspace are unchanged, and without a call to these three
 * functions nothing new launches, allocates or copies.  All arithmetic is integer: results are defined bit for bit.
 *
 * Definition, in the notation of "coded links": T steps, states with bit k = u[t-1-k], the deinterleaved (at a punctured
 * rate: depunctured) mother values d, the int32 path metric = sum of (2c - 1) * v, the branch metric of a step = its two
 * terms.
 *   decoded bits     u^[t], payload, ok and corrected are ofdm_fec_decode's / ofdm_fec_decode_soft's, ties included: the
 *                    same rule and the same traceback
 *   forward metric   alpha_0(0) = 0, alpha_0(s) = -2^29 for s != 0; alpha_{t+1}(s') = the maximum over the two
 *                    predecessors of alpha_t + branch metric (the values the decoder holds after step t)
 *   backward metric  beta_T(0) = 0, beta_T(s) = -2^29 for s != 0; beta_t(s) = the maximum over the two successors
 *                    s' = ((s & 31) << 1) | b of beta_{t+1}(s') + the branch metric of s -> s' at step t
 *   alternative      for an info bit t < 8(n+4) and b in {0, 1}: A_t(b) = max over s' with (s' & 1) = b of
 *                    alpha_{t+1}(s') + beta_{t+1}(s'), the best metric of a path from state 0 to state 0 with u[t] = b
 *   bit reliability  M* = alpha_T(0); Delta_t = M* - A_t(1 - u^[t]).  Delta_t >= 0 (u^'s path has metric M*), even (two
 *                    path metrics differ by 2 * sum of +-v) and finite (flipping one info bit and keeping the zero tail is
 *                    a path).  No sum leaves int32: |metric| <= 2 * 16358 * 127, and at most two -2^29 terms meet.
 *   byte reliability for payload byte m < n: q[m] = min(255, min over t = 8m .. 8m + 7 of Delta_t / 2).  0: a path as
 *                    good as the decoded one disagrees in this byte; 255 is ofdm_rs_decode_rel's "never erase".  Nothing
 *                    is produced for the CRC bytes or the tail.
 * This is the full (Battail / max-log-MAP) soft output, not a windowed one.  A length that is no block gives ok = 0, no
 * payload bytes and no reliability bytes.
 *
 * rel is a host or device pointer by the handle's mode, rel_cap its bytes; block k's n_k bytes lie at
 * rel + payload_off[k], the offsets of the payload blob.  In device-pointer mode payloads, rel and payload_off are
 * therefore ofdm_rs_decode_rel's coded, rel and coded_off with rel_off == NULL: the two layers chain without a host
 * round trip.  Errors as ofdm_fec_decode (ofdm_rx_fec_decode_soft for the third); in addition a null rel is
 * OFDM_E_INVAL, and rel_cap < payload_off[nblk] is OFDM_E_CAPACITY with the offsets set first.
 * Workspace: next to the decision words (8 bytes per step) the forward metrics at every 64th step, 4 bytes per step and
 * block in flight, in a buffer the handle owns, cut into the same slices.  At a punctured rate k_fec_depuncture runs
 * first, exactly as for ofdm_fec_decode.  After these calls ofdm_fec_last_ms reports k_fec_decode_rel's slices, and
 * ofdm_fec_punct_last_ms behaves as after ofdm_fec_decode. */
int ofdm_fec_decode_rel(ofdm_handle *h, const ofdm_fec_cfg *cfg, const uint8_t *coded, const uint64_t *coded_off,
                        const uint32_t *coded_len, int nblk, uint8_t *payloads, uint64_t payload_cap, uint64_t *payload_off,
                        uint8_t *ok, uint32_t *corrected, uint8_t *rel, uint64_t rel_cap);
int ofdm_fec_decode_soft_rel(ofdm_handle *h, const ofdm_fec_cfg *cfg, const int8_t *soft, const uint64_t *soft_off,
                             const uint32_t *coded_len, int nblk, uint8_t *payloads, uint64_t payload_cap,
                             uint64_t *payload_off, uint8_t *ok, uint32_t *corrected, uint8_t *rel, uint64_t rel_cap);
int ofdm_rx_fec_decode_soft_rel(ofdm_handle *h, const ofdm_fec_cfg *cfg, uint8_t *payloads, uint64_t payload_cap,
                                uint64_t *payload_off, uint8_t *ok, uint32_t *corrected, uint8_t *rel, uint64_t rel_cap,
                                int max_pkts, int *n);

/* --- outer code: Reed-Solomon over GF(2^8) on the GPU, the outer half of a concatenated link -----------------------------
 * A byte-oriented code at the payload boundary, above the coded links and independent of them (it also works on an
 * uncoded link): ofdm_rs_encode turns payloads into RS blocks that go to ofdm_fec_encode, or straight to ofdm_tx /
 * ofdm_make_packets, as payloads; ofdm_rs_decode takes what ofdm_fec_decode (whatever its CRC said) or ofdm_rx
 * delivered and returns what was sent.  Its correction unit is the Viterbi decoder's failure unit: a short burst of
 * wrong bytes.  Additions only: OFDM_ABI_VERSION stays 6, the OFDM_K_* table is unchanged, and without a call to these
 * functions nothing here launches, allocates or copies.  All arithmetic is integer: results are defined bit for bit.
 * The code has no parameters, hence no configuration struct.
 *
 * Field and generator.  GF(2^8) modulo x^8 + x^4 + x^3 + x^2 + 1 (0x11d), alpha = 0x02 (alpha^8 = 0x1d,
 * alpha^255 = 1).  g(x) = product over i = 0 .. 31 of (x - alpha^i): OFDM_RS_PARITY = 32 parity bytes per codeword,
 * t = 16.
 * Block layout.  Info bytes of an n-byte payload (0 <= n <= OFDM_RS_MAX_PAYLOAD): payload | CRC-32(payload)
 * big-endian, k = n + 4 bytes.  W = ceil(k / 223) codewords, byte-interleaved to depth W: info byte i is symbol i / W
 * (rounded down) of codeword i mod W, so codeword w has k_w = ceil((k - w) / W) <= 223 info symbols and is the
 * RS(255, 223) code shortened to k_w + 32 symbols.  The first symbol is the highest-degree coefficient; the parity is
 * m_w(x) x^32 mod g(x), parity byte j the coefficient of x^(31 - j).  Coded block: the k info bytes verbatim
 * (systematic), then the parity, byte j of codeword w at position k + j W + w.  Its length is
 * f(k) = k + 32 ceil(k / 223), strictly increasing in steps of 1 or 33: f(4) = 36, f(223) = 255, f(224) = 288,
 * f(1784) = 2040, f(1785) = 2073, f(3568) = 4080.  A length f never reaches, below 36 or above OFDM_RS_MAX_CODED is
 * no block: ok = 0, no payload bytes, corrected = failed = 0 for that entry, nothing of it is read, and no error for
 * the batch (as the coded links treat an odd length).  OFDM_RS_MAX_PAYLOAD = 3564 gives W = 16 and the largest block a
 * frame takes; under an inner code the RS block must fit OFDM_FEC_MAX_PAYLOAD, so n <= 1780 (W = 8, block 2040).
 * Decoding.  Per codeword bounded-distance: if a codeword of the shortened code lies within 16 symbol differences of
 * the received word it is unique, and the output is that codeword; otherwise the received symbols stay as they are and
 * the codeword counts as failed.  (An error locator with a root in the shortened, implicitly zero, region, with fewer
 * roots than its degree, or of degree above 16 is a failure, not a correction.)  Per block: the n payload bytes after
 * correction; ok = 1 when the CRC-32 of the corrected payload matches the corrected CRC bytes; corrected = symbols
 * changed, summed over the codewords that decoded; failed = codewords that failed.  Any burst of at most 15 W + 1
 * consecutive wrong bytes is corrected wherever it lies, up to 16 W where it stays inside the info part or inside the
 * parity part (across the boundary the interleaving phase jumps by k mod W).
 *
 * Pointers, offsets, capacities and errors exactly as ofdm_fec_encode / ofdm_fec_decode: the blobs (payloads, coded)
 * are host or device pointers by the handle's mode; the offset, length, ok, corrected and failed arrays are always host
 * memory.  coded_off / payload_off OUT have nblk + 1 entries and are set before the capacity check.  OFDM_E_INVAL: a
 * payload longer than OFDM_RS_MAX_PAYLOAD (encode), a null argument.  OFDM_E_CAPACITY: the output blob is too small.
 * In device-pointer mode the payload blob and payload_off of ofdm_fec_decode are the coded blob and coded_off of
 * ofdm_rs_decode (coded_len[k] = payload_off[k + 1] - payload_off[k]), and the coded blob and coded_off of
 * ofdm_rs_encode are the payloads of ofdm_fec_encode: the two layers chain without a host round trip.
 * ofdm_rs_last_ms: HIP-event time of k_rs_encode / k_rs_decode in the last of the two calls, which must have run with
 * profiling on (ofdm_prof_enable) and launched; OFDM_E_INVAL otherwise.  As ofdm_fec_last_ms. */
#define OFDM_RS_PARITY 32
#define OFDM_RS_MAX_PAYLOAD 3564
#define OFDM_RS_MAX_CODED 4080
/* pure host functions, usable without a GPU: f(n + 4), and its inverse (OFDM_E_INVAL for a length that is no block) */
int ofdm_rs_coded_len(uint32_t payload_len, uint32_t *coded_len);
int ofdm_rs_payload_len(uint32_t coded_len, uint32_t *payload_len);
int ofdm_rs_encode(ofdm_handle *h, const uint8_t *payloads, const uint64_t *payload_off, const uint32_t *payload_len,
                   int nblk, uint8_t *coded, uint64_t coded_cap, uint64_t *coded_off);
int ofdm_rs_decode(ofdm_handle *h, const uint8_t *coded, const uint64_t *coded_off, const uint32_t *coded_len, int nblk,
                   uint8_t *payloads, uint64_t payload_cap, uint64_t *payload_off, uint8_t *ok, uint32_t *corrected,
                   uint32_t *failed);
int ofdm_rs_last_ms(const ofdm_handle *h, double *ms);

/* --- outer code, decoding with reliabilities: errors-and-erasures, the erased symbols chosen per codeword --------------
 * ofdm_rs_decode_rel is ofdm_rs_decode with one reliability byte per received byte: a codeword the rule above fails is
 * tried once more with its least reliable symbols erased; an erased symbol costs half an error (2 e + f <= 32).
 * ofdm_rs_rel_from_soft makes the reliabilities of an RS link without an inner code from the soft demapper's values.
 * Additions only, as above: without a call to these two nothing new launches, allocates or copies, ofdm_rs_decode returns
 * what it returned, k_rs_encode and k_rs_decode are unchanged.  All arithmetic is integer.
 *
 * Inputs.  rel holds one uint8_t per byte of each coded block, block k at rel + rel_off[k]; rel_off == NULL means
 * coded_off.  0 is the least reliable value, 255 means "never erase".  rel is a host or device pointer by the handle's
 * mode, like coded.  M = cfg->max_erasures in 0 .. 32; cfg == NULL means M = 28 (chosen, not measured: it leaves four
 * parity symbols as a check on what the erasures fill in; the CRC-32 inside the block still decides ok).  rel == NULL or
 * M = 0 gives exactly ofdm_rs_decode's result.  second (host, may be NULL) receives, per block, the number of codewords
 * decoded by the second pass.
 * First pass.  Every codeword first gets ofdm_rs_decode's rule, unchanged: a codeword that decodes there gives that
 * result whatever rel says.
 * Second pass, for a codeword the first pass fails, with symbols r_p and reliabilities q_p over its real positions p (the
 * shortened region has none).  c(tau) = #{p : q_p <= tau}; tau* = the largest tau in 0 .. 254 with c(tau) <= M.  If
 * there is none (c(0) > M) or c(tau*) = 0 the codeword stays failed.  Otherwise J = {p : q_p <= tau*}, f = |J|.  If a
 * codeword of the shortened code differs from r in e positions outside J with 2 e + f <= 32 it is unique (two such would
 * differ in at most 32 < 33 positions) and is the output; corrected gains the number of symbols changed, inside J or
 * not, and second gains 1.  If there is none the symbols stay as received and the codeword counts as failed.  (An
 * errata locator with a root in the shortened region, with fewer roots among the real positions than its degree, or
 * with an error part of degree above (32 - f) / 2 is a failure.)  No smaller tau is tried after a failure.
 * ofdm_rs_rel_from_soft.  The reliability of byte m is the minimum of |v| over its eight values soft[8 m .. 8 m + 7],
 * -128 read as 127: 0 .. 127, and a byte holding an erased bit gets 0.  Value layout and offsets as
 * ofdm_fec_decode_soft (block k: 8 * coded_len[k] values from soft + soft_off[k], soft_off[k] a multiple of 8); every
 * entry is converted whatever its length; rel_off (OUT, nblk + 1 entries) is the running sum of coded_len.
 * Errors as ofdm_rs_decode.  OFDM_E_INVAL: a bad struct_size, M > 32, a non-zero reserved word, a null argument, a value
 * offset that is no multiple of 8.  OFDM_E_CAPACITY: rel_cap or payload_cap too small, the offsets set first.  A length
 * that is no block gives ok = 0 and zeros, and nothing of it, or of its reliabilities, is read.
 * ofdm_rs_last_ms reports the decode kernel (k_rs_decode_rel, or k_rs_decode where rel == NULL or M = 0) of the last call;
 * ofdm_rs_rel_last_ms: HIP-event time of k_rs_rel_soft in the last ofdm_rs_rel_from_soft, which must have run with
 * profiling on and launched; OFDM_E_INVAL otherwise. */
typedef struct ofdm_rs_rel_cfg {
  uint32_t struct_size;  /* = sizeof(ofdm_rs_rel_cfg) */
  uint32_t max_erasures; /* M: 0 .. 32 */
  uint32_t reserved[6];  /* 0 */
} ofdm_rs_rel_cfg;       /* 32 bytes */
int ofdm_rs_decode_rel(ofdm_handle *h, const ofdm_rs_rel_cfg *cfg, const uint8_t *coded, const uint64_t *coded_off,
                       const uint32_t *coded_len, int nblk, const uint8_t *rel, const uint64_t *rel_off, uint8_t *payloads,
                       uint64_t payload_cap, uint64_t *payload_off, uint8_t *ok, uint32_t *corrected, uint32_t *failed,
                       uint32_t *second);
int ofdm_rs_rel_from_soft(ofdm_handle *h, const int8_t *soft, const uint64_t *soft_off, const uint32_t *coded_len, int nblk,
                          uint8_t *rel, uint64_t rel_cap, uint64_t *rel_off);
int ofdm_rs_rel_last_ms(const ofdm_handle *h, double *ms);

/* --- coded links: LDPC -- quasi-cyclic codes of rate 1/2, 2/3, 3/4 and 5/6 with a layered min-sum decoder on the GPU -------
 * A second inner code next to the convolutional one, at the same boundary: ofdm_ldpc_encode turns payloads into coded
 * blocks that go to ofdm_tx / ofdm_make_packets as payloads; ofdm_ldpc_decode takes the payloads ofdm_rx delivered
 * (CRC-failed ones included).  Additions only: OFDM_ABI_VERSION stays 6, the OFDM_K_* table is unchanged, no existing
 * kernel, launch or workspace changes, and without a call to these functions nothing here launches, allocates or
 * copies.  All arithmetic is integer: results are defined bit for bit.
 *
 * Code.  Circulant size Z = 64, base matrix 12 rows x 24 columns: n = 1536 bits, k = 768 info bits per codeword.
 * Codeword bit 64 j + z is lane z of column j.  For a 64-bit column x, rot(x, s)[z] = x[(z + s) mod 64].  Check (i, z):
 * the XOR over the entries (i, j, s) of rot(x_j, s)[z] is 0.  Info part, the shift of row i (down) and column
 * j = 0 .. 11 (across), - for no entry:
 *    0:  -  1  -  - 25  -  - 42  - 59  - 24
 *    1:  -  -  - 17 48  -  -  - 37  - 21 42
 *    2:  2  -  -  -  -  -  0  - 56  - 20 50
 *    3:  - 52  -  -  -  5  -  - 45 19 45  -
 *    4:  -  - 34  -  -  - 30  - 29 31  - 55
 *    5: 17  -  -  -  -  -  5  - 53  - 21 36
 *    6:  -  -  -  -  -  - 25 16  - 22  -  -
 *    7:  -  - 38  -  - 54  - 48  - 56  3  -
 *    8:  - 58  -  -  -  -  -  7 60 36  - 20
 *    9:  -  -  - 59 35  -  -  -  - 46 38 25
 *   10: 40  -  - 42  -  -  -  - 24 33 16  -
 *   11:  -  - 46  -  -  1  -  - 51  - 25  5
 * Parity part: column 12 has shift 1 in row 0, shift 0 in row 6 and shift 1 in row 11; column 13 + i (i = 0 .. 10) has
 * shift 0 in rows i and i + 1.  58 + 25 = 83 entries; row degree 7, 6 in row 6; no 4-cycles.  The parity bits are the
 * unique solution of all checks: with lambda_i the XOR of the info entries of row i and p_c column 12 + c,
 *   p_0 = XOR of all lambda_i;  p_1 = lambda_0 ^ rot(p_0, 1);  p_{i+1} = lambda_i ^ p_i ^ (p_0 if i = 6), i = 1 .. 10.
 *
 * Rates.  The above is OFDM_LDPC_RATE_1_2, the rate of a NULL or zeroed cfg.  The other rates are other base matrices of
 * the same shape: Z = 64 and 24 columns (n = 1536 at every rate), mb rows and kb = 24 - mb info columns, KI = 8 kb info
 * bytes and PB = 8 mb parity bytes per codeword (96 / 96, 128 / 64, 144 / 48, 160 / 32).  Parity part, with
 * mid = mb / 2: column kb has shift 1 in row 0, shift 0 in row mid and shift 1 in row mb - 1; column kb + 1 + i
 * (i = 0 .. mb - 2) has shift 0 in rows i and i + 1.  With p_c column kb + c:
 *   p_0 = XOR of all lambda_i;  p_1 = lambda_0 ^ rot(p_0, 1);  p_{i+1} = lambda_i ^ p_i ^ (p_0 if i = mid), i = 1 .. mb - 2
 * (at mb = 12 the recursion above).  No table has a 4-cycle.  Info parts, laid out as above:
 * OFDM_LDPC_RATE_2_3: mb = 8, kb = 16, mid = 4; 54 + 17 = 71 entries, row degrees 8, 9, 9, 9, 9, 9, 9, 9.
 *  2/3 0:  -  1 61  - 10  -  - 43  -  - 15  -  - 28  -  -
 *  2/3 1:  7 21  - 32  - 25  -  -  -  - 60  - 56  - 16  -
 *  2/3 2: 30  - 37  -  4  - 12  - 58  -  - 14  -  -  2  -
 *  2/3 3: 34  -  -  9  -  4 47  -  9  -  -  - 10  - 23  -
 *  2/3 4:  -  -  - 14  - 28  - 47  - 58  -  -  5  -  - 42
 *  2/3 5:  - 13 43  -  - 11 13  -  -  - 63 36  - 16  -  -
 *  2/3 6:  - 12  - 61 57  -  -  -  0 19  -  -  - 35  - 50
 *  2/3 7:  0  - 29  - 16  -  - 21  - 12  - 43  -  -  - 41
 * OFDM_LDPC_RATE_3_4: mb = 6, kb = 18, mid = 3; 60 + 13 = 73 entries, row degrees 12, 12, 12, 12, 13, 12.
 *  3/4 0: 40 21  5  -  -  7 42  - 18  -  - 24  0  -  5  -  - 40
 *  3/4 1:  0  - 58  - 60  1 28  -  - 27 10  - 27  - 40  - 61  -
 *  3/4 2:  -  1 39 26  - 25  - 23 43  - 29  -  - 35  - 52  - 34
 *  3/4 3:  - 40  - 13  7  - 52  -  - 21  - 51 34  -  -  2 42  -
 *  3/4 4:  8  - 21 37 47  6  - 30  -  5  -  -  - 15  6  -  3 36
 *  3/4 5: 43 17  - 10 32  -  - 44  5  - 12 50  -  5  - 58  -  -
 * OFDM_LDPC_RATE_5_6: mb = 4, kb = 20, mid = 2; 64 + 9 = 73 entries, row degrees 18, 18, 19, 18.
 *  5/6 0: 38 18 31 40 46 13  -  1 40 47 43  - 16  0 29  - 33 15 49  -
 *  5/6 1: 14 30 51 26 63  0 14  0  - 51  -  5 59 39  -  2 27  - 23 55
 *  5/6 2: 57 40 19 23  -  9 34  - 41 52 25 62  -  - 41  7 22  0 40 27
 *  5/6 3: 48 42  8 33 34  - 33 62 15  - 17 30 48 59  0 61  - 44  - 14
 * Both ends of a link are set to the same rate; no field on the air names it.
 *
 * Block.  Info bytes of an n-byte payload (0 <= n <= OFDM_LDPC_MAX_PAYLOAD): payload | CRC-32(payload) big-endian,
 * k = n + 4 bytes, bits MSB first; info byte m of a codeword holds codeword bits 8m .. 8m + 7.  W = ceil(k / 96)
 * codewords, codeword w takes info bytes [96w, min(96w + 96, k)); the last codeword is shortened: its missing info bits
 * are 0 and are not sent.  Sent, codeword after codeword: its k_w info bytes, then its 96 parity bytes.  Coded length
 * k + 96 W, strictly increasing in n; OFDM_LDPC_MAX_PAYLOAD = 2012 gives W = 21 and OFDM_LDPC_MAX_CODED = 4032.
 * A received length m is a block iff 100 <= m <= 4032 and ((m - 1) mod 192) >= 96; then W = ceil(m / 192) and
 * k = m - 96 W.  Anything else is no block: ok = 0, no payload bytes, zeros in the per-block outputs, no error for the
 * batch, and nothing of it is read.
 * At the other rates the same with KI and PB in the place of 96: W = ceil(k / KI), codeword w takes info bytes
 * [KI w, min(KI w + KI, k)) and is sent as its info bytes and then its PB parity bytes; coded length k + PB W; a full
 * codeword is 192 bytes at every rate.  OFDM_LDPC_MAX_CODED stays 4032 (W <= 21), so the largest payload is 21 KI - 4:
 * 2012, 2684, 3020, 3356.  A received length m is a block at a rate iff PB + 4 <= m <= 4032 and
 * ((m - 1) mod 192) >= PB; then W = ceil(m / 192) and k = m - PB W.
 *
 * Decoder input: one signed value v per sent bit, v > 0 means 1, v = 0 is an erasure, -128 reads as -127; shortened
 * positions read as -127; a hard byte is v = +16 / -16 per bit.
 * Decoder: layered normalised min-sum.  P_b (int) starts as v_b, R_e = 0 for every entry e and lane z.  An iteration
 * visits rows i = 0 .. mb - 1 in order; for each entry e = (i, j, s) of the row and each lane z, b = 64 j + (z + s) mod 64:
 *   1. Q_e = clamp(P_b - R_e, -127, 127)
 *   2. beta_e = (Q_e > 0); pi = XOR of the row's beta; m_e = min of |Q_e'| over the row's other entries e' != e
 *   3. mu_e = (3 m_e) >> 2
 *   4. R_e = +mu_e if (pi ^ beta_e) = 1, else -mu_e
 *   5. P_b = Q_e + R_e   (no clamp: |P| <= 222)
 * After each full iteration x_b = (P_b > 0); a codeword stops at the first iteration after which every check holds, at
 * the latest after max_iters iterations; at least one iteration always runs.
 * Per block: the n payload bytes from the decoded info bits; ok = 1 when the decoded CRC matches; corrected = sent
 * positions with v != 0 whose sign disagrees with x; iters = the largest iteration count among the block's codewords;
 * cw_failed = codewords whose last syndrome is non-zero.
 *
 * Argument order, pointer modes, errors and the offsets-before-the-capacity-check rule as ofdm_fec_*: the blobs
 * (payloads, coded, soft) are host or device pointers by the handle's mode; the offset, length, ok, corrected, iters and
 * cw_failed arrays are host memory; coded_off / payload_off OUT have nblk + 1 entries.  cfg NULL: max_iters 20 at rate
 * 1/2 (the encoder checks its cfg and ignores max_iters).  OFDM_E_INVAL: bad struct_size, max_iters outside 1 .. 64, a
 * rate above OFDM_LDPC_RATE_5_6, a non-zero reserved word behind it, a payload longer than the rate's largest (encode),
 * a null argument.  OFDM_E_CAPACITY: the output blob is too small.  There is no per-batch workspace and no slicing: a
 * batch is as many one-wave codewords as it has.
 * ofdm_rx_ldpc_decode_soft: the last ofdm_rx call's packets through ofdm_ldpc_decode_soft's decoder, the values read
 * where they lie in the handle's buffer (ofdm_set_rx_soft), as ofdm_rx_fec_decode_soft.
 * ofdm_ldpc_last_ms: HIP-event time of k_ldpc_encode / k_ldpc_decode in the last of these calls, which must have run
 * with profiling on (ofdm_prof_enable) and launched; OFDM_E_INVAL otherwise.  As ofdm_fec_last_ms. */
#define OFDM_LDPC_MAX_PAYLOAD 2012 /* at rate 1/2; 2684, 3020 and 3356 at the other rates */
#define OFDM_LDPC_MAX_CODED 4032
#define OFDM_LDPC_RATE_1_2 0
#define OFDM_LDPC_RATE_2_3 1
#define OFDM_LDPC_RATE_3_4 2
#define OFDM_LDPC_RATE_5_6 3
typedef struct ofdm_ldpc_cfg {
  uint32_t struct_size; /* = sizeof(ofdm_ldpc_cfg) */
  uint32_t max_iters;   /* 1 .. 64 */
  union {
    uint32_t reserved[6]; /* 0 behind the first word */
    uint32_t rate;        /* OFDM_LDPC_RATE_*: the word that is reserved[0]; 0 is rate 1/2 */
  };
} ofdm_ldpc_cfg; /* 32 bytes */

/* pure host functions, usable without a GPU: n + 4 + 96 W, and its inverse (OFDM_E_INVAL for a length that is no block);
 * the _rate forms take OFDM_LDPC_RATE_* first (n + 4 + PB W), the other two mean rate 1/2 */
int ofdm_ldpc_coded_len(uint32_t payload_len, uint32_t *coded_len);
int ofdm_ldpc_payload_len(uint32_t coded_len, uint32_t *payload_len);
int ofdm_ldpc_coded_len_rate(uint32_t rate, uint32_t payload_len, uint32_t *coded_len);
int ofdm_ldpc_payload_len_rate(uint32_t rate, uint32_t coded_len, uint32_t *payload_len);
int ofdm_ldpc_encode(ofdm_handle *h, const ofdm_ldpc_cfg *cfg, const uint8_t *payloads, const uint64_t *payload_off,
                     const uint32_t *payload_len, int nblk, uint8_t *coded, uint64_t coded_cap, uint64_t *coded_off);
int ofdm_ldpc_decode(ofdm_handle *h, const ofdm_ldpc_cfg *cfg, const uint8_t *coded, const uint64_t *coded_off,
                     const uint32_t *coded_len, int nblk, uint8_t *payloads, uint64_t payload_cap, uint64_t *payload_off,
                     uint8_t *ok, uint32_t *corrected, uint8_t *iters, uint32_t *cw_failed);
/* the same from int8 values, 8 per coded byte: block k holds 8 * coded_len[k] values from soft + soft_off[k] */
int ofdm_ldpc_decode_soft(ofdm_handle *h, const ofdm_ldpc_cfg *cfg, const int8_t *soft, const uint64_t *soft_off,
                          const uint32_t *coded_len, int nblk, uint8_t *payloads, uint64_t payload_cap,
                          uint64_t *payload_off, uint8_t *ok, uint32_t *corrected, uint8_t *iters, uint32_t *cw_failed);
int ofdm_rx_ldpc_decode_soft(ofdm_handle *h, const ofdm_ldpc_cfg *cfg, uint8_t *payloads, uint64_t payload_cap,
                             uint64_t *payload_off, uint8_t *ok, uint32_t *corrected, uint8_t *iters, uint32_t *cw_failed,
                             int max_pkts, int *n);
int ofdm_ldpc_last_ms(const ofdm_handle *h, double *ms);

/* --- coded links: LDPC, reliabilities out: one byte per payload byte for errors-and-erasures decoding of the outer code ---
 * ofdm_ldpc_decode_rel / ofdm_ldpc_decode_soft_rel / ofdm_rx_ldpc_decode_soft_rel return exactly what ofdm_ldpc_decode /
 * ofdm_ldpc_decode_soft / ofdm_rx_ldpc_decode_soft return for the same input (payloads, ok, corrected, iters, cw_failed),
 * and one reliability byte per decoded payload byte in the format ofdm_rs_decode_rel takes.  Additions only:
 * OFDM_ABI_VERSION stays 6, the OFDM_K_* table is unchanged, k_ldpc_decode and its launches are unchanged, and without a
 * call to these three functions nothing new launches, allocates or copies.  All arithmetic is integer: results are
 * defined bit for bit.
 *
 * Definition.  The decoder is the one above, unchanged: same schedule, same normalisation, same stop rule, same
 * max_iters.  For one codeword of a block:
 *   P[b]   the value the decoder holds for bit b when the codeword stops (after its last iteration)
 *   conv   1 if the codeword's syndrome is zero at that point, else 0: the term that otherwise adds to cw_failed
 *   q[g]   for payload byte g < n of the block, info byte m of its codeword (bits 8m .. 8m + 7):
 *            q[g] = min(127, min over i = 0 .. 7 of |P[8m + i]|) + 128 * conv
 * q lies in 0 .. 255; every byte of a codeword that failed ranks below every byte of one that converged; 255 needs a
 * converged codeword with all eight |P| >= 127 and is ofdm_rs_decode_rel's "never erase".  Nothing is produced for the
 * block's CRC bytes, the shortened positions or the parity.  Hard input (+-16) uses the same rule.  A length that is no
 * block gives ok = 0, no payload bytes and no reliability bytes: nothing of it is read or written.
 *
 * rel is a host or device pointer by the handle's mode, rel_cap its bytes; block k's n_k bytes lie at
 * rel + payload_off[k], the offsets of the payload blob.  In device-pointer mode payloads, rel and payload_off are
 * therefore ofdm_rs_decode_rel's coded, rel and coded_off with rel_off == NULL: the two layers chain without a host
 * round trip.  Errors as ofdm_ldpc_decode (ofdm_rx_ldpc_decode_soft for the third); in addition a null rel is
 * OFDM_E_INVAL, and rel_cap < payload_off[nblk] is OFDM_E_CAPACITY with the offsets set first.  After these calls
 * ofdm_ldpc_last_ms reports k_ldpc_decode_rel. */
int ofdm_ldpc_decode_rel(ofdm_handle *h, const ofdm_ldpc_cfg *cfg, const uint8_t *coded, const uint64_t *coded_off,
                         const uint32_t *coded_len, int nblk, uint8_t *payloads, uint64_t payload_cap, uint64_t *payload_off,
                         uint8_t *ok, uint32_t *corrected, uint8_t *iters, uint32_t *cw_failed, uint8_t *rel, uint64_t rel_cap);
int ofdm_ldpc_decode_soft_rel(ofdm_handle *h, const ofdm_ldpc_cfg *cfg, const int8_t *soft, const uint64_t *soft_off,
                              const uint32_t *coded_len, int nblk, uint8_t *payloads, uint64_t payload_cap,
                              uint64_t *payload_off, uint8_t *ok, uint32_t *corrected, uint8_t *iters, uint32_t *cw_failed,
                              uint8_t *rel, uint64_t rel_cap);
int ofdm_rx_ldpc_decode_soft_rel(ofdm_handle *h, const ofdm_ldpc_cfg *cfg, uint8_t *payloads, uint64_t payload_cap,
                                 uint64_t *payload_off, uint8_t *ok, uint32_t *corrected, uint8_t *iters, uint32_t *cw_failed,
                                 uint8_t *rel, uint64_t rel_cap, int max_pkts, int *n);

/* --- coded links: the signal field ---------------------------------------------------------------------------------
 * A 12-byte field in front of a coded block that names the block's coding, so that a receiver needs no setting of its
 * own and a batch can hold packets of different codings.  The field lies inside the packet's payload: header, whitening
 * and packet CRC treat it like any payload byte.  A block is field | body, OFDM_SIG_FIELD_BYTES + len(body) bytes.
 *
 * The coding word, 12 bits, MSB first:
 *   bits 11..10  codec      OFDM_SIG_CODEC_NONE, _FEC (the convolutional code), _LDPC; 3 is reserved
 *   bits  9..8   rate id    OFDM_FEC_RATE_* / OFDM_LDPC_RATE_* (0 .. 3); 0 with OFDM_SIG_CODEC_NONE
 *   bit   7      the Reed-Solomon outer code is present
 *   bits  6..4   log2 of the convolutional interleaver's column count, 0 .. 4; 0 for the other codecs
 *   bits  3..0   reserved, zero
 * 2 + 40 + 8 = 50 words are valid.
 *
 * The codeword of a word w, extended Golay (24,12,8): the 12 word bits MSB first, then the 11 bits of the remainder of
 * w(x) x^11 modulo g(x) = x^11 + x^10 + x^6 + x^5 + x^4 + x^2 + 1 (0xC75), then one bit that makes the weight even.
 * The field is four copies of the codeword: field bit t (0 .. 95, MSB first within a byte) is codeword bit t mod 24.
 *
 * Decoding is exhaustive maximum likelihood in integers.  v_t is the value of field bit t (soft: the int8 value, v > 0
 * means 1, 0 is an erasure, -128 reads as -127; hard: +1 / -1 from the bit), c_j = v_j + v_(j+24) + v_(j+48) + v_(j+72),
 * m(w) = sum over j of c_j * (+1 where bit j of w's codeword is 1, else -1).  `word` is the w with the largest m, the
 * smallest such w on a tie, whether valid or not (ofdm_sig_word_valid tells); `margin` is m(word) minus the largest m
 * of any other w, 0 .. 24384.  A packet shorter than 12 bytes gives word OFDM_SIG_NO_WORD and margin 0.
 *
 * ofdm_sig_word packs a word (interleave_cols: 1, 2, 4, 8 or 16 with OFDM_SIG_CODEC_FEC, 0 or 1 otherwise),
 * ofdm_sig_word_fields unpacks one (interleave_cols 0 where the codec has none), ofdm_sig_word_valid returns 1 or 0;
 * the first two return OFDM_E_INVAL for what is no valid word.  None of the three needs a handle or a GPU.
 *
 * ofdm_sig_encode: block k of `out`, at out_off[k], is the field of words[k] followed by the body_len[k] bytes at
 * bodies + body_off[k]; out_off has nblk + 1 entries and is set before the capacity is checked.  `bodies` and `out` are
 * host or device pointers by the handle's mode; words, offsets and lengths are host arrays.  An invalid word is
 * OFDM_E_INVAL, out_cap < out_off[nblk] OFDM_E_CAPACITY.  Ordered with ofdm_tx like the other encode calls.
 *
 * ofdm_sig_decode (hard bytes) / ofdm_sig_decode_soft (int8 values, 8 per byte, soft_off in values, len in bytes):
 * word[k] and margin[k] (host arrays) of the packet of len[k] bytes at off[k]; only the field is read.
 * ofdm_rx_sig_decode_soft does the same for the packets of the last ofdm_rx from the handle's own soft values
 * (ofdm_set_rx_soft), *n of them; max_pkts < *n is OFDM_E_CAPACITY with *n set.  ofdm_sig_last_ms: the HIP-event time
 * of k_sig_encode / k_sig_decode in the last of these calls (ofdm_prof_enable), OFDM_E_INVAL if it was not timed. */
#define OFDM_SIG_FIELD_BYTES 12
#define OFDM_SIG_CODEC_NONE 0
#define OFDM_SIG_CODEC_FEC 1
#define OFDM_SIG_CODEC_LDPC 2
#define OFDM_SIG_NO_WORD 0xFFFF
int ofdm_sig_word(uint32_t codec, uint32_t rate, uint32_t rs, uint32_t interleave_cols, uint16_t *word);
int ofdm_sig_word_fields(uint32_t word, uint32_t *codec, uint32_t *rate, uint32_t *rs, uint32_t *interleave_cols);
int ofdm_sig_word_valid(uint32_t word);
int ofdm_sig_encode(ofdm_handle *h, const uint16_t *words, const uint8_t *bodies, const uint64_t *body_off,
                    const uint32_t *body_len, int nblk, uint8_t *out, uint64_t out_cap, uint64_t *out_off);
int ofdm_sig_decode(ofdm_handle *h, const uint8_t *in, const uint64_t *off, const uint32_t *len, int nblk, uint16_t *word,
                    uint16_t *margin);
int ofdm_sig_decode_soft(ofdm_handle *h, const int8_t *soft, const uint64_t *soft_off, const uint32_t *len, int nblk,
                         uint16_t *word, uint16_t *margin);
int ofdm_rx_sig_decode_soft(ofdm_handle *h, uint16_t *word, uint16_t *margin, int max_pkts, int *n);
int ofdm_sig_last_ms(const ofdm_handle *h, double *ms);

/* --- chunked streams -------------------------------------------------------------
 * ofdm_rx treats each call as one stream that starts at its first sample (filter and
 * correlator history zero, detector average 0, NCO phase 0), as the reference's flow graph
 * does at start-up.  A continuous capture is fed in overlapping chunks; these three entry
 * points give the caller what it needs to stitch them so that the result equals one call on
 * the whole capture (ofdm_uhd_amd/ofdm.py: ofdm_demod.feed / flush do exactly that):
 *  - the flag sample (last sample of the preamble symbol, relative to the call's iq) of every
 *    packet the last call delivered, in delivery order;
 *  - the flags of the last call with the NCO phase and per-sample phase step in force from
 *    each flag on: phi[n] = phase_j + step_j * (n - flag_j + 1)  (gr_frequency_modulator_fc
 *    driven by the sample-and-held sync angle, ofdm_receiver.py~:97-124).  phase_j is an
 *    integer, units of 2^-64 turn: phases add modulo one turn without rounding, which is what
 *    makes chunked and one-shot processing agree to the last bit; swallowed_j != 0 says the
 *    flag's frame was consumed as payload of a packet that began at an earlier flag;
 *  - the settled past for the following calls: the flags at or before trust_after (relative to
 *    the next call's iq, ascending, inside it) that earlier calls found, with their phase
 *    steps and swallowed marks -- they replace whatever that call detects up to trust_after, in the start of its
 *    overlap where its own detector has not settled -- and the NCO line (phase, step at
 *    pred_flag, which may be negative) of the flag before them, in force up to the call's
 *    first flag.  enable = 0 returns to independent calls.
 *  - ofdm_rx_set_origin: index, in the whole capture, of the first sample the following ofdm_rx calls are
 *    given (default 0).  gr_fft_filter_ccc (ofdm_receiver.py~:76) works in blocks that start at multiples of its
 *    block length counted from the first sample the flow graph ever saw; the engine lays its filter blocks on
 *    that same grid, so a capture handed over in pieces is filtered exactly as one call would filter it. */
int ofdm_rx_set_origin(ofdm_handle *h, uint64_t first_sample_index);
/* Pipelining across batches (one handle = a transmit stream and a receive stream on the GPU): ofdm_rx_submit queues
 * the receiver's input stage (the wait for the transmit batch that fills iq, the channel filter) and returns at
 * once; an ofdm_tx_async issued next is queued behind that stage only -- it may refill the same iq buffer -- and runs
 * while the following ofdm_rx(h, iq, nsamples, ...) (same arguments: it picks the submitted stage up) is busy with
 * its own kernels and host round trips.  Optional: ofdm_rx alone does the same work in order.
 * Exception: with OFDM_SYNC_FIXED (chan_filt is the input itself) or a fused sensor (ofdm_set_rx_sense) the receiver
 * reads iq until the end of ofdm_rx; between ofdm_rx_submit and that ofdm_rx a transmit call whose iq_out overlaps
 * the submitted buffer is refused with OFDM_E_INVAL (transmit into another buffer, or after ofdm_rx). */
int ofdm_rx_submit(ofdm_handle *h, const ofdm_c32 *iq, uint64_t nsamples);
int ofdm_rx_packet_pos(ofdm_handle *h, uint64_t *pos, int cap, int *n);
int ofdm_rx_nco_state(ofdm_handle *h, uint64_t *flags, uint64_t *phase, double *step, uint8_t *swallowed,
                      int cap, int *n);
int ofdm_rx_set_flag_history(ofdm_handle *h, int enable, int n, const int64_t *flags, const double *steps,
                             const uint8_t *swallowed, int64_t trust_after, int64_t pred_flag, uint64_t pred_phase, double pred_step);

/* --- debug taps: the reference's --log probe points (ofdm.py:123-131,253-254;
 *     ofdm_receiver.py~:144-152).  Enable before the call, read after.  Output
 *     is always copied to HOST memory. ---------------------------------------- */
enum {
  OFDM_TAP_TX_PACKETS = 0,   /* uint8: framed packets, concatenated                               */
  OFDM_TAP_TX_FREQ = 1,      /* c32[nsym][N]: ofdm_preambles.dat (mapper+preamble output)        */
  OFDM_TAP_RX_CHAN_FILT = 2, /* c32[nsamples]: ofdm_receiver-chan_filt_c.dat                      */
  OFDM_TAP_RX_METRIC = 3,    /* f32[nsamples]: peak-detector input (M-bar - 1)                    */
  OFDM_TAP_RX_PEAKS = 4,     /* u64[npeaks]: timing-flag sample indices                           */
  OFDM_TAP_RX_ANGLES = 5,    /* f32[npeaks]: sample-and-held angle(P) at each flag                */
  OFDM_TAP_RX_FRAMES = 6,    /* u64[nframes][2]: (flag index, data symbols emitted) per sampler frame */
  OFDM_TAP_RX_FFT = 7,       /* c32[nsym][N]: ofdm_receiver-fft_out_c.dat                         */
  OFDM_TAP_RX_ACQ = 8,       /* c32[nsym][occ]: ofdm_receiver-frame_acq_c.dat                     */
  OFDM_TAP_RX_SINK = 9,      /* c32[ndemapped][occ]: ofdm_frame_sink_c.dat (derotated carriers)   */
  OFDM_TAP_RX_PACKETS = 10,  /* uint8: frame-sink messages before dewhitening, concatenated      */
  OFDM_TAP_TX_MAPPER = 11,   /* c32[ndata][N]: ofdm_mapper_c.dat (mapper output: data symbols only, ofdm.py:124) */
  OFDM_TAP_TX_IFFT = 12,     /* c32[nsym][N]: ofdm_ifft_c.dat (transform output before the cyclic prefix, ofdm.py:128) */
  OFDM_TAP_RX_SAMPLER = 13,  /* c32[nsym][N]: ofdm_receiver-sampler_c.dat (the sampled, derotated symbols = FFT input) */
  OFDM_TAP_RX_SIGMIX = 14,   /* c32[nsamples]: ofdm_receiver-sigmix_c.dat (chan_filt * nco, whole stream)  */
  OFDM_TAP_RX_NCO = 15,      /* c32[nsamples]: ofdm_receiver-nco_c.dat (frequency_modulator_fc output)     */
  OFDM_TAP_RX_PRESEL = 16,   /* f32[nsamples]: the float32 pre-selection of the timing metric (engine-internal stage, DESIGN.md
                              * section 2: it picks the ranges the normative metric is evaluated on and feeds the peak
                              * detector's running average outside them); no reference probe point */
  OFDM_TAP_RX_DEMAPPED = 17, /* u8[nsym]: 1 where the frame sink demapped the symbol (row of RX_FFT / RX_ACQ / RX_SAMPLER): the rows
                              * OFDM_TAP_RX_SINK holds, in order.  Needs OFDM_TAP_RX_SINK enabled. */
  OFDM_TAP_RX_RUN_AVG = 18,  /* f64[nruns][2]: (first sample, detector average there) of every run of candidates the peak
                              * detector walks, by first sample; the average is the float32 value its state machine starts
                              * from (engine-internal stage); no reference probe point */
  OFDM_TAP_COUNT = 19
};
/* SIGMIX / NCO evaluate the NCO's closed form sample by sample over the whole stream; inside the symbols the
 * sampler picks, the receiver itself advances the same phasor by a float64 recurrence: RX_SAMPLER is
 * bit for bit what the FFT consumed, RX_SIGMIX may differ from it in the last float32 bit. */
int ofdm_set_taps(ofdm_handle *h, uint32_t tap_mask); /* bit i enables OFDM_TAP_i */
int ofdm_tap(ofdm_handle *h, int tap, void *out_host, uint64_t cap_bytes, uint64_t *nbytes);

/* --- measurement: per-kernel HIP-event timing on the handle's stream -------- */
enum {
  OFDM_K_FRAME = 0, /* make_packet: CRC-32 + header + whitening              */
  OFDM_K_TX = 1,    /* map + preamble + IFFT + CP + scale (+channel)         */
  OFDM_K_CHAN = 2,  /* standalone channel                                    */
  OFDM_K_SYNC = 3,  /* Schmidl-Cox metric, float32 pre-selection (streaming) */
  OFDM_K_PEAK = 4,  /* peak detector / sampler / NCO bookkeeping             */
  OFDM_K_DEMOD = 5, /* derotate + FFT + frame acquisition + frame sink       */
  OFDM_K_DEFRAME = 6, /* dewhiten + CRC check + output compaction            */
  OFDM_K_SENSE = 7, /* windowed FFT + |.|^2 + max-hold (+ decision tail)    */
  OFDM_K_FILTER = 8, /* channel filter (overlap-save transforms, streaming)  */
  OFDM_K_EXACT = 9,  /* fixed-point metric + candidates where the pre-selection fired */
  OFDM_K_FRONT = 10, /* fused front end: channel filter + float32 pre-selection in one pass (replaces FILTER + SYNC) */
  OFDM_K_COUNT = 11
};
int ofdm_prof_enable(ofdm_handle *h, int on);
int ofdm_prof_reset(ofdm_handle *h);
int ofdm_prof_get(ofdm_handle *h, int kernel, double *total_ms, uint64_t *launches);
const char *ofdm_kernel_name(int kernel);

#ifdef __cplusplus
}
#endif
#endif /* OFDM_HIP_H */
