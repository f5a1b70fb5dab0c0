// engine_stage.inc -- what the host sides of the ten wideband stream stages share (StreamStage, host_util.h): the
// steps of a configure call, reset, the argument checks, host-mode staging, timing, the history roll, the choice of a
// transmit kernel's <OUT, ADD> and the end of a call.  Included by engine.hip ahead of
// engine_{ddc,ddc_bank,pfb,resamp,resamp_bank,duc,duc_bank,pfb_synth,tx_resamp,tx_resamp_bank}.inc, which keep what is a stage's own: its
// configuration checks and messages, its table, its index limits, its output count and its launch.

#define RCCHK(expr)         \
  do {                      \
    int _rc = (expr);       \
    if (_rc) return _rc;    \
  } while (0)

// frac(cycles) in units of 2^-64 turn: the integer-turn convention of nco_turns (rx_demod.h)
static uint64_t ddc_turns(double cycles) {
  double t = cycles - floor(cycles);
  if (!(t < 1.0)) t = 0.0;  // a tiny negative product rounds up to a whole turn: phase 0
  return (uint64_t)(t * 18446744073709551616.0);  // t < 1: exact scaling, no overflow
}

// c[k] = complex64(h[k] exp(j 2 pi fc k / L)): float64, rounded once (L = 1, the DDC and the bank: the division is exact)
static std::vector<c32> bandpass_table(const float* taps, int ntaps, double fc, int L) {
  std::vector<c32> tab(ntaps);
  for (int k = 0; k < ntaps; k++) {
    const double a = 2.0 * M_PI * fc * (double)k / (double)L;
    tab[k] = c32{(float)((double)taps[k] * cos(a)), (float)((double)taps[k] * sin(a))};
  }
  return tab;
}

// the first output n whose newest input floor(n M / L) is at or behind a: ceil(a L / M).  (L = 1, M = R: the DDC's
// outputs m with m R >= a.)  Nothing overflows: the DDC and the bank have L = 1, so a L is a for every a; the
// resamplers keep a <= 2^57 (RESAMP_MAX_INDEX twice) and L <= 64, so a L <= 2^63; and the quotient is rounded up
// without adding to a L.
static uint64_t first_output(uint64_t a, uint64_t L, uint64_t M) {
  const uint64_t p = a * L;
  return p / M + (p % M ? 1 : 0);
}

static bool taps_finite(const float* taps, uint32_t ntaps) {
  for (uint32_t k = 0; k < ntaps; k++)
    if (!std::isfinite(taps[k])) return false;
  return true;
}

// out_format / out_scale of the transmit stages (`who` begins their messages): the full scale in force
static int stage_out_scale(ofdm_handle* h, const char* who, uint32_t out_format, float out_scale, float* scale) {
  if (out_format != OFDM_IQ_FC32 && out_format != OFDM_IQ_SC16) FAIL(h, OFDM_E_INVAL, std::string("unknown ") + who + " out_format");
  *scale = 32768.0f;
  if (out_format == OFDM_IQ_SC16 && out_scale != 0.0f) {
    if (!(std::isfinite(out_scale) && out_scale > 0.0f))
      FAIL(h, OFDM_E_INVAL, std::string(who) + " out_scale must be finite and positive (0: 2^15)");
    *scale = out_scale;
  }
  return OFDM_OK;
}

// set_*(NULL): touches no device memory
static int stage_off(StreamStage& d) {
  d.on = false;
  d.next = 0;
  d.timed = false;
  return OFDM_OK;
}

static int stage_zero_history(ofdm_handle* h, StreamStage& d) {
  const size_t bytes = sizeof(c32) * (size_t)std::max(d.hist, 1);
  for (int i = 0; i < 2; i++) HIPCHK(h, hipMemsetAsync(d.d_hist[i].p, 0, bytes, h->stream));
  d.cur = 0;
  return OFDM_OK;
}

// a configure call, once its arguments are checked: stage_disarm, the stage's own fields and uploads, stage_arm
static int stage_disarm(ofdm_handle* h, StreamStage& d) {
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  HIPCHK(h, hipStreamSynchronize(h->stream));  // a call in flight may still read the old table
  d.on = false;
  return OFDM_OK;
}
static int stage_arm(ofdm_handle* h, StreamStage& d, int hist) {
  d.hist = hist;
  for (int i = 0; i < 2; i++) HIPCHK(h, d.d_hist[i].ensure(sizeof(c32) * (size_t)std::max(d.hist, 1)));
  RCCHK(stage_zero_history(h, d));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  d.next = 0;
  d.timed = false;
  d.on = true;
  return OFDM_OK;
}

static int stage_reset(ofdm_handle* h, StreamStage& d, uint64_t first) {
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  RCCHK(stage_zero_history(h, d));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  d.next = first;
  return OFDM_OK;
}

static int stage_last_ms(const StreamStage& d, double* ms) {
  if (!ms || !d.timed) return OFDM_E_INVAL;
  *ms = d.last_ms;
  return OFDM_OK;
}

// a table of ntaps entries out: *n alone where out is NULL
static int stage_taps_out(const c32* tab, int ntaps, ofdm_c32* out, int cap, int* n) {
  *n = ntaps;
  if (!out) return OFDM_OK;
  if (cap < ntaps) return OFDM_E_CAPACITY;
  memcpy(out, tab, sizeof(c32) * (size_t)ntaps);
  return OFDM_OK;
}

// the caller's input of a receive stage, in the handle's receive format
static int stage_check_rx_in(ofdm_handle* h, const void* iq_in, uint64_t nin) {
  const bool s16 = h->rx_fmt == OFDM_IQ_SC16;
  if (nin && !iq_in) FAIL(h, OFDM_E_INVAL, "null iq_in");
  if (s16 && ((uintptr_t)iq_in & 3u)) FAIL(h, OFDM_E_INVAL, "ofdm_sc16 buffers must be 4-byte aligned");
  if (!s16 && ((uintptr_t)iq_in & 7u)) FAIL(h, OFDM_E_INVAL, "float32 IQ buffers must be 8-byte aligned");
  return OFDM_OK;
}

// the caller's buffers of a transmit stage: complex64 in and add, out in the stage's output format
static int stage_check_tx_bufs(ofdm_handle* h, bool s16, const void* iq_in, uint64_t nin, const void* add, const void* iq_out) {
  if (nin && !iq_in) FAIL(h, OFDM_E_INVAL, "null iq_in");
  if (((uintptr_t)iq_in & 7u) || ((uintptr_t)add & 7u)) FAIL(h, OFDM_E_INVAL, "float32 IQ buffers must be 8-byte aligned");
  if (s16 && ((uintptr_t)iq_out & 3u)) FAIL(h, OFDM_E_INVAL, "ofdm_sc16 buffers must be 4-byte aligned");
  if (!s16 && ((uintptr_t)iq_out & 7u)) FAIL(h, OFDM_E_INVAL, "float32 IQ buffers must be 8-byte aligned");
  return OFDM_OK;
}

// a transmit call's output format and whether it adds onto a band, as the <OUT, ADD> of its kernel:
// f(OUT(), std::bool_constant<ADD>())
template <typename F>
static auto stage_tx_variant(bool s16, bool add, F f) {
  if (s16) return add ? f(sc16{}, std::true_type{}) : f(sc16{}, std::false_type{});
  return add ? f(c32{}, std::true_type{}) : f(c32{}, std::false_type{});
}

// the first device work of a call: a transmit batch still in flight (ofdm_tx_async) may be writing the caller's input
static int stage_enter(ofdm_handle* h) {
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  if (h->tx_pending && h->txs != h->stream) HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_tx_done, 0));
  return OFDM_OK;
}

// host mode: a caller's buffer into the stage's device copy
static int stage_upload(ofdm_handle* h, DevBuf& b, const void* src, size_t bytes) {
  HIPCHK(h, b.ensure(bytes));
  HIPCHK(h, hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, h->stream));
  return OFDM_OK;
}

// the HIP-event pair around a stage's compute kernel, created with the first timed call
static int stage_time_begin(ofdm_handle* h, StreamStage& d, bool timing) {
  if (!timing) return OFDM_OK;
  if (!d.ev_a) {
    HIPCHK(h, hipEventCreate(&d.ev_a));
    HIPCHK(h, hipEventCreate(&d.ev_b));
  }
  HIPCHK(h, hipEventRecord(d.ev_a, h->stream));
  return OFDM_OK;
}
static int stage_time_end(ofdm_handle* h, StreamStage& d, bool timing) {
  if (timing) HIPCHK(h, hipEventRecord(d.ev_b, h->stream));
  HIPCHK(h, hipGetLastError());
  return OFDM_OK;
}

// the last d.hist samples after this call into the other history buffer (x: the call's input on the device)
template <typename XT>
static int stage_roll_history(ofdm_handle* h, StreamStage& d, const XT* x, uint64_t nin, float scale) {
  if (d.hist <= 0) return OFDM_OK;
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_stream_hist<XT>), dim3((unsigned)((d.hist + 255) / 256)), dim3(256), 0, h->stream, x, nin,
                     d.d_hist[d.cur].as<c32>(), d.d_hist[d.cur ^ 1].as<c32>(), d.hist, scale);
  HIPCHK(h, hipGetLastError());
  return OFDM_OK;
}
// a receive stage: x is in the handle's receive format
static int stage_roll_rx_history(ofdm_handle* h, StreamStage& d, const void* x, uint64_t nin) {
  if (h->rx_fmt == OFDM_IQ_SC16) return stage_roll_history(h, d, static_cast<const sc16*>(x), nin, h->rx_scale);
  return stage_roll_history(h, d, static_cast<const c32*>(x), nin, h->rx_scale);
}

// the end of a call: everything queued is done, the new history is the current one, the stream has moved on
static int stage_finish(ofdm_handle* h, StreamStage& d, uint64_t nin, bool timing) {
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (d.hist > 0) d.cur ^= 1;
  d.next += nin;
  if (timing) {
    float ms = 0.f;
    HIPCHK(h, hipEventElapsedTime(&ms, d.ev_a, d.ev_b));
    d.last_ms = (double)ms;
    d.timed = true;
  }
  return OFDM_OK;
}
