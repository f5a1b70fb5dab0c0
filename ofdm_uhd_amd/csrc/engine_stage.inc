// engine_stage.inc -- what the host sides of the ten wideband stream stages share (StreamStage, host_util.h): the
// steps of a configure call and its per-link checks and tables, reset, the argument checks, timing, the launch, the
// history roll, the choice of a transmit kernel's <OUT, ADD>, the end of a call, and host-mode staging, one function
// per step of the four call shapes:
//   receive single (ddc, resamp) and bank (ddc_bank, resamp_bank, pfb; `rows` runs at the caller's stride):
//     stage_rx_in, stage_rx_out, [launch], stage_roll_rx_history, stage_rx_readback
//   transmit single (duc, tx_resamp) and bank (duc_bank, tx_resamp_bank, pfb_synth; `rows` runs in):
//     stage_tx_rows_in, stage_tx_out, [launch], stage_roll_history / stage_roll_rows_history, stage_tx_readback
// A staging step leaves the caller's pointers (device mode) as they are and, in host mode, puts the stage's device
// copy in their place.  Included by engine.hip ahead of engine_{ddc,ddc_bank,duc,resamp,resamp_bank,tx_resamp,pfb,
// pfb_synth,duc_bank,tx_resamp_bank}.inc (in that order: a bank uses its single stage's index limit), which keep what
// is a stage's own: its configuration checks and messages, its index limits, its output count, its Params and its
// template dispatch.  engine_multipath.inc, the propagation channel stage, engine_cfr.inc, the crest-factor reduction
// stage, and engine_mempoly.inc, the memory-polynomial stage, follow them with the transmit single shape; the last two
// keep statistics (stream_stats.h) through the stage_stats_* steps below.  engine_psd.inc, the spectrum stage, uses the
// skeleton's arm, reset, enter, time, history-roll and finish steps; it has no sample output and stages its own input.

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
// the tables of a bank's K links, one after the other (link i's at [i * ntaps], as ofdm_*_bank_taps returns it)
static std::vector<c32> bank_tables(const float* taps, int ntaps, const double* fcs, int K, int L) {
  std::vector<c32> tab;
  for (int i = 0; i < K; i++) {
    const std::vector<c32> c = bandpass_table(taps, ntaps, fcs[i], L);
    tab.insert(tab.end(), c.begin(), c.end());
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

// nlinks and the n centre frequencies of a configuration (`who` begins the messages, `per` ends the second: the
// receive stages count cycles per "sample", the transmit stages per "output sample")
static int stage_check_nlinks(ofdm_handle* h, const char* who, uint32_t nlinks) {
  static_assert(OFDM_DDC_BANK_MAX_LINKS == 8 && OFDM_RESAMP_BANK_MAX_LINKS == 8 && OFDM_DUC_BANK_MAX_LINKS == 8 &&
                    OFDM_TX_RESAMP_BANK_MAX_LINKS == 8,
                "the message below names the limit");
  if (nlinks < 1 || nlinks > 8) FAIL(h, OFDM_E_INVAL, std::string(who) + " nlinks must be in [1, 8]");
  return OFDM_OK;
}
static int stage_check_center_freqs(ofdm_handle* h, const char* who, const double* fc, uint32_t n, const char* per) {
  for (uint32_t i = 0; i < n; i++)
    if (!(fabs(fc[i]) <= 0.5)) FAIL(h, OFDM_E_INVAL, std::string(who) + " center_freq must be in [-0.5, 0.5] cycles per " + per);
  return OFDM_OK;
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

// the table of one link of a bank (tab: bank_tables)
static int stage_bank_taps(bool on, const std::vector<c32>& tab, int ntaps, int K, int link, ofdm_c32* out, int cap, int* n) {
  if (!on || link < 0 || link >= K) return OFDM_E_INVAL;
  return stage_taps_out(tab.data() + (size_t)link * ntaps, ntaps, out, cap, n);
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

// host mode of a receive stage: the call's input into d.d_in
static int stage_rx_in(ofdm_handle* h, StreamStage& d, const void* iq_in, uint64_t nin, const void** d_in) {
  if (h->dev_ptrs) return OFDM_OK;
  RCCHK(stage_upload(h, d.d_in, iq_in, nin * rx_ss(h)));
  *d_in = d.d_in.p;
  return OFDM_OK;
}
// ... its `rows` runs of `no` outputs into d.d_out, one behind the other (rows = 1: stride may be NULL) ...
static int stage_rx_out(ofdm_handle* h, StreamStage& d, uint64_t rows, uint64_t no, c32** d_out, uint64_t* stride) {
  if (h->dev_ptrs || !no) return OFDM_OK;
  HIPCHK(h, d.d_out.ensure(rows * no * sizeof(c32)));
  *d_out = d.d_out.as<c32>();
  if (stride) *stride = no;
  return OFDM_OK;
}
// ... and from there into the caller's buffer, run i at iq_out + i * caller_stride
static int stage_rx_readback(ofdm_handle* h, ofdm_c32* iq_out, uint64_t caller_stride, uint64_t rows, uint64_t no, const c32* d_out) {
  if (h->dev_ptrs || !no) return OFDM_OK;
  for (uint64_t i = 0; i < rows; i++)
    HIPCHK(h, hipMemcpyAsync(iq_out + i * caller_stride, d_out + i * no, no * sizeof(c32), hipMemcpyDeviceToHost, h->stream));
  return OFDM_OK;
}

// host mode of a transmit stage: the `rows` runs of `nin` inputs, run i at iq_in + i * caller_stride, into d.d_in one
// behind the other (rows = 1: stride may be NULL)
static int stage_tx_rows_in(ofdm_handle* h, StreamStage& d, const ofdm_c32* iq_in, uint64_t caller_stride, uint64_t rows, uint64_t nin,
                            const c32** d_in, uint64_t* stride) {
  if (h->dev_ptrs) return OFDM_OK;
  HIPCHK(h, d.d_in.ensure(rows * nin * sizeof(c32)));
  for (uint64_t i = 0; i < rows; i++)
    HIPCHK(h, hipMemcpyAsync(d.d_in.as<c32>() + i * nin, iq_in + i * caller_stride, nin * sizeof(c32), hipMemcpyHostToDevice, h->stream));
  *d_in = d.d_in.as<c32>();
  if (stride) *stride = nin;
  return OFDM_OK;
}
// ... the band to add onto, where one is given, into d.d_add, and room for the `no` outputs of `oss` bytes in d.d_out
// (a stage whose call may complete no output asks for this step only where no > 0) ...
static int stage_tx_out(ofdm_handle* h, StreamStage& d, const ofdm_c32* add, uint64_t no, size_t oss, const c32** d_add, void** d_out) {
  if (h->dev_ptrs) return OFDM_OK;
  if (add) {
    RCCHK(stage_upload(h, d.d_add, add, no * sizeof(c32)));
    *d_add = d.d_add.as<c32>();
  }
  HIPCHK(h, d.d_out.ensure(no * oss));
  *d_out = d.d_out.p;
  return OFDM_OK;
}
// ... and the outputs into the caller's buffer (asked for as stage_tx_out is)
static int stage_tx_readback(ofdm_handle* h, void* iq_out, const void* d_out, uint64_t no, size_t oss) {
  if (h->dev_ptrs) return OFDM_OK;
  HIPCHK(h, hipMemcpyAsync(iq_out, d_out, no * oss, hipMemcpyDeviceToHost, h->stream));
  return OFDM_OK;
}

// a launch may have 2^31 - 1 workgroups (`who`: the entry point)
static int stage_check_grid(ofdm_handle* h, const char* who, uint64_t grid) {
  if (grid > 0x7FFFFFFFull) FAIL(h, OFDM_E_INVAL, std::string(who) + ": call too long (split it)");
  return OFDM_OK;
}

// a stage's compute kernel; tables of many links and long filters take a workgroup past the default 64 KB of dynamic
// LDS, and the limit is raised first
template <typename P>
static int stage_launch(ofdm_handle* h, void (*kernel)(P), unsigned grid, unsigned threads, size_t lds, const P& p) {
  if (lds > 64 * 1024)
    HIPCHK(h, hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(threads), lds, h->stream, p);
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

// a transmit bank: the last Q inputs of each of the `rows` runs at x + i * stride
static int stage_roll_rows_history(ofdm_handle* h, StreamStage& d, const c32* x, uint64_t stride, uint64_t nin, int Q, int rows) {
  if (Q <= 0) return OFDM_OK;
  hipLaunchKernelGGL(k_stream_hist_rows, dim3((unsigned)((Q + 255) / 256), (unsigned)rows), dim3(256), 0, h->stream, x, stride, nin,
                     d.d_hist[d.cur].as<c32>(), d.d_hist[d.cur ^ 1].as<c32>(), Q);
  HIPCHK(h, hipGetLastError());
  return OFDM_OK;
}

// the statistics of the stages that keep some (stream_stats.h): zero the totals; room for a call's `grid` partials (two
// levels of k_stat_reduce add at most STAT_REDUCE_SPAN^2 of them: stage_stats_fits, asked before anything moves); the
// reduction behind the compute kernel; the totals on the host
static int stage_stats_zero(ofdm_handle* h, StatState& st) {
  HIPCHK(h, st.d_tot.ensure(sizeof(StatTotals)));
  HIPCHK(h, hipMemsetAsync(st.d_tot.p, 0, sizeof(StatTotals), h->stream));
  st.n = 0;
  return OFDM_OK;
}
static bool stage_stats_fits(uint64_t grid) { return grid <= (uint64_t)STAT_REDUCE_SPAN * STAT_REDUCE_SPAN; }
static int stage_stats_room(ofdm_handle* h, StatState& st, uint64_t grid) {
  HIPCHK(h, st.d_part.ensure(sizeof(StatPartial) * grid));
  if (grid > (uint64_t)STAT_REDUCE_SPAN)
    HIPCHK(h, st.d_part2.ensure(sizeof(StatPartial) * ((grid + STAT_REDUCE_SPAN - 1) / STAT_REDUCE_SPAN)));
  return OFDM_OK;
}
static void stage_stats_reduce(ofdm_handle* h, StatState& st, uint64_t grid) {
  const StatPartial* parts = st.d_part.as<StatPartial>();
  uint32_t nparts = (uint32_t)grid;
  if (grid > (uint64_t)STAT_REDUCE_SPAN) {
    const uint32_t groups = (uint32_t)((grid + STAT_REDUCE_SPAN - 1) / STAT_REDUCE_SPAN);
    hipLaunchKernelGGL(k_stat_reduce<false>, dim3(groups), dim3(STAT_THREADS), 0, h->stream, parts, nparts, st.d_part2.as<StatPartial>(),
                       (StatTotals*)nullptr);
    parts = st.d_part2.as<StatPartial>();
    nparts = groups;
  }
  hipLaunchKernelGGL(k_stat_reduce<true>, dim3(1), dim3(STAT_THREADS), 0, h->stream, parts, nparts, (StatPartial*)nullptr,
                     st.d_tot.as<StatTotals>());
}
static int stage_stats_read(ofdm_handle* h, StatState& st, StatTotals* t) {
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  HIPCHK(h, hipMemcpyAsync(t, st.d_tot.p, sizeof(*t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return OFDM_OK;
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
