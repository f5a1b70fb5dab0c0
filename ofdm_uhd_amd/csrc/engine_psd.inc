// engine_psd.inc -- host side of the spectrum stage (psd.h): configuration, launch, the accumulators.  Included by
// engine.hip after engine_mempoly.inc; like the stages before it, it uses the stream skeleton of engine_stage.inc (arm,
// reset, enter, time, history roll, finish).  Its input format is the configuration's own, and it has no sample output:
// host mode stages the input and, where asked for, the rows.

template <int F>
static void psd_launch_n(const PsdParams& p, unsigned grid, bool in16, hipStream_t s) {
  if (in16) {
    if (sense_lds_bytes(F) > 64 * 1024)
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_psd<F, sc16>), hipFuncAttributeMaxDynamicSharedMemorySize, sense_lds_bytes(F));
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_psd<F, sc16>), dim3(grid), dim3(sense_threads(F)), sense_lds_bytes(F), s, p);
  } else {
    if (sense_lds_bytes(F) > 64 * 1024)
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_psd<F, c32>), hipFuncAttributeMaxDynamicSharedMemorySize, sense_lds_bytes(F));
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_psd<F, c32>), dim3(grid), dim3(sense_threads(F)), sense_lds_bytes(F), s, p);
  }
}

static int psd_zero_totals(ofdm_handle* h, PsdState& d) {
  HIPCHK(h, hipMemsetAsync(d.d_sum.p, 0, sizeof(double) * (size_t)d.F, h->stream));
  HIPCHK(h, hipMemsetAsync(d.d_peak.p, 0, sizeof(float) * (size_t)d.F, h->stream));
  d.nseg = 0;
  return OFDM_OK;
}

extern "C" int ofdm_set_psd(ofdm_handle* h, const ofdm_psd_cfg* cfg) {
  if (!h) return OFDM_E_INVAL;
  PsdState& d = h->psd;
  if (!cfg) return stage_off(d);
  if (cfg->struct_size != sizeof(ofdm_psd_cfg)) FAIL(h, OFDM_E_INVAL, "ofdm_psd_cfg.struct_size does not match this library");
  static_assert(OFDM_PSD_MAX_FFT == PSD_MAX_FFT && OFDM_PSD_MAX_FFT == OFDM_SENSE_MAX_FFT, "the lengths k_sense instantiates");
  if (!psd_fft_ok(cfg->nfft)) FAIL(h, OFDM_E_INVAL, "psd nfft must be a power of two in [64, 4096]");
  if (cfg->hop < 1 || cfg->hop > cfg->nfft) FAIL(h, OFDM_E_INVAL, "psd hop must be in [1, nfft]");
  if (cfg->in_format != OFDM_IQ_FC32 && cfg->in_format != OFDM_IQ_SC16) FAIL(h, OFDM_E_INVAL, "unknown psd in_format");
  float scale = 1.0f / 32768.0f;
  if (cfg->in_format == OFDM_IQ_SC16 && cfg->in_scale != 0.0f) {
    if (!(std::isfinite(cfg->in_scale) && cfg->in_scale > 0.0f)) FAIL(h, OFDM_E_INVAL, "psd in_scale must be finite and positive (0: 2^-15)");
    scale = cfg->in_scale;
  }
  if (!taps_finite(cfg->taps, cfg->nfft)) FAIL(h, OFDM_E_INVAL, "psd taps must be finite");
  bool any = false;
  for (uint32_t k = 0; k < cfg->nfft; k++) any = any || cfg->taps[k] != 0.0f;
  if (!any) FAIL(h, OFDM_E_INVAL, "psd taps must not all be zero");
  RCCHK(stage_disarm(h, d));
  const int F = (int)cfg->nfft;
  d.F = F;
  d.S = (int)cfg->hop;
  d.in_fmt = (int)cfg->in_format;
  d.in_scale = scale;
  // forward twiddles as the sensor builds them (engine_sense.inc): the same table, the same bits
  std::vector<c32> tw(F);
  for (int k = 0; k < F; k++) {
    double a = -2.0 * M_PI * (double)k / (double)F;
    tw[k] = c32{(float)cos(a), (float)sin(a)};
  }
  HIPCHK(h, d.d_w.ensure(sizeof(float) * (size_t)F));
  HIPCHK(h, d.d_tw.ensure(sizeof(c32) * (size_t)F));
  HIPCHK(h, d.d_sum.ensure(sizeof(double) * (size_t)F));
  HIPCHK(h, d.d_peak.ensure(sizeof(float) * (size_t)F));
  HIPCHK(h, hipMemcpyAsync(d.d_w.p, cfg->taps, sizeof(float) * (size_t)F, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(d.d_tw.p, tw.data(), sizeof(c32) * (size_t)F, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));  // (tw is this function's)
  RCCHK(psd_zero_totals(h, d));
  return stage_arm(h, d, F - 1);
}

extern "C" int ofdm_psd_reset(ofdm_handle* h) {
  if (!h) return OFDM_E_INVAL;
  PsdState& d = h->psd;
  if (!d.on) FAIL(h, OFDM_E_INVAL, "ofdm_psd_reset without ofdm_set_psd");
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  RCCHK(psd_zero_totals(h, d));
  return stage_reset(h, d, 0);
}

extern "C" int ofdm_psd_last_ms(const ofdm_handle* h, double* ms) {
  if (!h) return OFDM_E_INVAL;
  return stage_last_ms(h->psd, ms);
}

extern "C" int ofdm_psd_count(ofdm_handle* h, uint64_t nin, uint64_t* nrows) {
  if (!h) return OFDM_E_INVAL;
  PsdState& d = h->psd;
  if (!nrows) FAIL(h, OFDM_E_INVAL, "null argument");
  if (!d.on) FAIL(h, OFDM_E_INVAL, "ofdm_psd_count without ofdm_set_psd");
  PsdPlan pl;
  const bool ok = psd_plan(d.next, nin, (uint32_t)d.F, (uint32_t)d.S, &pl);
  *nrows = pl.nseg;
  if (!ok) FAIL(h, OFDM_E_INVAL, "ofdm_psd_count: call too long (split it)");
  return OFDM_OK;
}

extern "C" int ofdm_psd_read(ofdm_handle* h, double* sum, float* peak, uint64_t* nseg) {
  if (!h) return OFDM_E_INVAL;
  PsdState& d = h->psd;
  if (!d.on) FAIL(h, OFDM_E_INVAL, "ofdm_psd_read without ofdm_set_psd");
  if ((uintptr_t)sum & 7u) FAIL(h, OFDM_E_INVAL, "float64 buffers must be 8-byte aligned");
  if ((uintptr_t)peak & 3u) FAIL(h, OFDM_E_INVAL, "float32 buffers must be 4-byte aligned");
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  const hipMemcpyKind kind = h->dev_ptrs ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  if (sum) HIPCHK(h, hipMemcpyAsync(sum, d.d_sum.p, sizeof(double) * (size_t)d.F, kind, h->stream));
  if (peak) HIPCHK(h, hipMemcpyAsync(peak, d.d_peak.p, sizeof(float) * (size_t)d.F, kind, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (nseg) *nseg = d.nseg;
  return OFDM_OK;
}

/* the next nin samples of the stream; the rows of the segments they complete, where asked for */
extern "C" int ofdm_psd(ofdm_handle* h, const void* iq_in, uint64_t nin, float* rows, uint64_t rows_cap, uint64_t* nrows) {
  if (!h) return OFDM_E_INVAL;
  PsdState& d = h->psd;
  if (!nrows) FAIL(h, OFDM_E_INVAL, "null argument");
  if (!d.on) FAIL(h, OFDM_E_INVAL, "ofdm_psd without ofdm_set_psd");
  const bool s16 = d.in_fmt == OFDM_IQ_SC16;
  const size_t ss = s16 ? sizeof(sc16) : sizeof(c32);
  if (nin && !iq_in) FAIL(h, OFDM_E_INVAL, "null iq_in");
  if (s16 && ((uintptr_t)iq_in & 3u)) FAIL(h, OFDM_E_INVAL, "ofdm_sc16 buffers must be 4-byte aligned");
  if (!s16 && ((uintptr_t)iq_in & 7u)) FAIL(h, OFDM_E_INVAL, "float32 IQ buffers must be 8-byte aligned");
  if ((uintptr_t)rows & 3u) FAIL(h, OFDM_E_INVAL, "float32 buffers must be 4-byte aligned");
  const uint64_t F = (uint64_t)d.F;
  PsdPlan pl;
  const bool fits = psd_plan(d.next, nin, (uint32_t)d.F, (uint32_t)d.S, &pl);
  *nrows = pl.nseg;
  if (!fits) FAIL(h, OFDM_E_INVAL, "ofdm_psd: call too long (split it)");
  if (rows && pl.nseg > rows_cap) FAIL(h, OFDM_E_CAPACITY, "rows too small (the call's segments)");
  if (rows && pl.nseg) {
    // a workgroup stores rows while others still read the input
    const uintptr_t i0 = (uintptr_t)iq_in, i1 = i0 + nin * ss, o0 = (uintptr_t)rows, o1 = o0 + pl.nseg * F * sizeof(float);
    if (i0 < o1 && o0 < i1) FAIL(h, OFDM_E_INVAL, "ofdm_psd: rows overlaps iq_in");
  }
  d.timed = false;
  if (nin == 0) return OFDM_OK;
  RCCHK(stage_enter(h));

  const void* d_in = iq_in;
  float* d_rows = rows;
  if (!h->dev_ptrs) {
    RCCHK(stage_upload(h, d.d_in, iq_in, nin * ss));
    d_in = d.d_in.p;
    if (rows && pl.nseg) {
      HIPCHK(h, d.d_out.ensure(pl.nseg * F * sizeof(float)));
      d_rows = d.d_out.as<float>();
    }
  }
  const bool timing = h->prof.on && pl.nseg > 0;
  if (pl.nseg) {
    HIPCHK(h, d.d_psum.ensure(sizeof(double) * F * pl.grid));
    HIPCHK(h, d.d_ppeak.ensure(sizeof(float) * F * pl.grid));
    PsdParams p;
    memset(&p, 0, sizeof(p));
    p.x = d_in;
    p.hist = d.d_hist[d.cur].as<c32>();
    p.win = d.d_w.as<float>();
    p.tw = d.d_tw.as<c32>();
    p.rows = d_rows;
    p.part_sum = d.d_psum.as<double>();
    p.part_peak = d.d_ppeak.as<float>();
    p.nseg = pl.nseg;
    p.first = pl.first;
    p.hop = (uint32_t)d.S;
    p.per = pl.per;
    p.xscale = d.in_scale;
    RCCHK(stage_time_begin(h, d, timing));
    switch (d.F) {
      case 64: psd_launch_n<64>(p, pl.grid, s16, h->stream); break;
      case 128: psd_launch_n<128>(p, pl.grid, s16, h->stream); break;
      case 256: psd_launch_n<256>(p, pl.grid, s16, h->stream); break;
      case 512: psd_launch_n<512>(p, pl.grid, s16, h->stream); break;
      case 1024: psd_launch_n<1024>(p, pl.grid, s16, h->stream); break;
      case 2048: psd_launch_n<2048>(p, pl.grid, s16, h->stream); break;
      default: psd_launch_n<4096>(p, pl.grid, s16, h->stream); break;
    }
    hipLaunchKernelGGL(k_psd_reduce, dim3((unsigned)((F + 255) / 256)), dim3(256), 0, h->stream, p.part_sum, p.part_peak, pl.grid,
                       (uint32_t)F, d.d_sum.as<double>(), d.d_peak.as<float>());
    RCCHK(stage_time_end(h, d, timing));
  }
  if (s16) RCCHK(stage_roll_history(h, d, static_cast<const sc16*>(d_in), nin, d.in_scale));
  else RCCHK(stage_roll_history(h, d, static_cast<const c32*>(d_in), nin, 0.f));
  if (!h->dev_ptrs && rows && pl.nseg)
    HIPCHK(h, hipMemcpyAsync(rows, d_rows, pl.nseg * F * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  RCCHK(stage_finish(h, d, nin, timing));
  d.nseg += pl.nseg;
  return OFDM_OK;
}
