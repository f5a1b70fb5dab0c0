// engine_resamp.inc -- host side of the rational-rate front end (resamp.h): configuration, stream state, launches.
// Included by engine.hip after engine_ddc.inc (ddc_turns).

constexpr uint64_t RESAMP_MAX_INDEX = 1ull << 56;  // largest input index: i L and n M stay inside 64-bit integers

static int resamp_zero_history(ofdm_handle* h) {
  ResampState& d = h->resamp;
  const size_t bytes = sizeof(c32) * (size_t)std::max(d.Q, 1);
  for (int i = 0; i < 2; i++) HIPCHK(h, hipMemsetAsync(d.d_hist[i].p, 0, bytes, h->stream));
  d.cur = 0;
  return OFDM_OK;
}

/* blks2.rational_resampler_ccf(interpolation, decimation, taps) behind a tuner (gr.freq_xlating_fir_filter_ccf) */
extern "C" int ofdm_set_resamp(ofdm_handle* h, const ofdm_resamp_cfg* cfg) {
  if (!h) return OFDM_E_INVAL;
  ResampState& d = h->resamp;
  if (!cfg) {
    d.on = false;
    d.next = 0;
    d.timed = false;
    return OFDM_OK;
  }
  if (cfg->struct_size != sizeof(ofdm_resamp_cfg)) FAIL(h, OFDM_E_INVAL, "ofdm_resamp_cfg.struct_size does not match this library");
  if (cfg->interpolation < 1 || cfg->interpolation > RESAMP_MAX_RATIO) FAIL(h, OFDM_E_INVAL, "resampler interpolation must be in [1, 64]");
  if (cfg->decimation < 1 || cfg->decimation > RESAMP_MAX_RATIO) FAIL(h, OFDM_E_INVAL, "resampler decimation must be in [1, 64]");
  if (cfg->ntaps < 1 || cfg->ntaps > OFDM_RESAMP_MAX_TAPS) FAIL(h, OFDM_E_INVAL, "resampler ntaps must be in [1, 1024]");
  if (!(fabs(cfg->center_freq) <= 0.5)) FAIL(h, OFDM_E_INVAL, "resampler center_freq must be in [-0.5, 0.5] cycles per sample");
  for (uint32_t k = 0; k < cfg->ntaps; k++)
    if (!std::isfinite(cfg->taps[k])) FAIL(h, OFDM_E_INVAL, "resampler taps must be finite");
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  HIPCHK(h, hipStreamSynchronize(h->stream));  // a call in flight may still read the old table
  d.on = false;
  d.L = (int)cfg->interpolation;
  d.M = (int)cfg->decimation;
  d.ntaps = (int)cfg->ntaps;
  d.Q = (d.ntaps - 1) / d.L;
  d.fc = cfg->center_freq;
  d.D = ddc_turns(d.fc * (double)d.M / (double)d.L);
  // the band-pass table at L times the input rate: float64, rounded once
  d.tab.resize(d.ntaps);
  for (int k = 0; k < d.ntaps; k++) {
    const double a = 2.0 * M_PI * d.fc * (double)k / (double)d.L;
    d.tab[k] = c32{(float)((double)cfg->taps[k] * cos(a)), (float)((double)cfg->taps[k] * sin(a))};
  }
  HIPCHK(h, upload(d.d_tab, d.tab.data(), d.tab.size()));
  for (int i = 0; i < 2; i++) HIPCHK(h, d.d_hist[i].ensure(sizeof(c32) * (size_t)std::max(d.Q, 1)));
  int rc = resamp_zero_history(h);
  if (rc) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  d.next = 0;
  d.timed = false;
  d.on = true;
  return OFDM_OK;
}

extern "C" int ofdm_resamp_reset(ofdm_handle* h, uint64_t first_sample_index) {
  if (!h) return OFDM_E_INVAL;
  ResampState& d = h->resamp;
  if (!d.on) FAIL(h, OFDM_E_INVAL, "ofdm_resamp_reset without ofdm_set_resamp");
  if (first_sample_index > RESAMP_MAX_INDEX) FAIL(h, OFDM_E_INVAL, "ofdm_resamp_reset: first_sample_index must be at most 2^56");
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  int rc = resamp_zero_history(h);
  if (rc) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  d.next = first_sample_index;
  return OFDM_OK;
}

// the first output n with i_n = floor(n M / L) >= a: ceil(a L / M)   (a <= 2^56, L <= 64: no overflow)
static uint64_t resamp_first_output(uint64_t a, uint64_t L, uint64_t M) { return (a * L + M - 1) / M; }

extern "C" int ofdm_resamp_count(const ofdm_handle* h, uint64_t nin, uint64_t* nout) {
  if (!h || !nout) return OFDM_E_INVAL;
  const ResampState& d = h->resamp;
  if (!d.on) return OFDM_E_INVAL;
  if (nin > RESAMP_MAX_INDEX) return OFDM_E_INVAL;  // (the sum below stays inside 64 bits)
  *nout = resamp_first_output(d.next + nin, (uint64_t)d.L, (uint64_t)d.M) - resamp_first_output(d.next, (uint64_t)d.L, (uint64_t)d.M);
  return OFDM_OK;
}

extern "C" int ofdm_resamp_taps(const ofdm_handle* h, ofdm_c32* out, int cap, int* n) {
  if (!h || !n) return OFDM_E_INVAL;
  const ResampState& d = h->resamp;
  if (!d.on) return OFDM_E_INVAL;
  *n = d.ntaps;
  if (!out) return OFDM_OK;
  if (cap < d.ntaps) return OFDM_E_CAPACITY;
  memcpy(out, d.tab.data(), sizeof(c32) * (size_t)d.ntaps);
  return OFDM_OK;
}

extern "C" int ofdm_resamp_last_ms(const ofdm_handle* h, double* ms) {
  if (!h || !ms) return OFDM_E_INVAL;
  if (!h->resamp.timed) return OFDM_E_INVAL;
  *ms = h->resamp.last_ms;
  return OFDM_OK;
}

template <typename XT, int NG>
static hipError_t launch_resamp_g(ofdm_handle* h, const ResampParams& p, unsigned grid, size_t lds) {
  if (lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_resamp<XT, NG>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_resamp<XT, NG>), dim3(grid), dim3(RESAMP_THREADS), lds, h->stream, p);
  return hipSuccess;
}
template <typename XT>
static hipError_t launch_resamp(ofdm_handle* h, const ResampParams& p, const ResampGeom& g, unsigned grid, size_t lds) {
  return g.ng == 1 ? launch_resamp_g<XT, 1>(h, p, grid, lds) : launch_resamp_g<XT, 4>(h, p, grid, lds);
}

/* rational_resampler_ccf::work behind the tuner: the next nin wideband samples in, the samples at L / M times their
 * rate that they complete out */
extern "C" int ofdm_resamp(ofdm_handle* h, const void* iq_in, uint64_t nin, ofdm_c32* iq_out, uint64_t out_cap, uint64_t* nout) {
  if (!h) return OFDM_E_INVAL;
  ResampState& d = h->resamp;
  if (!nout) FAIL(h, OFDM_E_INVAL, "null argument");
  if (!d.on) FAIL(h, OFDM_E_INVAL, "ofdm_resamp without ofdm_set_resamp");
  const bool s16 = h->rx_fmt == OFDM_IQ_SC16;
  if (nin && !iq_in) FAIL(h, OFDM_E_INVAL, "null iq_in");
  if (s16 && ((uintptr_t)iq_in & 3u)) FAIL(h, OFDM_E_INVAL, "ofdm_sc16 buffers must be 4-byte aligned");
  if (!s16 && ((uintptr_t)iq_in & 7u)) FAIL(h, OFDM_E_INVAL, "float32 IQ buffers must be 8-byte aligned");
  const uint64_t L = (uint64_t)d.L, M = (uint64_t)d.M, a = d.next;
  if (nin > RESAMP_MAX_INDEX || a + nin > RESAMP_MAX_INDEX) FAIL(h, OFDM_E_INVAL, "ofdm_resamp: the stream's sample index would pass 2^56");
  const uint64_t n0 = resamp_first_output(a, L, M), no = resamp_first_output(a + nin, L, M) - n0;
  *nout = no;
  if (no > out_cap) FAIL(h, OFDM_E_CAPACITY, "iq_out too small (see ofdm_resamp_count)");
  if (no && !iq_out) FAIL(h, OFDM_E_INVAL, "null iq_out");
  d.timed = false;
  if (nin == 0) return OFDM_OK;
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  // a transmit batch still in flight (ofdm_tx_async) may be writing the caller's input
  if (h->tx_pending && h->txs != h->stream) HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_tx_done, 0));

  const void* d_in = iq_in;
  c32* d_out = reinterpret_cast<c32*>(iq_out);
  if (!h->dev_ptrs) {
    HIPCHK(h, d.d_in.ensure(nin * rx_ss(h)));
    HIPCHK(h, hipMemcpyAsync(d.d_in.p, iq_in, nin * rx_ss(h), hipMemcpyHostToDevice, h->stream));
    d_in = d.d_in.p;
    if (no) {
      HIPCHK(h, d.d_out.ensure(no * sizeof(c32)));
      d_out = d.d_out.as<c32>();
    }
  }
  const bool timing = h->prof.on && no > 0;
  if (timing && !d.ev_a) {
    HIPCHK(h, hipEventCreate(&d.ev_a));
    HIPCHK(h, hipEventCreate(&d.ev_b));
  }
  if (no) {
    const ResampGeom g = resamp_geom(d.L, d.M);
    const uint64_t TJ = (uint64_t)g.TJ();
    ResampParams p;
    memset(&p, 0, sizeof(p));
    p.x = d_in;
    p.hist = d.d_hist[d.cur].as<c32>();
    p.tab = d.d_tab.as<c32>();
    p.out = d_out;
    p.nin = nin;
    p.a = a;
    p.n0 = n0;
    p.nout = no;
    p.J0 = n0 / L;
    p.D = d.D;
    p.magicM = (1ull << 32) / M + 1;
    p.magicL = (1ull << 32) / L + 1;
    p.L = d.L;
    p.M = d.M;
    p.ntaps = d.ntaps;
    p.Q = d.Q;
    p.QM = resamp_hist_periods(d.Q, d.M);
    p.W = resamp_pitch(g.TJ(), p.QM);
    p.TP = g.TJ() | 1;
    p.KC = g.kc;
    p.scale = h->rx_scale;
    const uint64_t periods = (n0 + no + L - 1) / L - p.J0;
    const uint64_t grid = (periods + TJ - 1) / TJ;
    if (grid > 0x7FFFFFFFull) FAIL(h, OFDM_E_INVAL, "ofdm_resamp: call too long (split it)");
    const size_t lds = resamp_lds_bytes(d.L, d.M, d.ntaps);
    if (timing) HIPCHK(h, hipEventRecord(d.ev_a, h->stream));
    if (s16) HIPCHK(h, launch_resamp<sc16>(h, p, g, (unsigned)grid, lds));
    else HIPCHK(h, launch_resamp<c32>(h, p, g, (unsigned)grid, lds));
    if (timing) HIPCHK(h, hipEventRecord(d.ev_b, h->stream));
    HIPCHK(h, hipGetLastError());
  }
  if (d.Q > 0) {
    const unsigned grid = (unsigned)((d.Q + 255) / 256);
    c32* nw = d.d_hist[d.cur ^ 1].as<c32>();
    if (s16)
      hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ddc_hist<sc16>), dim3(grid), dim3(256), 0, h->stream, static_cast<const sc16*>(d_in), nin,
                         d.d_hist[d.cur].as<c32>(), nw, d.Q, h->rx_scale);
    else
      hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ddc_hist<c32>), dim3(grid), dim3(256), 0, h->stream, static_cast<const c32*>(d_in), nin,
                         d.d_hist[d.cur].as<c32>(), nw, d.Q, h->rx_scale);
    HIPCHK(h, hipGetLastError());
  }
  if (!h->dev_ptrs && no) HIPCHK(h, hipMemcpyAsync(iq_out, d_out, no * sizeof(c32), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (d.Q > 0) d.cur ^= 1;
  d.next = a + nin;
  if (timing) {
    float ms = 0.f;
    HIPCHK(h, hipEventElapsedTime(&ms, d.ev_a, d.ev_b));
    d.last_ms = (double)ms;
    d.timed = true;
  }
  return OFDM_OK;
}
