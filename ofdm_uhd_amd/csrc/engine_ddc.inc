// engine_ddc.inc -- host side of the wideband front end (ddc.h): configuration, stream state, launches.
// Included by engine.hip after the handle is defined.

constexpr uint64_t DDC_MAX_INDEX = 1ull << 62;  // largest first_sample_index; a stream may run on to 2^63

// frac(fc R) in units of 2^-64 turn: the integer-turn convention of nco_turns (rx_demod.h), from cycles
static uint64_t ddc_turns(double cycles) {
  double t = cycles - floor(cycles);
  if (!(t < 1.0)) t = 0.0;  // a tiny negative product rounds up to a whole turn: phase 0
  return (uint64_t)(t * 18446744073709551616.0);  // t < 1: exact scaling, no overflow
}

static int ddc_zero_history(ofdm_handle* h) {
  DdcState& d = h->ddc;
  const size_t bytes = sizeof(c32) * (size_t)std::max(d.ntaps - 1, 1);
  for (int i = 0; i < 2; i++) HIPCHK(h, hipMemsetAsync(d.d_hist[i].p, 0, bytes, h->stream));
  d.cur = 0;
  return OFDM_OK;
}

/* usrp2.source_32fc.set_decim + set_center_freq (usrp_receive_path.py) = gr.freq_xlating_fir_filter_ccf's ctor */
extern "C" int ofdm_set_ddc(ofdm_handle* h, const ofdm_ddc_cfg* cfg) {
  if (!h) return OFDM_E_INVAL;
  DdcState& d = h->ddc;
  if (!cfg) {
    d.on = false;
    d.next = 0;
    d.timed = false;
    return OFDM_OK;
  }
  if (cfg->struct_size != sizeof(ofdm_ddc_cfg)) FAIL(h, OFDM_E_INVAL, "ofdm_ddc_cfg.struct_size does not match this library");
  if (cfg->decimation < 1 || cfg->decimation > DDC_MAX_DECIM) FAIL(h, OFDM_E_INVAL, "DDC decimation must be in [1, 64]");
  if (cfg->ntaps < 1 || cfg->ntaps > OFDM_DDC_MAX_TAPS) FAIL(h, OFDM_E_INVAL, "DDC ntaps must be in [1, 1024]");
  if (!(fabs(cfg->center_freq) <= 0.5)) FAIL(h, OFDM_E_INVAL, "DDC center_freq must be in [-0.5, 0.5] cycles per sample");
  for (uint32_t k = 0; k < cfg->ntaps; k++)
    if (!std::isfinite(cfg->taps[k])) FAIL(h, OFDM_E_INVAL, "DDC taps must be finite");
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  HIPCHK(h, hipStreamSynchronize(h->stream));  // a call in flight may still read the old table
  d.on = false;
  d.R = (int)cfg->decimation;
  d.ntaps = (int)cfg->ntaps;
  d.fc = cfg->center_freq;
  d.D = ddc_turns(d.fc * (double)d.R);
  // the band-pass table: float64, rounded once
  d.tab.resize(d.ntaps);
  for (int k = 0; k < d.ntaps; k++) {
    const double a = 2.0 * M_PI * d.fc * (double)k;
    d.tab[k] = c32{(float)((double)cfg->taps[k] * cos(a)), (float)((double)cfg->taps[k] * sin(a))};
  }
  HIPCHK(h, upload(d.d_tab, d.tab.data(), d.tab.size()));
  for (int i = 0; i < 2; i++) HIPCHK(h, d.d_hist[i].ensure(sizeof(c32) * (size_t)std::max(d.ntaps - 1, 1)));
  int rc = ddc_zero_history(h);
  if (rc) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  d.next = 0;
  d.timed = false;
  d.on = true;
  return OFDM_OK;
}

extern "C" int ofdm_ddc_reset(ofdm_handle* h, uint64_t first_sample_index) {
  if (!h) return OFDM_E_INVAL;
  DdcState& d = h->ddc;
  if (!d.on) FAIL(h, OFDM_E_INVAL, "ofdm_ddc_reset without ofdm_set_ddc");
  if (first_sample_index > DDC_MAX_INDEX) FAIL(h, OFDM_E_INVAL, "ofdm_ddc_reset: first_sample_index must be at most 2^62");
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  int rc = ddc_zero_history(h);
  if (rc) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  d.next = first_sample_index;
  return OFDM_OK;
}

// outputs m with a <= m R < a + n
static uint64_t ddc_first_output(uint64_t a, uint64_t R) { return a / R + (a % R ? 1 : 0); }

extern "C" int ofdm_ddc_count(const ofdm_handle* h, uint64_t nin, uint64_t* nout) {
  if (!h || !nout) return OFDM_E_INVAL;
  const DdcState& d = h->ddc;
  if (!d.on) return OFDM_E_INVAL;
  *nout = ddc_first_output(d.next + nin, (uint64_t)d.R) - ddc_first_output(d.next, (uint64_t)d.R);
  return OFDM_OK;
}

extern "C" int ofdm_ddc_taps(const ofdm_handle* h, ofdm_c32* out, int cap, int* n) {
  if (!h || !n) return OFDM_E_INVAL;
  const DdcState& d = h->ddc;
  if (!d.on) return OFDM_E_INVAL;
  *n = d.ntaps;
  if (!out) return OFDM_OK;
  if (cap < d.ntaps) return OFDM_E_CAPACITY;
  memcpy(out, d.tab.data(), sizeof(c32) * (size_t)d.ntaps);
  return OFDM_OK;
}

extern "C" int ofdm_ddc_last_ms(const ofdm_handle* h, double* ms) {
  if (!h || !ms) return OFDM_E_INVAL;
  if (!h->ddc.timed) return OFDM_E_INVAL;
  *ms = h->ddc.last_ms;
  return OFDM_OK;
}

template <typename XT, int OPT, int TJ>
static void launch_ddc_g(ofdm_handle* h, const DdcParams& p, unsigned grid, size_t lds) {
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ddc<XT, OPT, TJ>), dim3(grid), dim3(DDC_THREADS), lds, h->stream, p);
}
template <typename XT>
static void launch_ddc(ofdm_handle* h, const DdcParams& p, const DdcGeom& g, unsigned grid, size_t lds) {
  if (g.opt == 4 && g.tj == 256) launch_ddc_g<XT, 4, 256>(h, p, grid, lds);
  else if (g.opt == 4) launch_ddc_g<XT, 4, 64>(h, p, grid, lds);
  else launch_ddc_g<XT, 1, 64>(h, p, grid, lds);
}

/* gr.freq_xlating_fir_filter_ccf::work: the next nin wideband samples in, the narrowband samples they complete out */
extern "C" int ofdm_ddc(ofdm_handle* h, const void* iq_in, uint64_t nin, ofdm_c32* iq_out, uint64_t out_cap, uint64_t* nout) {
  if (!h) return OFDM_E_INVAL;
  DdcState& d = h->ddc;
  if (!nout) FAIL(h, OFDM_E_INVAL, "null argument");
  if (!d.on) FAIL(h, OFDM_E_INVAL, "ofdm_ddc without ofdm_set_ddc");
  const bool s16 = h->rx_fmt == OFDM_IQ_SC16;
  if (nin && !iq_in) FAIL(h, OFDM_E_INVAL, "null iq_in");
  if (s16 && ((uintptr_t)iq_in & 3u)) FAIL(h, OFDM_E_INVAL, "ofdm_sc16 buffers must be 4-byte aligned");
  if (!s16 && ((uintptr_t)iq_in & 7u)) FAIL(h, OFDM_E_INVAL, "float32 IQ buffers must be 8-byte aligned");
  const uint64_t R = (uint64_t)d.R, a = d.next;
  // (indices stay below 2^63: a + nin, the tile's M0 R and the signed sample offsets in the kernel cannot wrap)
  if (nin > DDC_MAX_INDEX || a + nin > 2 * DDC_MAX_INDEX) FAIL(h, OFDM_E_INVAL, "ofdm_ddc: the stream's sample index would pass 2^63");
  const uint64_t m0 = ddc_first_output(a, R), no = ddc_first_output(a + nin, R) - m0;
  *nout = no;
  if (no > out_cap) FAIL(h, OFDM_E_CAPACITY, "iq_out too small (see ofdm_ddc_count)");
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
  const int H = d.ntaps - 1;
  const bool timing = h->prof.on && no > 0;
  if (timing && !d.ev_a) {
    HIPCHK(h, hipEventCreate(&d.ev_a));
    HIPCHK(h, hipEventCreate(&d.ev_b));
  }
  if (no) {
    const DdcGeom g = ddc_geom(d.R);
    DdcParams p;
    memset(&p, 0, sizeof(p));
    p.x = d_in;
    p.hist = d.d_hist[d.cur].as<c32>();
    p.tab = d.d_tab.as<c32>();
    p.out = d_out;
    p.nin = nin;
    p.a = a;
    p.m0 = m0;
    p.nout = no;
    p.D = d.D;
    p.magic = (1ull << 32) / R + 1;
    p.R = d.R;
    p.ntaps = d.ntaps;
    p.Q = H / d.R;
    p.W = ddc_pitch(g.T(), p.Q);
    p.scale = h->rx_scale;
    const uint64_t grid = (no + (uint64_t)g.T() - 1) / (uint64_t)g.T();
    if (grid > 0x7FFFFFFFull) FAIL(h, OFDM_E_INVAL, "ofdm_ddc: call too long (split it)");
    const size_t lds = ddc_lds_bytes(d.R, d.ntaps);
    if (timing) HIPCHK(h, hipEventRecord(d.ev_a, h->stream));
    if (s16) launch_ddc<sc16>(h, p, g, (unsigned)grid, lds);
    else launch_ddc<c32>(h, p, g, (unsigned)grid, lds);
    if (timing) HIPCHK(h, hipEventRecord(d.ev_b, h->stream));
    HIPCHK(h, hipGetLastError());
  }
  if (H > 0) {
    const unsigned grid = (unsigned)((H + 255) / 256);
    c32* nw = d.d_hist[d.cur ^ 1].as<c32>();
    if (s16)
      hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ddc_hist<sc16>), dim3(grid), dim3(256), 0, h->stream, static_cast<const sc16*>(d_in), nin,
                         d.d_hist[d.cur].as<c32>(), nw, H, h->rx_scale);
    else
      hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ddc_hist<c32>), dim3(grid), dim3(256), 0, h->stream, static_cast<const c32*>(d_in), nin,
                         d.d_hist[d.cur].as<c32>(), nw, H, h->rx_scale);
    HIPCHK(h, hipGetLastError());
  }
  if (!h->dev_ptrs && no) HIPCHK(h, hipMemcpyAsync(iq_out, d_out, no * sizeof(c32), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (H > 0) d.cur ^= 1;
  d.next = a + nin;
  if (timing) {
    float ms = 0.f;
    HIPCHK(h, hipEventElapsedTime(&ms, d.ev_a, d.ev_b));
    d.last_ms = (double)ms;
    d.timed = true;
  }
  return OFDM_OK;
}
