// engine_duc.inc -- host side of the wideband transmit stage (duc.h): configuration, stream state, launches.
// Included by engine.hip after engine_ddc.inc (ddc_turns).

constexpr uint64_t DUC_MAX_OUTPUT = 1ull << 63;  // no output index may pass it

static int duc_zero_history(ofdm_handle* h) {
  DucState& d = h->duc;
  const size_t bytes = sizeof(c32) * (size_t)std::max(d.Q, 1);
  for (int i = 0; i < 2; i++) HIPCHK(h, hipMemsetAsync(d.d_hist[i].p, 0, bytes, h->stream));
  d.cur = 0;
  return OFDM_OK;
}

/* sink.set_interp + set_center_freq (usrp_transmit_path.py:79-88, generic_usrp.set_interp) */
extern "C" int ofdm_set_duc(ofdm_handle* h, const ofdm_duc_cfg* cfg) {
  if (!h) return OFDM_E_INVAL;
  DucState& d = h->duc;
  if (!cfg) {
    d.on = false;
    d.next = 0;
    d.timed = false;
    return OFDM_OK;
  }
  if (cfg->struct_size != sizeof(ofdm_duc_cfg)) FAIL(h, OFDM_E_INVAL, "ofdm_duc_cfg.struct_size does not match this library");
  if (cfg->interpolation < 1 || cfg->interpolation > DUC_MAX_INTERP) FAIL(h, OFDM_E_INVAL, "DUC interpolation must be in [1, 64]");
  if (cfg->ntaps < 1 || cfg->ntaps > OFDM_DUC_MAX_TAPS) FAIL(h, OFDM_E_INVAL, "DUC ntaps must be in [1, 1024]");
  if (cfg->out_format != OFDM_IQ_FC32 && cfg->out_format != OFDM_IQ_SC16) FAIL(h, OFDM_E_INVAL, "unknown DUC out_format");
  float scale = 32768.0f;
  if (cfg->out_format == OFDM_IQ_SC16 && cfg->out_scale != 0.0f) {
    if (!(std::isfinite(cfg->out_scale) && cfg->out_scale > 0.0f)) FAIL(h, OFDM_E_INVAL, "DUC out_scale must be finite and positive (0: 2^15)");
    scale = cfg->out_scale;
  }
  if (!(fabs(cfg->center_freq) <= 0.5)) FAIL(h, OFDM_E_INVAL, "DUC center_freq must be in [-0.5, 0.5] cycles per output sample");
  for (uint32_t k = 0; k < cfg->ntaps; k++)
    if (!std::isfinite(cfg->taps[k])) FAIL(h, OFDM_E_INVAL, "DUC taps must be finite");
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  HIPCHK(h, hipStreamSynchronize(h->stream));  // a call in flight may still read the old taps
  d.on = false;
  d.L = (int)cfg->interpolation;
  d.ntaps = (int)cfg->ntaps;
  d.Q = (d.ntaps - 1) / d.L;
  d.out_fmt = (int)cfg->out_format;
  d.out_scale = scale;
  d.D = ddc_turns(cfg->center_freq);
  HIPCHK(h, upload(d.d_taps, cfg->taps, (size_t)d.ntaps));
  for (int i = 0; i < 2; i++) HIPCHK(h, d.d_hist[i].ensure(sizeof(c32) * (size_t)std::max(d.Q, 1)));
  int rc = duc_zero_history(h);
  if (rc) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  d.next = 0;
  d.timed = false;
  d.on = true;
  return OFDM_OK;
}

extern "C" int ofdm_duc_reset(ofdm_handle* h, uint64_t first_input_index) {
  if (!h) return OFDM_E_INVAL;
  DucState& d = h->duc;
  if (!d.on) FAIL(h, OFDM_E_INVAL, "ofdm_duc_reset without ofdm_set_duc");
  if (first_input_index > DUC_MAX_OUTPUT / (uint64_t)d.L) FAIL(h, OFDM_E_INVAL, "ofdm_duc_reset: the first output index would pass 2^63");
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  int rc = duc_zero_history(h);
  if (rc) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  d.next = first_input_index;
  return OFDM_OK;
}

extern "C" int ofdm_duc_last_ms(const ofdm_handle* h, double* ms) {
  if (!h || !ms) return OFDM_E_INVAL;
  if (!h->duc.timed) return OFDM_E_INVAL;
  *ms = h->duc.last_ms;
  return OFDM_OK;
}

template <typename OUT, bool ADD>
static void launch_duc(ofdm_handle* h, const DucParams& p, const DucGeom& g, unsigned grid, size_t lds) {
  if (g.opt == 8) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_duc<OUT, ADD, 8>), dim3(grid), dim3(DUC_THREADS), lds, h->stream, p);
  else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_duc<OUT, ADD, 4>), dim3(grid), dim3(DUC_THREADS), lds, h->stream, p);
}

/* the next nin narrowband samples in, their nin L wideband samples out (optionally added onto a band that is there) */
extern "C" int ofdm_duc(ofdm_handle* h, const ofdm_c32* iq_in, uint64_t nin, const ofdm_c32* add, void* iq_out, uint64_t out_cap,
                        uint64_t* nout) {
  if (!h) return OFDM_E_INVAL;
  DucState& d = h->duc;
  if (!nout) FAIL(h, OFDM_E_INVAL, "null argument");
  if (!d.on) FAIL(h, OFDM_E_INVAL, "ofdm_duc without ofdm_set_duc");
  const bool s16 = d.out_fmt == OFDM_IQ_SC16;
  if (nin && !iq_in) FAIL(h, OFDM_E_INVAL, "null iq_in");
  if (((uintptr_t)iq_in & 7u) || ((uintptr_t)add & 7u)) FAIL(h, OFDM_E_INVAL, "float32 IQ buffers must be 8-byte aligned");
  if (s16 && ((uintptr_t)iq_out & 3u)) FAIL(h, OFDM_E_INVAL, "ofdm_sc16 buffers must be 4-byte aligned");
  if (!s16 && ((uintptr_t)iq_out & 7u)) FAIL(h, OFDM_E_INVAL, "float32 IQ buffers must be 8-byte aligned");
  const uint64_t L = (uint64_t)d.L, a = d.next, lim = DUC_MAX_OUTPUT / L;
  // (a L + nin L stays at or below 2^63: neither the output index nor the signed sample offsets in the kernel wrap)
  if (nin > lim || a > lim - nin) FAIL(h, OFDM_E_INVAL, "ofdm_duc: the stream's output index would pass 2^63");
  const uint64_t no = nin * L;
  *nout = no;
  if (no > out_cap) FAIL(h, OFDM_E_CAPACITY, "iq_out too small (nin * interpolation samples)");
  if (no && !iq_out) FAIL(h, OFDM_E_INVAL, "null iq_out");
  d.timed = false;
  if (nin == 0) return OFDM_OK;
  const DucGeom g = duc_geom(d.L);
  const uint64_t grid = (no + (uint64_t)g.T() - 1) / (uint64_t)g.T();
  if (grid > 0x7FFFFFFFull) FAIL(h, OFDM_E_INVAL, "ofdm_duc: call too long (split it)");
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  // a transmit batch still in flight (ofdm_tx_async) may be writing the caller's input
  if (h->tx_pending && h->txs != h->stream) HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_tx_done, 0));

  const size_t oss = s16 ? sizeof(sc16) : sizeof(c32);
  const c32* d_in = reinterpret_cast<const c32*>(iq_in);
  const c32* d_add = reinterpret_cast<const c32*>(add);
  void* d_out = iq_out;
  if (!h->dev_ptrs) {
    HIPCHK(h, d.d_in.ensure(nin * sizeof(c32)));
    HIPCHK(h, hipMemcpyAsync(d.d_in.p, iq_in, nin * sizeof(c32), hipMemcpyHostToDevice, h->stream));
    d_in = d.d_in.as<c32>();
    if (add) {
      HIPCHK(h, d.d_add.ensure(no * sizeof(c32)));
      HIPCHK(h, hipMemcpyAsync(d.d_add.p, add, no * sizeof(c32), hipMemcpyHostToDevice, h->stream));
      d_add = d.d_add.as<c32>();
    }
    HIPCHK(h, d.d_out.ensure(no * oss));
    d_out = d.d_out.p;
  }
  const bool timing = h->prof.on;
  if (timing && !d.ev_a) {
    HIPCHK(h, hipEventCreate(&d.ev_a));
    HIPCHK(h, hipEventCreate(&d.ev_b));
  }
  DucParams p;
  memset(&p, 0, sizeof(p));
  p.x = d_in;
  p.hist = d.d_hist[d.cur].as<c32>();
  p.taps = d.d_taps.as<float>();
  p.add = d_add;
  p.out = d_out;
  p.nin = nin;
  p.a = a;
  p.nout = no;
  p.D = d.D;
  p.magic = (1ull << 32) / L + 1;
  p.L = d.L;
  p.ntaps = d.ntaps;
  p.Q = d.Q;
  p.scale = d.out_scale;
  const size_t lds = duc_lds_bytes(d.L, d.ntaps);
  if (timing) HIPCHK(h, hipEventRecord(d.ev_a, h->stream));
  if (s16) {
    if (add) launch_duc<sc16, true>(h, p, g, (unsigned)grid, lds);
    else launch_duc<sc16, false>(h, p, g, (unsigned)grid, lds);
  } else {
    if (add) launch_duc<c32, true>(h, p, g, (unsigned)grid, lds);
    else launch_duc<c32, false>(h, p, g, (unsigned)grid, lds);
  }
  if (timing) HIPCHK(h, hipEventRecord(d.ev_b, h->stream));
  HIPCHK(h, hipGetLastError());
  if (d.Q > 0) {
    hipLaunchKernelGGL(k_duc_hist, dim3((unsigned)((d.Q + 255) / 256)), dim3(256), 0, h->stream, d_in, nin, d.d_hist[d.cur].as<c32>(),
                       d.d_hist[d.cur ^ 1].as<c32>(), d.Q);
    HIPCHK(h, hipGetLastError());
  }
  if (!h->dev_ptrs) HIPCHK(h, hipMemcpyAsync(iq_out, d_out, no * oss, hipMemcpyDeviceToHost, h->stream));
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
