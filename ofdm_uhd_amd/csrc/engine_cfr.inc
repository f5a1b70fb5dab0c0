// engine_cfr.inc -- host side of the crest-factor reduction stage (cfr.h): configuration, launch, statistics.
// Included by engine.hip after engine_multipath.inc; like it, the stage uses the stream skeleton of engine_stage.inc
// with the transmit single shape (no `add`).

extern "C" int ofdm_set_cfr(ofdm_handle* h, const ofdm_cfr_cfg* cfg) {
  if (!h) return OFDM_E_INVAL;
  CfrState& d = h->cfr;
  if (!cfg) return stage_off(d);
  if (cfg->struct_size != sizeof(ofdm_cfr_cfg)) FAIL(h, OFDM_E_INVAL, "ofdm_cfr_cfg.struct_size does not match this library");
  if (!(std::isfinite(cfg->threshold) && cfg->threshold > 0.0f)) FAIL(h, OFDM_E_INVAL, "cfr threshold must be finite and positive");
  if (cfg->ntaps > OFDM_CFR_MAX_TAPS || cfg->ntaps % 2 == 0) FAIL(h, OFDM_E_INVAL, "cfr ntaps must be odd and in [1, 1023]");
  float scale;
  RCCHK(stage_out_scale(h, "cfr", cfg->out_format, cfg->out_scale, &scale));
  const int H = (int)(cfg->ntaps - 1) / 2;
  for (uint32_t k = 0; k < cfg->ntaps; k++)
    if (!(cfg->taps[k] >= 0.0f && cfg->taps[k] <= 1.0f)) FAIL(h, OFDM_E_INVAL, "cfr taps must be in [0, 1]");
  if (cfg->taps[H] != 1.0f) FAIL(h, OFDM_E_INVAL, "cfr taps[H] must be 1");
  RCCHK(stage_disarm(h, d));
  d.H = H;
  d.A = cfg->threshold;
  d.out_fmt = (int)cfg->out_format;
  d.out_scale = scale;
  HIPCHK(h, d.d_w.ensure(sizeof(float) * cfg->ntaps));
  HIPCHK(h, hipMemcpyAsync(d.d_w.p, cfg->taps, sizeof(float) * cfg->ntaps, hipMemcpyHostToDevice, h->stream));
  RCCHK(stage_stats_zero(h, d.st));
  return stage_arm(h, d, 2 * H);
}

extern "C" int ofdm_cfr_reset(ofdm_handle* h) {
  if (!h) return OFDM_E_INVAL;
  CfrState& d = h->cfr;
  if (!d.on) FAIL(h, OFDM_E_INVAL, "ofdm_cfr_reset without ofdm_set_cfr");
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  RCCHK(stage_stats_zero(h, d.st));
  return stage_reset(h, d, 0);
}

extern "C" int ofdm_cfr_last_ms(const ofdm_handle* h, double* ms) {
  if (!h) return OFDM_E_INVAL;
  return stage_last_ms(h->cfr, ms);
}

extern "C" int ofdm_cfr_stats(ofdm_handle* h, struct ofdm_cfr_stats* out) {
  if (!h) return OFDM_E_INVAL;
  CfrState& d = h->cfr;
  if (!out) FAIL(h, OFDM_E_INVAL, "null argument");
  if (!d.on) FAIL(h, OFDM_E_INVAL, "ofdm_cfr_stats without ofdm_set_cfr");
  StatTotals t;
  RCCHK(stage_stats_read(h, d.st, &t));
  out->n = d.st.n;
  out->n_over = t.n_over;
  out->n_touched = t.n_touched;
  out->peak_in = t.peak_in;
  out->peak_out = t.peak_out;
  out->sum_in = t.sum_in;
  out->sum_out = t.sum_out;
  out->sum_err = t.sum_err;
  return OFDM_OK;
}

/* the next nin samples of the stream in, nin samples out */
extern "C" int ofdm_cfr(ofdm_handle* h, const ofdm_c32* iq_in, uint64_t nin, void* iq_out, uint64_t out_cap, uint64_t* nout) {
  if (!h) return OFDM_E_INVAL;
  CfrState& d = h->cfr;
  if (!nout) FAIL(h, OFDM_E_INVAL, "null argument");
  if (!d.on) FAIL(h, OFDM_E_INVAL, "ofdm_cfr without ofdm_set_cfr");
  const bool s16 = d.out_fmt == OFDM_IQ_SC16;
  RCCHK(stage_check_tx_bufs(h, s16, iq_in, nin, nullptr, iq_out));
  *nout = nin;
  if (nin > out_cap) FAIL(h, OFDM_E_CAPACITY, "iq_out too small (nin samples)");
  if (nin && !iq_out) FAIL(h, OFDM_E_INVAL, "null iq_out");
  const size_t oss = s16 ? sizeof(sc16) : sizeof(c32);
  {
    // a tile reads the inputs of its neighbours' outputs: the two buffers may not share a byte
    const uintptr_t i0 = (uintptr_t)iq_in, i1 = i0 + nin * sizeof(c32), o0 = (uintptr_t)iq_out, o1 = o0 + nin * oss;
    if (nin && i0 < o1 && o0 < i1) FAIL(h, OFDM_E_INVAL, "ofdm_cfr: iq_in overlaps iq_out");
  }
  d.timed = false;
  if (nin == 0) return OFDM_OK;
  const uint64_t grid = (nin + (uint64_t)CFR_TILE - 1) / (uint64_t)CFR_TILE;
  if (!stage_stats_fits(grid)) FAIL(h, OFDM_E_INVAL, "ofdm_cfr: call too long (split it)");
  RCCHK(stage_enter(h));

  const c32* d_in = reinterpret_cast<const c32*>(iq_in);
  const c32* d_add = nullptr;
  void* d_out = iq_out;
  RCCHK(stage_tx_rows_in(h, d, iq_in, 0, 1, nin, &d_in, nullptr));
  RCCHK(stage_tx_out(h, d, nullptr, nin, oss, &d_add, &d_out));
  RCCHK(stage_stats_room(h, d.st, grid));
  const bool timing = h->prof.on;
  CfrParams p;
  memset(&p, 0, sizeof(p));
  p.x = d_in;
  p.hist = d.d_hist[d.cur].as<c32>();
  p.out = d_out;
  p.part = d.st.d_part.as<StatPartial>();
  p.nin = nin;
  p.A = d.A;
  p.H = d.H;
  p.scale = d.out_scale;
  const float* w = d.d_w.as<float>();
  RCCHK(stage_time_begin(h, d, timing));
  if (s16) hipLaunchKernelGGL(k_cfr<sc16>, dim3((unsigned)grid), dim3(CFR_THREADS), 0, h->stream, p, w);
  else hipLaunchKernelGGL(k_cfr<c32>, dim3((unsigned)grid), dim3(CFR_THREADS), 0, h->stream, p, w);
  stage_stats_reduce(h, d.st, grid);
  RCCHK(stage_time_end(h, d, timing));
  RCCHK(stage_roll_history(h, d, d_in, nin, 0.f));
  RCCHK(stage_tx_readback(h, iq_out, d_out, nin, oss));
  RCCHK(stage_finish(h, d, nin, timing));
  d.st.n += nin;
  return OFDM_OK;
}
