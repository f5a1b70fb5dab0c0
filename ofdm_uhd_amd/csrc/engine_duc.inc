// engine_duc.inc -- host side of the wideband transmit stage (duc.h): configuration, index limits, launches.
// Included by engine.hip after engine_stage.inc (the stream skeleton it shares with the other wideband stages).

constexpr uint64_t DUC_MAX_OUTPUT = 1ull << 63;  // no output index may pass it

/* sink.set_interp + set_center_freq (usrp_transmit_path.py:79-88, generic_usrp.set_interp) */
extern "C" int ofdm_set_duc(ofdm_handle* h, const ofdm_duc_cfg* cfg) {
  if (!h) return OFDM_E_INVAL;
  DucState& d = h->duc;
  if (!cfg) return stage_off(d);
  if (cfg->struct_size != sizeof(ofdm_duc_cfg)) FAIL(h, OFDM_E_INVAL, "ofdm_duc_cfg.struct_size does not match this library");
  if (cfg->interpolation < 1 || cfg->interpolation > DUC_MAX_INTERP) FAIL(h, OFDM_E_INVAL, "DUC interpolation must be in [1, 64]");
  if (cfg->ntaps < 1 || cfg->ntaps > OFDM_DUC_MAX_TAPS) FAIL(h, OFDM_E_INVAL, "DUC ntaps must be in [1, 1024]");
  float scale;
  RCCHK(stage_out_scale(h, "DUC", cfg->out_format, cfg->out_scale, &scale));
  RCCHK(stage_check_center_freqs(h, "DUC", &cfg->center_freq, 1, "output sample"));
  if (!taps_finite(cfg->taps, cfg->ntaps)) FAIL(h, OFDM_E_INVAL, "DUC taps must be finite");
  RCCHK(stage_disarm(h, d));
  d.L = (int)cfg->interpolation;
  d.ntaps = (int)cfg->ntaps;
  d.out_fmt = (int)cfg->out_format;
  d.out_scale = scale;
  d.D = ddc_turns(cfg->center_freq);
  HIPCHK(h, upload(d.d_taps, cfg->taps, (size_t)d.ntaps));
  return stage_arm(h, d, (d.ntaps - 1) / d.L);
}

extern "C" int ofdm_duc_reset(ofdm_handle* h, uint64_t first_input_index) {
  if (!h) return OFDM_E_INVAL;
  DucState& d = h->duc;
  if (!d.on) FAIL(h, OFDM_E_INVAL, "ofdm_duc_reset without ofdm_set_duc");
  if (first_input_index > DUC_MAX_OUTPUT / (uint64_t)d.L) FAIL(h, OFDM_E_INVAL, "ofdm_duc_reset: the first output index would pass 2^63");
  return stage_reset(h, d, first_input_index);
}

extern "C" int ofdm_duc_last_ms(const ofdm_handle* h, double* ms) {
  if (!h) return OFDM_E_INVAL;
  return stage_last_ms(h->duc, ms);
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
  RCCHK(stage_check_tx_bufs(h, s16, iq_in, nin, add, iq_out));
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
  RCCHK(stage_check_grid(h, "ofdm_duc", grid));
  RCCHK(stage_enter(h));

  const size_t oss = s16 ? sizeof(sc16) : sizeof(c32);
  const c32* d_in = reinterpret_cast<const c32*>(iq_in);
  const c32* d_add = reinterpret_cast<const c32*>(add);
  void* d_out = iq_out;
  RCCHK(stage_tx_rows_in(h, d, iq_in, 0, 1, nin, &d_in, nullptr));
  RCCHK(stage_tx_out(h, d, add, no, oss, &d_add, &d_out));  // (nin > 0: the call has outputs)
  const bool timing = h->prof.on;  // (nin > 0: the call has outputs)
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
  p.Q = d.hist;
  p.scale = d.out_scale;
  const size_t lds = duc_lds_bytes(d.L, d.ntaps);  // (never more than 64 KB: no hipFuncSetAttribute)
  RCCHK(stage_time_begin(h, d, timing));
  stage_tx_variant(s16, add != nullptr, [&](auto o, auto a) { launch_duc<decltype(o), decltype(a)::value>(h, p, g, (unsigned)grid, lds); });
  RCCHK(stage_time_end(h, d, timing));
  RCCHK(stage_roll_history(h, d, d_in, nin, 0.f));
  RCCHK(stage_tx_readback(h, iq_out, d_out, no, oss));
  return stage_finish(h, d, nin, timing);
}
