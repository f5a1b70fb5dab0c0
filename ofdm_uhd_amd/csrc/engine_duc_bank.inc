// engine_duc_bank.inc -- host side of the DUC bank (duc_bank.h): configuration, index limits, launch (the per-link
// upload: stage_tx_rows_in).  Included by engine.hip after engine_stage.inc and engine_duc.inc (DUC_MAX_OUTPUT).

/* one sink.set_interp + set_center_freq per link (usrp_transmit_path.py:79-88; the two-channel transmitter of
 * dual_channel/dual_channel.py), for K links that share interpolation and prototype */
extern "C" int ofdm_set_duc_bank(ofdm_handle* h, const ofdm_duc_bank_cfg* cfg) {
  if (!h) return OFDM_E_INVAL;
  DucBankState& d = h->duc_bank;
  if (!cfg) return stage_off(d);
  if (cfg->struct_size != sizeof(ofdm_duc_bank_cfg)) FAIL(h, OFDM_E_INVAL, "ofdm_duc_bank_cfg.struct_size does not match this library");
  if (cfg->interpolation < 1 || cfg->interpolation > DUC_MAX_INTERP) FAIL(h, OFDM_E_INVAL, "DUC bank interpolation must be in [1, 64]");
  if (cfg->ntaps < 1 || cfg->ntaps > OFDM_DUC_MAX_TAPS) FAIL(h, OFDM_E_INVAL, "DUC bank ntaps must be in [1, 1024]");
  RCCHK(stage_check_nlinks(h, "DUC bank", cfg->nlinks));
  float scale;
  RCCHK(stage_out_scale(h, "DUC bank", cfg->out_format, cfg->out_scale, &scale));
  RCCHK(stage_check_center_freqs(h, "DUC bank", cfg->center_freq, cfg->nlinks, "output sample"));
  if (!taps_finite(cfg->taps, cfg->ntaps)) FAIL(h, OFDM_E_INVAL, "DUC bank taps must be finite");
  RCCHK(stage_disarm(h, d));
  d.L = (int)cfg->interpolation;
  d.ntaps = (int)cfg->ntaps;
  d.K = (int)cfg->nlinks;
  d.Q = (d.ntaps - 1) / d.L;
  d.out_fmt = (int)cfg->out_format;
  d.out_scale = scale;
  // every link's table is the DDC bank's; its phase step per INPUT is L times the DUC's per output, modulo a turn
  d.tab = bank_tables(cfg->taps, d.ntaps, cfg->center_freq, d.K, 1);
  for (int i = 0; i < d.K; i++) d.E[i] = ddc_turns(cfg->center_freq[i]) * (uint64_t)d.L;
  HIPCHK(h, upload(d.d_tab, d.tab.data(), d.tab.size()));
  return stage_arm(h, d, d.K * d.Q);  // the last Q raw inputs of every link
}

extern "C" int ofdm_duc_bank_reset(ofdm_handle* h, uint64_t first_input_index) {
  if (!h) return OFDM_E_INVAL;
  DucBankState& d = h->duc_bank;
  if (!d.on) FAIL(h, OFDM_E_INVAL, "ofdm_duc_bank_reset without ofdm_set_duc_bank");
  if (first_input_index > DUC_MAX_OUTPUT / (uint64_t)d.L) FAIL(h, OFDM_E_INVAL, "ofdm_duc_bank_reset: the first output index would pass 2^63");
  return stage_reset(h, d, first_input_index);
}

extern "C" int ofdm_duc_bank_taps(const ofdm_handle* h, int link, ofdm_c32* out, int cap, int* n) {
  if (!h || !n) return OFDM_E_INVAL;
  const DucBankState& d = h->duc_bank;
  return stage_bank_taps(d.on, d.tab, d.ntaps, d.K, link, out, cap, n);
}

extern "C" int ofdm_duc_bank_last_ms(const ofdm_handle* h, double* ms) {
  if (!h) return OFDM_E_INVAL;
  return stage_last_ms(h->duc_bank, ms);
}

template <typename OUT, bool ADD>
static void launch_duc_bank(ofdm_handle* h, const DucBankParams& p, const DucGeom& g, unsigned grid, size_t lds) {
  // (never more than 64 KB of LDS, whatever K: no hipFuncSetAttribute)
  if (g.opt == 8) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_duc_bank<OUT, ADD, 8>), dim3(grid), dim3(DUC_THREADS), lds, h->stream, p);
  else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_duc_bank<OUT, ADD, 4>), dim3(grid), dim3(DUC_THREADS), lds, h->stream, p);
}

/* the next nin samples of every link in (link i's run begins at iq_in + i * link_stride), the nin L samples of the
 * band out (optionally added onto a band that is there) */
extern "C" int ofdm_duc_bank(ofdm_handle* h, const ofdm_c32* iq_in, uint64_t link_stride, uint64_t nin, const ofdm_c32* add, void* iq_out,
                             uint64_t out_cap, uint64_t* nout) {
  if (!h) return OFDM_E_INVAL;
  DucBankState& d = h->duc_bank;
  if (!nout) FAIL(h, OFDM_E_INVAL, "null argument");
  if (!d.on) FAIL(h, OFDM_E_INVAL, "ofdm_duc_bank without ofdm_set_duc_bank");
  const bool s16 = d.out_fmt == OFDM_IQ_SC16;
  RCCHK(stage_check_tx_bufs(h, s16, iq_in, nin, add, iq_out));
  const uint64_t L = (uint64_t)d.L, K = (uint64_t)d.K, a = d.next, lim = DUC_MAX_OUTPUT / L;
  // (a L + nin L stays at or below 2^63: neither the output index nor the signed sample offsets in the kernel wrap)
  if (nin > lim || a > lim - nin) FAIL(h, OFDM_E_INVAL, "ofdm_duc_bank: the stream's output index would pass 2^63");
  const uint64_t no = nin * L;
  *nout = no;
  if (no > out_cap) FAIL(h, OFDM_E_CAPACITY, "iq_out too small (nin * interpolation samples)");
  if (K > 1 && link_stride < nin) FAIL(h, OFDM_E_INVAL, "ofdm_duc_bank: link_stride is smaller than the inputs of one link");
  if (no && !iq_out) FAIL(h, OFDM_E_INVAL, "null iq_out");
  d.timed = false;
  if (nin == 0) return OFDM_OK;
  const DucGeom g = duc_geom(d.L);
  const uint64_t grid = (no + (uint64_t)g.T() - 1) / (uint64_t)g.T();
  RCCHK(stage_check_grid(h, "ofdm_duc_bank", grid));
  RCCHK(stage_enter(h));

  const size_t oss = s16 ? sizeof(sc16) : sizeof(c32);
  const c32* d_in = reinterpret_cast<const c32*>(iq_in);
  const c32* d_add = reinterpret_cast<const c32*>(add);
  void* d_out = iq_out;
  uint64_t stride = link_stride;
  RCCHK(stage_tx_rows_in(h, d, iq_in, link_stride, K, nin, &d_in, &stride));
  RCCHK(stage_tx_out(h, d, add, no, oss, &d_add, &d_out));  // (nin > 0: the call has outputs)
  const bool timing = h->prof.on;  // (nin > 0: the call has outputs)
  DucBankParams p;
  memset(&p, 0, sizeof(p));
  p.x = d_in;
  p.hist = d.d_hist[d.cur].as<c32>();
  p.tab = d.d_tab.as<c32>();
  p.add = d_add;
  p.out = d_out;
  p.nin = nin;
  p.stride = stride;
  p.a = a;
  p.nout = no;
  memcpy(p.E, d.E, sizeof(p.E));
  p.magic = (1ull << 32) / L + 1;
  p.L = d.L;
  p.ntaps = d.ntaps;
  p.Q = d.Q;
  p.K = d.K;
  p.scale = d.out_scale;
  const size_t lds = duc_bank_lds_bytes(d.L, d.ntaps);
  RCCHK(stage_time_begin(h, d, timing));
  stage_tx_variant(s16, add != nullptr, [&](auto o, auto a) { launch_duc_bank<decltype(o), decltype(a)::value>(h, p, g, (unsigned)grid, lds); });
  RCCHK(stage_time_end(h, d, timing));
  RCCHK(stage_roll_rows_history(h, d, d_in, stride, nin, d.Q, d.K));
  RCCHK(stage_tx_readback(h, iq_out, d_out, no, oss));
  return stage_finish(h, d, nin, timing);
}
