// engine_pfb_synth.inc -- host side of the polyphase-FFT synthesis bank (pfb_synth.h): configuration, index limits,
// launch (the per-channel upload: stage_tx_rows_in).  Included by engine.hip after engine_stage.inc and engine_duc.inc (DUC_MAX_OUTPUT).

/* one set_center_freq per radio channel on a uniform grid, transmit side (the two-channel transmitter of
 * dual_channel/dual_channel.py), for every slot of the band at once */
extern "C" int ofdm_set_pfb_synth(ofdm_handle* h, const ofdm_pfb_synth_cfg* cfg) {
  if (!h) return OFDM_E_INVAL;
  PfbSynthState& d = h->pfb_synth;
  if (!cfg) return stage_off(d);
  if (cfg->struct_size != sizeof(ofdm_pfb_synth_cfg)) FAIL(h, OFDM_E_INVAL, "ofdm_pfb_synth_cfg.struct_size does not match this library");
  const uint32_t M = cfg->nchannels;
  if (M < 2 || M > OFDM_PFB_MAX_CHANNELS || (M & (M - 1))) FAIL(h, OFDM_E_INVAL, "synthesis bank nchannels must be 2, 4, 8, 16, 32 or 64");
  if (cfg->ntaps < 1 || cfg->ntaps > OFDM_PFB_MAX_TAPS) FAIL(h, OFDM_E_INVAL, "synthesis bank ntaps must be in [1, 1024]");
  if (cfg->nsel < 1 || cfg->nsel > M) FAIL(h, OFDM_E_INVAL, "synthesis bank nsel must be in [1, nchannels]");
  signed char pos[PFB_MAX_CHANNELS];
  memset(pos, -1, sizeof(pos));
  for (uint32_t i = 0; i < cfg->nsel; i++) {
    if (cfg->channel[i] >= M) FAIL(h, OFDM_E_INVAL, "synthesis bank channel must be below nchannels");
    if (pos[cfg->channel[i]] >= 0) FAIL(h, OFDM_E_INVAL, "synthesis bank channels must all be different");
    pos[cfg->channel[i]] = (signed char)i;
  }
  float scale;
  RCCHK(stage_out_scale(h, "synthesis bank", cfg->out_format, cfg->out_scale, &scale));
  if (!taps_finite(cfg->taps, cfg->ntaps)) FAIL(h, OFDM_E_INVAL, "synthesis bank taps must be finite");
  RCCHK(stage_disarm(h, d));
  d.M = (int)M;
  d.ntaps = (int)cfg->ntaps;
  d.K = (int)cfg->nsel;
  d.Q = (d.ntaps - 1) / d.M;
  d.out_fmt = (int)cfg->out_format;
  d.out_scale = scale;
  memcpy(d.pos, pos, sizeof(d.pos));
  // w[j] = complex64(exp(+2 pi i j / M)): float64, rounded once (ofdm_set_pfb's table)
  std::vector<c32> w(M);
  for (uint32_t j = 0; j < M; j++) {
    const double a = 2.0 * M_PI * (double)j / (double)M;
    w[j] = c32{(float)cos(a), (float)sin(a)};
  }
  HIPCHK(h, upload(d.d_w, w.data(), w.size()));
  HIPCHK(h, upload(d.d_taps, cfg->taps, (size_t)d.ntaps));
  return stage_arm(h, d, d.K * d.Q);  // the last Q inputs of every selected channel
}

extern "C" int ofdm_pfb_synth_reset(ofdm_handle* h, uint64_t first_input_index) {
  if (!h) return OFDM_E_INVAL;
  PfbSynthState& d = h->pfb_synth;
  if (!d.on) FAIL(h, OFDM_E_INVAL, "ofdm_pfb_synth_reset without ofdm_set_pfb_synth");
  if (first_input_index > DUC_MAX_OUTPUT / (uint64_t)d.M) FAIL(h, OFDM_E_INVAL, "ofdm_pfb_synth_reset: the first output index would pass 2^63");
  return stage_reset(h, d, first_input_index);
}

extern "C" int ofdm_pfb_synth_last_ms(const ofdm_handle* h, double* ms) {
  if (!h) return OFDM_E_INVAL;
  return stage_last_ms(h->pfb_synth, ms);
}

template <typename OUT, bool ADD>
static void launch_pfb_synth(ofdm_handle* h, const PfbSynthParams& p, int M, unsigned grid, size_t lds) {
  // (never more than 64 KB of LDS: no hipFuncSetAttribute)
  switch (M) {
    case 2: hipLaunchKernelGGL(HIP_KERNEL_NAME(k_pfb_synth<OUT, ADD, 2>), dim3(grid), dim3(PFS_THREADS), lds, h->stream, p); break;
    case 4: hipLaunchKernelGGL(HIP_KERNEL_NAME(k_pfb_synth<OUT, ADD, 4>), dim3(grid), dim3(PFS_THREADS), lds, h->stream, p); break;
    case 8: hipLaunchKernelGGL(HIP_KERNEL_NAME(k_pfb_synth<OUT, ADD, 8>), dim3(grid), dim3(PFS_THREADS), lds, h->stream, p); break;
    case 16: hipLaunchKernelGGL(HIP_KERNEL_NAME(k_pfb_synth<OUT, ADD, 16>), dim3(grid), dim3(PFS_THREADS), lds, h->stream, p); break;
    case 32: hipLaunchKernelGGL(HIP_KERNEL_NAME(k_pfb_synth<OUT, ADD, 32>), dim3(grid), dim3(PFS_THREADS), lds, h->stream, p); break;
    default: hipLaunchKernelGGL(HIP_KERNEL_NAME(k_pfb_synth<OUT, ADD, 64>), dim3(grid), dim3(PFS_THREADS), lds, h->stream, p); break;
  }
}

/* the next nin samples of every selected channel in (channel i's run begins at iq_in + i * chan_stride), the nin M
 * samples of the band out (optionally added onto a band that is there) */
extern "C" int ofdm_pfb_synth(ofdm_handle* h, const ofdm_c32* iq_in, uint64_t chan_stride, uint64_t nin, const ofdm_c32* add, void* iq_out,
                              uint64_t out_cap, uint64_t* nout) {
  if (!h) return OFDM_E_INVAL;
  PfbSynthState& d = h->pfb_synth;
  if (!nout) FAIL(h, OFDM_E_INVAL, "null argument");
  if (!d.on) FAIL(h, OFDM_E_INVAL, "ofdm_pfb_synth without ofdm_set_pfb_synth");
  const bool s16 = d.out_fmt == OFDM_IQ_SC16;
  RCCHK(stage_check_tx_bufs(h, s16, iq_in, nin, add, iq_out));
  const uint64_t M = (uint64_t)d.M, K = (uint64_t)d.K, a = d.next, lim = DUC_MAX_OUTPUT / M;
  // (a M + nin M stays at or below 2^63: neither the output index nor the signed sample offsets in the kernel wrap)
  if (nin > lim || a > lim - nin) FAIL(h, OFDM_E_INVAL, "ofdm_pfb_synth: the stream's output index would pass 2^63");
  const uint64_t no = nin * M;
  *nout = no;
  if (no > out_cap) FAIL(h, OFDM_E_CAPACITY, "iq_out too small (nin * nchannels samples)");
  if (K > 1 && chan_stride < nin) FAIL(h, OFDM_E_INVAL, "ofdm_pfb_synth: chan_stride is smaller than the inputs of one channel");
  if (no && !iq_out) FAIL(h, OFDM_E_INVAL, "null iq_out");
  d.timed = false;
  if (nin == 0) return OFDM_OK;
  const uint64_t T = (uint64_t)pfb_synth_tile_inputs(d.M), grid = (nin + T - 1) / T;
  RCCHK(stage_check_grid(h, "ofdm_pfb_synth", grid));
  RCCHK(stage_enter(h));

  const size_t oss = s16 ? sizeof(sc16) : sizeof(c32);
  const c32* d_in = reinterpret_cast<const c32*>(iq_in);
  const c32* d_add = reinterpret_cast<const c32*>(add);
  void* d_out = iq_out;
  uint64_t stride = chan_stride;
  RCCHK(stage_tx_rows_in(h, d, iq_in, chan_stride, K, nin, &d_in, &stride));
  RCCHK(stage_tx_out(h, d, add, no, oss, &d_add, &d_out));  // (nin > 0: the call has outputs)
  const bool timing = h->prof.on;  // (nin > 0: the call has outputs)
  PfbSynthParams p;
  memset(&p, 0, sizeof(p));
  p.x = d_in;
  p.hist = d.d_hist[d.cur].as<c32>();
  p.taps = d.d_taps.as<float>();
  p.w = d.d_w.as<c32>();
  p.add = d_add;
  p.out = d_out;
  p.nin = nin;
  p.stride = stride;
  p.nout = no;
  p.ntaps = d.ntaps;
  p.Q = d.Q;
  p.P = pfb_synth_pitch(d.M, d.Q);
  p.scale = d.out_scale;
  memcpy(p.pos, d.pos, sizeof(p.pos));
  const size_t lds = pfb_synth_lds_bytes(d.M, d.ntaps);
  RCCHK(stage_time_begin(h, d, timing));
  stage_tx_variant(s16, add != nullptr, [&](auto o, auto a) { launch_pfb_synth<decltype(o), decltype(a)::value>(h, p, d.M, (unsigned)grid, lds); });
  RCCHK(stage_time_end(h, d, timing));
  RCCHK(stage_roll_rows_history(h, d, d_in, stride, nin, d.Q, d.K));
  RCCHK(stage_tx_readback(h, iq_out, d_out, no, oss));
  return stage_finish(h, d, nin, timing);
}
