// engine_multipath.inc -- host side of the propagation channel stage (multipath.h): configuration, index limit, launch.
// Included by engine.hip after engine_stage.inc and the ten wideband stages (the stream skeleton it shares with them).

/* the air between usrp_transmit_path.py and usrp_receive_path.py */
extern "C" int ofdm_set_multipath(ofdm_handle* h, const ofdm_multipath_cfg* cfg) {
  if (!h) return OFDM_E_INVAL;
  MultipathState& d = h->multipath;
  if (!cfg) return stage_off(d);
  if (cfg->struct_size != sizeof(ofdm_multipath_cfg)) FAIL(h, OFDM_E_INVAL, "ofdm_multipath_cfg.struct_size does not match this library");
  if (cfg->npaths < 1 || cfg->npaths > OFDM_MULTIPATH_MAX_PATHS) FAIL(h, OFDM_E_INVAL, "multipath npaths must be in [1, 16]");
  if (cfg->ntones > OFDM_MULTIPATH_MAX_TONES) FAIL(h, OFDM_E_INVAL, "multipath ntones must be in [0, 4]");
  float scale;
  RCCHK(stage_out_scale(h, "multipath", cfg->out_format, cfg->out_scale, &scale));
  if (!(std::isfinite(cfg->sigma) && cfg->sigma >= 0.0f)) FAIL(h, OFDM_E_INVAL, "multipath sigma must be finite and not negative");
  if (!std::isfinite(cfg->cfo)) FAIL(h, OFDM_E_INVAL, "multipath cfo must be finite");
  int Dmax = 0;
  for (uint32_t p = 0; p < cfg->npaths; p++) {
    if (cfg->delay[p] > OFDM_MULTIPATH_MAX_DELAY) FAIL(h, OFDM_E_INVAL, "multipath delay must be in [0, 1023] samples");
    if (!(std::isfinite(cfg->gain[p].re) && std::isfinite(cfg->gain[p].im))) FAIL(h, OFDM_E_INVAL, "multipath gain must be finite");
    if (!(fabs(cfg->doppler[p]) <= 0.5)) FAIL(h, OFDM_E_INVAL, "multipath doppler must be in [-0.5, 0.5] cycles per sample");
    Dmax = std::max(Dmax, (int)cfg->delay[p]);
  }
  for (uint32_t j = 0; j < cfg->ntones; j++) {
    if (!(std::isfinite(cfg->tone_amp[j]) && cfg->tone_amp[j] >= 0.0f)) FAIL(h, OFDM_E_INVAL, "multipath tone_amp must be finite and not negative");
    if (!(fabs(cfg->tone_freq[j]) <= 0.5)) FAIL(h, OFDM_E_INVAL, "multipath tone_freq must be in [-0.5, 0.5] cycles per sample");
    if (!std::isfinite(cfg->tone_phase[j])) FAIL(h, OFDM_E_INVAL, "multipath tone_phase must be finite");
  }
  RCCHK(stage_disarm(h, d));
  d.P = (int)cfg->npaths;
  d.J = (int)cfg->ntones;
  d.out_fmt = (int)cfg->out_format;
  d.out_scale = scale;
  d.sigma = cfg->sigma;
  d.cfo = cfg->cfo;
  d.seed = cfg->seed;
  d.stream_id = cfg->stream_id;
  d.phasor = d.J > 0 || d.cfo != 0.0f;
  for (int p = 0; p < d.P; p++) {
    d.d[p] = (int)cfg->delay[p];
    d.g[p] = c32{cfg->gain[p].re, cfg->gain[p].im};
    d.D[p] = ddc_turns(cfg->doppler[p]);
    d.phasor = d.phasor || d.D[p] != 0;
  }
  for (int j = 0; j < d.J; j++) {
    d.amp[j] = cfg->tone_amp[j];
    d.F[j] = ddc_turns(cfg->tone_freq[j]);
    d.Psi[j] = ddc_turns(cfg->tone_phase[j]);
  }
  return stage_arm(h, d, Dmax);
}

extern "C" int ofdm_multipath_reset(ofdm_handle* h, uint64_t first_index) {
  if (!h) return OFDM_E_INVAL;
  MultipathState& d = h->multipath;
  if (!d.on) FAIL(h, OFDM_E_INVAL, "ofdm_multipath_reset without ofdm_set_multipath");
  if (first_index > MULTIPATH_MAX_INDEX) FAIL(h, OFDM_E_INVAL, "ofdm_multipath_reset: the first index would pass 2^53");
  return stage_reset(h, d, first_index);
}

extern "C" int ofdm_multipath_last_ms(const ofdm_handle* h, double* ms) {
  if (!h) return OFDM_E_INVAL;
  return stage_last_ms(h->multipath, ms);
}

template <typename OUT, bool ADD>
static void launch_multipath(ofdm_handle* h, const MultipathParams& p, bool phasor, bool noise, unsigned grid, size_t lds) {
  auto go = [&](auto ph, auto nz) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_multipath<OUT, ADD, decltype(ph)::value, decltype(nz)::value>), dim3(grid), dim3(MP_THREADS),
                       lds, h->stream, p);
  };
  if (phasor) {
    if (noise) go(std::true_type{}, std::true_type{});
    else go(std::true_type{}, std::false_type{});
  } else {
    if (noise) go(std::false_type{}, std::true_type{});
    else go(std::false_type{}, std::false_type{});
  }
}

/* the next nin samples of the stream in, nin samples out (optionally added onto a band that is there) */
extern "C" int ofdm_multipath(ofdm_handle* h, const ofdm_c32* iq_in, uint64_t nin, const ofdm_c32* add, void* iq_out, uint64_t out_cap,
                              uint64_t* nout) {
  if (!h) return OFDM_E_INVAL;
  MultipathState& d = h->multipath;
  if (!nout) FAIL(h, OFDM_E_INVAL, "null argument");
  if (!d.on) FAIL(h, OFDM_E_INVAL, "ofdm_multipath without ofdm_set_multipath");
  const bool s16 = d.out_fmt == OFDM_IQ_SC16;
  RCCHK(stage_check_tx_bufs(h, s16, iq_in, nin, add, iq_out));
  const uint64_t a = d.next;
  // (a + nin stays at or below 2^53: the rotation's float64 phase is exact, the signed sample offsets do not wrap)
  if (nin > MULTIPATH_MAX_INDEX || a > MULTIPATH_MAX_INDEX - nin) FAIL(h, OFDM_E_INVAL, "ofdm_multipath: the stream's index would pass 2^53");
  *nout = nin;
  if (nin > out_cap) FAIL(h, OFDM_E_CAPACITY, "iq_out too small (nin samples)");
  if (nin && !iq_out) FAIL(h, OFDM_E_INVAL, "null iq_out");
  const size_t oss = s16 ? sizeof(sc16) : sizeof(c32);
  {
    // a tile reads the inputs of its neighbours' outputs: the two buffers may not share a byte
    const uintptr_t i0 = (uintptr_t)iq_in, i1 = i0 + nin * sizeof(c32), o0 = (uintptr_t)iq_out, o1 = o0 + nin * oss;
    if (nin && i0 < o1 && o0 < i1) FAIL(h, OFDM_E_INVAL, "ofdm_multipath: iq_in overlaps iq_out");
  }
  d.timed = false;
  if (nin == 0) return OFDM_OK;
  const uint64_t grid = (nin + (uint64_t)MP_TILE - 1) / (uint64_t)MP_TILE;
  RCCHK(stage_check_grid(h, "ofdm_multipath", grid));
  RCCHK(stage_enter(h));

  const c32* d_in = reinterpret_cast<const c32*>(iq_in);
  const c32* d_add = reinterpret_cast<const c32*>(add);
  void* d_out = iq_out;
  RCCHK(stage_tx_rows_in(h, d, iq_in, 0, 1, nin, &d_in, nullptr));
  RCCHK(stage_tx_out(h, d, add, nin, oss, &d_add, &d_out));  // (nin > 0: the call has outputs)
  const bool timing = h->prof.on;
  MultipathParams p;
  memset(&p, 0, sizeof(p));
  p.x = d_in;
  p.hist = d.d_hist[d.cur].as<c32>();
  p.add = d_add;
  p.out = d_out;
  p.nin = nin;
  p.a = a;
  p.seed = d.seed;
  p.stream_id = d.stream_id;
  memcpy(p.D, d.D, sizeof(p.D));
  memcpy(p.F, d.F, sizeof(p.F));
  memcpy(p.Psi, d.Psi, sizeof(p.Psi));
  memcpy(p.g, d.g, sizeof(p.g));
  memcpy(p.d, d.d, sizeof(p.d));
  memcpy(p.amp, d.amp, sizeof(p.amp));
  p.P = d.P;
  p.J = d.J;
  p.Dmax = d.hist;
  p.sigma = d.sigma;
  p.cfo = d.cfo;
  p.scale = d.out_scale;
  const size_t lds = multipath_lds_bytes(d.hist);  // (16 KB at the most: no hipFuncSetAttribute)
  RCCHK(stage_time_begin(h, d, timing));
  stage_tx_variant(s16, add != nullptr, [&](auto o, auto ad) {
    launch_multipath<decltype(o), decltype(ad)::value>(h, p, d.phasor, d.sigma > 0.0f, (unsigned)grid, lds);
  });
  RCCHK(stage_time_end(h, d, timing));
  RCCHK(stage_roll_history(h, d, d_in, nin, 0.f));
  RCCHK(stage_tx_readback(h, iq_out, d_out, nin, oss));
  return stage_finish(h, d, nin, timing);
}
