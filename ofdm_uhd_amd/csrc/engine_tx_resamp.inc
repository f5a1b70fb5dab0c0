// engine_tx_resamp.inc -- host side of the rational-rate transmit stage (tx_resamp.h): configuration, index limits,
// launches.  Included by engine.hip after engine_stage.inc (the stream skeleton it shares with the other stages).

constexpr uint64_t TX_RESAMP_MAX_INDEX = 1ull << 56;  // largest input index: i L and n M stay inside 64-bit integers

/* blks2.rational_resampler_ccf(interpolation, decimation, taps) in front of the radio's set_center_freq */
extern "C" int ofdm_set_tx_resamp(ofdm_handle* h, const ofdm_tx_resamp_cfg* cfg) {
  if (!h) return OFDM_E_INVAL;
  TxResampState& d = h->tx_resamp;
  if (!cfg) return stage_off(d);
  if (cfg->struct_size != sizeof(ofdm_tx_resamp_cfg)) FAIL(h, OFDM_E_INVAL, "ofdm_tx_resamp_cfg.struct_size does not match this library");
  if (cfg->interpolation < 1 || cfg->interpolation > TX_RESAMP_MAX_RATIO) FAIL(h, OFDM_E_INVAL, "transmit resampler interpolation must be in [1, 64]");
  if (cfg->decimation < 1 || cfg->decimation > TX_RESAMP_MAX_RATIO) FAIL(h, OFDM_E_INVAL, "transmit resampler decimation must be in [1, 64]");
  if (cfg->ntaps < 1 || cfg->ntaps > OFDM_TX_RESAMP_MAX_TAPS) FAIL(h, OFDM_E_INVAL, "transmit resampler ntaps must be in [1, 1024]");
  float scale;
  RCCHK(stage_out_scale(h, "transmit resampler", cfg->out_format, cfg->out_scale, &scale));
  RCCHK(stage_check_center_freqs(h, "transmit resampler", &cfg->center_freq, 1, "output sample"));
  if (!taps_finite(cfg->taps, cfg->ntaps)) FAIL(h, OFDM_E_INVAL, "transmit resampler taps must be finite");
  RCCHK(stage_disarm(h, d));
  d.L = (int)cfg->interpolation;
  d.M = (int)cfg->decimation;
  d.ntaps = (int)cfg->ntaps;
  d.out_fmt = (int)cfg->out_format;
  d.out_scale = scale;
  d.D = ddc_turns(cfg->center_freq);
  HIPCHK(h, upload(d.d_taps, cfg->taps, (size_t)d.ntaps));
  return stage_arm(h, d, (d.ntaps - 1) / d.L);
}

extern "C" int ofdm_tx_resamp_reset(ofdm_handle* h, uint64_t first_input_index) {
  if (!h) return OFDM_E_INVAL;
  if (!h->tx_resamp.on) FAIL(h, OFDM_E_INVAL, "ofdm_tx_resamp_reset without ofdm_set_tx_resamp");
  if (first_input_index > TX_RESAMP_MAX_INDEX) FAIL(h, OFDM_E_INVAL, "ofdm_tx_resamp_reset: first_input_index must be at most 2^56");
  return stage_reset(h, h->tx_resamp, first_input_index);
}

extern "C" int ofdm_tx_resamp_count(const ofdm_handle* h, uint64_t nin, uint64_t* nout) {
  if (!h || !nout) return OFDM_E_INVAL;
  const TxResampState& d = h->tx_resamp;
  if (!d.on) return OFDM_E_INVAL;
  if (nin > TX_RESAMP_MAX_INDEX || d.next + nin > TX_RESAMP_MAX_INDEX) return OFDM_E_INVAL;
  *nout = first_output(d.next + nin, (uint64_t)d.L, (uint64_t)d.M) - first_output(d.next, (uint64_t)d.L, (uint64_t)d.M);
  return OFDM_OK;
}

extern "C" int ofdm_tx_resamp_last_ms(const ofdm_handle* h, double* ms) {
  if (!h) return OFDM_E_INVAL;
  return stage_last_ms(h->tx_resamp, ms);
}

/* the next nin narrowband samples in, the wideband samples at L / M times their rate that they complete out (optionally
 * added onto a band that is there) */
extern "C" int ofdm_tx_resamp(ofdm_handle* h, const ofdm_c32* iq_in, uint64_t nin, const ofdm_c32* add, void* iq_out, uint64_t out_cap,
                              uint64_t* nout) {
  if (!h) return OFDM_E_INVAL;
  TxResampState& d = h->tx_resamp;
  if (!nout) FAIL(h, OFDM_E_INVAL, "null argument");
  if (!d.on) FAIL(h, OFDM_E_INVAL, "ofdm_tx_resamp without ofdm_set_tx_resamp");
  const bool s16 = d.out_fmt == OFDM_IQ_SC16;
  RCCHK(stage_check_tx_bufs(h, s16, iq_in, nin, add, iq_out));
  const uint64_t L = (uint64_t)d.L, M = (uint64_t)d.M, a = d.next;
  if (nin > TX_RESAMP_MAX_INDEX || a + nin > TX_RESAMP_MAX_INDEX) FAIL(h, OFDM_E_INVAL, "ofdm_tx_resamp: the stream's input index would pass 2^56");
  const uint64_t n0 = first_output(a, L, M), no = first_output(a + nin, L, M) - n0;
  *nout = no;
  if (no > out_cap) FAIL(h, OFDM_E_CAPACITY, "iq_out too small (see ofdm_tx_resamp_count)");
  if (no && !iq_out) FAIL(h, OFDM_E_INVAL, "null iq_out");
  d.timed = false;
  if (nin == 0) return OFDM_OK;
  const TxResampGeom g = tx_resamp_geom(d.L, d.M);
  const uint64_t TJ = (uint64_t)g.TJ(), J0 = n0 / L;
  const uint64_t grid = no ? ((n0 + no + L - 1) / L - J0 + TJ - 1) / TJ : 0;
  RCCHK(stage_check_grid(h, "ofdm_tx_resamp", grid));
  RCCHK(stage_enter(h));

  const size_t oss = s16 ? sizeof(sc16) : sizeof(c32);
  const c32* d_in = reinterpret_cast<const c32*>(iq_in);
  const c32* d_add = reinterpret_cast<const c32*>(add);
  void* d_out = iq_out;
  RCCHK(stage_tx_rows_in(h, d, iq_in, 0, 1, nin, &d_in, nullptr));
  if (no) RCCHK(stage_tx_out(h, d, add, no, oss, &d_add, &d_out));
  const bool timing = h->prof.on && no > 0;
  if (no) {
    TxResampParams p;
    memset(&p, 0, sizeof(p));
    p.x = d_in;
    p.hist = d.d_hist[d.cur].as<c32>();
    p.taps = d.d_taps.as<float>();
    p.add = d_add;
    p.out = d_out;
    p.nin = nin;
    p.a = a;
    p.n0 = n0;
    p.nout = no;
    p.J0 = J0;
    p.D = d.D;
    p.magicM = (1ull << 32) / M + 1;
    p.magicL = (1ull << 32) / L + 1;
    p.L = d.L;
    p.M = d.M;
    p.ntaps = d.ntaps;
    p.Q = d.hist;
    p.QM = resamp_hist_periods(p.Q, d.M);
    p.W = resamp_pitch(g.TJ(), p.QM);
    p.TP = g.TJ() | 1;
    p.KC = g.kc;
    p.scale = d.out_scale;
    const size_t lds = tx_resamp_lds_bytes(d.L, d.M, d.ntaps);
    RCCHK(stage_time_begin(h, d, timing));
    RCCHK(stage_tx_variant(s16, add != nullptr, [&](auto o, auto a) {
      return stage_launch(h, &k_tx_resamp<decltype(o), decltype(a)::value>, (unsigned)grid, TX_RESAMP_THREADS, lds, p);
    }));
    RCCHK(stage_time_end(h, d, timing));
  }
  RCCHK(stage_roll_history(h, d, d_in, nin, 0.f));
  if (no) RCCHK(stage_tx_readback(h, iq_out, d_out, no, oss));
  return stage_finish(h, d, nin, timing);
}
