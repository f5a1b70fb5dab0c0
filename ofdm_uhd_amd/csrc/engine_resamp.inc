// engine_resamp.inc -- host side of the rational-rate front end (resamp.h): configuration, index limits, launches.
// Included by engine.hip after engine_stage.inc (the stream skeleton it shares with the other wideband stages).

constexpr uint64_t RESAMP_MAX_INDEX = 1ull << 56;  // largest input index: i L and n M stay inside 64-bit integers

/* blks2.rational_resampler_ccf(interpolation, decimation, taps) behind a tuner (gr.freq_xlating_fir_filter_ccf) */
extern "C" int ofdm_set_resamp(ofdm_handle* h, const ofdm_resamp_cfg* cfg) {
  if (!h) return OFDM_E_INVAL;
  ResampState& d = h->resamp;
  if (!cfg) return stage_off(d);
  if (cfg->struct_size != sizeof(ofdm_resamp_cfg)) FAIL(h, OFDM_E_INVAL, "ofdm_resamp_cfg.struct_size does not match this library");
  if (cfg->interpolation < 1 || cfg->interpolation > RESAMP_MAX_RATIO) FAIL(h, OFDM_E_INVAL, "resampler interpolation must be in [1, 64]");
  if (cfg->decimation < 1 || cfg->decimation > RESAMP_MAX_RATIO) FAIL(h, OFDM_E_INVAL, "resampler decimation must be in [1, 64]");
  if (cfg->ntaps < 1 || cfg->ntaps > OFDM_RESAMP_MAX_TAPS) FAIL(h, OFDM_E_INVAL, "resampler ntaps must be in [1, 1024]");
  RCCHK(stage_check_center_freqs(h, "resampler", &cfg->center_freq, 1, "sample"));
  if (!taps_finite(cfg->taps, cfg->ntaps)) FAIL(h, OFDM_E_INVAL, "resampler taps must be finite");
  RCCHK(stage_disarm(h, d));
  d.L = (int)cfg->interpolation;
  d.M = (int)cfg->decimation;
  d.ntaps = (int)cfg->ntaps;
  d.fc = cfg->center_freq;
  d.D = ddc_turns(d.fc * (double)d.M / (double)d.L);
  d.tab = bandpass_table(cfg->taps, d.ntaps, d.fc, d.L);  // at L times the input rate
  HIPCHK(h, upload(d.d_tab, d.tab.data(), d.tab.size()));
  return stage_arm(h, d, (d.ntaps - 1) / d.L);
}

extern "C" int ofdm_resamp_reset(ofdm_handle* h, uint64_t first_sample_index) {
  if (!h) return OFDM_E_INVAL;
  if (!h->resamp.on) FAIL(h, OFDM_E_INVAL, "ofdm_resamp_reset without ofdm_set_resamp");
  if (first_sample_index > RESAMP_MAX_INDEX) FAIL(h, OFDM_E_INVAL, "ofdm_resamp_reset: first_sample_index must be at most 2^56");
  return stage_reset(h, h->resamp, first_sample_index);
}

extern "C" int ofdm_resamp_count(const ofdm_handle* h, uint64_t nin, uint64_t* nout) {
  if (!h || !nout) return OFDM_E_INVAL;
  const ResampState& d = h->resamp;
  if (!d.on) return OFDM_E_INVAL;
  if (nin > RESAMP_MAX_INDEX) return OFDM_E_INVAL;  // (the sum below stays inside 64 bits; next + nin is not bounded here)
  *nout = first_output(d.next + nin, (uint64_t)d.L, (uint64_t)d.M) - first_output(d.next, (uint64_t)d.L, (uint64_t)d.M);
  return OFDM_OK;
}

extern "C" int ofdm_resamp_taps(const ofdm_handle* h, ofdm_c32* out, int cap, int* n) {
  if (!h || !n || !h->resamp.on) return OFDM_E_INVAL;
  return stage_taps_out(h->resamp.tab.data(), h->resamp.ntaps, out, cap, n);
}

extern "C" int ofdm_resamp_last_ms(const ofdm_handle* h, double* ms) {
  if (!h) return OFDM_E_INVAL;
  return stage_last_ms(h->resamp, ms);
}

template <typename XT>
static int launch_resamp(ofdm_handle* h, const ResampParams& p, const ResampGeom& g, unsigned grid, size_t lds) {
  return stage_launch(h, g.ng == 1 ? &k_resamp<XT, 1> : &k_resamp<XT, 4>, grid, RESAMP_THREADS, lds, p);
}

/* rational_resampler_ccf::work behind the tuner: the next nin wideband samples in, the samples at L / M times their
 * rate that they complete out */
extern "C" int ofdm_resamp(ofdm_handle* h, const void* iq_in, uint64_t nin, ofdm_c32* iq_out, uint64_t out_cap, uint64_t* nout) {
  if (!h) return OFDM_E_INVAL;
  ResampState& d = h->resamp;
  if (!nout) FAIL(h, OFDM_E_INVAL, "null argument");
  if (!d.on) FAIL(h, OFDM_E_INVAL, "ofdm_resamp without ofdm_set_resamp");
  RCCHK(stage_check_rx_in(h, iq_in, nin));
  const uint64_t L = (uint64_t)d.L, M = (uint64_t)d.M, a = d.next;
  if (nin > RESAMP_MAX_INDEX || a + nin > RESAMP_MAX_INDEX) FAIL(h, OFDM_E_INVAL, "ofdm_resamp: the stream's sample index would pass 2^56");
  const uint64_t n0 = first_output(a, L, M), no = first_output(a + nin, L, M) - n0;
  *nout = no;
  if (no > out_cap) FAIL(h, OFDM_E_CAPACITY, "iq_out too small (see ofdm_resamp_count)");
  if (no && !iq_out) FAIL(h, OFDM_E_INVAL, "null iq_out");
  d.timed = false;
  if (nin == 0) return OFDM_OK;
  RCCHK(stage_enter(h));

  const void* d_in = iq_in;
  c32* d_out = reinterpret_cast<c32*>(iq_out);
  RCCHK(stage_rx_in(h, d, iq_in, nin, &d_in));
  RCCHK(stage_rx_out(h, d, 1, no, &d_out, nullptr));
  const bool timing = h->prof.on && no > 0;
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
    p.Q = d.hist;
    p.QM = resamp_hist_periods(p.Q, d.M);
    p.W = resamp_pitch(g.TJ(), p.QM);
    p.TP = g.TJ() | 1;
    p.KC = g.kc;
    p.scale = h->rx_scale;
    const uint64_t periods = (n0 + no + L - 1) / L - p.J0;
    const uint64_t grid = (periods + TJ - 1) / TJ;
    RCCHK(stage_check_grid(h, "ofdm_resamp", grid));
    const size_t lds = resamp_lds_bytes(d.L, d.M, d.ntaps);
    RCCHK(stage_time_begin(h, d, timing));
    RCCHK(h->rx_fmt == OFDM_IQ_SC16 ? launch_resamp<sc16>(h, p, g, (unsigned)grid, lds) : launch_resamp<c32>(h, p, g, (unsigned)grid, lds));
    RCCHK(stage_time_end(h, d, timing));
  }
  RCCHK(stage_roll_rx_history(h, d, d_in, nin));
  RCCHK(stage_rx_readback(h, iq_out, 0, 1, no, d_out));
  return stage_finish(h, d, nin, timing);
}
