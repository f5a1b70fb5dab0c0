// engine_resamp_bank.inc -- host side of the resampler bank (resamp_bank.h): configuration, launches (the per-link
// copy-back: stage_rx_readback).  Included by engine.hip after engine_stage.inc and engine_resamp.inc (RESAMP_MAX_INDEX).

/* K blks2.rational_resampler_ccf ctors behind K tuners that share ratio and prototype (a recorder's capture holding
 * several links at a rate that is no integer multiple of theirs) */
extern "C" int ofdm_set_resamp_bank(ofdm_handle* h, const ofdm_resamp_bank_cfg* cfg) {
  if (!h) return OFDM_E_INVAL;
  ResampBankState& d = h->resamp_bank;
  if (!cfg) return stage_off(d);
  if (cfg->struct_size != sizeof(ofdm_resamp_bank_cfg)) FAIL(h, OFDM_E_INVAL, "ofdm_resamp_bank_cfg.struct_size does not match this library");
  if (cfg->interpolation < 1 || cfg->interpolation > RESAMP_MAX_RATIO) FAIL(h, OFDM_E_INVAL, "resampler bank interpolation must be in [1, 64]");
  if (cfg->decimation < 1 || cfg->decimation > RESAMP_MAX_RATIO) FAIL(h, OFDM_E_INVAL, "resampler bank decimation must be in [1, 64]");
  if (cfg->ntaps < 1 || cfg->ntaps > OFDM_RESAMP_MAX_TAPS) FAIL(h, OFDM_E_INVAL, "resampler bank ntaps must be in [1, 1024]");
  RCCHK(stage_check_nlinks(h, "resampler bank", cfg->nlinks));
  RCCHK(stage_check_center_freqs(h, "resampler bank", cfg->center_freq, cfg->nlinks, "sample"));
  if (!taps_finite(cfg->taps, cfg->ntaps)) FAIL(h, OFDM_E_INVAL, "resampler bank taps must be finite");
  RCCHK(stage_disarm(h, d));
  d.L = (int)cfg->interpolation;
  d.M = (int)cfg->decimation;
  d.ntaps = (int)cfg->ntaps;
  d.K = (int)cfg->nlinks;
  const int KP = (d.K + 1) & ~1;
  // every link's table is the resampler's; the device copy is link-minor
  d.tab = bank_tables(cfg->taps, d.ntaps, cfg->center_freq, d.K, d.L);
  std::vector<c32> dev((size_t)d.ntaps * KP, c32{0.f, 0.f});
  for (int i = 0; i < d.K; i++) {
    d.fc[i] = cfg->center_freq[i];
    d.D[i] = ddc_turns(d.fc[i] * (double)d.M / (double)d.L);
    for (int k = 0; k < d.ntaps; k++) dev[(size_t)k * KP + i] = d.tab[(size_t)i * d.ntaps + k];
  }
  HIPCHK(h, upload(d.d_tab, dev.data(), dev.size()));
  return stage_arm(h, d, (d.ntaps - 1) / d.L);
}

extern "C" int ofdm_resamp_bank_reset(ofdm_handle* h, uint64_t first_sample_index) {
  if (!h) return OFDM_E_INVAL;
  if (!h->resamp_bank.on) FAIL(h, OFDM_E_INVAL, "ofdm_resamp_bank_reset without ofdm_set_resamp_bank");
  if (first_sample_index > RESAMP_MAX_INDEX) FAIL(h, OFDM_E_INVAL, "ofdm_resamp_bank_reset: first_sample_index must be at most 2^56");
  return stage_reset(h, h->resamp_bank, first_sample_index);
}

extern "C" int ofdm_resamp_bank_count(const ofdm_handle* h, uint64_t nin, uint64_t* nout) {
  if (!h || !nout) return OFDM_E_INVAL;
  const ResampBankState& d = h->resamp_bank;
  if (!d.on) return OFDM_E_INVAL;
  if (nin > RESAMP_MAX_INDEX) return OFDM_E_INVAL;  // (as in ofdm_resamp_count)
  *nout = first_output(d.next + nin, (uint64_t)d.L, (uint64_t)d.M) - first_output(d.next, (uint64_t)d.L, (uint64_t)d.M);
  return OFDM_OK;
}

extern "C" int ofdm_resamp_bank_taps(const ofdm_handle* h, int link, ofdm_c32* out, int cap, int* n) {
  if (!h || !n) return OFDM_E_INVAL;
  const ResampBankState& d = h->resamp_bank;
  return stage_bank_taps(d.on, d.tab, d.ntaps, d.K, link, out, cap, n);
}

extern "C" int ofdm_resamp_bank_last_ms(const ofdm_handle* h, double* ms) {
  if (!h) return OFDM_E_INVAL;
  return stage_last_ms(h->resamp_bank, ms);
}

template <typename XT>
static int launch_resamp_bank(ofdm_handle* h, const ResampBankParams& p, const ResampGeom& g, unsigned grid, size_t lds) {
  return stage_launch(h, g.ng == 1 ? &k_resamp_bank<XT, 1> : &k_resamp_bank<XT, 4>, grid, RESAMP_THREADS, lds, p);
}

/* the next nin wideband samples in, the samples at L / M times their rate that they complete out, for every link:
 * link i's run begins at iq_out + i * link_stride */
extern "C" int ofdm_resamp_bank(ofdm_handle* h, const void* iq_in, uint64_t nin, ofdm_c32* iq_out, uint64_t link_stride, uint64_t out_cap,
                                uint64_t* nout) {
  if (!h) return OFDM_E_INVAL;
  ResampBankState& d = h->resamp_bank;
  if (!nout) FAIL(h, OFDM_E_INVAL, "null argument");
  if (!d.on) FAIL(h, OFDM_E_INVAL, "ofdm_resamp_bank without ofdm_set_resamp_bank");
  RCCHK(stage_check_rx_in(h, iq_in, nin));
  const uint64_t L = (uint64_t)d.L, M = (uint64_t)d.M, a = d.next, K = (uint64_t)d.K;
  if (nin > RESAMP_MAX_INDEX || a + nin > RESAMP_MAX_INDEX) FAIL(h, OFDM_E_INVAL, "ofdm_resamp_bank: the stream's sample index would pass 2^56");
  const uint64_t n0 = first_output(a, L, M), no = first_output(a + nin, L, M) - n0;
  *nout = no;
  if (no > out_cap) FAIL(h, OFDM_E_CAPACITY, "iq_out too small per link (see ofdm_resamp_bank_count)");
  if (K > 1 && link_stride < no) FAIL(h, OFDM_E_INVAL, "ofdm_resamp_bank: link_stride is smaller than the outputs of one link");
  if (no && !iq_out) FAIL(h, OFDM_E_INVAL, "null iq_out");
  d.timed = false;
  if (nin == 0) return OFDM_OK;
  RCCHK(stage_enter(h));

  const void* d_in = iq_in;
  c32* d_out = reinterpret_cast<c32*>(iq_out);
  uint64_t stride = link_stride;
  RCCHK(stage_rx_in(h, d, iq_in, nin, &d_in));
  RCCHK(stage_rx_out(h, d, K, no, &d_out, &stride));
  const bool timing = h->prof.on && no > 0;
  if (no) {
    const ResampGeom g = resamp_geom(d.L, d.M);
    const uint64_t TJ = (uint64_t)g.TJ();
    ResampBankParams p;
    memset(&p, 0, sizeof(p));
    p.b.x = d_in;
    p.b.hist = d.d_hist[d.cur].as<c32>();
    p.b.tab = d.d_tab.as<c32>();
    p.b.out = d_out;
    p.b.nin = nin;
    p.b.a = a;
    p.b.n0 = n0;
    p.b.nout = no;
    p.b.J0 = n0 / L;
    p.b.magicM = (1ull << 32) / M + 1;
    p.b.magicL = (1ull << 32) / L + 1;
    p.b.L = d.L;
    p.b.M = d.M;
    p.b.ntaps = d.ntaps;
    p.b.Q = d.hist;
    p.b.QM = resamp_hist_periods(p.b.Q, d.M);
    p.b.W = resamp_pitch(g.TJ(), p.b.QM);
    p.b.TP = g.TJ() | 1;
    p.b.KC = g.kc;
    p.b.scale = h->rx_scale;
    for (int i = 0; i < d.K; i++) p.D[i] = d.D[i];
    p.stride = stride;
    p.K = d.K;
    p.KP = (d.K + 1) & ~1;
    p.NB = resamp_bank_sum_links(d.L, d.M, d.ntaps, d.K);
    const uint64_t periods = (n0 + no + L - 1) / L - p.b.J0;
    const uint64_t grid = (periods + TJ - 1) / TJ;
    RCCHK(stage_check_grid(h, "ofdm_resamp_bank", grid));
    const size_t lds = resamp_bank_lds_bytes(d.L, d.M, d.ntaps, d.K, p.NB);
    RCCHK(stage_time_begin(h, d, timing));
    RCCHK(h->rx_fmt == OFDM_IQ_SC16 ? launch_resamp_bank<sc16>(h, p, g, (unsigned)grid, lds)
                                    : launch_resamp_bank<c32>(h, p, g, (unsigned)grid, lds));
    RCCHK(stage_time_end(h, d, timing));
  }
  RCCHK(stage_roll_rx_history(h, d, d_in, nin));
  RCCHK(stage_rx_readback(h, iq_out, link_stride, K, no, d_out));
  return stage_finish(h, d, nin, timing);
}
