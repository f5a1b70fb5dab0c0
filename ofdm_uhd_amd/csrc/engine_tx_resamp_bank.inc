// engine_tx_resamp_bank.inc -- host side of the transmit resampler bank (tx_resamp_bank.h): configuration, index
// limits, launch (the per-link upload: stage_tx_rows_in).  Included by engine.hip after engine_stage.inc and engine_tx_resamp.inc
// (TX_RESAMP_MAX_INDEX).

/* K blks2.rational_resampler_ccf(interpolation, decimation, taps) + set_center_freq that share ratio and prototype,
 * summed onto one band */
extern "C" int ofdm_set_tx_resamp_bank(ofdm_handle* h, const ofdm_tx_resamp_bank_cfg* cfg) {
  if (!h) return OFDM_E_INVAL;
  TxResampBankState& d = h->tx_resamp_bank;
  if (!cfg) return stage_off(d);
  if (cfg->struct_size != sizeof(ofdm_tx_resamp_bank_cfg)) FAIL(h, OFDM_E_INVAL, "ofdm_tx_resamp_bank_cfg.struct_size does not match this library");
  if (cfg->interpolation < 1 || cfg->interpolation > TX_RESAMP_MAX_RATIO) FAIL(h, OFDM_E_INVAL, "transmit resampler bank interpolation must be in [1, 64]");
  if (cfg->decimation < 1 || cfg->decimation > TX_RESAMP_MAX_RATIO) FAIL(h, OFDM_E_INVAL, "transmit resampler bank decimation must be in [1, 64]");
  if (cfg->ntaps < 1 || cfg->ntaps > OFDM_TX_RESAMP_MAX_TAPS) FAIL(h, OFDM_E_INVAL, "transmit resampler bank ntaps must be in [1, 1024]");
  RCCHK(stage_check_nlinks(h, "transmit resampler bank", cfg->nlinks));
  float scale;
  RCCHK(stage_out_scale(h, "transmit resampler bank", cfg->out_format, cfg->out_scale, &scale));
  RCCHK(stage_check_center_freqs(h, "transmit resampler bank", cfg->center_freq, cfg->nlinks, "output sample"));
  if (!taps_finite(cfg->taps, cfg->ntaps)) FAIL(h, OFDM_E_INVAL, "transmit resampler bank taps must be finite");
  // (holds for every ratio and length accepted above; the launch relies on it)
  if (tx_resamp_bank_lds_bytes((int)cfg->interpolation, (int)cfg->decimation, (int)cfg->ntaps) > TX_RESAMP_BANK_MAX_LDS)
    FAIL(h, OFDM_E_INVAL, "transmit resampler bank: the tile does not fit the workgroup's memory");
  RCCHK(stage_disarm(h, d));
  d.L = (int)cfg->interpolation;
  d.M = (int)cfg->decimation;
  d.ntaps = (int)cfg->ntaps;
  d.K = (int)cfg->nlinks;
  d.Q = (d.ntaps - 1) / d.L;
  d.out_fmt = (int)cfg->out_format;
  d.out_scale = scale;
  // G = turns(fc / M), the phase per step of the L-times grid (ONE double division: the table below divides the same
  // way); a link's step per INPUT is L G modulo a turn.  Its table is the receive bank's at interpolation = M.
  d.tab = bank_tables(cfg->taps, d.ntaps, cfg->center_freq, d.K, d.M);
  for (int i = 0; i < d.K; i++) d.E[i] = ddc_turns(cfg->center_freq[i] / (double)d.M) * (uint64_t)d.L;
  HIPCHK(h, upload(d.d_tab, d.tab.data(), d.tab.size()));
  return stage_arm(h, d, d.K * d.Q);  // the last Q raw inputs of every link
}

extern "C" int ofdm_tx_resamp_bank_reset(ofdm_handle* h, uint64_t first_input_index) {
  if (!h) return OFDM_E_INVAL;
  if (!h->tx_resamp_bank.on) FAIL(h, OFDM_E_INVAL, "ofdm_tx_resamp_bank_reset without ofdm_set_tx_resamp_bank");
  if (first_input_index > TX_RESAMP_MAX_INDEX) FAIL(h, OFDM_E_INVAL, "ofdm_tx_resamp_bank_reset: first_input_index must be at most 2^56");
  return stage_reset(h, h->tx_resamp_bank, first_input_index);
}

extern "C" int ofdm_tx_resamp_bank_count(const ofdm_handle* h, uint64_t nin, uint64_t* nout) {
  if (!h || !nout) return OFDM_E_INVAL;
  const TxResampBankState& d = h->tx_resamp_bank;
  if (!d.on) return OFDM_E_INVAL;
  if (nin > TX_RESAMP_MAX_INDEX || d.next + nin > TX_RESAMP_MAX_INDEX) return OFDM_E_INVAL;
  *nout = first_output(d.next + nin, (uint64_t)d.L, (uint64_t)d.M) - first_output(d.next, (uint64_t)d.L, (uint64_t)d.M);
  return OFDM_OK;
}

extern "C" int ofdm_tx_resamp_bank_taps(const ofdm_handle* h, int link, ofdm_c32* out, int cap, int* n) {
  if (!h || !n) return OFDM_E_INVAL;
  const TxResampBankState& d = h->tx_resamp_bank;
  return stage_bank_taps(d.on, d.tab, d.ntaps, d.K, link, out, cap, n);
}

extern "C" int ofdm_tx_resamp_bank_last_ms(const ofdm_handle* h, double* ms) {
  if (!h) return OFDM_E_INVAL;
  return stage_last_ms(h->tx_resamp_bank, ms);
}

/* the next nin samples of every link in (link i's run begins at iq_in + i * link_stride), the samples of the band at
 * L / M times their rate that they complete out (optionally added onto a band that is there) */
extern "C" int ofdm_tx_resamp_bank(ofdm_handle* h, const ofdm_c32* iq_in, uint64_t link_stride, uint64_t nin, const ofdm_c32* add, void* iq_out,
                                   uint64_t out_cap, uint64_t* nout) {
  if (!h) return OFDM_E_INVAL;
  TxResampBankState& d = h->tx_resamp_bank;
  if (!nout) FAIL(h, OFDM_E_INVAL, "null argument");
  if (!d.on) FAIL(h, OFDM_E_INVAL, "ofdm_tx_resamp_bank without ofdm_set_tx_resamp_bank");
  const bool s16 = d.out_fmt == OFDM_IQ_SC16;
  RCCHK(stage_check_tx_bufs(h, s16, iq_in, nin, add, iq_out));
  const uint64_t L = (uint64_t)d.L, M = (uint64_t)d.M, K = (uint64_t)d.K, a = d.next;
  if (nin > TX_RESAMP_MAX_INDEX || a + nin > TX_RESAMP_MAX_INDEX) FAIL(h, OFDM_E_INVAL, "ofdm_tx_resamp_bank: the stream's input index would pass 2^56");
  const uint64_t n0 = first_output(a, L, M), no = first_output(a + nin, L, M) - n0;
  *nout = no;
  if (no > out_cap) FAIL(h, OFDM_E_CAPACITY, "iq_out too small (see ofdm_tx_resamp_bank_count)");
  if (K > 1 && link_stride < nin) FAIL(h, OFDM_E_INVAL, "ofdm_tx_resamp_bank: link_stride is smaller than the inputs of one link");
  if (no && !iq_out) FAIL(h, OFDM_E_INVAL, "null iq_out");
  d.timed = false;
  if (nin == 0) return OFDM_OK;
  const TxResampGeom g = tx_resamp_geom(d.L, d.M);
  const uint64_t TJ = (uint64_t)g.TJ(), J0 = n0 / L;
  const uint64_t grid = no ? ((n0 + no + L - 1) / L - J0 + TJ - 1) / TJ : 0;
  RCCHK(stage_check_grid(h, "ofdm_tx_resamp_bank", grid));
  RCCHK(stage_enter(h));

  const size_t oss = s16 ? sizeof(sc16) : sizeof(c32);
  const c32* d_in = reinterpret_cast<const c32*>(iq_in);
  const c32* d_add = reinterpret_cast<const c32*>(add);
  void* d_out = iq_out;
  uint64_t stride = link_stride;
  RCCHK(stage_tx_rows_in(h, d, iq_in, link_stride, K, nin, &d_in, &stride));
  if (no) RCCHK(stage_tx_out(h, d, add, no, oss, &d_add, &d_out));
  const bool timing = h->prof.on && no > 0;
  if (no) {
    TxResampBankParams p;
    memset(&p, 0, sizeof(p));
    p.x = d_in;
    p.hist = d.d_hist[d.cur].as<c32>();
    p.tab = d.d_tab.as<c32>();
    p.add = d_add;
    p.out = d_out;
    p.nin = nin;
    p.stride = stride;
    p.a = a;
    p.n0 = n0;
    p.nout = no;
    p.J0 = J0;
    memcpy(p.E, d.E, sizeof(p.E));
    p.magicM = (1ull << 32) / M + 1;
    p.magicL = (1ull << 32) / L + 1;
    p.L = d.L;
    p.M = d.M;
    p.ntaps = d.ntaps;
    p.Q = d.Q;
    p.QM = resamp_hist_periods(d.Q, d.M);
    p.W = resamp_pitch(g.TJ(), p.QM);
    p.TP = g.TJ() | 1;
    p.KC = g.kc;
    p.K = d.K;
    p.scale = d.out_scale;
    const size_t lds = tx_resamp_bank_lds_bytes(d.L, d.M, d.ntaps);
    RCCHK(stage_time_begin(h, d, timing));
    RCCHK(stage_tx_variant(s16, add != nullptr, [&](auto o, auto a) {
      return stage_launch(h, &k_tx_resamp_bank<decltype(o), decltype(a)::value>, (unsigned)grid, TX_RESAMP_THREADS, lds, p);
    }));
    RCCHK(stage_time_end(h, d, timing));
  }
  RCCHK(stage_roll_rows_history(h, d, d_in, stride, nin, d.Q, d.K));
  if (no) RCCHK(stage_tx_readback(h, iq_out, d_out, no, oss));
  return stage_finish(h, d, nin, timing);
}
