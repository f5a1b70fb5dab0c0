// engine_ddc_bank.inc -- host side of the DDC bank (ddc_bank.h): configuration, launches (the per-link copy-back: stage_rx_readback).
// Included by engine.hip after engine_stage.inc and engine_ddc.inc (DDC_MAX_INDEX).

/* K gr.freq_xlating_fir_filter_ccf ctors that share decimation and prototype (dual_channel/dual_channel.py tunes one
 * radio channel per link) */
extern "C" int ofdm_set_ddc_bank(ofdm_handle* h, const ofdm_ddc_bank_cfg* cfg) {
  if (!h) return OFDM_E_INVAL;
  DdcBankState& d = h->bank;
  if (!cfg) return stage_off(d);
  if (cfg->struct_size != sizeof(ofdm_ddc_bank_cfg)) FAIL(h, OFDM_E_INVAL, "ofdm_ddc_bank_cfg.struct_size does not match this library");
  if (cfg->decimation < 1 || cfg->decimation > DDC_MAX_DECIM) FAIL(h, OFDM_E_INVAL, "DDC bank decimation must be in [1, 64]");
  if (cfg->ntaps < 1 || cfg->ntaps > OFDM_DDC_MAX_TAPS) FAIL(h, OFDM_E_INVAL, "DDC bank ntaps must be in [1, 1024]");
  RCCHK(stage_check_nlinks(h, "DDC bank", cfg->nlinks));
  RCCHK(stage_check_center_freqs(h, "DDC bank", cfg->center_freq, cfg->nlinks, "sample"));
  if (!taps_finite(cfg->taps, cfg->ntaps)) FAIL(h, OFDM_E_INVAL, "DDC bank taps must be finite");
  RCCHK(stage_disarm(h, d));
  d.R = (int)cfg->decimation;
  d.ntaps = (int)cfg->ntaps;
  d.K = (int)cfg->nlinks;
  const int KP = (d.K + 1) & ~1;
  // every link's table is the DDC's; the device copy is link-minor
  d.tab = bank_tables(cfg->taps, d.ntaps, cfg->center_freq, d.K, 1);
  std::vector<c32> dev((size_t)d.ntaps * KP, c32{0.f, 0.f});
  for (int i = 0; i < d.K; i++) {
    d.fc[i] = cfg->center_freq[i];
    d.D[i] = ddc_turns(d.fc[i] * (double)d.R);
    for (int k = 0; k < d.ntaps; k++) dev[(size_t)k * KP + i] = d.tab[(size_t)i * d.ntaps + k];
  }
  HIPCHK(h, upload(d.d_tab, dev.data(), dev.size()));
  return stage_arm(h, d, d.ntaps - 1);
}

extern "C" int ofdm_ddc_bank_reset(ofdm_handle* h, uint64_t first_sample_index) {
  if (!h) return OFDM_E_INVAL;
  if (!h->bank.on) FAIL(h, OFDM_E_INVAL, "ofdm_ddc_bank_reset without ofdm_set_ddc_bank");
  if (first_sample_index > DDC_MAX_INDEX) FAIL(h, OFDM_E_INVAL, "ofdm_ddc_bank_reset: first_sample_index must be at most 2^62");
  return stage_reset(h, h->bank, first_sample_index);
}

// (nin is not bounded here, as in ofdm_ddc_count)
extern "C" int ofdm_ddc_bank_count(const ofdm_handle* h, uint64_t nin, uint64_t* nout) {
  if (!h || !nout) return OFDM_E_INVAL;
  const DdcBankState& d = h->bank;
  if (!d.on) return OFDM_E_INVAL;
  *nout = first_output(d.next + nin, 1, (uint64_t)d.R) - first_output(d.next, 1, (uint64_t)d.R);
  return OFDM_OK;
}

extern "C" int ofdm_ddc_bank_taps(const ofdm_handle* h, int link, ofdm_c32* out, int cap, int* n) {
  if (!h || !n) return OFDM_E_INVAL;
  const DdcBankState& d = h->bank;
  return stage_bank_taps(d.on, d.tab, d.ntaps, d.K, link, out, cap, n);
}

extern "C" int ofdm_ddc_bank_last_ms(const ofdm_handle* h, double* ms) {
  if (!h) return OFDM_E_INVAL;
  return stage_last_ms(h->bank, ms);
}

template <typename XT>
static int launch_ddc_bank(ofdm_handle* h, const DdcBankParams& p, const DdcGeom& g, unsigned grid, size_t lds) {
  if (g.opt == 4 && g.tj == 256) return stage_launch(h, &k_ddc_bank<XT, 4, 256>, grid, DDC_THREADS, lds, p);
  if (g.opt == 4) return stage_launch(h, &k_ddc_bank<XT, 4, 64>, grid, DDC_THREADS, lds, p);
  return stage_launch(h, &k_ddc_bank<XT, 1, 64>, grid, DDC_THREADS, lds, p);
}

/* the next nin wideband samples in, the narrowband samples they complete out, for every link: link i's run begins at
 * iq_out + i * link_stride */
extern "C" int ofdm_ddc_bank(ofdm_handle* h, const void* iq_in, uint64_t nin, ofdm_c32* iq_out, uint64_t link_stride, uint64_t out_cap,
                             uint64_t* nout) {
  if (!h) return OFDM_E_INVAL;
  DdcBankState& d = h->bank;
  if (!nout) FAIL(h, OFDM_E_INVAL, "null argument");
  if (!d.on) FAIL(h, OFDM_E_INVAL, "ofdm_ddc_bank without ofdm_set_ddc_bank");
  RCCHK(stage_check_rx_in(h, iq_in, nin));
  const uint64_t R = (uint64_t)d.R, a = d.next, K = (uint64_t)d.K;
  // (indices stay below 2^63: a + nin, the tile's M0 R and the signed sample offsets in the kernel cannot wrap)
  if (nin > DDC_MAX_INDEX || a + nin > 2 * DDC_MAX_INDEX) FAIL(h, OFDM_E_INVAL, "ofdm_ddc_bank: the stream's sample index would pass 2^63");
  const uint64_t m0 = first_output(a, 1, R), no = first_output(a + nin, 1, R) - m0;
  *nout = no;
  if (no > out_cap) FAIL(h, OFDM_E_CAPACITY, "iq_out too small per link (see ofdm_ddc_bank_count)");
  if (K > 1 && link_stride < no) FAIL(h, OFDM_E_INVAL, "ofdm_ddc_bank: link_stride is smaller than the outputs of one link");
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
    const DdcGeom g = ddc_geom(d.R);
    DdcBankParams p;
    memset(&p, 0, sizeof(p));
    p.b.x = d_in;
    p.b.hist = d.d_hist[d.cur].as<c32>();
    p.b.tab = d.d_tab.as<c32>();
    p.b.out = d_out;
    p.b.nin = nin;
    p.b.a = a;
    p.b.m0 = m0;
    p.b.nout = no;
    p.b.magic = (1ull << 32) / R + 1;
    p.b.R = d.R;
    p.b.ntaps = d.ntaps;
    p.b.Q = d.hist / d.R;
    p.b.W = ddc_pitch(g.T(), p.b.Q);
    p.b.scale = h->rx_scale;
    for (int i = 0; i < d.K; i++) p.D[i] = d.D[i];
    p.stride = stride;
    p.K = d.K;
    p.KP = (d.K + 1) & ~1;
    const uint64_t grid = (no + (uint64_t)g.T() - 1) / (uint64_t)g.T();
    RCCHK(stage_check_grid(h, "ofdm_ddc_bank", grid));
    const size_t lds = ddc_bank_lds_bytes(d.R, d.ntaps, d.K);
    RCCHK(stage_time_begin(h, d, timing));
    RCCHK(h->rx_fmt == OFDM_IQ_SC16 ? launch_ddc_bank<sc16>(h, p, g, (unsigned)grid, lds) : launch_ddc_bank<c32>(h, p, g, (unsigned)grid, lds));
    RCCHK(stage_time_end(h, d, timing));
  }
  RCCHK(stage_roll_rx_history(h, d, d_in, nin));
  RCCHK(stage_rx_readback(h, iq_out, link_stride, K, no, d_out));
  return stage_finish(h, d, nin, timing);
}
