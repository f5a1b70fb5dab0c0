// engine_ddc.inc -- host side of the wideband front end (ddc.h): configuration, index limits, launches.
// Included by engine.hip after engine_stage.inc (the stream skeleton it shares with the other wideband stages).

constexpr uint64_t DDC_MAX_INDEX = 1ull << 62;  // largest first_sample_index; a stream may run on to 2^63

/* usrp2.source_32fc.set_decim + set_center_freq (usrp_receive_path.py) = gr.freq_xlating_fir_filter_ccf's ctor */
extern "C" int ofdm_set_ddc(ofdm_handle* h, const ofdm_ddc_cfg* cfg) {
  if (!h) return OFDM_E_INVAL;
  DdcState& d = h->ddc;
  if (!cfg) return stage_off(d);
  if (cfg->struct_size != sizeof(ofdm_ddc_cfg)) FAIL(h, OFDM_E_INVAL, "ofdm_ddc_cfg.struct_size does not match this library");
  if (cfg->decimation < 1 || cfg->decimation > DDC_MAX_DECIM) FAIL(h, OFDM_E_INVAL, "DDC decimation must be in [1, 64]");
  if (cfg->ntaps < 1 || cfg->ntaps > OFDM_DDC_MAX_TAPS) FAIL(h, OFDM_E_INVAL, "DDC ntaps must be in [1, 1024]");
  RCCHK(stage_check_center_freqs(h, "DDC", &cfg->center_freq, 1, "sample"));
  if (!taps_finite(cfg->taps, cfg->ntaps)) FAIL(h, OFDM_E_INVAL, "DDC taps must be finite");
  RCCHK(stage_disarm(h, d));
  d.R = (int)cfg->decimation;
  d.ntaps = (int)cfg->ntaps;
  d.fc = cfg->center_freq;
  d.D = ddc_turns(d.fc * (double)d.R);
  d.tab = bandpass_table(cfg->taps, d.ntaps, d.fc, 1);
  HIPCHK(h, upload(d.d_tab, d.tab.data(), d.tab.size()));
  return stage_arm(h, d, d.ntaps - 1);
}

extern "C" int ofdm_ddc_reset(ofdm_handle* h, uint64_t first_sample_index) {
  if (!h) return OFDM_E_INVAL;
  if (!h->ddc.on) FAIL(h, OFDM_E_INVAL, "ofdm_ddc_reset without ofdm_set_ddc");
  if (first_sample_index > DDC_MAX_INDEX) FAIL(h, OFDM_E_INVAL, "ofdm_ddc_reset: first_sample_index must be at most 2^62");
  return stage_reset(h, h->ddc, first_sample_index);
}

// (outputs m with a <= m R < a + n; nin is not bounded here)
extern "C" int ofdm_ddc_count(const ofdm_handle* h, uint64_t nin, uint64_t* nout) {
  if (!h || !nout) return OFDM_E_INVAL;
  const DdcState& d = h->ddc;
  if (!d.on) return OFDM_E_INVAL;
  *nout = first_output(d.next + nin, 1, (uint64_t)d.R) - first_output(d.next, 1, (uint64_t)d.R);
  return OFDM_OK;
}

extern "C" int ofdm_ddc_taps(const ofdm_handle* h, ofdm_c32* out, int cap, int* n) {
  if (!h || !n || !h->ddc.on) return OFDM_E_INVAL;
  return stage_taps_out(h->ddc.tab.data(), h->ddc.ntaps, out, cap, n);
}

extern "C" int ofdm_ddc_last_ms(const ofdm_handle* h, double* ms) {
  if (!h) return OFDM_E_INVAL;
  return stage_last_ms(h->ddc, ms);
}

template <typename XT, int OPT, int TJ>
static void launch_ddc_g(ofdm_handle* h, const DdcParams& p, unsigned grid, size_t lds) {
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ddc<XT, OPT, TJ>), dim3(grid), dim3(DDC_THREADS), lds, h->stream, p);
}
template <typename XT>
static void launch_ddc(ofdm_handle* h, const DdcParams& p, const DdcGeom& g, unsigned grid, size_t lds) {
  if (g.opt == 4 && g.tj == 256) launch_ddc_g<XT, 4, 256>(h, p, grid, lds);
  else if (g.opt == 4) launch_ddc_g<XT, 4, 64>(h, p, grid, lds);
  else launch_ddc_g<XT, 1, 64>(h, p, grid, lds);
}

/* gr.freq_xlating_fir_filter_ccf::work: the next nin wideband samples in, the narrowband samples they complete out */
extern "C" int ofdm_ddc(ofdm_handle* h, const void* iq_in, uint64_t nin, ofdm_c32* iq_out, uint64_t out_cap, uint64_t* nout) {
  if (!h) return OFDM_E_INVAL;
  DdcState& d = h->ddc;
  if (!nout) FAIL(h, OFDM_E_INVAL, "null argument");
  if (!d.on) FAIL(h, OFDM_E_INVAL, "ofdm_ddc without ofdm_set_ddc");
  RCCHK(stage_check_rx_in(h, iq_in, nin));
  const uint64_t R = (uint64_t)d.R, a = d.next;
  // (indices stay below 2^63: a + nin, the tile's M0 R and the signed sample offsets in the kernel cannot wrap)
  if (nin > DDC_MAX_INDEX || a + nin > 2 * DDC_MAX_INDEX) FAIL(h, OFDM_E_INVAL, "ofdm_ddc: the stream's sample index would pass 2^63");
  const uint64_t m0 = first_output(a, 1, R), no = first_output(a + nin, 1, R) - m0;
  *nout = no;
  if (no > out_cap) FAIL(h, OFDM_E_CAPACITY, "iq_out too small (see ofdm_ddc_count)");
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
    const DdcGeom g = ddc_geom(d.R);
    DdcParams p;
    memset(&p, 0, sizeof(p));
    p.x = d_in;
    p.hist = d.d_hist[d.cur].as<c32>();
    p.tab = d.d_tab.as<c32>();
    p.out = d_out;
    p.nin = nin;
    p.a = a;
    p.m0 = m0;
    p.nout = no;
    p.D = d.D;
    p.magic = (1ull << 32) / R + 1;
    p.R = d.R;
    p.ntaps = d.ntaps;
    p.Q = d.hist / d.R;
    p.W = ddc_pitch(g.T(), p.Q);
    p.scale = h->rx_scale;
    const uint64_t grid = (no + (uint64_t)g.T() - 1) / (uint64_t)g.T();
    RCCHK(stage_check_grid(h, "ofdm_ddc", grid));
    const size_t lds = ddc_lds_bytes(d.R, d.ntaps);  // (never more than 64 KB: no hipFuncSetAttribute)
    RCCHK(stage_time_begin(h, d, timing));
    if (h->rx_fmt == OFDM_IQ_SC16) launch_ddc<sc16>(h, p, g, (unsigned)grid, lds);
    else launch_ddc<c32>(h, p, g, (unsigned)grid, lds);
    RCCHK(stage_time_end(h, d, timing));
  }
  RCCHK(stage_roll_rx_history(h, d, d_in, nin));
  RCCHK(stage_rx_readback(h, iq_out, 0, 1, no, d_out));
  return stage_finish(h, d, nin, timing);
}
