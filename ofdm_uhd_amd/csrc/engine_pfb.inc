// engine_pfb.inc -- host side of the polyphase-FFT channeliser (pfb.h): configuration, launch (the per-channel copy-back: stage_rx_readback).
// Included by engine.hip after engine_stage.inc and engine_ddc.inc (DDC_MAX_INDEX).

/* one set_center_freq per radio channel on a uniform grid (dual_channel/dual_channel.py tunes one channel per link; the
 * sensing apps step through every slot of the band) */
extern "C" int ofdm_set_pfb(ofdm_handle* h, const ofdm_pfb_cfg* cfg) {
  if (!h) return OFDM_E_INVAL;
  PfbState& d = h->pfb;
  if (!cfg) return stage_off(d);
  if (cfg->struct_size != sizeof(ofdm_pfb_cfg)) FAIL(h, OFDM_E_INVAL, "ofdm_pfb_cfg.struct_size does not match this library");
  const uint32_t M = cfg->nchannels;
  if (M < 2 || M > OFDM_PFB_MAX_CHANNELS || (M & (M - 1))) FAIL(h, OFDM_E_INVAL, "channeliser nchannels must be 2, 4, 8, 16, 32 or 64");
  if (cfg->ntaps < 1 || cfg->ntaps > OFDM_PFB_MAX_TAPS) FAIL(h, OFDM_E_INVAL, "channeliser ntaps must be in [1, 1024]");
  if (cfg->nsel < 1 || cfg->nsel > M) FAIL(h, OFDM_E_INVAL, "channeliser nsel must be in [1, nchannels]");
  for (uint32_t i = 0; i < cfg->nsel; i++)
    if (cfg->channel[i] >= M) FAIL(h, OFDM_E_INVAL, "channeliser channel must be below nchannels");
  if (!taps_finite(cfg->taps, cfg->ntaps)) FAIL(h, OFDM_E_INVAL, "channeliser taps must be finite");
  RCCHK(stage_disarm(h, d));
  d.M = (int)M;
  d.ntaps = (int)cfg->ntaps;
  d.K = (int)cfg->nsel;
  // the selection as one list of positions per channel, ascending
  memset(d.sel_first, -1, sizeof(d.sel_first));
  memset(d.sel_next, -1, sizeof(d.sel_next));
  for (int i = d.K - 1; i >= 0; i--) {
    d.sel_next[i] = d.sel_first[cfg->channel[i]];
    d.sel_first[cfg->channel[i]] = (signed char)i;
  }
  // w[j] = complex64(exp(+2 pi i j / M)): float64, rounded once
  std::vector<c32> w(M);
  for (uint32_t j = 0; j < M; j++) {
    const double a = 2.0 * M_PI * (double)j / (double)M;
    w[j] = c32{(float)cos(a), (float)sin(a)};
  }
  HIPCHK(h, upload(d.d_w, w.data(), w.size()));
  HIPCHK(h, upload(d.d_taps, cfg->taps, (size_t)d.ntaps));
  return stage_arm(h, d, d.ntaps - 1);
}

extern "C" int ofdm_pfb_reset(ofdm_handle* h, uint64_t first_sample_index) {
  if (!h) return OFDM_E_INVAL;
  if (!h->pfb.on) FAIL(h, OFDM_E_INVAL, "ofdm_pfb_reset without ofdm_set_pfb");
  if (first_sample_index > DDC_MAX_INDEX) FAIL(h, OFDM_E_INVAL, "ofdm_pfb_reset: first_sample_index must be at most 2^62");
  return stage_reset(h, h->pfb, first_sample_index);
}

// (nin is not bounded here, as in ofdm_ddc_count)
extern "C" int ofdm_pfb_count(const ofdm_handle* h, uint64_t nin, uint64_t* nout) {
  if (!h || !nout) return OFDM_E_INVAL;
  const PfbState& d = h->pfb;
  if (!d.on) return OFDM_E_INVAL;
  *nout = first_output(d.next + nin, 1, (uint64_t)d.M) - first_output(d.next, 1, (uint64_t)d.M);
  return OFDM_OK;
}

extern "C" int ofdm_pfb_last_ms(const ofdm_handle* h, double* ms) {
  if (!h) return OFDM_E_INVAL;
  return stage_last_ms(h->pfb, ms);
}

// (no shape of the definition takes stage_launch past 64 KB of LDS today; a longer filter or a larger tile would)
template <typename XT>
static int launch_pfb(ofdm_handle* h, const PfbParams& p, int M, unsigned grid, size_t lds) {
  switch (M) {
    case 2: return stage_launch(h, &k_pfb<XT, 2>, grid, PFB_THREADS, lds, p);
    case 4: return stage_launch(h, &k_pfb<XT, 4>, grid, PFB_THREADS, lds, p);
    case 8: return stage_launch(h, &k_pfb<XT, 8>, grid, PFB_THREADS, lds, p);
    case 16: return stage_launch(h, &k_pfb<XT, 16>, grid, PFB_THREADS, lds, p);
    case 32: return stage_launch(h, &k_pfb<XT, 32>, grid, PFB_THREADS, lds, p);
    default: return stage_launch(h, &k_pfb<XT, 64>, grid, PFB_THREADS, lds, p);
  }
}

/* the next nin wideband samples in, the samples they complete out, for every selected channel: position i's run begins
 * at iq_out + i * chan_stride */
extern "C" int ofdm_pfb(ofdm_handle* h, const void* iq_in, uint64_t nin, ofdm_c32* iq_out, uint64_t chan_stride, uint64_t out_cap,
                        uint64_t* nout) {
  if (!h) return OFDM_E_INVAL;
  PfbState& d = h->pfb;
  if (!nout) FAIL(h, OFDM_E_INVAL, "null argument");
  if (!d.on) FAIL(h, OFDM_E_INVAL, "ofdm_pfb without ofdm_set_pfb");
  RCCHK(stage_check_rx_in(h, iq_in, nin));
  if ((uintptr_t)iq_out & 7u) FAIL(h, OFDM_E_INVAL, "float32 IQ buffers must be 8-byte aligned");
  const uint64_t M = (uint64_t)d.M, a = d.next, K = (uint64_t)d.K;
  // (indices stay below 2^63: a + nin, the tile's M0 M and the signed sample offsets in the kernel cannot wrap)
  if (nin > DDC_MAX_INDEX || a + nin > 2 * DDC_MAX_INDEX) FAIL(h, OFDM_E_INVAL, "ofdm_pfb: the stream's sample index would pass 2^63");
  const uint64_t m0 = first_output(a, 1, M), no = first_output(a + nin, 1, M) - m0;
  *nout = no;
  if (no > out_cap) FAIL(h, OFDM_E_CAPACITY, "iq_out too small per channel (see ofdm_pfb_count)");
  if (K > 1 && chan_stride < no) FAIL(h, OFDM_E_INVAL, "ofdm_pfb: chan_stride is smaller than the outputs of one channel");
  if (no && !iq_out) FAIL(h, OFDM_E_INVAL, "null iq_out");
  d.timed = false;
  if (nin == 0) return OFDM_OK;
  RCCHK(stage_enter(h));

  const void* d_in = iq_in;
  c32* d_out = reinterpret_cast<c32*>(iq_out);
  uint64_t stride = chan_stride;
  RCCHK(stage_rx_in(h, d, iq_in, nin, &d_in));
  RCCHK(stage_rx_out(h, d, K, no, &d_out, &stride));
  const bool timing = h->prof.on && no > 0;
  if (no) {
    const int T = pfb_tile_outputs(d.M);
    PfbParams p;
    memset(&p, 0, sizeof(p));
    p.b.x = d_in;
    p.b.hist = d.d_hist[d.cur].as<c32>();
    p.b.out = d_out;
    p.b.nin = nin;
    p.b.a = a;
    p.b.m0 = m0;
    p.b.nout = no;
    p.b.magic = (1ull << 32) / M + 1;
    p.b.R = d.M;
    p.b.ntaps = d.ntaps;
    p.b.Q = d.hist / d.M;
    p.b.W = ddc_pitch(T, p.b.Q);
    p.b.scale = h->rx_scale;
    p.taps = d.d_taps.as<float>();
    p.w = d.d_w.as<c32>();
    p.stride = stride;
    memcpy(p.first, d.sel_first, sizeof(p.first));
    memcpy(p.next, d.sel_next, sizeof(p.next));
    const uint64_t grid = (no + (uint64_t)T - 1) / (uint64_t)T;
    RCCHK(stage_check_grid(h, "ofdm_pfb", grid));
    const size_t lds = pfb_lds_bytes(d.M, d.ntaps);
    RCCHK(stage_time_begin(h, d, timing));
    RCCHK(h->rx_fmt == OFDM_IQ_SC16 ? launch_pfb<sc16>(h, p, d.M, (unsigned)grid, lds) : launch_pfb<c32>(h, p, d.M, (unsigned)grid, lds));
    RCCHK(stage_time_end(h, d, timing));
  }
  RCCHK(stage_roll_rx_history(h, d, d_in, nin));
  RCCHK(stage_rx_readback(h, iq_out, chan_stride, K, no, d_out));
  return stage_finish(h, d, nin, timing);
}
