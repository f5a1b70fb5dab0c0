// engine_mempoly.inc -- host side of the memory-polynomial stage (mempoly.h): configuration, launch, statistics.
// Included by engine.hip after engine_cfr.inc; like it, the stage uses the stream skeleton of engine_stage.inc with the
// transmit single shape (no `add`) and the statistics of stream_stats.h.  The handle holds one MempolyState per slot
// (OFDM_MEMPOLY_DPD, OFDM_MEMPOLY_PA): two instances of this one implementation.

static int mempoly_slot(ofdm_handle* h, uint32_t slot, MempolyState** d) {
  if (slot >= OFDM_MEMPOLY_SLOTS) FAIL(h, OFDM_E_INVAL, "mempoly slot must be OFDM_MEMPOLY_DPD or OFDM_MEMPOLY_PA");
  *d = &h->mempoly[slot];
  return OFDM_OK;
}

extern "C" int ofdm_set_mempoly(ofdm_handle* h, uint32_t slot, const ofdm_mempoly_cfg* cfg) {
  if (!h) return OFDM_E_INVAL;
  MempolyState* dp;
  RCCHK(mempoly_slot(h, slot, &dp));
  MempolyState& d = *dp;
  if (!cfg) return stage_off(d);
  if (cfg->struct_size != sizeof(ofdm_mempoly_cfg)) FAIL(h, OFDM_E_INVAL, "ofdm_mempoly_cfg.struct_size does not match this library");
  static_assert(OFDM_MEMPOLY_MAX_MEMORY == 8 && OFDM_MEMPOLY_MAX_ORDERS == 5, "the messages below name the limits");
  if (cfg->memory < 1 || cfg->memory > OFDM_MEMPOLY_MAX_MEMORY) FAIL(h, OFDM_E_INVAL, "mempoly memory must be in [1, 8]");
  if (cfg->orders < 1 || cfg->orders > OFDM_MEMPOLY_MAX_ORDERS) FAIL(h, OFDM_E_INVAL, "mempoly orders must be in [1, 5]");
  for (uint32_t m = 0; m < cfg->memory; m++)
    for (uint32_t k = 0; k < cfg->orders; k++) {
      const ofdm_c32& c = cfg->coef[m * OFDM_MEMPOLY_MAX_ORDERS + k];
      if (!(std::isfinite(c.re) && std::isfinite(c.im))) FAIL(h, OFDM_E_INVAL, "mempoly coef must be finite");
    }
  if (!(cfg->limit > 0.0f)) FAIL(h, OFDM_E_INVAL, "mempoly limit must be positive (+inf: nothing is counted)");
  float scale;
  RCCHK(stage_out_scale(h, "mempoly", cfg->out_format, cfg->out_scale, &scale));
  RCCHK(stage_disarm(h, d));
  d.M = (int)cfg->memory;
  d.K = (int)cfg->orders;
  d.out_fmt = (int)cfg->out_format;
  d.out_scale = scale;
  d.limit2 = cfg->limit * cfg->limit;
  memset(d.a, 0, sizeof(d.a));
  for (int m = 0; m < d.M; m++)
    for (int k = 0; k < d.K; k++) {
      const ofdm_c32& c = cfg->coef[m * OFDM_MEMPOLY_MAX_ORDERS + k];
      d.a[m][k] = c32{c.re, c.im};
    }
  RCCHK(stage_stats_zero(h, d.st));
  return stage_arm(h, d, d.M - 1);
}

extern "C" int ofdm_mempoly_reset(ofdm_handle* h, uint32_t slot) {
  if (!h) return OFDM_E_INVAL;
  MempolyState* dp;
  RCCHK(mempoly_slot(h, slot, &dp));
  MempolyState& d = *dp;
  if (!d.on) FAIL(h, OFDM_E_INVAL, "ofdm_mempoly_reset without ofdm_set_mempoly");
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  RCCHK(stage_stats_zero(h, d.st));
  return stage_reset(h, d, 0);
}

extern "C" int ofdm_mempoly_last_ms(const ofdm_handle* h, uint32_t slot, double* ms) {
  if (!h || slot >= OFDM_MEMPOLY_SLOTS) return OFDM_E_INVAL;
  return stage_last_ms(h->mempoly[slot], ms);
}

extern "C" int ofdm_mempoly_stats(ofdm_handle* h, uint32_t slot, struct ofdm_mempoly_stats* out) {
  if (!h) return OFDM_E_INVAL;
  MempolyState* dp;
  RCCHK(mempoly_slot(h, slot, &dp));
  MempolyState& d = *dp;
  if (!out) FAIL(h, OFDM_E_INVAL, "null argument");
  if (!d.on) FAIL(h, OFDM_E_INVAL, "ofdm_mempoly_stats without ofdm_set_mempoly");
  StatTotals t;
  RCCHK(stage_stats_read(h, d.st, &t));
  out->n = d.st.n;
  out->n_over = t.n_over;
  out->peak_in = t.peak_in;
  out->peak_out = t.peak_out;
  out->sum_in = t.sum_in;
  out->sum_out = t.sum_out;
  return OFDM_OK;
}

// k_mempoly<OUT, K> for the stage's output format and number of orders
template <typename OUT>
static void mempoly_launch(ofdm_handle* h, int K, unsigned grid, const MempolyParams& p) {
  const dim3 g(grid), b(MPOLY_THREADS);
  switch (K) {
    case 1: hipLaunchKernelGGL(HIP_KERNEL_NAME(k_mempoly<OUT, 1>), g, b, 0, h->stream, p); break;
    case 2: hipLaunchKernelGGL(HIP_KERNEL_NAME(k_mempoly<OUT, 2>), g, b, 0, h->stream, p); break;
    case 3: hipLaunchKernelGGL(HIP_KERNEL_NAME(k_mempoly<OUT, 3>), g, b, 0, h->stream, p); break;
    case 4: hipLaunchKernelGGL(HIP_KERNEL_NAME(k_mempoly<OUT, 4>), g, b, 0, h->stream, p); break;
    default: hipLaunchKernelGGL(HIP_KERNEL_NAME(k_mempoly<OUT, 5>), g, b, 0, h->stream, p); break;
  }
}

/* the next nin samples of the slot's stream in, nin samples out */
extern "C" int ofdm_mempoly(ofdm_handle* h, uint32_t slot, const ofdm_c32* iq_in, uint64_t nin, void* iq_out, uint64_t out_cap,
                            uint64_t* nout) {
  if (!h) return OFDM_E_INVAL;
  MempolyState* dp;
  RCCHK(mempoly_slot(h, slot, &dp));
  MempolyState& d = *dp;
  if (!nout) FAIL(h, OFDM_E_INVAL, "null argument");
  if (!d.on) FAIL(h, OFDM_E_INVAL, "ofdm_mempoly without ofdm_set_mempoly");
  const bool s16 = d.out_fmt == OFDM_IQ_SC16;
  RCCHK(stage_check_tx_bufs(h, s16, iq_in, nin, nullptr, iq_out));
  *nout = nin;
  if (nin > out_cap) FAIL(h, OFDM_E_CAPACITY, "iq_out too small (nin samples)");
  if (nin && !iq_out) FAIL(h, OFDM_E_INVAL, "null iq_out");
  const size_t oss = s16 ? sizeof(sc16) : sizeof(c32);
  {
    // a tile reads the inputs of its neighbour's outputs: the two buffers may not share a byte
    const uintptr_t i0 = (uintptr_t)iq_in, i1 = i0 + nin * sizeof(c32), o0 = (uintptr_t)iq_out, o1 = o0 + nin * oss;
    if (nin && i0 < o1 && o0 < i1) FAIL(h, OFDM_E_INVAL, "ofdm_mempoly: iq_in overlaps iq_out");
  }
  d.timed = false;
  if (nin == 0) return OFDM_OK;
  const uint64_t grid = (nin + (uint64_t)MPOLY_TILE - 1) / (uint64_t)MPOLY_TILE;
  if (!stage_stats_fits(grid)) FAIL(h, OFDM_E_INVAL, "ofdm_mempoly: call too long (split it)");
  RCCHK(stage_enter(h));

  const c32* d_in = reinterpret_cast<const c32*>(iq_in);
  const c32* d_add = nullptr;
  void* d_out = iq_out;
  RCCHK(stage_tx_rows_in(h, d, iq_in, 0, 1, nin, &d_in, nullptr));
  RCCHK(stage_tx_out(h, d, nullptr, nin, oss, &d_add, &d_out));
  RCCHK(stage_stats_room(h, d.st, grid));
  const bool timing = h->prof.on;
  MempolyParams p;
  memset(&p, 0, sizeof(p));
  p.x = d_in;
  p.hist = d.d_hist[d.cur].as<c32>();
  p.out = d_out;
  p.part = d.st.d_part.as<StatPartial>();
  p.nin = nin;
  p.M = d.M;
  p.limit2 = d.limit2;
  p.scale = d.out_scale;
  memcpy(p.a, d.a, sizeof(p.a));
  RCCHK(stage_time_begin(h, d, timing));
  if (s16) mempoly_launch<sc16>(h, d.K, (unsigned)grid, p);
  else mempoly_launch<c32>(h, d.K, (unsigned)grid, p);
  stage_stats_reduce(h, d.st, grid);
  RCCHK(stage_time_end(h, d, timing));
  RCCHK(stage_roll_history(h, d, d_in, nin, 0.f));
  RCCHK(stage_tx_readback(h, iq_out, d_out, nin, oss));
  RCCHK(stage_finish(h, d, nin, timing));
  d.st.n += nin;
  return OFDM_OK;
}
