// engine_rx.inc -- host orchestration of the receive path (included by engine.hip).

// exclusive scan of n elements on the handle's stream; *d_total (device, optional) receives the sum
template <typename T>
static int dev_excl_scan(ofdm_handle* h, const T* d_in, uint64_t n, T* d_out, T* d_total) {
  const uint64_t nb = (n + SCAN_BLOCK - 1) / SCAN_BLOCK;
  HIPCHK(h, h->rx.partial.ensure(sizeof(T) * std::max<uint64_t>(nb, 1)));
  T* part = h->rx.partial.as<T>();
  if (n == 0) {
    if (d_total) HIPCHK(h, hipMemsetAsync(d_total, 0, sizeof(T), h->stream));
    return OFDM_OK;
  }
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_scan_partials<T>), dim3((unsigned)nb), dim3(256), 0, h->stream, d_in, n, part);
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_scan_top<T>), dim3(1), dim3(256), 0, h->stream, part, nb, d_total);
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_scan_final<T>), dim3((unsigned)nb), dim3(256), 0, h->stream, d_in, n, part, d_out);
  HIPCHK(h, hipGetLastError());
  return OFDM_OK;
}

template <int N, bool TWL, bool TAPS, bool CSI = false>
static int launch_demod_t(ofdm_handle* h, const DemodParams& q, size_t shmem) {
  constexpr int T = N / 8, FPW = demod_fpw(N);
  if (shmem > 64 * 1024)
    HIPCHK(h, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_rx_demod<N, TWL, TAPS, CSI>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_rx_demod<N, TWL, TAPS, CSI>), dim3((q.nframes + FPW - 1) / FPW), dim3(T * FPW), shmem,
                     h->stream, q);
  HIPCHK(h, hipGetLastError());
  return OFDM_OK;
}
// (a call without symbol taps and without link quality runs the kernel compiled without them: rx_demod.h; a call with
// per-subcarrier channel state runs the CSI instantiation for its optimistic pass)
template <int N, bool TWL>
static int launch_demod_v(ofdm_handle* h, const DemodParams& q, size_t shmem) {
  if (q.csi_eq) return launch_demod_t<N, TWL, true, true>(h, q, shmem);
  const bool instr = q.tap_mode != 0 || q.tap_sampler || q.tap_fft || q.tap_acq || q.tap_sink || q.tap_demapped || q.qual;
  return instr ? launch_demod_t<N, TWL, true>(h, q, shmem) : launch_demod_t<N, TWL, false>(h, q, shmem);
}

// LDS extras of the demodulator (twiddle table for long transforms, the sink's carrier map): demod_launch_choice
// (rx_demod.h) decides from the geometry, the tuning knob afterwards.
template <int N>
static int launch_demod(ofdm_handle* h, const DemodParams& q0) {
  DemodParams q = q0;
  const bool grid = q.grid != nullptr;
  const bool csi = q.csi_eq != nullptr;
  const DemodLaunch dl = demod_launch_choice(N, q.occ, q.arity, q.nmap, q.nbits, q.shift, grid, csi);
  bool twl = dl.twl;
  q.smap_lds = dl.smap_lds ? 1 : 0;
  if (const char* e = getenv("OFDM_DEMOD_LDS")) {  // tuning knob: bit 0 twiddles (N >= 2048), bit 1 carrier map
    const int v = atoi(e);
    if constexpr (fft_onebuf(N)) twl = (v & 1) != 0;
    q.smap_lds = (v >> 1) & 1;
  }
  const size_t shmem = (size_t)demod_lds_bytes(N, twl, q.smap_lds != 0, q.occ, q.arity, q.nmap, q.nbits, q.shift, grid, csi);
  if (shmem > CU_LDS_BYTES) FAIL(h, OFDM_E_INVAL, "configuration needs more than 160 KiB of LDS in k_rx_demod");
  if constexpr (fft_onebuf(N)) {
    return twl ? launch_demod_v<N, true>(h, q, shmem) : launch_demod_v<N, false>(h, q, shmem);
  } else {
    return launch_demod_v<N, true>(h, q, shmem);
  }
}

static int run_demod(ofdm_handle* h, const DemodParams& q) {
  switch (h->N) {
    case 64: return launch_demod<64>(h, q);
    case 128: return launch_demod<128>(h, q);
    case 256: return launch_demod<256>(h, q);
    case 512: return launch_demod<512>(h, q);
    case 1024: return launch_demod<1024>(h, q);
    case 2048: return launch_demod<2048>(h, q);
    default: return launch_demod<4096>(h, q);
  }
}

// counter slots in rx.counters (uint64 each)
enum { CT_CAND = 0, CT_OVERFLOW = 1, CT_NLO = 2, CT_NHI = 3, CT_CHAIN = 4, CT_NPEAKS = 5, CT_NSYM = 6, CT_KEYTOT = 7,
       CT_DEFR = 8 /* 5 slots */, CT_RAWTOT = 13, CT_PIECES = 14, CT_STASH = 15, CT_RECS = 16, CT_COUNT = 17 };

// ------------------------------------------------------------------------------------
// Workspaces and parameters of the synchronisation pass (k_sync / the fused front end, k_sync_exact, k_peak) for a
// capture of nsamples.  cap_full: candidate / piece storage for every sample (second attempt after an overflow).
// ------------------------------------------------------------------------------------
static int sync_params(ofdm_handle* h, uint64_t nsamples, bool cap_full, SyncParams* out) {
  RxState& rx = h->rx;
  const int N = h->N, CP = h->CP, T = SYNC_TILE;
  const uint64_t ntiles = (nsamples + T - 1) / T;
  const int tiles_per_seg = sync_tiles_per_seg(N, CP);  // (the tiles one k_sync workgroup walks: rx_sync.h)
  // (k_sync_exact's workgroups take candidate / piece storage in chunks: one chunk of slack per workgroup)
  const uint64_t egrid = std::min<uint64_t>(ntiles, 256ull * 8ull), egrid_small = std::min<uint64_t>(ntiles, 256ull * 16ull);
  // candidate storage: 1/16 of the samples plus one allocation chunk per workgroup; full-size buffers serve as the
  // second attempt when the first one overflows (a carrier, a periodic sequence: the metric sits above the threshold
  // everywhere -- legitimate input for which the reference simply finds no frame).
  const uint64_t cand_cap = (cap_full ? nsamples + nsamples / 8 : nsamples / 16) + (egrid + 16) * SYNC_CHUNK_C + egrid_small * 2048ull;
  // a piece is a maximal run of candidates: at most every other sample starts one
  const uint64_t piece_cap = (cap_full ? nsamples / 2 + 1 : nsamples / 128) + (egrid + egrid_small + 16) * SYNC_CHUNK_P;
  HIPCHK(h, rx.y.ensure(nsamples * sizeof(c32)));
  HIPCHK(h, rx.tile_B.ensure(ntiles * sizeof(double)));
  HIPCHK(h, rx.tile_np.ensure(ntiles * sizeof(uint32_t)));
  HIPCHK(h, rx.tile_pieces.ensure(piece_cap * sizeof(SyncPiece)));
  HIPCHK(h, rx.tile_first.ensure(ntiles * sizeof(uint64_t)));
  HIPCHK(h, rx.avg_in.ensure(ntiles * sizeof(double)));
  HIPCHK(h, rx.cand_u.ensure(cand_cap * sizeof(float)));
  HIPCHK(h, rx.cand_P.ensure(cand_cap * sizeof(c32)));
  HIPCHK(h, rx.counters.ensure(CT_COUNT * sizeof(uint64_t)));
  HIPCHK(h, rx.counts.ensure(ntiles * sizeof(uint32_t)));
  HIPCHK(h, rx.offsets.ensure(ntiles * sizeof(uint32_t)));
  HIPCHK(h, rx.recs.ensure(ntiles * sizeof(SyncRec)));
  float *d_metric = nullptr, *d_presel = nullptr;
  if (h->tap_mask & (1u << OFDM_TAP_RX_METRIC)) {
    HIPCHK(h, rx.metric.ensure(nsamples * sizeof(float)));
    d_metric = rx.metric.as<float>();
  }
  if (h->tap_mask & (1u << OFDM_TAP_RX_PRESEL)) {
    HIPCHK(h, rx.presel.ensure(nsamples * sizeof(float)));
    d_presel = rx.presel.as<float>();
  }
  uint64_t* ctr = rx.counters.as<uint64_t>();
  SyncParams sp;
  memset(&sp, 0, sizeof(sp));
  sp.N = N;
  sp.D = N / 2;
  sp.CP = CP;
  sp.HY = sync_hist_y(N);  // 2*D: the correlator's two lags (the fixed-point re-evaluation reads y from global memory)
  sp.HM = CP;
  sp.R = sync_ring_samples(sp.HY);
  sp.tiles_per_seg = tiles_per_seg;
  sp.nsamples = nsamples;
  sp.ntiles = ntiles;
  sp.tapcp = (float)(1.0 / (double)CP);
  sp.cand_thr = -fmaxf(h->cfg.peak_rise, h->cfg.peak_fall);
  sp.alpha = h->cfg.peak_alpha;
  sp.decay = (double)(1.0f - h->cfg.peak_alpha);
  sp.y = rx.y.as<c32>();
  sp.metric_tap = d_metric;
  sp.presel_tap = d_presel;
  sp.dpow = h->d_synctab.as<double>();
  sp.ipow = sp.dpow + (SYNC_TILE + 1);
  sp.wtab = reinterpret_cast<const float*>(sp.ipow + (SYNC_TILE + 1));
  sp.tile_B = rx.tile_B.as<double>();
  sp.tile_npieces = rx.tile_np.as<uint32_t>();
  sp.tile_first = rx.tile_first.as<uint64_t>();
  sp.pieces = rx.tile_pieces.as<SyncPiece>();
  sp.piece_cap = piece_cap;
  sp.piece_count = reinterpret_cast<unsigned long long*>(ctr + CT_PIECES);
  sp.cand_u = rx.cand_u.as<float>();
  sp.cand_P = rx.cand_P.as<c32>();
  sp.cand_cap = cand_cap;
  sp.cand_count = reinterpret_cast<unsigned long long*>(ctr + CT_CAND);
  sp.overflow = reinterpret_cast<unsigned int*>(ctr + CT_OVERFLOW);
  sp.recs = rx.recs.as<SyncRec>();
  sp.rec_count = reinterpret_cast<unsigned long long*>(ctr + CT_RECS);
  sp.exact_small = sync_exact_small(CP, N / 2);
  if (const char* es = getenv("OFDM_EXACT_SMALL")) sp.exact_small = std::max(0, std::min(atoi(es), (int)SYNC_TILE));  // tuning knob
#ifdef SYNC_DIAG
  if (const char* ab = getenv("OFDM_ABLATE")) sp.ablate = atoi(ab);  // diagnostic library only
#endif
  if (sp.HM > T) FAIL(h, OFDM_E_INVAL, "cyclic prefix longer than a k_sync tile");
  *out = sp;
  return OFDM_OK;
}

static uint64_t sync_nseg(const SyncParams& sp) { return (sp.ntiles + (uint64_t)sp.tiles_per_seg - 1) / (uint64_t)sp.tiles_per_seg; }

#ifdef SYNC_STAMPS
static DevBuf g_stamp_buf;
// cleared stamp slots for the nseg workgroups of one k_sync launch
static int stamps_prepare(ofdm_handle* h, SyncParams& sp, uint64_t nseg) {
  HIPCHK(h, g_stamp_buf.ensure(nseg * 16 * sizeof(unsigned long long)));
  HIPCHK(h, hipMemsetAsync(g_stamp_buf.p, 0, nseg * 16 * sizeof(unsigned long long), h->stream));
  sp.stamps = g_stamp_buf.as<unsigned long long>();
  return OFDM_OK;
}
static int sync_stamps_report(ofdm_handle* h, const unsigned long long* d_stamps, uint64_t nseg, int tiles_per_seg) {
  HIPCHK(h, hipStreamSynchronize(h->stream));
  std::vector<unsigned long long> st(nseg * 16);
  HIPCHK(h, hipMemcpy(st.data(), d_stamps, st.size() * 8, hipMemcpyDeviceToHost));
  double sum[16] = {0};
  for (uint64_t i = 0; i < nseg; i++)
    for (int k = 0; k < 16; k++) sum[k] += (double)st[i * 16 + k];
  const char* nm[16] = {"-", "y tile -> ring / filter", "B2 wait", "terms", "scan3 (B3)", "M + B4", "mavg + B5", "summary", "filter: block A", "filter: block B", "filter: taps + windows in", "-", "-", "-", "-", "-"};
  double tot = 0;
  for (int k = 0; k < 16; k++) tot += sum[k];
  fprintf(stderr, "[k_sync stamps] %llu workgroups, s_memtime ticks per workgroup-tile (wave 0):\n", (unsigned long long)nseg);
  for (int k = 0; k < 11; k++)
    fprintf(stderr, "  %-26s %10.0f  %5.1f%%\n", nm[k], sum[k] / (double)nseg / (double)(tiles_per_seg + 1), 100.0 * sum[k] / tot);
  return OFDM_OK;
}
#endif

// The fused front end (channel filter inside k_sync: the filtered stream is written once and never read back by the
// metric -- 5.3 KB per symbol less HBM traffic at C2) needs wave-sized transforms (F <= 512) and the fixed LDS layout
// with history + carry no longer than a tile.  It is bit-exact with the two-kernel path and selected with OFDM_FRONT=1;
// the default stays two kernels: every kernel of this pipeline is instruction-issue-bound (SQ_ACTIVE_INST_ANY ~ its
// duration), so the traffic saved buys no time, and the fused kernel's 3 workgroups per CU with 5.7 filter blocks
// per tile on 8 block slots issue less densely (C2: 7.9 ms against 3.3 + 2.7 ms; tools/experiments/README.md).
static bool front_fused(const ofdm_handle* h) {
  if (h->cfg.sync_mode != OFDM_SYNC_PN) return false;
  const char* e = getenv("OFDM_FRONT");
  if (!e || atoi(e) == 0) return false;
  return front_eligible(h->N, h->CP, (int)h->cfg.ntaps);
}

// k_sync over the whole filtered stream (the float32 pre-selection; the counters are cleared first)
static int launch_sync(ofdm_handle* h, SyncParams& sp) {
  RxState& rx = h->rx;
  const uint64_t nseg = sync_nseg(sp);
  HIPCHK(h, hipMemsetAsync(rx.counters.p, 0, CT_COUNT * sizeof(uint64_t), h->stream));
#ifdef SYNC_STAMPS
  if (int rs = stamps_prepare(h, sp, nseg)) return rs;
#endif
  const SyncLaunch sl = sync_launch_choice(sp.N, sp.CP);
  const size_t sync_shmem = sl.lds;
  if (sync_shmem > CU_LDS_BYTES) FAIL(h, OFDM_E_INVAL, "configuration needs more than 160 KiB of LDS in k_sync");
  {
    ProfScope span(h->prof, OFDM_K_SYNC, h->stream);
    int wg = sl.wg;
    if (const char* w = getenv("OFDM_SYNC_W")) wg = std::min(wg, atoi(w));  // tuning knob: a larger register budget
    bool fixed_layout = sl.fixed_layout;
    // tuning knob: the ring where the fixed layout would do.  Not where the tile's M values overlay its samples
    // (sync_mt_overlay: N <= 512) -- only the fixed layout has the tile at one place, the ring would read M for y.
    if (const char* e = getenv("OFDM_SYNC_STATIC")) fixed_layout = fixed_layout && (atoi(e) != 0 || sync_mt_overlay(sp.R));
    const void* fn = fixed_layout ? (wg >= 6   ? reinterpret_cast<const void*>(&k_sync<6, true>)
                                     : wg == 5 ? reinterpret_cast<const void*>(&k_sync<5, true>)
                                     : wg == 4 ? reinterpret_cast<const void*>(&k_sync<4, true>)
                                     : wg == 3 ? reinterpret_cast<const void*>(&k_sync<3, true>)
                                               : reinterpret_cast<const void*>(&k_sync<2, true>))
                                  : (wg >= 4   ? reinterpret_cast<const void*>(&k_sync<4, false>)
                                     : wg == 3 ? reinterpret_cast<const void*>(&k_sync<3, false>)
                                               : reinterpret_cast<const void*>(&k_sync<2, false>));
    HIPCHK(h, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sync_shmem));
    FilterParams nofp;
    memset(&nofp, 0, sizeof(nofp));
    void* args[] = {&sp, &nofp};
    HIPCHK(h, hipLaunchKernel(fn, dim3((unsigned)nseg), dim3(SYNC_THREADS), args, sync_shmem, h->stream));
  }
  HIPCHK(h, hipGetLastError());
  return OFDM_OK;
}

// a new "input consumed" event is about to be recorded: the previous one moves to the second slot
static void rx_note_input(ofdm_handle* h, const ofdm_c32* iq, uint64_t nsamples) {
  std::swap(h->ev_rx_in, h->ev_rx_in_old);
  h->rx_in_old_pending = h->rx_in_pending;
  h->rx_in_lo[1] = h->rx_in_lo[0];
  h->rx_in_hi[1] = h->rx_in_hi[0];
  h->rx_in_lo[0] = (uintptr_t)iq;
  h->rx_in_hi[0] = (uintptr_t)iq + nsamples * rx_ss(h);
}

// fused front end: channel filter + Schmidl-Cox pre-selection in one pass over x (k_sync<W, true, F>)
static int launch_front(ofdm_handle* h, FilterParams& fp, uint64_t nsamples) {
  const int F = h->filtF;
  SyncParams sp;
  int rcs = sync_params(h, nsamples, false, &sp);
  if (rcs != OFDM_OK) return rcs;
  HIPCHK(h, hipMemsetAsync(h->rx.counters.p, 0, CT_COUNT * sizeof(uint64_t), h->stream));
  const size_t shm = front_lds_layout(sp.R, sp.HM, fp.B, F).total;
  const uint64_t nseg = sync_nseg(sp);
  const void* fn = F == 64    ? reinterpret_cast<const void*>(&k_sync<3, true, 64>)
                   : F == 128 ? reinterpret_cast<const void*>(&k_sync<3, true, 128>)
                   : F == 256 ? reinterpret_cast<const void*>(&k_sync<3, true, 256>)
                              : reinterpret_cast<const void*>(&k_sync<3, true, 512>);
  HIPCHK(h, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm));
#ifdef SYNC_STAMPS
  if (int rs = stamps_prepare(h, sp, nseg)) return rs;
#endif
  void* args[] = {&sp, &fp};
  {
    ProfScope span(h->prof, OFDM_K_FRONT, h->stream);
    HIPCHK(h, hipLaunchKernel(fn, dim3((unsigned)nseg), dim3(SYNC_THREADS), args, shm, h->stream));
  }
  HIPCHK(h, hipGetLastError());
#ifdef SYNC_STAMPS
  if (int rs = sync_stamps_report(h, sp.stamps, nseg, sp.tiles_per_seg)) return rs;
#endif
  h->rx.front_done = true;
  return OFDM_OK;
}

// channel filter: x -> y (streaming)
template <typename XT>
static int launch_filter_t(ofdm_handle* h, FilterParams& fp, uint64_t nsamples) {
  const int F = h->filtF;
  const uint64_t bpr = 256 / (F / 8);
  const uint64_t nblk = (nsamples + (uint64_t)fp.goff + (uint64_t)fp.B - 1) / (uint64_t)fp.B;
  fp.nrounds = (nblk + bpr - 1) / bpr;
  const size_t fsh = (size_t)256 * 9 * sizeof(c32);  // 256/(F/8) transforms x (F + F/8) points
  const unsigned fgrid = (unsigned)std::min<uint64_t>(fp.nrounds, 256ull * 8ull * 4ull);
  {
    ProfScope span(h->prof, OFDM_K_FILTER, h->stream);
    switch (F) {
      case 64: hipLaunchKernelGGL(HIP_KERNEL_NAME(k_chan_filter<64, XT>), dim3(fgrid), dim3(256), fsh, h->stream, fp); break;
      case 128: hipLaunchKernelGGL(HIP_KERNEL_NAME(k_chan_filter<128, XT>), dim3(fgrid), dim3(256), fsh, h->stream, fp); break;
      case 256: hipLaunchKernelGGL(HIP_KERNEL_NAME(k_chan_filter<256, XT>), dim3(fgrid), dim3(256), fsh, h->stream, fp); break;
      case 512: hipLaunchKernelGGL(HIP_KERNEL_NAME(k_chan_filter<512, XT>), dim3(fgrid), dim3(256), fsh, h->stream, fp); break;
      case 1024: hipLaunchKernelGGL(HIP_KERNEL_NAME(k_chan_filter<1024, XT>), dim3(fgrid), dim3(256), fsh, h->stream, fp); break;
      default: FAIL(h, OFDM_E_INVAL, "unsupported channel filter transform length");
    }
  }
  HIPCHK(h, hipGetLastError());
  return OFDM_OK;
}

static int launch_filter(ofdm_handle* h, FilterParams& fp, uint64_t nsamples) {
  return h->rx_fmt == OFDM_IQ_SC16 ? launch_filter_t<sc16>(h, fp, nsamples) : launch_filter_t<c32>(h, fp, nsamples);
}

// ------------------------------------------------------------------------------------
// The receiver's input stage: wait for the transmit batch that fills the buffer (if one is queued), stage a host
// buffer, run the channel filter x -> y.  With SYNC "pn" and no fused sensing nothing reads the input afterwards:
// ev_rx_in is recorded right here and the NEXT transmit batch (queued on the transmit stream while this call's
// kernels and host round trips are still under way) may overwrite it.
// ------------------------------------------------------------------------------------
static int rx_submit_impl(ofdm_handle* h, const ofdm_c32* iq, uint64_t nsamples, const c32** d_x_out) {
  RxState& rx = h->rx;
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  if (h->tx_pending && h->txs != h->stream) HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_tx_done, 0));
  h->tx_pending = false;
  // (d_x: the input on the device in the handle's receive format -- ofdm_sc16 samples when that says so)
  const c32* d_x = reinterpret_cast<const c32*>(iq);
  if (h->rx_fmt == OFDM_IQ_SC16) {
    if ((uintptr_t)iq & 3u) FAIL(h, OFDM_E_INVAL, "ofdm_sc16 buffers must be 4-byte aligned");
    if (front_fused(h)) FAIL(h, OFDM_E_INVAL, "the fused front end (OFDM_FRONT=1) takes float32 samples only");
  }
  if (!h->dev_ptrs) {
    HIPCHK(h, rx.x_stage.ensure(nsamples * rx_ss(h)));
    HIPCHK(h, hipMemcpyAsync(rx.x_stage.p, iq, nsamples * rx_ss(h), hipMemcpyHostToDevice, h->stream));
    d_x = rx.x_stage.as<c32>();
  }
  *d_x_out = d_x;
  rx.in_event_at_end = true;
  if (h->cfg.sync_mode != OFDM_SYNC_PN) return OFDM_OK;  // SYNC "fixed": chan_filt is the input itself, read to the end
  HIPCHK(h, rx.y.ensure(nsamples * sizeof(c32)));
  FilterParams fp;
  memset(&fp, 0, sizeof(fp));
  fp.B = h->filtF - (int)h->cfg.ntaps + 1;
  fp.ntm1 = (int)h->cfg.ntaps - 1;
  fp.goff = (int)(rx.origin % (uint64_t)fp.B);
  fp.nsamples = nsamples;
  fp.x = d_x;
  fp.y = rx.y.as<c32>();
  fp.Hf = h->d_Hf.as<c32>();
  fp.twF = h->d_twF.as<c32>();
  fp.xscale = h->rx_scale;
  rx.front_done = false;
  if (int rc = front_fused(h) ? launch_front(h, fp, nsamples) : launch_filter(h, fp, nsamples)) return rc;
  if (!h->sense.rx_on) {
    rx_note_input(h, iq, nsamples);
    HIPCHK(h, hipEventRecord(h->ev_rx_in, h->stream));
    h->rx_in_pending = true;
    rx.in_event_at_end = false;
  }
  return OFDM_OK;
}

extern "C" int ofdm_rx_submit(ofdm_handle* h, const ofdm_c32* iq, uint64_t nsamples) {
  if (!h) return OFDM_E_INVAL;
  if (nsamples && !iq) FAIL(h, OFDM_E_INVAL, "null argument");
  RxState& rx = h->rx;
  rx.sub_valid = false;
  if (nsamples == 0) return OFDM_OK;
  const c32* d_x = nullptr;
  int rc = rx_submit_impl(h, iq, nsamples, &d_x);
  if (rc != OFDM_OK) return rc;
  rx.sub_valid = true;
  rx.sub_iq = iq;
  rx.sub_n = nsamples;
  rx.sub_dx = d_x;
  // SYNC "fixed" and fused sensing read the input to the end of ofdm_rx: no event exists yet that a transmit batch
  // could wait on, so until that call a batch into this buffer is refused (tx_enqueue)
  rx.sub_hold = rx.in_event_at_end;
  return OFDM_OK;
}

// ------------------------------------------------------------------------------------
// One ofdm_rx call: the caller's arguments and what its stages hand to each other.
// ------------------------------------------------------------------------------------
struct RxCall {
  ofdm_handle* h;
  const ofdm_c32* iq;  // the arguments of ofdm_rx, in its order
  uint64_t nsamples;
  uint8_t* payload_out;
  uint64_t payload_cap;
  uint64_t* payload_off;
  uint32_t* payload_len;
  uint8_t* crc_ok;
  int max_pkts;
  int* npkt;
  ofdm_stats* stats;
  const c32* d_x = nullptr;  // the input on the device
  bool fixed = false;        // SYNC "fixed"
  bool done = false;         // a stage found nothing left to do (no flag, no frame)
  // Count path.  dyn: the frame count (flags the sampler accepts) and the packet count stay on the device (DynFrames),
  // dependent launches are sized by their upper bound npeaks and leave early, and the call has two host round trips
  // (flag count, final) instead of four.  Probes and the chunked-stream splice need the counts on the host as they go.
  bool dyn = false;
  uint64_t npeaks = 0, nforced = 0;  // timing flags; those of them a chunked stream's history supplied
  // the counter block as rx_read_counts decoded it last (dyn: n_lo = 0, nframes = npeaks are bounds until the final one)
  uint64_t n_lo = 0, nframes = 0, nsym = 0, npk = 0, nbytes = 0, rawtot = 0;
  uint64_t npk_ub = 0;  // packets the outputs are sized for
  DynFrames dynf;
  DemodParams dq;  // (zero from the call's start; rx_frames puts the NCO's reference line in, make_demod_params the rest)
  DeframeParams fq;
  CsiRows csi_fr = {nullptr, nullptr, nullptr, nullptr};
  uint8_t* d_pay = nullptr;  // where the deframer writes: the caller's device buffer, or the staging buffer
};

static uint64_t* rx_ctr(ofdm_handle* h) { return h->rx.counters.as<uint64_t>(); }

// The one read-back and decoding of the counter block (slots no kernel has written yet read zero): frames the sampler
// accepted, their symbols, packets and payload bytes the deframer counted.  A host round trip.
static int rx_read_counts(RxCall& c) {
  ofdm_handle* h = c.h;
  RxState& rx = h->rx;
  uint64_t hc[CT_COUNT];
  HIPCHK(h, hipMemcpyAsync(hc, rx.counters.p, sizeof(hc), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  c.n_lo = hc[CT_NLO] & 0xFFFFFFFFull;
  c.nframes = c.npeaks - c.n_lo - (hc[CT_NHI] & 0xFFFFFFFFull);
  c.nsym = hc[CT_NSYM];
  c.npk = hc[CT_KEYTOT] >> 40;
  c.nbytes = hc[CT_KEYTOT] & ((1ull << 40) - 1);
  c.rawtot = hc[CT_RAWTOT];
  rx.nframes = c.nframes;
  rx.j0 = c.n_lo;
  rx.nsym_total = c.nsym;
  if (c.stats) {
    c.stats->frames = c.nframes;
    c.stats->symbols = c.nsym;
    c.stats->headers_ok = hc[CT_DEFR + 0];
    c.stats->chained_frames = hc[CT_DEFR + 3];
    c.stats->overflow = hc[CT_OVERFLOW] & 0xFFFFFFFFull;
  }
  return OFDM_OK;
}

// the one capacity check, on decoded counts: *npkt tells the caller how many packets there are
static int rx_check_capacity(RxCall& c) {
  if (c.npk <= (uint64_t)c.max_pkts && c.nbytes <= c.payload_cap) return OFDM_OK;
  *c.npkt = (int)std::min<uint64_t>(c.npk, 0x7FFFFFFF);
  FAIL(c.h, OFDM_E_CAPACITY, "payload_out / max_pkts too small for the packets found");
}

// ------------------------------------------------------------------------------------
// SYNC = "pn" (ofdm_receiver.py~:97-101): channel filter, Schmidl-Cox metric, peak detector.  Leaves the timing
// flags and P at the flags in rx.peaks / rx.peak_P.
// ------------------------------------------------------------------------------------
static hipError_t launch_sync_exact(const void* fn, unsigned grid, size_t shmem, SyncParams sp, hipStream_t s) {
  void* args[] = {&sp};
  return hipLaunchKernel(fn, dim3(grid), dim3(SYNC_THREADS), args, shmem, s);
}

// the tiles the pre-selection fired in: fixed-point metric, candidate pieces, detector summary
static int rx_sync_exact(RxCall& c, SyncParams& sp, bool cap_full) {
  ofdm_handle* h = c.h;
  if (cap_full) {
    // Second attempt after a candidate / piece overflow: storage for every sample.  The pre-selection's results (the
    // records, the summaries of the tiles without a range) stand; only k_sync_exact and the detector run again.
    int rcs = sync_params(h, c.nsamples, true, &sp);
    if (rcs != OFDM_OK) return rcs;
    uint64_t* ctr = rx_ctr(h);
    HIPCHK(h, hipMemsetAsync(ctr + CT_CAND, 0, 2 * sizeof(uint64_t), h->stream));     // CT_CAND, CT_OVERFLOW
    HIPCHK(h, hipMemsetAsync(ctr + CT_NPEAKS, 0, sizeof(uint64_t), h->stream));
    HIPCHK(h, hipMemsetAsync(ctr + CT_PIECES, 0, 2 * sizeof(uint64_t), h->stream));   // CT_PIECES, CT_STASH
  }
  const unsigned egrid = (unsigned)std::min<uint64_t>(sp.ntiles, 256ull * 8ull);
  const unsigned egrid_small = (unsigned)std::min<uint64_t>(sp.ntiles, 256ull * 16ull);
  {
    ProfScope span(h->prof, OFDM_K_EXACT, h->stream);
    const size_t esh = exact_lds_layout(sp.CP, SYNC_TILE).total, esh_small = exact_lds_layout(sp.CP, sp.exact_small).total;
    // (deltas kept in registers between the two passes: pays for long symbols only)
    const void* fbig = sync_exact_keep(sp.N) ? reinterpret_cast<const void*>(&k_sync_exact<SYNC_THREADS, true>)
                                    : reinterpret_cast<const void*>(&k_sync_exact<SYNC_THREADS, false>);
    if (esh > 64 * 1024) HIPCHK(h, hipFuncSetAttribute(fbig, hipFuncAttributeMaxDynamicSharedMemorySize, (int)esh));
    if (sp.exact_small > 0)
      hipLaunchKernelGGL(HIP_KERNEL_NAME(k_sync_exact<WAVE, false>), dim3(egrid_small), dim3(WAVE), esh_small, h->stream, sp);
    HIPCHK(h, launch_sync_exact(fbig, egrid, esh, sp, h->stream));
    if (sp.metric_tap) {
      // the metric tap: the normative metric of EVERY sample, in a pass of its own that writes nothing else -- the
      // detector works from exactly what it works from without the tap
      SyncParams tp = sp;
      tp.tap_only = 1;
      HIPCHK(h, launch_sync_exact(fbig, egrid, esh, tp, h->stream));
    }
  }
  HIPCHK(h, hipGetLastError());
#ifdef SYNC_STAMPS
  if (!h->rx.front_done)
    if (int rs = sync_stamps_report(h, sp.stamps, sync_nseg(sp), sp.tiles_per_seg)) return rs;
#endif
  return OFDM_OK;
}

// fused spectrum sensing (BASELINE config 5): same IQ buffer, second stream.  It starts when k_sync has drained (both
// are VALU/LDS-bound: run side by side they only slow each other) and runs beside the peak pass and the demodulator;
// joined at the end of ofdm_rx
static int rx_sense_fork(RxCall& c) {
  ofdm_handle* h = c.h;
  SenseState& ss = h->sense;
  HIPCHK(h, hipEventRecord(ss.ev_in, h->stream));
  HIPCHK(h, hipStreamWaitEvent(ss.side, ss.ev_in, 0));
  int src = sense_enqueue(h, &ss.rx_cfg, c.d_x, c.nsamples, ss.side);
  if (src != OFDM_OK) return src;
  HIPCHK(h, hipEventRecord(ss.ev_out, ss.side));
  return OFDM_OK;
}

// (the stash and, with OFDM_TAP_RX_RUN_AVG, the run rows are sized by the caller)
static PeakParams make_peak_params(ofdm_handle* h, const SyncParams& sp) {
  RxState& rx = h->rx;
  PeakParams pp;
  memset(&pp, 0, sizeof(pp));
  pp.ntiles = sp.ntiles;
  pp.nsamples = sp.nsamples;
  pp.rise = h->cfg.peak_rise;
  pp.fall = h->cfg.peak_fall;
  pp.alpha = h->cfg.peak_alpha;
  pp.dpow = sp.dpow;
  pp.tile_npieces = rx.tile_np.as<uint32_t>();
  pp.tile_first = rx.tile_first.as<uint64_t>();
  pp.pieces = rx.tile_pieces.as<SyncPiece>();
  pp.avg_in = rx.avg_in.as<double>();
  pp.cand_u = rx.cand_u.as<float>();
  pp.cand_P = rx.cand_P.as<c32>();
  pp.counts = rx.counts.as<uint32_t>();
  pp.offsets = rx.offsets.as<uint32_t>();
  pp.stash_peaks = rx.stash_peaks.as<uint64_t>();
  pp.stash_P = rx.stash_P.as<c32>();
  pp.stash_overflow = reinterpret_cast<unsigned int*>(rx_ctr(h) + CT_STASH);
  if (h->tap_mask & (1u << OFDM_TAP_RX_RUN_AVG)) pp.run_rows = rx.run_rows.as<double>();
  return pp;
}

// The peak detector over the candidates of this attempt; the flag count is the call's first host round trip.
// *overflow: non-zero when the candidate / piece storage did not suffice.  c.done: no flag and no carried history.
static int rx_flags_pn(RxCall& c, const SyncParams& sp, uint64_t* overflow) {
  ofdm_handle* h = c.h;
  RxState& rx = h->rx;
  const uint64_t ntiles = sp.ntiles;
  const unsigned grid = (unsigned)((ntiles + 255) / 256);
  uint64_t* ctr = rx_ctr(h);
  // OFDM_TAP_RX_RUN_AVG: one row per piece slot; slots no interval starts in stay NaN (compacted when read)
  const uint64_t run_cap = (h->tap_mask & (1u << OFDM_TAP_RX_RUN_AVG)) ? sp.piece_cap : 0;
  HIPCHK(h, rx.stash_peaks.ensure(ntiles * PEAK_STASH * sizeof(uint64_t)));
  HIPCHK(h, rx.stash_P.ensure(ntiles * PEAK_STASH * sizeof(c32)));
  if (run_cap) HIPCHK(h, rx.run_rows.ensure(run_cap * 2 * sizeof(double)));
  PeakParams pp = make_peak_params(h, sp);
  hipLaunchKernelGGL(k_avg_carry, dim3(grid), dim3(256), 0, h->stream, rx.tile_B.as<double>(), ntiles, c.nsamples, sp.dpow,
                     rx.avg_in.as<double>());
  if (run_cap) HIPCHK(h, hipMemsetAsync(rx.run_rows.p, 0xFF, run_cap * 2 * sizeof(double), h->stream));  // NaN
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_peak<false>), dim3(grid), dim3(256), 0, h->stream, pp);
  HIPCHK(h, hipGetLastError());
  int rc = dev_excl_scan<uint32_t>(h, rx.counts.as<uint32_t>(), ntiles, rx.offsets.as<uint32_t>(),
                                   reinterpret_cast<uint32_t*>(ctr + CT_NPEAKS));
  if (rc) return rc;
  uint64_t hc[CT_COUNT];
  HIPCHK(h, hipMemcpyAsync(hc, ctr, sizeof(hc), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if ((*overflow = hc[CT_OVERFLOW] & 0xFFFFFFFFull)) return OFDM_OK;
  rx.run_slots = std::min<uint64_t>(hc[CT_PIECES], run_cap);
  const uint64_t npeaks = hc[CT_NPEAKS] & 0xFFFFFFFFull;
  c.npeaks = rx.npeaks = npeaks;
  if (c.stats) c.stats->peaks = npeaks;
  if (npeaks == 0 && !(rx.nco_ref_on && !rx.hist_flags.empty())) {
    c.done = true;
    return OFDM_OK;
  }
  HIPCHK(h, rx.peaks.ensure(std::max<uint64_t>(npeaks, 1) * sizeof(uint64_t)));
  HIPCHK(h, rx.peak_P.ensure(std::max<uint64_t>(npeaks, 1) * sizeof(c32)));
  pp.peaks = rx.peaks.as<uint64_t>();
  pp.peak_P = rx.peak_P.as<c32>();
  if (npeaks > 0) {
    if (hc[CT_STASH] & 0xFFFFFFFFull)  // some tile raised more flags than the count pass stashes: run the machine again
      hipLaunchKernelGGL(HIP_KERNEL_NAME(k_peak<true>), dim3(grid), dim3(256), 0, h->stream, pp);
    else
      hipLaunchKernelGGL(k_peak_compact, dim3(grid), dim3(256), 0, h->stream, pp);
    HIPCHK(h, hipGetLastError());
  }
  return OFDM_OK;
}

// SYNC = "fixed" (ofdm_receiver.py~:108-119, "for testing only"): ofdm_sync_fixed raises a flag on the last sample of
// the first symbol of every fixed_nsymbols symbols, i.e. at L-1 + k*nsymbols*L counted from the capture's first sample
__global__ void __launch_bounds__(256) k_fixed_flags(uint64_t npeaks, uint64_t first, uint64_t period, uint64_t* __restrict__ peaks,
                                                      c32* __restrict__ peak_P) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= npeaks) return;
  peaks[k] = first + k * period;
  peak_P[k] = mk(0.f, 0.f);
}

// the flag count of SYNC "fixed" (known without the device) and cleared counters; c.done: the capture holds no symbol
static int rx_fixed_count(RxCall& c) {
  ofdm_handle* h = c.h;
  RxState& rx = h->rx;
  const uint64_t L = (uint64_t)h->L;
  c.npeaks = rx.npeaks = c.nsamples >= L ? (c.nsamples - L) / ((uint64_t)h->cfg.fixed_nsymbols * L) + 1 : 0;
  if (c.stats) c.stats->peaks = c.npeaks;
  HIPCHK(h, rx.counters.ensure(CT_COUNT * sizeof(uint64_t)));
  HIPCHK(h, hipMemsetAsync(rx.counters.p, 0, CT_COUNT * sizeof(uint64_t), h->stream));
  if (c.npeaks == 0) {
    HIPCHK(h, hipStreamSynchronize(h->stream));
    c.done = true;
  }
  return OFDM_OK;
}

static int rx_flags_fixed(RxCall& c) {
  ofdm_handle* h = c.h;
  RxState& rx = h->rx;
  HIPCHK(h, rx.peaks.ensure(c.npeaks * sizeof(uint64_t)));
  HIPCHK(h, rx.peak_P.ensure(c.npeaks * sizeof(c32)));
  hipLaunchKernelGGL(k_fixed_flags, dim3((unsigned)((c.npeaks + 255) / 256)), dim3(256), 0, h->stream, c.npeaks, (uint64_t)h->L - 1,
                     (uint64_t)h->cfg.fixed_nsymbols * (uint64_t)h->L, rx.peaks.as<uint64_t>(), rx.peak_P.as<c32>());
  HIPCHK(h, hipGetLastError());
  return OFDM_OK;
}

// Chunked stream: flags up to trust_after are the ones earlier calls settled, not what this call detects in its
// unsettled overlap.  Splice on the host (a few hundred flags; this path is not timed).  c.done: no flag either way.
static int rx_splice(RxCall& c) {
  ofdm_handle* h = c.h;
  RxState& rx = h->rx;
  if (!rx.nco_ref_on) return OFDM_OK;
  const uint64_t npeaks = c.npeaks;
  std::vector<uint64_t> hp(npeaks);
  if (npeaks) HIPCHK(h, hipMemcpyAsync(hp.data(), rx.peaks.p, npeaks * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  uint64_t kdrop = 0;
  while (kdrop < npeaks && (int64_t)hp[kdrop] <= rx.nco_trust_after) kdrop++;
  const uint64_t m = rx.hist_flags.size(), np2 = m + npeaks - kdrop;
  c.done = np2 == 0;
  if (!c.done) {
    HIPCHK(h, rx.peaks2.ensure(np2 * sizeof(uint64_t)));
    HIPCHK(h, rx.peak_P2.ensure(np2 * sizeof(c32)));
    HIPCHK(h, rx.fstep.ensure(std::max<uint64_t>(m, 1) * sizeof(double)));
    if (m) {
      HIPCHK(h, hipMemcpyAsync(rx.peaks2.p, rx.hist_flags.data(), m * sizeof(uint64_t), hipMemcpyHostToDevice, h->stream));
      HIPCHK(h, hipMemsetAsync(rx.peak_P2.p, 0, m * sizeof(c32), h->stream));
      HIPCHK(h, hipMemcpyAsync(rx.fstep.p, rx.hist_steps.data(), m * sizeof(double), hipMemcpyHostToDevice, h->stream));
    }
    if (npeaks > kdrop) {
      HIPCHK(h, hipMemcpyAsync(rx.peaks2.as<uint64_t>() + m, rx.peaks.as<uint64_t>() + kdrop, (npeaks - kdrop) * sizeof(uint64_t),
                               hipMemcpyDeviceToDevice, h->stream));
      HIPCHK(h, hipMemcpyAsync(rx.peak_P2.as<c32>() + m, rx.peak_P.as<c32>() + kdrop, (npeaks - kdrop) * sizeof(c32),
                               hipMemcpyDeviceToDevice, h->stream));
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));  // the host vectors may change after this call
    std::swap(rx.peaks, rx.peaks2);
    std::swap(rx.peak_P, rx.peak_P2);
    c.nforced = m;
  }
  c.npeaks = rx.npeaks = np2;
  if (c.stats) c.stats->peaks = np2;
  return OFDM_OK;
}

static FramesParams make_frames_params(const RxCall& c) {
  ofdm_handle* h = c.h;
  RxState& rx = h->rx;
  uint64_t* ctr = rx_ctr(h);
  FramesParams fp;
  memset(&fp, 0, sizeof(fp));
  fp.npeaks = c.npeaks;
  fp.nsamples = c.nsamples;
  fp.N = h->N;
  fp.L = h->L;
  fp.timeout = h->cfg.sampler_timeout;
  fp.sens = (float)(-2.0 / (double)h->N);  // nco_sensitivity, ofdm_receiver.py~:98
  fp.peaks = rx.peaks.as<uint64_t>();
  fp.peak_P = rx.peak_P.as<c32>();
  fp.angle = rx.angle.as<float>();
  fp.step = rx.step.as<double>();
  fp.inc = rx.inc.as<uint64_t>();
  fp.K = rx.K.as<uint32_t>();
  fp.nsym = rx.nsym.as<uint64_t>();
  fp.n_lo = reinterpret_cast<unsigned int*>(ctr + CT_NLO);
  fp.n_hi = reinterpret_cast<unsigned int*>(ctr + CT_NHI);
  fp.nforced = c.nforced;
  fp.forced_step = rx.fstep.as<double>();
  fp.fixed_on = c.fixed ? 1 : 0;
  fp.fixed_angle = h->cfg.fixed_freq_offset;
  return fp;
}

// sample & hold, NCO, sampler: per flag the frequency step, the NCO phase, the symbols its frame takes
static int rx_frames(RxCall& c) {
  ofdm_handle* h = c.h;
  RxState& rx = h->rx;
  const uint64_t npeaks = c.npeaks;
  const unsigned grid = (unsigned)((npeaks + 255) / 256);
  HIPCHK(h, rx.angle.ensure(npeaks * sizeof(float)));
  HIPCHK(h, rx.step.ensure(npeaks * sizeof(double)));
  HIPCHK(h, rx.inc.ensure(npeaks * sizeof(uint64_t)));
  HIPCHK(h, rx.inc_acc.ensure(npeaks * sizeof(uint64_t)));
  HIPCHK(h, rx.Phi_u.ensure(npeaks * sizeof(uint64_t)));
  HIPCHK(h, rx.Phi.ensure(npeaks * sizeof(double)));
  HIPCHK(h, rx.K.ensure(npeaks * sizeof(uint32_t)));
  HIPCHK(h, rx.nsym.ensure(npeaks * sizeof(uint64_t)));
  HIPCHK(h, rx.sym_base.ensure(npeaks * sizeof(uint64_t)));
  const FramesParams fp = make_frames_params(c);
  // the NCO line in force before the first flag: none (phase 0), the one a chunked stream carries in, or -- SYNC
  // "fixed", whose frequency input is constant from the first sample on -- the line through (sample 0, phase 0)
  const uint64_t ref_u = rx.nco_ref_on ? rx.nco_ref_u : 0ull;
  c.dq.ref_on = (rx.nco_ref_on || (c.fixed && h->cfg.fixed_freq_offset != 0.0f)) ? 1 : 0;
  c.dq.ref_peak = rx.nco_ref_on ? rx.nco_ref_peak : 0;
  c.dq.ref_phi = nco_radians(ref_u);
  c.dq.ref_step = rx.nco_ref_on ? rx.nco_ref_step : (double)(fp.sens * h->cfg.fixed_freq_offset);
  hipLaunchKernelGGL(k_frames, dim3(grid), dim3(256), 0, h->stream, fp);
  HIPCHK(h, hipGetLastError());
  int rc = dev_excl_scan<uint64_t>(h, rx.inc.as<uint64_t>(), npeaks, rx.inc_acc.as<uint64_t>(), (uint64_t*)nullptr);
  if (rc) return rc;
  hipLaunchKernelGGL(k_nco_phase, dim3(grid), dim3(256), 0, h->stream, rx.peaks.as<uint64_t>(), rx.inc_acc.as<uint64_t>(), npeaks,
                     c.dq.ref_on, c.dq.ref_peak, ref_u, c.dq.ref_step, rx.Phi_u.as<uint64_t>(), rx.Phi.as<double>());
  HIPCHK(h, hipGetLastError());
  return dev_excl_scan<uint64_t>(h, rx.nsym.as<uint64_t>(), npeaks, rx.sym_base.as<uint64_t>(), rx_ctr(h) + CT_NSYM);
}

// Timing: flags -> chunked-stream splice -> frames / NCO / sampler, the last three under one detector span.  SYNC "pn"
// runs k_sync_exact and the detector a second time, with room for every sample, when the sparse candidate storage
// overflows (a carrier, a periodic sequence: legitimate input in which the reference simply finds no frame).
static int rx_timing(RxCall& c) {
  ofdm_handle* h = c.h;
  SyncParams sp;
  uint64_t overflow = 0;
  int rc = c.fixed ? rx_fixed_count(c) : sync_params(h, c.nsamples, false, &sp);
  if (rc || c.done) return rc;
  // (a fused front end has queued the pre-selection already: the input stage, rx_submit_impl)
  if (!c.fixed && !h->rx.front_done && (rc = launch_sync(h, sp))) return rc;
  for (int attempt = 0; attempt < 2; attempt++) {
    if (!c.fixed && (rc = rx_sync_exact(c, sp, attempt == 1))) return rc;
    if (!c.fixed && attempt == 0 && h->sense.rx_on && (rc = rx_sense_fork(c))) return rc;
    ProfScope span(h->prof, OFDM_K_PEAK, h->stream);
    if ((rc = c.fixed ? rx_flags_fixed(c) : rx_flags_pn(c, sp, &overflow))) return rc;
    if (overflow) continue;
    if (c.done) {  // no flag: the span ends before the stream drains, so that the call's one collect() sees it complete
      span.end();
      HIPCHK(h, hipStreamSynchronize(h->stream));
      return OFDM_OK;
    }
    if ((rc = rx_splice(c)) || c.done) return rc;
    return rx_frames(c);
  }
  if (c.stats) c.stats->overflow = overflow;
  FAIL(h, OFDM_E_OVERFLOW, "candidate / piece buffer exhausted");
}

// four row arrays carved from one buffer, structure of arrays: eq | pre | err | ref, [rows][stride] each
static size_t csi_bytes(uint64_t rows, uint64_t stride) { return rows * stride * (sizeof(c32) + 3 * sizeof(float)); }
static CsiRows csi_carve(const DevBuf& b, uint64_t rows, uint64_t stride) {
  const uint64_t cell = rows * stride;
  CsiRows r;
  r.eq = b.as<c32>();
  r.pre = reinterpret_cast<float*>(r.eq + cell);
  r.err = r.pre + cell;
  r.ref = r.err + cell;
  return r;
}

// parameters of the optimistic demodulator pass; link quality and channel state bring their per-frame workspaces
static int make_demod_params(RxCall& c) {
  ofdm_handle* h = c.h;
  RxState& rx = h->rx;
  DemodParams& dq = c.dq;
  dq.dyn = c.dynf;
  dq.N = h->N;
  dq.CP = h->CP;
  dq.L = h->L;
  dq.occ = h->occ;
  dq.zl = h->zl;
  dq.nmap = h->nmap;
  dq.nbits = h->nbits;
  dq.arity = (int)h->cfg.arity;
  dq.shift = (int)h->cfg.max_fft_shift_len;
  dq.phase_gain = h->cfg.phase_gain;
  dq.freq_gain = h->cfg.freq_gain;
  dq.eq_gain = h->cfg.eq_gain;
  dq.sign_kind = h->sign_kind;
  memcpy(dq.sign_idx, h->sign_idx, 4);
  dq.sign_eps = h->sign_eps;
  dq.sign_bound = h->sign_bound;
  dq.nsamples = c.nsamples;
  dq.j0 = (uint32_t)c.n_lo;
  dq.nframes = (uint32_t)c.nframes;
  dq.npeaks = (uint32_t)c.npeaks;
  dq.y = rx.y_ptr;
  dq.peaks = rx.peaks.as<uint64_t>();
  dq.Phi = rx.Phi.as<double>();
  dq.step = rx.step.as<double>();
  dq.K = rx.K.as<uint32_t>();
  dq.sym_base = rx.sym_base.as<uint64_t>();
  dq.tw = h->d_tw.as<c32>();
  dq.ks = h->d_ks.as<c32>();
  dq.kd = h->d_kd.as<float>();
  dq.smap = h->d_smap.as<int16_t>();
  dq.constellation = h->d_const.as<c32>();
  dq.grid = h->has_grid ? h->d_grid.as<SlicerGrid>() : nullptr;
  dq.invalid = rx.invalid.as<uint8_t>();
  dq.res = rx.res.as<FrameResult>();
  dq.raw = rx.raw.as<uint8_t>();
  if (rx.quality_on) {
    HIPCHK(h, rx.qual_frame.ensure(c.nframes * sizeof(FrameQuality)));
    dq.qual = rx.qual_frame.as<FrameQuality>();
  }
  if (rx.csi_on || rx.soft_on) {  // (soft-decision receive weighs the carriers by the frame's own equaliser row)
    rx.csi_stride = (h->occ + 3) & ~3;
    HIPCHK(h, rx.csi_frame.ensure(csi_bytes(c.nframes, (uint64_t)rx.csi_stride)));
    c.csi_fr = csi_carve(rx.csi_frame, c.nframes, (uint64_t)rx.csi_stride);  // per-frame rows
    dq.csi_eq = c.csi_fr.eq;
    dq.csi_pre = c.csi_fr.pre;
    dq.csi_err = c.csi_fr.err;
    dq.csi_ref = c.csi_fr.ref;
    dq.csi_stride = rx.csi_stride;
  }
  return OFDM_OK;
}

#ifdef SYNC_STAMPS
static int demod_stamps_report(ofdm_handle* h) {
  HIPCHK(h, hipStreamSynchronize(h->stream));
  unsigned long long st[16];
  HIPCHK(h, hipMemcpyFromSymbol(st, HIP_SYMBOL(g_demod_stamps), sizeof(st)));
  const unsigned long long zero[16] = {0};
  HIPCHK(h, hipMemcpyToSymbol(HIP_SYMBOL(g_demod_stamps), zero, sizeof(zero)));
  const char* nm[8] = {"frame prologue", "derotation (+ sample wait)", "transform", "prefetch issue + spectrum to LDS", "frame acquisition",
                       "demapper", "loop bookkeeping", "PLL, header, bytes"};
  double tot = 0;
  for (int k = 0; k < 8; k++) tot += (double)st[k];
  fprintf(stderr, "[k_rx_demod stamps] s_memtime ticks summed over the workgroups' thread 0 (%.3e in all):\n", tot);
  for (int k = 0; k < 8; k++) fprintf(stderr, "  %-34s %12.4e  %5.1f%%\n", nm[k], (double)st[k], 100.0 * (double)st[k] / (tot > 0 ? tot : 1));
  return OFDM_OK;
}
#endif

// demodulate every frame (dyn: every flag; the frames the sampler refused leave early)
static int rx_demodulate(RxCall& c) {
  ofdm_handle* h = c.h;
  RxState& rx = h->rx;
  const uint64_t nframes = c.nframes;
  HIPCHK(h, rx.res.ensure(nframes * sizeof(FrameResult)));
  HIPCHK(h, rx.raw.ensure(nframes * (uint64_t)RAW_SLOT));
  HIPCHK(h, rx.invalid.ensure(nframes));
  HIPCHK(h, rx.chain_list.ensure(4096 * sizeof(uint32_t)));
  HIPCHK(h, rx.key.ensure(nframes * sizeof(uint64_t)));
  HIPCHK(h, rx.pos.ensure(nframes * sizeof(uint64_t)));
  HIPCHK(h, hipMemsetAsync(rx.invalid.p, 0, nframes, h->stream));
  int rc = make_demod_params(c);
  if (rc) return rc;
  ProfScope span(h->prof, OFDM_K_DEMOD, h->stream);
  rc = run_demod(h, c.dq);
#ifdef SYNC_STAMPS
  if (rc == OFDM_OK) rc = demod_stamps_report(h);
#endif
  return rc;
}

// chains: frames swallowed by the packet of an earlier flag are marked invalid (a chunked stream brings the verdicts
// of its settled frames: frame f is flag j0 + f of the spliced list)
static int rx_chains(RxCall& c) {
  ofdm_handle* h = c.h;
  RxState& rx = h->rx;
  uint64_t* ctr = rx_ctr(h);
  const uint32_t nframes = (uint32_t)c.nframes;
  hipLaunchKernelGGL(k_chain_collect, dim3((nframes + 255) / 256), dim3(256), 0, h->stream, rx.res.as<FrameResult>(), nframes, c.dynf,
                     rx.chain_list.as<uint32_t>(), 4096u, reinterpret_cast<unsigned int*>(ctr + CT_CHAIN));
  uint32_t npre = 0;
  std::vector<uint8_t> pre_host;
  if (rx.nco_ref_on && c.nforced > c.n_lo) {
    npre = (uint32_t)std::min<uint64_t>(c.nforced - c.n_lo, c.nframes);
    pre_host.assign(rx.hist_swallowed.begin() + c.n_lo, rx.hist_swallowed.begin() + c.n_lo + npre);
    HIPCHK(h, rx.pre_inv.ensure(npre));
    HIPCHK(h, hipMemcpyAsync(rx.pre_inv.p, pre_host.data(), npre, hipMemcpyHostToDevice, h->stream));
  }
  hipLaunchKernelGGL(k_chain_resolve, dim3(1), dim3(64), 0, h->stream, rx.res.as<FrameResult>(), nframes, c.dynf,
                     rx.chain_list.as<uint32_t>(), 4096u, reinterpret_cast<const unsigned int*>(ctr + CT_CHAIN),
                     rx.invalid.as<uint8_t>(), reinterpret_cast<unsigned int*>(ctr + CT_OVERFLOW), rx.pre_inv.as<uint8_t>(), npre);
  HIPCHK(h, hipGetLastError());
  if (npre) HIPCHK(h, hipStreamSynchronize(h->stream));  // pre_host is read by the copy above
  return OFDM_OK;
}

// debug taps of the mixer and of the demodulator's stages: the latter from a second, instrumented pass over the frames
static int rx_tap_pass(RxCall& c) {
  ofdm_handle* h = c.h;
  RxState& rx = h->rx;
  // (soft-decision receive reads the sink's rows: it asks for them whatever the caller's mask says)
  const uint32_t tapm = h->tap_mask | (rx.soft_on ? (1u << OFDM_TAP_RX_SINK) : 0u);
  auto on = [&](int tap) { return (tapm >> tap) & 1u; };
  const uint64_t nsamples = c.nsamples, nsym = c.nsym;
  if (on(OFDM_TAP_RX_SIGMIX) || on(OFDM_TAP_RX_NCO)) {
    c32 *d_sm = nullptr, *d_nco = nullptr;
    if (on(OFDM_TAP_RX_SIGMIX)) {
      HIPCHK(h, rx.tap_sigmix.ensure(nsamples * sizeof(c32)));
      d_sm = rx.tap_sigmix.as<c32>();
    }
    if (on(OFDM_TAP_RX_NCO)) {
      HIPCHK(h, rx.tap_nco.ensure(nsamples * sizeof(c32)));
      d_nco = rx.tap_nco.as<c32>();
    }
    hipLaunchKernelGGL(k_sigmix_tap, dim3((unsigned)((nsamples + 255) / 256)), dim3(256), 0, h->stream, rx.y_ptr, nsamples,
                       rx.peaks.as<uint64_t>(), rx.Phi.as<double>(), rx.step.as<double>(), c.npeaks, c.dq.ref_on, c.dq.ref_peak,
                       c.dq.ref_phi, c.dq.ref_step, d_sm, d_nco);
    HIPCHK(h, hipGetLastError());
  }
  if (!(on(OFDM_TAP_RX_FFT) || on(OFDM_TAP_RX_ACQ) || on(OFDM_TAP_RX_SINK) || on(OFDM_TAP_RX_SAMPLER))) return OFDM_OK;
  DemodParams tq = c.dq;
  tq.tap_mode = 1;
  tq.qual = nullptr;  // (the records come from the optimistic pass)
  tq.csi_eq = nullptr;  // (so do the channel-state rows)
  tq.csi_pre = tq.csi_err = tq.csi_ref = nullptr;
  if (on(OFDM_TAP_RX_SAMPLER)) {
    HIPCHK(h, rx.tap_sampler.ensure(nsym * (uint64_t)h->N * sizeof(c32)));
    tq.tap_sampler = rx.tap_sampler.as<c32>();
  }
  if (on(OFDM_TAP_RX_FFT)) {
    HIPCHK(h, rx.tap_fft.ensure(nsym * (uint64_t)h->N * sizeof(c32)));
    tq.tap_fft = rx.tap_fft.as<c32>();
  }
  if (on(OFDM_TAP_RX_ACQ)) {
    HIPCHK(h, rx.tap_acq.ensure(nsym * (uint64_t)h->occ * sizeof(c32)));
    tq.tap_acq = rx.tap_acq.as<c32>();
  }
  if (on(OFDM_TAP_RX_SINK)) {
    HIPCHK(h, rx.tap_sink.ensure(nsym * (uint64_t)h->occ * sizeof(c32)));
    HIPCHK(h, rx.tap_demapped.ensure(nsym));
    HIPCHK(h, hipMemsetAsync(rx.tap_sink.p, 0, nsym * (uint64_t)h->occ * sizeof(c32), h->stream));
    HIPCHK(h, hipMemsetAsync(rx.tap_demapped.p, 0, nsym, h->stream));
    tq.tap_sink = rx.tap_sink.as<c32>();
    tq.tap_demapped = rx.tap_demapped.as<uint8_t>();
  }
  return run_demod(h, tq);
}

static DeframeParams make_deframe_params(const RxCall& c) {
  ofdm_handle* h = c.h;
  RxState& rx = h->rx;
  DeframeParams fq;
  memset(&fq, 0, sizeof(fq));
  fq.dyn = c.dynf;
  fq.nframes = (uint32_t)c.nframes;
  fq.res = rx.res.as<FrameResult>();
  fq.invalid = rx.invalid.as<uint8_t>();
  fq.raw = rx.raw.as<uint8_t>();
  fq.mask = h->d_mask.as<uint8_t>();
  fq.crc_table = h->d_crc.as<uint32_t>();
  fq.xp8 = h->d_xp8.as<uint32_t>();
  fq.key = rx.key.as<uint64_t>();
  fq.pos = rx.pos.as<uint64_t>();
  fq.counters = rx_ctr(h) + CT_DEFR;
  return fq;
}

// the deframer's count pass: which frames deliver a packet, where each goes in the call's packet list and payload
static int rx_deframe_count(RxCall& c) {
  ofdm_handle* h = c.h;
  RxState& rx = h->rx;
  const uint64_t nframes = c.nframes;
  const unsigned grid = (unsigned)((nframes + 255) / 256);
  c.fq = make_deframe_params(c);
  hipLaunchKernelGGL(k_deframe_count, dim3(grid), dim3(256), 0, h->stream, c.fq);
  HIPCHK(h, hipGetLastError());
  int rc = dev_excl_scan<uint64_t>(h, rx.key.as<uint64_t>(), nframes, rx.pos.as<uint64_t>(), rx_ctr(h) + CT_KEYTOT);
  if (rc) return rc;
  if (h->tap_mask & (1u << OFDM_TAP_RX_PACKETS)) {
    HIPCHK(h, rx.raw_lens.ensure(nframes * sizeof(uint64_t)));
    HIPCHK(h, rx.raw_pos.ensure(nframes * sizeof(uint64_t)));
    hipLaunchKernelGGL(k_raw_len, dim3(grid), dim3(256), 0, h->stream, c.fq, rx.raw_lens.as<uint64_t>());
    rc = dev_excl_scan<uint64_t>(h, rx.raw_lens.as<uint64_t>(), nframes, rx.raw_pos.as<uint64_t>(), rx_ctr(h) + CT_RAWTOT);
  }
  return rc;
}

static QualityParams make_quality_params(ofdm_handle* h) {
  RxState& rx = h->rx;
  QualityParams qw;
  qw.fq = rx.qual_frame.as<FrameQuality>();
  qw.step = rx.step.as<double>();
  qw.out = rx.qual_out.as<ofdm_pkt_quality>();
  qw.inv_npilot = h->q_npilot ? 1.0f / (float)h->q_npilot : 0.0f;
  qw.inv_nnull = h->q_nnull ? 1.0f / (float)h->q_nnull : 0.0f;
  qw.N = h->N;
  qw.nmap = h->nmap;
  return qw;
}

// Outputs: payload bytes and packet metadata (k_deframe_write), link quality, channel state, the raw-packet tap, and
// the copies of the metadata to the caller.  dyn: the packet count is not known here -- at most one per frame, and no
// more than the caller has room for; the entries behind the real count are scratch.
static int rx_outputs(RxCall& c) {
  ofdm_handle* h = c.h;
  RxState& rx = h->rx;
  DeframeParams& fq = c.fq;
  const uint64_t nframes = c.nframes;
  const uint64_t npk_ub = c.npk_ub = c.dyn ? std::min<uint64_t>(nframes, (uint64_t)c.max_pkts) : c.npk;
  c.d_pay = c.payload_out;
  if (npk_ub == 0) return OFDM_OK;
  HIPCHK(h, rx.out_off.ensure((npk_ub + 1) * sizeof(uint64_t)));
  HIPCHK(h, rx.out_len.ensure(npk_ub * sizeof(uint32_t)));
  HIPCHK(h, rx.out_ok.ensure(npk_ub));
  HIPCHK(h, rx.out_pos.ensure(npk_ub * sizeof(uint64_t)));
  if (!h->dev_ptrs) {
    // (dyn: every frame could carry a maximum-length message -- but never more than the caller's buffer takes)
    const uint64_t stage = c.dyn ? std::min<uint64_t>(c.payload_cap, nframes * (uint64_t)OFDM_MAX_PKT_LEN) : c.nbytes;
    HIPCHK(h, rx.out_payload.ensure(std::max<uint64_t>(stage, 1)));
    c.d_pay = rx.out_payload.as<uint8_t>();
  }
  fq.payload_out = c.d_pay;
  fq.payload_cap = c.dyn ? c.payload_cap : c.nbytes;
  fq.out_off = rx.out_off.as<uint64_t>();
  fq.out_len = rx.out_len.as<uint32_t>();
  fq.out_ok = rx.out_ok.as<uint8_t>();
  fq.out_pos = rx.out_pos.as<uint64_t>();
  fq.peaks = rx.peaks.as<uint64_t>();
  fq.j0 = (uint32_t)c.n_lo;
  fq.max_pkts = (uint32_t)npk_ub;
  hipLaunchKernelGGL(k_deframe_write, dim3((unsigned)((nframes + 3) / 4)), dim3(256), 0, h->stream, fq);
  HIPCHK(h, hipGetLastError());
  if (rx.quality_on) {
    HIPCHK(h, rx.qual_out.ensure(npk_ub * sizeof(ofdm_pkt_quality)));
    hipLaunchKernelGGL(k_quality_write, dim3((unsigned)((nframes + 255) / 256)), dim3(256), 0, h->stream, fq, make_quality_params(h));
    HIPCHK(h, hipGetLastError());
  }
  if (rx.csi_on) {
    HIPCHK(h, rx.csi_rows.ensure(csi_bytes(npk_ub, (uint64_t)rx.csi_stride)));
    rx.csi_rows_cap = npk_ub;
    hipLaunchKernelGGL(k_csi_write, dim3((unsigned)((nframes + 3) / 4)), dim3(256), 0, h->stream, fq, c.csi_fr,
                       csi_carve(rx.csi_rows, npk_ub, (uint64_t)rx.csi_stride), rx.csi_stride);
    HIPCHK(h, hipGetLastError());
  }
  if (h->tap_mask & (1u << OFDM_TAP_RX_PACKETS)) {
    rx.raw_tap_bytes = c.rawtot;
    HIPCHK(h, rx.raw_tap.ensure(std::max<uint64_t>(rx.raw_tap_bytes, 1)));
    hipLaunchKernelGGL(k_raw_tap, dim3((unsigned)((nframes + 255) / 256)), dim3(256), 0, h->stream, fq, rx.raw_pos.as<uint64_t>(),
                       rx.raw_tap.as<uint8_t>());
    HIPCHK(h, hipGetLastError());
  }
  HIPCHK(h, hipMemcpyAsync(c.payload_off, rx.out_off.p, npk_ub * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(c.payload_len, rx.out_len.p, npk_ub * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(c.crc_ok, rx.out_ok.p, npk_ub, hipMemcpyDeviceToHost, h->stream));
  rx.last_pos.resize(npk_ub);
  HIPCHK(h, hipMemcpyAsync(rx.last_pos.data(), rx.out_pos.p, npk_ub * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
  if (rx.quality_on) {
    rx.last_quality.resize(npk_ub);
    HIPCHK(h, hipMemcpyAsync(rx.last_quality.data(), rx.qual_out.p, npk_ub * sizeof(ofdm_pkt_quality), hipMemcpyDeviceToHost,
                             h->stream));
  }
  if (!c.dyn && !h->dev_ptrs && c.nbytes)
    HIPCHK(h, hipMemcpyAsync(c.payload_out, c.d_pay, c.nbytes, hipMemcpyDeviceToHost, h->stream));
  return OFDM_OK;
}

// Soft-decision receive: the values of the packets k_deframe_write kept, 8 per payload byte at 8 times the payload's
// offset, from the tap pass's sink rows and the frames' equaliser rows (rx_soft.h).  Such a call reads its counts as it
// goes (rx_counts_on_device), so the packet list is final here.
static int rx_soft_values(RxCall& c) {
  ofdm_handle* h = c.h;
  RxState& rx = h->rx;
  if (!rx.soft_on || c.npk_ub == 0) return OFDM_OK;
  HIPCHK(h, rx.soft_vals.ensure(std::max<uint64_t>(soft_values(c.nbytes), 16)));
  SoftParams sp;
  memset(&sp, 0, sizeof(sp));
  sp.sink = rx.tap_sink.as<c32>();
  sp.sink_rows = c.nsym;
  sp.sym_base = rx.sym_base.as<uint64_t>();
  sp.eq = c.csi_fr.eq;
  sp.eq_stride = rx.csi_stride;
  sp.smap = h->d_smap.as<int16_t>();
  sp.cst = h->d_const.as<c32>();
  sp.occ = h->occ;
  sp.nmap = h->nmap;
  sp.nbits = h->nbits;
  sp.arity = (int)h->cfg.arity;
  sp.scale = rx.soft_scale;
  sp.dmin2 = rx.soft_dmin2;
  sp.out = rx.soft_vals.as<int8_t>();
  if (sp.nbits < 1 || sp.nbits > (int)SOFT_MAX_BITS || sp.arity > (1 << SOFT_MAX_BITS) || sp.nmap < 1)
    FAIL(h, OFDM_E_INVAL, "soft-decision receive needs 1 to 8 bits per carrier");
  const bool timing = h->prof.on;
  if (timing) {
    if (!rx.soft_ev_a) {
      HIPCHK(h, hipEventCreate(&rx.soft_ev_a));
      HIPCHK(h, hipEventCreate(&rx.soft_ev_b));
    }
    HIPCHK(h, hipEventRecord(rx.soft_ev_a, h->stream));
  }
  const dim3 grid((unsigned)c.nframes), block(SOFT_THREADS);
  const size_t shmem = (size_t)sp.nmap * sizeof(float);
  switch (sp.nbits) {  // (the kernel unrolls its per-bit work to the constellation's bits)
#define SOFT_LAUNCH(NB) \
  case NB: hipLaunchKernelGGL(HIP_KERNEL_NAME(k_soft_demap<NB>), grid, block, shmem, h->stream, c.fq, sp); break;
    SOFT_LAUNCH(1) SOFT_LAUNCH(2) SOFT_LAUNCH(3) SOFT_LAUNCH(4) SOFT_LAUNCH(5) SOFT_LAUNCH(6) SOFT_LAUNCH(7) SOFT_LAUNCH(8)
#undef SOFT_LAUNCH
  }
  HIPCHK(h, hipGetLastError());
  if (timing) {
    HIPCHK(h, hipEventRecord(rx.soft_ev_b, h->stream));
    rx.soft_timed = true;  // (read after the call's final synchronisation: ofdm_rx_soft_last_ms)
  }
  return OFDM_OK;
}

// The final read-back (dyn: the first time the host learns the frame and packet counts, hence the capacity check and
// the payload copy here) and what the call leaves for its accessors.
static int rx_finish(RxCall& c) {
  ofdm_handle* h = c.h;
  RxState& rx = h->rx;
  int rc = rx_read_counts(c);
  if (rc) return rc;
  const uint64_t npk = c.npk, nframes = c.nframes;
  if (c.dyn) {
    rx.last_pos.resize(std::min<uint64_t>(npk, c.npk_ub));
    if (rx.quality_on) rx.last_quality.resize(std::min<uint64_t>(npk, c.npk_ub));
    if ((rc = rx_check_capacity(c))) return rc;
    if (!h->dev_ptrs && c.nbytes) HIPCHK(h, hipMemcpy(c.payload_out, c.d_pay, c.nbytes, hipMemcpyDeviceToHost));
  }
  rx.last_swallowed.assign(rx.npeaks, 0);
  if (nframes) {
    std::vector<uint8_t> inv(nframes);
    HIPCHK(h, hipMemcpy(inv.data(), rx.invalid.p, nframes, hipMemcpyDeviceToHost));
    for (uint64_t f = 0; f < nframes && rx.j0 + f < rx.npeaks; f++) rx.last_swallowed[rx.j0 + f] = inv[f];
  }
  if (npk > 0) c.payload_off[npk] = c.nbytes;
  *c.npkt = (int)npk;
  if (rx.csi_on) {
    rx.csi_n = npk;
    rx.csi_ok.assign(c.crc_ok, c.crc_ok + npk);
  }
  if (rx.soft_on && npk > 0) {
    rx.soft_off.resize(npk + 1);
    soft_plan_offsets(c.payload_off, npk, rx.soft_off.data());
    rx.soft_len.assign(c.payload_len, c.payload_len + npk);
  }
  if (c.stats) {
    uint64_t nok = 0;
    for (uint64_t i = 0; i < npk; i++) nok += c.crc_ok[i] ? 1 : 0;
    c.stats->packets = npk;
    c.stats->crc_ok = nok;
  }
  return OFDM_OK;
}

// validate the arguments, reset what the last call left
static int rx_begin(RxCall& c) {
  ofdm_handle* h = c.h;
  if (!c.npkt || c.max_pkts < 0 || (c.nsamples && !c.iq)) FAIL(h, OFDM_E_INVAL, "null argument");
  if (c.max_pkts > 0 && (!c.payload_off || !c.payload_len || !c.crc_ok)) FAIL(h, OFDM_E_INVAL, "null metadata array");
  *c.npkt = 0;
  if (c.payload_off) c.payload_off[0] = 0;
  if (c.stats) memset(c.stats, 0, sizeof(*c.stats));
  RxState& rx = h->rx;
  rx.nsamples = c.nsamples;
  rx.npeaks = rx.nframes = rx.j0 = rx.nsym_total = rx.raw_tap_bytes = rx.run_slots = 0;
  rx.last_pos.clear();
  rx.last_swallowed.clear();
  rx.last_quality.clear();
  rx.quality_valid = rx.quality_on;
  rx.csi_valid = rx.csi_on;
  rx.csi_n = 0;
  rx.csi_ok.clear();
  rx.soft_valid = rx.soft_on;
  rx.soft_timed = false;
  rx.soft_off.assign(1, 0);
  rx.soft_len.clear();
  if (c.stats) c.stats->samples = c.nsamples;
  return OFDM_OK;
}

// the input stage (already queued when the caller went through ofdm_rx_submit)
static int rx_input(RxCall& c) {
  ofdm_handle* h = c.h;
  RxState& rx = h->rx;
  if (rx.sub_valid && rx.sub_iq == c.iq && rx.sub_n == c.nsamples) {
    c.d_x = rx.sub_dx;
    rx.in_event_at_end = h->cfg.sync_mode != OFDM_SYNC_PN || h->sense.rx_on;
  } else {
    int rcs = rx_submit_impl(h, c.iq, c.nsamples, &c.d_x);
    if (rcs != OFDM_OK) return rcs;
  }
  rx.sub_valid = false;
  // chan_filt: the filtered stream, or -- SYNC "fixed": gr.multiply_const_cc(1.0) -- the input itself
  rx.y_ptr = c.fixed ? c.d_x : rx.y.as<c32>();
  if (c.fixed && h->rx_fmt == OFDM_IQ_SC16) {
    // no filter to convert in, and the demodulator gathers float samples: expand once into the y workspace
    HIPCHK(h, rx.y.ensure(c.nsamples * sizeof(c32)));
    const unsigned grid = (unsigned)std::min<uint64_t>((c.nsamples + 255) / 256, 256 * 8);
    hipLaunchKernelGGL(k_expand_sc16, dim3(grid), dim3(256), 0, h->stream, reinterpret_cast<const sc16*>(c.d_x), c.nsamples,
                       h->rx_scale, rx.y.as<c32>());
    HIPCHK(h, hipGetLastError());
    rx.y_ptr = rx.y.as<c32>();
  }
  return OFDM_OK;
}

// which count path this call takes (RxCall::dyn)
static bool rx_counts_on_device(const ofdm_handle* h) {
  const uint32_t probes = (1u << OFDM_TAP_RX_SIGMIX) | (1u << OFDM_TAP_RX_NCO) | (1u << OFDM_TAP_RX_FFT) | (1u << OFDM_TAP_RX_ACQ) |
                          (1u << OFDM_TAP_RX_SINK) | (1u << OFDM_TAP_RX_SAMPLER) | (1u << OFDM_TAP_RX_PACKETS);
  return !h->rx.nco_ref_on && !(h->tap_mask & probes) && !h->rx.soft_on && !getenv("OFDM_RX_SYNCS");
}

static int rx_impl(RxCall& c) {
  ofdm_handle* h = c.h;
  int rc = rx_begin(c);
  if (rc || c.nsamples == 0) return rc;
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  c.fixed = h->cfg.sync_mode == OFDM_SYNC_FIXED;
  if ((rc = rx_input(c))) return rc;
  if ((rc = rx_timing(c)) || c.done) return rc;  // flags -> splice -> frames / NCO / sampler
  // From here on nothing the HOST needs is known before the end of the call, unless this call reads the counts as it goes
  c.dyn = rx_counts_on_device(h);
  c.nframes = c.npeaks;  // (dyn: an upper bound until the final read-back)
  if (!c.dyn && ((rc = rx_read_counts(c)) || c.nframes == 0)) return rc;
  c.dynf.lo = c.dyn ? reinterpret_cast<const unsigned int*>(rx_ctr(h) + CT_NLO) : nullptr;
  c.dynf.hi = c.dyn ? reinterpret_cast<const unsigned int*>(rx_ctr(h) + CT_NHI) : nullptr;
  c.dynf.npeaks = (uint32_t)c.npeaks;
  if ((rc = rx_demodulate(c))) return rc;
  {
    ProfScope span(h->prof, OFDM_K_DEFRAME, h->stream);
    if ((rc = rx_chains(c)) || (rc = rx_tap_pass(c)) || (rc = rx_deframe_count(c))) return rc;
    if (!c.dyn && ((rc = rx_read_counts(c)) || (rc = rx_check_capacity(c)))) return rc;
    if ((rc = rx_outputs(c))) return rc;
  }
  if ((rc = rx_soft_values(c))) return rc;
  return rx_finish(c);
}

extern "C" int ofdm_rx(ofdm_handle* h, const ofdm_c32* iq, uint64_t nsamples, uint8_t* payload_out, uint64_t payload_cap,
                       uint64_t* payload_off, uint32_t* payload_len, uint8_t* crc_ok, int max_pkts, int* npkt,
                       ofdm_stats* stats) {
  if (!h) return OFDM_E_INVAL;
  h->rx.in_event_at_end = false;
  RxCall c{h, iq, nsamples, payload_out, payload_cap, payload_off, payload_len, crc_ok, max_pkts, npkt, stats};
  const int rc = rx_impl(c);
  h->rx.sub_valid = false;
  h->rx.sub_hold = false;
  // the fused sensor works on its own stream beside the peak pass and the demodulator: joined here, before the caller
  // gets its input buffer back
  if (h->sense.rx_on && h->sense.side) (void)hipStreamSynchronize(h->sense.side);
  h->prof.collect();  // every exit of the call comes through here, its spans closed
  if (h->rx.in_event_at_end) {  // the input was read to the end of the call (SYNC "fixed", fused sensing)
    h->rx.in_event_at_end = false;
    rx_note_input(h, iq, nsamples);
    if (hipEventRecord(h->ev_rx_in, h->stream) == hipSuccess) h->rx_in_pending = true;
  }
  return rc;
}

// ------------------------------------------------------------------------------------
// debug taps
// ------------------------------------------------------------------------------------
static int copy_tap(ofdm_handle* h, const void* d_src, uint64_t bytes, void* out, uint64_t cap, uint64_t* nbytes) {
  if (nbytes) *nbytes = bytes;
  if (!out || bytes == 0) return OFDM_OK;
  if (cap < bytes) FAIL(h, OFDM_E_CAPACITY, "tap buffer too small");
  HIPCHK(h, hipMemcpy(out, d_src, bytes, hipMemcpyDeviceToHost));
  return OFDM_OK;
}

__global__ void k_gather_frames(const uint64_t* __restrict__ peaks, const uint32_t* __restrict__ K, uint64_t j0, uint64_t nframes,
                                uint64_t* __restrict__ out) {
  const uint64_t f = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= nframes) return;
  out[2 * f] = peaks[j0 + f];
  out[2 * f + 1] = K[j0 + f];
}

extern "C" int ofdm_tap(ofdm_handle* h, int tap, void* out, uint64_t cap, uint64_t* nbytes) {
  if (!h) return OFDM_E_INVAL;
  if (tap < 0 || tap >= OFDM_TAP_COUNT) FAIL(h, OFDM_E_INVAL, "unknown tap");
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  // the transmit taps are written on the transmit stream (ofdm_tx_async, a pipelined batch)
  if (h->txs != h->stream) HIPCHK(h, hipStreamSynchronize(h->txs));
  RxState& rx = h->rx;
  const bool en = (h->tap_mask >> tap) & 1u;
  switch (tap) {
    case OFDM_TAP_TX_PACKETS:
      return copy_tap(h, h->d_framed.p, h->last_tx_framed_bytes, out, cap, nbytes);
    case OFDM_TAP_TX_FREQ:
      if (!en && !((h->tap_mask >> OFDM_TAP_TX_MAPPER) & 1u)) FAIL(h, OFDM_E_INVAL, "tap not enabled (ofdm_set_taps)");
      return copy_tap(h, h->d_freq_tap.p, h->last_tx_nsym * (uint64_t)h->N * sizeof(c32), out, cap, nbytes);
    case OFDM_TAP_RX_CHAN_FILT:
      return copy_tap(h, rx.y_ptr, rx.y_ptr ? rx.nsamples * sizeof(c32) : 0, out, cap, nbytes);
    case OFDM_TAP_TX_IFFT:
      if (!en) FAIL(h, OFDM_E_INVAL, "tap not enabled (ofdm_set_taps)");
      return copy_tap(h, h->d_ifft_tap.p, h->last_tx_nsym * (uint64_t)h->N * sizeof(c32), out, cap, nbytes);
    case OFDM_TAP_TX_MAPPER: {
      // ofdm_mapper_c.dat: the mapper's own output, i.e. every symbol but the preamble insert_preamble puts in front of
      // each packet -- the rows of TX_FREQ that are not the first symbol of a packet
      if (!en) FAIL(h, OFDM_E_INVAL, "tap not enabled (ofdm_set_taps)");
      const uint64_t rowb = (uint64_t)h->N * sizeof(c32);
      const uint64_t npk = h->last_sym_off.empty() ? 0 : h->last_sym_off.size() - 1;
      const uint64_t rows = h->last_tx_nsym - npk;
      if (nbytes) *nbytes = rows * rowb;
      if (!out || rows == 0) return OFDM_OK;
      if (cap < rows * rowb) FAIL(h, OFDM_E_CAPACITY, "tap buffer too small");
      uint64_t r = 0;
      for (uint64_t k = 0; k < npk; k++) {
        const uint64_t s0 = h->last_sym_off[k] + 1, s1 = h->last_sym_off[k + 1];
        if (s1 > s0)
          HIPCHK(h, hipMemcpy((uint8_t*)out + r * rowb, (const uint8_t*)h->d_freq_tap.p + s0 * rowb, (s1 - s0) * rowb, hipMemcpyDeviceToHost));
        r += s1 - s0;
      }
      return OFDM_OK;
    }
    case OFDM_TAP_RX_SAMPLER:
      if (!en) FAIL(h, OFDM_E_INVAL, "tap not enabled (ofdm_set_taps)");
      return copy_tap(h, rx.tap_sampler.p, rx.nframes ? rx.nsym_total * (uint64_t)h->N * sizeof(c32) : 0, out, cap, nbytes);
    case OFDM_TAP_RX_SIGMIX:
      if (!en) FAIL(h, OFDM_E_INVAL, "tap not enabled (ofdm_set_taps)");
      return copy_tap(h, rx.tap_sigmix.p, rx.nframes ? rx.nsamples * sizeof(c32) : 0, out, cap, nbytes);
    case OFDM_TAP_RX_NCO:
      if (!en) FAIL(h, OFDM_E_INVAL, "tap not enabled (ofdm_set_taps)");
      return copy_tap(h, rx.tap_nco.p, rx.nframes ? rx.nsamples * sizeof(c32) : 0, out, cap, nbytes);
    case OFDM_TAP_RX_METRIC:
      if (!en) FAIL(h, OFDM_E_INVAL, "tap not enabled (ofdm_set_taps)");
      if (h->cfg.sync_mode == OFDM_SYNC_FIXED) FAIL(h, OFDM_E_INVAL, "SYNC \"fixed\" computes no timing metric");
      return copy_tap(h, rx.metric.p, rx.nsamples * sizeof(float), out, cap, nbytes);
    case OFDM_TAP_RX_PRESEL:
      if (!en) FAIL(h, OFDM_E_INVAL, "tap not enabled (ofdm_set_taps)");
      if (h->cfg.sync_mode == OFDM_SYNC_FIXED) FAIL(h, OFDM_E_INVAL, "SYNC \"fixed\" computes no timing metric");
      return copy_tap(h, rx.presel.p, rx.nsamples * sizeof(float), out, cap, nbytes);
    case OFDM_TAP_RX_RUN_AVG: {
      // rows of the piece slots the count pass wrote (their order follows the chunked allocation), by first sample
      if (!en) FAIL(h, OFDM_E_INVAL, "tap not enabled (ofdm_set_taps)");
      if (h->cfg.sync_mode == OFDM_SYNC_FIXED) FAIL(h, OFDM_E_INVAL, "SYNC \"fixed\" runs no peak detector");
      std::vector<double> all(rx.run_slots * 2);
      if (rx.run_slots) HIPCHK(h, hipMemcpy(all.data(), rx.run_rows.p, all.size() * sizeof(double), hipMemcpyDeviceToHost));
      std::vector<std::pair<double, double>> rows;
      for (uint64_t i = 0; i < rx.run_slots; i++)
        if (all[2 * i] == all[2 * i]) rows.emplace_back(all[2 * i], all[2 * i + 1]);
      std::sort(rows.begin(), rows.end());
      const uint64_t nb = rows.size() * 2 * sizeof(double);
      if (nbytes) *nbytes = nb;
      if (!out || nb == 0) return OFDM_OK;
      if (cap < nb) FAIL(h, OFDM_E_CAPACITY, "tap buffer too small");
      double* o = static_cast<double*>(out);
      for (size_t i = 0; i < rows.size(); i++) {
        o[2 * i] = rows[i].first;
        o[2 * i + 1] = rows[i].second;
      }
      return OFDM_OK;
    }
    case OFDM_TAP_RX_PEAKS:
      return copy_tap(h, rx.peaks.p, rx.npeaks * sizeof(uint64_t), out, cap, nbytes);
    case OFDM_TAP_RX_ANGLES:
      return copy_tap(h, rx.angle.p, rx.npeaks * sizeof(float), out, cap, nbytes);
    case OFDM_TAP_RX_FRAMES: {
      if (nbytes) *nbytes = rx.nframes * 2 * sizeof(uint64_t);
      if (!out || rx.nframes == 0) return OFDM_OK;
      HIPCHK(h, rx.partial.ensure(rx.nframes * 2 * sizeof(uint64_t)));
      hipLaunchKernelGGL(k_gather_frames, dim3((unsigned)((rx.nframes + 255) / 256)), dim3(256), 0, h->stream,
                         rx.peaks.as<uint64_t>(), rx.K.as<uint32_t>(), rx.j0, rx.nframes, rx.partial.as<uint64_t>());
      HIPCHK(h, hipStreamSynchronize(h->stream));
      return copy_tap(h, rx.partial.p, rx.nframes * 2 * sizeof(uint64_t), out, cap, nbytes);
    }
    case OFDM_TAP_RX_FFT:
      if (!en) FAIL(h, OFDM_E_INVAL, "tap not enabled (ofdm_set_taps)");
      return copy_tap(h, rx.tap_fft.p, rx.nframes ? rx.nsym_total * (uint64_t)h->N * sizeof(c32) : 0, out, cap, nbytes);
    case OFDM_TAP_RX_ACQ:
      if (!en) FAIL(h, OFDM_E_INVAL, "tap not enabled (ofdm_set_taps)");
      return copy_tap(h, rx.tap_acq.p, rx.nframes ? rx.nsym_total * (uint64_t)h->occ * sizeof(c32) : 0, out, cap, nbytes);
    case OFDM_TAP_RX_SINK: {
      // rows of the symbols the sink actually demapped, in stream order (host-side compaction)
      if (!en) FAIL(h, OFDM_E_INVAL, "tap not enabled (ofdm_set_taps)");
      if (rx.nframes == 0 || rx.nsym_total == 0) {
        if (nbytes) *nbytes = 0;
        return OFDM_OK;
      }
      std::vector<uint8_t> flags(rx.nsym_total);
      HIPCHK(h, hipMemcpy(flags.data(), rx.tap_demapped.p, rx.nsym_total, hipMemcpyDeviceToHost));
      uint64_t rows = 0;
      for (uint64_t i = 0; i < rx.nsym_total; i++) rows += flags[i] ? 1 : 0;
      const uint64_t rowb = (uint64_t)h->occ * sizeof(c32);
      if (nbytes) *nbytes = rows * rowb;
      if (!out) return OFDM_OK;
      if (cap < rows * rowb) FAIL(h, OFDM_E_CAPACITY, "tap buffer too small");
      uint64_t r = 0;
      for (uint64_t i = 0; i < rx.nsym_total; i++)
        if (flags[i]) {
          HIPCHK(h, hipMemcpy((uint8_t*)out + r * rowb, (const uint8_t*)rx.tap_sink.p + i * rowb, rowb, hipMemcpyDeviceToHost));
          r++;
        }
      return OFDM_OK;
    }
    case OFDM_TAP_RX_PACKETS:
      if (!en) FAIL(h, OFDM_E_INVAL, "tap not enabled (ofdm_set_taps)");
      return copy_tap(h, rx.raw_tap.p, rx.raw_tap_bytes, out, cap, nbytes);
    case OFDM_TAP_RX_DEMAPPED:
      if (!((h->tap_mask >> OFDM_TAP_RX_SINK) & 1u)) FAIL(h, OFDM_E_INVAL, "tap needs OFDM_TAP_RX_SINK enabled (ofdm_set_taps)");
      return copy_tap(h, rx.tap_demapped.p, rx.nframes ? rx.nsym_total : 0, out, cap, nbytes);
  }
  return OFDM_E_INVAL;
}

// ------------------------------------------------------------------------------------
// chunked streams: packet positions and NCO phase continuity
// ------------------------------------------------------------------------------------
extern "C" int ofdm_rx_packet_pos(ofdm_handle* h, uint64_t* pos, int cap, int* n) {
  if (!h) return OFDM_E_INVAL;
  const size_t np = h->rx.last_pos.size();
  if (n) *n = (int)np;
  if (np == 0 || !pos) return OFDM_OK;  // pos == NULL: size query
  if ((size_t)cap < np) FAIL(h, OFDM_E_CAPACITY, "position array too small");
  memcpy(pos, h->rx.last_pos.data(), np * sizeof(uint64_t));
  return OFDM_OK;
}

extern "C" int ofdm_rx_nco_state(ofdm_handle* h, uint64_t* peaks, uint64_t* phi, double* step, uint8_t* swallowed, int cap,
                                 int* n) {
  if (!h) return OFDM_E_INVAL;
  RxState& rx = h->rx;
  if (n) *n = (int)std::min<uint64_t>(rx.npeaks, 0x7FFFFFFF);
  if (rx.npeaks == 0 || (!peaks && !phi && !step && !swallowed)) return OFDM_OK;  // all NULL: size query
  if (!peaks || !phi || !step || !swallowed || (uint64_t)cap < rx.npeaks) FAIL(h, OFDM_E_CAPACITY, "NCO state arrays too small");
  for (uint64_t i = 0; i < rx.npeaks; i++) swallowed[i] = i < rx.last_swallowed.size() ? rx.last_swallowed[i] : 0;
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  HIPCHK(h, hipMemcpy(peaks, rx.peaks.p, rx.npeaks * sizeof(uint64_t), hipMemcpyDeviceToHost));
  HIPCHK(h, hipMemcpy(phi, rx.Phi_u.p, rx.npeaks * sizeof(uint64_t), hipMemcpyDeviceToHost));
  HIPCHK(h, hipMemcpy(step, rx.step.p, rx.npeaks * sizeof(double), hipMemcpyDeviceToHost));
  return OFDM_OK;
}

extern "C" int ofdm_rx_snr(const ofdm_handle* h, float* snr_est) {
  if (!h || !snr_est) return OFDM_E_INVAL;
  *snr_est = 0.0f;  // d_snr_est of digital_ofdm_frame_acquisition: set to 0 by the constructor, never updated (GR 3.6.0)
  return OFDM_OK;
}

extern "C" int ofdm_set_rx_quality(ofdm_handle* h, int enable) {
  if (!h) return OFDM_E_INVAL;
  h->rx.quality_on = enable != 0;
  return OFDM_OK;
}

extern "C" int ofdm_rx_quality(ofdm_handle* h, ofdm_pkt_quality* out, int cap, int* n) {
  if (!h) return OFDM_E_INVAL;
  const RxState& rx = h->rx;
  if (!rx.quality_valid) FAIL(h, OFDM_E_INVAL, "the last ofdm_rx ran without link quality (ofdm_set_rx_quality)");
  const size_t np = rx.last_quality.size();
  if (n) *n = (int)np;
  if (np == 0 || !out) return OFDM_OK;  // out == NULL: size query
  if ((size_t)cap < np) FAIL(h, OFDM_E_CAPACITY, "quality array too small");
  memcpy(out, rx.last_quality.data(), np * sizeof(ofdm_pkt_quality));
  return OFDM_OK;
}

extern "C" int ofdm_set_rx_csi(ofdm_handle* h, int enable) {
  if (!h) return OFDM_E_INVAL;
  h->rx.csi_on = enable != 0;
  return OFDM_OK;
}

// the four packet-row arrays of the last call
static CsiRows csi_packet_rows(const RxState& rx) { return csi_carve(rx.csi_rows, rx.csi_rows_cap, (uint64_t)rx.csi_stride); }

extern "C" int ofdm_rx_csi(ofdm_handle* h, int first, int count, ofdm_c32* eq, float* pre_power, float* err, float* ref, int* n) {
  if (!h) return OFDM_E_INVAL;
  if (!n) FAIL(h, OFDM_E_INVAL, "null argument");
  const RxState& rx = h->rx;
  if (!rx.csi_valid) FAIL(h, OFDM_E_INVAL, "the last ofdm_rx ran without channel state (ofdm_set_rx_csi)");
  *n = (int)rx.csi_n;
  if (count == 0) return OFDM_OK;  // size query
  if (first < 0 || count < 0 || (uint64_t)first + (uint64_t)count > rx.csi_n) FAIL(h, OFDM_E_INVAL, "rows out of range");
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  const CsiRows pk = csi_packet_rows(rx);
  const size_t st = (size_t)rx.csi_stride, occ = (size_t)h->occ, r0 = (size_t)first * st;
  if (eq)
    HIPCHK(h, hipMemcpy2DAsync(eq, occ * sizeof(c32), pk.eq + r0, st * sizeof(c32), occ * sizeof(c32), (size_t)count,
                               hipMemcpyDeviceToHost, h->stream));
  float* dst[3] = {pre_power, err, ref};
  const float* src[3] = {pk.pre, pk.err, pk.ref};
  for (int a = 0; a < 3; a++)
    if (dst[a])
      HIPCHK(h, hipMemcpy2DAsync(dst[a], occ * sizeof(float), src[a] + r0, st * sizeof(float), occ * sizeof(float), (size_t)count,
                                 hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return OFDM_OK;
}

extern "C" int ofdm_rx_csi_summary(ofdm_handle* h, int crc_ok_only, uint32_t* npkt, double* pre_power, double* err, double* ref,
                                   double* inv_gain, uint32_t* ninv) {
  if (!h) return OFDM_E_INVAL;
  RxState& rx = h->rx;
  if (!rx.csi_valid) FAIL(h, OFDM_E_INVAL, "the last ofdm_rx ran without channel state (ofdm_set_rx_csi)");
  const int occ = h->occ;
  uint64_t np = 0;
  for (uint64_t p = 0; p < rx.csi_n; p++) np += (!crc_ok_only || rx.csi_ok[p]) ? 1 : 0;
  if (npkt) *npkt = (uint32_t)np;
  double* dst[CSI_S_COUNT] = {pre_power, err, ref, inv_gain};
  if (np == 0) {
    for (int k = 0; k < CSI_S_COUNT; k++)
      if (dst[k]) std::fill(dst[k], dst[k] + occ, 0.0);
    if (ninv) std::fill(ninv, ninv + occ, 0u);
    return OFDM_OK;
  }
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  CsiSumParams s;
  s.rows = csi_packet_rows(rx);
  s.ok = rx.out_ok.as<uint8_t>();  // (the device copy of the verdicts: intact until the next ofdm_rx)
  s.npk = (uint32_t)rx.csi_n;
  s.occ = occ;
  s.stride = rx.csi_stride;
  s.crc_ok_only = crc_ok_only ? 1 : 0;
  s.nchunks = (uint32_t)((rx.csi_n + CSI_SUM_CHUNK - 1) / CSI_SUM_CHUNK);
  const uint64_t part = (uint64_t)s.nchunks * (uint64_t)occ;
  HIPCHK(h, rx.csi_part.ensure(part * (CSI_S_COUNT * sizeof(double) + sizeof(uint32_t))));
  HIPCHK(h, rx.csi_sum.ensure((uint64_t)occ * (CSI_S_COUNT * sizeof(double) + sizeof(uint32_t))));
  s.part = rx.csi_part.as<double>();
  s.part_n = reinterpret_cast<uint32_t*>(s.part + CSI_S_COUNT * part);
  s.out = rx.csi_sum.as<double>();
  s.out_n = reinterpret_cast<uint32_t*>(s.out + CSI_S_COUNT * occ);
  const unsigned gx = (unsigned)((occ + 255) / 256);
  hipLaunchKernelGGL(k_csi_summary, dim3(gx, s.nchunks), dim3(256), 0, h->stream, s);
  HIPCHK(h, hipGetLastError());
  hipLaunchKernelGGL(k_csi_summary_combine, dim3(gx), dim3(256), 0, h->stream, s);
  HIPCHK(h, hipGetLastError());
  for (int k = 0; k < CSI_S_COUNT; k++)
    if (dst[k])
      HIPCHK(h, hipMemcpyAsync(dst[k], s.out + (size_t)k * occ, occ * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (ninv) HIPCHK(h, hipMemcpyAsync(ninv, s.out_n, occ * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return OFDM_OK;
}

extern "C" int ofdm_rx_set_origin(ofdm_handle* h, uint64_t first_sample_index) {
  if (!h) return OFDM_E_INVAL;
  h->rx.origin = first_sample_index;
  return OFDM_OK;
}

extern "C" int ofdm_rx_set_flag_history(ofdm_handle* h, int enable, int n, const int64_t* flags, const double* steps,
                                        const uint8_t* swallowed, int64_t trust_after, int64_t pred_flag, uint64_t pred_phase, double pred_step) {
  if (!h) return OFDM_E_INVAL;
  RxState& rx = h->rx;
  rx.nco_ref_on = false;
  rx.hist_flags.clear();
  rx.hist_steps.clear();
  rx.hist_swallowed.clear();
  if (!enable) return OFDM_OK;
  if (n < 0 || (n > 0 && (!flags || !steps || !swallowed))) FAIL(h, OFDM_E_INVAL, "null argument");
  for (int i = 0; i < n; i++) {
    if (flags[i] < 0 || flags[i] > trust_after || (i > 0 && flags[i] <= flags[i - 1]) || flags[i] <= pred_flag)
      FAIL(h, OFDM_E_INVAL, "history flags must ascend inside [0, trust_after] and follow the predecessor");
    rx.hist_flags.push_back((uint64_t)flags[i]);
    rx.hist_steps.push_back(steps[i]);
    rx.hist_swallowed.push_back(swallowed[i]);
  }
  rx.nco_ref_on = true;
  rx.nco_trust_after = trust_after;
  rx.nco_ref_peak = pred_flag;
  rx.nco_ref_u = pred_phase;
  rx.nco_ref_step = pred_step;
  return OFDM_OK;
}
