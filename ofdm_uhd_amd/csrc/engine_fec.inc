// engine_fec.inc -- host side of the coded-link layer (fec.h): lengths, batch layout, slicing, launches.
// Included by engine.hip after engine_multipath.inc.  The arithmetic that needs no GPU is fec_plan.h.

extern "C" int ofdm_fec_coded_len(uint32_t payload_len, uint32_t* coded_len) { return fec_coded_len(payload_len, coded_len); }
extern "C" int ofdm_fec_payload_len(uint32_t coded_len, uint32_t* payload_len) { return fec_payload_len(coded_len, payload_len); }

extern "C" int ofdm_fec_last_ms(const ofdm_handle* h, double* ms) {
  if (!h || !ms || !h->fec.timed) return OFDM_E_INVAL;
  *ms = h->fec.last_ms;
  return OFDM_OK;
}

extern "C" int ofdm_fec_coded_len_rate(uint32_t rate, uint32_t payload_len, uint32_t* coded_len) {
  return punct_coded_len(rate, payload_len, coded_len);
}
extern "C" int ofdm_fec_payload_len_rate(uint32_t rate, uint32_t coded_len, uint32_t* payload_len) {
  return punct_payload_len(rate, coded_len, payload_len);
}

extern "C" int ofdm_fec_punct_last_ms(const ofdm_handle* h, double* ms) {
  if (!h || !ms || !h->fec_punct.timed) return OFDM_E_INVAL;
  *ms = h->fec_punct.last_ms;
  return OFDM_OK;
}

// the rate of a call (after fec_cols has checked the struct); every fec call passes here, so the punctured kernels'
// time is of the last call or of none
static int fec_rate(ofdm_handle* h, const ofdm_fec_cfg* cfg, uint32_t* rate) {
  h->fec_punct.timed = false;
  *rate = cfg ? cfg->rate : (uint32_t)OFDM_FEC_RATE_1_2;
  if (!punct_rate_ok(*rate)) FAIL(h, OFDM_E_INVAL, "fec rate must be OFDM_FEC_RATE_1_2, _2_3, _3_4 or _5_6");
  return OFDM_OK;
}

static int fec_cols(ofdm_handle* h, const ofdm_fec_cfg* cfg, uint32_t* lgC) {
  uint32_t cols = 16;
  if (cfg) {
    if (cfg->struct_size != sizeof(ofdm_fec_cfg)) FAIL(h, OFDM_E_INVAL, "ofdm_fec_cfg.struct_size does not match this library");
    cols = cfg->interleave_cols;
  }
  const int l = fec_log2_cols(cols);
  if (l < 0) FAIL(h, OFDM_E_INVAL, "fec interleave_cols must be 1, 2, 4, 8 or 16");
  *lgC = (uint32_t)l;
  return OFDM_OK;
}

static int fec_time_begin(ofdm_handle* h, FecState& f, hipStream_t st, bool timing) {
  if (!timing) return OFDM_OK;
  if (!f.ev_a) {
    HIPCHK(h, hipEventCreate(&f.ev_a));
    HIPCHK(h, hipEventCreate(&f.ev_b));
  }
  HIPCHK(h, hipEventRecord(f.ev_a, st));
  return OFDM_OK;
}

static int fec_finish(ofdm_handle* h, FecState& f, hipStream_t st, bool timing) {
  HIPCHK(h, hipStreamSynchronize(st));
  if (timing) {
    float ms = 0.f;
    HIPCHK(h, hipEventElapsedTime(&ms, f.ev_a, f.ev_b));
    f.last_ms = (double)ms;
    f.timed = true;
  }
  return OFDM_OK;
}

// ---- punctured rates (fec_punct.h): the same two calls with k_fec_puncture in the encoder's place and k_fec_depuncture in
// front of every decoder slice.  Entered from ofdm_fec_encode / fec_decode_impl behind their argument checks.
template <uint32_t RATE>
static void fec_launch_puncture(hipStream_t st, unsigned nblk, const uint8_t* d_in, const FecBlk* d_blk, uint8_t* d_out, const uint32_t* crc,
                                const uint32_t* xp8, uint32_t lgC) {
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fec_puncture<RATE>), dim3(nblk), dim3(FEC_ENC_THREADS), 0, st, d_in, d_blk, d_out, crc, xp8, lgC);
}
template <uint32_t RATE, bool SOFT>
static void fec_launch_depuncture(hipStream_t st, unsigned nblk, const uint8_t* d_in, const FecBlk* d_blk, int8_t* d_mother, uint32_t lgC) {
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fec_depuncture<RATE, SOFT>), dim3(nblk), dim3(FEC_DEPUNCT_THREADS), 0, st, d_in, d_blk, d_mother, lgC);
}

static int fec_encode_punct(ofdm_handle* h, uint32_t rate, uint32_t lgC, const uint8_t* payloads, const uint64_t* payload_off,
                            const uint32_t* payload_len, int nblk, uint8_t* coded, uint64_t coded_cap, uint64_t* coded_off) {
  FecState& f = h->fec;
  FecPunctState& fp = h->fec_punct;
  f.blk.resize((size_t)nblk);
  uint64_t extent = 0;
  const uint64_t total = punct_plan_encode(rate, payload_off, payload_len, (uint64_t)nblk, f.blk.data(), coded_off, &extent);
  if (total == ~0ull) FAIL(h, OFDM_E_INVAL, "fec: len(payload) must be in [0, 2040]");
  f.timed = false;
  if (total > coded_cap) FAIL(h, OFDM_E_CAPACITY, "coded buffer too small (see ofdm_fec_coded_len_rate)");
  if (nblk == 0) return OFDM_OK;
  if (!coded) FAIL(h, OFDM_E_INVAL, "null argument");
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  hipStream_t st = h->txs;
  const uint8_t* d_in = payloads;
  uint8_t* d_out = coded;
  HIPCHK(h, f.d_blk.ensure(sizeof(FecBlk) * (size_t)nblk));
  HIPCHK(h, hipMemcpyAsync(f.d_blk.p, f.blk.data(), sizeof(FecBlk) * (size_t)nblk, hipMemcpyHostToDevice, st));
  if (!h->dev_ptrs) {
    HIPCHK(h, f.d_in.ensure(std::max<uint64_t>(extent, 1)));
    if (extent) HIPCHK(h, hipMemcpyAsync(f.d_in.p, payloads, extent, hipMemcpyHostToDevice, st));
    HIPCHK(h, f.d_out.ensure(total));
    d_in = f.d_in.as<uint8_t>();
    d_out = f.d_out.as<uint8_t>();
  }
  const bool timing = h->prof.on;
  RCCHK(fec_time_begin(h, f, st, timing));
  const uint32_t *crc = h->d_crc.as<uint32_t>(), *xp8 = h->d_xp8.as<uint32_t>();
  switch (rate) {
    case OFDM_FEC_RATE_2_3: fec_launch_puncture<OFDM_FEC_RATE_2_3>(st, (unsigned)nblk, d_in, f.d_blk.as<FecBlk>(), d_out, crc, xp8, lgC); break;
    case OFDM_FEC_RATE_3_4: fec_launch_puncture<OFDM_FEC_RATE_3_4>(st, (unsigned)nblk, d_in, f.d_blk.as<FecBlk>(), d_out, crc, xp8, lgC); break;
    default: fec_launch_puncture<OFDM_FEC_RATE_5_6>(st, (unsigned)nblk, d_in, f.d_blk.as<FecBlk>(), d_out, crc, xp8, lgC); break;
  }
  if (timing) HIPCHK(h, hipEventRecord(f.ev_b, st));
  HIPCHK(h, hipGetLastError());
  if (!h->dev_ptrs) HIPCHK(h, hipMemcpyAsync(coded, d_out, total, hipMemcpyDeviceToHost, st));
  RCCHK(fec_finish(h, f, st, timing));
  if (timing) {  // k_fec_puncture is this call's encoder and its only kernel
    fp.last_ms = f.last_ms;
    fp.timed = true;
  }
  return OFDM_OK;
}

template <bool SOFT>
static int fec_decode_punct(ofdm_handle* h, uint32_t rate, uint32_t lgC, const uint8_t* in, const uint64_t* in_off, const uint32_t* coded_len,
                            int nblk, uint8_t* payloads, uint64_t payload_cap, uint64_t* payload_off, uint8_t* ok, uint32_t* corrected,
                            bool in_on_device) {
  FecState& f = h->fec;
  FecPunctState& fp = h->fec_punct;
  fp.pblk.resize((size_t)nblk);
  f.blk.resize((size_t)nblk);
  uint64_t stride = 0, mstride = 0, extent = 0;
  const uint64_t total = punct_plan_decode_sizes(rate, in_off, coded_len, (uint64_t)nblk, SOFT ? 8u : 1u, fp.pblk.data(), payload_off, &stride,
                                                 &mstride, &extent);
  f.timed = false;
  if (total > payload_cap) FAIL(h, OFDM_E_CAPACITY, "payload buffer too small (see ofdm_fec_payload_len_rate)");
  if (nblk == 0) return OFDM_OK;
  if (total && !payloads) FAIL(h, OFDM_E_INVAL, "null argument");
  if (stride == 0) {  // not one block among them: nothing to launch
    memset(ok, 0, (size_t)nblk);
    memset(corrected, 0, sizeof(uint32_t) * (size_t)nblk);
    return OFDM_OK;
  }
  const uint64_t per = fec_slice_blocks((uint64_t)nblk, stride, FEC_WS_MAX_BYTES);
  punct_plan_decode_slots((uint64_t)nblk, per, mstride, payload_off, fp.pblk.data(), f.blk.data());
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  hipStream_t st = h->stream;
  if (h->tx_pending && h->txs != h->stream) HIPCHK(h, hipStreamWaitEvent(st, h->ev_tx_done, 0));
  const uint8_t* d_in = in;
  uint8_t* d_out = payloads;
  const size_t tbytes = sizeof(FecBlk) * (size_t)nblk;
  HIPCHK(h, f.d_blk.ensure(tbytes));
  HIPCHK(h, fp.d_pblk.ensure(tbytes));
  HIPCHK(h, hipMemcpyAsync(f.d_blk.p, f.blk.data(), tbytes, hipMemcpyHostToDevice, st));
  HIPCHK(h, hipMemcpyAsync(fp.d_pblk.p, fp.pblk.data(), tbytes, hipMemcpyHostToDevice, st));
  HIPCHK(h, f.d_ok.ensure((size_t)nblk));
  HIPCHK(h, f.d_corr.ensure(sizeof(uint32_t) * (size_t)nblk));
  if (!h->dev_ptrs) {
    if (!in_on_device) {
      HIPCHK(h, f.d_in.ensure(std::max<uint64_t>(extent, 1)));
      HIPCHK(h, hipMemcpyAsync(f.d_in.p, in, extent, hipMemcpyHostToDevice, st));
      d_in = f.d_in.as<uint8_t>();
    }
    HIPCHK(h, f.d_out.ensure(std::max<uint64_t>(total, 1)));
    d_out = f.d_out.as<uint8_t>();
  }
  // the mother values are cut like the decision workspace: a slice's blocks own `mstride` values each, a quarter of
  // their share of the workspace, and the next slice writes over them behind this slice's decoder (stream order)
  HIPCHK(h, f.d_ws.ensure(per * stride * sizeof(uint64_t)));
  HIPCHK(h, fp.d_mother.ensure(per * mstride));
  const bool timing = h->prof.on;
  const uint64_t nslices = ((uint64_t)nblk + per - 1) / per;
  if (timing) {  // three events per slice: depuncture | decoder
    while (fp.ev.size() < 3 * nslices) {
      hipEvent_t e = nullptr;
      HIPCHK(h, hipEventCreate(&e));
      fp.ev.push_back(e);
    }
  }
  uint64_t s = 0;
  for (uint64_t b0 = 0; b0 < (uint64_t)nblk; b0 += per, s++) {
    const unsigned nb = (unsigned)std::min<uint64_t>(per, (uint64_t)nblk - b0);
    const FecBlk* d_pblk = fp.d_pblk.as<FecBlk>() + b0;
    int8_t* d_mother = fp.d_mother.as<int8_t>();
    if (timing) HIPCHK(h, hipEventRecord(fp.ev[3 * s], st));
    switch (rate) {
      case OFDM_FEC_RATE_2_3: fec_launch_depuncture<OFDM_FEC_RATE_2_3, SOFT>(st, nb, d_in, d_pblk, d_mother, lgC); break;
      case OFDM_FEC_RATE_3_4: fec_launch_depuncture<OFDM_FEC_RATE_3_4, SOFT>(st, nb, d_in, d_pblk, d_mother, lgC); break;
      default: fec_launch_depuncture<OFDM_FEC_RATE_5_6, SOFT>(st, nb, d_in, d_pblk, d_mother, lgC); break;
    }
    if (timing) HIPCHK(h, hipEventRecord(fp.ev[3 * s + 1], st));
    // the unchanged soft decoder on the mother values, coded order: one column
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fec_decode<true>), dim3(nb), dim3(WAVE), 0, st, fp.d_mother.as<uint8_t>(), f.d_blk.as<FecBlk>() + b0,
                       d_out, f.d_ok.as<uint8_t>() + b0, f.d_corr.as<uint32_t>() + b0, f.d_ws.as<uint64_t>(), stride, h->d_crc.as<uint32_t>(),
                       h->d_xp8.as<uint32_t>(), 0u);
    if (timing) HIPCHK(h, hipEventRecord(fp.ev[3 * s + 2], st));
  }
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipMemcpyAsync(ok, f.d_ok.p, (size_t)nblk, hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipMemcpyAsync(corrected, f.d_corr.p, sizeof(uint32_t) * (size_t)nblk, hipMemcpyDeviceToHost, st));
  if (!h->dev_ptrs && total) HIPCHK(h, hipMemcpyAsync(payloads, d_out, total, hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipStreamSynchronize(st));
  if (timing) {
    double dep = 0.0, dec = 0.0;
    for (uint64_t k = 0; k < nslices; k++) {
      float a = 0.f, b = 0.f;
      HIPCHK(h, hipEventElapsedTime(&a, fp.ev[3 * k], fp.ev[3 * k + 1]));
      HIPCHK(h, hipEventElapsedTime(&b, fp.ev[3 * k + 1], fp.ev[3 * k + 2]));
      dep += (double)a;
      dec += (double)b;
    }
    fp.last_ms = dep;
    fp.timed = true;
    f.last_ms = dec;
    f.timed = true;
  }
  return OFDM_OK;
}

/* payloads in, coded blocks out: what ofdm_tx / ofdm_make_packets then take as payloads */
extern "C" int ofdm_fec_encode(ofdm_handle* h, const ofdm_fec_cfg* cfg, const uint8_t* payloads, const uint64_t* payload_off,
                               const uint32_t* payload_len, int nblk, uint8_t* coded, uint64_t coded_cap, uint64_t* coded_off) {
  if (!h) return OFDM_E_INVAL;
  FecState& f = h->fec;
  if (nblk < 0 || (nblk && (!payloads || !payload_off || !payload_len)) || !coded_off) FAIL(h, OFDM_E_INVAL, "null argument");
  uint32_t lgC, rate;
  RCCHK(fec_cols(h, cfg, &lgC));
  RCCHK(fec_rate(h, cfg, &rate));
  if (rate != OFDM_FEC_RATE_1_2) return fec_encode_punct(h, rate, lgC, payloads, payload_off, payload_len, nblk, coded, coded_cap, coded_off);
  f.blk.resize((size_t)nblk);
  uint64_t total = 0, extent = 0;
  for (int k = 0; k < nblk; k++) {
    uint32_t cl;
    if (fec_coded_len(payload_len[k], &cl) != OFDM_OK) FAIL(h, OFDM_E_INVAL, "fec: len(payload) must be in [0, 2040]");
    f.blk[k] = FecBlk{payload_off[k], total, payload_len[k], 0};
    coded_off[k] = total;
    total += cl;
    extent = std::max<uint64_t>(extent, payload_off[k] + payload_len[k]);
  }
  coded_off[nblk] = total;
  f.timed = false;
  if (total > coded_cap) FAIL(h, OFDM_E_CAPACITY, "coded buffer too small (see ofdm_fec_coded_len)");
  if (nblk == 0) return OFDM_OK;
  if (!coded) FAIL(h, OFDM_E_INVAL, "null argument");
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  hipStream_t st = h->txs;  // the transmit side: ordered with the ofdm_tx that takes the blocks
  const uint8_t* d_in = payloads;
  uint8_t* d_out = coded;
  HIPCHK(h, f.d_blk.ensure(sizeof(FecBlk) * (size_t)nblk));
  HIPCHK(h, hipMemcpyAsync(f.d_blk.p, f.blk.data(), sizeof(FecBlk) * (size_t)nblk, hipMemcpyHostToDevice, st));
  if (!h->dev_ptrs) {
    HIPCHK(h, f.d_in.ensure(std::max<uint64_t>(extent, 1)));
    if (extent) HIPCHK(h, hipMemcpyAsync(f.d_in.p, payloads, extent, hipMemcpyHostToDevice, st));
    HIPCHK(h, f.d_out.ensure(total));
    d_in = f.d_in.as<uint8_t>();
    d_out = f.d_out.as<uint8_t>();
  }
  const bool timing = h->prof.on;
  RCCHK(fec_time_begin(h, f, st, timing));
  hipLaunchKernelGGL(k_fec_encode, dim3((unsigned)nblk), dim3(FEC_ENC_THREADS), 0, st, d_in, f.d_blk.as<FecBlk>(), d_out,
                     h->d_crc.as<uint32_t>(), h->d_xp8.as<uint32_t>(), lgC);
  if (timing) HIPCHK(h, hipEventRecord(f.ev_b, st));
  HIPCHK(h, hipGetLastError());
  if (!h->dev_ptrs) HIPCHK(h, hipMemcpyAsync(coded, d_out, total, hipMemcpyDeviceToHost, st));
  return fec_finish(h, f, st, timing);  // (synchronises: the staged block table is the caller's again)
}

// `unit` input items per coded byte: 1 (hard bytes) or 8 (int8 values).  in_on_device: the input blob is device memory
// whatever the handle's pointer mode (the handle's own soft values: ofdm_rx_fec_decode_soft)
template <bool SOFT>
static int fec_decode_impl(ofdm_handle* h, const ofdm_fec_cfg* cfg, const uint8_t* in, const uint64_t* in_off, const uint32_t* coded_len,
                           int nblk, uint8_t* payloads, uint64_t payload_cap, uint64_t* payload_off, uint8_t* ok, uint32_t* corrected,
                           bool in_on_device = false) {
  if (!h) return OFDM_E_INVAL;
  FecState& f = h->fec;
  if (nblk < 0 || (nblk && (!in || !in_off || !coded_len || !ok || !corrected)) || !payload_off) FAIL(h, OFDM_E_INVAL, "null argument");
  uint32_t lgC, rate;
  RCCHK(fec_cols(h, cfg, &lgC));
  RCCHK(fec_rate(h, cfg, &rate));
  if (rate != OFDM_FEC_RATE_1_2)
    return fec_decode_punct<SOFT>(h, rate, lgC, in, in_off, coded_len, nblk, payloads, payload_cap, payload_off, ok, corrected, in_on_device);
  f.blk.resize((size_t)nblk);
  uint64_t stride = 0, extent = 0;
  const uint64_t total = fec_plan_decode(in_off, coded_len, (uint64_t)nblk, SOFT ? 8u : 1u, f.blk.data(), payload_off, &stride, &extent);
  f.timed = false;
  if (total > payload_cap) FAIL(h, OFDM_E_CAPACITY, "payload buffer too small (see ofdm_fec_payload_len)");
  if (nblk == 0) return OFDM_OK;
  if (total && !payloads) FAIL(h, OFDM_E_INVAL, "null argument");
  if (stride == 0) {  // not one block among them: nothing to launch
    memset(ok, 0, (size_t)nblk);
    memset(corrected, 0, sizeof(uint32_t) * (size_t)nblk);
    return OFDM_OK;
  }
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  hipStream_t st = h->stream;  // the receive side: ordered behind the ofdm_rx that delivered the blocks
  if (h->tx_pending && h->txs != h->stream) HIPCHK(h, hipStreamWaitEvent(st, h->ev_tx_done, 0));
  const uint8_t* d_in = in;
  uint8_t* d_out = payloads;
  HIPCHK(h, f.d_blk.ensure(sizeof(FecBlk) * (size_t)nblk));
  HIPCHK(h, hipMemcpyAsync(f.d_blk.p, f.blk.data(), sizeof(FecBlk) * (size_t)nblk, hipMemcpyHostToDevice, st));
  HIPCHK(h, f.d_ok.ensure((size_t)nblk));
  HIPCHK(h, f.d_corr.ensure(sizeof(uint32_t) * (size_t)nblk));
  if (!h->dev_ptrs) {
    if (!in_on_device) {
      HIPCHK(h, f.d_in.ensure(std::max<uint64_t>(extent, 1)));
      HIPCHK(h, hipMemcpyAsync(f.d_in.p, in, extent, hipMemcpyHostToDevice, st));
      d_in = f.d_in.as<uint8_t>();
    }
    HIPCHK(h, f.d_out.ensure(std::max<uint64_t>(total, 1)));
    d_out = f.d_out.as<uint8_t>();
  }
  // every block in flight owns `stride` decision words; the workspace is bounded, a larger batch goes in slices
  const uint64_t per = fec_slice_blocks((uint64_t)nblk, stride, FEC_WS_MAX_BYTES);
  HIPCHK(h, f.d_ws.ensure(per * stride * sizeof(uint64_t)));
  const bool timing = h->prof.on;
  RCCHK(fec_time_begin(h, f, st, timing));
  for (uint64_t b0 = 0; b0 < (uint64_t)nblk; b0 += per) {
    const uint64_t nb = std::min<uint64_t>(per, (uint64_t)nblk - b0);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fec_decode<SOFT>), dim3((unsigned)nb), dim3(WAVE), 0, st, d_in, f.d_blk.as<FecBlk>() + b0, d_out,
                       f.d_ok.as<uint8_t>() + b0, f.d_corr.as<uint32_t>() + b0, f.d_ws.as<uint64_t>(), stride, h->d_crc.as<uint32_t>(),
                       h->d_xp8.as<uint32_t>(), lgC);
  }
  if (timing) HIPCHK(h, hipEventRecord(f.ev_b, st));
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipMemcpyAsync(ok, f.d_ok.p, (size_t)nblk, hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipMemcpyAsync(corrected, f.d_corr.p, sizeof(uint32_t) * (size_t)nblk, hipMemcpyDeviceToHost, st));
  if (!h->dev_ptrs && total) HIPCHK(h, hipMemcpyAsync(payloads, d_out, total, hipMemcpyDeviceToHost, st));
  return fec_finish(h, f, st, timing);
}

/* hard bytes in; payloads, ok[] and corrected[] out */
extern "C" int ofdm_fec_decode(ofdm_handle* h, const ofdm_fec_cfg* cfg, const uint8_t* coded, const uint64_t* coded_off,
                               const uint32_t* coded_len, int nblk, uint8_t* payloads, uint64_t payload_cap, uint64_t* payload_off,
                               uint8_t* ok, uint32_t* corrected) {
  return fec_decode_impl<false>(h, cfg, coded, coded_off, coded_len, nblk, payloads, payload_cap, payload_off, ok, corrected);
}

/* the same from int8 values, 8 per coded byte */
extern "C" int ofdm_fec_decode_soft(ofdm_handle* h, const ofdm_fec_cfg* cfg, const int8_t* soft, const uint64_t* soft_off,
                                    const uint32_t* coded_len, int nblk, uint8_t* payloads, uint64_t payload_cap,
                                    uint64_t* payload_off, uint8_t* ok, uint32_t* corrected) {
  return fec_decode_impl<true>(h, cfg, reinterpret_cast<const uint8_t*>(soft), soft_off, coded_len, nblk, payloads, payload_cap,
                               payload_off, ok, corrected);
}
