// engine_fec.inc -- host side of the coded-link layer (fec.h): lengths, batch layout, slicing, launches.
// Included by engine.hip after engine_multipath.inc.  The arithmetic that needs no GPU is fec_plan.h.

extern "C" int ofdm_fec_coded_len(uint32_t payload_len, uint32_t* coded_len) { return fec_coded_len(payload_len, coded_len); }
extern "C" int ofdm_fec_payload_len(uint32_t coded_len, uint32_t* payload_len) { return fec_payload_len(coded_len, payload_len); }

extern "C" int ofdm_fec_last_ms(const ofdm_handle* h, double* ms) {
  if (!h || !ms || !h->fec.timed) return OFDM_E_INVAL;
  *ms = h->fec.last_ms;
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

/* payloads in, coded blocks out: what ofdm_tx / ofdm_make_packets then take as payloads */
extern "C" int ofdm_fec_encode(ofdm_handle* h, const ofdm_fec_cfg* cfg, const uint8_t* payloads, const uint64_t* payload_off,
                               const uint32_t* payload_len, int nblk, uint8_t* coded, uint64_t coded_cap, uint64_t* coded_off) {
  if (!h) return OFDM_E_INVAL;
  FecState& f = h->fec;
  if (nblk < 0 || (nblk && (!payloads || !payload_off || !payload_len)) || !coded_off) FAIL(h, OFDM_E_INVAL, "null argument");
  uint32_t lgC;
  RCCHK(fec_cols(h, cfg, &lgC));
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
  uint32_t lgC;
  RCCHK(fec_cols(h, cfg, &lgC));
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
