// engine_rs.inc -- host side of the outer code (rs.h): lengths, batch layout, launches.  Included by engine.hip after
// engine_soft.inc.  The arithmetic that needs no GPU is rs_plan.h.  One block table per call, one kernel per call.

extern "C" int ofdm_rs_coded_len(uint32_t payload_len, uint32_t* coded_len) { return rs_coded_len(payload_len, coded_len); }
extern "C" int ofdm_rs_payload_len(uint32_t coded_len, uint32_t* payload_len) { return rs_payload_len(coded_len, payload_len); }

extern "C" int ofdm_rs_last_ms(const ofdm_handle* h, double* ms) {
  if (!h || !ms || !h->rs.timed) return OFDM_E_INVAL;
  *ms = h->rs.last_ms;
  return OFDM_OK;
}

static int rs_time_begin(ofdm_handle* h, RsState& f, hipStream_t st, bool timing) {
  if (!timing) return OFDM_OK;
  if (!f.ev_a) {
    HIPCHK(h, hipEventCreate(&f.ev_a));
    HIPCHK(h, hipEventCreate(&f.ev_b));
  }
  HIPCHK(h, hipEventRecord(f.ev_a, st));
  return OFDM_OK;
}

static int rs_finish(ofdm_handle* h, RsState& f, hipStream_t st, bool timing) {
  HIPCHK(h, hipStreamSynchronize(st));
  if (timing) {
    float ms = 0.f;
    HIPCHK(h, hipEventElapsedTime(&ms, f.ev_a, f.ev_b));
    f.last_ms = (double)ms;
    f.timed = true;
  }
  return OFDM_OK;
}

/* payloads in, RS blocks out: what ofdm_fec_encode, or ofdm_tx / ofdm_make_packets, then take as payloads */
extern "C" int ofdm_rs_encode(ofdm_handle* h, const uint8_t* payloads, const uint64_t* payload_off, const uint32_t* payload_len, int nblk,
                              uint8_t* coded, uint64_t coded_cap, uint64_t* coded_off) {
  if (!h) return OFDM_E_INVAL;
  RsState& f = h->rs;
  if (nblk < 0 || (nblk && (!payloads || !payload_off || !payload_len)) || !coded_off) FAIL(h, OFDM_E_INVAL, "null argument");
  f.blk.resize((size_t)nblk);
  uint64_t extent = 0;
  const uint64_t total = rs_plan_encode(payload_off, payload_len, (uint64_t)nblk, f.blk.data(), coded_off, &extent);
  if (total == ~0ull) FAIL(h, OFDM_E_INVAL, "rs: len(payload) must be in [0, 3564]");
  f.timed = false;
  if (total > coded_cap) FAIL(h, OFDM_E_CAPACITY, "coded buffer too small (see ofdm_rs_coded_len)");
  if (nblk == 0) return OFDM_OK;
  if (!coded) FAIL(h, OFDM_E_INVAL, "null argument");
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  hipStream_t st = h->txs;  // the transmit side: ordered with the ofdm_fec_encode / ofdm_tx that takes the blocks
  const uint8_t* d_in = payloads;
  uint8_t* d_out = coded;
  HIPCHK(h, f.d_blk.ensure(sizeof(RsBlk) * (size_t)nblk));
  HIPCHK(h, hipMemcpyAsync(f.d_blk.p, f.blk.data(), sizeof(RsBlk) * (size_t)nblk, hipMemcpyHostToDevice, st));
  if (!h->dev_ptrs) {
    HIPCHK(h, f.d_in.ensure(std::max<uint64_t>(extent, 1)));
    if (extent) HIPCHK(h, hipMemcpyAsync(f.d_in.p, payloads, extent, hipMemcpyHostToDevice, st));
    HIPCHK(h, f.d_out.ensure(total));
    d_in = f.d_in.as<uint8_t>();
    d_out = f.d_out.as<uint8_t>();
  }
  const bool timing = h->prof.on;
  RCCHK(rs_time_begin(h, f, st, timing));
  hipLaunchKernelGGL(k_rs_encode, dim3((unsigned)nblk), dim3(RS_THREADS), 0, st, d_in, f.d_blk.as<RsBlk>(), d_out, h->d_crc.as<uint32_t>(),
                     h->d_xp8.as<uint32_t>());
  if (timing) HIPCHK(h, hipEventRecord(f.ev_b, st));
  HIPCHK(h, hipGetLastError());
  if (!h->dev_ptrs) HIPCHK(h, hipMemcpyAsync(coded, d_out, total, hipMemcpyDeviceToHost, st));
  return rs_finish(h, f, st, timing);  // (synchronises: the staged block table is the caller's again)
}

// The decode call.  rel == NULL: ofdm_rs_decode (k_rs_decode); otherwise k_rs_decode_rel with M > 0 erasures at the most.
static int rs_decode_impl(ofdm_handle* h, const uint8_t* coded, const uint64_t* coded_off, const uint32_t* coded_len, int nblk,
                          const uint8_t* rel, const uint64_t* rel_off, uint32_t M, uint8_t* payloads, uint64_t payload_cap,
                          uint64_t* payload_off, uint8_t* ok, uint32_t* corrected, uint32_t* failed, uint32_t* second) {
  if (!h) return OFDM_E_INVAL;
  RsState& f = h->rs;
  if (nblk < 0 || (nblk && (!coded || !coded_off || !coded_len || !ok || !corrected || !failed)) || !payload_off)
    FAIL(h, OFDM_E_INVAL, "null argument");
  f.blk.resize((size_t)nblk);
  uint64_t nvalid = 0, extent = 0;
  const uint64_t total = rs_plan_decode(coded_off, coded_len, (uint64_t)nblk, f.blk.data(), payload_off, &nvalid, &extent);
  f.timed = false;
  if (total > payload_cap) FAIL(h, OFDM_E_CAPACITY, "payload buffer too small (see ofdm_rs_payload_len)");
  if (nblk == 0) return OFDM_OK;
  if (total && !payloads) FAIL(h, OFDM_E_INVAL, "null argument");
  if (second) memset(second, 0, sizeof(uint32_t) * (size_t)nblk);
  if (nvalid == 0) {  // not one block among them: nothing to launch
    memset(ok, 0, (size_t)nblk);
    memset(corrected, 0, sizeof(uint32_t) * (size_t)nblk);
    memset(failed, 0, sizeof(uint32_t) * (size_t)nblk);
    return OFDM_OK;
  }
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  hipStream_t st = h->stream;  // the receive side: ordered behind the ofdm_rx / ofdm_fec_decode that delivered the blocks
  if (h->tx_pending && h->txs != h->stream) HIPCHK(h, hipStreamWaitEvent(st, h->ev_tx_done, 0));
  const uint8_t* d_in = coded;
  const uint8_t* d_rel = rel;
  uint8_t* d_out = payloads;
  HIPCHK(h, f.d_blk.ensure(sizeof(RsBlk) * (size_t)nblk));
  HIPCHK(h, hipMemcpyAsync(f.d_blk.p, f.blk.data(), sizeof(RsBlk) * (size_t)nblk, hipMemcpyHostToDevice, st));
  HIPCHK(h, f.d_ok.ensure((size_t)nblk));
  HIPCHK(h, f.d_corr.ensure(sizeof(uint32_t) * (size_t)nblk));
  HIPCHK(h, f.d_fail.ensure(sizeof(uint32_t) * (size_t)nblk));
  if (!h->dev_ptrs) {
    HIPCHK(h, f.d_in.ensure(std::max<uint64_t>(extent, 1)));
    HIPCHK(h, hipMemcpyAsync(f.d_in.p, coded, extent, hipMemcpyHostToDevice, st));
    HIPCHK(h, f.d_out.ensure(std::max<uint64_t>(total, 1)));
    d_in = f.d_in.as<uint8_t>();
    d_out = f.d_out.as<uint8_t>();
  }
  if (rel) {
    uint64_t rel_extent = 0;
    f.reloff.resize((size_t)nblk);
    rs_plan_rel(coded_off, rel_off, coded_len, (uint64_t)nblk, f.reloff.data(), &rel_extent);
    HIPCHK(h, f.d_reloff.ensure(sizeof(uint64_t) * (size_t)nblk));
    HIPCHK(h, hipMemcpyAsync(f.d_reloff.p, f.reloff.data(), sizeof(uint64_t) * (size_t)nblk, hipMemcpyHostToDevice, st));
    HIPCHK(h, f.d_sec.ensure(sizeof(uint32_t) * (size_t)nblk));
    if (!h->dev_ptrs) {
      HIPCHK(h, f.d_rel.ensure(std::max<uint64_t>(rel_extent, 1)));
      HIPCHK(h, hipMemcpyAsync(f.d_rel.p, rel, rel_extent, hipMemcpyHostToDevice, st));
      d_rel = f.d_rel.as<uint8_t>();
    }
  }
  const bool timing = h->prof.on;
  RCCHK(rs_time_begin(h, f, st, timing));
  if (rel)
    hipLaunchKernelGGL(k_rs_decode_rel, dim3((unsigned)nblk), dim3(RS_THREADS), 0, st, d_in, d_rel, f.d_blk.as<RsBlk>(),
                       f.d_reloff.as<uint64_t>(), M, d_out, f.d_ok.as<uint8_t>(), f.d_corr.as<uint32_t>(), f.d_fail.as<uint32_t>(),
                       f.d_sec.as<uint32_t>(), h->d_crc.as<uint32_t>(), h->d_xp8.as<uint32_t>());
  else
    hipLaunchKernelGGL(k_rs_decode, dim3((unsigned)nblk), dim3(RS_THREADS), 0, st, d_in, f.d_blk.as<RsBlk>(), d_out, f.d_ok.as<uint8_t>(),
                       f.d_corr.as<uint32_t>(), f.d_fail.as<uint32_t>(), h->d_crc.as<uint32_t>(), h->d_xp8.as<uint32_t>());
  if (timing) HIPCHK(h, hipEventRecord(f.ev_b, st));
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipMemcpyAsync(ok, f.d_ok.p, (size_t)nblk, hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipMemcpyAsync(corrected, f.d_corr.p, sizeof(uint32_t) * (size_t)nblk, hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipMemcpyAsync(failed, f.d_fail.p, sizeof(uint32_t) * (size_t)nblk, hipMemcpyDeviceToHost, st));
  if (rel && second) HIPCHK(h, hipMemcpyAsync(second, f.d_sec.p, sizeof(uint32_t) * (size_t)nblk, hipMemcpyDeviceToHost, st));
  if (!h->dev_ptrs && total) HIPCHK(h, hipMemcpyAsync(payloads, d_out, total, hipMemcpyDeviceToHost, st));
  return rs_finish(h, f, st, timing);
}

/* received blocks in (what ofdm_fec_decode, or ofdm_rx, delivered); payloads, ok[], corrected[] and failed[] out */
extern "C" int ofdm_rs_decode(ofdm_handle* h, const uint8_t* coded, const uint64_t* coded_off, const uint32_t* coded_len, int nblk,
                              uint8_t* payloads, uint64_t payload_cap, uint64_t* payload_off, uint8_t* ok, uint32_t* corrected,
                              uint32_t* failed) {
  return rs_decode_impl(h, coded, coded_off, coded_len, nblk, nullptr, nullptr, 0, payloads, payload_cap, payload_off, ok, corrected, failed,
                        nullptr);
}

/* the same with one reliability byte per received byte: a codeword the first pass fails gets its weakest symbols erased */
extern "C" int ofdm_rs_decode_rel(ofdm_handle* h, const ofdm_rs_rel_cfg* cfg, const uint8_t* coded, const uint64_t* coded_off,
                                  const uint32_t* coded_len, int nblk, const uint8_t* rel, const uint64_t* rel_off, uint8_t* payloads,
                                  uint64_t payload_cap, uint64_t* payload_off, uint8_t* ok, uint32_t* corrected, uint32_t* failed,
                                  uint32_t* second) {
  if (!h) return OFDM_E_INVAL;
  uint32_t M;
  if (!rs_rel_max_erasures(cfg, &M)) FAIL(h, OFDM_E_INVAL, "rs: bad ofdm_rs_rel_cfg (struct_size, max_erasures in [0, 32], reserved 0)");
  if (M == 0) rel = nullptr;  // no erasures: ofdm_rs_decode's result, by ofdm_rs_decode's kernel
  return rs_decode_impl(h, coded, coded_off, coded_len, nblk, rel, rel_off, M, payloads, payload_cap, payload_off, ok, corrected, failed,
                        second);
}

extern "C" int ofdm_rs_rel_last_ms(const ofdm_handle* h, double* ms) {
  if (!h || !ms || !h->rs.rel_timed) return OFDM_E_INVAL;
  *ms = h->rs.rel_last_ms;
  return OFDM_OK;
}

/* int8 values in (8 per byte, as ofdm_fec_decode_soft reads them), one reliability byte per byte out */
extern "C" int ofdm_rs_rel_from_soft(ofdm_handle* h, const int8_t* soft, const uint64_t* soft_off, const uint32_t* coded_len, int nblk,
                                     uint8_t* rel, uint64_t rel_cap, uint64_t* rel_off) {
  if (!h) return OFDM_E_INVAL;
  RsState& f = h->rs;
  if (nblk < 0 || (nblk && (!soft || !soft_off || !coded_len)) || !rel_off) FAIL(h, OFDM_E_INVAL, "null argument");
  f.blk.resize((size_t)nblk);
  uint64_t extent = 0;
  const uint64_t total = rs_plan_rel_soft(soft_off, coded_len, (uint64_t)nblk, f.blk.data(), rel_off, &extent);
  if (total == ~0ull) FAIL(h, OFDM_E_INVAL, "rs: value offsets must be multiples of 8");
  f.rel_timed = false;
  if (total > rel_cap) FAIL(h, OFDM_E_CAPACITY, "reliability buffer too small (the sum of coded_len)");
  if (total == 0) return OFDM_OK;
  if (!rel) FAIL(h, OFDM_E_INVAL, "null argument");
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  hipStream_t st = h->stream;  // the receive side: ordered behind the ofdm_rx that made the values
  const int8_t* d_in = soft;
  uint8_t* d_out = rel;
  HIPCHK(h, f.d_blk.ensure(sizeof(RsBlk) * (size_t)nblk));
  HIPCHK(h, hipMemcpyAsync(f.d_blk.p, f.blk.data(), sizeof(RsBlk) * (size_t)nblk, hipMemcpyHostToDevice, st));
  if (!h->dev_ptrs) {
    HIPCHK(h, f.d_soft.ensure(extent));
    HIPCHK(h, hipMemcpyAsync(f.d_soft.p, soft, extent, hipMemcpyHostToDevice, st));
    HIPCHK(h, f.d_rel.ensure(total));
    d_in = f.d_soft.as<int8_t>();
    d_out = f.d_rel.as<uint8_t>();
  }
  const bool timing = h->prof.on;
  if (timing) {
    if (!f.ev_ra) {
      HIPCHK(h, hipEventCreate(&f.ev_ra));
      HIPCHK(h, hipEventCreate(&f.ev_rb));
    }
    HIPCHK(h, hipEventRecord(f.ev_ra, st));
  }
  hipLaunchKernelGGL(k_rs_rel_soft, dim3((unsigned)nblk), dim3(RS_THREADS), 0, st, d_in, f.d_blk.as<RsBlk>(), d_out);
  if (timing) HIPCHK(h, hipEventRecord(f.ev_rb, st));
  HIPCHK(h, hipGetLastError());
  if (!h->dev_ptrs) HIPCHK(h, hipMemcpyAsync(rel, d_out, total, hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipStreamSynchronize(st));  // (the staged block table is the caller's again)
  if (timing) {
    float ms = 0.f;
    HIPCHK(h, hipEventElapsedTime(&ms, f.ev_ra, f.ev_rb));
    f.rel_last_ms = (double)ms;
    f.rel_timed = true;
  }
  return OFDM_OK;
}
