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

/* received blocks in (what ofdm_fec_decode, or ofdm_rx, delivered); payloads, ok[], corrected[] and failed[] out */
extern "C" int ofdm_rs_decode(ofdm_handle* h, const uint8_t* coded, const uint64_t* coded_off, const uint32_t* coded_len, int nblk,
                              uint8_t* payloads, uint64_t payload_cap, uint64_t* payload_off, uint8_t* ok, uint32_t* corrected,
                              uint32_t* failed) {
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
  const bool timing = h->prof.on;
  RCCHK(rs_time_begin(h, f, st, timing));
  hipLaunchKernelGGL(k_rs_decode, dim3((unsigned)nblk), dim3(RS_THREADS), 0, st, d_in, f.d_blk.as<RsBlk>(), d_out, f.d_ok.as<uint8_t>(),
                     f.d_corr.as<uint32_t>(), f.d_fail.as<uint32_t>(), h->d_crc.as<uint32_t>(), h->d_xp8.as<uint32_t>());
  if (timing) HIPCHK(h, hipEventRecord(f.ev_b, st));
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipMemcpyAsync(ok, f.d_ok.p, (size_t)nblk, hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipMemcpyAsync(corrected, f.d_corr.p, sizeof(uint32_t) * (size_t)nblk, hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipMemcpyAsync(failed, f.d_fail.p, sizeof(uint32_t) * (size_t)nblk, hipMemcpyDeviceToHost, st));
  if (!h->dev_ptrs && total) HIPCHK(h, hipMemcpyAsync(payloads, d_out, total, hipMemcpyDeviceToHost, st));
  return rs_finish(h, f, st, timing);
}
