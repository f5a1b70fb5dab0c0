// engine_rs.inc -- host side of the outer code (rs.h): lengths, batch layout, launches, over the steps of
// engine_codec.inc.  Included by engine.hip after engine_soft.inc.  The arithmetic that needs no GPU is rs_plan.h.  One
// block table per call, one kernel per call.

extern "C" int ofdm_rs_coded_len(uint32_t payload_len, uint32_t* coded_len) { return rs_coded_len(payload_len, coded_len); }
extern "C" int ofdm_rs_payload_len(uint32_t coded_len, uint32_t* payload_len) { return rs_payload_len(coded_len, payload_len); }

extern "C" int ofdm_rs_last_ms(const ofdm_handle* h, double* ms) { return h ? codec_last_ms(h->rs, ms) : OFDM_E_INVAL; }
extern "C" int ofdm_rs_rel_last_ms(const ofdm_handle* h, double* ms) { return h ? codec_last_ms(h->rs.rel_clock, ms) : OFDM_E_INVAL; }

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
  hipStream_t st;
  RCCHK(codec_begin_encode(h, &st));
  const uint8_t* d_in;
  uint8_t* d_out;
  RCCHK(codec_upload(h, st, f.d_blk, f.blk, (size_t)nblk));
  RCCHK(codec_stage_in(h, st, f.d_in, payloads, extent, false, &d_in));
  RCCHK(codec_stage_out(h, f.d_out, coded, total, &d_out));
  const bool timing = h->prof.on;
  RCCHK(codec_time_begin(h, f, st, timing));
  hipLaunchKernelGGL(k_rs_encode, dim3((unsigned)nblk), dim3(RS_THREADS), 0, st, d_in, f.d_blk.as<RsBlk>(), d_out, h->d_crc.as<uint32_t>(),
                     h->d_xp8.as<uint32_t>());
  RCCHK(codec_launched(h, f, st, timing));
  RCCHK(codec_read_out(h, st, coded, d_out, total));
  return codec_finish(h, f, st, timing);
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
  hipStream_t st;
  RCCHK(codec_begin_decode(h, &st));
  const uint8_t *d_in, *d_rel = nullptr;
  uint8_t* d_out;
  RCCHK(codec_upload(h, st, f.d_blk, f.blk, (size_t)nblk));
  HIPCHK(h, f.d_ok.ensure((size_t)nblk));
  HIPCHK(h, f.d_corr.ensure(sizeof(uint32_t) * (size_t)nblk));
  HIPCHK(h, f.d_fail.ensure(sizeof(uint32_t) * (size_t)nblk));
  RCCHK(codec_stage_in(h, st, f.d_in, coded, extent, false, &d_in));
  RCCHK(codec_stage_out(h, f.d_out, payloads, total, &d_out));
  if (rel) {
    uint64_t rel_extent = 0;
    f.reloff.resize((size_t)nblk);
    rs_plan_rel(coded_off, rel_off, coded_len, (uint64_t)nblk, f.reloff.data(), &rel_extent);
    RCCHK(codec_upload(h, st, f.d_reloff, f.reloff, (size_t)nblk));
    HIPCHK(h, f.d_sec.ensure(sizeof(uint32_t) * (size_t)nblk));
    RCCHK(codec_stage_in(h, st, f.d_rel, rel, rel_extent, false, &d_rel));
  }
  const bool timing = h->prof.on;
  RCCHK(codec_time_begin(h, f, st, timing));
  if (rel)
    hipLaunchKernelGGL(k_rs_decode_rel, dim3((unsigned)nblk), dim3(RS_THREADS), 0, st, d_in, d_rel, f.d_blk.as<RsBlk>(),
                       f.d_reloff.as<uint64_t>(), M, d_out, f.d_ok.as<uint8_t>(), f.d_corr.as<uint32_t>(), f.d_fail.as<uint32_t>(),
                       f.d_sec.as<uint32_t>(), h->d_crc.as<uint32_t>(), h->d_xp8.as<uint32_t>());
  else
    hipLaunchKernelGGL(k_rs_decode, dim3((unsigned)nblk), dim3(RS_THREADS), 0, st, d_in, f.d_blk.as<RsBlk>(), d_out, f.d_ok.as<uint8_t>(),
                       f.d_corr.as<uint32_t>(), f.d_fail.as<uint32_t>(), h->d_crc.as<uint32_t>(), h->d_xp8.as<uint32_t>());
  RCCHK(codec_launched(h, f, st, timing));
  RCCHK(codec_read(h, st, ok, f.d_ok, nblk));
  RCCHK(codec_read(h, st, corrected, f.d_corr, nblk));
  RCCHK(codec_read(h, st, failed, f.d_fail, nblk));
  if (rel && second) RCCHK(codec_read(h, st, second, f.d_sec, nblk));
  RCCHK(codec_read_out(h, st, payloads, d_out, total));
  return codec_finish(h, f, st, timing);
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
  f.rel_clock.timed = false;
  if (total > rel_cap) FAIL(h, OFDM_E_CAPACITY, "reliability buffer too small (the sum of coded_len)");
  if (total == 0) return OFDM_OK;
  if (!rel) FAIL(h, OFDM_E_INVAL, "null argument");
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  hipStream_t st = h->stream;  // the receive side: ordered behind the ofdm_rx that made the values
  const uint8_t* d_in;
  uint8_t* d_out;
  RCCHK(codec_upload(h, st, f.d_blk, f.blk, (size_t)nblk));
  RCCHK(codec_stage_in(h, st, f.d_soft, soft, extent, false, &d_in));
  RCCHK(codec_stage_out(h, f.d_rel, rel, total, &d_out));
  const bool timing = h->prof.on;
  RCCHK(codec_time_begin(h, f.rel_clock, st, timing));
  hipLaunchKernelGGL(k_rs_rel_soft, dim3((unsigned)nblk), dim3(RS_THREADS), 0, st, reinterpret_cast<const int8_t*>(d_in), f.d_blk.as<RsBlk>(),
                     d_out);
  RCCHK(codec_launched(h, f.rel_clock, st, timing));
  RCCHK(codec_read_out(h, st, rel, d_out, total));
  return codec_finish(h, f.rel_clock, st, timing);
}
