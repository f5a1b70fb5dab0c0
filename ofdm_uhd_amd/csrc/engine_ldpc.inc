// engine_ldpc.inc -- host side of the LDPC coded-link layer (ldpc.h): lengths, the codeword map of a batch, launches,
// over the steps of engine_codec.inc.  The three *_rel calls are the decode calls with k_ldpc_decode_rel in
// k_ldpc_decode's place and one reliability byte per payload byte next to the payloads, at the payloads' offsets.
// Included by engine.hip after engine_rs.inc.  The arithmetic that needs no GPU is ldpc_plan.h.

extern "C" int ofdm_ldpc_coded_len(uint32_t payload_len, uint32_t* coded_len) { return ldpc_coded_len(payload_len, coded_len); }
extern "C" int ofdm_ldpc_payload_len(uint32_t coded_len, uint32_t* payload_len) { return ldpc_payload_len(coded_len, payload_len); }
extern "C" int ofdm_ldpc_coded_len_rate(uint32_t rate, uint32_t payload_len, uint32_t* coded_len) {
  return ldpc_coded_len_rate(rate, payload_len, coded_len);
}
extern "C" int ofdm_ldpc_payload_len_rate(uint32_t rate, uint32_t coded_len, uint32_t* payload_len) {
  return ldpc_payload_len_rate(rate, coded_len, payload_len);
}

extern "C" int ofdm_ldpc_last_ms(const ofdm_handle* h, double* ms) { return h ? codec_last_ms(h->ldpc, ms) : OFDM_E_INVAL; }

// the call's max_iters and rate: 20 and rate 1/2 without a cfg
static int ldpc_cfg_check(ofdm_handle* h, const ofdm_ldpc_cfg* cfg, uint32_t* max_iters, uint32_t* rate) {
  *max_iters = LDPC_DEFAULT_ITERS;
  *rate = OFDM_LDPC_RATE_1_2;
  if (!cfg) return OFDM_OK;
  if (cfg->struct_size != sizeof(ofdm_ldpc_cfg)) FAIL(h, OFDM_E_INVAL, "ofdm_ldpc_cfg.struct_size does not match this library");
  if (cfg->max_iters < 1 || cfg->max_iters > LDPC_MAX_ITERS) FAIL(h, OFDM_E_INVAL, "ldpc max_iters must be in [1, 64]");
  if (cfg->rate >= LDPC_RATES) FAIL(h, OFDM_E_INVAL, "ldpc rate must be one of OFDM_LDPC_RATE_*");
  for (int i = 1; i < 6; i++)  // (reserved[0] is the rate)
    if (cfg->reserved[i]) FAIL(h, OFDM_E_INVAL, "ofdm_ldpc_cfg.reserved must be 0");
  *max_iters = cfg->max_iters;
  *rate = cfg->rate;
  return OFDM_OK;
}

// one instantiation per rate (ldpc_cfg_check has refused any other value)
static void ldpc_launch_encode(uint32_t rate, unsigned grid, hipStream_t st, const uint8_t* d_in, const LdpcBlk* blk, const uint32_t* cw,
                               uint32_t ncw, uint8_t* d_out, const uint32_t* crc, const uint32_t* xp8) {
#define LDPC_ENC(R) \
  case R: hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ldpc_encode<R>), dim3(grid), dim3(LDPC_THREADS), 0, st, d_in, blk, cw, ncw, d_out, crc, xp8); break
  switch (rate) {
    LDPC_ENC(OFDM_LDPC_RATE_1_2);
    LDPC_ENC(OFDM_LDPC_RATE_2_3);
    LDPC_ENC(OFDM_LDPC_RATE_3_4);
    LDPC_ENC(OFDM_LDPC_RATE_5_6);
  }
#undef LDPC_ENC
}
// k_ldpc_decode, or with REL k_ldpc_decode_rel and the reliabilities to d_rel
template <bool SOFT, bool REL>
static void ldpc_launch_decode(uint32_t rate, unsigned grid, hipStream_t st, const uint8_t* d_in, const LdpcBlk* blk, const uint32_t* cw,
                               uint32_t ncw, uint8_t* d_out, uint8_t* d_rel, LdpcRes* res, const uint32_t* crc, const uint32_t* xp8,
                               uint32_t max_iters) {
#define LDPC_DEC(R)                                                                                                                      \
  case R:                                                                                                                                \
    if constexpr (REL)                                                                                                                   \
      hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ldpc_decode_rel<SOFT, R>), dim3(grid), dim3(LDPC_THREADS), 0, st, d_in, blk, cw, ncw, d_out,  \
                         d_rel, res, crc, xp8, max_iters);                                                                               \
    else                                                                                                                                 \
      hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ldpc_decode<SOFT, R>), dim3(grid), dim3(LDPC_THREADS), 0, st, d_in, blk, cw, ncw, d_out, res, \
                         crc, xp8, max_iters);                                                                                           \
    break
  switch (rate) {
    LDPC_DEC(OFDM_LDPC_RATE_1_2);
    LDPC_DEC(OFDM_LDPC_RATE_2_3);
    LDPC_DEC(OFDM_LDPC_RATE_3_4);
    LDPC_DEC(OFDM_LDPC_RATE_5_6);
  }
#undef LDPC_DEC
}

/* payloads in, coded blocks out: what ofdm_tx / ofdm_make_packets then take as payloads */
extern "C" int ofdm_ldpc_encode(ofdm_handle* h, const ofdm_ldpc_cfg* cfg, const uint8_t* payloads, const uint64_t* payload_off,
                                const uint32_t* payload_len, int nblk, uint8_t* coded, uint64_t coded_cap, uint64_t* coded_off) {
  if (!h) return OFDM_E_INVAL;
  LdpcState& f = h->ldpc;
  if (nblk < 0 || (nblk && (!payloads || !payload_off || !payload_len)) || !coded_off) FAIL(h, OFDM_E_INVAL, "null argument");
  uint32_t iters, rate;
  RCCHK(ldpc_cfg_check(h, cfg, &iters, &rate));
  f.blk.resize((size_t)nblk);
  f.cw.resize((size_t)nblk * LDPC_MAX_WORDS);
  uint64_t ncw = 0, extent = 0;
  const uint64_t total =
      ldpc_plan_encode_rate(rate, payload_off, payload_len, (uint64_t)nblk, f.blk.data(), coded_off, f.cw.data(), &ncw, &extent);
  if (total == ~0ull) FAIL(h, OFDM_E_INVAL, "ldpc: len(payload) must be in [0, 2012] (2684, 3020, 3356 at rates 2/3, 3/4, 5/6)");
  f.timed = false;
  if (total > coded_cap) FAIL(h, OFDM_E_CAPACITY, "coded buffer too small (see ofdm_ldpc_coded_len)");
  if (nblk == 0) return OFDM_OK;
  if (!coded) FAIL(h, OFDM_E_INVAL, "null argument");
  hipStream_t st;
  RCCHK(codec_begin_encode(h, &st));
  const uint8_t* d_in;
  uint8_t* d_out;
  RCCHK(codec_upload(h, st, f.d_blk, f.blk, (size_t)nblk));  // the batch's two tables: blocks, and the block of every codeword
  RCCHK(codec_upload(h, st, f.d_cw, f.cw, (size_t)ncw));
  RCCHK(codec_stage_in(h, st, f.d_in, payloads, extent, false, &d_in));
  RCCHK(codec_stage_out(h, f.d_out, coded, total, &d_out));
  const bool timing = h->prof.on;
  RCCHK(codec_time_begin(h, f, st, timing));
  const unsigned grid = (unsigned)((ncw + LDPC_WAVES - 1) / LDPC_WAVES);  // every block has a codeword: ncw >= nblk >= 1
  ldpc_launch_encode(rate, grid, st, d_in, f.d_blk.as<LdpcBlk>(), f.d_cw.as<uint32_t>(), (uint32_t)ncw, d_out, h->d_crc.as<uint32_t>(),
                     h->d_xp8.as<uint32_t>());
  RCCHK(codec_launched(h, f, st, timing));
  RCCHK(codec_read_out(h, st, coded, d_out, total));
  return codec_finish(h, f, st, timing);
}

static void ldpc_no_blocks(int nblk, uint8_t* ok, uint32_t* corrected, uint8_t* iters, uint32_t* cw_failed) {
  memset(ok, 0, (size_t)nblk);
  memset(iters, 0, (size_t)nblk);
  memset(corrected, 0, sizeof(uint32_t) * (size_t)nblk);
  memset(cw_failed, 0, sizeof(uint32_t) * (size_t)nblk);
}

// REL: k_ldpc_decode_rel in k_ldpc_decode's place, one reliability byte per payload byte to `rel` at the payloads' offsets
// (NULL, 0 without).  in_on_device: the input blob is device memory whatever the handle's pointer mode (the handle's own
// soft values: ofdm_rx_ldpc_decode_soft)
template <bool SOFT, bool REL>
static int ldpc_decode_impl(ofdm_handle* h, const ofdm_ldpc_cfg* cfg, const uint8_t* in, const uint64_t* in_off, const uint32_t* coded_len,
                            int nblk, uint8_t* payloads, uint64_t payload_cap, uint64_t* payload_off, uint8_t* ok, uint32_t* corrected,
                            uint8_t* iters, uint32_t* cw_failed, uint8_t* rel, uint64_t rel_cap, bool in_on_device = false) {
  if (!h) return OFDM_E_INVAL;
  LdpcState& f = h->ldpc;
  if (nblk < 0 || (nblk && (!in || !in_off || !coded_len || !ok || !corrected || !iters || !cw_failed)) || !payload_off || (REL && !rel))
    FAIL(h, OFDM_E_INVAL, "null argument");
  uint32_t max_iters, rate;
  RCCHK(ldpc_cfg_check(h, cfg, &max_iters, &rate));
  f.blk.resize((size_t)nblk);
  f.cw.resize((size_t)nblk * LDPC_MAX_WORDS);
  uint64_t ncw = 0, extent = 0;
  const uint64_t total =
      ldpc_plan_decode_rate(rate, in_off, coded_len, (uint64_t)nblk, SOFT ? 8u : 1u, f.blk.data(), payload_off, f.cw.data(), &ncw, &extent);
  f.timed = false;
  if (total > payload_cap) FAIL(h, OFDM_E_CAPACITY, "payload buffer too small (see ofdm_ldpc_payload_len)");
  if (REL && total > rel_cap) FAIL(h, OFDM_E_CAPACITY, "reliability buffer too small (one byte per payload byte)");
  if (nblk == 0) return OFDM_OK;
  if (total && !payloads) FAIL(h, OFDM_E_INVAL, "null argument");
  if (ncw == 0) {  // not one block among them: nothing to launch
    ldpc_no_blocks(nblk, ok, corrected, iters, cw_failed);
    return OFDM_OK;
  }
  hipStream_t st;
  RCCHK(codec_begin_decode(h, &st));
  const uint8_t* d_in;
  uint8_t *d_out, *d_rel = nullptr;
  RCCHK(codec_upload(h, st, f.d_blk, f.blk, (size_t)nblk));
  RCCHK(codec_upload(h, st, f.d_cw, f.cw, (size_t)ncw));
  HIPCHK(h, f.d_res.ensure(sizeof(LdpcRes) * (size_t)nblk));
  HIPCHK(h, hipMemsetAsync(f.d_res.p, 0, sizeof(LdpcRes) * (size_t)nblk, st));
  RCCHK(codec_stage_in(h, st, f.d_in, in, extent, in_on_device, &d_in));
  RCCHK(codec_stage_out(h, f.d_out, payloads, total, &d_out));
  if (REL) RCCHK(codec_stage_out(h, f.d_rel, rel, total, &d_rel));
  const bool timing = h->prof.on;
  RCCHK(codec_time_begin(h, f, st, timing));
  const unsigned grid = (unsigned)((ncw + LDPC_WAVES - 1) / LDPC_WAVES);
  ldpc_launch_decode<SOFT, REL>(rate, grid, st, d_in, f.d_blk.as<LdpcBlk>(), f.d_cw.as<uint32_t>(), (uint32_t)ncw, d_out, d_rel,
                                f.d_res.as<LdpcRes>(), h->d_crc.as<uint32_t>(), h->d_xp8.as<uint32_t>(), max_iters);
  RCCHK(codec_launched(h, f, st, timing));
  f.res.resize((size_t)nblk);
  RCCHK(codec_read(h, st, f.res.data(), f.d_res, nblk));
  RCCHK(codec_read_out(h, st, payloads, d_out, total));
  if (REL) RCCHK(codec_read_out(h, st, rel, d_rel, total));
  RCCHK(codec_finish(h, f, st, timing));
  for (int b = 0; b < nblk; b++) {  // a length that is no block had no codeword: its record is still zero
    const LdpcRes& r = f.res[(size_t)b];
    ok[b] = (ldpc_is_block_rate(rate, coded_len[b]) && r.crc == r.got) ? 1 : 0;
    corrected[b] = r.corrected;
    iters[b] = (uint8_t)r.iters;
    cw_failed[b] = r.failed;
  }
  return OFDM_OK;
}

/* hard bytes in; payloads, ok[], corrected[], iters[] and cw_failed[] out */
extern "C" int ofdm_ldpc_decode(ofdm_handle* h, const ofdm_ldpc_cfg* cfg, const uint8_t* coded, const uint64_t* coded_off,
                                const uint32_t* coded_len, int nblk, uint8_t* payloads, uint64_t payload_cap, uint64_t* payload_off,
                                uint8_t* ok, uint32_t* corrected, uint8_t* iters, uint32_t* cw_failed) {
  return ldpc_decode_impl<false, false>(h, cfg, coded, coded_off, coded_len, nblk, payloads, payload_cap, payload_off, ok, corrected,
                                        iters, cw_failed, nullptr, 0);
}

/* the same from int8 values, 8 per coded byte */
extern "C" int ofdm_ldpc_decode_soft(ofdm_handle* h, const ofdm_ldpc_cfg* cfg, const int8_t* soft, const uint64_t* soft_off,
                                     const uint32_t* coded_len, int nblk, uint8_t* payloads, uint64_t payload_cap,
                                     uint64_t* payload_off, uint8_t* ok, uint32_t* corrected, uint8_t* iters, uint32_t* cw_failed) {
  return ldpc_decode_impl<true, false>(h, cfg, reinterpret_cast<const uint8_t*>(soft), soft_off, coded_len, nblk, payloads, payload_cap,
                                       payload_off, ok, corrected, iters, cw_failed, nullptr, 0);
}

/* the last ofdm_rx call's packets, decoded from the handle's own soft values */
extern "C" int ofdm_rx_ldpc_decode_soft(ofdm_handle* h, const ofdm_ldpc_cfg* cfg, uint8_t* payloads, uint64_t payload_cap,
                                        uint64_t* payload_off, uint8_t* ok, uint32_t* corrected, uint8_t* iters, uint32_t* cw_failed,
                                        int max_pkts, int* n) {
  if (!h) return OFDM_E_INVAL;
  RCCHK(codec_rx_soft_batch(h, max_pkts, n, "ok / corrected / iters / cw_failed / payload_off arrays too small"));
  const RxState& rx = h->rx;
  return ldpc_decode_impl<true, false>(h, cfg, rx.soft_vals.as<uint8_t>(), rx.soft_off.data(), rx.soft_len.data(), *n, payloads,
                                       payload_cap, payload_off, ok, corrected, iters, cw_failed, nullptr, 0, true);
}

/* ofdm_ldpc_decode with one reliability byte per payload byte */
extern "C" int ofdm_ldpc_decode_rel(ofdm_handle* h, const ofdm_ldpc_cfg* cfg, const uint8_t* coded, const uint64_t* coded_off,
                                    const uint32_t* coded_len, int nblk, uint8_t* payloads, uint64_t payload_cap, uint64_t* payload_off,
                                    uint8_t* ok, uint32_t* corrected, uint8_t* iters, uint32_t* cw_failed, uint8_t* rel, uint64_t rel_cap) {
  return ldpc_decode_impl<false, true>(h, cfg, coded, coded_off, coded_len, nblk, payloads, payload_cap, payload_off, ok, corrected,
                                       iters, cw_failed, rel, rel_cap);
}

/* ofdm_ldpc_decode_soft with one reliability byte per payload byte */
extern "C" int ofdm_ldpc_decode_soft_rel(ofdm_handle* h, const ofdm_ldpc_cfg* cfg, const int8_t* soft, const uint64_t* soft_off,
                                         const uint32_t* coded_len, int nblk, uint8_t* payloads, uint64_t payload_cap,
                                         uint64_t* payload_off, uint8_t* ok, uint32_t* corrected, uint8_t* iters, uint32_t* cw_failed,
                                         uint8_t* rel, uint64_t rel_cap) {
  return ldpc_decode_impl<true, true>(h, cfg, reinterpret_cast<const uint8_t*>(soft), soft_off, coded_len, nblk, payloads, payload_cap,
                                      payload_off, ok, corrected, iters, cw_failed, rel, rel_cap);
}

/* ofdm_rx_ldpc_decode_soft with one reliability byte per payload byte */
extern "C" int ofdm_rx_ldpc_decode_soft_rel(ofdm_handle* h, const ofdm_ldpc_cfg* cfg, uint8_t* payloads, uint64_t payload_cap,
                                            uint64_t* payload_off, uint8_t* ok, uint32_t* corrected, uint8_t* iters, uint32_t* cw_failed,
                                            uint8_t* rel, uint64_t rel_cap, int max_pkts, int* n) {
  if (!h) return OFDM_E_INVAL;
  RCCHK(codec_rx_soft_batch(h, max_pkts, n, "ok / corrected / iters / cw_failed / payload_off arrays too small"));
  const RxState& rx = h->rx;
  return ldpc_decode_impl<true, true>(h, cfg, rx.soft_vals.as<uint8_t>(), rx.soft_off.data(), rx.soft_len.data(), *n, payloads,
                                      payload_cap, payload_off, ok, corrected, iters, cw_failed, rel, rel_cap, true);
}
