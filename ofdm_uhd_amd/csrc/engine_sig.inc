// engine_sig.inc -- host side of the signal field (sig.h): the word's fields, the offsets of a batch, launches, over the
// steps of engine_codec.inc.  Included by engine.hip after engine_ldpc.inc.  The arithmetic that needs no GPU is
// sig_plan.h.

extern "C" int ofdm_sig_word(uint32_t codec, uint32_t rate, uint32_t rs, uint32_t interleave_cols, uint16_t* word) {
  return word ? sig_word_pack(codec, rate, rs, interleave_cols, word) : OFDM_E_INVAL;
}
extern "C" int ofdm_sig_word_fields(uint32_t word, uint32_t* codec, uint32_t* rate, uint32_t* rs, uint32_t* interleave_cols) {
  return (codec && rate && rs && interleave_cols) ? sig_word_unpack(word, codec, rate, rs, interleave_cols) : OFDM_E_INVAL;
}
extern "C" int ofdm_sig_word_valid(uint32_t word) { return sig_word_valid(word) ? 1 : 0; }

extern "C" int ofdm_sig_last_ms(const ofdm_handle* h, double* ms) { return h ? codec_last_ms(h->sig, ms) : OFDM_E_INVAL; }

/* bodies in, blocks (field | body) out: what ofdm_tx / ofdm_make_packets then take as payloads */
extern "C" int ofdm_sig_encode(ofdm_handle* h, const uint16_t* words, const uint8_t* bodies, const uint64_t* body_off,
                               const uint32_t* body_len, int nblk, uint8_t* out, uint64_t out_cap, uint64_t* out_off) {
  if (!h) return OFDM_E_INVAL;
  SigState& f = h->sig;
  if (nblk < 0 || (nblk && (!words || !body_off || !body_len)) || !out_off) FAIL(h, OFDM_E_INVAL, "null argument");
  f.blk.resize((size_t)nblk);
  uint64_t extent = 0, bad = 0;
  const uint64_t total = sig_plan_encode(words, body_off, body_len, (uint64_t)nblk, f.blk.data(), out_off, &extent, &bad);
  f.timed = false;
  if (bad != (uint64_t)nblk) FAIL(h, OFDM_E_INVAL, "sig: not a valid coding word (ofdm_sig_word_valid)");
  if (total > out_cap) FAIL(h, OFDM_E_CAPACITY, "block buffer too small (12 bytes and the body per block)");
  if (nblk == 0) return OFDM_OK;
  if (!out || (extent && !bodies)) FAIL(h, OFDM_E_INVAL, "null argument");
  hipStream_t st;
  RCCHK(codec_begin_encode(h, &st));
  const uint8_t* d_in;
  uint8_t* d_out;
  RCCHK(codec_upload(h, st, f.d_blk, f.blk, (size_t)nblk));
  RCCHK(codec_stage_in(h, st, f.d_in, bodies, extent, false, &d_in));
  RCCHK(codec_stage_out(h, f.d_out, out, total, &d_out));
  const bool timing = h->prof.on;
  RCCHK(codec_time_begin(h, f, st, timing));
  const unsigned grid = (unsigned)(((uint64_t)nblk + SIG_WAVES - 1) / SIG_WAVES);
  hipLaunchKernelGGL(k_sig_encode, dim3(grid), dim3(SIG_THREADS), 0, st, d_in, f.d_blk.as<SigBlk>(), (uint32_t)nblk, d_out);
  RCCHK(codec_launched(h, f, st, timing));
  RCCHK(codec_read_out(h, st, out, d_out, total));
  return codec_finish(h, f, st, timing);
}

// in_on_device: the input blob is device memory whatever the handle's pointer mode (the handle's own soft values:
// ofdm_rx_sig_decode_soft)
template <bool SOFT>
static int sig_decode_impl(ofdm_handle* h, const uint8_t* in, const uint64_t* in_off, const uint32_t* len, int nblk, uint16_t* word,
                           uint16_t* margin, bool in_on_device = false) {
  if (!h) return OFDM_E_INVAL;
  SigState& f = h->sig;
  if (nblk < 0 || (nblk && (!in_off || !len || !word || !margin))) FAIL(h, OFDM_E_INVAL, "null argument");
  f.blk.resize((size_t)nblk);
  uint64_t extent = 0;
  const uint64_t fields = sig_plan_decode(in_off, len, (uint64_t)nblk, SOFT ? 8u : 1u, f.blk.data(), &extent);
  f.timed = false;
  if (nblk == 0) return OFDM_OK;
  if (fields == 0) {  // not one packet holds a field: nothing to launch
    for (int b = 0; b < nblk; b++) {
      word[b] = OFDM_SIG_NO_WORD;
      margin[b] = 0;
    }
    return OFDM_OK;
  }
  if (!in) FAIL(h, OFDM_E_INVAL, "null argument");
  hipStream_t st;
  RCCHK(codec_begin_decode(h, &st));
  const uint8_t* d_in;
  RCCHK(codec_upload(h, st, f.d_blk, f.blk, (size_t)nblk));
  HIPCHK(h, f.d_res.ensure(sizeof(uint32_t) * (size_t)nblk));
  RCCHK(codec_stage_in(h, st, f.d_in, in, extent, in_on_device, &d_in));
  const bool timing = h->prof.on;
  RCCHK(codec_time_begin(h, f, st, timing));
  const unsigned grid = (unsigned)(((uint64_t)nblk + SIG_WAVES - 1) / SIG_WAVES);
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_sig_decode<SOFT>), dim3(grid), dim3(SIG_THREADS), 0, st, d_in, f.d_blk.as<SigBlk>(), (uint32_t)nblk,
                     f.d_res.as<uint32_t>());
  RCCHK(codec_launched(h, f, st, timing));
  f.res.resize((size_t)nblk);
  RCCHK(codec_read(h, st, f.res.data(), f.d_res, nblk));
  RCCHK(codec_finish(h, f, st, timing));
  for (int b = 0; b < nblk; b++) {
    word[b] = (uint16_t)(f.res[(size_t)b] & 0xFFFFu);
    margin[b] = (uint16_t)(f.res[(size_t)b] >> 16);
  }
  return OFDM_OK;
}

/* hard bytes in; word[] and margin[] out */
extern "C" int ofdm_sig_decode(ofdm_handle* h, const uint8_t* in, const uint64_t* off, const uint32_t* len, int nblk, uint16_t* word,
                               uint16_t* margin) {
  return sig_decode_impl<false>(h, in, off, len, nblk, word, margin);
}

/* the same from int8 values, 8 per byte */
extern "C" int ofdm_sig_decode_soft(ofdm_handle* h, const int8_t* soft, const uint64_t* soft_off, const uint32_t* len, int nblk,
                                    uint16_t* word, uint16_t* margin) {
  return sig_decode_impl<true>(h, reinterpret_cast<const uint8_t*>(soft), soft_off, len, nblk, word, margin);
}

/* the last ofdm_rx call's packets, their fields decoded from the handle's own soft values */
extern "C" int ofdm_rx_sig_decode_soft(ofdm_handle* h, uint16_t* word, uint16_t* margin, int max_pkts, int* n) {
  if (!h) return OFDM_E_INVAL;
  RCCHK(codec_rx_soft_batch(h, max_pkts, n, "word / margin arrays too small"));
  const RxState& rx = h->rx;
  return sig_decode_impl<true>(h, rx.soft_vals.as<uint8_t>(), rx.soft_off.data(), rx.soft_len.data(), *n, word, margin, true);
}
