// engine_fec.inc -- host side of the coded-link layer (fec.h, fec_punct.h, fec_rel.h): lengths, batch layout, slicing,
// launches.  One encode call and one decode call over the steps of engine_codec.inc; the punctured rates put
// k_fec_puncture in the encoder's place and k_fec_depuncture in front of every decoder slice, the soft-output decoder
// k_fec_decode_rel in k_fec_decode's place and one reliability byte per payload byte next to the payloads.  Included by
// engine.hip after engine_codec.inc.  The arithmetic that needs no GPU is fec_plan.h and punct_plan.h.

extern "C" int ofdm_fec_coded_len(uint32_t payload_len, uint32_t* coded_len) { return fec_coded_len(payload_len, coded_len); }
extern "C" int ofdm_fec_payload_len(uint32_t coded_len, uint32_t* payload_len) { return fec_payload_len(coded_len, payload_len); }

extern "C" int ofdm_fec_last_ms(const ofdm_handle* h, double* ms) { return h ? codec_last_ms(h->fec, ms) : OFDM_E_INVAL; }

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

template <uint32_t RATE>
static void fec_launch_puncture(hipStream_t st, unsigned nblk, const uint8_t* d_in, const FecBlk* d_blk, uint8_t* d_out, const uint32_t* crc,
                                const uint32_t* xp8, uint32_t lgC) {
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fec_puncture<RATE>), dim3(nblk), dim3(FEC_ENC_THREADS), 0, st, d_in, d_blk, d_out, crc, xp8, lgC);
}
template <uint32_t RATE, bool SOFT>
static void fec_launch_depuncture(hipStream_t st, unsigned nblk, const uint8_t* d_in, const FecBlk* d_blk, int8_t* d_mother, uint32_t lgC) {
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fec_depuncture<RATE, SOFT>), dim3(nblk), dim3(FEC_DEPUNCT_THREADS), 0, st, d_in, d_blk, d_mother, lgC);
}

/* payloads in, coded blocks out: what ofdm_tx / ofdm_make_packets then take as payloads */
extern "C" int ofdm_fec_encode(ofdm_handle* h, const ofdm_fec_cfg* cfg, const uint8_t* payloads, const uint64_t* payload_off,
                               const uint32_t* payload_len, int nblk, uint8_t* coded, uint64_t coded_cap, uint64_t* coded_off) {
  if (!h) return OFDM_E_INVAL;
  FecState& f = h->fec;
  FecPunctState& fp = h->fec_punct;
  if (nblk < 0 || (nblk && (!payloads || !payload_off || !payload_len)) || !coded_off) FAIL(h, OFDM_E_INVAL, "null argument");
  uint32_t lgC, rate;
  RCCHK(fec_cols(h, cfg, &lgC));
  RCCHK(fec_rate(h, cfg, &rate));
  f.blk.resize((size_t)nblk);
  uint64_t extent = 0;
  const uint64_t total = punct_plan_encode(rate, payload_off, payload_len, (uint64_t)nblk, f.blk.data(), coded_off, &extent);
  if (total == ~0ull) FAIL(h, OFDM_E_INVAL, "fec: len(payload) must be in [0, 2040]");
  f.timed = false;
  if (total > coded_cap) FAIL(h, OFDM_E_CAPACITY, "coded buffer too small (see ofdm_fec_coded_len_rate)");
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
  const FecBlk* d_blk = f.d_blk.as<FecBlk>();
  const uint32_t *crc = h->d_crc.as<uint32_t>(), *xp8 = h->d_xp8.as<uint32_t>();
  switch (rate) {
    case OFDM_FEC_RATE_1_2:
      hipLaunchKernelGGL(k_fec_encode, dim3((unsigned)nblk), dim3(FEC_ENC_THREADS), 0, st, d_in, d_blk, d_out, crc, xp8, lgC);
      break;
    case OFDM_FEC_RATE_2_3: fec_launch_puncture<OFDM_FEC_RATE_2_3>(st, (unsigned)nblk, d_in, d_blk, d_out, crc, xp8, lgC); break;
    case OFDM_FEC_RATE_3_4: fec_launch_puncture<OFDM_FEC_RATE_3_4>(st, (unsigned)nblk, d_in, d_blk, d_out, crc, xp8, lgC); break;
    default: fec_launch_puncture<OFDM_FEC_RATE_5_6>(st, (unsigned)nblk, d_in, d_blk, d_out, crc, xp8, lgC); break;
  }
  RCCHK(codec_launched(h, f, st, timing));
  RCCHK(codec_read_out(h, st, coded, d_out, total));
  RCCHK(codec_finish(h, f, st, timing));
  if (timing && rate != OFDM_FEC_RATE_1_2) {  // k_fec_puncture is this call's encoder and its only kernel
    fp.last_ms = f.last_ms;
    fp.timed = true;
  }
  return OFDM_OK;
}

// one slice's decoder: k_fec_decode, or k_fec_decode_rel with its checkpoints and the reliabilities out
template <bool SOFT, bool REL>
static void fec_launch_decode(ofdm_handle* h, hipStream_t st, unsigned nb, uint64_t b0, const uint8_t* d_in, uint8_t* d_out, uint8_t* d_rel,
                              uint64_t stride, uint32_t lgC) {
  FecState& f = h->fec;
  if constexpr (REL)
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fec_decode_rel<SOFT>), dim3(nb), dim3(WAVE), 0, st, d_in, f.d_blk.as<FecBlk>() + b0, d_out, d_rel,
                       f.d_ok.as<uint8_t>() + b0, f.d_corr.as<uint32_t>() + b0, f.d_ws.as<uint64_t>(), h->fec_rel.d_ckpt.as<int>(), stride,
                       h->d_crc.as<uint32_t>(), h->d_xp8.as<uint32_t>(), lgC);
  else
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fec_decode<SOFT>), dim3(nb), dim3(WAVE), 0, st, d_in, f.d_blk.as<FecBlk>() + b0, d_out,
                       f.d_ok.as<uint8_t>() + b0, f.d_corr.as<uint32_t>() + b0, f.d_ws.as<uint64_t>(), stride, h->d_crc.as<uint32_t>(),
                       h->d_xp8.as<uint32_t>(), lgC);
}

// The decode call, every rate.  SOFT: int8 values in, 8 per coded byte, where hard bytes are 1 item per byte.  REL: the
// soft-output decoder, one reliability byte per payload byte to `rel` (NULL, 0 without).  in_on_device: the input blob
// is device memory whatever the handle's pointer mode (the handle's own soft values: ofdm_rx_fec_decode_soft*).
template <bool SOFT, bool REL>
static int fec_decode_impl(ofdm_handle* h, const ofdm_fec_cfg* cfg, const uint8_t* in, const uint64_t* in_off, const uint32_t* coded_len,
                           int nblk, uint8_t* payloads, uint64_t payload_cap, uint64_t* payload_off, uint8_t* ok, uint32_t* corrected,
                           uint8_t* rel, uint64_t rel_cap, bool in_on_device = false) {
  if (!h) return OFDM_E_INVAL;
  FecState& f = h->fec;
  FecPunctState& fp = h->fec_punct;
  FecRelState& fr = h->fec_rel;
  if (nblk < 0 || (nblk && (!in || !in_off || !coded_len || !ok || !corrected)) || !payload_off || (REL && !rel))
    FAIL(h, OFDM_E_INVAL, "null argument");
  uint32_t lgC, rate;
  RCCHK(fec_cols(h, cfg, &lgC));
  RCCHK(fec_rate(h, cfg, &rate));
  const bool punct = rate != OFDM_FEC_RATE_1_2;
  f.blk.resize((size_t)nblk);
  uint64_t stride = 0, mstride = 0, extent = 0, total;
  if (punct) {
    fp.pblk.resize((size_t)nblk);
    total = punct_plan_decode_sizes(rate, in_off, coded_len, (uint64_t)nblk, SOFT ? 8u : 1u, fp.pblk.data(), payload_off, &stride, &mstride,
                                    &extent);
  } else {
    total = fec_plan_decode(in_off, coded_len, (uint64_t)nblk, SOFT ? 8u : 1u, f.blk.data(), payload_off, &stride, &extent);
  }
  f.timed = false;
  if (total > payload_cap) FAIL(h, OFDM_E_CAPACITY, "payload buffer too small (see ofdm_fec_payload_len_rate)");
  if (REL && total > rel_cap) FAIL(h, OFDM_E_CAPACITY, "reliability buffer too small (one byte per payload byte)");
  if (nblk == 0) return OFDM_OK;
  if (total && !payloads) FAIL(h, OFDM_E_INVAL, "null argument");
  if (stride == 0) {  // not one block among them: nothing to launch
    memset(ok, 0, (size_t)nblk);
    memset(corrected, 0, sizeof(uint32_t) * (size_t)nblk);
    return OFDM_OK;
  }
  // every block in flight owns `stride` decision words (and as many checkpoint words); the workspace is bounded, a
  // larger batch goes in slices.  The mother values of a punctured rate are cut like it: a slice's blocks own `mstride`
  // values each, and the next slice writes over them behind this slice's decoder (stream order)
  const uint64_t per = fec_slice_blocks((uint64_t)nblk, stride, FEC_WS_MAX_BYTES);
  if (punct) punct_plan_decode_slots((uint64_t)nblk, per, mstride, payload_off, fp.pblk.data(), f.blk.data());
  hipStream_t st;
  RCCHK(codec_begin_decode(h, &st));
  const uint8_t* d_in;
  uint8_t *d_out, *d_rel = nullptr;
  RCCHK(codec_upload(h, st, f.d_blk, f.blk, (size_t)nblk));
  if (punct) RCCHK(codec_upload(h, st, fp.d_pblk, fp.pblk, (size_t)nblk));
  HIPCHK(h, f.d_ok.ensure((size_t)nblk));
  HIPCHK(h, f.d_corr.ensure(sizeof(uint32_t) * (size_t)nblk));
  RCCHK(codec_stage_in(h, st, f.d_in, in, extent, in_on_device, &d_in));
  RCCHK(codec_stage_out(h, f.d_out, payloads, total, &d_out));
  HIPCHK(h, f.d_ws.ensure(per * stride * sizeof(uint64_t)));
  if (REL) {
    RCCHK(codec_stage_out(h, fr.d_rel, rel, total, &d_rel));
    HIPCHK(h, fr.d_ckpt.ensure(per * stride * sizeof(int)));
  }
  if (punct) HIPCHK(h, fp.d_mother.ensure(per * mstride));
  const bool timing = h->prof.on;
  const uint64_t nslices = ((uint64_t)nblk + per - 1) / per;
  if (timing) {  // three events per slice: depuncture | decoder
    while (f.ev.size() < 3 * nslices) {
      hipEvent_t e = nullptr;
      HIPCHK(h, hipEventCreate(&e));
      f.ev.push_back(e);
    }
  }
  uint64_t s = 0;
  for (uint64_t b0 = 0; b0 < (uint64_t)nblk; b0 += per, s++) {
    const unsigned nb = (unsigned)std::min<uint64_t>(per, (uint64_t)nblk - b0);
    if (punct) {
      const FecBlk* d_pblk = fp.d_pblk.as<FecBlk>() + b0;
      int8_t* d_mother = fp.d_mother.as<int8_t>();
      if (timing) HIPCHK(h, hipEventRecord(f.ev[3 * s], st));
      switch (rate) {
        case OFDM_FEC_RATE_2_3: fec_launch_depuncture<OFDM_FEC_RATE_2_3, SOFT>(st, nb, d_in, d_pblk, d_mother, lgC); break;
        case OFDM_FEC_RATE_3_4: fec_launch_depuncture<OFDM_FEC_RATE_3_4, SOFT>(st, nb, d_in, d_pblk, d_mother, lgC); break;
        default: fec_launch_depuncture<OFDM_FEC_RATE_5_6, SOFT>(st, nb, d_in, d_pblk, d_mother, lgC); break;
      }
    }
    if (timing) HIPCHK(h, hipEventRecord(f.ev[3 * s + 1], st));
    if (punct)  // the soft decoder on the mother values, coded order: one column
      fec_launch_decode<true, REL>(h, st, nb, b0, fp.d_mother.as<uint8_t>(), d_out, d_rel, stride, 0u);
    else
      fec_launch_decode<SOFT, REL>(h, st, nb, b0, d_in, d_out, d_rel, stride, lgC);
    if (timing) HIPCHK(h, hipEventRecord(f.ev[3 * s + 2], st));
  }
  HIPCHK(h, hipGetLastError());
  RCCHK(codec_read(h, st, ok, f.d_ok, nblk));
  RCCHK(codec_read(h, st, corrected, f.d_corr, nblk));
  RCCHK(codec_read_out(h, st, payloads, d_out, total));
  if (REL) RCCHK(codec_read_out(h, st, rel, d_rel, total));
  HIPCHK(h, hipStreamSynchronize(st));
  if (timing) {  // the kernels' own time, slice by slice
    double dep = 0.0, dec = 0.0;
    for (uint64_t k = 0; k < nslices; k++) {
      float a = 0.f, b = 0.f;
      if (punct) HIPCHK(h, hipEventElapsedTime(&a, f.ev[3 * k], f.ev[3 * k + 1]));
      HIPCHK(h, hipEventElapsedTime(&b, f.ev[3 * k + 1], f.ev[3 * k + 2]));
      dep += (double)a;
      dec += (double)b;
    }
    if (punct) {
      fp.last_ms = dep;
      fp.timed = true;
    }
    f.last_ms = dec;
    f.timed = true;
  }
  return OFDM_OK;
}

/* hard bytes in; payloads, ok[] and corrected[] out */
extern "C" int ofdm_fec_decode(ofdm_handle* h, const ofdm_fec_cfg* cfg, const uint8_t* coded, const uint64_t* coded_off,
                               const uint32_t* coded_len, int nblk, uint8_t* payloads, uint64_t payload_cap, uint64_t* payload_off,
                               uint8_t* ok, uint32_t* corrected) {
  return fec_decode_impl<false, false>(h, cfg, coded, coded_off, coded_len, nblk, payloads, payload_cap, payload_off, ok, corrected, nullptr, 0);
}

/* the same from int8 values, 8 per coded byte */
extern "C" int ofdm_fec_decode_soft(ofdm_handle* h, const ofdm_fec_cfg* cfg, const int8_t* soft, const uint64_t* soft_off,
                                    const uint32_t* coded_len, int nblk, uint8_t* payloads, uint64_t payload_cap,
                                    uint64_t* payload_off, uint8_t* ok, uint32_t* corrected) {
  return fec_decode_impl<true, false>(h, cfg, reinterpret_cast<const uint8_t*>(soft), soft_off, coded_len, nblk, payloads, payload_cap,
                                      payload_off, ok, corrected, nullptr, 0);
}

/* ofdm_fec_decode with one reliability byte per payload byte */
extern "C" int ofdm_fec_decode_rel(ofdm_handle* h, const ofdm_fec_cfg* cfg, const uint8_t* coded, const uint64_t* coded_off,
                                   const uint32_t* coded_len, int nblk, uint8_t* payloads, uint64_t payload_cap, uint64_t* payload_off,
                                   uint8_t* ok, uint32_t* corrected, uint8_t* rel, uint64_t rel_cap) {
  return fec_decode_impl<false, true>(h, cfg, coded, coded_off, coded_len, nblk, payloads, payload_cap, payload_off, ok, corrected, rel,
                                      rel_cap);
}

/* the same from int8 values, 8 per coded byte */
extern "C" int ofdm_fec_decode_soft_rel(ofdm_handle* h, const ofdm_fec_cfg* cfg, const int8_t* soft, const uint64_t* soft_off,
                                        const uint32_t* coded_len, int nblk, uint8_t* payloads, uint64_t payload_cap,
                                        uint64_t* payload_off, uint8_t* ok, uint32_t* corrected, uint8_t* rel, uint64_t rel_cap) {
  return fec_decode_impl<true, true>(h, cfg, reinterpret_cast<const uint8_t*>(soft), soft_off, coded_len, nblk, payloads, payload_cap,
                                     payload_off, ok, corrected, rel, rel_cap);
}

/* the last ofdm_rx's packets, the values read where they lie */
extern "C" int ofdm_rx_fec_decode_soft(ofdm_handle* h, const ofdm_fec_cfg* cfg, uint8_t* payloads, uint64_t payload_cap,
                                       uint64_t* payload_off, uint8_t* ok, uint32_t* corrected, int max_pkts, int* n) {
  if (!h) return OFDM_E_INVAL;
  RCCHK(codec_rx_soft_batch(h, max_pkts, n, "ok / corrected / payload_off arrays too small"));
  const RxState& rx = h->rx;
  return fec_decode_impl<true, false>(h, cfg, rx.soft_vals.as<uint8_t>(), rx.soft_off.data(), rx.soft_len.data(), *n, payloads, payload_cap,
                                      payload_off, ok, corrected, nullptr, 0, true);
}

extern "C" int ofdm_rx_fec_decode_soft_rel(ofdm_handle* h, const ofdm_fec_cfg* cfg, uint8_t* payloads, uint64_t payload_cap,
                                           uint64_t* payload_off, uint8_t* ok, uint32_t* corrected, uint8_t* rel, uint64_t rel_cap,
                                           int max_pkts, int* n) {
  if (!h) return OFDM_E_INVAL;
  RCCHK(codec_rx_soft_batch(h, max_pkts, n, "ok / corrected / payload_off arrays too small"));
  const RxState& rx = h->rx;
  return fec_decode_impl<true, true>(h, cfg, rx.soft_vals.as<uint8_t>(), rx.soft_off.data(), rx.soft_len.data(), *n, payloads, payload_cap,
                                     payload_off, ok, corrected, rel, rel_cap, true);
}
