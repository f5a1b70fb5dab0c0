// engine_fec_rel.inc -- host side of the soft-output decoder (fec_rel.h): the batch layout, slicing and staging of
// engine_fec.inc's two decode paths (rate 1/2 and punctured) with k_fec_decode_rel in k_fec_decode's place and one
// reliability byte per payload byte next to the payloads.  Included by engine.hip after engine_soft.inc.

template <bool SOFT>
static void fec_rel_launch(ofdm_handle* h, hipStream_t st, unsigned nb, uint64_t b0, const uint8_t* d_in, uint8_t* d_out, uint8_t* d_rel,
                           uint64_t stride, uint32_t lgC) {
  FecState& f = h->fec;
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fec_decode_rel<SOFT>), dim3(nb), dim3(WAVE), 0, st, d_in, f.d_blk.as<FecBlk>() + b0, d_out, d_rel,
                     f.d_ok.as<uint8_t>() + b0, f.d_corr.as<uint32_t>() + b0, f.d_ws.as<uint64_t>(), h->fec_rel.d_ckpt.as<int>(), stride,
                     h->d_crc.as<uint32_t>(), h->d_xp8.as<uint32_t>(), lgC);
}

template <bool SOFT>
static int fec_decode_rel_impl(ofdm_handle* h, const ofdm_fec_cfg* cfg, const uint8_t* in, const uint64_t* in_off, const uint32_t* coded_len,
                               int nblk, uint8_t* payloads, uint64_t payload_cap, uint64_t* payload_off, uint8_t* ok, uint32_t* corrected,
                               uint8_t* rel, uint64_t rel_cap, bool in_on_device = false) {
  if (!h) return OFDM_E_INVAL;
  FecState& f = h->fec;
  FecPunctState& fp = h->fec_punct;
  FecRelState& fr = h->fec_rel;
  if (nblk < 0 || (nblk && (!in || !in_off || !coded_len || !ok || !corrected)) || !payload_off || !rel) FAIL(h, OFDM_E_INVAL, "null argument");
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
  if (total > rel_cap) FAIL(h, OFDM_E_CAPACITY, "reliability buffer too small (one byte per payload byte)");
  if (nblk == 0) return OFDM_OK;
  if (total && !payloads) FAIL(h, OFDM_E_INVAL, "null argument");
  if (stride == 0) {  // not one block among them: nothing to launch
    memset(ok, 0, (size_t)nblk);
    memset(corrected, 0, sizeof(uint32_t) * (size_t)nblk);
    return OFDM_OK;
  }
  // every block in flight owns `stride` decision words and as many checkpoint words; both are cut into the same slices
  const uint64_t per = fec_slice_blocks((uint64_t)nblk, stride, FEC_WS_MAX_BYTES);
  if (punct) punct_plan_decode_slots((uint64_t)nblk, per, mstride, payload_off, fp.pblk.data(), f.blk.data());
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  hipStream_t st = h->stream;  // the receive side: ordered behind the ofdm_rx that delivered the blocks
  if (h->tx_pending && h->txs != h->stream) HIPCHK(h, hipStreamWaitEvent(st, h->ev_tx_done, 0));
  const uint8_t* d_in = in;
  uint8_t *d_out = payloads, *d_rel = rel;
  const size_t tbytes = sizeof(FecBlk) * (size_t)nblk;
  HIPCHK(h, f.d_blk.ensure(tbytes));
  HIPCHK(h, hipMemcpyAsync(f.d_blk.p, f.blk.data(), tbytes, hipMemcpyHostToDevice, st));
  if (punct) {
    HIPCHK(h, fp.d_pblk.ensure(tbytes));
    HIPCHK(h, hipMemcpyAsync(fp.d_pblk.p, fp.pblk.data(), tbytes, hipMemcpyHostToDevice, st));
  }
  HIPCHK(h, f.d_ok.ensure((size_t)nblk));
  HIPCHK(h, f.d_corr.ensure(sizeof(uint32_t) * (size_t)nblk));
  if (!h->dev_ptrs) {
    if (!in_on_device) {
      HIPCHK(h, f.d_in.ensure(std::max<uint64_t>(extent, 1)));
      HIPCHK(h, hipMemcpyAsync(f.d_in.p, in, extent, hipMemcpyHostToDevice, st));
      d_in = f.d_in.as<uint8_t>();
    }
    HIPCHK(h, f.d_out.ensure(std::max<uint64_t>(total, 1)));
    HIPCHK(h, fr.d_rel.ensure(std::max<uint64_t>(total, 1)));
    d_out = f.d_out.as<uint8_t>();
    d_rel = fr.d_rel.as<uint8_t>();
  }
  HIPCHK(h, f.d_ws.ensure(per * stride * sizeof(uint64_t)));
  HIPCHK(h, fr.d_ckpt.ensure(per * stride * sizeof(int)));
  if (punct) HIPCHK(h, fp.d_mother.ensure(per * mstride));
  const bool timing = h->prof.on;
  const uint64_t nslices = ((uint64_t)nblk + per - 1) / per;
  if (timing) {  // three events per slice: depuncture | decoder
    while (fr.ev.size() < 3 * nslices) {
      hipEvent_t e = nullptr;
      HIPCHK(h, hipEventCreate(&e));
      fr.ev.push_back(e);
    }
  }
  uint64_t s = 0;
  for (uint64_t b0 = 0; b0 < (uint64_t)nblk; b0 += per, s++) {
    const unsigned nb = (unsigned)std::min<uint64_t>(per, (uint64_t)nblk - b0);
    if (punct) {
      const FecBlk* d_pblk = fp.d_pblk.as<FecBlk>() + b0;
      int8_t* d_mother = fp.d_mother.as<int8_t>();
      if (timing) HIPCHK(h, hipEventRecord(fr.ev[3 * s], st));
      switch (rate) {
        case OFDM_FEC_RATE_2_3: fec_launch_depuncture<OFDM_FEC_RATE_2_3, SOFT>(st, nb, d_in, d_pblk, d_mother, lgC); break;
        case OFDM_FEC_RATE_3_4: fec_launch_depuncture<OFDM_FEC_RATE_3_4, SOFT>(st, nb, d_in, d_pblk, d_mother, lgC); break;
        default: fec_launch_depuncture<OFDM_FEC_RATE_5_6, SOFT>(st, nb, d_in, d_pblk, d_mother, lgC); break;
      }
    }
    if (timing) HIPCHK(h, hipEventRecord(fr.ev[3 * s + 1], st));
    if (punct)  // the soft decoder on the mother values, coded order: one column
      fec_rel_launch<true>(h, st, nb, b0, fp.d_mother.as<uint8_t>(), d_out, d_rel, stride, 0u);
    else
      fec_rel_launch<SOFT>(h, st, nb, b0, d_in, d_out, d_rel, stride, lgC);
    if (timing) HIPCHK(h, hipEventRecord(fr.ev[3 * s + 2], st));
  }
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipMemcpyAsync(ok, f.d_ok.p, (size_t)nblk, hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipMemcpyAsync(corrected, f.d_corr.p, sizeof(uint32_t) * (size_t)nblk, hipMemcpyDeviceToHost, st));
  if (!h->dev_ptrs && total) {
    HIPCHK(h, hipMemcpyAsync(payloads, d_out, total, hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipMemcpyAsync(rel, d_rel, total, hipMemcpyDeviceToHost, st));
  }
  HIPCHK(h, hipStreamSynchronize(st));
  if (timing) {
    double dep = 0.0, dec = 0.0;
    for (uint64_t k = 0; k < nslices; k++) {
      float a = 0.f, b = 0.f;
      if (punct) HIPCHK(h, hipEventElapsedTime(&a, fr.ev[3 * k], fr.ev[3 * k + 1]));
      HIPCHK(h, hipEventElapsedTime(&b, fr.ev[3 * k + 1], fr.ev[3 * k + 2]));
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

/* ofdm_fec_decode with one reliability byte per payload byte */
extern "C" int ofdm_fec_decode_rel(ofdm_handle* h, const ofdm_fec_cfg* cfg, const uint8_t* coded, const uint64_t* coded_off,
                                   const uint32_t* coded_len, int nblk, uint8_t* payloads, uint64_t payload_cap, uint64_t* payload_off,
                                   uint8_t* ok, uint32_t* corrected, uint8_t* rel, uint64_t rel_cap) {
  return fec_decode_rel_impl<false>(h, cfg, coded, coded_off, coded_len, nblk, payloads, payload_cap, payload_off, ok, corrected, rel, rel_cap);
}

/* the same from int8 values, 8 per coded byte */
extern "C" int ofdm_fec_decode_soft_rel(ofdm_handle* h, const ofdm_fec_cfg* cfg, const int8_t* soft, const uint64_t* soft_off,
                                        const uint32_t* coded_len, int nblk, uint8_t* payloads, uint64_t payload_cap,
                                        uint64_t* payload_off, uint8_t* ok, uint32_t* corrected, uint8_t* rel, uint64_t rel_cap) {
  return fec_decode_rel_impl<true>(h, cfg, reinterpret_cast<const uint8_t*>(soft), soft_off, coded_len, nblk, payloads, payload_cap,
                                   payload_off, ok, corrected, rel, rel_cap);
}

/* the last ofdm_rx's packets, the values read where they lie */
extern "C" int ofdm_rx_fec_decode_soft_rel(ofdm_handle* h, const ofdm_fec_cfg* cfg, uint8_t* payloads, uint64_t payload_cap,
                                           uint64_t* payload_off, uint8_t* ok, uint32_t* corrected, uint8_t* rel, uint64_t rel_cap,
                                           int max_pkts, int* n) {
  if (!h) return OFDM_E_INVAL;
  if (!n || max_pkts < 0) FAIL(h, OFDM_E_INVAL, "null argument");
  RxState& rx = h->rx;
  if (!rx.soft_valid) FAIL(h, OFDM_E_INVAL, "the last ofdm_rx ran without soft values (ofdm_set_rx_soft)");
  const size_t np = rx.soft_len.size();
  *n = (int)np;
  if ((size_t)max_pkts < np) FAIL(h, OFDM_E_CAPACITY, "ok / corrected / payload_off arrays too small");
  return fec_decode_rel_impl<true>(h, cfg, rx.soft_vals.as<uint8_t>(), rx.soft_off.data(), rx.soft_len.data(), (int)np, payloads,
                                   payload_cap, payload_off, ok, corrected, rel, rel_cap, true);
}
