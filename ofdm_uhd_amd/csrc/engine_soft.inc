// engine_soft.inc -- host side of the soft-decision receive option (rx_soft.h): the setting and the accessors of the
// last call's values.  The decoder calls that read them where they lie (ofdm_rx_*_decode_soft*) are with their codecs,
// behind codec_rx_soft_batch (engine_codec.inc).  Included by engine.hip after engine_fec.inc; the stage itself
// (rx_soft_values) runs inside ofdm_rx: engine_rx.inc.  The arithmetic that needs no GPU is soft_plan.h.

extern "C" int ofdm_set_rx_soft(ofdm_handle* h, const ofdm_soft_cfg* cfg) {
  if (!h) return OFDM_E_INVAL;
  RxState& rx = h->rx;
  if (!cfg) {
    rx.soft_on = rx.soft_valid = rx.soft_timed = false;
    // the buffers live only while the option is on (the last call's values go with them); the workspaces it asked for
    // internally stay where the caller's own settings use them
    rx.soft_vals.release();
    if (!((h->tap_mask >> OFDM_TAP_RX_SINK) & 1u)) {
      rx.tap_sink.release();
      rx.tap_demapped.release();
    }
    if (!rx.csi_on) rx.csi_frame.release();
    return OFDM_OK;
  }
  if (cfg->struct_size != sizeof(ofdm_soft_cfg)) FAIL(h, OFDM_E_INVAL, "ofdm_soft_cfg.struct_size does not match this library");
  if (!(cfg->scale > 0.0f) || !std::isfinite(cfg->scale)) FAIL(h, OFDM_E_INVAL, "soft scale must be positive and finite");
  // the smallest squared distance between two constellation points, float32, the kernel's own expression
  const uint32_t arity = h->cfg.arity;
  float dmin2 = INFINITY;
  for (uint32_t a = 0; a < arity; a++)
    for (uint32_t b = 0; b < arity; b++) {
      if (a == b) continue;
      const float dr = h->cfg.constellation[a].re - h->cfg.constellation[b].re;
      const float di = h->cfg.constellation[a].im - h->cfg.constellation[b].im;
      const float d = dr * dr + di * di;
      if (d < dmin2) dmin2 = d;
    }
  if (!(dmin2 > 0.0f) || !std::isfinite(dmin2)) FAIL(h, OFDM_E_INVAL, "soft-decision receive needs distinct constellation points");
  rx.soft_scale = cfg->scale;
  rx.soft_dmin2 = dmin2;
  rx.soft_on = true;
  return OFDM_OK;
}

extern "C" int ofdm_rx_soft(ofdm_handle* h, int8_t* out, uint64_t cap, uint64_t* off, int* n) {
  if (!h) return OFDM_E_INVAL;
  if (!n) FAIL(h, OFDM_E_INVAL, "null argument");
  const RxState& rx = h->rx;
  if (!rx.soft_valid) FAIL(h, OFDM_E_INVAL, "the last ofdm_rx ran without soft values (ofdm_set_rx_soft)");
  const size_t np = rx.soft_len.size();
  *n = (int)np;
  if (off) memcpy(off, rx.soft_off.data(), (np + 1) * sizeof(uint64_t));
  const uint64_t total = rx.soft_off[np];
  if (!out || total == 0) return OFDM_OK;  // out == NULL: size query
  if (cap < total) FAIL(h, OFDM_E_CAPACITY, "soft value buffer too small");
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  HIPCHK(h, hipMemcpyAsync(out, rx.soft_vals.p, total, h->dev_ptrs ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return OFDM_OK;
}

extern "C" int ofdm_rx_soft_last_ms(ofdm_handle* h, double* ms) {
  if (!h || !ms || !h->rx.soft_timed) return OFDM_E_INVAL;
  RxState& rx = h->rx;
  float t = 0.f;
  HIPCHK(h, hipEventElapsedTime(&t, rx.soft_ev_a, rx.soft_ev_b));
  rx.soft_ms = (double)t;
  *ms = rx.soft_ms;
  return OFDM_OK;
}
