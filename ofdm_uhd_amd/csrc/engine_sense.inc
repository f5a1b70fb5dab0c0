// engine_sense.inc -- host side of the spectrum sensor (included by engine.hip):
// ofdm_sense_count / ofdm_sense / ofdm_set_rx_sense / ofdm_rx_sense_result.

static bool sense_cfg_ok(const ofdm_sense_cfg* sc) {
  if (!sc || sc->struct_size != sizeof(ofdm_sense_cfg)) return false;
  const uint32_t n = sc->fft_size;
  if (n < 64 || n > OFDM_SENSE_MAX_FFT || (n & (n - 1))) return false;
  if (sc->dwell_delay < 1 || sc->avg_msgs < 1) return false;
  return true;
}

extern "C" int ofdm_sense_count(const ofdm_sense_cfg* sc, uint64_t nsamples, uint64_t* nmsgs, uint64_t* ndecisions) {
  if (!sense_cfg_ok(sc)) return OFDM_E_INVAL;
  const uint64_t nvec = nsamples / sc->fft_size;
  const uint64_t nm = nvec / ((uint64_t)sc->tune_delay + sc->dwell_delay);
  if (nmsgs) *nmsgs = nm;
  if (ndecisions) *ndecisions = nm / ((uint64_t)sc->avg_msgs + sc->skip_msgs);
  return OFDM_OK;
}

static int sense_decide_enqueue(ofdm_handle* h, const ofdm_sense_cfg* sc, uint64_t nd, hipStream_t s);

template <int NS, typename XT>
static void sense_launch_t(SenseParams p, uint64_t nm, hipStream_t s) {
  if (sense_lds_bytes(NS) > 64 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_sense<NS, XT>), hipFuncAttributeMaxDynamicSharedMemorySize, sense_lds_bytes(NS));
  for (uint64_t m0 = 0; m0 < nm; m0 += 65535) {
    p.msg0 = m0;
    const unsigned ny = (unsigned)std::min<uint64_t>(65535, nm - m0);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_sense<NS, XT>), dim3(p.nsplit, ny), dim3(sense_threads(NS)), sense_lds_bytes(NS), s, p);
  }
}
template <int NS>
static void sense_launch_n(SenseParams p, uint64_t nm, hipStream_t s, bool in16) {
  if (in16)
    sense_launch_t<NS, sc16>(p, nm, s);
  else
    sense_launch_t<NS, c32>(p, nm, s);
}

// enqueue the sensing kernels for `d_x` (samples in the handle's receive format) on stream `s`; results stay in h->sense buffers
static int sense_enqueue(ofdm_handle* h, const ofdm_sense_cfg* sc, const c32* d_x, uint64_t nsamples, hipStream_t s) {
  SenseState& ss = h->sense;
  const int S = (int)sc->fft_size;
  uint64_t nm = 0, nd = 0;
  (void)ofdm_sense_count(sc, nsamples, &nm, &nd);
  ss.nm = nm;
  ss.nd = nd;
  ss.S = S;
  if (nm == 0) return OFDM_OK;
  // tables: window taps as given, forward twiddles of this length
  if (ss.tab_S != S || memcmp(ss.tab_win.data(), sc->window, sizeof(float) * (size_t)S) != 0) {
    std::vector<c32> tw(S);
    for (int k = 0; k < S; k++) {
      double a = -2.0 * M_PI * (double)k / (double)S;
      tw[k] = c32{(float)cos(a), (float)sin(a)};
    }
    HIPCHK(h, hipStreamSynchronize(s));  // a previous call may still read the old tables
    HIPCHK(h, upload(ss.d_tw, tw.data(), tw.size()));
    HIPCHK(h, upload(ss.d_win, sc->window, (size_t)S));
    ss.tab_win.assign(sc->window, sc->window + S);
    ss.tab_S = S;
  }
  HIPCHK(h, ss.d_msgs.ensure(nm * S * sizeof(float)));
  HIPCHK(h, ss.d_mean.ensure(std::max<uint64_t>(nd, 1) * S * sizeof(double)));
  HIPCHK(h, ss.d_bits.ensure(std::max<uint64_t>(nd, 1) * S));
  HIPCHK(h, ss.d_hex.ensure(std::max<uint64_t>(nd, 1) * (S / 4)));
  HIPCHK(h, hipMemsetAsync(ss.d_msgs.p, 0, nm * S * sizeof(float), s));

  SenseParams p;
  p.x = d_x;
  p.xscale = h->rx_scale;
  const bool in16 = h->rx_fmt == OFDM_IQ_SC16;
  p.win = ss.d_win.as<float>();
  p.tw = ss.d_tw.as<c32>();
  p.msgs = ss.d_msgs.as<float>();
  p.tune_delay = sc->tune_delay;
  p.dwell_delay = sc->dwell_delay;
  // enough workgroups to fill 256 CUs a few times over, never more than the dwell offers
  const uint32_t G = (uint32_t)std::max(1, 256 / (S / 8));
  const uint32_t max_split = (sc->dwell_delay + G - 1) / G;
  uint32_t want = (uint32_t)((2048 + nm - 1) / nm);
  if (const char* e = getenv("OFDM_SENSE_SPLIT")) want = (uint32_t)std::max(1, atoi(e));  // tuning knob: workgroups per message
  p.nsplit = std::max(1u, std::min(max_split, want));
  h->prof.begin(OFDM_K_SENSE, s);
  switch (S) {
    case 64: sense_launch_n<64>(p, nm, s, in16); break;
    case 128: sense_launch_n<128>(p, nm, s, in16); break;
    case 256: sense_launch_n<256>(p, nm, s, in16); break;
    case 512: sense_launch_n<512>(p, nm, s, in16); break;
    case 1024: sense_launch_n<1024>(p, nm, s, in16); break;
    case 2048: sense_launch_n<2048>(p, nm, s, in16); break;
    default: sense_launch_n<4096>(p, nm, s, in16); break;
  }
  HIPCHK(h, hipGetLastError());
  if (nd > 0) {
    int rc = sense_decide_enqueue(h, sc, nd, s);
    if (rc != OFDM_OK) return rc;
  }
  h->prof.end(s);
  return OFDM_OK;
}

// copy the results of the last sense_enqueue to host memory (blocking on stream s)
static int sense_fetch(ofdm_handle* h, hipStream_t s, float* msgs, uint64_t msgs_cap, double* mean, uint8_t* bits, char* hex,
                       uint64_t dec_cap, uint64_t* nmsgs, uint64_t* ndecisions) {
  SenseState& ss = h->sense;
  if (nmsgs) *nmsgs = ss.nm;
  if (ndecisions) *ndecisions = ss.nd;
  if ((msgs && ss.nm > msgs_cap) || ((mean || bits || hex) && ss.nd > dec_cap))
    FAIL(h, OFDM_E_CAPACITY, "sensing output arrays too small");
  const uint64_t S = (uint64_t)ss.S;
  if (msgs && ss.nm) HIPCHK(h, hipMemcpyAsync(msgs, ss.d_msgs.p, ss.nm * S * sizeof(float), hipMemcpyDeviceToHost, s));
  if (mean && ss.nd) HIPCHK(h, hipMemcpyAsync(mean, ss.d_mean.p, ss.nd * S * sizeof(double), hipMemcpyDeviceToHost, s));
  if (bits && ss.nd) HIPCHK(h, hipMemcpyAsync(bits, ss.d_bits.p, ss.nd * S, hipMemcpyDeviceToHost, s));
  if (hex && ss.nd) HIPCHK(h, hipMemcpyAsync(hex, ss.d_hex.p, ss.nd * (S / 4), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  return OFDM_OK;
}

extern "C" int ofdm_sense(ofdm_handle* h, const ofdm_sense_cfg* sc, const ofdm_c32* iq, uint64_t nsamples, float* msgs,
                          uint64_t msgs_cap, double* mean_inorder, uint8_t* bits_inorder, char* hex, uint64_t dec_cap,
                          uint64_t* nmsgs, uint64_t* ndecisions) {
  if (!h) return OFDM_E_INVAL;
  if (!sense_cfg_ok(sc)) FAIL(h, OFDM_E_INVAL, "bad ofdm_sense_cfg (struct_size, fft_size 64..4096 pow2, dwell_delay>=1, avg_msgs>=1)");
  if (nsamples && !iq) FAIL(h, OFDM_E_INVAL, "null argument");
  if (h->rx_fmt == OFDM_IQ_SC16 && ((uintptr_t)iq & 3u)) FAIL(h, OFDM_E_INVAL, "ofdm_sc16 buffers must be 4-byte aligned");
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  const c32* d_x = reinterpret_cast<const c32*>(iq);
  uint64_t nm = 0;
  (void)ofdm_sense_count(sc, nsamples, &nm, nullptr);
  if (!h->dev_ptrs && nm) {
    // only whole message periods are ever read
    const uint64_t used = nm * ((uint64_t)sc->tune_delay + sc->dwell_delay) * sc->fft_size;
    HIPCHK(h, h->sense.x_stage.ensure(used * rx_ss(h)));
    HIPCHK(h, hipMemcpyAsync(h->sense.x_stage.p, iq, used * rx_ss(h), hipMemcpyHostToDevice, h->stream));
    d_x = h->sense.x_stage.as<c32>();
  }
  int rc = sense_enqueue(h, sc, d_x, nsamples, h->stream);
  if (rc != OFDM_OK) return rc;
  rc = sense_fetch(h, h->stream, msgs, msgs_cap, mean_inorder, bits_inorder, hex, dec_cap, nmsgs, ndecisions);
  h->prof.collect();
  return rc;
}

static int sense_decide_enqueue(ofdm_handle* h, const ofdm_sense_cfg* sc, uint64_t nd, hipStream_t s) {
  SenseState& ss = h->sense;
  SenseDecideParams q;
  q.msgs = ss.d_msgs.as<float>();
  q.mean = ss.d_mean.as<double>();
  q.bits = ss.d_bits.as<uint8_t>();
  q.hex = ss.d_hex.as<char>();
  q.S = sc->fft_size;
  q.avg_msgs = sc->avg_msgs;
  q.skip_msgs = sc->skip_msgs;
  q.threshold = sc->threshold;
  hipLaunchKernelGGL(k_sense_decide, dim3((unsigned)nd), dim3(256), 0, s, q);
  HIPCHK(h, hipGetLastError());
  return OFDM_OK;
}

extern "C" int ofdm_sense_decide(ofdm_handle* h, const ofdm_sense_cfg* sc, const float* msgs, uint64_t nmsgs,
                                 double* mean_inorder, uint8_t* bits_inorder, char* hex, uint64_t dec_cap,
                                 uint64_t* ndecisions) {
  if (!h) return OFDM_E_INVAL;
  if (!sense_cfg_ok(sc)) FAIL(h, OFDM_E_INVAL, "bad ofdm_sense_cfg (struct_size, fft_size 64..4096 pow2, dwell_delay>=1, avg_msgs>=1)");
  if (nmsgs && !msgs) FAIL(h, OFDM_E_INVAL, "null argument");
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  SenseState& ss = h->sense;
  const uint64_t S = sc->fft_size;
  const uint64_t nd = nmsgs / ((uint64_t)sc->avg_msgs + sc->skip_msgs);
  ss.S = (int)S;
  ss.nm = nmsgs;
  ss.nd = nd;
  if (nd > 0x7FFFFFFFull) FAIL(h, OFDM_E_CAPACITY, "too many decisions in one call");
  if (nd) {
    HIPCHK(h, ss.d_msgs.ensure(nmsgs * S * sizeof(float)));
    HIPCHK(h, ss.d_mean.ensure(nd * S * sizeof(double)));
    HIPCHK(h, ss.d_bits.ensure(nd * S));
    HIPCHK(h, ss.d_hex.ensure(nd * (S / 4)));
    HIPCHK(h, hipMemcpyAsync(ss.d_msgs.p, msgs, nmsgs * S * sizeof(float), hipMemcpyHostToDevice, h->stream));
    int rc = sense_decide_enqueue(h, sc, nd, h->stream);
    if (rc != OFDM_OK) return rc;
  }
  return sense_fetch(h, h->stream, nullptr, 0, mean_inorder, bits_inorder, hex, dec_cap, nullptr, ndecisions);
}

extern "C" int ofdm_set_rx_sense(ofdm_handle* h, const ofdm_sense_cfg* sc) {
  if (!h) return OFDM_E_INVAL;
  if (!sc) {
    h->sense.rx_on = false;
    return OFDM_OK;
  }
  if (!sense_cfg_ok(sc)) FAIL(h, OFDM_E_INVAL, "bad ofdm_sense_cfg (struct_size, fft_size 64..4096 pow2, dwell_delay>=1, avg_msgs>=1)");
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  SenseState& ss = h->sense;
  if (!ss.side) {
    HIPCHK(h, hipStreamCreateWithFlags(&ss.side, hipStreamNonBlocking));
    HIPCHK(h, hipEventCreateWithFlags(&ss.ev_in, hipEventDisableTiming));
    HIPCHK(h, hipEventCreateWithFlags(&ss.ev_out, hipEventDisableTiming));
  }
  ss.rx_cfg = *sc;
  ss.rx_on = true;
  ss.nm = ss.nd = 0;
  return OFDM_OK;
}

extern "C" int ofdm_rx_sense_result(ofdm_handle* h, float* msgs, uint64_t msgs_cap, double* mean_inorder,
                                    uint8_t* bits_inorder, char* hex, uint64_t dec_cap, uint64_t* nmsgs,
                                    uint64_t* ndecisions) {
  if (!h) return OFDM_E_INVAL;
  if (!h->sense.rx_on) FAIL(h, OFDM_E_INVAL, "ofdm_set_rx_sense has not been called");
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  if (h->sense.ev_out) HIPCHK(h, hipStreamWaitEvent(h->stream, h->sense.ev_out, 0));
  return sense_fetch(h, h->stream, msgs, msgs_cap, mean_inorder, bits_inorder, hex, dec_cap, nmsgs, ndecisions);
}

extern "C" int ofdm_sense_device_msgs(ofdm_handle* h, void** d_msgs, uint64_t* nmsgs, uint32_t* fft_size) {
  if (!h) return OFDM_E_INVAL;
  if (!d_msgs) FAIL(h, OFDM_E_INVAL, "null argument");
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  SenseState& ss = h->sense;
  // the caller will touch the buffer from another stream: finish what produced it
  if (ss.side) HIPCHK(h, hipStreamSynchronize(ss.side));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  *d_msgs = ss.nm ? ss.d_msgs.p : nullptr;
  if (nmsgs) *nmsgs = ss.nm;
  if (fft_size) *fft_size = (uint32_t)ss.S;
  return OFDM_OK;
}

extern "C" int ofdm_sense_redecide(ofdm_handle* h, const ofdm_sense_cfg* sc) {
  if (!h) return OFDM_E_INVAL;
  if (!sense_cfg_ok(sc)) FAIL(h, OFDM_E_INVAL, "bad ofdm_sense_cfg");
  SenseState& ss = h->sense;
  if ((int)sc->fft_size != ss.S) FAIL(h, OFDM_E_INVAL, "fft_size differs from the run that produced the messages");
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  const uint64_t nd = ss.nm / ((uint64_t)sc->avg_msgs + sc->skip_msgs);
  if (nd > ss.nd) {
    HIPCHK(h, ss.d_mean.ensure(nd * sc->fft_size * sizeof(double)));
    HIPCHK(h, ss.d_bits.ensure(nd * sc->fft_size));
    HIPCHK(h, ss.d_hex.ensure(nd * (sc->fft_size / 4)));
  }
  ss.nd = nd;
  if (nd == 0) return OFDM_OK;
  return sense_decide_enqueue(h, sc, nd, h->stream);
}
