// engine_codec.inc -- what the host sides of the coded-link calls share (CodecStage, host_util.h): one function per step
// of the two call shapes, around a codec's own checks, plan call, launch and result post-processing:
//   encode (payloads in, blocks out, the transmit side):
//     [checks, plan, capacity], codec_begin_encode, codec_upload, codec_stage_in, codec_stage_out, codec_time_begin,
//     [launch], codec_launched, codec_read_out, codec_finish
//   decode (blocks in; payloads and per-block arrays out, the receive side):
//     [checks, plan, capacity, "not one block"], codec_begin_decode, codec_upload, codec_stage_in, codec_stage_out,
//     codec_time_begin, [launch], codec_launched, codec_read per array, codec_read_out, codec_finish
// A staging step leaves the caller's pointers (device mode) as they are and, in host mode, puts the codec's device copy
// in their place.  Included by engine.hip ahead of engine_{fec,soft,rs,ldpc}.inc.

static int codec_last_ms(const CodecClock& c, double* ms) {
  if (!ms || !c.timed) return OFDM_E_INVAL;
  *ms = c.last_ms;
  return OFDM_OK;
}

// the transmit side: ordered with the ofdm_fec_encode / ofdm_tx that takes the blocks
static int codec_begin_encode(ofdm_handle* h, hipStream_t* st) {
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  *st = h->txs;
  return OFDM_OK;
}

// the receive side: ordered behind the ofdm_rx / inner decoder that delivered the blocks
static int codec_begin_decode(ofdm_handle* h, hipStream_t* st) {
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  *st = h->stream;
  if (h->tx_pending && h->txs != h->stream) HIPCHK(h, hipStreamWaitEvent(*st, h->ev_tx_done, 0));
  return OFDM_OK;
}

// the first n entries of a host table on the device
template <typename T>
static int codec_upload(ofdm_handle* h, hipStream_t st, DevBuf& d, const std::vector<T>& tab, size_t n) {
  HIPCHK(h, d.ensure(sizeof(T) * n));
  HIPCHK(h, hipMemcpyAsync(d.p, tab.data(), sizeof(T) * n, hipMemcpyHostToDevice, st));
  return OFDM_OK;
}

// in_on_device: the input is device memory whatever the handle's pointer mode (the handle's own soft values)
static int codec_stage_in(ofdm_handle* h, hipStream_t st, DevBuf& d, const void* in, uint64_t extent, bool in_on_device, const uint8_t** d_in) {
  *d_in = static_cast<const uint8_t*>(in);
  if (h->dev_ptrs || in_on_device) return OFDM_OK;
  HIPCHK(h, d.ensure(std::max<uint64_t>(extent, 1)));
  if (extent) HIPCHK(h, hipMemcpyAsync(d.p, in, extent, hipMemcpyHostToDevice, st));
  *d_in = d.as<uint8_t>();
  return OFDM_OK;
}

static int codec_stage_out(ofdm_handle* h, DevBuf& d, uint8_t* out, uint64_t total, uint8_t** d_out) {
  *d_out = out;
  if (h->dev_ptrs) return OFDM_OK;
  HIPCHK(h, d.ensure(std::max<uint64_t>(total, 1)));
  *d_out = d.as<uint8_t>();
  return OFDM_OK;
}

static int codec_time_begin(ofdm_handle* h, CodecClock& c, hipStream_t st, bool timing) {
  if (!timing) return OFDM_OK;
  if (!c.ev_a) {
    HIPCHK(h, hipEventCreate(&c.ev_a));
    HIPCHK(h, hipEventCreate(&c.ev_b));
  }
  HIPCHK(h, hipEventRecord(c.ev_a, st));
  return OFDM_OK;
}

static int codec_launched(ofdm_handle* h, CodecClock& c, hipStream_t st, bool timing) {
  if (timing) HIPCHK(h, hipEventRecord(c.ev_b, st));
  HIPCHK(h, hipGetLastError());
  return OFDM_OK;
}

// one per-block array of a decode call back to the caller (host memory in both pointer modes)
template <typename T>
static int codec_read(ofdm_handle* h, hipStream_t st, T* dst, const DevBuf& d, int nblk) {
  HIPCHK(h, hipMemcpyAsync(dst, d.p, sizeof(T) * (size_t)nblk, hipMemcpyDeviceToHost, st));
  return OFDM_OK;
}

// host mode: what codec_stage_out staged, back to the caller
static int codec_read_out(ofdm_handle* h, hipStream_t st, uint8_t* out, const uint8_t* d_out, uint64_t total) {
  if (!h->dev_ptrs && total) HIPCHK(h, hipMemcpyAsync(out, d_out, total, hipMemcpyDeviceToHost, st));
  return OFDM_OK;
}

// synchronises: the staged tables are the caller's again
static int codec_finish(ofdm_handle* h, CodecClock& c, hipStream_t st, bool timing) {
  HIPCHK(h, hipStreamSynchronize(st));
  if (timing) {
    float ms = 0.f;
    HIPCHK(h, hipEventElapsedTime(&ms, c.ev_a, c.ev_b));
    c.last_ms = (double)ms;
    c.timed = true;
  }
  return OFDM_OK;
}

// The ofdm_rx_*_decode_soft* calls, ahead of their decoder: the last ofdm_rx's packets are the batch, *n of them, their
// values read where they lie.  `too_small` names the arrays of max_pkts entries.
static int codec_rx_soft_batch(ofdm_handle* h, int max_pkts, int* n, const char* too_small) {
  if (!n || max_pkts < 0) FAIL(h, OFDM_E_INVAL, "null argument");
  if (!h->rx.soft_valid) FAIL(h, OFDM_E_INVAL, "the last ofdm_rx ran without soft values (ofdm_set_rx_soft)");
  const size_t np = h->rx.soft_len.size();
  *n = (int)np;
  if ((size_t)max_pkts < np) FAIL(h, OFDM_E_CAPACITY, too_small);
  return OFDM_OK;
}
