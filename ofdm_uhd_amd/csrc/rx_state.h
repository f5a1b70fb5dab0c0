// rx_state.h -- host state of the receive path: workspaces and what one ofdm_rx call leaves for the accessors.
#pragma once
#include "host_util.h"
#include "rx_demod.h"

// every device buffer of the receiver, named once: the members and release() both come from this list
#define RX_DEVBUFS(X)                                                                                                       \
  X(recs) X(x_stage) X(y) X(metric) X(presel) X(tile_B) X(tile_np) X(tile_first) X(tile_pieces) X(avg_in) X(cand_u)        \
  X(cand_P) X(counters) X(counts) X(offsets) X(partial) X(peaks) X(peak_P) X(angle) X(step) X(inc) X(Phi) X(K) X(nsym)     \
  X(sym_base) X(res) X(raw) X(invalid) X(chain_list) X(key) X(pos) X(out_payload) X(out_off) X(out_len) X(out_ok)          \
  X(out_pos) X(inc_acc) X(Phi_u) X(peaks2) X(peak_P2) X(fstep) X(pre_inv) X(stash_peaks) X(stash_P) X(tap_fft) X(tap_acq)  \
  X(tap_sink) X(tap_demapped) X(raw_tap) X(raw_lens) X(raw_pos) X(tap_sampler) X(tap_sigmix) X(tap_nco) X(qual_frame)      \
  X(qual_out) X(csi_frame) X(csi_rows) X(csi_part) X(csi_sum) X(run_rows) X(soft_vals)

struct RxState {
#define X(name) DevBuf name;
  RX_DEVBUFS(X)
#undef X
  uint64_t nsamples = 0, npeaks = 0, nframes = 0, j0 = 0, nsym_total = 0, raw_tap_bytes = 0;
  uint64_t run_slots = 0;  // OFDM_TAP_RX_RUN_AVG: piece slots of the last call (unwritten ones hold NaN)
  const c32* y_ptr = nullptr;  // chan_filt's output of the last call: rx.y, or the input itself (SYNC "fixed")
  // ofdm_rx_submit: the input stage of the next ofdm_rx call is already queued for this buffer
  bool sub_valid = false, in_event_at_end = false;
  bool front_done = false;  // the fused front end (filter + pre-selection) of the pending call has been queued
  bool sub_hold = false;  // a submitted input stage whose buffer stays in use until the end of the ofdm_rx that picks it up
  const void* sub_iq = nullptr;
  uint64_t sub_n = 0;
  const c32* sub_dx = nullptr;
  uint64_t origin = 0;  // index, in its capture, of the first sample of the ofdm_rx calls (ofdm_rx_set_origin)
  std::vector<uint64_t> last_pos;  // host copy: flag sample of every packet of the last call
  // chunked streams (ofdm_rx_set_flag_history): flags settled by earlier calls replace whatever this call
  // detects up to trust_after; the NCO line of the flag before them
  bool nco_ref_on = false;
  int64_t nco_ref_peak = 0, nco_trust_after = 0;
  uint64_t nco_ref_u = 0;
  double nco_ref_step = 0.0;
  std::vector<uint64_t> hist_flags;
  std::vector<double> hist_steps;
  std::vector<uint8_t> hist_swallowed;
  std::vector<uint8_t> last_swallowed;  // per flag of the last call: its frame was swallowed by an earlier packet
  // link quality (ofdm_set_rx_quality): on for the following calls; whether the last call ran with it, its records
  bool quality_on = false, quality_valid = false;
  std::vector<ofdm_pkt_quality> last_quality;
  // per-subcarrier channel state (ofdm_set_rx_csi): on for the following calls; whether the last call ran with it, its
  // packet count and CRC verdicts.  The rows themselves stay in csi_rows (device) until the next call.
  bool csi_on = false, csi_valid = false;
  uint64_t csi_n = 0, csi_rows_cap = 0;
  int csi_stride = 0;
  std::vector<uint8_t> csi_ok;
  // soft-decision receive (ofdm_set_rx_soft): on for the following calls; whether the last call ran with it, and where
  // its packets' values lie in soft_vals (device; intact until the next call): value offsets [n + 1], payload lengths [n]
  bool soft_on = false, soft_valid = false;
  float soft_scale = 32.0f, soft_dmin2 = 0.0f;
  std::vector<uint64_t> soft_off;
  std::vector<uint32_t> soft_len;
  hipEvent_t soft_ev_a = nullptr, soft_ev_b = nullptr;
  double soft_ms = 0.0;
  bool soft_timed = false;  // soft_ms is of the last call's k_soft_demap
  void release() {
    if (soft_ev_a) (void)hipEventDestroy(soft_ev_a);
    if (soft_ev_b) (void)hipEventDestroy(soft_ev_b);
    soft_ev_a = soft_ev_b = nullptr;
#define X(name) name.release();
    RX_DEVBUFS(X)
#undef X
  }
};
