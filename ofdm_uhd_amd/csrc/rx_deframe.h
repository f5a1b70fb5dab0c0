// rx_deframe.h -- what follows the demodulator's optimistic pass.
//
//   k_chain_*   frames swallowed by an earlier, still unfinished packet are invalidated (see rx_demod.h, "chains").
//   k_deframe_* unmake_packet (ofdm_packet_utils.py:169-191): dewhiten, CRC-32 check, compaction of the (ok, payload)
//               pairs in stream order; k_quality_write and k_csi_* turn the kept frames' records into packet records.
//   taps        k_raw_*, k_nco_phase, k_sigmix_tap.
#pragma once
#include "rx_demod.h"

// ------------------------------------------------------------------------------------
// chain resolution: frames swallowed by an earlier, still unfinished packet are invalid
// ------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_chain_collect(const FrameResult* __restrict__ res, uint32_t nframes_s, DynFrames dyn,
                                                        uint32_t* __restrict__ list, uint32_t cap, unsigned int* count) {
  const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t nframes = dyn_nframes(dyn, nframes_s);
  if (f >= nframes) return;
  if (res[f].end_frame > f) {
    const unsigned int k = atomicAdd(count, 1u);
    if (k < cap) list[k] = f;
  }
}

// single thread: sort the (short) list of chain heads, walk it, mark swallowed frames
// `pre` (chunked streams): the first npre frames were settled by earlier calls -- pre[f] != 0 says frame f was
// swallowed by a packet that began before it (possibly before this call's first sample): it is invalid and is
// no chain head here either.
__global__ void k_chain_resolve(const FrameResult* __restrict__ res, uint32_t nframes_s, DynFrames dyn, uint32_t* __restrict__ list,
                                uint32_t cap, const unsigned int* __restrict__ count, uint8_t* __restrict__ invalid,
                                unsigned int* overflow, const uint8_t* __restrict__ pre, uint32_t npre) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const uint32_t nframes = dyn_nframes(dyn, nframes_s);
  for (uint32_t f = 0; f < npre && f < nframes; f++)
    if (pre[f]) invalid[f] = 1;
  unsigned int n = *count;
  if (n > cap) {
    // more chain heads than the list holds (a detector set to fire on noise): walk every frame in order instead
    int64_t cover = -1;
    for (uint32_t f = 0; f < nframes; f++) {
      if ((int64_t)f <= cover) continue;
      if (f < npre && pre[f]) continue;
      const uint32_t e = res[f].end_frame;
      if (e > f) {
        for (uint32_t g = f + 1; g <= e && g < nframes; g++) invalid[g] = 1;
        cover = (int64_t)e;
      }
    }
    return;
  }
  for (unsigned int i = 1; i < n; i++) {  // insertion sort
    const uint32_t v = list[i];
    int k = (int)i - 1;
    while (k >= 0 && list[k] > v) {
      list[k + 1] = list[k];
      k--;
    }
    list[k + 1] = v;
  }
  int64_t cover = -1;
  for (unsigned int i = 0; i < n; i++) {
    const uint32_t f = list[i];
    if ((int64_t)f <= cover) continue;  // itself swallowed: its optimistic result does not count
    if (f < npre && pre[f]) continue;   // swallowed by a packet of an earlier chunk
    const uint32_t e = res[f].end_frame;
    for (uint32_t g = f + 1; g <= e && g < nframes; g++) invalid[g] = 1;
    cover = (int64_t)e;
  }
}

// ------------------------------------------------------------------------------------
// unmake_packet
// ------------------------------------------------------------------------------------
struct DeframeParams {
  DynFrames dyn;
  uint32_t nframes;
  const FrameResult* res;
  const uint8_t* invalid;
  const uint8_t* raw;
  const uint8_t* mask;
  const uint32_t* crc_table;
  const uint32_t* xp8;  // [4097] x^(8k) mod P, reflected (crc32_combine operator for k following bytes)
  uint64_t* key;        // [nframes] (is_message << 40) | payload_bytes
  const uint64_t* pos;  // exclusive scan of key
  uint8_t* payload_out;
  uint64_t payload_cap;
  uint64_t* out_off;  // [max_pkts+1]
  uint32_t* out_len;  // [max_pkts]
  uint8_t* out_ok;    // [max_pkts]
  uint64_t* out_pos;  // [max_pkts] flag sample of the packet's preamble
  const uint64_t* peaks;  // flags of the stream; frame f belongs to peaks[j0 + f]
  uint32_t j0;
  uint32_t max_pkts;
  uint8_t* raw_tap;       // optional: concatenated messages before dewhitening
  uint64_t* counters;     // [0] headers_ok [1] packets [2] crc_ok [3] chained [4] capacity overflow
};

__global__ void __launch_bounds__(256) k_deframe_count(DeframeParams q) {
  const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= dyn_nframes(q.dyn, q.nframes)) {
    if (q.dyn.lo && f < q.dyn.npeaks) q.key[f] = 0;  // (the scan behind this kernel runs over the upper bound)
    return;
  }
  uint64_t key = 0;
  if (q.invalid[f]) {
    atomicAdd((unsigned long long*)&q.counters[3], 1ull);
  } else {
    const FrameResult r = q.res[f];
    if (r.header_ok) atomicAdd((unsigned long long*)&q.counters[0], 1ull);
    if (r.status == FR_COMPLETE) {
      const uint64_t plen = r.packetlen >= 4 ? r.packetlen - 4 : 0;
      key = (1ull << 40) | plen;
    }
  }
  q.key[f] = key;
}

// One WAVE per frame: coalesced 16-byte loads of the raw message, dewhitening, CRC-32 as 64 independent
// 16-byte CRCs per KiB combined with crc(A||B) = crc(A) * x^(8|B|) + crc(B)  (mod P), and dword-aligned
// coalesced stores of the payload through an LDS staging line.
__global__ void __launch_bounds__(256) k_deframe_write(DeframeParams q) {
  __shared__ uint32_t tab[256];
  __shared__ __align__(16) uint32_t stage_all[4][260];
  tab[threadIdx.x] = q.crc_table[threadIdx.x];
  __syncthreads();
  const int lane = lane_id(), w = wave_id();
  uint32_t* stage = stage_all[w];
  const uint32_t f = blockIdx.x * 4 + (uint32_t)w;
  if (f >= dyn_nframes(q.dyn, q.nframes)) return;
  if (q.invalid[f]) return;
  const FrameResult r = q.res[f];
  if (r.status != FR_COMPLETE) return;
  const uint64_t pos = q.pos[f];
  const uint64_t ord = pos >> 40, boff = pos & ((1ull << 40) - 1);
  const uint32_t len = r.packetlen;
  const uint32_t plen = len >= 4 ? len - 4 : 0;
  if (ord >= q.max_pkts || boff + plen > q.payload_cap) {
    if (lane == 0) atomicAdd((unsigned long long*)&q.counters[4], 1ull);
    return;
  }
  const uint8_t* msg = q.raw + (uint64_t)f * RAW_SLOT;
  const uint4* msg4 = reinterpret_cast<const uint4*>(msg);
  const uint4* mask4 = reinterpret_cast<const uint4*>(q.mask);
  uint8_t* out = q.payload_out + boff;
  uint32_t acc = 0;
  // dewhiten with offset 0 (ofdm.py:303 passes no offset) and check the CRC (crc.check_crc32)
  for (uint32_t c0 = 0; c0 < plen; c0 += 1024) {
    const uint32_t o = c0 + 16u * (uint32_t)lane;
    uint4 d = make_uint4(0, 0, 0, 0);
    if (o < plen) {
      const uint4 m = msg4[o >> 4], k = mask4[o >> 4];
      d = make_uint4(m.x ^ k.x, m.y ^ k.y, m.z ^ k.z, m.w ^ k.w);
      const uint32_t nb = (plen - o < 16u) ? (plen - o) : 16u;
      uint32_t crc = 0xFFFFFFFFu;
      const uint32_t wds[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
      for (int b = 0; b < 16; b++) {
        if ((uint32_t)b < nb) {
          const uint32_t byte = (wds[b >> 2] >> (8 * (b & 3))) & 0xFFu;
          crc = tab[(crc ^ byte) & 0xFF] ^ (crc >> 8);
        }
      }
      crc ^= 0xFFFFFFFFu;
      acc ^= crc_multmodp(q.xp8[plen - (o + nb)], crc);
    }
    // ---- payload bytes of this KiB to the output, dword-aligned ------------------------------
    reinterpret_cast<uint4*>(stage)[lane] = d;
    if (lane == 0) stage[256] = 0;
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): the staging line is written
    const uint32_t rem = (plen - c0 < 1024u) ? (plen - c0) : 1024u;
    uint8_t* og = out + c0;
    const uint32_t head0 = (4u - (uint32_t)((uintptr_t)og & 3u)) & 3u;
    const uint32_t head = head0 < rem ? head0 : rem;
    const uint32_t nd = (rem - head) >> 2;
    const uint8_t* st8 = reinterpret_cast<const uint8_t*>(stage);
    if ((uint32_t)lane < head) og[lane] = st8[lane];
    for (uint32_t dw = (uint32_t)lane; dw < nd; dw += WAVE) {
      const uint32_t i0 = head + 4u * dw;
      const uint32_t w0 = stage[i0 >> 2], w1 = stage[(i0 >> 2) + 1];
      reinterpret_cast<uint32_t*>(og + i0)[0] = __builtin_amdgcn_alignbyte(w1, w0, i0 & 3u);
    }
    const uint32_t tail0 = head + 4u * nd;
    if (tail0 + (uint32_t)lane < rem) og[tail0 + lane] = st8[tail0 + lane];
    __builtin_amdgcn_wave_barrier();
  }
#pragma unroll
  for (int d = WAVE / 2; d > 0; d >>= 1) acc ^= __shfl_xor(acc, d, WAVE);
  if (lane == 0) {
    int ok = 0;
    if (len >= 4) {
      const uint32_t got = ((uint32_t)(msg[plen] ^ q.mask[plen]) << 24) | ((uint32_t)(msg[plen + 1] ^ q.mask[plen + 1]) << 16) |
                           ((uint32_t)(msg[plen + 2] ^ q.mask[plen + 2]) << 8) | (uint32_t)(msg[plen + 3] ^ q.mask[plen + 3]);
      ok = (acc == got);  // crc32 of an empty payload is 0 = the empty XOR
    }
    q.out_off[ord] = boff;
    q.out_len[ord] = plen;
    q.out_ok[ord] = (uint8_t)ok;  // (packet / CRC totals are summed by the host from these flags)
    q.out_pos[ord] = q.peaks[dyn_j0(q.dyn, q.j0) + f];
  }
}

// Link quality of the delivered packets: one thread per frame, keeping exactly the frames k_deframe_write keeps, record
// `ord` of the call's packet list.
struct QualityParams {
  const FrameQuality* fq;  // [nframes]
  const double* step;      // [npeaks] NCO step per flag
  ofdm_pkt_quality* out;   // [max_pkts]
  float inv_npilot, inv_nnull;
  int N, nmap;
};
__global__ void __launch_bounds__(256) k_quality_write(DeframeParams q, QualityParams w) {
  const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= dyn_nframes(q.dyn, q.nframes)) return;
  if (q.invalid[f]) return;
  const FrameResult r = q.res[f];
  if (r.status != FR_COMPLETE) return;
  const uint64_t pos = q.pos[f];
  const uint64_t ord = pos >> 40, boff = pos & ((1ull << 40) - 1);
  const uint32_t plen = r.packetlen >= 4 ? r.packetlen - 4 : 0;
  if (ord >= q.max_pkts || boff + plen > q.payload_cap) return;
  const uint32_t j = dyn_j0(q.dyn, q.j0) + f;
  const FrameQuality a = w.fq[f];
  ofdm_pkt_quality o;
  o.flag = q.peaks[j];
  o.first_symbol = (uint32_t)a.first_symbol;
  o.nsym = a.nsym;
  o.ncarriers = a.nsym * (uint32_t)w.nmap;
  o.coarse = a.coarse;
  // the NCO turns by step per sample: it removes an offset of -step * N / (2 pi) subcarrier spacings
  o.cfo_bins = (float)((double)a.coarse - w.step[j] * (double)w.N * 0.15915494309189533577);
  o.pilot_power = a.pilot * w.inv_npilot;
  o.null_power = a.null_ * w.inv_nnull;
  o.err_energy = a.err;
  o.ref_energy = a.ref;
  const double ratio = (double)o.pilot_power / (double)fmaxf(o.null_power, 1e-30f) - 1.0;
  o.snr_preamble_db = (float)(10.0 * log10(fmax(ratio, 1e-6)));
  o.snr_decision_db = (float)(10.0 * log10((double)a.ref / (double)fmaxf(a.err, 1e-30f)));
  w.out[ord] = o;
}

// Per-subcarrier channel state of the delivered packets: one WAVE per frame, keeping exactly the frames k_deframe_write
// keeps, copies the frame's four rows (k_rx_demod's CSI instantiation) to packet row `ord` with coalesced 16-byte moves.
struct CsiRows {
  c32* eq;  // [rows][stride]
  float* pre;
  float* err;
  float* ref;
};
__device__ __forceinline__ void csi_copy16(const void* src, void* dst, uint32_t n16, int lane) {
  const uint4* s = reinterpret_cast<const uint4*>(src);
  uint4* d = reinterpret_cast<uint4*>(dst);
  for (uint32_t k = (uint32_t)lane; k < n16; k += WAVE) d[k] = s[k];
}
__global__ void __launch_bounds__(256) k_csi_write(DeframeParams q, CsiRows fr, CsiRows pk, int stride) {
  const int lane = lane_id();
  const uint32_t f = blockIdx.x * 4 + (uint32_t)wave_id();
  if (f >= dyn_nframes(q.dyn, q.nframes)) return;
  if (q.invalid[f]) return;
  const FrameResult r = q.res[f];
  if (r.status != FR_COMPLETE) return;
  const uint64_t pos = q.pos[f];
  const uint64_t ord = pos >> 40, boff = pos & ((1ull << 40) - 1);
  const uint32_t plen = r.packetlen >= 4 ? r.packetlen - 4 : 0;
  if (ord >= q.max_pkts || boff + plen > q.payload_cap) return;
  const uint64_t fo = (uint64_t)f * (uint64_t)stride, po = ord * (uint64_t)stride;
  const uint32_t n16 = (uint32_t)stride / 4;  // (stride: a multiple of 4)
  csi_copy16(fr.eq + fo, pk.eq + po, 2 * n16, lane);
  csi_copy16(fr.pre + fo, pk.pre + po, n16, lane);
  csi_copy16(fr.err + fo, pk.err + po, n16, lane);
  csi_copy16(fr.ref + fo, pk.ref + po, n16, lane);
}

// Per-carrier summary of the packet rows (ofdm_rx_csi_summary), float64, in a fixed order: k_csi_summary sums the
// packets of chunk blockIdx.y (CSI_SUM_CHUNK consecutive rows) in row order, one thread per carrier; k_csi_summary_combine
// adds the chunks' partials in chunk order.  No atomics: the same rows give the same bits.
#define CSI_SUM_CHUNK 128
enum { CSI_S_PRE = 0, CSI_S_ERR = 1, CSI_S_REF = 2, CSI_S_INV = 3, CSI_S_COUNT = 4 };
struct CsiSumParams {
  CsiRows rows;
  const uint8_t* ok;   // [npk] CRC verdicts
  uint32_t npk;
  int occ, stride, crc_ok_only;
  double* part;        // [nchunks][CSI_S_COUNT][occ]
  uint32_t* part_n;    // [nchunks][occ] finite non-zero eq entries
  double* out;         // [CSI_S_COUNT][occ]
  uint32_t* out_n;     // [occ]
  uint32_t nchunks;
};
__global__ void __launch_bounds__(256) k_csi_summary(CsiSumParams s) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= s.occ) return;
  const uint32_t b = blockIdx.y;
  const uint32_t p0 = b * CSI_SUM_CHUNK, p1 = min(s.npk, p0 + CSI_SUM_CHUNK);
  double a_pre = 0.0, a_err = 0.0, a_ref = 0.0, a_inv = 0.0;
  uint32_t n_inv = 0;
  for (uint32_t p = p0; p < p1; p++) {
    if (s.crc_ok_only && !s.ok[p]) continue;
    const uint64_t o = (uint64_t)p * (uint64_t)s.stride + (uint64_t)i;
    a_pre += (double)s.rows.pre[o];
    a_err += (double)s.rows.err[o];
    a_ref += (double)s.rows.ref[o];
    const c32 e = s.rows.eq[o];
    const double re = (double)e.re, im = (double)e.im, m = re * re + im * im;
    if (isfinite(re) && isfinite(im) && m != 0.0) {
      a_inv += 1.0 / m;  // |1/eq|^2
      n_inv++;
    }
  }
  double* pp = s.part + (uint64_t)b * CSI_S_COUNT * (uint64_t)s.occ;
  pp[CSI_S_PRE * s.occ + i] = a_pre;
  pp[CSI_S_ERR * s.occ + i] = a_err;
  pp[CSI_S_REF * s.occ + i] = a_ref;
  pp[CSI_S_INV * s.occ + i] = a_inv;
  s.part_n[(uint64_t)b * (uint64_t)s.occ + i] = n_inv;
}
__global__ void __launch_bounds__(256) k_csi_summary_combine(CsiSumParams s) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= s.occ) return;
  double a[CSI_S_COUNT] = {0.0, 0.0, 0.0, 0.0};
  uint32_t n = 0;
  for (uint32_t b = 0; b < s.nchunks; b++) {
    const double* pp = s.part + (uint64_t)b * CSI_S_COUNT * (uint64_t)s.occ;
#pragma unroll
    for (int k = 0; k < CSI_S_COUNT; k++) a[k] += pp[k * s.occ + i];
    n += s.part_n[(uint64_t)b * (uint64_t)s.occ + i];
  }
#pragma unroll
  for (int k = 0; k < CSI_S_COUNT; k++) s.out[k * s.occ + i] = a[k];
  s.out_n[i] = n;
}

// raw (pre-dewhitening) messages, concatenated in stream order, for the PACKETS tap
__global__ void __launch_bounds__(256) k_raw_tap(DeframeParams q, const uint64_t* __restrict__ rawpos, uint8_t* __restrict__ dst) {
  const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= q.nframes) return;
  if (q.invalid[f]) return;
  const FrameResult r = q.res[f];
  if (r.status != FR_COMPLETE) return;
  const uint8_t* msg = q.raw + (uint64_t)f * RAW_SLOT;
  for (uint32_t i = 0; i < r.packetlen; i++) dst[rawpos[f] + i] = msg[i];
}
__global__ void __launch_bounds__(256) k_raw_len(DeframeParams q, uint64_t* __restrict__ lens) {
  const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= q.nframes) return;
  uint64_t l = 0;
  if (!q.invalid[f] && q.res[f].status == FR_COMPLETE) l = q.res[f].packetlen;
  lens[f] = l;
}

// Phases of the flags from their scanned integer advances.  Chunked streams: the line carried in from the
// flag that precedes this call's first one (phase ref_u at sample ref, step step_ref) is in force up to
// that first flag, which therefore starts from ref_u + turns(step_ref * (flag0 - ref)).
__global__ void __launch_bounds__(256) k_nco_phase(const uint64_t* __restrict__ peaks, const uint64_t* __restrict__ acc,
                                                    uint64_t npeaks, int ref_on, int64_t ref, uint64_t ref_u, double step_ref,
                                                    uint64_t* __restrict__ Phi_u, double* __restrict__ Phi) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= npeaks) return;
  uint64_t off = 0;
  if (ref_on) off = ref_u + nco_turns(step_ref * (double)((int64_t)peaks[0] - ref));
  const uint64_t u = acc[i] + off;
  Phi_u[i] = u;
  Phi[i] = nco_radians(u);
}

// ofdm_receiver-sigmix_c.dat / -nco_c.dat (ofdm_receiver.py~:150-152): the NCO's closed form sample by sample over
// the whole stream, phi[n] = Phi_j + step_j (n - p_j + 1) for p_j <= n < p_{j+1} (0 before the first flag, or the
// line carried in / the constant of SYNC "fixed"), nco = expj(phi) rounded to float32, sigmix = chan_filt * nco.
__global__ void __launch_bounds__(256) k_sigmix_tap(const c32* __restrict__ y, uint64_t n, const uint64_t* __restrict__ peaks,
                                                     const double* __restrict__ Phi, const double* __restrict__ step,
                                                     uint64_t npeaks, int ref_on, int64_t ref_peak, double ref_phi,
                                                     double ref_step, c32* __restrict__ sigmix, c32* __restrict__ nco) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint64_t lo = 0, hi = npeaks;  // first flag > i
  while (lo < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    if (peaks[mid] <= i) lo = mid + 1;
    else hi = mid;
  }
  double ph = 0.0;
  if (lo > 0) ph = Phi[lo - 1] + step[lo - 1] * (double)(i - peaks[lo - 1] + 1);
  else if (ref_on) ph = ref_phi + ref_step * (double)((int64_t)i - ref_peak + 1);
  const dc r = dexpj(ph);
  const c32 rot = mk((float)r.re, (float)r.im);
  if (nco) nco[i] = rot;
  if (sigmix) sigmix[i] = cmul(y[i], rot);
}
