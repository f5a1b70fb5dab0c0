// fec.h -- coded links: the rate-1/2, K = 7 convolutional code (133 / 171 octal, 802.11a arrangement) over the
// payload, a block interleaver, and a full-sequence Viterbi decoder.  Works at the payload boundary, like k_frame_pack:
// no modem kernel knows about it.  All arithmetic is integer: the result is defined bit for bit.
//
//   info bits   u[0 .. 8(n+4)) = payload | CRC-32 big-endian, MSB first; six zero tail bits; u[t] = 0 for t < 0
//   coded bits  c[2t] = A[t], c[2t+1] = B[t] over T = 8(n+4) + 6 steps, four zero pad bits: 16n + 80 bits
//   sent bit j  = c[(j mod R) * C + j / R], R = (16n + 80) / C, packed MSB first
//
// The shift register r of a step has bit k = u[t-k]; A = parity(r & 0x6D), B = parity(r & 0x4F).  State s of the
// trellis is r >> 1 of the step before: bit k = u[t-1-k], 64 states, one per lane of a wave.
#pragma once
#include "common.h"
#include "fec_plan.h"
#include "host_util.h"

#include <utility>

#define FEC_MASK_A 0x6Du
#define FEC_MASK_B 0x4Fu
#define FEC_ENC_THREADS 256
#define FEC_INFO_LDS (8 + 2048)  // info byte i at [8 + i]: zero before the first, room for payload + CRC + tail
// start metric of the 63 states the trellis cannot start in: below every reachable path (|metric| <= 2 * 16358 * 127)
#define FEC_UNREACHABLE (-(1 << 29))

// host side (engine_fec.inc): CodecStage (host_util.h) and the code's own
struct FecState : CodecStage {
  DevBuf d_ok, d_corr, d_ws;
  std::vector<FecBlk> blk;
  std::vector<hipEvent_t> ev;  // three per slice of a timed decode: depuncture | decoder
  void release() {
    d_ok.release();
    d_corr.release();
    d_ws.release();
    for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    ev.clear();
    CodecStage::release();
  }
};

// the seven register bits u[t-6 .. t] of step t out of the info bytes in LDS (info: FEC_INFO_LDS layout)
__device__ __forceinline__ uint32_t fec_register(const uint8_t* info, uint32_t t) {
  const uint32_t q = 8u + (t >> 3);
  const uint32_t w = ((uint32_t)info[q - 1] << 8) | (uint32_t)info[q];
  return (w >> (7u - (t & 7u))) & 0x7Fu;
}

// CRC-32 of info bytes [0, n) in LDS by `nthreads` threads, PIECE bytes each (nthreads * PIECE >= n): the caller
// XOR-reduces the returned parts (crc_multmodp, common.h)
template <int PIECE>
__device__ __forceinline__ uint32_t fec_crc_part(const uint8_t* info, uint32_t n, int tid, const uint32_t* __restrict__ crc_table,
                                                 const uint32_t* __restrict__ xp8) {
  const uint32_t o = (uint32_t)PIECE * (uint32_t)tid;
  if (o >= n) return 0u;
  const uint32_t nb = (n - o < (uint32_t)PIECE) ? (n - o) : (uint32_t)PIECE;
  uint32_t crc = 0xFFFFFFFFu;
  for (uint32_t b = 0; b < nb; b++) crc = crc_table[(crc ^ info[8u + o + b]) & 0xFFu] ^ (crc >> 8);
  crc ^= 0xFFFFFFFFu;
  return crc_multmodp(xp8[n - (o + nb)], crc);
}

// ---------------------------------------------------------------------------------
// Encoders (k_fec_encode here, k_fec_puncture in fec_punct.h): one workgroup per block.  The payload goes to LDS once,
// the CRC is summed there in 8-byte pieces (fec_stage_info), then every thread composes whole output bytes
// (fec_compose): a sent bit is one parity over seven info bits, found through the interleaver.  No atomics: each
// output byte has one writer.
// ---------------------------------------------------------------------------------
// The n payload bytes at src to LDS in the FEC_INFO_LDS layout, zeros around them, the CRC-32 of them big-endian behind
// them.  `red` holds one word per wave.  Ends with a barrier: every thread may read info[] after it.
__device__ __forceinline__ void fec_stage_info(uint8_t* info, uint32_t* red, const uint8_t* __restrict__ src, uint32_t n, int tid,
                                               const uint32_t* __restrict__ crc_table, const uint32_t* __restrict__ xp8) {
  for (int i = tid; i < FEC_INFO_LDS; i += FEC_ENC_THREADS) {
    const int k = i - 8;
    info[i] = (k >= 0 && (uint32_t)k < n) ? src[k] : (uint8_t)0;
  }
  __syncthreads();
  uint32_t acc = fec_crc_part<8>(info, n, tid, crc_table, xp8);
#pragma unroll
  for (int d = WAVE / 2; d > 0; d >>= 1) acc ^= __shfl_xor(acc, d, WAVE);
  if (lane_id() == 0) red[wave_id()] = acc;
  __syncthreads();
  if (tid < 4) {
    uint32_t crc32 = 0;
#pragma unroll
    for (int w = 0; w < FEC_ENC_THREADS / WAVE; w++) crc32 ^= red[w];
    info[8u + n + (uint32_t)tid] = (uint8_t)(crc32 >> (8 * (3 - tid)));  // struct.pack(">I", crc)
  }
  __syncthreads();
}

// The nout bytes of a block behind a 2^lgc-column interleaver: sent bit j is position (j mod R) * 2^lgc + j / R,
// R = 8 nout >> lgc, of the sequence before the interleaver.  Position q < nbits is coded bit coded_of(q) of the
// mother code (c[2t] = A[t], c[2t+1] = B[t]); the positions from nbits on are zero.
template <typename CodedOf>
__device__ __forceinline__ void fec_compose(uint8_t* __restrict__ out, const uint8_t* info, uint32_t nout, uint32_t lgc, uint32_t nbits,
                                            int tid, CodedOf coded_of) {
  const uint32_t R = (8u * nout) >> lgc;
  for (uint32_t ob = (uint32_t)tid; ob < nout; ob += FEC_ENC_THREADS) {
    uint32_t col = (8u * ob) / R, row = 8u * ob - col * R;
    uint32_t by = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) {
      const uint32_t q = (row << lgc) + col;
      uint32_t bit = 0;
      if (q < nbits) {
        const uint32_t i = coded_of(q);
        bit = (uint32_t)__popc(fec_register(info, i >> 1) & ((i & 1u) ? FEC_MASK_B : FEC_MASK_A)) & 1u;
      }
      by = (by << 1) | bit;
      if (++row == R) {
        row = 0;
        col++;
      }
    }
    out[ob] = (uint8_t)by;
  }
}

__global__ void __launch_bounds__(FEC_ENC_THREADS) k_fec_encode(const uint8_t* __restrict__ payloads, const FecBlk* __restrict__ blk,
                                                                uint8_t* __restrict__ coded, const uint32_t* __restrict__ crc_table,
                                                                const uint32_t* __restrict__ xp8, uint32_t lgC) {
  __shared__ uint8_t info[FEC_INFO_LDS];
  __shared__ uint32_t red[FEC_ENC_THREADS / WAVE];
  const FecBlk b = blk[blockIdx.x];
  const uint32_t n = b.len;  // <= OFDM_FEC_MAX_PAYLOAD (the host refuses longer ones)
  const int tid = threadIdx.x;
  fec_stage_info(info, red, payloads + b.in_off, n, tid, crc_table, xp8);
  const uint32_t ncoded = 2u * (8u * (n + 4u) + 6u);  // the four bits behind them are the pad
  fec_compose(coded + b.out_off, info, 2u * n + 10u, lgC, ncoded, tid, [](uint32_t q) { return q; });
}

// ---------------------------------------------------------------------------------
// Decoder: one wave per block, lane = state.  Three passes, each a function of its own below (fec_forward,
// fec_traceback, fec_check); k_fec_decode_rel (fec_rel.h) runs the same three in front of its backward sweep.
//   forward    64 steps at a time: lane k fetches the two values of step 64c + k (deinterleaved on load), the step loop
//              reads them as wave-uniform scalars; a step is two cross-lane reads of the predecessors' metrics (lanes
//              s >> 1 and (s >> 1) | 32), add-compare-select, and one __ballot = the step's 64 decisions.  Lane k keeps
//              the word of step k; a chunk's 64 words leave in one 512-byte store.
//   traceback  the chunks come back the same way, newest first; the walk from state 0 runs on wave-uniform values
//              (a lane read of the step's word, shifted by the state): no memory access per step.  A step's decision
//              is the info bit six steps earlier, so the decided bits of a chunk are one 64-bit scalar and the state
//              is a six-bit field of it.
//   check      payload out, CRC-32 of it against the decoded one, and `corrected`: the decoded sequence is encoded
//              again, 64 steps per pass, and compared with the signs of the values that are no erasure.
// Both branches into state s carry the same input bit s & 1; their register words differ in bit 6 only, which both
// generators tap, so the second branch's metric is the negative of the first's.
// ---------------------------------------------------------------------------------
template <bool SOFT>
__device__ __forceinline__ int fec_value(const uint8_t* __restrict__ in, uint32_t i, uint32_t lgC, uint32_t R) {
  const uint32_t j = (i & ((1u << lgC) - 1u)) * R + (i >> lgC);  // where coded bit i was sent
  if (SOFT) {
    const int v = (int)(int8_t)in[j];
    return v < -127 ? -127 : v;
  }
  return ((in[j >> 3] >> (7u - (j & 7u))) & 1u) ? 1 : -1;
}

typedef short fec_s16x2 __attribute__((ext_vector_type(2)));

// What lane = state s keeps for every step into it: the ds_bpermute byte addresses of its two predecessors' metrics, and
// the signs of the first branch's two coded bits, packed like the step's values, with their negatives.
struct FecLane {
  int a0, a1;
  fec_s16x2 sAB, nAB;
  __device__ __forceinline__ explicit FecLane(int lane) {
    a0 = (lane >> 1) << 2, a1 = a0 + 128;
    const short sA = (__popc((uint32_t)lane & FEC_MASK_A) & 1) ? 1 : -1;
    const short sB = (__popc((uint32_t)lane & FEC_MASK_B) & 1) ? 1 : -1;
    sAB = {sA, sB}, nAB = {(short)-sA, (short)-sB};
  }
};

// One trellis step for every state at once.  K is the step's place in its chunk: the values come from lane K of `pk`
// as scalars, and lane K keeps the step's decision word (two single-lane register writes; the lane select of
// v_writelane_b32 has to be a constant or M0, hence the template; this compiler has no builtin for it).
template <int K>
__device__ __forceinline__ void fec_step(int& metric, int& dlo, int& dhi, int pk, const FecLane& ln) {
  // both values of the step in one scalar (A low, B high); the lane's two signs packed the same way: one dot product
  // adds the branch metric to the first predecessor's metric, one with the signs inverted to the second's
  const fec_s16x2 v = __builtin_bit_cast(fec_s16x2, __builtin_amdgcn_readlane(pk, K));
  const int m0 = __builtin_amdgcn_sdot2(ln.sAB, v, __builtin_amdgcn_ds_bpermute(ln.a0, metric), false);
  const int m1 = __builtin_amdgcn_sdot2(ln.nAB, v, __builtin_amdgcn_ds_bpermute(ln.a1, metric), false);
  const bool d = m1 > m0;  // a tie keeps the predecessor with u[t-6] = 0
  metric = d ? m1 : m0;
  const uint64_t word = __ballot(d);
  const int wl = (int)(uint32_t)word, wh = (int)(uint32_t)(word >> 32);
  // (gfx950 wants two wait states between a VALU write of an SGPR and a VALU read of it; the compiler places them
  // for its own instructions, not for operands of inline assembly: without the s_nop the word of the compare right
  // in front is read before it is written)
  asm volatile("s_nop 1\n\tv_writelane_b32 %0, %2, %4\n\tv_writelane_b32 %1, %3, %4" : "+v"(dlo), "+v"(dhi) : "s"(wl), "s"(wh), "n"(K));
}
template <int... Ks>
__device__ __forceinline__ void fec_chunk(int& metric, int& dlo, int& dhi, int pk, const FecLane& ln, std::integer_sequence<int, Ks...>) {
  (fec_step<Ks>(metric, dlo, dhi, pk, ln), ...);
}

// One step of the walk back, all on wave-uniform values.  W holds the chunk's decided bits: bit 63 - p is
// u[64c - 6 + p] (a step's decision IS the info bit six steps before it).  From step 57 down the state is a field of W
// (FIELD); the six steps above it still need bits of the chunk behind and carry the state along.
template <int K, bool FIELD>
__device__ __forceinline__ void fec_back(uint64_t& W, uint32_t& cur, int mlo, int mhi) {
  const uint64_t word = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane(mhi, K) << 32) | (uint64_t)(uint32_t)__builtin_amdgcn_readlane(mlo, K);
  if (FIELD) cur = (uint32_t)(W >> (57 - (K < 58 ? K : 57))) & 63u;
  const uint64_t d = (word >> cur) & 1ull;
  W |= d << (63 - K);
  if (!FIELD) cur = (cur >> 1) | ((uint32_t)d << 5);
}
template <int... Ks>
__device__ __forceinline__ void fec_back_chunk(uint64_t& W, uint32_t& cur, int mlo, int mhi, std::integer_sequence<int, Ks...>) {
  (fec_back<63 - Ks, (63 - Ks < 58)>(W, cur, mlo, mhi), ...);
}

// ---- the decoder's passes ----
// One block as a decoder sees it: `len` is a block length (fec_is_block), nch <= ws_stride / 64 (the host sized the
// stride by the widest block).
struct FecGeom {
  uint32_t n, T, nch, R, lgC;  // payload bytes, trellis steps, chunks of 64 steps, interleaver rows and log2 columns
  __device__ __forceinline__ FecGeom(uint32_t len, uint32_t lgC_)
      : n((len - 10u) >> 1), T(4u * len - 2u), nch((T + 63u) >> 6), R((8u * len) >> lgC_), lgC(lgC_) {}
};

// The packed values of step t (A low, B high), 0 behind step T: such a step adds nothing, its decisions are never read.
template <bool SOFT>
__device__ __forceinline__ int fec_pair(const uint8_t* in, uint32_t t, const FecGeom& g) {
  int pk = 0;
  if (t < g.T) {
    const int vA = fec_value<SOFT>(in, 2u * t, g.lgC, g.R), vB = fec_value<SOFT>(in, 2u * t + 1u, g.lgC, g.R);
    pk = (vA & 0xFFFF) | (vB << 16);
  }
  return pk;
}

// Forward: the decision words of every step to w.  CKPT: the 64 metrics in front of every chunk (alpha_{64c}) to ck.
template <bool SOFT, bool CKPT>
__device__ __forceinline__ void fec_forward(const uint8_t* in, const FecGeom& g, int lane, const FecLane& ln, uint64_t* w, int* ck) {
  int metric = lane == 0 ? 0 : FEC_UNREACHABLE;
  for (uint32_t c = 0; c < g.nch; c++) {
    const int pk = fec_pair<SOFT>(in, 64u * c + (uint32_t)lane, g);
    if (CKPT) ck[64u * c + (uint32_t)lane] = metric;
    int dlo = 0, dhi = 0;
    fec_chunk(metric, dlo, dhi, pk, ln, std::make_integer_sequence<int, WAVE>{});
    w[64u * c + (uint32_t)lane] = ((uint64_t)(uint32_t)dhi << 32) | (uint64_t)(uint32_t)dlo;
  }
}

// Traceback from state 0 (every lane reads back the words it stored itself): the info bytes to info[8 ..]; the eight
// zeros in front of them are the kernel's to write.  Ends with a barrier.
__device__ __forceinline__ void fec_traceback(const uint64_t* w, uint8_t* info, const FecGeom& g, int lane) {
  uint32_t cur = 0;   // state behind the step the walk stands at
  uint64_t next = 0;  // W of the chunk behind this one
  for (int c = (int)g.nch - 1; c >= 0; c--) {
    const uint64_t mine = w[64u * (uint32_t)c + (uint32_t)lane];
    const int mlo = (int)(uint32_t)mine, mhi = (int)(uint32_t)(mine >> 32);
    uint64_t W = 0;
    const uint32_t last = g.T - 1u - 64u * (uint32_t)c;  // the chunk's last step: under 63 in the final chunk only
    if (last >= 63u) {
      fec_back_chunk(W, cur, mlo, mhi, std::make_integer_sequence<int, WAVE>{});
    } else {
#pragma unroll 1
      for (int k = (int)last; k >= 0; k--) {
        const uint64_t word = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane(mhi, k) << 32) | (uint64_t)(uint32_t)__builtin_amdgcn_readlane(mlo, k);
        const uint64_t d = (word >> cur) & 1ull;
        W |= d << (63 - k);
        cur = (cur >> 1) | ((uint32_t)d << 5);
      }
    }
    cur = (uint32_t)(W >> 58);  // u[64c-1 .. 64c-6]: the state in front of the chunk
    const uint64_t Q = (W << 6) | (next >> 58);  // bit 63 - i = u[64c + i]: the chunk's eight info bytes, MSB first
    next = W;
    if (lane < 8) info[8u + 8u * (uint32_t)c + (uint32_t)lane] = (uint8_t)(Q >> (56 - 8 * lane));
  }
  __syncthreads();
}

// Check: the payload to out, the CRC verdict and `corrected` of block blockIdx.x.
template <bool SOFT>
__device__ __forceinline__ void fec_check(const uint8_t* in, const uint8_t* info, const FecGeom& g, int lane, uint8_t* out,
                                          uint8_t* ok, uint32_t* corrected, const uint32_t* crc_table, const uint32_t* xp8) {
  const uint32_t n = g.n;
  for (uint32_t i = (uint32_t)lane; i < n; i += WAVE) out[i] = info[8u + i];
  uint32_t acc = fec_crc_part<32>(info, n, lane, crc_table, xp8);
#pragma unroll
  for (int d = WAVE / 2; d > 0; d >>= 1) acc ^= __shfl_xor(acc, d, WAVE);
  const uint32_t got = ((uint32_t)info[8u + n] << 24) | ((uint32_t)info[9u + n] << 16) | ((uint32_t)info[10u + n] << 8) | (uint32_t)info[11u + n];
  uint32_t bad = 0;
  for (uint32_t c = 0; c < g.nch; c++) {
    const uint32_t t = 64u * c + (uint32_t)lane;
    if (t < g.T) {
      const uint32_t r = fec_register(info, t);
      const int vA = fec_value<SOFT>(in, 2u * t, g.lgC, g.R), vB = fec_value<SOFT>(in, 2u * t + 1u, g.lgC, g.R);
      const int A = __popc(r & FEC_MASK_A) & 1, B = __popc(r & FEC_MASK_B) & 1;
      bad += (vA != 0 && (vA > 0) != (A != 0)) ? 1u : 0u;
      bad += (vB != 0 && (vB > 0) != (B != 0)) ? 1u : 0u;
    }
  }
  bad = wave_sum(bad);
  if (lane == 0) {
    ok[blockIdx.x] = acc == got ? 1 : 0;
    corrected[blockIdx.x] = bad;
  }
}

template <bool SOFT>
__global__ void __launch_bounds__(WAVE) k_fec_decode(const uint8_t* __restrict__ in_all, const FecBlk* __restrict__ blk,
                                                     uint8_t* __restrict__ payloads, uint8_t* __restrict__ ok,
                                                     uint32_t* __restrict__ corrected, uint64_t* __restrict__ ws, uint64_t ws_stride,
                                                     const uint32_t* __restrict__ crc_table, const uint32_t* __restrict__ xp8,
                                                     uint32_t lgC) {
  __shared__ uint8_t info[FEC_INFO_LDS];
  const int lane = threadIdx.x;
  const FecBlk b = blk[blockIdx.x];
  if (!fec_is_block(b.len)) {
    if (lane == 0) {
      ok[blockIdx.x] = 0;
      corrected[blockIdx.x] = 0;
    }
    return;
  }
  const FecGeom g(b.len, lgC);
  const uint8_t* in = in_all + b.in_off;
  uint64_t* w = ws + (uint64_t)blockIdx.x * ws_stride;
  if (lane < 8) info[lane] = 0;
  fec_forward<SOFT, false>(in, g, lane, FecLane(lane), w, nullptr);
  fec_traceback(w, info, g, lane);
  fec_check<SOFT>(in, info, g, lane, payloads + b.out_off, ok, corrected, crc_table, xp8);
}
