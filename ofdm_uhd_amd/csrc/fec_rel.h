// fec_rel.h -- coded links, reliabilities out: the Viterbi decoder of fec.h with the full (max-log-MAP) soft output, one
// reliability byte per decoded payload byte in the format ofdm_rs_decode_rel takes.  Integer arithmetic, defined bit
// for bit (include/ofdm_hip.h, "coded links, reliabilities out").
//
//   alpha_t(s)   best metric of a path from state 0 at step 0 to state s at step t: k_fec_decode's `metric`
//   beta_t(s)    best metric of a path from state s at step t to state 0 at step T
//   Delta_t      alpha_T(0) - max over s' with (s' & 1) != u^[t] of alpha_{t+1}(s') + beta_{t+1}(s')
//   q[m]         min(255, min over the byte's eight bits of Delta_t / 2)
#pragma once
#include "fec.h"

#define FEC_REL_ROW 66  // words per row of the alpha + beta image: 8-byte rows, and lane k's pair reads fall on banks 2k + 2j

// what the soft-output decoder keeps on a handle next to FecState: nothing of it exists until a call to it
struct FecRelState {
  DevBuf d_ckpt, d_rel;          // the forward metrics at every chunk start (4 bytes per step and block in flight); rel staging
  void release() {
    d_ckpt.release();
    d_rel.release();
  }
};

// ---------------------------------------------------------------------------------
// Decoder with reliabilities: one wave per block, lane = state, as k_fec_decode.
//   forward, traceback, check   k_fec_decode's, statement for statement (fec_chunk, fec_back_chunk); the forward pass also
//              stores its 64 metrics at every chunk start (ckpt, 256 bytes per chunk).
//   backward   chunk by chunk, newest first.  The chunk's 64 alpha vectors are formed again from its checkpoint, row k of
//              an LDS image = alpha_{64c+k+1}.  Then beta runs back over the chunk: lane s reads beta_{t+1} of its two
//              successors ((s & 31) << 1) | b with two ds_bpermute, adds the branch metric (the two differ in sign only:
//              both generators tap u[t]) and keeps the larger; before that step, row k becomes alpha_{t+1} + beta_{t+1}.
//   maximum    transposed: lane k owns step 64c + k and runs over row k's 32 states with (s' & 1) != u^[t], as 32 pair
//              reads.  A byte's eight steps lie in eight neighbouring lanes; three cross-lane minima make q.
// ---------------------------------------------------------------------------------
template <bool SOFT>
__global__ void __launch_bounds__(WAVE) k_fec_decode_rel(const uint8_t* __restrict__ in_all, const FecBlk* __restrict__ blk,
                                                         uint8_t* __restrict__ payloads, uint8_t* __restrict__ rel,
                                                         uint8_t* __restrict__ ok, uint32_t* __restrict__ corrected,
                                                         uint64_t* __restrict__ ws, int* __restrict__ ckpt, uint64_t ws_stride,
                                                         const uint32_t* __restrict__ crc_table, const uint32_t* __restrict__ xp8,
                                                         uint32_t lgC) {
  __shared__ uint8_t info[FEC_INFO_LDS];
  __shared__ __attribute__((aligned(8))) int ab[WAVE * FEC_REL_ROW];
  const int lane = threadIdx.x;
  const FecBlk b = blk[blockIdx.x];
  const uint32_t len = b.len;
  if (!fec_is_block(len)) {
    if (lane == 0) {
      ok[blockIdx.x] = 0;
      corrected[blockIdx.x] = 0;
    }
    return;
  }
  const uint32_t n = (len - 10u) >> 1;
  const uint32_t T = 4u * len - 2u;
  const uint32_t nch = (T + 63u) >> 6;  // <= ws_stride / 64 (the host sized the stride by the widest block)
  const uint32_t R = (8u * len) >> lgC;
  const uint8_t* in = in_all + b.in_off;
  uint64_t* w = ws + (uint64_t)blockIdx.x * ws_stride;
  int* ck = ckpt + (uint64_t)blockIdx.x * ws_stride;
  if (lane < 8) info[lane] = 0;

  // ---- forward ------------------------------------------------------------------------------------------------
  int metric = lane == 0 ? 0 : FEC_UNREACHABLE;
  const int a0 = (lane >> 1) << 2, a1 = a0 + 128;  // ds_bpermute byte addresses of the two predecessors
  const short sA = (__popc((uint32_t)lane & FEC_MASK_A) & 1) ? 1 : -1;
  const short sB = (__popc((uint32_t)lane & FEC_MASK_B) & 1) ? 1 : -1;
  const fec_s16x2 sAB = {sA, sB}, nAB = {(short)-sA, (short)-sB};
  for (uint32_t c = 0; c < nch; c++) {
    const uint32_t t = 64u * c + (uint32_t)lane;
    int pk = 0;
    if (t < T) {
      const int vA = fec_value<SOFT>(in, 2u * t, lgC, R), vB = fec_value<SOFT>(in, 2u * t + 1u, lgC, R);
      pk = (vA & 0xFFFF) | (vB << 16);
    }
    ck[64u * c + (uint32_t)lane] = metric;  // alpha_{64c}
    int dlo = 0, dhi = 0;
    fec_chunk(metric, dlo, dhi, pk, a0, a1, sAB, nAB, std::make_integer_sequence<int, WAVE>{});
    w[64u * c + (uint32_t)lane] = ((uint64_t)(uint32_t)dhi << 32) | (uint64_t)(uint32_t)dlo;
  }

  // ---- traceback from state 0 ----------------------------------------------------------------------------------
  uint32_t cur = 0;
  uint64_t next = 0;
  for (int c = (int)nch - 1; c >= 0; c--) {
    const uint64_t mine = w[64u * (uint32_t)c + (uint32_t)lane];
    const int mlo = (int)(uint32_t)mine, mhi = (int)(uint32_t)(mine >> 32);
    uint64_t W = 0;
    const uint32_t last = T - 1u - 64u * (uint32_t)c;
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
    cur = (uint32_t)(W >> 58);
    const uint64_t Q = (W << 6) | (next >> 58);
    next = W;
    if (lane < 8) info[8u + 8u * (uint32_t)c + (uint32_t)lane] = (uint8_t)(Q >> (56 - 8 * lane));
  }
  __syncthreads();

  // ---- payload, CRC verdict, corrected ----------------------------------------------------------------------------
  uint8_t* out = payloads + b.out_off;
  for (uint32_t i = (uint32_t)lane; i < n; i += WAVE) out[i] = info[8u + i];
  uint32_t acc = fec_crc_part<32>(info, n, lane, crc_table, xp8);
#pragma unroll
  for (int d = WAVE / 2; d > 0; d >>= 1) acc ^= __shfl_xor(acc, d, WAVE);
  const uint32_t got = ((uint32_t)info[8u + n] << 24) | ((uint32_t)info[9u + n] << 16) | ((uint32_t)info[10u + n] << 8) | (uint32_t)info[11u + n];
  uint32_t bad = 0;
  for (uint32_t c = 0; c < nch; c++) {
    const uint32_t t = 64u * c + (uint32_t)lane;
    if (t < T) {
      const uint32_t r = fec_register(info, t);
      const int vA = fec_value<SOFT>(in, 2u * t, lgC, R), vB = fec_value<SOFT>(in, 2u * t + 1u, lgC, R);
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
  if (n == 0) return;  // no payload byte, no reliability

  // ---- backward sweep: beta, alpha + beta, the masked maximum, q ------------------------------------------------------
  uint8_t* q = rel + b.out_off;
  const int b0 = (lane & 31) << 3, b1 = b0 + 4;  // ds_bpermute byte addresses of the successors with input bit 0 and 1
  // the register of the branch into the successor with input bit 0: bit k = u[t-k], bit 0 clear
  const uint32_t r0 = ((uint32_t)lane << 1) & 0x7Fu;
  const short tA = (__popc(r0 & FEC_MASK_A) & 1) ? 1 : -1;
  const short tB = (__popc(r0 & FEC_MASK_B) & 1) ? 1 : -1;
  const fec_s16x2 tAB = {tA, tB}, ntAB = {(short)-tA, (short)-tB};
  int beta = lane == 0 ? 0 : FEC_UNREACHABLE;  // beta_T
  int best = 0;                                // M* = alpha_T(0)
  for (int c = (int)nch - 1; c >= 0; c--) {
    const uint32_t t = 64u * (uint32_t)c + (uint32_t)lane;
    int pk = 0;
    if (t < T) {
      const int vA = fec_value<SOFT>(in, 2u * t, lgC, R), vB = fec_value<SOFT>(in, 2u * t + 1u, lgC, R);
      pk = (vA & 0xFFFF) | (vB << 16);
    }
    int alpha = ck[64u * (uint32_t)c + (uint32_t)lane];
#pragma unroll
    for (int k = 0; k < WAVE; k++) {  // row k = alpha_{64c+k+1} (rows behind step T - 1 are never read)
      const fec_s16x2 v = __builtin_bit_cast(fec_s16x2, __builtin_amdgcn_readlane(pk, k));
      const int m0 = __builtin_amdgcn_sdot2(sAB, v, __builtin_amdgcn_ds_bpermute(a0, alpha), false);
      const int m1 = __builtin_amdgcn_sdot2(nAB, v, __builtin_amdgcn_ds_bpermute(a1, alpha), false);
      alpha = m1 > m0 ? m1 : m0;
      ab[k * FEC_REL_ROW + lane] = alpha;
    }
    __syncthreads();
    const int last = (int)(T - 1u - 64u * (uint32_t)c);  // the chunk's last step: under 63 in the final chunk only
    if (c == (int)nch - 1) best = ab[last * FEC_REL_ROW];
#pragma unroll
    for (int k = WAVE - 1; k >= 0; k--) {
      if (k <= last) {  // (wave-uniform)
        ab[k * FEC_REL_ROW + lane] += beta;  // alpha_{t+1} + beta_{t+1}, t = 64c + k
        const fec_s16x2 v = __builtin_bit_cast(fec_s16x2, __builtin_amdgcn_readlane(pk, k));
        const int n0 = __builtin_amdgcn_sdot2(tAB, v, __builtin_amdgcn_ds_bpermute(b0, beta), false);
        const int n1 = __builtin_amdgcn_sdot2(ntAB, v, __builtin_amdgcn_ds_bpermute(b1, beta), false);
        beta = n1 > n0 ? n1 : n0;  // beta_t
      }
    }
    __syncthreads();
    int h = 255;
    if (t < 8u * n) {  // a payload bit: lane k reduces row k
      const uint32_t ub = ((uint32_t)info[8u + (t >> 3)] >> (7u - (t & 7u))) & 1u;  // u^[t]
      const int2* row = reinterpret_cast<const int2*>(&ab[lane * FEC_REL_ROW]);
      int m = INT32_MIN;
#pragma unroll
      for (int j = 0; j < WAVE / 2; j++) {
        const int2 p = row[j];
        const int cand = ub ? p.x : p.y;  // the states whose newest bit is not u^[t]
        m = cand > m ? cand : m;
      }
      const int half = (best - m) >> 1;  // Delta_t / 2, Delta_t >= 0 and even
      h = half < 255 ? half : 255;
    }
#pragma unroll
    for (int d = 1; d < 8; d <<= 1) {
      const int o = __shfl_xor(h, d, WAVE);
      h = o < h ? o : h;
    }
    const uint32_t m = 8u * (uint32_t)c + ((uint32_t)lane >> 3);
    if ((lane & 7) == 0 && m < n) q[m] = (uint8_t)h;
    __syncthreads();  // the next chunk writes the image again
  }
}
