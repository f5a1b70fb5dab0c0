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
//   forward, traceback, check   k_fec_decode's own passes (fec.h: fec_forward, fec_traceback, fec_check); the forward pass
//              here also stores its 64 metrics at every chunk start (CKPT: ckpt, 256 bytes per chunk).
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
  if (!fec_is_block(b.len)) {
    if (lane == 0) {
      ok[blockIdx.x] = 0;
      corrected[blockIdx.x] = 0;
    }
    return;
  }
  const FecGeom g(b.len, lgC);
  const uint32_t n = g.n, T = g.T;
  const uint8_t* in = in_all + b.in_off;
  uint64_t* w = ws + (uint64_t)blockIdx.x * ws_stride;
  int* ck = ckpt + (uint64_t)blockIdx.x * ws_stride;
  if (lane < 8) info[lane] = 0;
  const FecLane ln(lane);
  fec_forward<SOFT, true>(in, g, lane, ln, w, ck);
  fec_traceback(w, info, g, lane);
  fec_check<SOFT>(in, info, g, lane, payloads + b.out_off, ok, corrected, crc_table, xp8);
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
  for (int c = (int)g.nch - 1; c >= 0; c--) {
    const uint32_t t = 64u * (uint32_t)c + (uint32_t)lane;
    const int pk = fec_pair<SOFT>(in, t, g);
    int alpha = ck[64u * (uint32_t)c + (uint32_t)lane];
#pragma unroll
    for (int k = 0; k < WAVE; k++) {  // row k = alpha_{64c+k+1} (rows behind step T - 1 are never read)
      const fec_s16x2 v = __builtin_bit_cast(fec_s16x2, __builtin_amdgcn_readlane(pk, k));
      const int m0 = __builtin_amdgcn_sdot2(ln.sAB, v, __builtin_amdgcn_ds_bpermute(ln.a0, alpha), false);
      const int m1 = __builtin_amdgcn_sdot2(ln.nAB, v, __builtin_amdgcn_ds_bpermute(ln.a1, alpha), false);
      alpha = m1 > m0 ? m1 : m0;
      ab[k * FEC_REL_ROW + lane] = alpha;
    }
    __syncthreads();
    const int last = (int)(T - 1u - 64u * (uint32_t)c);  // the chunk's last step: under 63 in the final chunk only
    if (c == (int)g.nch - 1) best = ab[last * FEC_REL_ROW];
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
