// sig.h -- the signal field's kernels (include/ofdm_hip.h, "coded links: the signal field"; host arithmetic: sig_plan.h).
//   k_sig_encode        one wave per block: the field of the block's word, then the body, copied
//   k_sig_decode<SOFT>  one wave per packet: exhaustive maximum-likelihood decoding of the (24,12) codeword from the
//                       sum of its four copies, all 4096 metrics across the wave's 64 lanes, no LDS
// Both run four blocks per 256-thread workgroup.
#pragma once
#include "common.h"
#include "host_util.h"
#include "sig_plan.h"

constexpr int SIG_WAVES = 4, SIG_THREADS = SIG_WAVES * WAVE;

struct SigState : CodecStage {
  DevBuf d_res;
  std::vector<SigBlk> blk;
  std::vector<uint32_t> res;  // word | margin << 16 per packet
  void release() {
    d_res.release();
    CodecStage::release();
  }
};

__device__ __forceinline__ bool sig_my_block(const SigBlk* __restrict__ blk, uint32_t nblk, uint32_t& k, SigBlk& b) {
  k = blockIdx.x * SIG_WAVES + (uint32_t)__builtin_amdgcn_readfirstlane(wave_id());
  if (k >= nblk) return false;
  b = blk[k];
  return true;
}

// Bytes where source and destination differ in their alignment, dwords between a byte head and a byte tail where they
// agree; lane-contiguous either way.
__global__ __launch_bounds__(SIG_THREADS) void k_sig_encode(const uint8_t* __restrict__ bodies, const SigBlk* __restrict__ blk, uint32_t nblk,
                                                            uint8_t* __restrict__ out) {
  uint32_t k;
  SigBlk b;
  if (!sig_my_block(blk, nblk, k, b)) return;
  const uint32_t lane = (uint32_t)lane_id();
  uint8_t* d = out + b.out_off;
  if (lane < SIG_FIELD_BYTES) d[lane] = sig_field_byte(sig_codeword(b.word), lane);
  d += SIG_FIELD_BYTES;
  const uint8_t* s = bodies + b.in_off;
  const uint32_t n = b.len;
  uint32_t head = 0, mid = 0;
  if ((((uintptr_t)s ^ (uintptr_t)d) & 3u) == 0) {
    head = min(n, (uint32_t)((4u - ((uintptr_t)d & 3u)) & 3u));
    mid = (n - head) & ~3u;
  }
  if (lane < head) d[lane] = s[lane];
  const uint32_t* s4 = reinterpret_cast<const uint32_t*>(s + head);
  uint32_t* d4 = reinterpret_cast<uint32_t*>(d + head);
  for (uint32_t i = lane; i < mid / 4; i += WAVE) d4[i] = s4[i];
  for (uint32_t i = head + mid + lane; i < n; i += WAVE) d[i] = s[i];
}

// ---- decode ---------------------------------------------------------------------------------------------------------
// (metric, word) under the decoder's total order -- the larger metric first, the smaller word on a tie -- as one
// number: the keys of different words differ, and the larger key is the better word.
__device__ __forceinline__ uint32_t sig_key(int m, uint32_t w) { return ((uint32_t)(m + SIG_MAX_METRIC) << 12) | (SIG_WORDS - 1 - w); }
// the best two of a set and one more
__device__ __forceinline__ void sig_top2(uint32_t& k1, uint32_t& k2, uint32_t k) {
  k2 = max(k2, min(k1, k));
  k1 = max(k1, k);
}

// byte i (i < 16 n) of the 4 n-byte words that lanes 0 .. 4 n - 1 hold, as every lane's own value for its own i
template <int BYTES>
__device__ __forceinline__ uint32_t sig_byte_of(uint32_t word, uint32_t i) {
  return ((uint32_t)__shfl((int)word, (int)(i / BYTES), WAVE) >> (8 * (i % BYTES))) & 0xFFu;
}

// The value of field bit t of the packet at p for t = lane (a) and t = 64 + lane (b, lanes 0 .. 31), from the widest
// loads p's alignment allows.  SOFT: 96 int8 values; else 12 bytes, a bit giving +1 or -1.
template <bool SOFT>
__device__ __forceinline__ void sig_load(const uint8_t* __restrict__ p, uint32_t lane, int& a, int& b) {
  const uint32_t ta = lane, tb = (64 + lane) % SIG_FIELD_BITS;  // (lanes 32 .. 63: b is not used)
  if constexpr (SOFT) {
    uint32_t va, vb;
    if (((uintptr_t)p & 15u) == 0) {  // six lanes, 16 bytes each
      uint4 q = make_uint4(0, 0, 0, 0);
      if (lane < 6) q = *reinterpret_cast<const uint4*>(p + 16 * lane);
      // dword i of the field is component i & 3 of lane i >> 2
      const uint32_t ia = ta / 4, ib = tb / 4;
      const uint32_t xa = (uint32_t)__shfl((int)q.x, (int)(ia >> 2), WAVE), ya = (uint32_t)__shfl((int)q.y, (int)(ia >> 2), WAVE),
                     za = (uint32_t)__shfl((int)q.z, (int)(ia >> 2), WAVE), wa = (uint32_t)__shfl((int)q.w, (int)(ia >> 2), WAVE);
      const uint32_t xb = (uint32_t)__shfl((int)q.x, (int)(ib >> 2), WAVE), yb = (uint32_t)__shfl((int)q.y, (int)(ib >> 2), WAVE),
                     zb = (uint32_t)__shfl((int)q.z, (int)(ib >> 2), WAVE), wb = (uint32_t)__shfl((int)q.w, (int)(ib >> 2), WAVE);
      const uint32_t da = (ia & 2) ? ((ia & 1) ? wa : za) : ((ia & 1) ? ya : xa);
      const uint32_t db = (ib & 2) ? ((ib & 1) ? wb : zb) : ((ib & 1) ? yb : xb);
      va = (da >> (8 * (ta & 3))) & 0xFFu;
      vb = (db >> (8 * (tb & 3))) & 0xFFu;
    } else if (((uintptr_t)p & 3u) == 0) {  // 24 lanes, a dword each
      uint32_t q = 0;
      if (lane < 24) q = *reinterpret_cast<const uint32_t*>(p + 4 * lane);
      va = sig_byte_of<4>(q, ta);
      vb = sig_byte_of<4>(q, tb);
    } else {  // a byte per lane
      va = p[ta];
      vb = lane < 32 ? p[tb] : 0;
    }
    a = max((int)(int8_t)va, -127);
    b = max((int)(int8_t)vb, -127);
  } else {
    uint32_t ba, bb;  // the bytes that hold bits ta and tb
    if (((uintptr_t)p & 3u) == 0) {
      uint32_t q = 0;
      if (lane < 3) q = *reinterpret_cast<const uint32_t*>(p + 4 * lane);
      ba = sig_byte_of<4>(q, ta / 8);
      bb = sig_byte_of<4>(q, tb / 8);
    } else {
      uint32_t q = 0;
      if (lane < SIG_FIELD_BYTES) q = p[lane];
      ba = sig_byte_of<1>(q, ta / 8);
      bb = sig_byte_of<1>(q, tb / 8);
    }
    a = ((ba >> (7 - (ta & 7))) & 1u) ? 1 : -1;
    b = ((bb >> (7 - (tb & 7))) & 1u) ? 1 : -1;
  }
}

// The wave's packet k: res[k] = word | margin << 16.
//
// The 24 combined values c_j go to every lane.  The codeword's 24 bits are four slices of 6; lane x holds, per slice s,
// T_s[x] = the slice's part of the metric when the slice's bits are x -- four 64-entry tables, one entry per lane, so a
// metric is four cross-lane reads and three adds.  Lane l evaluates the 32 words w = 32 l + i, i = 0 .. 31 (bit 11
// clear): the codeword is linear, cw(w) = cw(32 l) ^ cw(i), and cw(i) is a constant of the unrolled loop.  The
// all-ones word is a codeword, so the word w ^ 0xFFF has the metric -m(w): the other 2048 come free.
template <bool SOFT>
__global__ __launch_bounds__(SIG_THREADS) void k_sig_decode(const uint8_t* __restrict__ in, const SigBlk* __restrict__ blk, uint32_t nblk,
                                                            uint32_t* __restrict__ res) {
  uint32_t k;
  SigBlk b;
  if (!sig_my_block(blk, nblk, k, b)) return;
  const uint32_t lane = (uint32_t)lane_id();
  if (b.len < SIG_FIELD_BYTES) {  // (wave-uniform)
    if (lane == 0) res[k] = OFDM_SIG_NO_WORD;
    return;
  }
  int va, vb;
  sig_load<SOFT>(in + b.in_off, lane, va, vb);
  // c_j in lane j < 24: field bits j, j + 24, j + 48 (lane j + 48, or b of lane j - 16), j + 72 (b of lane j + 8)
  const int a24 = __shfl(va, (int)((lane + 24) & 63u), WAVE), a48 = __shfl(va, (int)((lane + 48) & 63u), WAVE);
  const int b16 = __shfl(vb, (int)((lane - 16) & 63u), WAVE), b8 = __shfl(vb, (int)((lane + 8) & 63u), WAVE);
  const int c = va + a24 + (lane < 16 ? a48 : b16) + b8;
  int T[4] = {0, 0, 0, 0};
#pragma unroll
  for (int s = 0; s < 4; s++)
#pragma unroll
    for (int q = 0; q < 6; q++) {
      const int cj = __builtin_amdgcn_readlane(c, 6 * s + q);
      T[s] += ((lane >> (5 - q)) & 1u) ? cj : -cj;
    }
  const uint32_t cwl = sig_codeword(lane << 5);
  const int m0 = __shfl(T[0], (int)(cwl >> 18), WAVE);  // (bits 23 .. 18 are w >> 6: the same for every i)
  uint32_t k1 = 0, k2 = 0;                              // (no key is below 0, and every lane has 64 of them)
#pragma unroll
  for (uint32_t i = 0; i < 32; i++) {
    const uint32_t cw = cwl ^ sig_codeword(i);
    const int m = m0 + __shfl(T[1], (int)((cw >> 12) & 63u), WAVE) + __shfl(T[2], (int)((cw >> 6) & 63u), WAVE) +
                  __shfl(T[3], (int)(cw & 63u), WAVE);
    const uint32_t w = (lane << 5) | i;
    const uint32_t ka = sig_key(m, w), kb = sig_key(-m, w ^ (SIG_WORDS - 1));
    sig_top2(k1, k2, ka);
    sig_top2(k1, k2, kb);
  }
  // the lanes hold disjoint sets of words: the best two of two sets' best twos are the best two of their union
#pragma unroll
  for (int d = WAVE / 2; d > 0; d >>= 1) {
    const uint32_t o1 = (uint32_t)__shfl_xor((int)k1, d, WAVE), o2 = (uint32_t)__shfl_xor((int)k2, d, WAVE);
    k2 = max(min(k1, o1), max(k2, o2));
    k1 = max(k1, o1);
  }
  if (lane == 0) {
    const uint32_t word = SIG_WORDS - 1 - (k1 & (SIG_WORDS - 1)), margin = (k1 >> 12) - (k2 >> 12);
    res[k] = word | (margin << 16);
  }
}
