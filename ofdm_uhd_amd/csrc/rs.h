// rs.h -- the outer code of a concatenated link: Reed-Solomon over GF(2^8), 32 parity bytes per codeword (t = 16),
// byte-interleaved to the depth W a payload needs.  Works at the payload boundary like fec.h, above it and independent
// of it: no other kernel knows about it.  All arithmetic is integer: the result is defined bit for bit (DESIGN.md
// section 7; the definition is in include/ofdm_hip.h, "outer code").
//
//   field      GF(2^8) mod x^8 + x^4 + x^3 + x^2 + 1 (0x11d), alpha = 0x02
//   generator  g(x) = prod_{i = 0..31} (x - alpha^i)
//   block      k = n + 4 info bytes (payload | CRC-32 big-endian), W = ceil(k / 223) codewords; info byte i is symbol
//              i / W of codeword i mod W; parity byte j of codeword w at k + j W + w
//
// Layout of both kernels: one workgroup of four waves per block, the block staged in LDS once with 16-byte loads, one
// codeword per 32-lane half of a wave (lane i owns syndrome i, or parity register cell i), the codewords of a block
// in passes of eight.  Multiplication by a constant is an 8 x 8 bit matrix kept in two registers (RsCols): no table,
// no LDS traffic, no bank conflicts; a product of two variables builds the matrix of one factor first.
#pragma once
#include "common.h"
#include "host_util.h"
#include "rs_plan.h"

#define RS_THREADS 256
#define RS_HALVES (RS_THREADS / 32)
#define RS_LDS_BLOCK (OFDM_RS_MAX_CODED + 16)  // the block behind the up to 15 bytes that align it with its source

// host side (engine_rs.inc): CodecStage (host_util.h) and the code's own
struct RsState : CodecStage {
  DevBuf d_ok, d_corr, d_fail;
  std::vector<RsBlk> blk;
  // decoding with reliabilities (ofdm_rs_decode_rel, ofdm_rs_rel_from_soft): nothing of it exists before their first call
  DevBuf d_rel, d_reloff, d_sec, d_soft;
  std::vector<uint64_t> reloff;
  CodecClock rel_clock;  // of the last ofdm_rs_rel_from_soft
  void release() {
    DevBuf* bufs[] = {&d_ok, &d_corr, &d_fail, &d_rel, &d_reloff, &d_sec, &d_soft};
    for (DevBuf* b : bufs) b->release();
    rel_clock.release();
    CodecStage::release();
  }
};

// ---- the field's constants, made by the compiler --------------------------------------------------------------------
struct RsTables {
  uint8_t exp[256];  // alpha^e, e = 0 .. 255 (alpha^255 = 1)
  uint8_t gen[32];   // g_j, the coefficient of x^j of g(x); g_32 = 1
};
constexpr uint32_t rs_xtime_c(uint32_t a) { return ((a << 1) ^ ((a & 0x80u) ? 0x11du : 0u)) & 0xFFu; }
constexpr uint32_t rs_mul_c(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (int j = 0; j < 8; j++) {
    if (b & 1u) p ^= a;
    a = rs_xtime_c(a);
    b >>= 1;
  }
  return p;
}
constexpr RsTables rs_make_tables() {
  RsTables t{};
  uint32_t v = 1;
  for (int e = 0; e < 256; e++) {
    t.exp[e] = (uint8_t)v;
    v = rs_xtime_c(v);
  }
  uint32_t g[33] = {1};
  for (int i = 0; i < 32; i++) {  // times (x + alpha^i)
    for (int j = i + 1; j >= 1; j--) g[j] = g[j - 1] ^ rs_mul_c(g[j], t.exp[i]);
    g[0] = rs_mul_c(g[0], t.exp[i]);
  }
  for (int j = 0; j < 32; j++) t.gen[j] = (uint8_t)g[j];
  return t;
}
__constant__ RsTables rs_tab = rs_make_tables();

// ---- GF(2^8) in registers -------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t rs_xtime(uint32_t a) { return ((a << 1) ^ ((a >> 7) * 0x11du)) & 0xFFu; }

// the matrix of "times c": byte j of (lo | hi << 32) is c x^j
struct RsCols {
  uint32_t lo, hi;
};
__device__ __forceinline__ RsCols rs_cols(uint32_t c) {
  const uint32_t c1 = rs_xtime(c), c2 = rs_xtime(c1), c3 = rs_xtime(c2), c4 = rs_xtime(c3), c5 = rs_xtime(c4), c6 = rs_xtime(c5),
                 c7 = rs_xtime(c6);
  RsCols m;
  m.lo = c | (c1 << 8) | (c2 << 16) | (c3 << 24);
  m.hi = c4 | (c5 << 8) | (c6 << 16) | (c7 << 24);
  return m;
}
// c * x: bit j of x selects column j.  A nibble times 0x204081 puts its four bits at the feet of four bytes (the
// shifted copies do not overlap, the product fits 24-bit operands); times 255 makes byte masks of them.
__device__ __forceinline__ uint32_t rs_mulc(RsCols m, uint32_t x) {
  uint32_t a = __umul24(x & 0xFu, 0x204081u) & 0x01010101u;
  uint32_t b = __umul24(x >> 4, 0x204081u) & 0x01010101u;
  a = (a << 8) - a;
  b = (b << 8) - b;
  uint32_t v = (a & m.lo) ^ (b & m.hi);
  v ^= v >> 16;
  v ^= v >> 8;
  return v & 0xFFu;
}
__device__ __forceinline__ uint32_t rs_mul(uint32_t a, uint32_t b) { return rs_mulc(rs_cols(a), b); }
// a^254 = 1 / a (0 for 0)
__device__ __forceinline__ uint32_t rs_inv(uint32_t a) {
  const uint32_t a2 = rs_mul(a, a), a4 = rs_mul(a2, a2), a8 = rs_mul(a4, a4), a16 = rs_mul(a8, a8), a32 = rs_mul(a16, a16),
                 a64 = rs_mul(a32, a32), a128 = rs_mul(a64, a64);
  return rs_mul(rs_mul(rs_mul(a2, a4), rs_mul(a8, a16)), rs_mul(rs_mul(a32, a64), a128));
}
// XOR over the 32 lanes of a half
__device__ __forceinline__ uint32_t rs_half_xor(uint32_t v) {
#pragma unroll
  for (int d = 16; d > 0; d >>= 1) v ^= (uint32_t)__shfl_xor((int)v, d, 32);
  return v;
}
__device__ __forceinline__ uint32_t rs_half_sum(uint32_t v) {
#pragma unroll
  for (int d = 16; d > 0; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d, 32);
  return v;
}

// LDS written and then read by lanes of ONE wave: DS instructions of a wave execute in issue order, so no s_barrier is
// needed; the fences and the scheduling barrier keep the compiler's accesses on their side (as FftWaveSync, fft.h)
__device__ __forceinline__ void rs_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- staging --------------------------------------------------------------------------------------------------------
// `len` bytes from src to LDS so that byte i lies at lds[a + i], a = the source address mod 16: every 16-byte piece
// that lies whole inside the bytes is one aligned 16-byte load, the two edges go by bytes.  Nothing outside
// [src, src + len) is read.  Returns a.
__device__ __forceinline__ uint32_t rs_stage_in(uint8_t* lds, const uint8_t* __restrict__ src, uint32_t len, int tid) {
  const uint32_t a = (uint32_t)(reinterpret_cast<uintptr_t>(src) & 15u);
  const uint32_t end = a + len, nch = (end + 15u) >> 4;
  for (uint32_t c = (uint32_t)tid; c < nch; c += RS_THREADS) {
    const uint32_t lo = 16u * c;
    if (lo >= a && lo + 16u <= end) {
      *reinterpret_cast<uint4*>(lds + lo) = *reinterpret_cast<const uint4*>(src + (lo - a));
    } else {
      for (uint32_t o = (lo > a ? lo : a); o < lo + 16u && o < end; o++) lds[o] = src[o - a];
    }
  }
  return a;
}
// `len` bytes from lds (byte i at lds[i], any alignment) to dst: aligned 16-byte stores inside, bytes at the edges; one
// writer per byte, nothing outside [dst, dst + len) is written
__device__ __forceinline__ void rs_stage_out(uint8_t* __restrict__ dst, const uint8_t* lds, uint32_t len, int tid) {
  const uint32_t a = (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15u);
  const uint32_t end = a + len, nch = (end + 15u) >> 4;
  for (uint32_t c = (uint32_t)tid; c < nch; c += RS_THREADS) {
    const uint32_t lo = 16u * c;
    if (lo >= a && lo + 16u <= end) {
      const uint8_t* s = lds + (lo - a);
      uint32_t q[4];
#pragma unroll
      for (int d = 0; d < 4; d++)
        q[d] = (uint32_t)s[4 * d] | ((uint32_t)s[4 * d + 1] << 8) | ((uint32_t)s[4 * d + 2] << 16) | ((uint32_t)s[4 * d + 3] << 24);
      *reinterpret_cast<uint4*>(dst + (lo - a)) = make_uint4(q[0], q[1], q[2], q[3]);
    } else {
      for (uint32_t o = (lo > a ? lo : a); o < lo + 16u && o < end; o++) dst[o - a] = lds[o - a];
    }
  }
}

// CRC-32 of info[0, n) in LDS by RS_THREADS threads, 16 bytes each (256 * 16 >= OFDM_RS_MAX_PAYLOAD): XOR over the
// workgroup (crc_multmodp, common.h).  `red` holds one word per wave; two __syncthreads().
__device__ __forceinline__ uint32_t rs_crc(const uint8_t* info, uint32_t n, int tid, uint32_t* red, const uint32_t* __restrict__ crc_table,
                                           const uint32_t* __restrict__ xp8) {
  uint32_t acc = 0;
  const uint32_t o = 16u * (uint32_t)tid;
  if (o < n) {
    const uint32_t nb = (n - o < 16u) ? (n - o) : 16u;
    uint32_t crc = 0xFFFFFFFFu;
    for (uint32_t b = 0; b < nb; b++) crc = crc_table[(crc ^ info[o + b]) & 0xFFu] ^ (crc >> 8);
    crc ^= 0xFFFFFFFFu;
    acc = crc_multmodp(xp8[n - (o + nb)], crc);
  }
#pragma unroll
  for (int d = WAVE / 2; d > 0; d >>= 1) acc ^= __shfl_xor(acc, d, WAVE);
  if (lane_id() == 0) red[wave_id()] = acc;
  __syncthreads();
  uint32_t crc32 = 0;
#pragma unroll
  for (int w = 0; w < RS_THREADS / WAVE; w++) crc32 ^= red[w];
  __syncthreads();
  return crc32;
}

// ---------------------------------------------------------------------------------
// Encoder.  Payload to LDS, CRC behind it, then per codeword the division register of m(x) x^32 mod g(x): lane i holds
// the coefficient of x^i and multiplies the feedback by its own g_i; the shift is a lane shift within the half.  The
// parity goes to its interleaved place in LDS and the whole block leaves in 16-byte stores.
// ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(RS_THREADS) k_rs_encode(const uint8_t* __restrict__ payloads, const RsBlk* __restrict__ blk,
                                                          uint8_t* __restrict__ coded, const uint32_t* __restrict__ crc_table,
                                                          const uint32_t* __restrict__ xp8) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[RS_LDS_BLOCK];
  __shared__ uint32_t red[RS_THREADS / WAVE];
  const RsBlk b = blk[blockIdx.x];
  const uint32_t n = b.len;  // <= OFDM_RS_MAX_PAYLOAD (the host refuses longer ones)
  const uint32_t k = n + 4u, W = rs_words(k);
  const int tid = threadIdx.x;
  const uint32_t a = rs_stage_in(lds, payloads + b.in_off, n, tid);
  uint8_t* info = lds + a;  // a + k + 32 W <= 15 + OFDM_RS_MAX_CODED
  __syncthreads();
  const uint32_t crc32 = rs_crc(info, n, tid, red, crc_table, xp8);
  if (tid < 4) info[n + (uint32_t)tid] = (uint8_t)(crc32 >> (8 * (3 - tid)));  // struct.pack(">I", crc)
  __syncthreads();

  const uint32_t i = (uint32_t)tid & 31u, half = (uint32_t)tid >> 5;
  const RsCols gi = rs_cols(rs_tab.gen[i]);
  for (uint32_t base = 0; base < W; base += RS_HALVES) {
    const uint32_t w = base + half;
    const bool active = w < W;
    const uint32_t kw = active ? rs_cw_info(k, W, w) : 0u;  // (a half without a codeword runs no step)
    uint32_t reg = 0;
    for (uint32_t s = 0; s < kw; s++) {
      const uint32_t fb = (uint32_t)info[s * W + w] ^ (uint32_t)__shfl((int)reg, 31, 32);
      uint32_t up = (uint32_t)__shfl_up((int)reg, 1, 32);
      if (i == 0) up = 0;
      reg = up ^ rs_mulc(gi, fb);
    }
    if (active) info[k + (31u - i) * W + w] = (uint8_t)reg;  // parity byte j is the coefficient of x^(31 - j)
  }
  __syncthreads();
  rs_stage_out(coded + b.out_off, info, k + OFDM_RS_PARITY * W, tid);
}

// ---- what both decoders begin and end with.  SEC: with the `second` count and its per-codeword column s_sec, which
// only the decoder with reliabilities has (nullptr in the other) ----
// a length that is no block: every count 0, nothing else written
template <bool SEC>
__device__ __forceinline__ void rs_no_block(int tid, uint8_t* __restrict__ ok, uint32_t* __restrict__ corrected, uint32_t* __restrict__ failed,
                                            uint32_t* __restrict__ second) {
  if (tid == 0) {
    ok[blockIdx.x] = 0;
    corrected[blockIdx.x] = 0;
    failed[blockIdx.x] = 0;
    if (SEC) second[blockIdx.x] = 0;
  }
}
// the n payload bytes of the decoded block to dst, the CRC-32 of them held against the corrected CRC bytes, and the sums
// over the block's W codewords.  Follows the barrier behind the codeword loop.
template <bool SEC>
__device__ __forceinline__ void rs_finish(uint8_t* __restrict__ dst, const uint8_t* blkb, uint32_t n, uint32_t W, int tid, uint32_t* red,
                                          const uint32_t* s_corr, const uint32_t* s_fail, const uint32_t* s_sec, uint8_t* __restrict__ ok,
                                          uint32_t* __restrict__ corrected, uint32_t* __restrict__ failed, uint32_t* __restrict__ second,
                                          const uint32_t* __restrict__ crc_table, const uint32_t* __restrict__ xp8) {
  rs_stage_out(dst, blkb, n, tid);
  const uint32_t crc32 = rs_crc(blkb, n, tid, red, crc_table, xp8);
  if (tid == 0) {
    const uint32_t got = ((uint32_t)blkb[n] << 24) | ((uint32_t)blkb[n + 1u] << 16) | ((uint32_t)blkb[n + 2u] << 8) | (uint32_t)blkb[n + 3u];
    uint32_t c = 0, f = 0, s2 = 0;
    for (uint32_t w = 0; w < W; w++) {
      c += s_corr[w];
      f += s_fail[w];
      if (SEC) s2 += s_sec[w];
    }
    ok[blockIdx.x] = crc32 == got ? 1 : 0;
    corrected[blockIdx.x] = c;
    failed[blockIdx.x] = f;
    if (SEC) second[blockIdx.x] = s2;
  }
}

// ---------------------------------------------------------------------------------
// Decoder, per codeword (half of a wave):
//   syndromes  lane i runs Horner by its constant alpha^i over the codeword's k_w + 32 symbols, read from the staged
//              block at stride W (both halves read one byte each: broadcast reads).  A wave whose codewords all have
//              zero syndromes leaves here.
//   locator    Berlekamp-Massey without inversion (Lambda <- gamma Lambda - d x B), lane j holds coefficient j; the
//              discrepancy is an XOR over the half.  Lambda is a scalar multiple of the usual one: same roots, and the
//              scalar cancels in Forney's quotient.
//   roots      lane i tries the real positions i, i + 32, ...: Lambda(z) = E(z^2) + z O(z^2) at z = X^-1.  A root in the
//              shortened region is never found, so such a locator has fewer roots than its degree and fails.
//   Forney     e = Omega(z) / (z O(z^2)), Omega = S Lambda mod x^32 (first root alpha^0: X z cancels).
//   verdict    degree L <= 16 with L roots found: the L symbols are changed in LDS; else the codeword failed and stays.
// Then the n payload bytes leave, and the CRC-32 of them is held against the corrected CRC bytes (rs_finish).
// The steps from the locator to the verdict are rs_errors_only.inc, one text for this kernel and k_rs_decode_rel.
// ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(RS_THREADS) k_rs_decode(const uint8_t* __restrict__ coded, const RsBlk* __restrict__ blk,
                                                          uint8_t* __restrict__ payloads, uint8_t* __restrict__ ok,
                                                          uint32_t* __restrict__ corrected, uint32_t* __restrict__ failed,
                                                          const uint32_t* __restrict__ crc_table, const uint32_t* __restrict__ xp8) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[RS_LDS_BLOCK];
  __shared__ uint32_t red[RS_THREADS / WAVE];
  __shared__ uint32_t s_corr[RS_MAX_WORDS], s_fail[RS_MAX_WORDS];
  const RsBlk b = blk[blockIdx.x];
  const int tid = threadIdx.x;
  uint32_t k;
  if (!rs_info_len(b.len, &k)) return rs_no_block<false>(tid, ok, corrected, failed, nullptr);  // (uniform over the workgroup)
  const uint32_t n = k - 4u, W = rs_words(k);
  const uint32_t a = rs_stage_in(lds, coded + b.in_off, b.len, tid);
  uint8_t* blkb = lds + a;
#ifdef RS_SYNDROME_TABLE
  // experiment build (make variant NAME=rstab DEFS=-DRS_SYNDROME_TABLE): the syndromes' Horner step through a log /
  // antilog table in LDS in place of the bit matrix; measured next to it in DESIGN.md section 7, never the default
  __shared__ uint8_t t_exp[512], t_log[256];
  for (int t = tid; t < 510; t += RS_THREADS) t_exp[t] = rs_tab.exp[t % 255];
  if (tid < 255) t_log[rs_tab.exp[tid]] = (uint8_t)tid;
#define RS_SYN_STEP(S, r) (((S) ? (uint32_t)t_exp[(uint32_t)t_log[(S)] + i] : 0u) ^ (r))
#else
#define RS_SYN_STEP(S, r) (rs_mulc(ai, (S)) ^ (r))
#endif
  __syncthreads();

  const uint32_t i = (uint32_t)tid & 31u, half = (uint32_t)tid >> 5;
  [[maybe_unused]] const RsCols ai = rs_cols(rs_tab.exp[i]);
  for (uint32_t base = 0; base < W; base += RS_HALVES) {
    const uint32_t w = base + half;
    const bool active = w < W;
    const uint32_t kw = active ? rs_cw_info(k, W, w) : 0u;  // (a half without a codeword sees the empty word: clean)
    const uint32_t len = active ? kw + OFDM_RS_PARITY : 0u;
    // ---- syndromes S_i = r(alpha^i) ----
    uint32_t S = 0;
    for (uint32_t s = 0; s < kw; s++) S = RS_SYN_STEP(S, (uint32_t)blkb[s * W + w]);
    for (uint32_t s = kw; s < len; s++) S = RS_SYN_STEP(S, (uint32_t)blkb[k + (s - kw) * W + w]);
    if (__ballot(S != 0) == 0ull) {  // clean input, the common case: wave-uniform
      if (active && i == 0) {
        s_corr[w] = 0;
        s_fail[w] = 0;
      }
      continue;
    }
    const bool dirty = rs_half_sum(S != 0 ? 1u : 0u) != 0;
    uint32_t L;  // locator, roots, Forney, verdict
    bool good;
    {
#include "rs_errors_only.inc"
    }
    if (active && i == 0) {
      s_corr[w] = good ? L : 0u;
      s_fail[w] = (dirty && !good) ? 1u : 0u;
    }
  }
  __syncthreads();

  rs_finish<false>(payloads + b.out_off, blkb, n, W, tid, red, s_corr, s_fail, nullptr, ok, corrected, failed, nullptr, crc_table, xp8);
}

// ---------------------------------------------------------------------------------
// Decoder with reliabilities (include/ofdm_hip.h, "decoding with reliabilities").  k_rs_decode's layout and, as the first
// pass, k_rs_decode's steps: syndromes by the same Horner loop, then the same rs_errors_only.inc; the block's reliability
// bytes are staged next to it.  Two wave-uniform exits: clean input, and no half of the wave failing the first pass.
// A half whose codeword failed goes on:
//   threshold  tau* by an 8-step search upwards bit by bit; each step counts over the lane's <= 8 positions and sums over
//              the half.  f = c(tau*) positions are erased
//   erasures   their X = alpha^deg, compacted by ballot ranks into 32 bytes of LDS per half (written and read by the
//              half's own wave: rs_wave_sync)
//   Gamma      prod (1 - X_j x) by f steps of shift-and-multiply.  A polynomial of degree <= 32 lies on a half with
//              coefficient i + 1 in lane i and coefficient 0 in a register of its own, equal in every lane
//   Psi        Berlekamp-Massey without inversion started from lambda = B = Gamma, L = f, rounds f .. 31: always a
//              multiple of Gamma, so the erased positions are roots by construction
//   roots      as the first pass with Psi_0 .. Psi_32 and Omega_0 .. Omega_31 = S Psi mod x^32 copied to every lane; the
//              eight positions of a lane in a loop that is not unrolled, the eight errata values packed in two registers
//   verdict    2 (L - f) + f <= 32 and L roots found: the non-zero errata values are applied, one writer per byte
// ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(RS_THREADS) k_rs_decode_rel(const uint8_t* __restrict__ coded, const uint8_t* __restrict__ rel,
                                                              const RsBlk* __restrict__ blk, const uint64_t* __restrict__ rel_off,
                                                              uint32_t M, uint8_t* __restrict__ payloads, uint8_t* __restrict__ ok,
                                                              uint32_t* __restrict__ corrected, uint32_t* __restrict__ failed,
                                                              uint32_t* __restrict__ second, const uint32_t* __restrict__ crc_table,
                                                              const uint32_t* __restrict__ xp8) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[RS_LDS_BLOCK];
  __shared__ __attribute__((aligned(16))) uint8_t lds_rel[RS_LDS_BLOCK];
  __shared__ uint32_t red[RS_THREADS / WAVE];
  __shared__ uint32_t s_corr[RS_MAX_WORDS], s_fail[RS_MAX_WORDS], s_sec[RS_MAX_WORDS];
  __shared__ uint8_t s_x[RS_HALVES][32];
  const RsBlk b = blk[blockIdx.x];
  const int tid = threadIdx.x;
  uint32_t k;
  if (!rs_info_len(b.len, &k)) return rs_no_block<true>(tid, ok, corrected, failed, second);  // (uniform over the workgroup)
  const uint32_t n = k - 4u, W = rs_words(k);
  const uint32_t a = rs_stage_in(lds, coded + b.in_off, b.len, tid);
  const uint32_t ar = rs_stage_in(lds_rel, rel + rel_off[blockIdx.x], b.len, tid);
  uint8_t* blkb = lds + a;
  const uint8_t* relb = lds_rel + ar;
  __syncthreads();

  const uint32_t i = (uint32_t)tid & 31u, half = (uint32_t)tid >> 5;
  const RsCols ai = rs_cols(rs_tab.exp[i]);
  for (uint32_t base = 0; base < W; base += RS_HALVES) {
    const uint32_t w = base + half;
    const bool active = w < W;
    const uint32_t kw = active ? rs_cw_info(k, W, w) : 0u;  // (a half without a codeword sees the empty word: clean)
    const uint32_t len = active ? kw + OFDM_RS_PARITY : 0u;
    // ---- first pass: syndromes, then the errors-only pass ----
    uint32_t S = 0;
    for (uint32_t s = 0; s < kw; s++) S = rs_mulc(ai, S) ^ (uint32_t)blkb[s * W + w];
    for (uint32_t s = kw; s < len; s++) S = rs_mulc(ai, S) ^ (uint32_t)blkb[k + (s - kw) * W + w];
    if (__ballot(S != 0) == 0ull) {  // clean input, the common case: wave-uniform
      if (active && i == 0) {
        s_corr[w] = 0;
        s_fail[w] = 0;
        s_sec[w] = 0;
      }
      continue;
    }
    const bool dirty = rs_half_sum(S != 0 ? 1u : 0u) != 0;
    uint32_t L;
    bool good;
    {
#include "rs_errors_only.inc"
    }
    const bool fail1 = dirty && !good;
    if (__ballot(fail1) == 0ull) {  // the first pass decoded every codeword of the wave: wave-uniform
      if (active && i == 0) {
        s_corr[w] = good ? L : 0u;
        s_fail[w] = 0;
        s_sec[w] = 0;
      }
      continue;
    }

    // ---- second pass.  Both halves of the wave run every step, the lane exchanges stay inside a half; a half that
    // did not fail computes on nothing and changes nothing (sec is false) ----
    uint32_t rq[8];  // reliabilities of the lane's positions, 256 where there is none
#pragma unroll
    for (int q = 0; q < 8; q++) {
      const uint32_t p = i + 32u * (uint32_t)q;
      rq[q] = p < len ? (uint32_t)relb[p < kw ? p * W + w : k + (p - kw) * W + w] : 256u;
    }
    uint32_t tau = 0, f = 0, c0;
    {
      uint32_t c = 0;
#pragma unroll
      for (int q = 0; q < 8; q++) c += rq[q] == 0u ? 1u : 0u;
      c0 = f = rs_half_sum(c);
    }
#pragma unroll 1
    for (int bit = 7; bit >= 0; bit--) {  // the largest tau in 0 .. 254 with c(tau) <= M, given c(0) <= M
      const uint32_t cand = tau | (1u << bit);
      uint32_t c = 0;
#pragma unroll
      for (int q = 0; q < 8; q++) c += rq[q] <= cand ? 1u : 0u;
      c = rs_half_sum(c);
      const bool take = cand <= 254u && c <= M;
      tau = take ? cand : tau;
      f = take ? c : f;
    }
    const bool sec = fail1 && c0 <= M && f >= 1u;  // (f <= M <= 32)
    {
      uint32_t at = 0;
#pragma unroll
      for (int q = 0; q < 8; q++) {
        const bool er = sec && rq[q] <= tau;
        const uint32_t m = (uint32_t)(__ballot(er) >> (32u * (half & 1u)));
        if (er) s_x[half][at + (uint32_t)__popc(m & ((1u << i) - 1u))] = rs_tab.exp[len - 1u - (i + 32u * (uint32_t)q)];  // rank < f <= 32
        at += (uint32_t)__popc(m);
      }
    }
    rs_wave_sync();
    uint32_t ps = 0, ps0 = 1;  // Gamma: coefficient i + 1 here, coefficient 0 is 1
#pragma unroll 1
    for (uint32_t j = 0; j < OFDM_RS_PARITY; j++) {
      const uint32_t X = s_x[half][j];  // (beyond f: whatever lies there, unused)
      uint32_t dn = (uint32_t)__shfl_up((int)ps, 1, 32);
      if (i == 0) dn = 1u;
      const uint32_t t = ps ^ rs_mul(X, dn);
      ps = j < f ? t : ps;
    }
    rs_wave_sync();  // (the next pass of the loop writes s_x again)
    uint32_t Bp = ps, Bp0 = 1, L2 = f, gam2 = 1;
#pragma unroll 1
    for (uint32_t r = 0; r < OFDM_RS_PARITY; r++) {
      uint32_t sv = (uint32_t)__shfl((int)S, (int)((r - 1u - i) & 31u), 32);
      sv = i + 1u <= r ? sv : 0u;
      const uint32_t Sr = (uint32_t)__shfl((int)S, (int)r, 32);
      const uint32_t d = rs_half_xor(rs_mul(ps, sv)) ^ rs_mul(ps0, Sr);
      uint32_t Bs = (uint32_t)__shfl_up((int)Bp, 1, 32);
      if (i == 0) Bs = Bp0;  // x B: its coefficient i + 1 is B's coefficient i
      const uint32_t T = rs_mul(gam2, ps) ^ rs_mul(d, Bs);
      const uint32_t T0 = rs_mul(gam2, ps0);
      const bool run = r >= f;
      const bool upd = run && d != 0 && 2u * L2 <= r + f;
      Bp = run ? (upd ? ps : Bs) : Bp;
      Bp0 = run ? (upd ? ps0 : 0u) : Bp0;
      gam2 = upd ? d : gam2;
      L2 = upd ? r + 1u - L2 + f : L2;
      ps = run ? T : ps;
      ps0 = run ? T0 : ps0;
    }
    uint32_t pc[33], om[32];
    pc[0] = ps0;
#pragma unroll
    for (int j = 1; j < 33; j++) pc[j] = (uint32_t)__shfl((int)ps, j - 1, 32);
    {
      uint32_t acc = 0;  // Omega_i = sum_{j <= i} Psi_j S_(i - j), in lane i
#pragma unroll
      for (int j = 0; j < 32; j++) {
        const uint32_t sv = (uint32_t)__shfl((int)S, (int)((i - (uint32_t)j) & 31u), 32);
        acc ^= (uint32_t)j <= i ? rs_mul(pc[j], sv) : 0u;
      }
#pragma unroll
      for (int j = 0; j < 32; j++) om[j] = (uint32_t)__shfl((int)acc, j, 32);
    }
    const bool try2 = sec && 2u * L2 <= OFDM_RS_PARITY + f;  // 2 e + f <= 32 with e = L - f
    uint32_t elo = 0, ehi = 0, nroot2 = 0;
#pragma unroll 1
    for (uint32_t q = 0; q < 8u; q++) {
      const uint32_t p = i + 32u * q;
      if (try2 && p < len) {
        const uint32_t deg = len - 1u - p;
        const uint32_t z = rs_tab.exp[deg ? 255u - deg : 0u];
        const RsCols cz = rs_cols(z);
        const RsCols cy = rs_cols(rs_mulc(cz, z));
        uint32_t E = pc[32], O = pc[31];
#pragma unroll
        for (int j = 14; j >= 0; j--) {
          E = rs_mulc(cy, E) ^ pc[2 * j + 2];
          O = rs_mulc(cy, O) ^ pc[2 * j + 1];
        }
        E = rs_mulc(cy, E) ^ pc[0];
        const uint32_t zO = rs_mulc(cz, O);
        if ((E ^ zO) == 0u) {
          nroot2++;
          uint32_t v = om[31];
#pragma unroll
          for (int j = 30; j >= 0; j--) v = rs_mulc(cz, v) ^ om[j];
          const uint32_t e = rs_mul(v, rs_inv(zO)) << (8u * (q & 3u));
          elo |= q < 4u ? e : 0u;
          ehi |= q < 4u ? 0u : e;
        }
      }
    }
    nroot2 = rs_half_sum(nroot2);
    const bool good2 = try2 && nroot2 == L2;
    uint32_t changed = 0;
#pragma unroll 1
    for (uint32_t q = 0; q < 8u; q++) {
      const uint32_t e = ((q < 4u ? elo : ehi) >> (8u * (q & 3u))) & 0xFFu;
      if (good2 && e) {  // (only where p < len) one writer per byte: position p of codeword w is this lane's alone
        const uint32_t p = i + 32u * q;
        const uint32_t at = p < kw ? p * W + w : k + (p - kw) * W + w;
        blkb[at] = (uint8_t)((uint32_t)blkb[at] ^ e);
        changed++;
      }
    }
    changed = rs_half_sum(changed);
    if (active && i == 0) {
      s_corr[w] = fail1 ? changed : (good ? L : 0u);
      s_fail[w] = (fail1 && !good2) ? 1u : 0u;
      s_sec[w] = good2 ? 1u : 0u;
    }
  }
  __syncthreads();

  rs_finish<true>(payloads + b.out_off, blkb, n, W, tid, red, s_corr, s_fail, s_sec, ok, corrected, failed, second, crc_table, xp8);
}

// ---------------------------------------------------------------------------------
// Reliabilities from soft values: byte m of a block gets the smallest |v| of its eight values (rs_rel_of_values).  One
// workgroup per block; a thread turns 32 values into the 4 bytes of one aligned word of the output: two 16-byte loads
// where the values lie on a 16-byte boundary (four 8-byte loads where on an 8-byte one), one 4-byte store.  The up to
// three bytes before the first aligned word and behind the last one go by bytes.  Value offsets are multiples of 8 (the
// host refuses others).  Nothing outside the blocks is read or written.
// ---------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t rs_rel_of_words(uint32_t lo, uint32_t hi) {
  uint32_t m = 127u;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int x = (int)(int8_t)(lo >> (8 * j)), y = (int)(int8_t)(hi >> (8 * j));
    const uint32_t ax = (uint32_t)(x < 0 ? -x : x), ay = (uint32_t)(y < 0 ? -y : y);
    m = min(m, min(ax, ay));
  }
  return m;
}

__global__ void __launch_bounds__(RS_THREADS) k_rs_rel_soft(const int8_t* __restrict__ soft, const RsBlk* __restrict__ blk,
                                                            uint8_t* __restrict__ rel) {
  const RsBlk b = blk[blockIdx.x];
  const int8_t* v = soft + b.in_off;
  uint8_t* out = rel + b.out_off;
  const uint32_t n = b.len;
  const uint32_t lead = (uint32_t)((4u - (uint32_t)(reinterpret_cast<uintptr_t>(out) & 3u)) & 3u);
  const uint32_t head = lead < n ? lead : n;
  const uint32_t nword = (n - head) >> 2, tail = (n - head) & 3u;
  const uint32_t tid = threadIdx.x;
  for (uint32_t g = tid; g < nword; g += RS_THREADS) {
    const uint32_t m = head + 4u * g;
    const int8_t* s = v + 8ull * m;
    uint32_t q[8];
    const uintptr_t al = reinterpret_cast<uintptr_t>(s);
    if ((al & 15u) == 0) {
      const uint4 x = *reinterpret_cast<const uint4*>(s), y = *reinterpret_cast<const uint4*>(s + 16);
      q[0] = x.x, q[1] = x.y, q[2] = x.z, q[3] = x.w, q[4] = y.x, q[5] = y.y, q[6] = y.z, q[7] = y.w;
    } else if ((al & 7u) == 0) {
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const uint2 x = *reinterpret_cast<const uint2*>(s + 8 * j);
        q[2 * j] = x.x, q[2 * j + 1] = x.y;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 8; j++)
        q[j] = (uint32_t)(uint8_t)s[4 * j] | ((uint32_t)(uint8_t)s[4 * j + 1] << 8) | ((uint32_t)(uint8_t)s[4 * j + 2] << 16) |
               ((uint32_t)(uint8_t)s[4 * j + 3] << 24);
    }
    *reinterpret_cast<uint32_t*>(out + m) = rs_rel_of_words(q[0], q[1]) | (rs_rel_of_words(q[2], q[3]) << 8) |
                                            (rs_rel_of_words(q[4], q[5]) << 16) | (rs_rel_of_words(q[6], q[7]) << 24);
  }
  if (tid < head + tail) {  // at most six bytes at the two edges
    const uint32_t m = tid < head ? tid : head + 4u * nword + (tid - head);
    out[m] = (uint8_t)rs_rel_of_values(v + 8ull * m);
  }
}
