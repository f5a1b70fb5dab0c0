// punct_plan.h -- the host arithmetic of the punctured rates of the coded-link layer (fec_punct.h / engine_fec.inc): the
// three 802.11 patterns over the mother coded bits, kept-bit counts and block lengths with their inverse, the column
// count of a punctured block's interleaver, rank / unrank between mother and kept indices, and the batch layouts.
// Plain C++ without a HIP include, so that a stand-alone program can check it (tools/punct_plan_check.cpp).
//
//   mother bits  c[0 .. 2T), T = 8(n+4) + 6: 2T = 16n + 76 (fec.h); bit i is kept when bit (i mod period) of the mask is set
//   kept stream  p[q] = c[unrank(q)], q < K; P = ceil(K / 8) bytes, p[q] = 0 for K <= q < 8P
//   sent bit j   = p[(j mod R') * C' + j / R'], R' = 8P / C', C' the largest power of two <= interleave_cols dividing 8P
#pragma once
#include "fec_plan.h"

// per rate (index = OFDM_FEC_RATE_*; entry 0, the mother code, keeps everything)
constexpr uint32_t PUNCT_PERIOD[4] = {2, 4, 6, 10};
constexpr uint32_t PUNCT_KEPT[4] = {2, 3, 4, 6};                  // kept bits of one period
constexpr uint32_t PUNCT_MASK[4] = {0x3u, 0x7u, 0x27u, 0x267u};   // bit r: position r of a period is kept
constexpr uint32_t PUNCT_NIB[4] = {0x10u, 0x210u, 0x5210u, 0x965210u};  // nibble k: the k-th kept position of a period

FEC_HD static inline bool punct_rate_ok(uint32_t rate) { return rate <= OFDM_FEC_RATE_5_6; }

// mother coded bits of an n-byte payload (the four pad bits behind them are not among them)
FEC_HD static inline uint32_t punct_mother_bits(uint32_t n) { return 16u * n + 76u; }

template <uint32_t RATE>
FEC_HD static inline bool punct_kept(uint32_t i) {
  return (PUNCT_MASK[RATE] >> (i % PUNCT_PERIOD[RATE])) & 1u;
}
// kept bits in front of mother bit i (its kept index, where it is kept itself)
template <uint32_t RATE>
FEC_HD static inline uint32_t punct_rank(uint32_t i) {
  const uint32_t r = i % PUNCT_PERIOD[RATE];
  return (i / PUNCT_PERIOD[RATE]) * PUNCT_KEPT[RATE] + (uint32_t)__builtin_popcount(PUNCT_MASK[RATE] & ((1u << r) - 1u));
}
// mother index of kept bit q
template <uint32_t RATE>
FEC_HD static inline uint32_t punct_unrank(uint32_t q) {
  return (q / PUNCT_KEPT[RATE]) * PUNCT_PERIOD[RATE] + ((PUNCT_NIB[RATE] >> (4u * (q % PUNCT_KEPT[RATE]))) & 15u);
}
// kept bits K and block bytes P of an n-byte payload
template <uint32_t RATE>
FEC_HD static inline uint32_t punct_kept_bits(uint32_t n) {
  return punct_rank<RATE>(punct_mother_bits(n));
}
template <uint32_t RATE>
FEC_HD static inline uint32_t punct_block_len(uint32_t n) {
  return (punct_kept_bits<RATE>(n) + 7u) >> 3;
}

// the same by a run-time rate (host side; the kernels take the rate as a template argument)
#define PUNCT_BY_RATE(rate, expr1, expr2, expr3) ((rate) == 1 ? (expr1) : (rate) == 2 ? (expr2) : (expr3))
static inline uint32_t punct_kept_bits_rt(uint32_t rate, uint32_t n) {
  return PUNCT_BY_RATE(rate, punct_kept_bits<1>(n), punct_kept_bits<2>(n), punct_kept_bits<3>(n));
}
static inline uint32_t punct_block_len_rt(uint32_t rate, uint32_t n) {
  return PUNCT_BY_RATE(rate, punct_block_len<1>(n), punct_block_len<2>(n), punct_block_len<3>(n));
}
static inline uint32_t punct_rank_rt(uint32_t rate, uint32_t i) {
  return PUNCT_BY_RATE(rate, punct_rank<1>(i), punct_rank<2>(i), punct_rank<3>(i));
}
static inline uint32_t punct_unrank_rt(uint32_t rate, uint32_t q) {
  return PUNCT_BY_RATE(rate, punct_unrank<1>(q), punct_unrank<2>(q), punct_unrank<3>(q));
}
static inline bool punct_kept_rt(uint32_t rate, uint32_t i) {
  return PUNCT_BY_RATE(rate, punct_kept<1>(i), punct_kept<2>(i), punct_kept<3>(i));
}

// P(n) at any rate, 0 = the mother code's 2n + 10
static inline int punct_coded_len(uint32_t rate, uint32_t payload_len, uint32_t* coded_len) {
  if (!punct_rate_ok(rate)) return OFDM_E_INVAL;
  if (rate == OFDM_FEC_RATE_1_2) return fec_coded_len(payload_len, coded_len);
  if (!coded_len || payload_len > OFDM_FEC_MAX_PAYLOAD) return OFDM_E_INVAL;
  *coded_len = punct_block_len_rt(rate, payload_len);
  return OFDM_OK;
}

// The inverse.  P is strictly increasing in n (steps of 1 or 2), so a length names at most one n; a length P never
// reaches is no block.  K = 8P - (0..7) kept bits stand for 8P * period / kept mother bits, give or take a period, and
// 16 mother bits make a payload byte: the estimate is off by one at most, the two neighbours on either side are tried.
static inline int punct_payload_len(uint32_t rate, uint32_t coded_len, uint32_t* payload_len) {
  if (!punct_rate_ok(rate)) return OFDM_E_INVAL;
  if (rate == OFDM_FEC_RATE_1_2) return fec_payload_len(coded_len, payload_len);
  if (!payload_len || coded_len > OFDM_FEC_MAX_CODED) return OFDM_E_INVAL;
  const uint32_t bits = 8u * coded_len * PUNCT_PERIOD[rate] / PUNCT_KEPT[rate];
  const uint32_t n0 = bits > 76u ? (bits - 76u) / 16u : 0u;
  const int32_t order[5] = {0, 1, -1, 2, -2};  // the likeliest first
  for (int32_t d : order) {
    const int64_t n = (int64_t)n0 + d;
    if (n < 0 || n > (int64_t)OFDM_FEC_MAX_PAYLOAD) continue;
    if (punct_block_len_rt(rate, (uint32_t)n) == coded_len) {
      *payload_len = (uint32_t)n;
      return OFDM_OK;
    }
  }
  return OFDM_E_INVAL;
}

// log2 of C': the caller's columns, or 8 where they are 16 and the block has an odd number of bytes
FEC_HD static inline uint32_t punct_log2_cols(uint32_t lgC, uint32_t block_len) { return (lgC == 4u && (block_len & 1u)) ? 3u : lgC; }

// Layout of a punctured encode batch: FecBlk k = {payload offset, block offset, payload bytes}; out_off[0..nblk].
// Returns the total block bytes, or ~0 where a payload is longer than OFDM_FEC_MAX_PAYLOAD; *in_extent: payload bytes read.
static inline uint64_t punct_plan_encode(uint32_t rate, const uint64_t* in_off, const uint32_t* payload_len, uint64_t nblk, FecBlk* blk,
                                         uint64_t* out_off, uint64_t* in_extent) {
  uint64_t o = 0, ext = 0;
  for (uint64_t k = 0; k < nblk; k++) {
    uint32_t P = 0;
    if (punct_coded_len(rate, payload_len[k], &P) != OFDM_OK) return ~0ull;
    blk[k] = FecBlk{in_off[k], o, payload_len[k], 0};
    out_off[k] = o;
    o += P;
    if (in_off[k] + payload_len[k] > ext) ext = in_off[k] + payload_len[k];
  }
  out_off[nblk] = o;
  *in_extent = ext;
  return o;
}

// Layout of a punctured decode batch over slices of `per` blocks (fec_slice_blocks).  Two tables:
//   pblk[k]  what k_fec_depuncture reads: in_off into the caller's blob, out_off into the mother-value buffer (the
//            block's place in its slice: (k mod per) * mother_stride), len = the punctured length as given, pad = the
//            mother block's bytes 2n + 10, or 0 for a length that is no block at this rate
//   mblk[k]  what k_fec_decode<true> reads at one column: in_off = the same place in the mother-value buffer,
//            out_off into the payloads, len = 2n + 10, or 0 (no block to the decoder either)
// punct_plan_decode_sizes runs first: payload offsets, the widest block's workspace stride in words, its mother values
// (8 per mother byte, a multiple of 16) and the input the valid blocks reach (`unit` items per byte: 1 hard, 8 soft).
static inline uint64_t punct_plan_decode_sizes(uint32_t rate, const uint64_t* in_off, const uint32_t* coded_len, uint64_t nblk,
                                               uint64_t unit, FecBlk* pblk, uint64_t* out_off, uint64_t* stride_words,
                                               uint64_t* mother_stride, uint64_t* in_extent) {
  uint64_t o = 0, stride = 0, ms = 0, ext = 0;
  uint32_t last_len = 0, n = 0;  // a batch mostly repeats its lengths: the inverse of the block before is kept
  bool is = false;
  for (uint64_t k = 0; k < nblk; k++) {
    if (k == 0 || coded_len[k] != last_len) {
      last_len = coded_len[k];
      is = punct_payload_len(rate, last_len, &n) == OFDM_OK;
    }
    const uint32_t mlen = is ? 2u * n + 10u : 0u;
    pblk[k] = FecBlk{in_off[k], 0, coded_len[k], mlen};
    out_off[k] = o;
    if (is) {
      o += n;
      const uint64_t w = 64ull * fec_chunks(mlen);
      if (w > stride) stride = w;
      if (8ull * mlen > ms) ms = 8ull * mlen;
      const uint64_t e = in_off[k] + unit * coded_len[k];
      if (e > ext) ext = e;
    }
  }
  out_off[nblk] = o;
  *stride_words = stride;
  *mother_stride = ms;
  *in_extent = ext;
  return o;
}
static inline void punct_plan_decode_slots(uint64_t nblk, uint64_t per, uint64_t mother_stride, const uint64_t* out_off, FecBlk* pblk,
                                           FecBlk* mblk) {
  uint64_t slot = 0;  // k mod per
  for (uint64_t k = 0; k < nblk; k++) {
    const uint64_t at = slot * mother_stride;
    pblk[k].out_off = at;
    mblk[k] = FecBlk{at, out_off[k], pblk[k].pad, 0};
    if (++slot == per) slot = 0;
  }
}
