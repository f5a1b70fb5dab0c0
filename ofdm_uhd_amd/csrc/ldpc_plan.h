// ldpc_plan.h -- the host arithmetic of the LDPC coded-link layer (ldpc.h / engine_ldpc.inc): the base matrices of the four
// rates, block lengths, and the codeword map of a batch (block -> first codeword, codeword -> block, info bytes per
// codeword).  Every function takes the rate (OFDM_LDPC_RATE_*); the names without _rate are the rate-1/2 case.
// Plain C++ without a HIP include, so that a stand-alone program can check it (tools/ldpc_plan_check.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/ofdm_hip.h"

#ifdef __HIPCC__
#define LDPC_HD __host__ __device__
#else
#define LDPC_HD
#endif

constexpr int LDPC_Z = 64;                        // circulant size: one circulant is one wave
constexpr int LDPC_ROWS = 12, LDPC_COLS = 24;     // base matrix at rate 1/2; the other rates have fewer, longer rows
constexpr uint32_t LDPC_CW_INFO = 96;             // info bytes of a full codeword at rate 1/2 (768 bits)
constexpr uint32_t LDPC_CW_PARITY = 96;           // parity bytes of every codeword at rate 1/2
constexpr uint32_t LDPC_CW_SENT = 192;            // a full codeword on the air, at every rate
constexpr uint32_t LDPC_MAX_WORDS = 21;           // codewords of the longest block
constexpr int LDPC_MAX_DEG = 19;                  // longest row (rate 5/6); 7 at rate 1/2
constexpr uint32_t LDPC_DEFAULT_ITERS = 20, LDPC_MAX_ITERS = 64;
constexpr uint32_t LDPC_RATES = 4;                // OFDM_LDPC_RATE_1_2 .. OFDM_LDPC_RATE_5_6

// rows mb of the base matrix at a rate; kb = 24 - mb info columns, 8 kb info bytes and 8 mb parity bytes per codeword
LDPC_HD constexpr uint32_t ldpc_rate_rows(uint32_t rate) { return rate == OFDM_LDPC_RATE_1_2 ? 12u : rate == OFDM_LDPC_RATE_2_3 ? 8u : rate == OFDM_LDPC_RATE_3_4 ? 6u : 4u; }
LDPC_HD constexpr uint32_t ldpc_rate_info(uint32_t rate) { return 8u * ((uint32_t)LDPC_COLS - ldpc_rate_rows(rate)); }
LDPC_HD constexpr uint32_t ldpc_rate_parity(uint32_t rate) { return 8u * ldpc_rate_rows(rate); }
LDPC_HD constexpr uint32_t ldpc_rate_max_payload(uint32_t rate) { return LDPC_MAX_WORDS * ldpc_rate_info(rate) - 4u; }
static_assert(ldpc_rate_max_payload(OFDM_LDPC_RATE_1_2) == OFDM_LDPC_MAX_PAYLOAD, "21 codewords of 96 info bytes");
static_assert(ldpc_rate_max_payload(OFDM_LDPC_RATE_2_3) == 2684 && ldpc_rate_max_payload(OFDM_LDPC_RATE_3_4) == 3020 &&
                  ldpc_rate_max_payload(OFDM_LDPC_RATE_5_6) == 3356,
              "largest payloads of the other rates");

// The base matrix: shift[i][j] of row i and column j, -1 for no entry; per row its entries in column order.
struct LdpcTable {
  int8_t shift[LDPC_ROWS][LDPC_COLS];
  int deg[LDPC_ROWS];
  int col[LDPC_ROWS][LDPC_MAX_DEG];
  int sh[LDPC_ROWS][LDPC_MAX_DEG];
  int entries;
  int mb, kb, mid, max_deg;  // rows, info columns, the row of column kb's middle entry, the longest row
};

// info shifts of the four rates, -1 for no entry (include/ofdm_hip.h, "coded links: LDPC")
struct LdpcInfoShifts {
  int8_t s[LDPC_ROWS][20];
};
constexpr LdpcInfoShifts ldpc_info_shifts(uint32_t rate) {
  constexpr int8_t X = -1;
  switch (rate) {
    case OFDM_LDPC_RATE_1_2:
      return LdpcInfoShifts{{
          {X, 1, X, X, 25, X, X, 42, X, 59, X, 24},   {X, X, X, 17, 48, X, X, X, 37, X, 21, 42}, {2, X, X, X, X, X, 0, X, 56, X, 20, 50},
          {X, 52, X, X, X, 5, X, X, 45, 19, 45, X},   {X, X, 34, X, X, X, 30, X, 29, 31, X, 55}, {17, X, X, X, X, X, 5, X, 53, X, 21, 36},
          {X, X, X, X, X, X, 25, 16, X, 22, X, X},    {X, X, 38, X, X, 54, X, 48, X, 56, 3, X},  {X, 58, X, X, X, X, X, 7, 60, 36, X, 20},
          {X, X, X, 59, 35, X, X, X, X, 46, 38, 25},  {40, X, X, 42, X, X, X, X, 24, 33, 16, X}, {X, X, 46, X, X, 1, X, X, 51, X, 25, 5},
      }};
    case OFDM_LDPC_RATE_2_3:
      return LdpcInfoShifts{{
          {X, 1, 61, X, 10, X, X, 43, X, X, 15, X, X, 28, X, X},
          {7, 21, X, 32, X, 25, X, X, X, X, 60, X, 56, X, 16, X},
          {30, X, 37, X, 4, X, 12, X, 58, X, X, 14, X, X, 2, X},
          {34, X, X, 9, X, 4, 47, X, 9, X, X, X, 10, X, 23, X},
          {X, X, X, 14, X, 28, X, 47, X, 58, X, X, 5, X, X, 42},
          {X, 13, 43, X, X, 11, 13, X, X, X, 63, 36, X, 16, X, X},
          {X, 12, X, 61, 57, X, X, X, 0, 19, X, X, X, 35, X, 50},
          {0, X, 29, X, 16, X, X, 21, X, 12, X, 43, X, X, X, 41},
      }};
    case OFDM_LDPC_RATE_3_4:
      return LdpcInfoShifts{{
          {40, 21, 5, X, X, 7, 42, X, 18, X, X, 24, 0, X, 5, X, X, 40},
          {0, X, 58, X, 60, 1, 28, X, X, 27, 10, X, 27, X, 40, X, 61, X},
          {X, 1, 39, 26, X, 25, X, 23, 43, X, 29, X, X, 35, X, 52, X, 34},
          {X, 40, X, 13, 7, X, 52, X, X, 21, X, 51, 34, X, X, 2, 42, X},
          {8, X, 21, 37, 47, 6, X, 30, X, 5, X, X, X, 15, 6, X, 3, 36},
          {43, 17, X, 10, 32, X, X, 44, 5, X, 12, 50, X, 5, X, 58, X, X},
      }};
    default:
      return LdpcInfoShifts{{
          {38, 18, 31, 40, 46, 13, X, 1, 40, 47, 43, X, 16, 0, 29, X, 33, 15, 49, X},
          {14, 30, 51, 26, 63, 0, 14, 0, X, 51, X, 5, 59, 39, X, 2, 27, X, 23, 55},
          {57, 40, 19, 23, X, 9, 34, X, 41, 52, 25, 62, X, X, 41, 7, 22, 0, 40, 27},
          {48, 42, 8, 33, 34, X, 33, 62, 15, X, 17, 30, 48, 59, 0, 61, X, 44, X, 14},
      }};
  }
}

constexpr LdpcTable ldpc_make_table(uint32_t rate = OFDM_LDPC_RATE_1_2) {
  constexpr int8_t X = -1;
  const LdpcInfoShifts info = ldpc_info_shifts(rate);
  LdpcTable t{};
  t.mb = (int)ldpc_rate_rows(rate);
  t.kb = LDPC_COLS - t.mb;
  t.mid = t.mb / 2;
  for (int i = 0; i < LDPC_ROWS; i++)
    for (int j = 0; j < LDPC_COLS; j++) t.shift[i][j] = (i < t.mb && j < t.kb) ? info.s[i][j] : X;
  // parity part: column kb in rows 0, mid and mb - 1; column kb + 1 + i in rows i and i + 1 (the staircase)
  t.shift[0][t.kb] = 1;
  t.shift[t.mid][t.kb] = 0;
  t.shift[t.mb - 1][t.kb] = 1;
  for (int i = 0; i < t.mb - 1; i++) t.shift[i][t.kb + 1 + i] = t.shift[i + 1][t.kb + 1 + i] = 0;
  t.entries = 0;
  t.max_deg = 0;
  for (int i = 0; i < LDPC_ROWS; i++) {
    t.deg[i] = 0;
    for (int e = 0; e < LDPC_MAX_DEG; e++) t.col[i][e] = t.sh[i][e] = 0;
    for (int j = 0; j < LDPC_COLS; j++)
      if (t.shift[i][j] >= 0) {
        t.col[i][t.deg[i]] = j;
        t.sh[i][t.deg[i]] = t.shift[i][j];
        t.deg[i]++;
        t.entries++;
      }
    if (t.deg[i] > t.max_deg) t.max_deg = t.deg[i];
  }
  return t;
}
template <uint32_t RATE>
constexpr LdpcTable LDPC_TABLE_R = ldpc_make_table(RATE);
constexpr LdpcTable LDPC_TABLE = ldpc_make_table();  // rate 1/2
static_assert(LDPC_TABLE.entries == 83, "58 info entries + 25 parity entries");
static_assert(LDPC_TABLE_R<OFDM_LDPC_RATE_1_2>.entries == 83 && LDPC_TABLE_R<OFDM_LDPC_RATE_2_3>.entries == 71 &&
                  LDPC_TABLE_R<OFDM_LDPC_RATE_3_4>.entries == 73 && LDPC_TABLE_R<OFDM_LDPC_RATE_5_6>.entries == 73,
              "entries of the four tables");
static_assert(LDPC_TABLE.max_deg == 7 && LDPC_TABLE_R<OFDM_LDPC_RATE_2_3>.max_deg == 9 && LDPC_TABLE_R<OFDM_LDPC_RATE_3_4>.max_deg == 13 &&
                  LDPC_TABLE_R<OFDM_LDPC_RATE_5_6>.max_deg == LDPC_MAX_DEG,
              "no row is longer than 19");

// codewords of a block with k info bytes
LDPC_HD static inline uint32_t ldpc_words_rate(uint32_t rate, uint32_t k) { return (k + ldpc_rate_info(rate) - 1u) / ldpc_rate_info(rate); }
LDPC_HD static inline uint32_t ldpc_words(uint32_t k) { return ldpc_words_rate(OFDM_LDPC_RATE_1_2, k); }
// info bytes of codeword w: all KI but in the last, shortened one
LDPC_HD static inline uint32_t ldpc_cw_info_rate(uint32_t rate, uint32_t k, uint32_t w) {
  const uint32_t KI = ldpc_rate_info(rate), left = k - KI * w;
  return left < KI ? left : KI;
}
LDPC_HD static inline uint32_t ldpc_cw_info(uint32_t k, uint32_t w) { return ldpc_cw_info_rate(OFDM_LDPC_RATE_1_2, k, w); }

// coded block of an n-byte payload: k = n + 4 info bytes and PB parity bytes per codeword
static inline int ldpc_coded_len_rate(uint32_t rate, uint32_t payload_len, uint32_t* coded_len) {
  if (!coded_len || rate >= LDPC_RATES || payload_len > ldpc_rate_max_payload(rate)) return OFDM_E_INVAL;
  const uint32_t k = payload_len + 4u;
  *coded_len = k + ldpc_rate_parity(rate) * ldpc_words_rate(rate, k);
  return OFDM_OK;
}
static inline int ldpc_coded_len(uint32_t payload_len, uint32_t* coded_len) { return ldpc_coded_len_rate(OFDM_LDPC_RATE_1_2, payload_len, coded_len); }

// a received length is a block iff its last codeword has at least one info byte in front of its parity (and the first
// one the four CRC bytes): PB + 4 <= m <= 4032 and ((m - 1) mod 192) >= PB
LDPC_HD static inline bool ldpc_is_block_rate(uint32_t rate, uint32_t coded_len) {
  return coded_len >= ldpc_rate_parity(rate) + 4u && coded_len <= OFDM_LDPC_MAX_CODED && ((coded_len - 1u) % LDPC_CW_SENT) >= ldpc_rate_parity(rate);
}
LDPC_HD static inline bool ldpc_is_block(uint32_t coded_len) { return ldpc_is_block_rate(OFDM_LDPC_RATE_1_2, coded_len); }
// codewords and info bytes of a received block (ldpc_is_block holds)
LDPC_HD static inline uint32_t ldpc_block_words(uint32_t coded_len) { return (coded_len + LDPC_CW_SENT - 1u) / LDPC_CW_SENT; }
LDPC_HD static inline uint32_t ldpc_block_info_rate(uint32_t rate, uint32_t coded_len) {
  return coded_len - ldpc_rate_parity(rate) * ldpc_block_words(coded_len);
}
LDPC_HD static inline uint32_t ldpc_block_info(uint32_t coded_len) { return ldpc_block_info_rate(OFDM_LDPC_RATE_1_2, coded_len); }

static inline int ldpc_payload_len_rate(uint32_t rate, uint32_t coded_len, uint32_t* payload_len) {
  if (!payload_len || rate >= LDPC_RATES || !ldpc_is_block_rate(rate, coded_len)) return OFDM_E_INVAL;
  *payload_len = ldpc_block_info_rate(rate, coded_len) - 4u;
  return OFDM_OK;
}
static inline int ldpc_payload_len(uint32_t coded_len, uint32_t* payload_len) { return ldpc_payload_len_rate(OFDM_LDPC_RATE_1_2, coded_len, payload_len); }

// one block of a batch as the kernels see it
struct LdpcBlk {
  uint64_t in_off;   // into the input blob: bytes (payloads, hard blocks) or values (soft blocks)
  uint64_t out_off;  // into the output blob, bytes
  uint32_t len;      // encode: payload bytes; decode: coded bytes of a block (a length that is no block has no codeword)
  uint32_t cw0;      // the block's first codeword in the batch
};

// what the decoder's codewords add up per block; ok = (crc == got) on the host
struct LdpcRes {
  uint32_t crc, got, corrected, iters, failed;
};

// Codeword map of an encode batch: blk[], out_off[0..nblk], cw_blk[c] = block of codeword c (may be NULL to count
// only), the codeword count and the bytes of input reached.  Returns the total coded bytes, ~0 for a payload that is
// too long.
static inline uint64_t ldpc_plan_encode_rate(uint32_t rate, const uint64_t* in_off, const uint32_t* payload_len, uint64_t nblk, LdpcBlk* blk,
                                             uint64_t* out_off, uint32_t* cw_blk, uint64_t* ncw, uint64_t* in_extent) {
  uint64_t o = 0, c = 0, ext = 0;
  for (uint64_t b = 0; b < nblk; b++) {
    uint32_t cl = 0;
    if (ldpc_coded_len_rate(rate, payload_len[b], &cl) != OFDM_OK) return ~0ull;
    const uint32_t W = ldpc_words_rate(rate, payload_len[b] + 4u);
    blk[b] = LdpcBlk{in_off[b], o, payload_len[b], (uint32_t)c};
    out_off[b] = o;
    o += cl;
    if (cw_blk)
      for (uint32_t w = 0; w < W; w++) cw_blk[c + w] = (uint32_t)b;
    c += W;
    const uint64_t e = in_off[b] + payload_len[b];
    if (e > ext) ext = e;
  }
  out_off[nblk] = o;
  *ncw = c;
  *in_extent = ext;
  return o;
}

static inline uint64_t ldpc_plan_encode(const uint64_t* in_off, const uint32_t* payload_len, uint64_t nblk, LdpcBlk* blk, uint64_t* out_off,
                                        uint32_t* cw_blk, uint64_t* ncw, uint64_t* in_extent) {
  return ldpc_plan_encode_rate(OFDM_LDPC_RATE_1_2, in_off, payload_len, nblk, blk, out_off, cw_blk, ncw, in_extent);
}

// The same for a decode batch (`unit` input items per coded byte: 1 hard, 8 soft): a length that is no block takes no
// room, has no codeword and reaches no input.  Returns the total payload bytes.
static inline uint64_t ldpc_plan_decode_rate(uint32_t rate, const uint64_t* in_off, const uint32_t* coded_len, uint64_t nblk, uint64_t unit,
                                             LdpcBlk* blk, uint64_t* out_off, uint32_t* cw_blk, uint64_t* ncw, uint64_t* in_extent) {
  uint64_t o = 0, c = 0, ext = 0;
  for (uint64_t b = 0; b < nblk; b++) {
    blk[b] = LdpcBlk{in_off[b], o, coded_len[b], (uint32_t)c};
    out_off[b] = o;
    if (!ldpc_is_block_rate(rate, coded_len[b])) continue;
    const uint32_t W = ldpc_block_words(coded_len[b]);
    o += ldpc_block_info_rate(rate, coded_len[b]) - 4u;
    if (cw_blk)
      for (uint32_t w = 0; w < W; w++) cw_blk[c + w] = (uint32_t)b;
    c += W;
    const uint64_t e = in_off[b] + unit * coded_len[b];
    if (e > ext) ext = e;
  }
  out_off[nblk] = o;
  *ncw = c;
  *in_extent = ext;
  return o;
}
static inline uint64_t ldpc_plan_decode(const uint64_t* in_off, const uint32_t* coded_len, uint64_t nblk, uint64_t unit, LdpcBlk* blk,
                                        uint64_t* out_off, uint32_t* cw_blk, uint64_t* ncw, uint64_t* in_extent) {
  return ldpc_plan_decode_rate(OFDM_LDPC_RATE_1_2, in_off, coded_len, nblk, unit, blk, out_off, cw_blk, ncw, in_extent);
}
