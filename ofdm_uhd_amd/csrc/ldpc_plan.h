// ldpc_plan.h -- the host arithmetic of the LDPC coded-link layer (ldpc.h / engine_ldpc.inc): the base matrix, block
// lengths, and the codeword map of a batch (block -> first codeword, codeword -> block, info bytes per codeword).
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
constexpr int LDPC_ROWS = 12, LDPC_COLS = 24;     // base matrix
constexpr uint32_t LDPC_CW_INFO = 96;             // info bytes of a full codeword (768 bits)
constexpr uint32_t LDPC_CW_PARITY = 96;           // parity bytes of every codeword
constexpr uint32_t LDPC_CW_SENT = LDPC_CW_INFO + LDPC_CW_PARITY;
constexpr uint32_t LDPC_MAX_WORDS = 21;           // codewords of the longest block
constexpr int LDPC_MAX_DEG = 7;
constexpr uint32_t LDPC_DEFAULT_ITERS = 20, LDPC_MAX_ITERS = 64;

// The base matrix: shift[i][j] of row i and column j, -1 for no entry; per row its entries in column order.
struct LdpcTable {
  int8_t shift[LDPC_ROWS][LDPC_COLS];
  int deg[LDPC_ROWS];
  int col[LDPC_ROWS][LDPC_MAX_DEG];
  int sh[LDPC_ROWS][LDPC_MAX_DEG];
  int entries;
};

constexpr LdpcTable ldpc_make_table() {
  constexpr int8_t X = -1;
  constexpr int8_t info[LDPC_ROWS][12] = {
      {X, 1, X, X, 25, X, X, 42, X, 59, X, 24},   {X, X, X, 17, 48, X, X, X, 37, X, 21, 42}, {2, X, X, X, X, X, 0, X, 56, X, 20, 50},
      {X, 52, X, X, X, 5, X, X, 45, 19, 45, X},   {X, X, 34, X, X, X, 30, X, 29, 31, X, 55}, {17, X, X, X, X, X, 5, X, 53, X, 21, 36},
      {X, X, X, X, X, X, 25, 16, X, 22, X, X},    {X, X, 38, X, X, 54, X, 48, X, 56, 3, X},  {X, 58, X, X, X, X, X, 7, 60, 36, X, 20},
      {X, X, X, 59, 35, X, X, X, X, 46, 38, 25},  {40, X, X, 42, X, X, X, X, 24, 33, 16, X}, {X, X, 46, X, X, 1, X, X, 51, X, 25, 5},
  };
  LdpcTable t{};
  for (int i = 0; i < LDPC_ROWS; i++)
    for (int j = 0; j < LDPC_COLS; j++) t.shift[i][j] = j < 12 ? info[i][j] : X;
  // parity part: column 12 in rows 0, 6 and 11; column 13 + i in rows i and i + 1 (the staircase)
  t.shift[0][12] = 1;
  t.shift[6][12] = 0;
  t.shift[11][12] = 1;
  for (int i = 0; i < 11; i++) t.shift[i][13 + i] = t.shift[i + 1][13 + i] = 0;
  t.entries = 0;
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
  }
  return t;
}
constexpr LdpcTable LDPC_TABLE = ldpc_make_table();
static_assert(LDPC_TABLE.entries == 83, "58 info entries + 25 parity entries");

// codewords of a block with k info bytes
LDPC_HD static inline uint32_t ldpc_words(uint32_t k) { return (k + LDPC_CW_INFO - 1u) / LDPC_CW_INFO; }
// info bytes of codeword w: all 96 but in the last, shortened one
LDPC_HD static inline uint32_t ldpc_cw_info(uint32_t k, uint32_t w) {
  const uint32_t left = k - LDPC_CW_INFO * w;
  return left < LDPC_CW_INFO ? left : LDPC_CW_INFO;
}

// coded block of an n-byte payload: k = n + 4 info bytes and 96 parity bytes per codeword
static inline int ldpc_coded_len(uint32_t payload_len, uint32_t* coded_len) {
  if (!coded_len || payload_len > OFDM_LDPC_MAX_PAYLOAD) return OFDM_E_INVAL;
  const uint32_t k = payload_len + 4u;
  *coded_len = k + LDPC_CW_PARITY * ldpc_words(k);
  return OFDM_OK;
}

// a received length is a block iff its last codeword has at least one info byte in front of its parity (and the first
// one the four CRC bytes): 100 <= m <= 4032 and ((m - 1) mod 192) >= 96
LDPC_HD static inline bool ldpc_is_block(uint32_t coded_len) {
  return coded_len >= 100u && coded_len <= OFDM_LDPC_MAX_CODED && ((coded_len - 1u) % LDPC_CW_SENT) >= LDPC_CW_PARITY;
}
// codewords and info bytes of a received block (ldpc_is_block holds)
LDPC_HD static inline uint32_t ldpc_block_words(uint32_t coded_len) { return (coded_len + LDPC_CW_SENT - 1u) / LDPC_CW_SENT; }
LDPC_HD static inline uint32_t ldpc_block_info(uint32_t coded_len) { return coded_len - LDPC_CW_PARITY * ldpc_block_words(coded_len); }

static inline int ldpc_payload_len(uint32_t coded_len, uint32_t* payload_len) {
  if (!payload_len || !ldpc_is_block(coded_len)) return OFDM_E_INVAL;
  *payload_len = ldpc_block_info(coded_len) - 4u;
  return OFDM_OK;
}

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
static inline uint64_t ldpc_plan_encode(const uint64_t* in_off, const uint32_t* payload_len, uint64_t nblk, LdpcBlk* blk, uint64_t* out_off,
                                        uint32_t* cw_blk, uint64_t* ncw, uint64_t* in_extent) {
  uint64_t o = 0, c = 0, ext = 0;
  for (uint64_t b = 0; b < nblk; b++) {
    uint32_t cl = 0;
    if (ldpc_coded_len(payload_len[b], &cl) != OFDM_OK) return ~0ull;
    const uint32_t W = ldpc_words(payload_len[b] + 4u);
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

// The same for a decode batch (`unit` input items per coded byte: 1 hard, 8 soft): a length that is no block takes no
// room, has no codeword and reaches no input.  Returns the total payload bytes.
static inline uint64_t ldpc_plan_decode(const uint64_t* in_off, const uint32_t* coded_len, uint64_t nblk, uint64_t unit, LdpcBlk* blk,
                                        uint64_t* out_off, uint32_t* cw_blk, uint64_t* ncw, uint64_t* in_extent) {
  uint64_t o = 0, c = 0, ext = 0;
  for (uint64_t b = 0; b < nblk; b++) {
    blk[b] = LdpcBlk{in_off[b], o, coded_len[b], (uint32_t)c};
    out_off[b] = o;
    if (!ldpc_is_block(coded_len[b])) continue;
    const uint32_t W = ldpc_block_words(coded_len[b]);
    o += ldpc_block_info(coded_len[b]) - 4u;
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
