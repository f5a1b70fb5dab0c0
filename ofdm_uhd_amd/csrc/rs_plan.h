// rs_plan.h -- the host arithmetic of the outer code (rs.h / engine_rs.inc): block lengths f(k) and their inverse, the
// interleaving depth W, the info symbols k_w of a codeword, where a codeword's symbols lie in a block, and the batch
// tables.  Plain C++ without a HIP include, so that a stand-alone program can check it (tools/rs_plan_check.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/ofdm_hip.h"

#ifdef __HIPCC__
#define RS_HD __host__ __device__
#else
#define RS_HD
#endif

constexpr uint32_t RS_N = 255;                     // RS(255, 223) over GF(2^8), shortened per codeword
constexpr uint32_t RS_K = RS_N - OFDM_RS_PARITY;   // 223
constexpr uint32_t RS_MAX_WORDS = 16;              // W of the largest block: ceil((OFDM_RS_MAX_PAYLOAD + 4) / 223)

// W of k info bytes (k >= 1)
RS_HD static inline uint32_t rs_words(uint32_t k) { return (k + RS_K - 1u) / RS_K; }

// f(k) = k + 32 ceil(k / 223)
RS_HD static inline uint32_t rs_block_len(uint32_t k) { return k + OFDM_RS_PARITY * rs_words(k); }

static inline int rs_coded_len(uint32_t payload_len, uint32_t* coded_len) {
  if (!coded_len || payload_len > OFDM_RS_MAX_PAYLOAD) return OFDM_E_INVAL;
  *coded_len = rs_block_len(payload_len + 4u);
  return OFDM_OK;
}

// The inverse of f: a block of `coded_len` bytes has W = ceil(coded_len / 255) codewords (f(k) <= 255 W, and
// f(k) > 255 (W - 1) since k > 223 (W - 1)), so k = coded_len - 32 W; the length is a block when that k has W words.
// Lengths f never reaches, below f(4) = 36 or above OFDM_RS_MAX_CODED are no block.
RS_HD static inline bool rs_info_len(uint32_t coded_len, uint32_t* k) {
  if (coded_len < 36u || coded_len > OFDM_RS_MAX_CODED) return false;
  const uint32_t W = (coded_len + RS_N - 1u) / RS_N;
  const uint32_t kk = coded_len - OFDM_RS_PARITY * W;  // (no wrap: coded_len > 255 (W - 1) >= 32 W from W = 2 on, 36 > 32)
  if (kk < 4u || rs_words(kk) != W) return false;
  *k = kk;
  return true;
}

static inline int rs_payload_len(uint32_t coded_len, uint32_t* payload_len) {
  uint32_t k;
  if (!payload_len || !rs_info_len(coded_len, &k)) return OFDM_E_INVAL;
  *payload_len = k - 4u;
  return OFDM_OK;
}

// info symbols of codeword w < W: info byte i is symbol i / W of codeword i mod W
RS_HD static inline uint32_t rs_cw_info(uint32_t k, uint32_t W, uint32_t w) { return (k - w + W - 1u) / W; }

// byte of the block that holds symbol s (0 = first = highest degree) of codeword w: info symbols s < k_w, then parity
// byte j = s - k_w at k + j W + w
RS_HD static inline uint32_t rs_sym_pos(uint32_t k, uint32_t W, uint32_t w, uint32_t s) {
  const uint32_t kw = rs_cw_info(k, W, w);
  return s < kw ? s * W + w : k + (s - kw) * W + w;
}

// one block of a batch as the kernels see it
struct RsBlk {
  uint64_t in_off;   // into the input blob, bytes
  uint64_t out_off;  // into the output blob, bytes
  uint32_t len;      // encode: payload bytes; decode: coded bytes (any value: a length that is no block decodes to nothing)
  uint32_t pad;
};

// Layout of an encode batch: coded_off[0..nblk], the bytes of input the payloads reach.  Returns the total coded bytes,
// ~0 for a payload above OFDM_RS_MAX_PAYLOAD.
static inline uint64_t rs_plan_encode(const uint64_t* payload_off, const uint32_t* payload_len, uint64_t nblk, RsBlk* blk,
                                      uint64_t* coded_off, uint64_t* in_extent) {
  uint64_t o = 0, ext = 0;
  for (uint64_t b = 0; b < nblk; b++) {
    uint32_t cl;
    if (rs_coded_len(payload_len[b], &cl) != OFDM_OK) return ~0ull;
    blk[b].in_off = payload_off[b];
    blk[b].out_off = o;
    blk[b].len = payload_len[b];
    blk[b].pad = 0;
    coded_off[b] = o;
    o += cl;
    const uint64_t e = payload_off[b] + payload_len[b];
    if (e > ext) ext = e;
  }
  coded_off[nblk] = o;
  *in_extent = ext;
  return o;
}

// Layout of a decode batch: out_off[0..nblk] of the payloads (a length that is no block takes no room), how many
// entries are blocks and the bytes of input those reach.  Returns the total payload bytes.
static inline uint64_t rs_plan_decode(const uint64_t* in_off, const uint32_t* coded_len, uint64_t nblk, RsBlk* blk, uint64_t* out_off,
                                      uint64_t* nvalid, uint64_t* in_extent) {
  uint64_t o = 0, ext = 0, nv = 0;
  for (uint64_t b = 0; b < nblk; b++) {
    blk[b].in_off = in_off[b];
    blk[b].out_off = o;
    blk[b].len = coded_len[b];
    blk[b].pad = 0;
    out_off[b] = o;
    uint32_t k;
    if (rs_info_len(coded_len[b], &k)) {
      o += k - 4u;
      nv++;
      const uint64_t e = in_off[b] + coded_len[b];
      if (e > ext) ext = e;
    }
  }
  out_off[nblk] = o;
  *nvalid = nv;
  *in_extent = ext;
  return o;
}

// ---- reliability-driven errors-and-erasures decoding (ofdm_rs_decode_rel, ofdm_rs_rel_from_soft) ---------------------
constexpr uint32_t RS_REL_DEFAULT_ERASURES = 28;  // M of cfg == NULL: four parity symbols stay a check on what the erasures fill in

// M of a call: the default for cfg == NULL; false for a cfg the call refuses (size, M > 32, a non-zero reserved word)
static inline bool rs_rel_max_erasures(const ofdm_rs_rel_cfg* cfg, uint32_t* M) {
  if (!cfg) {
    *M = RS_REL_DEFAULT_ERASURES;
    return true;
  }
  if (cfg->struct_size != sizeof(ofdm_rs_rel_cfg) || cfg->max_erasures > OFDM_RS_PARITY) return false;
  for (uint32_t r : cfg->reserved)
    if (r) return false;
  *M = cfg->max_erasures;
  return true;
}

// reliability of one byte from its eight values: the smallest |v|, -128 read as 127 (0 .. 127)
RS_HD static inline uint32_t rs_rel_of_values(const int8_t* v) {
  uint32_t m = 127u;
  for (int j = 0; j < 8; j++) {
    const int x = v[j];
    const uint32_t a = (uint32_t)(x < 0 ? -x : x);
    m = a < m ? a : m;
  }
  return m;
}

// Where the reliabilities of a decode batch lie (rel_off == NULL: where the blocks lie) and the bytes of `rel` that the
// blocks among the entries reach.
static inline void rs_plan_rel(const uint64_t* coded_off, const uint64_t* rel_off, const uint32_t* coded_len, uint64_t nblk, uint64_t* out,
                               uint64_t* rel_extent) {
  uint64_t ext = 0;
  for (uint64_t b = 0; b < nblk; b++) {
    out[b] = rel_off ? rel_off[b] : coded_off[b];
    uint32_t k;
    if (rs_info_len(coded_len[b], &k)) {
      const uint64_t e = out[b] + coded_len[b];
      if (e > ext) ext = e;
    }
  }
  *rel_extent = ext;
}

// Layout of an ofdm_rs_rel_from_soft batch: entry b reads 8 coded_len[b] values from soft_off[b] (a multiple of 8) and
// writes coded_len[b] bytes at rel_off[b], the running sum.  Returns the total bytes, ~0 for an offset that is no
// multiple of 8; *in_extent is the number of values the batch reaches.
static inline uint64_t rs_plan_rel_soft(const uint64_t* soft_off, const uint32_t* coded_len, uint64_t nblk, RsBlk* blk, uint64_t* rel_off,
                                        uint64_t* in_extent) {
  uint64_t o = 0, ext = 0;
  for (uint64_t b = 0; b < nblk; b++)
    if (soft_off[b] & 7u) return ~0ull;
  for (uint64_t b = 0; b < nblk; b++) {
    blk[b].in_off = soft_off[b];
    blk[b].out_off = o;
    blk[b].len = coded_len[b];
    blk[b].pad = 0;
    rel_off[b] = o;
    o += coded_len[b];
    const uint64_t e = soft_off[b] + 8ull * coded_len[b];
    if (coded_len[b] && e > ext) ext = e;
  }
  rel_off[nblk] = o;
  *in_extent = ext;
  return o;
}
