// sig_plan.h -- the host arithmetic of the signal field (sig.h / engine_sig.inc): the extended Golay (24,12,8) codeword
// of a 12-bit coding word, the word's fields and which words are valid, the field's 12-byte image, block lengths and
// the offsets of a batch.  Plain C++ without a HIP include, so that a stand-alone program can check it
// (tools/sig_plan_check.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/ofdm_hip.h"

#ifdef __HIPCC__
#define SIG_HD __host__ __device__
#else
#define SIG_HD
#endif

constexpr uint32_t SIG_WORD_BITS = 12, SIG_WORDS = 1u << SIG_WORD_BITS;
constexpr uint32_t SIG_CW_BITS = 24, SIG_COPIES = 4;
constexpr uint32_t SIG_FIELD_BITS = SIG_CW_BITS * SIG_COPIES, SIG_FIELD_BYTES = SIG_FIELD_BITS / 8;
constexpr uint32_t SIG_GEN = 0xC75;             // g(x) = x^11 + x^10 + x^6 + x^5 + x^4 + x^2 + 1
constexpr int SIG_MAX_METRIC = 24 * 4 * 127;    // |m(w)| <= 12192, so a margin is at most 24384
static_assert(SIG_FIELD_BYTES == OFDM_SIG_FIELD_BYTES, "four copies of 24 bits");

// The codeword of w as a 24-bit number, codeword bit j (0 is sent first) at bit 23 - j: the 12 word bits, the 11-bit
// remainder of w x^11 modulo g, one bit that makes the weight even.
SIG_HD constexpr uint32_t sig_codeword(uint32_t w) {
  w &= SIG_WORDS - 1;
  uint32_t r = w << 11;
  for (int i = 22; i >= 11; i--)
    if ((r >> i) & 1u) r ^= SIG_GEN << (i - 11);
  const uint32_t c = (w << 11) | r;
  uint32_t p = c;
  p ^= p >> 16;
  p ^= p >> 8;
  p ^= p >> 4;
  p ^= p >> 2;
  p ^= p >> 1;
  return (c << 1) | (p & 1u);
}
static_assert(sig_codeword(0) == 0 && sig_codeword(0xFFF) == 0xFFFFFF, "the all-ones word is a codeword: cw(~w) = ~cw(w)");
static_assert(sig_codeword(1) == ((1u << 12) | (SIG_GEN << 1) | 1u), "word 1 sends g itself, weight 7, and the parity bit");

// word <-> fields.  `cols` is the convolutional interleaver's column count (1, 2, 4, 8, 16); the other codecs have
// none and take 0 (1 is accepted, too) -- the field then holds log2 = 0.
SIG_HD constexpr bool sig_word_valid(uint32_t word) {
  if (word >= SIG_WORDS || (word & 0xFu)) return false;
  const uint32_t codec = word >> 10, rate = (word >> 8) & 3u, lg = (word >> 4) & 7u;
  if (codec == OFDM_SIG_CODEC_NONE) return rate == 0 && lg == 0;
  if (codec == OFDM_SIG_CODEC_FEC) return lg <= 4;
  if (codec == OFDM_SIG_CODEC_LDPC) return lg == 0;
  return false;
}
SIG_HD constexpr int sig_word_pack(uint32_t codec, uint32_t rate, uint32_t rs, uint32_t cols, uint16_t* word) {
  uint32_t lg = 0;
  if (codec == OFDM_SIG_CODEC_FEC) {
    while (lg < 5 && (1u << lg) != cols) lg++;
    if (lg == 5) return OFDM_E_INVAL;
  } else if (cols > 1) {
    return OFDM_E_INVAL;
  }
  if (codec > 3 || rate > 3 || rs > 1) return OFDM_E_INVAL;
  const uint32_t w = (codec << 10) | (rate << 8) | (rs << 7) | (lg << 4);
  if (!sig_word_valid(w)) return OFDM_E_INVAL;
  *word = (uint16_t)w;
  return OFDM_OK;
}
SIG_HD constexpr int sig_word_unpack(uint32_t word, uint32_t* codec, uint32_t* rate, uint32_t* rs, uint32_t* cols) {
  if (!sig_word_valid(word)) return OFDM_E_INVAL;
  *codec = word >> 10;
  *rate = (word >> 8) & 3u;
  *rs = (word >> 7) & 1u;
  *cols = *codec == OFDM_SIG_CODEC_FEC ? 1u << ((word >> 4) & 7u) : 0u;
  return OFDM_OK;
}

// the field's bytes: four copies of the codeword, field bit t MSB first within a byte.  Byte i of a copy (i = 0 .. 2)
// is bits 23 - 8 i .. 16 - 8 i of the codeword, and the copies are 3 bytes each
SIG_HD constexpr uint8_t sig_field_byte(uint32_t cw, uint32_t i) { return (uint8_t)(cw >> (16 - 8 * (i % 3))); }
inline void sig_field_image(uint32_t word, uint8_t out[SIG_FIELD_BYTES]) {
  const uint32_t cw = sig_codeword(word);
  for (uint32_t i = 0; i < SIG_FIELD_BYTES; i++) out[i] = sig_field_byte(cw, i);
}

// One block of a batch.  Encode: body `len` bytes at in_off, the block (field | body) at out_off.  Decode: the packet
// of `len` bytes at in_off (bytes, or values with 8 per byte); out_off is unused.
struct SigBlk {
  uint64_t in_off, out_off;
  uint32_t len, word;
};

inline uint64_t sig_block_len(uint32_t body_len) { return (uint64_t)SIG_FIELD_BYTES + body_len; }

// Fills blk[] and out_off[0 .. nblk]; returns the bytes of all blocks, *extent the bytes of the body blob that are read.
// *bad is the first block with an invalid word, nblk when there is none.
inline uint64_t sig_plan_encode(const uint16_t* words, const uint64_t* body_off, const uint32_t* body_len, uint64_t nblk, SigBlk* blk,
                                uint64_t* out_off, uint64_t* extent, uint64_t* bad) {
  uint64_t total = 0, ext = 0;
  *bad = nblk;
  for (uint64_t k = 0; k < nblk; k++) {
    if (*bad == nblk && !sig_word_valid(words[k])) *bad = k;
    blk[k] = SigBlk{body_off[k], total, body_len[k], words[k]};
    out_off[k] = total;
    total += sig_block_len(body_len[k]);
    if (body_len[k] && body_off[k] + body_len[k] > ext) ext = body_off[k] + body_len[k];
  }
  out_off[nblk] = total;
  *extent = ext;
  return total;
}

// `unit`: 1 for bytes, 8 for values.  Returns the packets that hold a field (len >= 12), *extent the bytes read.
inline uint64_t sig_plan_decode(const uint64_t* in_off, const uint32_t* len, uint64_t nblk, uint32_t unit, SigBlk* blk, uint64_t* extent) {
  uint64_t fields = 0, ext = 0;
  for (uint64_t k = 0; k < nblk; k++) {
    blk[k] = SigBlk{in_off[k], 0, len[k], 0};
    if (len[k] < SIG_FIELD_BYTES) continue;
    fields++;
    const uint64_t end = in_off[k] + (uint64_t)SIG_FIELD_BYTES * unit;  // the body behind the field is not read
    if (end > ext) ext = end;
  }
  *extent = ext;
  return fields;
}
