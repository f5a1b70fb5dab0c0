// sig_plan_check.cpp -- the signal field's host arithmetic (ofdm_uhd_amd/csrc/sig_plan.h) as a program of its own: the
// code's weight distribution (1, 759, 2576, 759, 1 at weights 0, 8, 12, 16, 24), its linearity and minimum distance,
// the codeword against a second statement (the generator matrix's rows, built by long division bit by bit), exactly 50
// valid words and their pack / unpack round trip, the field's byte image bit by bit, and the offsets of encode and
// decode batches.
// Needs no GPU and no HIP.  For a sanitizer run build it with
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include -o sig_plan_check tools/sig_plan_check.cpp
// tests/test_sig_host.py builds and runs it without the sanitizers.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../ofdm_uhd_amd/csrc/sig_plan.h"

#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #c); \
      exit(1);                                                    \
    }                                                             \
  } while (0)

static int weight(uint32_t x) {
  int n = 0;
  for (; x; x &= x - 1) n++;
  return n;
}

// the second statement: x^(11 + e) mod g by shifting one power at a time, for the row of word bit e
static uint32_t row_of_bit(int e) {
  uint32_t r = 1;  // x^0
  for (int s = 0; s < 11 + e; s++) {
    r <<= 1;
    if (r & (1u << 11)) r ^= SIG_GEN;
  }
  const uint32_t c23 = (1u << (11 + e)) | r;  // x^(11 + e) + its remainder: 23 bits, the word's bit e set
  return (c23 << 1) | (uint32_t)(weight(c23) & 1);
}

int main() {
  // ---- the code ---------------------------------------------------------------------------------------------------
  uint32_t rows[12];
  for (int e = 0; e < 12; e++) {
    rows[e] = row_of_bit(e);
    CHECK(rows[e] == sig_codeword(1u << e));
  }
  int dist[25] = {0};
  for (uint32_t w = 0; w < SIG_WORDS; w++) {
    const uint32_t cw = sig_codeword(w);
    CHECK(cw < (1u << 24) && (cw >> 12) == w);  // systematic: the word's bits first
    uint32_t x = 0;
    for (int e = 0; e < 12; e++)
      if ((w >> e) & 1u) x ^= rows[e];
    CHECK(x == cw);  // linear, and equal to the second statement
    CHECK(sig_codeword(w ^ 0xFFFu) == (cw ^ 0xFFFFFFu));
    dist[weight(cw)]++;
  }
  for (int i = 0; i <= 24; i++) CHECK(dist[i] == (i == 0 || i == 24 ? 1 : i == 8 || i == 16 ? 759 : i == 12 ? 2576 : 0));
  for (uint32_t a = 0; a < SIG_WORDS; a += 37)
    for (uint32_t b = 0; b < SIG_WORDS; b++) CHECK(sig_codeword(a ^ b) == (sig_codeword(a) ^ sig_codeword(b)));

  // ---- the words ----------------------------------------------------------------------------------------------------
  int valid = 0;
  for (uint32_t w = 0; w < 0x2000; w++) {
    uint32_t codec = 9, rate = 9, rs = 9, cols = 9;
    const int rc = sig_word_unpack(w, &codec, &rate, &rs, &cols);
    CHECK((rc == OFDM_OK) == sig_word_valid(w));
    if (rc != OFDM_OK) continue;
    valid++;
    // the table of include/ofdm_hip.h, stated once more
    CHECK(w < SIG_WORDS && (w & 0xFu) == 0 && codec == (w >> 10) && rate == ((w >> 8) & 3u) && rs == ((w >> 7) & 1u));
    const uint32_t lg = (w >> 4) & 7u;
    if (codec == OFDM_SIG_CODEC_NONE) CHECK(rate == 0 && lg == 0 && cols == 0);
    if (codec == OFDM_SIG_CODEC_FEC) CHECK(lg <= 4 && cols == (1u << lg));
    if (codec == OFDM_SIG_CODEC_LDPC) CHECK(lg == 0 && cols == 0);
    CHECK(codec != 3);
    uint16_t back = 0xFFFF;
    CHECK(sig_word_pack(codec, rate, rs, cols, &back) == OFDM_OK && back == w);
  }
  CHECK(valid == 50);
  uint16_t word = 0;
  CHECK(sig_word_pack(OFDM_SIG_CODEC_FEC, 0, 0, 3, &word) == OFDM_E_INVAL);    // no power of two
  CHECK(sig_word_pack(OFDM_SIG_CODEC_FEC, 0, 0, 32, &word) == OFDM_E_INVAL);   // too many columns
  CHECK(sig_word_pack(OFDM_SIG_CODEC_FEC, 0, 0, 0, &word) == OFDM_E_INVAL);
  CHECK(sig_word_pack(OFDM_SIG_CODEC_LDPC, 0, 0, 16, &word) == OFDM_E_INVAL);  // columns without the convolutional code
  CHECK(sig_word_pack(OFDM_SIG_CODEC_NONE, 1, 0, 0, &word) == OFDM_E_INVAL);   // a rate without a code
  CHECK(sig_word_pack(3, 0, 0, 0, &word) == OFDM_E_INVAL && sig_word_pack(2, 4, 0, 0, &word) == OFDM_E_INVAL);
  CHECK(sig_word_pack(2, 0, 2, 0, &word) == OFDM_E_INVAL);
  CHECK(sig_word_pack(OFDM_SIG_CODEC_LDPC, 3, 1, 1, &word) == OFDM_OK && word == ((2u << 10) | (3u << 8) | (1u << 7)));
  CHECK(sig_word_pack(OFDM_SIG_CODEC_FEC, 2, 1, 16, &word) == OFDM_OK && word == ((1u << 10) | (2u << 8) | (1u << 7) | (4u << 4)));

  // ---- the field's image: field bit t, MSB first within a byte, is codeword bit t mod 24 ----------------------------
  for (uint32_t w = 0; w < SIG_WORDS; w += 5) {
    uint8_t img[SIG_FIELD_BYTES];
    sig_field_image(w, img);
    const uint32_t cw = sig_codeword(w);
    for (uint32_t t = 0; t < SIG_FIELD_BITS; t++) {
      const uint32_t bit = (img[t / 8] >> (7 - t % 8)) & 1u;
      CHECK(bit == ((cw >> (23 - t % 24)) & 1u));
    }
  }

  // ---- batches ------------------------------------------------------------------------------------------------------
  {
    const uint16_t words[4] = {0, 0x480, 0x440, 0xB80};
    const uint64_t off[4] = {100, 0, 7, 40};
    const uint32_t len[4] = {0, 7, 33, 4080};
    SigBlk blk[4];
    uint64_t out_off[5], extent = 0, bad = 99;
    const uint64_t total = sig_plan_encode(words, off, len, 4, blk, out_off, &extent, &bad);
    CHECK(bad == 4 && total == 4 * 12 + 7 + 33 + 4080 && out_off[4] == total && extent == 40 + 4080);
    uint64_t at = 0;
    for (int k = 0; k < 4; k++) {
      CHECK(out_off[k] == at && blk[k].out_off == at && blk[k].in_off == off[k] && blk[k].len == len[k] && blk[k].word == words[k]);
      at += sig_block_len(len[k]);
    }
    const uint16_t wrong[3] = {0, 0x001, 0xC00};
    CHECK(sig_plan_encode(wrong, off, len, 3, blk, out_off, &extent, &bad) == 3 * 12 + 7 + 33 && bad == 1);
    CHECK(sig_plan_encode(words, off, len, 0, blk, out_off, &extent, &bad) == 0 && out_off[0] == 0 && extent == 0 && bad == 0);
    // decode: only the fields are read; a packet under 12 bytes holds none
    const uint32_t plen[4] = {11, 12, 0, 500};
    const uint64_t poff[4] = {0, 1000, 3, 17};
    CHECK(sig_plan_decode(poff, plen, 4, 1, blk, &extent) == 2 && extent == 1012);
    CHECK(sig_plan_decode(poff, plen, 4, 8, blk, &extent) == 2 && extent == 1096);
    CHECK(blk[3].in_off == 17 && blk[3].len == 500);
    CHECK(sig_plan_decode(poff, plen, 1, 8, blk, &extent) == 0 && extent == 0);
  }
  printf("sig_plan_check ok\n");
  return 0;
}
