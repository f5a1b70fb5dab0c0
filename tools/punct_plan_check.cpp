// punct_plan_check.cpp -- the host arithmetic of the punctured rates (ofdm_uhd_amd/csrc/punct_plan.h) as a program of its
// own: the three patterns, kept-bit counts and block lengths for every payload length and rate, monotonicity, the inverse,
// rank / unrank as bijections, the C' rule and the two batch layouts.  Needs no GPU and no HIP.  For a sanitizer run
// build it with
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include -o punct_plan_check tools/punct_plan_check.cpp
// tests/test_punct_host.py builds and runs it without the sanitizers.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../ofdm_uhd_amd/csrc/punct_plan.h"

#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #c); \
      exit(1);                                                    \
    }                                                             \
  } while (0)

int main() {
  // the patterns: mask, nibble table, period and kept count agree with each other and with 802.11's keep sets
  const uint32_t keep23[] = {0, 1, 2}, keep34[] = {0, 1, 2, 5}, keep56[] = {0, 1, 2, 5, 6, 9};
  const uint32_t* keeps[4] = {nullptr, keep23, keep34, keep56};
  for (uint32_t r = 1; r <= 3; r++) {
    uint32_t mask = 0;
    for (uint32_t k = 0; k < PUNCT_KEPT[r]; k++) {
      mask |= 1u << keeps[r][k];
      CHECK(((PUNCT_NIB[r] >> (4 * k)) & 15u) == keeps[r][k]);
    }
    CHECK(mask == PUNCT_MASK[r] && (mask >> PUNCT_PERIOD[r]) == 0);
    CHECK(PUNCT_PERIOD[r] % 2 == 0);  // a period is whole trellis steps
    // rate = (period / 2) info bits per kept bits
    CHECK((r == 1 && PUNCT_KEPT[r] * 2 == 3 * PUNCT_PERIOD[r] / 2) || (r == 2 && PUNCT_KEPT[r] * 3 == 4 * PUNCT_PERIOD[r] / 2) ||
          (r == 3 && PUNCT_KEPT[r] * 5 == 6 * PUNCT_PERIOD[r] / 2));
  }
  CHECK(punct_rate_ok(0) && punct_rate_ok(3) && !punct_rate_ok(4) && !punct_rate_ok(0xFFFFFFFFu));

  // every n and rate: K by counting, P, strict monotonicity in steps of 1 or 2, the inverse, rank / unrank
  const uint32_t known_n[] = {0, 1, 2, 1026, 2040};
  const uint32_t known_P[4][5] = {{10, 12, 14, 2062, 4090}, {8, 9, 11, 1547, 3068}, {7, 8, 9, 1375, 2727}, {6, 7, 9, 1237, 2454}};
  for (uint32_t r = 0; r <= 3; r++) {
    for (int k = 0; k < 5; k++) {
      uint32_t P = 0;
      CHECK(punct_coded_len(r, known_n[k], &P) == OFDM_OK && P == known_P[r][k]);
    }
    uint32_t v = 0;
    CHECK(punct_coded_len(r, OFDM_FEC_MAX_PAYLOAD + 1, &v) == OFDM_E_INVAL && punct_coded_len(r, 0xFFFFFFFFu, &v) == OFDM_E_INVAL);
    CHECK(punct_coded_len(r, 0, nullptr) == OFDM_E_INVAL && punct_payload_len(r, known_P[r][0], nullptr) == OFDM_E_INVAL);
  }
  {
    uint32_t v = 0;
    CHECK(punct_coded_len(4, 0, &v) == OFDM_E_INVAL && punct_payload_len(4, 10, &v) == OFDM_E_INVAL);
  }
  for (uint32_t r = 1; r <= 3; r++) {
    std::vector<int> owner(OFDM_FEC_MAX_CODED + 2, -1);
    uint32_t prev = 0, kept_so_far = 0, at = 0;
    for (uint32_t n = 0; n <= OFDM_FEC_MAX_PAYLOAD; n++) {
      const uint32_t bits = punct_mother_bits(n);
      for (; at < bits; at++) {  // count the pattern, and walk rank / unrank along it
        if (punct_kept_rt(r, at)) {
          CHECK(punct_rank_rt(r, at) == kept_so_far && punct_unrank_rt(r, kept_so_far) == at);
          kept_so_far++;
        } else {
          CHECK(punct_rank_rt(r, at) == kept_so_far);  // kept bits in front of a dropped one
        }
      }
      const uint32_t K = punct_kept_bits_rt(r, n);
      CHECK(K == kept_so_far && punct_unrank_rt(r, K) >= bits);  // kept bit K would lie behind the block
      uint32_t P = 0, back = 77;
      CHECK(punct_coded_len(r, n, &P) == OFDM_OK && P == (K + 7) / 8 && P == punct_block_len_rt(r, n));
      CHECK(8 * P >= K && 8 * P < K + 8 && P < 2 * n + 10);
      if (n) CHECK(P == prev + 1 || P == prev + 2);
      prev = P;
      CHECK(punct_payload_len(r, P, &back) == OFDM_OK && back == n);
      CHECK(owner[P] < 0);
      owner[P] = (int)n;
      // C': the largest power of two <= the columns that divides 8P
      for (uint32_t lgC = 0; lgC <= 4; lgC++) {
        const uint32_t l = punct_log2_cols(lgC, P);
        CHECK(l <= lgC && (8 * P) % (1u << l) == 0);
        CHECK(l == lgC || (8 * P) % (1u << (l + 1)) != 0);
        CHECK((l != lgC) == (lgC == 4 && (P & 1)));
      }
    }
    // lengths P never reaches, and lengths out of range, are refused
    for (uint32_t m = 0; m <= OFDM_FEC_MAX_CODED + 1; m++) {
      uint32_t back = 77;
      CHECK((punct_payload_len(r, m, &back) == OFDM_OK) == (owner[m] >= 0));
      if (owner[m] >= 0) CHECK(back == (uint32_t)owner[m]);
    }
    const uint32_t far[] = {0x7FFFFFFFu, 0xFFFFFFFEu, 0xFFFFFFFFu};
    for (uint32_t m : far) {
      uint32_t back = 0;
      CHECK(punct_payload_len(r, m, &back) == OFDM_E_INVAL);
    }
  }

  // rate 0 is the mother code's pair of functions
  for (uint32_t n = 0; n <= OFDM_FEC_MAX_PAYLOAD + 2; n++) {
    uint32_t a = 1, b = 2;
    CHECK(punct_coded_len(0, n, &a) == fec_coded_len(n, &b) && (n > OFDM_FEC_MAX_PAYLOAD || a == b));
  }
  for (uint32_t m = 0; m <= OFDM_FEC_MAX_CODED + 2; m++) {
    uint32_t a = 1, b = 1;
    CHECK(punct_payload_len(0, m, &a) == fec_payload_len(m, &b) && a == b);
  }

  // encode layout
  {
    const uint32_t len[] = {0, 1, 2, 1026, 2040, 5};
    const uint64_t in_off[] = {0, 0, 1, 3, 1029, 3069};
    std::vector<FecBlk> blk(6);
    uint64_t out_off[7], ext = 0;
    CHECK(punct_plan_encode(2, in_off, len, 6, blk.data(), out_off, &ext) == 7 + 8 + 9 + 1375 + 2727 + punct_block_len_rt(2, 5));
    CHECK(ext == 3074 && out_off[0] == 0 && out_off[4] == 7 + 8 + 9 + 1375 && blk[4].out_off == out_off[4] && blk[4].len == 2040);
    const uint32_t too_long[] = {3, 2041};
    CHECK(punct_plan_encode(2, in_off, too_long, 2, blk.data(), out_off, &ext) == ~0ull);
    CHECK(punct_plan_encode(1, in_off, len, 0, blk.data(), out_off, &ext) == 0 && out_off[0] == 0 && ext == 0);
  }

  // decode layout: lengths that are no block at the rate take no room, reach no input, size nothing and are no block
  // to the decoder; the places in the mother-value buffer repeat from slice to slice and never overlap inside one
  for (uint32_t r = 1; r <= 3; r++) {
    uint32_t gap = 0;  // the first length above P(0) that P skips
    for (uint32_t m = punct_block_len_rt(r, 0); !gap; m++) {
      uint32_t back;
      if (punct_payload_len(r, m, &back) != OFDM_OK) gap = m;
    }
    const uint32_t len[] = {punct_block_len_rt(r, 0), 0, punct_block_len_rt(r, 2040), gap, punct_block_len_rt(r, 1), 4090, 0xFFFFFFFFu,
                            punct_block_len_rt(r, 1026), punct_block_len_rt(r, 3)};
    const uint32_t n_of[] = {0, 0, 2040, 0, 1, 0, 0, 1026, 3};
    const bool is[] = {true, false, true, false, true, false, false, true, true};
    const size_t nb = sizeof(len) / sizeof(len[0]);
    std::vector<uint64_t> in_off(nb), out_off(nb + 1, 77);
    for (uint64_t unit : {1ull, 8ull}) {
      uint64_t o = 0;
      for (size_t k = 0; k < nb; k++) {
        in_off[k] = o;
        o += is[k] ? unit * len[k] : 3;
      }
      std::vector<FecBlk> pblk(nb), mblk(nb);
      uint64_t stride = 0, ms = 0, ext = 0;
      const uint64_t total = punct_plan_decode_sizes(r, in_off.data(), len, nb, unit, pblk.data(), out_off.data(), &stride, &ms, &ext);
      CHECK(total == 2040 + 1 + 1026 + 3 && out_off[nb] == total);
      CHECK(stride == 64 * 256 && ms == 8 * 4090 && ms % 16 == 0 && 4 * ms <= stride * 8);
      CHECK(ext == in_off[nb - 1] + unit * len[nb - 1]);
      for (uint64_t per : {1ull, 2ull, 4ull, 9ull, 100ull}) {
        punct_plan_decode_slots(nb, per, ms, out_off.data(), pblk.data(), mblk.data());
        uint64_t at = 0;
        for (size_t k = 0; k < nb; k++) {
          CHECK(pblk[k].in_off == in_off[k] && pblk[k].len == len[k] && out_off[k] == at && mblk[k].out_off == at);
          CHECK(pblk[k].out_off == (k % per) * ms && mblk[k].in_off == pblk[k].out_off && pblk[k].out_off + ms <= per * ms);
          CHECK(pblk[k].pad == (is[k] ? 2 * n_of[k] + 10 : 0) && mblk[k].len == pblk[k].pad);
          CHECK(fec_is_block(mblk[k].len) == is[k]);
          if (is[k]) at += n_of[k];
        }
      }
    }
    const uint32_t none[] = {0, gap, 4091};
    std::vector<FecBlk> pblk(3);
    uint64_t stride = 1, ms = 1, ext = 1;
    CHECK(punct_plan_decode_sizes(r, in_off.data(), none, 3, 1, pblk.data(), out_off.data(), &stride, &ms, &ext) == 0);
    CHECK(stride == 0 && ms == 0 && ext == 0 && out_off[3] == 0);
  }
  printf("punct_plan_check ok\n");
  return 0;
}
