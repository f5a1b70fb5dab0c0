// rs_plan_check.cpp -- the outer code's host arithmetic (ofdm_uhd_amd/csrc/rs_plan.h) as a program of its own: the block
// length f and its inverse as a bijection, every length accepted or refused as the count says, the interleaving depth,
// every byte of a block owned by exactly one codeword symbol, and the batch tables.
// Needs no GPU and no HIP.  For a sanitizer run build it with
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include -o rs_plan_check tools/rs_plan_check.cpp
// tests/test_rs_host.py builds and runs it without the sanitizers.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../ofdm_uhd_amd/csrc/rs_plan.h"

#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #c); \
      exit(1);                                                    \
    }                                                             \
  } while (0)

int main() {
  // f over every k up to 3568: strictly increasing in steps of 1 or 33, inverted by rs_info_len
  std::vector<int> reached(4092 + 1, 0);
  uint32_t prev = 0;
  for (uint32_t k = 4; k <= OFDM_RS_MAX_PAYLOAD + 4u; k++) {
    const uint32_t W = rs_words(k), f = rs_block_len(k);
    CHECK(W >= 1 && W <= RS_MAX_WORDS && 223u * W >= k && 223u * (W - 1u) < k);
    CHECK(f == k + 32u * W && f <= OFDM_RS_MAX_CODED);
    CHECK(k == 4 || f - prev == 1 || f - prev == 33);
    CHECK((f - prev == 33) == (k > 4 && (k - 1) % 223 == 0) || k == 4);
    prev = f;
    reached[f]++;
    uint32_t v = 0, back = 0;
    CHECK(rs_coded_len(k - 4u, &v) == OFDM_OK && v == f);
    CHECK(rs_info_len(f, &back) && back == k);
    CHECK(rs_payload_len(f, &back) == OFDM_OK && back == k - 4u);
    // codewords: k_w sums to k, each at most 223, sizes differ by at most one and never grow with w
    uint32_t sum = 0;
    for (uint32_t w = 0; w < W; w++) {
      const uint32_t kw = rs_cw_info(k, W, w);
      CHECK(kw >= 1 && kw <= RS_K && kw + OFDM_RS_PARITY <= RS_N);
      CHECK(w == 0 || (kw <= rs_cw_info(k, W, w - 1) && kw + 1 >= rs_cw_info(k, W, 0)));
      sum += kw;
    }
    CHECK(sum == k);
    // every info and parity byte of the block is owned by exactly one codeword symbol
    std::vector<uint8_t> owner(f, 0);
    for (uint32_t w = 0; w < W; w++) {
      const uint32_t kw = rs_cw_info(k, W, w);
      for (uint32_t s = 0; s < kw + OFDM_RS_PARITY; s++) {
        const uint32_t at = rs_sym_pos(k, W, w, s);
        CHECK(at < f);
        CHECK(s < kw ? (at < k && at % W == w && at / W == s) : (at >= k && (at - k) % W == w && (at - k) / W == s - kw));
        owner[at]++;
      }
    }
    for (uint32_t at = 0; at < f; at++) CHECK(owner[at] == 1);
  }
  // the known values
  CHECK(rs_block_len(4) == 36 && rs_block_len(223) == 255 && rs_block_len(224) == 288 && rs_block_len(1784) == 2040);
  CHECK(rs_block_len(1785) == 2073 && rs_block_len(3568) == 4080 && rs_block_len(3569) == 4113);
  // every length up to 4091, and far ones, accepted or refused as the count says
  uint32_t nblocks = 0;
  for (uint32_t m = 0; m <= 4091; m++) {
    uint32_t k = 0, n = 77;
    CHECK(reached[m] <= 1);
    CHECK(rs_info_len(m, &k) == (reached[m] == 1));
    CHECK((rs_payload_len(m, &n) == OFDM_OK) == (reached[m] == 1));
    if (!reached[m]) CHECK(n == 77);
    nblocks += (uint32_t)reached[m];
  }
  CHECK(nblocks == OFDM_RS_MAX_PAYLOAD + 1u);
  const uint32_t bad[] = {0, 1, 35, 256, 287, 511, 542, 4081, 4112, 4113, 0x7FFFFFFFu, 0xFFFFFFFFu};
  uint32_t v = 0;
  for (uint32_t m : bad) CHECK(!rs_info_len(m, &v) && rs_payload_len(m, &v) == OFDM_E_INVAL);
  CHECK(rs_coded_len(OFDM_RS_MAX_PAYLOAD + 1u, &v) == OFDM_E_INVAL && rs_coded_len(0xFFFFFFFFu, &v) == OFDM_E_INVAL);
  CHECK(rs_coded_len(0, nullptr) == OFDM_E_INVAL && rs_payload_len(36, nullptr) == OFDM_E_INVAL);

  // batch tables: lengths that are no block take no room and reach no input
  {
    const uint32_t len[] = {36, 0, 4080, 35, 255, 256, 4081, 0xFFFFFFFFu, 288};
    const size_t nb = sizeof(len) / sizeof(len[0]);
    std::vector<uint64_t> in_off(nb), out_off(nb + 1, 77);
    uint64_t o = 0, reach = 0;
    for (size_t b = 0; b < nb; b++) {
      uint32_t k;
      in_off[b] = o;
      if (rs_info_len(len[b], &k)) reach = o + len[b];
      o += rs_info_len(len[b], &k) ? len[b] : 3;
    }
    std::vector<RsBlk> blk(nb);
    uint64_t nvalid = 0, ext = 0;
    const uint64_t total = rs_plan_decode(in_off.data(), len, nb, blk.data(), out_off.data(), &nvalid, &ext);
    CHECK(total == 0 + 3564 + 219 + 220 && out_off[nb] == total && nvalid == 4 && ext == reach);
    uint64_t at = 0;
    for (size_t b = 0; b < nb; b++) {
      uint32_t k;
      CHECK(out_off[b] == at && blk[b].out_off == at && blk[b].in_off == in_off[b] && blk[b].len == len[b] && blk[b].pad == 0);
      if (rs_info_len(len[b], &k)) at += k - 4;
    }
    const uint32_t none[] = {35, 256};
    const uint64_t off2[] = {0, 5};
    CHECK(rs_plan_decode(off2, none, 2, blk.data(), out_off.data(), &nvalid, &ext) == 0 && nvalid == 0 && ext == 0);
    CHECK(rs_plan_decode(nullptr, nullptr, 0, nullptr, out_off.data(), &nvalid, &ext) == 0 && out_off[0] == 0);
  }
  {
    const uint32_t plen[] = {0, 3, 3564, 219, 220};
    const uint64_t poff[] = {0, 0, 100, 4000, 9};
    std::vector<RsBlk> blk(5);
    std::vector<uint64_t> coff(6, 77);
    uint64_t ext = 0;
    const uint64_t total = rs_plan_encode(poff, plen, 5, blk.data(), coff.data(), &ext);
    CHECK(total == 36 + 39 + 4080 + 255 + 288 && coff[5] == total && ext == 4219);
    CHECK(coff[0] == 0 && coff[1] == 36 && coff[2] == 75 && coff[3] == 4155 && coff[4] == 4410);
    for (int b = 0; b < 5; b++) CHECK(blk[b].in_off == poff[b] && blk[b].out_off == coff[b] && blk[b].len == plen[b]);
    const uint32_t over[] = {3, 3565};
    CHECK(rs_plan_encode(poff, over, 2, blk.data(), coff.data(), &ext) == ~0ull);
    CHECK(rs_plan_encode(nullptr, nullptr, 0, nullptr, coff.data(), &ext) == 0 && coff[0] == 0 && ext == 0);
  }
  printf("rs_plan_check ok\n");
  return 0;
}
