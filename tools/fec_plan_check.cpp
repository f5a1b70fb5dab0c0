// fec_plan_check.cpp -- the coded-link layer's host arithmetic (ofdm_uhd_amd/csrc/fec_plan.h) as a program of its own:
// block lengths, trellis geometry, the decode batch layout and the slicing of a batch over the bounded workspace.
// Needs no GPU and no HIP.  For a sanitizer run build it with
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include -o fec_plan_check tools/fec_plan_check.cpp
// tests/test_fec_host.py builds and runs it without the sanitizers.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../ofdm_uhd_amd/csrc/fec_plan.h"

#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #c); \
      exit(1);                                                    \
    }                                                             \
  } while (0)

int main() {
  // lengths and their refusals
  uint32_t v = 0;
  for (uint32_t n = 0; n <= OFDM_FEC_MAX_PAYLOAD; n++) {
    CHECK(fec_coded_len(n, &v) == OFDM_OK && v == 2 * n + 10);
    uint32_t back = 0;
    CHECK(fec_payload_len(v, &back) == OFDM_OK && back == n);
    CHECK(fec_steps(v) == 8 * (n + 4) + 6);
    CHECK(64ull * fec_chunks(v) >= fec_steps(v) && 64ull * (fec_chunks(v) - 1) < fec_steps(v));
    CHECK((8 * v) % 16 == 0);  // every column count divides the block's bits
  }
  CHECK(fec_chunks(OFDM_FEC_MAX_CODED) == 256);
  CHECK(fec_coded_len(OFDM_FEC_MAX_PAYLOAD + 1, &v) == OFDM_E_INVAL && fec_coded_len(0xFFFFFFFFu, &v) == OFDM_E_INVAL);
  CHECK(fec_coded_len(0, nullptr) == OFDM_E_INVAL && fec_payload_len(10, nullptr) == OFDM_E_INVAL);
  const uint32_t bad[] = {0, 1, 9, 11, 4089, 4091, 4092, 0x7FFFFFFEu, 0xFFFFFFFEu, 0xFFFFFFFFu};
  for (uint32_t m : bad) CHECK(!fec_is_block(m) && fec_payload_len(m, &v) == OFDM_E_INVAL);
  for (uint32_t c = 0; c <= 40; c++) {
    const int l = fec_log2_cols(c);
    CHECK((l >= 0) == (c == 1 || c == 2 || c == 4 || c == 8 || c == 16));
    if (l >= 0) CHECK((1u << l) == c);
  }
  CHECK(fec_log2_cols(0xFFFFFFFFu) < 0);

  // batch layout: lengths that are no block take no room, reach no input and size no workspace
  {
    const uint32_t len[] = {10, 0, 4090, 9, 12, 11, 4091, 0xFFFFFFFFu, 2062};
    const size_t nb = sizeof(len) / sizeof(len[0]);
    std::vector<uint64_t> in_off(nb), out_off(nb + 1, 77);
    uint64_t o = 0;
    for (size_t k = 0; k < nb; k++) {
      in_off[k] = o;
      o += fec_is_block(len[k]) ? len[k] : 3;
    }
    for (uint64_t unit : {1ull, 8ull}) {
      std::vector<FecBlk> blk(nb);
      uint64_t stride = 0, ext = 0;
      const uint64_t total = fec_plan_decode(in_off.data(), len, nb, unit, blk.data(), out_off.data(), &stride, &ext);
      CHECK(total == 0 + 2040 + 1 + 1026 && out_off[nb] == total);
      CHECK(stride == 64 * 256);
      uint64_t at = 0, reach = 0;
      for (size_t k = 0; k < nb; k++) {
        CHECK(out_off[k] == at && blk[k].out_off == at && blk[k].in_off == in_off[k] && blk[k].len == len[k]);
        if (!fec_is_block(len[k])) continue;
        at += (len[k] - 10) / 2;
        if (in_off[k] + unit * len[k] > reach) reach = in_off[k] + unit * len[k];
      }
      CHECK(ext == reach && ext == (unit == 1 ? in_off[8] + 2062 : in_off[2] + 8 * 4090));
    }
    // not one block among them
    const uint32_t none[] = {0, 9, 11};
    std::vector<FecBlk> blk(3);
    uint64_t stride = 1, ext = 1;
    CHECK(fec_plan_decode(in_off.data(), none, 3, 1, blk.data(), out_off.data(), &stride, &ext) == 0 && stride == 0 && ext == 0);
    CHECK(fec_plan_decode(in_off.data(), none, 0, 1, blk.data(), out_off.data(), &stride, &ext) == 0 && out_off[0] == 0);
  }

  // slicing: the slices cover the batch exactly, none is empty, and none needs more than the cap (one block always fits)
  const uint64_t caps[] = {0, 8, 512, 128 << 10, FEC_WS_MAX_BYTES, ~0ull};
  const uint64_t strides[] = {0, 64, 64 * 129, 64 * 256};
  const uint64_t counts[] = {0, 1, 2, 4063, 4064, 4065, 65536, 1ull << 31};
  for (uint64_t cap : caps)
    for (uint64_t st : strides)
      for (uint64_t n : counts) {
        const uint64_t per = fec_slice_blocks(n, st, cap);
        if (n == 0) {
          CHECK(per == 0);
          continue;
        }
        CHECK(per >= 1 && per <= n);
        CHECK(per == 1 || per * st * 8 <= cap);
        uint64_t covered = 0, slices = 0;
        for (uint64_t b0 = 0; b0 < n && slices < 100000; b0 += per, slices++) covered += (per < n - b0) ? per : n - b0;
        if (slices < 100000) CHECK(covered == n);
      }
  CHECK(fec_slice_blocks(65536, 64 * 129, FEC_WS_MAX_BYTES) == FEC_WS_MAX_BYTES / (64 * 129 * 8));
  printf("fec_plan_check ok\n");
  return 0;
}
