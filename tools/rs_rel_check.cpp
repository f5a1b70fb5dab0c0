// rs_rel_check.cpp -- the host arithmetic of decoding with reliabilities (ofdm_uhd_amd/csrc/rs_plan.h) as a program of its
// own: the configuration rule (struct size, M, reserved words, the default), the reliability of a byte from its eight
// values over every value, where a batch's reliabilities lie and how far they reach, and the layout of an
// ofdm_rs_rel_from_soft batch.
// Needs no GPU and no HIP.  For a sanitizer run build it with
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include -o rs_rel_check tools/rs_rel_check.cpp
// tests/test_rs_rel_host.py builds and runs it without the sanitizers.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

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
  // the configuration
  static_assert(sizeof(ofdm_rs_rel_cfg) == 32, "ofdm_rs_rel_cfg is 32 bytes");
  uint32_t M = 77;
  CHECK(rs_rel_max_erasures(nullptr, &M) && M == 28 && RS_REL_DEFAULT_ERASURES == 28);
  for (uint32_t m = 0; m <= 40; m++) {
    ofdm_rs_rel_cfg c;
    memset(&c, 0, sizeof(c));
    c.struct_size = sizeof(c);
    c.max_erasures = m;
    M = 77;
    CHECK(rs_rel_max_erasures(&c, &M) == (m <= OFDM_RS_PARITY));
    CHECK(M == (m <= OFDM_RS_PARITY ? m : 77u));
    for (int r = 0; r < 6; r++) {
      ofdm_rs_rel_cfg d = c;
      d.reserved[r] = 1u << r;
      CHECK(!rs_rel_max_erasures(&d, &M));
    }
    ofdm_rs_rel_cfg d = c;
    d.struct_size = 28;
    CHECK(!rs_rel_max_erasures(&d, &M));
    d.struct_size = 36;
    CHECK(!rs_rel_max_erasures(&d, &M));
  }

  // the reliability of a byte: every value in every place, -128 read as 127, never above 127
  for (int place = 0; place < 8; place++)
    for (int x = -128; x <= 127; x++) {
      int8_t v[8];
      for (int j = 0; j < 8; j++) v[j] = (int8_t)(j & 1 ? 127 : -128);
      v[place] = (int8_t)x;
      const uint32_t want = x == -128 ? 127u : (uint32_t)(x < 0 ? -x : x);
      CHECK(rs_rel_of_values(v) == want);
    }
  {
    const int8_t a[8] = {5, -4, 3, -128, 9, 100, -100, 7}, z[8] = {90, 90, 90, 0, 90, 90, 90, 90};
    CHECK(rs_rel_of_values(a) == 3 && rs_rel_of_values(z) == 0);
  }

  // where the reliabilities lie: at the blocks' offsets by default, only blocks count for the extent
  {
    const uint32_t len[] = {36, 35, 4080, 256, 288};
    const uint64_t coff[] = {0, 36, 100, 5000, 6000}, roff[] = {9000, 1, 17, 99999, 4097};
    uint64_t out[5], ext = 77;
    rs_plan_rel(coff, nullptr, len, 5, out, &ext);
    for (int b = 0; b < 5; b++) CHECK(out[b] == coff[b]);
    CHECK(ext == 6288);
    rs_plan_rel(coff, roff, len, 5, out, &ext);
    for (int b = 0; b < 5; b++) CHECK(out[b] == roff[b]);
    CHECK(ext == 9036);  // (entry 3, no block, reaches nothing)
    const uint32_t none[] = {35, 256};
    rs_plan_rel(coff, roff, none, 2, out, &ext);
    CHECK(ext == 0);
    rs_plan_rel(nullptr, nullptr, nullptr, 0, out, &ext);
    CHECK(ext == 0);
  }

  // reliabilities from values: the running sum, every length converted, offsets in values that are multiples of 8
  {
    const uint32_t len[] = {1, 0, 3, 4080, 5};
    const uint64_t soff[] = {0, 8, 8, 40, 80000};
    std::vector<RsBlk> blk(5);
    std::vector<uint64_t> roff(6, 77);
    uint64_t ext = 0;
    const uint64_t total = rs_plan_rel_soft(soff, len, 5, blk.data(), roff.data(), &ext);
    CHECK(total == 4089 && roff[5] == total && ext == 80040);
    uint64_t at = 0;
    for (int b = 0; b < 5; b++) {
      CHECK(roff[b] == at && blk[b].out_off == at && blk[b].in_off == soff[b] && blk[b].len == len[b] && blk[b].pad == 0);
      at += len[b];
    }
    const uint64_t odd[] = {0, 8, 12, 40, 80000};
    std::vector<uint64_t> keep(6, 77);
    CHECK(rs_plan_rel_soft(odd, len, 5, blk.data(), keep.data(), &ext) == ~0ull);
    for (uint64_t v : keep) CHECK(v == 77);  // refused before anything is written
    CHECK(rs_plan_rel_soft(nullptr, nullptr, 0, nullptr, roff.data(), &ext) == 0 && roff[0] == 0 && ext == 0);
    const uint32_t zero[] = {0, 0};
    CHECK(rs_plan_rel_soft(soff, zero, 2, blk.data(), roff.data(), &ext) == 0 && ext == 0 && roff[2] == 0);
  }
  printf("rs_rel_check ok\n");
  return 0;
}
