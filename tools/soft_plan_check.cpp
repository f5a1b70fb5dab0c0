// soft_plan_check.cpp -- the host arithmetic of the soft-decision receive option (ofdm_uhd_amd/csrc/soft_plan.h) as a
// program of its own: value offsets, carrier and symbol counts, the map between the frame sink's stream bits and the
// decoder's input order, and the tiles k_soft_demap walks.  Needs no GPU and no HIP.  For a sanitizer run build it with
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include -o soft_plan_check tools/soft_plan_check.cpp
// tests/test_soft_host.py builds and runs it without the sanitizers.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../ofdm_uhd_amd/csrc/soft_plan.h"

#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #c); \
      exit(1);                                                    \
    }                                                             \
  } while (0)

int main() {
  // value offsets: 8 per payload byte, an empty call
  {
    const uint64_t pay[] = {0, 0, 1, 301, 301, 4392};
    std::vector<uint64_t> off(6, 77);
    CHECK(soft_plan_offsets(pay, 5, off.data()) == 8 * 4392);
    for (int k = 0; k < 6; k++) CHECK(off[k] == 8 * pay[k]);
    uint64_t one = 5;
    const uint64_t zero = 0;
    CHECK(soft_plan_offsets(&zero, 0, &one) == 0 && one == 0);
  }
  const uint32_t bits[] = {1, 2, 3, 4, 6, 8};
  const uint32_t nmaps[] = {1, 5, 8, 43, 48, 187, 200};
  const uint32_t plens[] = {0, 1, 2, 3, 29, 100, 511, 4091};
  for (uint32_t nbits : bits)
    for (uint32_t nmap : nmaps)
      for (uint32_t plen : plens) {
        const uint64_t ncar = soft_carriers(plen, nbits), nsym = soft_symbols(plen, nmap, nbits);
        if (plen == 0) {
          CHECK(ncar == 0 && nsym == 0);
          continue;
        }
        // the carriers reach the last payload bit and not a whole carrier further; the symbols hold them
        CHECK(ncar * nbits >= 8ull * (4 + plen) && (ncar - 1) * nbits < 8ull * (4 + plen));
        CHECK(nsym * nmap >= ncar && (nsym - 1) * nmap < ncar);
        // the map is a bijection between the packet's stream bits and [0, 8 plen)
        std::vector<uint8_t> seen(8 * (size_t)plen, 0);
        uint64_t hits = 0;
        for (uint64_t beta = 0; beta < nsym * nmap * (uint64_t)nbits + 64; beta++) {
          const int64_t o = soft_out_index(beta, plen);
          if (o < 0) {
            CHECK((beta >> 3) < 4 || (beta >> 3) >= 4ull + plen);
            continue;
          }
          CHECK((uint64_t)o < 8ull * plen && !seen[(size_t)o] && soft_beta((uint64_t)o) == beta);
          CHECK(beta < ncar * nbits);  // inside the carriers counted
          seen[(size_t)o] = 1;
          hits++;
        }
        CHECK(hits == 8ull * plen);
        // the tiles: byte-aligned, their packet parts in whole 8-value groups, covering [0, 8 plen) once and in order
        uint64_t next = 0;
        for (uint64_t t0 = 0; t0 < ncar; t0 += SOFT_TILE_CARRIERS) {
          const SoftTile t = soft_tile(t0, nbits, plen);
          CHECK(t.byte0 * 8 == t0 * nbits && t.nbytes == 32 * nbits && t.nbytes <= SOFT_TILE_MAX_BYTES);
          CHECK(t.lo <= t.hi && t.hi <= 8 * t.nbytes && t.lo % 8 == 0 && t.hi % 8 == 0);
          if (t.hi == t.lo) continue;
          CHECK(t.out0 == next && t.out0 % 8 == 0);
          // staging index i of the tile is value out0 + (i - lo): the same place the per-bit map gives
          for (uint32_t i = t.lo; i < t.hi; i += 5) {
            const uint64_t beta = 8 * (t.byte0 + (i >> 3)) + 7 - (i & 7);
            CHECK(soft_out_index(beta, plen) == (int64_t)(t.out0 + (i - t.lo)));
          }
          next += t.hi - t.lo;
        }
        CHECK(next == 8ull * plen);
      }
  // a tile wholly in front of or behind the packet stores nothing
  CHECK(soft_tile(0, 1, 0).hi == soft_tile(0, 1, 0).lo);
  CHECK(soft_tile(256, 8, 10).hi == soft_tile(256, 8, 10).lo);
  CHECK(soft_tile(0, 1, 100).lo == 32 && soft_tile(0, 1, 100).hi == 256 && soft_tile(0, 1, 100).out0 == 0);
  CHECK(soft_carriers(5, 0) == 0 && soft_symbols(5, 0, 2) == 0);
  printf("soft_plan_check ok\n");
  return 0;
}
