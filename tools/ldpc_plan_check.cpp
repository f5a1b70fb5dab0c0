// ldpc_plan_check.cpp -- the LDPC layer's host arithmetic (ofdm_uhd_amd/csrc/ldpc_plan.h) as a program of its own: the
// base matrix (entry count, degrees, no 4-cycles), an encoded word's zero syndrome by the header's own recursion, the
// coded length and its inverse as a bijection over every length 0 .. 4200, every sent byte of a block owned by exactly
// one codeword, and the codeword maps of encode and decode batches.
// Needs no GPU and no HIP.  For a sanitizer run build it with
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include -o ldpc_plan_check tools/ldpc_plan_check.cpp
// tests/test_ldpc_host.py builds and runs it without the sanitizers.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../ofdm_uhd_amd/csrc/ldpc_plan.h"

#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #c); \
      exit(1);                                                    \
    }                                                             \
  } while (0)

// lane z at bit z: rot(x, s)[z] = x[(z + s) mod 64] is a rotate right
static uint64_t rot(uint64_t x, int s) { return s ? (x >> s) | (x << (64 - s)) : x; }

int main() {
  const LdpcTable& T = LDPC_TABLE;
  // ---- the table ------------------------------------------------------------------------------------------------
  int entries = 0;
  for (int i = 0; i < LDPC_ROWS; i++) {
    CHECK(T.deg[i] == (i == 6 ? 6 : 7));
    int seen = 0;
    for (int j = 0; j < LDPC_COLS; j++) {
      CHECK(T.shift[i][j] >= -1 && T.shift[i][j] < LDPC_Z);
      if (T.shift[i][j] >= 0) {
        CHECK(T.col[i][seen] == j && T.sh[i][seen] == T.shift[i][j]);
        seen++;
      }
    }
    CHECK(seen == T.deg[i]);
    entries += seen;
  }
  CHECK(entries == 83 && T.entries == 83);
  for (int r = 0; r < LDPC_ROWS; r++)
    for (int r2 = r + 1; r2 < LDPC_ROWS; r2++)
      for (int c = 0; c < LDPC_COLS; c++)
        for (int c2 = c + 1; c2 < LDPC_COLS; c2++) {
          if (T.shift[r][c] < 0 || T.shift[r2][c] < 0 || T.shift[r][c2] < 0 || T.shift[r2][c2] < 0) continue;
          CHECK(((T.shift[r][c] - T.shift[r2][c] - T.shift[r][c2] + T.shift[r2][c2]) % 64 + 64) % 64 != 0);  // no 4-cycle
        }
  // ---- the parity recursion solves every check ---------------------------------------------------------------------
  {
    uint64_t x[LDPC_COLS], lam[LDPC_ROWS], seed = 0x9E3779B97F4A7C15ull;
    for (int rep = 0; rep < 50; rep++) {
      for (int j = 0; j < 12; j++) {
        seed = seed * 6364136223846793005ull + 1442695040888963407ull;
        x[j] = seed ^ (seed >> 29);
      }
      uint64_t p0 = 0;
      for (int i = 0; i < LDPC_ROWS; i++) {
        lam[i] = 0;
        for (int j = 0; j < 12; j++)
          if (T.shift[i][j] >= 0) lam[i] ^= rot(x[j], T.shift[i][j]);
        p0 ^= lam[i];
      }
      x[12] = p0;
      x[13] = lam[0] ^ rot(p0, 1);
      for (int i = 1; i <= 10; i++) x[13 + i] = lam[i] ^ x[12 + i] ^ (i == 6 ? p0 : 0ull);
      for (int i = 0; i < LDPC_ROWS; i++) {
        uint64_t s = 0;
        for (int e = 0; e < T.deg[i]; e++) s ^= rot(x[T.col[i][e]], T.sh[i][e]);
        CHECK(s == 0);
      }
    }
  }
  // ---- lengths: n -> m strictly increasing, inverted by ldpc_payload_len; every m accepted or refused as the count says --
  std::vector<int> reached(4200 + 1, 0);
  uint32_t prev = 0;
  for (uint32_t n = 0; n <= 4200; n++) {
    uint32_t m = 77;
    if (n > OFDM_LDPC_MAX_PAYLOAD) {
      CHECK(ldpc_coded_len(n, &m) == OFDM_E_INVAL && m == 77);
      continue;
    }
    CHECK(ldpc_coded_len(n, &m) == OFDM_OK);
    const uint32_t k = n + 4u, W = ldpc_words(k);
    CHECK(W >= 1 && W <= LDPC_MAX_WORDS && LDPC_CW_INFO * W >= k && LDPC_CW_INFO * (W - 1u) < k);
    CHECK(m == k + LDPC_CW_PARITY * W && m <= OFDM_LDPC_MAX_CODED && m <= 2u * n + 104u);
    CHECK(n == 0 || m - prev == 1 || m - prev == 97);
    prev = m;
    reached[m]++;
    uint32_t back = 0;
    CHECK(ldpc_is_block(m) && ldpc_payload_len(m, &back) == OFDM_OK && back == n);
    CHECK(ldpc_block_words(m) == W && ldpc_block_info(m) == k);
    // codewords: k_w sums to k; every sent byte of the block belongs to exactly one codeword
    std::vector<uint8_t> owner(m, 0);
    uint32_t sum = 0;
    for (uint32_t w = 0; w < W; w++) {
      const uint32_t kw = ldpc_cw_info(k, w);
      CHECK(kw >= 1 && kw <= LDPC_CW_INFO && (kw == LDPC_CW_INFO || w == W - 1u));
      sum += kw;
      for (uint32_t s = 0; s < kw + LDPC_CW_PARITY; s++) {
        const uint32_t at = LDPC_CW_SENT * w + s;
        CHECK(at < m);
        owner[at]++;
      }
    }
    CHECK(sum == k);
    for (uint32_t at = 0; at < m; at++) CHECK(owner[at] == 1);
  }
  uint32_t v = 0;
  CHECK(ldpc_coded_len(0, &v) == OFDM_OK && v == 100);
  CHECK(ldpc_coded_len(92, &v) == OFDM_OK && v == 192);
  CHECK(ldpc_coded_len(93, &v) == OFDM_OK && v == 289);
  CHECK(ldpc_coded_len(OFDM_LDPC_MAX_PAYLOAD, &v) == OFDM_OK && v == OFDM_LDPC_MAX_CODED);
  uint32_t nblocks = 0;
  for (uint32_t m = 0; m <= 4200; m++) {
    uint32_t n = 77;
    CHECK(reached[m] <= 1);
    CHECK(ldpc_is_block(m) == (reached[m] == 1));
    CHECK((ldpc_payload_len(m, &n) == OFDM_OK) == (reached[m] == 1));
    if (!reached[m]) CHECK(n == 77);
    nblocks += (uint32_t)reached[m];
  }
  CHECK(nblocks == OFDM_LDPC_MAX_PAYLOAD + 1u);
  const uint32_t bad[] = {0, 1, 99, 193, 288, 4033, 4128, 0x7FFFFFFFu, 0xFFFFFFFFu};
  for (uint32_t m : bad) CHECK(!ldpc_is_block(m) && ldpc_payload_len(m, &v) == OFDM_E_INVAL);
  CHECK(ldpc_coded_len(0xFFFFFFFFu, &v) == OFDM_E_INVAL);
  CHECK(ldpc_coded_len(0, nullptr) == OFDM_E_INVAL && ldpc_payload_len(100, nullptr) == OFDM_E_INVAL);

  // ---- codeword maps: every length 0 .. 4200 as one decode batch; lengths that are no block take no room, have no
  // codeword and reach no input
  {
    const size_t nb = 4201;
    std::vector<uint32_t> len(nb);
    std::vector<uint64_t> in_off(nb), out_off(nb + 1, 77);
    uint64_t o = 0, reach = 0, want_cw = 0, want_total = 0;
    for (size_t b = 0; b < nb; b++) {
      len[b] = (uint32_t)b;
      in_off[b] = o;
      if (ldpc_is_block(len[b])) {
        reach = o + 8ull * len[b];
        want_cw += ldpc_block_words(len[b]);
        want_total += ldpc_block_info(len[b]) - 4u;
      }
      o += 8ull * len[b];
    }
    std::vector<LdpcBlk> blk(nb);
    std::vector<uint32_t> cw(nb * LDPC_MAX_WORDS, 0xFFFFFFFFu);
    uint64_t ncw = 0, ext = 0;
    const uint64_t total = ldpc_plan_decode(in_off.data(), len.data(), nb, 8, blk.data(), out_off.data(), cw.data(), &ncw, &ext);
    CHECK(total == want_total && out_off[nb] == total && ncw == want_cw && ext == reach);
    uint64_t at = 0, c = 0;
    for (size_t b = 0; b < nb; b++) {
      CHECK(out_off[b] == at && blk[b].out_off == at && blk[b].in_off == in_off[b] && blk[b].len == len[b] && blk[b].cw0 == c);
      if (!ldpc_is_block(len[b])) continue;
      for (uint32_t w = 0; w < ldpc_block_words(len[b]); w++) CHECK(cw[c + w] == b);
      c += ldpc_block_words(len[b]);
      at += ldpc_block_info(len[b]) - 4u;
    }
    for (uint64_t k = ncw; k < cw.size(); k++) CHECK(cw[k] == 0xFFFFFFFFu);  // nothing written behind the map
    uint64_t ncw2 = 5;
    CHECK(ldpc_plan_decode(in_off.data(), len.data(), nb, 1, blk.data(), out_off.data(), nullptr, &ncw2, &ext) == want_total && ncw2 == want_cw);
    const uint32_t none[] = {99, 193};
    const uint64_t off2[] = {0, 5};
    CHECK(ldpc_plan_decode(off2, none, 2, 1, blk.data(), out_off.data(), cw.data(), &ncw, &ext) == 0 && ncw == 0 && ext == 0);
    CHECK(ldpc_plan_decode(nullptr, nullptr, 0, 1, nullptr, out_off.data(), nullptr, &ncw, &ext) == 0 && out_off[0] == 0);
  }
  {
    const uint32_t plen[] = {0, 92, 93, 2012, 188};
    const uint64_t poff[] = {0, 0, 100, 4000, 9};
    std::vector<LdpcBlk> blk(5);
    std::vector<uint64_t> coff(6, 77);
    std::vector<uint32_t> cw(5 * LDPC_MAX_WORDS, 0xFFFFFFFFu);
    uint64_t ncw = 0, ext = 0;
    const uint64_t total = ldpc_plan_encode(poff, plen, 5, blk.data(), coff.data(), cw.data(), &ncw, &ext);
    CHECK(total == 100 + 192 + 289 + 4032 + 384 && coff[5] == total && ext == 6012 && ncw == 1 + 1 + 2 + 21 + 2);
    CHECK(coff[0] == 0 && coff[1] == 100 && coff[2] == 292 && coff[3] == 581 && coff[4] == 4613);
    const uint32_t cw0[] = {0, 1, 2, 4, 25};
    for (int b = 0; b < 5; b++) CHECK(blk[b].in_off == poff[b] && blk[b].out_off == coff[b] && blk[b].len == plen[b] && blk[b].cw0 == cw0[b]);
    CHECK(cw[0] == 0 && cw[1] == 1 && cw[2] == 2 && cw[3] == 2 && cw[4] == 3 && cw[24] == 3 && cw[25] == 4 && cw[26] == 4 && cw[27] == 0xFFFFFFFFu);
    const uint32_t over[] = {3, 2013};
    CHECK(ldpc_plan_encode(poff, over, 2, blk.data(), coff.data(), cw.data(), &ncw, &ext) == ~0ull);
    CHECK(ldpc_plan_encode(nullptr, nullptr, 0, nullptr, coff.data(), nullptr, &ncw, &ext) == 0 && coff[0] == 0 && ext == 0 && ncw == 0);
  }
  printf("ldpc_plan_check ok\n");
  return 0;
}
