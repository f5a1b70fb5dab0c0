// ldpc_rate_plan_check.cpp -- the LDPC layer's host arithmetic (ofdm_uhd_amd/csrc/ldpc_plan.h) at every rate, as a program
// of its own, next to ldpc_plan_check.cpp (which pins the rate-1/2 names): per rate the base matrix (rows, entry count,
// degrees, the parity part's shape, no 4-cycles over all 24 columns), an encoded word's zero syndrome by the header's
// recursion and a broken check after any single flipped parity bit, the coded length and its inverse as a bijection
// over every length 0 .. 4200, every sent byte of a block owned by exactly one codeword, the codeword maps of encode and
// decode batches, and the names without a rate as the rate-1/2 case.
// Needs no GPU and no HIP.  For a sanitizer run build it with
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include -o ldpc_rate_plan_check tools/ldpc_rate_plan_check.cpp
// tests/test_ldpc_rates_host.py builds and runs it both ways.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../ofdm_uhd_amd/csrc/ldpc_plan.h"

#define CHECK(c)                                                     \
  do {                                                               \
    if (!(c)) {                                                      \
      fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #c); \
      exit(1);                                                       \
    }                                                                \
  } while (0)

// lane z at bit z: rot(x, s)[z] = x[(z + s) mod 64] is a rotate right
static uint64_t rot(uint64_t x, int s) { return s ? (x >> s) | (x << (64 - s)) : x; }

static bool all_checks_hold(const LdpcTable& T, const uint64_t* x) {
  for (int i = 0; i < T.mb; i++) {
    uint64_t s = 0;
    for (int e = 0; e < T.deg[i]; e++) s ^= rot(x[T.col[i][e]], T.sh[i][e]);
    if (s) return false;
  }
  return true;
}

struct Want {
  int mb, entries, info_entries, max_deg;
  int deg[LDPC_ROWS];
  uint32_t max_payload;
};

static void check_rate(uint32_t rate, const LdpcTable& T, const Want& W_) {
  const uint32_t KI = ldpc_rate_info(rate), PB = ldpc_rate_parity(rate);
  // ---- the table ------------------------------------------------------------------------------------------------
  CHECK(T.mb == W_.mb && T.kb == LDPC_COLS - T.mb && T.mid == T.mb / 2 && (int)ldpc_rate_rows(rate) == T.mb);
  CHECK(KI == 8u * (uint32_t)T.kb && PB == 8u * (uint32_t)T.mb && KI + PB == LDPC_CW_SENT);
  int entries = 0, info_entries = 0;
  for (int i = 0; i < LDPC_ROWS; i++) {
    CHECK(T.deg[i] == (i < T.mb ? W_.deg[i] : 0) && T.deg[i] <= LDPC_MAX_DEG);
    int seen = 0;
    for (int j = 0; j < LDPC_COLS; j++) {
      CHECK(T.shift[i][j] >= -1 && T.shift[i][j] < LDPC_Z);
      if (T.shift[i][j] >= 0) {
        CHECK(T.col[i][seen] == j && T.sh[i][seen] == T.shift[i][j]);
        seen++;
        info_entries += j < T.kb;
      }
    }
    CHECK(seen == T.deg[i]);
    entries += seen;
  }
  CHECK(entries == W_.entries && T.entries == entries && info_entries == W_.info_entries && T.max_deg == W_.max_deg);
  // the parity part: column kb in rows 0 (1), mid (0) and mb - 1 (1), the staircase behind it
  for (int i = 0; i < T.mb; i++) {
    const int want = (i == 0 || i == T.mb - 1) ? 1 : (i == T.mid ? 0 : -1);
    CHECK(T.shift[i][T.kb] == want);
    for (int c = 0; c < T.mb - 1; c++) CHECK(T.shift[i][T.kb + 1 + c] == ((i == c || i == c + 1) ? 0 : -1));
  }
  for (int r = 0; r < T.mb; r++)
    for (int r2 = r + 1; r2 < T.mb; r2++)
      for (int c = 0; c < LDPC_COLS; c++)
        for (int c2 = c + 1; c2 < LDPC_COLS; c2++) {
          if (T.shift[r][c] < 0 || T.shift[r2][c] < 0 || T.shift[r][c2] < 0 || T.shift[r2][c2] < 0) continue;
          CHECK(((T.shift[r][c] - T.shift[r2][c] - T.shift[r][c2] + T.shift[r2][c2]) % 64 + 64) % 64 != 0);  // no 4-cycle
        }
  // ---- the parity recursion solves every check, and no other parity does ---------------------------------------------
  {
    uint64_t x[LDPC_COLS], lam[LDPC_ROWS], seed = 0x9E3779B97F4A7C15ull + rate;
    for (int rep = 0; rep < 20; rep++) {
      for (int j = 0; j < T.kb; j++) {
        seed = seed * 6364136223846793005ull + 1442695040888963407ull;
        x[j] = seed ^ (seed >> 29);
      }
      uint64_t p0 = 0;
      for (int i = 0; i < T.mb; i++) {
        lam[i] = 0;
        for (int j = 0; j < T.kb; j++)
          if (T.shift[i][j] >= 0) lam[i] ^= rot(x[j], T.shift[i][j]);
        p0 ^= lam[i];
      }
      x[T.kb] = p0;
      x[T.kb + 1] = lam[0] ^ rot(p0, 1);
      for (int i = 1; i <= T.mb - 2; i++) x[T.kb + 1 + i] = lam[i] ^ x[T.kb + i] ^ (i == T.mid ? p0 : 0ull);
      CHECK(all_checks_hold(T, x));
      if (rep < 2)
        for (int j = T.kb; j < LDPC_COLS; j++)
          for (int z = 0; z < LDPC_Z; z++) {
            x[j] ^= 1ull << z;
            CHECK(!all_checks_hold(T, x));
            x[j] ^= 1ull << z;
          }
    }
  }
  // ---- lengths: n -> m strictly increasing, inverted by ldpc_payload_len_rate; every m accepted or refused as the count says
  CHECK(ldpc_rate_max_payload(rate) == W_.max_payload && W_.max_payload == LDPC_MAX_WORDS * KI - 4u);
  std::vector<int> reached(4200 + 1, 0);
  uint32_t prev = 0;
  for (uint32_t n = 0; n <= 4200; n++) {
    uint32_t m = 77;
    if (n > W_.max_payload) {
      CHECK(ldpc_coded_len_rate(rate, n, &m) == OFDM_E_INVAL && m == 77);
      continue;
    }
    CHECK(ldpc_coded_len_rate(rate, n, &m) == OFDM_OK);
    const uint32_t k = n + 4u, W = ldpc_words_rate(rate, k);
    CHECK(W >= 1 && W <= LDPC_MAX_WORDS && KI * W >= k && KI * (W - 1u) < k);
    CHECK(m == k + PB * W && m <= OFDM_LDPC_MAX_CODED && m <= 2u * n + 104u && m > n);
    CHECK(n == 0 || m - prev == 1 || m - prev == PB + 1u);
    prev = m;
    reached[m]++;
    uint32_t back = 0;
    CHECK(ldpc_is_block_rate(rate, m) && ldpc_payload_len_rate(rate, m, &back) == OFDM_OK && back == n);
    CHECK(ldpc_block_words(m) == W && ldpc_block_info_rate(rate, m) == k);
    std::vector<uint8_t> owner(m, 0);
    uint32_t sum = 0;
    for (uint32_t w = 0; w < W; w++) {
      const uint32_t kw = ldpc_cw_info_rate(rate, k, w);
      CHECK(kw >= 1 && kw <= KI && (kw == KI || w == W - 1u));
      sum += kw;
      for (uint32_t s = 0; s < kw + PB; s++) {
        const uint32_t at = LDPC_CW_SENT * w + s;
        CHECK(at < m);
        owner[at]++;
      }
    }
    CHECK(sum == k);
    for (uint32_t at = 0; at < m; at++) CHECK(owner[at] == 1);
  }
  uint32_t v = 0, nblocks = 0;
  CHECK(ldpc_coded_len_rate(rate, 0, &v) == OFDM_OK && v == PB + 4u);
  CHECK(ldpc_coded_len_rate(rate, KI - 4u, &v) == OFDM_OK && v == LDPC_CW_SENT);
  CHECK(ldpc_coded_len_rate(rate, KI - 3u, &v) == OFDM_OK && v == LDPC_CW_SENT + PB + 1u);
  CHECK(ldpc_coded_len_rate(rate, W_.max_payload, &v) == OFDM_OK && v == OFDM_LDPC_MAX_CODED);
  for (uint32_t m = 0; m <= 4200; m++) {
    uint32_t n = 77;
    CHECK(reached[m] <= 1);
    CHECK(ldpc_is_block_rate(rate, m) == (reached[m] == 1));
    CHECK((ldpc_payload_len_rate(rate, m, &n) == OFDM_OK) == (reached[m] == 1));
    CHECK(ldpc_is_block_rate(rate, m) == (m >= PB + 4u && m <= 4032u && (m - 1u) % 192u >= PB));
    if (!reached[m]) CHECK(n == 77);
    nblocks += (uint32_t)reached[m];
  }
  CHECK(nblocks == W_.max_payload + 1u);
  const uint32_t bad[] = {0, 1, PB + 3u, 192u + PB, 4033, 0x7FFFFFFFu, 0xFFFFFFFFu};
  for (uint32_t m : bad) CHECK(!ldpc_is_block_rate(rate, m) && ldpc_payload_len_rate(rate, m, &v) == OFDM_E_INVAL);
  CHECK(ldpc_is_block_rate(rate, 192u + PB + 1u) && ldpc_is_block_rate(rate, PB + 4u));
  CHECK(ldpc_coded_len_rate(rate, 0xFFFFFFFFu, &v) == OFDM_E_INVAL);
  CHECK(ldpc_coded_len_rate(rate, 0, nullptr) == OFDM_E_INVAL && ldpc_payload_len_rate(rate, 192, nullptr) == OFDM_E_INVAL);

  // ---- codeword maps: every length 0 .. 4200 as one decode batch ---------------------------------------------------------
  {
    const size_t nb = 4201;
    std::vector<uint32_t> len(nb);
    std::vector<uint64_t> in_off(nb), out_off(nb + 1, 77);
    uint64_t o = 0, reach = 0, want_cw = 0, want_total = 0;
    for (size_t b = 0; b < nb; b++) {
      len[b] = (uint32_t)b;
      in_off[b] = o;
      if (ldpc_is_block_rate(rate, len[b])) {
        reach = o + 8ull * len[b];
        want_cw += ldpc_block_words(len[b]);
        want_total += ldpc_block_info_rate(rate, len[b]) - 4u;
      }
      o += 8ull * len[b];
    }
    std::vector<LdpcBlk> blk(nb);
    std::vector<uint32_t> cw(nb * LDPC_MAX_WORDS, 0xFFFFFFFFu);
    uint64_t ncw = 0, ext = 0;
    const uint64_t total = ldpc_plan_decode_rate(rate, in_off.data(), len.data(), nb, 8, blk.data(), out_off.data(), cw.data(), &ncw, &ext);
    CHECK(total == want_total && out_off[nb] == total && ncw == want_cw && ext == reach);
    uint64_t at = 0, c = 0;
    for (size_t b = 0; b < nb; b++) {
      CHECK(out_off[b] == at && blk[b].out_off == at && blk[b].in_off == in_off[b] && blk[b].len == len[b] && blk[b].cw0 == c);
      if (!ldpc_is_block_rate(rate, len[b])) continue;
      for (uint32_t w = 0; w < ldpc_block_words(len[b]); w++) CHECK(cw[c + w] == b);
      c += ldpc_block_words(len[b]);
      at += ldpc_block_info_rate(rate, len[b]) - 4u;
    }
    for (uint64_t k = ncw; k < cw.size(); k++) CHECK(cw[k] == 0xFFFFFFFFu);  // nothing written behind the map
    const uint32_t none[] = {PB + 3u, 192u + PB};
    const uint64_t off2[] = {0, 5};
    CHECK(ldpc_plan_decode_rate(rate, off2, none, 2, 1, blk.data(), out_off.data(), cw.data(), &ncw, &ext) == 0 && ncw == 0 && ext == 0);
  }
  {
    const uint32_t plen[] = {0, KI - 4u, KI - 3u, W_.max_payload, 2u * KI - 4u};
    const uint64_t poff[] = {0, 0, 100, 4000, 9};
    std::vector<LdpcBlk> blk(5);
    std::vector<uint64_t> coff(6, 77);
    std::vector<uint32_t> cw(5 * LDPC_MAX_WORDS, 0xFFFFFFFFu);
    uint64_t ncw = 0, ext = 0;
    const uint64_t total = ldpc_plan_encode_rate(rate, poff, plen, 5, blk.data(), coff.data(), cw.data(), &ncw, &ext);
    CHECK(total == (PB + 4u) + 192u + (193u + PB) + 4032u + 384u && coff[5] == total && ext == 4000u + W_.max_payload && ncw == 1 + 1 + 2 + 21 + 2);
    const uint32_t cw0[] = {0, 1, 2, 4, 25};
    for (int b = 0; b < 5; b++) CHECK(blk[b].in_off == poff[b] && blk[b].out_off == coff[b] && blk[b].len == plen[b] && blk[b].cw0 == cw0[b]);
    CHECK(cw[0] == 0 && cw[1] == 1 && cw[2] == 2 && cw[3] == 2 && cw[4] == 3 && cw[24] == 3 && cw[25] == 4 && cw[26] == 4 && cw[27] == 0xFFFFFFFFu);
    const uint32_t over[] = {3, W_.max_payload + 1u};
    CHECK(ldpc_plan_encode_rate(rate, poff, over, 2, blk.data(), coff.data(), cw.data(), &ncw, &ext) == ~0ull);
  }
}

int main() {
  check_rate(OFDM_LDPC_RATE_1_2, LDPC_TABLE_R<OFDM_LDPC_RATE_1_2>, Want{12, 83, 58, 7, {7, 7, 7, 7, 7, 7, 6, 7, 7, 7, 7, 7}, 2012});
  check_rate(OFDM_LDPC_RATE_2_3, LDPC_TABLE_R<OFDM_LDPC_RATE_2_3>, Want{8, 71, 54, 9, {8, 9, 9, 9, 9, 9, 9, 9}, 2684});
  check_rate(OFDM_LDPC_RATE_3_4, LDPC_TABLE_R<OFDM_LDPC_RATE_3_4>, Want{6, 73, 60, 13, {12, 12, 12, 12, 13, 12}, 3020});
  check_rate(OFDM_LDPC_RATE_5_6, LDPC_TABLE_R<OFDM_LDPC_RATE_5_6>, Want{4, 73, 64, 19, {18, 18, 19, 18}, 3356});
  // the names without a rate are the rate-1/2 case, entry for entry and length for length
  for (int i = 0; i < LDPC_ROWS; i++)
    for (int j = 0; j < LDPC_COLS; j++) CHECK(LDPC_TABLE.shift[i][j] == LDPC_TABLE_R<OFDM_LDPC_RATE_1_2>.shift[i][j]);
  for (uint32_t x = 0; x <= 4200; x++) {
    uint32_t a = 77, b = 77;
    CHECK(ldpc_coded_len(x, &a) == ldpc_coded_len_rate(OFDM_LDPC_RATE_1_2, x, &b) && a == b);
    a = b = 77;
    CHECK(ldpc_payload_len(x, &a) == ldpc_payload_len_rate(OFDM_LDPC_RATE_1_2, x, &b) && a == b);
    CHECK(ldpc_is_block(x) == ldpc_is_block_rate(OFDM_LDPC_RATE_1_2, x));
  }
  // a rate that is none
  uint32_t v = 77;
  CHECK(ldpc_coded_len_rate(4, 10, &v) == OFDM_E_INVAL && ldpc_payload_len_rate(4, 192, &v) == OFDM_E_INVAL && v == 77);
  CHECK(ldpc_coded_len_rate(0xFFFFFFFFu, 10, &v) == OFDM_E_INVAL && v == 77);
  printf("ldpc_rate_plan_check ok\n");
  return 0;
}
