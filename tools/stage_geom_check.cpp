// stage_geom_check.cpp -- the host geometry of the ten wideband stream stages (ofdm_uhd_amd/csrc/{ddc,ddc_bank,resamp,
// resamp_bank,pfb,pfb_synth,duc,duc_bank,tx_resamp,tx_resamp_bank}.h) as a program of its own, over the WHOLE space the
// stages accept: every L, M, R in [1, 64], every channel count, every ntaps in [1, 1024], every K in [1, 8].  For every
// configuration: the dynamic LDS the launch passes fits what the launch may have, the row pitches are odd where the
// headers say so, a region that overlays another fits into it, the magic division of the staging and store loops is exact
// for every index of a tile, and the index arithmetic of the call and of its first and last tile does not wrap at the
// index limits.  Needs no GPU and calls no HIP function; the headers hold kernels, so hipcc builds it (the kernels are
// templates that nothing here instantiates),
//   hipcc --offload-arch=gfx950 -x hip -std=c++17 -O1 -I include -o stage_geom_check tools/stage_geom_check.cpp
// and for a sanitizer run of the host code add
//   -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all
// tests/test_stage_geom_host.py builds and runs it without the sanitizers and compares `--table` (one line per stage and
// shape with the tile's outputs and inputs, one per stage, P and run of ntaps with the history) with the restatements
// of tests/*_cases.py.
//
// What the headers do not hold is restated here, each with the line it restates: the index limits and the magic
// constants are set in the engine_<stage>.inc files, which need the whole library around them.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../ofdm_uhd_amd/csrc/ddc_bank.h"
#include "../ofdm_uhd_amd/csrc/duc_bank.h"
#include "../ofdm_uhd_amd/csrc/pfb_synth.h"
#include "../ofdm_uhd_amd/csrc/resamp_bank.h"
#include "../ofdm_uhd_amd/csrc/tx_resamp_bank.h"

#define CHECK(c, ...)                                                    \
  do {                                                                   \
    if (!(c)) {                                                          \
      fprintf(stderr, "%s:%d: %s failed: ", __FILE__, __LINE__, #c);     \
      fprintf(stderr, __VA_ARGS__);                                      \
      fprintf(stderr, "\n");                                             \
      exit(1);                                                           \
    }                                                                    \
  } while (0)

typedef __int128 wide;

static const size_t LDS_DEFAULT = 64 * 1024;   // a launch without hipFuncSetAttribute (ddc, duc, duc_bank, pfb_synth)
static const size_t LDS_DEVICE = 160 * 1024;   // stage_launch (engine_stage.inc) raises the limit: a gfx950 workgroup's LDS
static const int MAX_TAPS = 1024;              // OFDM_DDC_MAX_TAPS and its siblings
static const uint64_t GRID_MAX = 0x7FFFFFFFull;  // stage_check_grid (engine_stage.inc)

// engine_ddc.inc: DDC_MAX_INDEX (the DDC, its bank and the channeliser); engine_resamp.inc / engine_tx_resamp.inc:
// RESAMP_MAX_INDEX, TX_RESAMP_MAX_INDEX; engine_duc.inc: DUC_MAX_OUTPUT (the DUC, its bank and the synthesis bank)
static const uint64_t DDC_MAX_INDEX = 1ull << 62, RESAMP_MAX_INDEX = 1ull << 56, DUC_MAX_OUTPUT = 1ull << 63;

static bool table = false;
static size_t lds_max[10];
static const char* const NAMES[10] = {"ddc",       "ddc_bank", "resamp",   "resamp_bank", "pfb",
                                      "pfb_synth", "duc",      "duc_bank", "tx_resamp",   "tx_resamp_bank"};
enum { DDC, DDC_BANK, RESAMP, RESAMP_BANK, PFB, PFB_SYNTH, DUC, DUC_BANK, TX_RESAMP, TX_RESAMP_BANK };

static void lds(int stage, size_t bytes, size_t limit, int a, int b, int ntaps, int K) {
  CHECK(bytes <= limit, "%s (%d, %d) ntaps=%d K=%d: %zu bytes of LDS", NAMES[stage], a, b, ntaps, K, bytes);
  if (bytes > lds_max[stage]) lds_max[stage] = bytes;
}

// p.magic = (1ull << 32) / P + 1 (engine_<stage>.inc); u / P = (u * magic) >> 32 as stream_tile.h and the kernels form it
static void magic_exact(int P, int count, const char* what) {
  const uint64_t magic = (1ull << 32) / (uint64_t)P + 1;
  for (int u = 0; u < count; u++)
    CHECK((int)(((uint64_t)(uint32_t)u * magic) >> 32) == u / P, "%s: P=%d u=%d", what, P, u);
}

// first_output (engine_stage.inc): ceil(a L / M), formed without adding to a L
static uint64_t first_output(uint64_t a, uint64_t L, uint64_t M) {
  const uint64_t p = a * L;
  return p / M + (p % M ? 1 : 0);
}
static wide ceil_div(wide a, wide b) { return (a + b - 1) / b; }
static bool fits_u64(wide v) { return v >= 0 && v <= (wide)UINT64_MAX; }
static bool fits_i64(wide v) { return v >= (wide)INT64_MIN && v <= (wide)INT64_MAX; }

// the starts a call is tried from, and the longest call each allows: a + nin <= sum_max, nin <= nin_max
static int starts(uint64_t first_max, uint64_t sum_max, uint64_t nin_max, uint64_t tile, uint64_t a[4], uint64_t nin[4]) {
  const uint64_t s[4] = {first_max, first_max - 3 * tile - 1, first_max / 2 + 1, 0};
  for (int i = 0; i < 4; i++) {
    a[i] = s[i];
    nin[i] = sum_max - s[i] < nin_max ? sum_max - s[i] : nin_max;
  }
  return 4;
}

// ofdm_ddc / ofdm_ddc_bank / ofdm_pfb and k_ddc / k_ddc_bank / k_pfb: decimation R (M), T outputs per tile
static void ddc_indices(int R, int T, int ntaps, const char* who) {
  const int Q = (ntaps - 1) / R;
  uint64_t as[4], nins[4];
  const int ns = starts(DDC_MAX_INDEX, 2 * DDC_MAX_INDEX, DDC_MAX_INDEX, (uint64_t)T * R, as, nins);
  for (int i = 0; i < ns; i++) {
    const uint64_t a = as[i], nin = nins[i];
    CHECK(fits_u64((wide)a + nin), "%s", who);                                    // a + nin
    const uint64_t m0 = first_output(a, 1, (uint64_t)R), no = first_output(a + nin, 1, (uint64_t)R) - m0;
    CHECK((wide)m0 == ceil_div(a, R) && (wide)(m0 + no) == ceil_div((wide)a + nin, R), "%s", who);
    uint64_t grid = (no + (uint64_t)T - 1) / (uint64_t)T;
    if (grid > GRID_MAX) grid = GRID_MAX;                                         // (a longer call is refused)
    const uint64_t blocks[2] = {0, grid ? grid - 1 : 0};
    for (uint64_t b : blocks) {
      const uint64_t M0 = m0 + b * (uint64_t)T;                                   // k_ddc: M0, g0, total
      CHECK(fits_u64((wide)M0 * R) && fits_i64((wide)M0 * R - a), "%s R=%d a=%llu", who, R, (unsigned long long)a);
      const int64_t g0 = (int64_t)(M0 * (uint64_t)R - a) - (int64_t)Q * R - (R - 1);
      const int total = (T + Q) * R;
      CHECK((wide)g0 == ((wide)M0 - Q) * R - (R - 1) - a && fits_i64((wide)g0 + total + 1), "%s", who);
      const int64_t last = g0 + total + 1;                                        // the interior test's right side
      (void)last;
      CHECK(fits_u64((wide)M0 + T), "%s", who);                                   // m = M0 + j
    }
  }
}

// ofdm_resamp / _bank / ofdm_tx_resamp / _bank and their kernels: TJ periods of L outputs and M inputs per tile
static void resamp_indices(int L, int M, int TJ, int ntaps, uint64_t max_index, const char* who) {
  const int QM = resamp_hist_periods((ntaps - 1) / L, M);
  uint64_t as[4], nins[4];
  const int ns = starts(max_index, max_index, max_index, (uint64_t)TJ * M, as, nins);
  for (int i = 0; i < ns; i++) {
    const uint64_t a = as[i], nin = nins[i];
    CHECK(fits_u64((wide)(a + nin) * L), "%s", who);                              // first_output: p = a L
    const uint64_t n0 = first_output(a, (uint64_t)L, (uint64_t)M), no = first_output(a + nin, (uint64_t)L, (uint64_t)M) - n0;
    CHECK((wide)n0 == ceil_div((wide)a * L, M) && (wide)(n0 + no) == ceil_div((wide)(a + nin) * L, M), "%s", who);
    const uint64_t J0 = n0 / (uint64_t)L;
    CHECK(fits_u64((wide)n0 + no + L - 1), "%s", who);
    const uint64_t periods = (n0 + no + (uint64_t)L - 1) / (uint64_t)L - J0;
    uint64_t grid = (periods + (uint64_t)TJ - 1) / (uint64_t)TJ;
    if (grid > GRID_MAX) grid = GRID_MAX;
    const uint64_t blocks[2] = {0, grid ? grid - 1 : 0};
    for (uint64_t b : blocks) {
      const uint64_t Jb = J0 + b * (uint64_t)TJ;                                  // k_resamp: J0, g0, total, n
      CHECK(fits_i64((wide)Jb) && fits_i64(((wide)Jb - QM) * M) && fits_i64(((wide)Jb - QM) * M - a), "%s", who);
      const int64_t g0 = ((int64_t)Jb - QM) * M - (int64_t)a;
      const int total = (TJ + QM) * M;
      CHECK(fits_i64((wide)g0 + total + 1), "%s", who);
      CHECK(fits_u64(((wide)Jb + TJ) * L), "%s", who);                            // n = J0 L + j, j < TJ L
    }
  }
}

// ofdm_duc / ofdm_duc_bank / ofdm_pfb_synth and their kernels: interpolation L (M), T outputs per tile
static void duc_indices(int L, int T, int ntaps, const char* who) {
  const int Q = (ntaps - 1) / L;
  const uint64_t lim = DUC_MAX_OUTPUT / (uint64_t)L;
  uint64_t as[4], nins[4];
  const int ns = starts(lim, lim, lim, (uint64_t)T, as, nins);
  for (int i = 0; i < ns; i++) {
    const uint64_t a = as[i], nin = nins[i];
    CHECK(nin <= lim && a <= lim - nin, "%s", who);                               // the call's own test, as it forms it
    CHECK(fits_u64(((wide)a + nin) * L), "%s", who);                              // no = nin L, n = a L + o
    const uint64_t no = nin * (uint64_t)L;
    uint64_t grid = (no + (uint64_t)T - 1) / (uint64_t)T;
    if (grid > GRID_MAX) grid = GRID_MAX;
    const uint64_t blocks[2] = {0, grid ? grid - 1 : 0};
    for (uint64_t b : blocks) {
      const uint64_t off = b * (uint64_t)T, dq = off / (uint64_t)L;               // k_duc: off, dq, r0, g0, total
      const int r0 = (int)(off - dq * (uint64_t)L);
      const int64_t g0 = (int64_t)dq - Q;
      const int total = Q + (r0 + T + L - 1) / L;
      CHECK(fits_i64((wide)g0 + total) && fits_u64((wide)a * L + off + T), "%s", who);
      CHECK(total <= duc_staged(T, L, Q), "%s L=%d ntaps=%d: %d staged samples", who, L, ntaps, total);
    }
  }
}

static void check_ddc_family() {
  for (int R = 1; R <= DDC_MAX_DECIM; R++) {
    const DdcGeom g = ddc_geom(R);
    CHECK(g.T() * g.NG() == DDC_THREADS * g.opt && DDC_THREADS % g.tj == 0, "R=%d", R);
    if (table) printf("tile ddc %d out=%d in=%d\ntile ddc_bank %d out=%d in=%d\n", R, g.T(), g.T() * R, R, g.T(), g.T() * R);
    magic_exact(R, (g.T() + (MAX_TAPS - 1) / R) * R, "ddc");
    for (int ntaps = 1; ntaps <= MAX_TAPS; ntaps++) {
      const int Q = (ntaps - 1) / R, W = ddc_pitch(g.T(), Q);
      CHECK((W & 1) && W >= g.T() + Q, "ddc R=%d ntaps=%d", R, ntaps);
      CHECK((g.T() + Q) * R <= (g.T() + (MAX_TAPS - 1) / R) * R, "ddc");          // (the magic division above covers it)
      const size_t tab = (size_t)((ntaps + 1) & ~1) * sizeof(c32), bytes = ddc_lds_bytes(R, ntaps);
      const size_t combine = g.NG() > 1 ? (size_t)g.NG() * g.T() * sizeof(ddc_f4) : 0;
      CHECK(bytes - tab >= (size_t)R * W * sizeof(c32) && bytes - tab >= combine, "ddc R=%d ntaps=%d", R, ntaps);
      lds(DDC, bytes, LDS_DEFAULT, R, 0, ntaps, 1);
      if (table) printf("hist ddc %d %d %d %d\nhist ddc_bank %d %d %d %d\n", R, ntaps, ntaps, ntaps - 1, R, ntaps, ntaps, ntaps - 1);
      ddc_indices(R, g.T(), ntaps, "ddc");
      for (int K = 1; K <= DDC_BANK_MAX_LINKS; K++) {
        const int KP = (K + 1) & ~1;
        const size_t words = ddc_bank_sample_words(R, ntaps);
        CHECK(words % 2 == 0 && words >= (size_t)R * W && ((size_t)ntaps * KP) % 2 == 0, "ddc_bank R=%d", R);
        CHECK(ddc_bank_lds_bytes(R, ntaps, K) == (words + (size_t)ntaps * KP) * sizeof(c32) + combine, "ddc_bank R=%d", R);
        CHECK(ddc_bank_group(R) == (g.opt == 4 ? 4 : 8), "ddc_bank R=%d", R);
        lds(DDC_BANK, ddc_bank_lds_bytes(R, ntaps, K), LDS_DEVICE, R, 0, ntaps, K);
      }
    }
  }
}

static void check_pfb_family() {
  for (int M = 2; M <= PFB_MAX_CHANNELS; M *= 2) {
    const int T = pfb_tile_outputs(M);
    CHECK(T * M == PFB_TILE && T == pfb_synth_tile_inputs(M), "M=%d", M);
    if (table) printf("tile pfb %d out=%d in=%d\ntile pfb_synth %d out=%d in=%d\n", M, T, T * M, M, PFB_TILE, T);
    magic_exact(M, (T + (MAX_TAPS - 1) / M) * M, "pfb");
    for (int ntaps = 1; ntaps <= MAX_TAPS; ntaps++) {
      const int Q = (ntaps - 1) / M, W = ddc_pitch(T, Q);
      // the branch sums take the rows' first T columns (k_pfb): they fit the pitch
      CHECK((W & 1) && W >= T + Q && pfb_sample_words(M, ntaps) >= (size_t)M * W, "pfb M=%d ntaps=%d", M, ntaps);
      lds(PFB, pfb_lds_bytes(M, ntaps), LDS_DEFAULT, M, 0, ntaps, 1);    // (engine_pfb.inc: no shape takes stage_launch past 64 KB)
      ddc_indices(M, T, ntaps, "pfb");
      const int P = pfb_synth_pitch(M, Q);
      CHECK(P >= T + Q && P < T + Q + 32, "pfb_synth M=%d ntaps=%d", M, ntaps);
      if (M >= 32) CHECK(P & 1, "pfb_synth M=%d ntaps=%d", M, ntaps);
      else CHECK((P & 31) == ((32 / M) & 31), "pfb_synth M=%d ntaps=%d", M, ntaps);
      CHECK(pfb_synth_lds_bytes(M, ntaps) == ((size_t)M * P + M) * sizeof(c32) + (size_t)ntaps * sizeof(float), "pfb_synth");
      lds(PFB_SYNTH, pfb_synth_lds_bytes(M, ntaps), LDS_DEFAULT, M, 0, ntaps, 1);
      if (table) printf("hist pfb %d %d %d %d\nhist pfb_synth %d %d %d %d\n", M, ntaps, ntaps, ntaps - 1, M, ntaps, ntaps, Q);
      // k_pfb_synth: M0 = block T input indices, g0 = M0 - Q, O0 = block PFB_TILE outputs: the DUC's arithmetic at L = M
      // with a tile of PFB_TILE outputs (r0 = 0: PFB_TILE is a multiple of M)
      duc_indices(M, PFB_TILE, ntaps, "pfb_synth");
    }
  }
}

static void check_duc_family() {
  for (int L = 1; L <= DUC_MAX_INTERP; L++) {
    const DucGeom g = duc_geom(L);
    if (table) printf("tile duc %d out=%d in=%d\ntile duc_bank %d out=%d in=%d\n", L, g.T(), g.T() / L, L, g.T(), g.T() / L);
    magic_exact(L, L - 1 + g.T(), "duc");                                         // u = r0 + tid + i NT, r0 < L
    for (int ntaps = 1; ntaps <= MAX_TAPS; ntaps++) {
      const int Q = (ntaps - 1) / L;
      lds(DUC, duc_lds_bytes(L, ntaps), LDS_DEFAULT, L, 0, ntaps, 1);
      lds(DUC_BANK, duc_bank_lds_bytes(L, ntaps), LDS_DEFAULT, L, 0, ntaps, DUC_BANK_MAX_LINKS);   // (whatever K)
      if (table) printf("hist duc %d %d %d %d\nhist duc_bank %d %d %d %d\n", L, ntaps, ntaps, Q, L, ntaps, ntaps, Q);
      duc_indices(L, g.T(), ntaps, "duc");
    }
  }
}

static void check_resamp_family() {
  for (int L = 1; L <= RESAMP_MAX_RATIO; L++)
    for (int M = 1; M <= RESAMP_MAX_RATIO; M++) {
      const ResampGeom g = resamp_geom(L, M);
      const TxResampGeom t = tx_resamp_geom(L, M);
      CHECK(t.kc >= g.kc && (t.kc == g.kc || t.TJ() * M <= TX_RESAMP_WIDE_INPUTS), "(%d, %d)", L, M);
      if (table) {
        printf("tile resamp %d %d out=%d in=%d\ntile resamp_bank %d %d out=%d in=%d\n", L, M, g.TJ() * L, g.TJ() * M, L, M,
               g.TJ() * L, g.TJ() * M);
        printf("tile tx_resamp %d %d out=%d in=%d\ntile tx_resamp_bank %d %d out=%d in=%d\n", L, M, t.TJ() * L, t.TJ() * M, L, M,
               t.TJ() * L, t.TJ() * M);
      }
      const int QMmax = resamp_hist_periods((MAX_TAPS - 1) / L, M);
      magic_exact(M, ((t.TJ() > g.TJ() ? t.TJ() : g.TJ()) + QMmax) * M, "resamp magicM");
      magic_exact(L, (t.TJ() > g.TJ() ? t.TJ() : g.TJ()) * L, "resamp magicL");
      for (int ntaps = 1; ntaps <= MAX_TAPS; ntaps++) {
        const int Q = (ntaps - 1) / L, QM = resamp_hist_periods(Q, M);
        CHECK(QM <= QMmax && QM * M >= Q && (QM - 1) * M < Q + (Q == 0), "(%d, %d) ntaps=%d", L, M, ntaps);
        for (int TJ : {g.TJ(), t.TJ()}) {
          const int W = resamp_pitch(TJ, QM);
          CHECK((W & 1) && W >= TJ + QM && ((TJ | 1) & 1), "(%d, %d) ntaps=%d", L, M, ntaps);
        }
        lds(RESAMP, resamp_lds_bytes(L, M, ntaps), LDS_DEVICE, L, M, ntaps, 1);
        lds(TX_RESAMP, tx_resamp_lds_bytes(L, M, ntaps), LDS_DEVICE, L, M, ntaps, 1);
        // (ofdm_set_tx_resamp_bank refuses a shape beyond TX_RESAMP_BANK_MAX_LDS: none is)
        lds(TX_RESAMP_BANK, tx_resamp_bank_lds_bytes(L, M, ntaps), TX_RESAMP_BANK_MAX_LDS, L, M, ntaps, TX_RESAMP_BANK_MAX_LINKS);
        for (int K = 1; K <= RESAMP_BANK_MAX_LINKS; K++) {
          const int NB = resamp_bank_sum_links(L, M, ntaps, K);
          CHECK(NB >= 1 && NB <= K && (NB & (NB - 1)) == 0, "(%d, %d) ntaps=%d K=%d", L, M, ntaps, K);
          lds(RESAMP_BANK, resamp_bank_lds_bytes(L, M, ntaps, K, NB), RESAMP_BANK_LDS_MAX, L, M, ntaps, K);
        }
        if (M == 1 && table)
          printf("hist resamp %d %d %d %d\nhist resamp_bank %d %d %d %d\nhist tx_resamp %d %d %d %d\nhist tx_resamp_bank %d %d %d %d\n",
                 L, ntaps, ntaps, Q, L, ntaps, ntaps, Q, L, ntaps, ntaps, Q, L, ntaps, ntaps, Q);
        if (ntaps == 1 || ntaps == MAX_TAPS || (ntaps - 1) % L == 0) {            // (the arithmetic depends on ntaps through QM)
          resamp_indices(L, M, g.TJ(), ntaps, RESAMP_MAX_INDEX, "resamp");
          resamp_indices(L, M, t.TJ(), ntaps, RESAMP_MAX_INDEX, "tx_resamp");      // TX_RESAMP_MAX_INDEX is the same
        }
      }
    }
}

int main(int argc, char** argv) {
  table = argc > 1 && !strcmp(argv[1], "--table");
  static_assert(RESAMP_BANK_LDS_MAX == 160 * 1024 && TX_RESAMP_BANK_MAX_LDS == 160 * 1024, "LDS_DEVICE");
  CHECK(RESAMP_BANK_LDS_MAX == LDS_DEVICE, "LDS_DEVICE");
  check_ddc_family();
  check_pfb_family();
  check_duc_family();
  check_resamp_family();
  for (int s = 0; s < 10; s++) printf("lds %s %zu\n", NAMES[s], lds_max[s]);
  printf("stage_geom_check ok\n");
  return 0;
}
