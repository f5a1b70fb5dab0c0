// core_geom_check.cpp -- the launch decisions and LDS layouts of the core modem's receive kernels (k_chan_filter, k_sync
// and its fused front end, k_sync_exact, k_rx_demod: ofdm_uhd_amd/csrc/{rx_sync,rx_demod}.h) as a program of its own, over
// the WHOLE space ofdm_create accepts: every fft_length in {64 .. 4096}, every cp_length in [1, N], every ntaps in
// [1, 512], and for the demodulator every even occupied_tones in [16, N] x arity x max_fft_shift_len in {1, 2, 4, 8, 64}
// x slicer grid x channel state.  For every geometry: the filter block B = F - ntaps + 1 is at least one sample and F one
// of the five transform lengths that are built; k_sync's LDS fits a compute unit whenever the cyclic prefix is one the
// receiver takes (CP <= a tile); the overlay and the fixed layout hold what the comments of sync_lds_layout promise;
// every LDS region is 16-byte aligned and regions that are not overlaid on purpose do not overlap; k_sync_exact's two
// launches fit what they may have; the demodulator fits, or is the configuration launch_demod refuses in words.
// Needs no GPU and calls no HIP function; the headers hold kernels, so hipcc builds it (templates nothing here
// instantiates),
//   hipcc --offload-arch=gfx950 -x hip -std=c++17 -O1 -I include -o core_geom_check tools/core_geom_check.cpp
// and for a sanitizer run of the host code add
//   -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all
// and run the program as it is, on the CPU.  tests/test_core_geom_host.py builds and runs it without the sanitizers and
// compares `--table` (one line per run of cp_length / ntaps / occupied_tones over which no decision changes) with the
// class functions of tests/core_sweep_cases.py.
//
// What the headers do not hold is restated here, each with the line it restates.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../ofdm_uhd_amd/csrc/rx_demod.h"
#include "../ofdm_uhd_amd/csrc/rx_sync.h"

#define CHECK(c, ...)                                                    \
  do {                                                                   \
    if (!(c)) {                                                          \
      fprintf(stderr, "%s:%d: %s failed: ", __FILE__, __LINE__, #c);     \
      fprintf(stderr, __VA_ARGS__);                                      \
      fprintf(stderr, "\n");                                             \
      exit(1);                                                           \
    }                                                                    \
  } while (0)

static const size_t LDS_DEFAULT = 64 * 1024;  // a launch without hipFuncSetAttribute
static const size_t LDS_CU = (size_t)CU_LDS_BYTES;
static const int MAX_TAPS = 512;              // OFDM_MAX_TAPS (include/ofdm_hip.h); ofdm_create refuses 0 and 513
static bool table = false;
static size_t lds_sync = 0, lds_front = 0, lds_exact = 0, lds_exact_small = 0, lds_filter = 0, lds_demod = 0;
static long demod_refused = 0, demod_total = 0;

static size_t up16(size_t b) { return (b + 15) & ~(size_t)15; }
static bool al16(size_t b) { return (b & 15) == 0; }

// ---- channel filter: launch_filter_t (engine_rx.inc) ----------------------------------------------------------------
static void check_filter() {
  int run_lo = 1, run_F = sync_filter_F(1);
  for (int ntaps = 1; ntaps <= MAX_TAPS + 1; ntaps++) {
    const int F = ntaps <= MAX_TAPS ? sync_filter_F(ntaps) : -1;
    if (F != run_F) {
      if (table) printf("filter %d %d F=%d Bmax=%d Bmin=%d\n", run_lo, ntaps - 1, run_F, run_F - run_lo + 1, run_F - (ntaps - 1) + 1);
      run_lo = ntaps;
      run_F = F;
    }
    if (ntaps > MAX_TAPS) break;
    CHECK(F == 64 || F == 128 || F == 256 || F == 512 || F == 1024, "ntaps=%d F=%d", ntaps, F);
    const int B = F - ntaps + 1;
    CHECK(B >= 1 && B <= F && ntaps - 1 < F, "ntaps=%d F=%d B=%d", ntaps, F, B);
    // 256 threads, F/8 per block: bpr blocks side by side, each with F + F/8 points of scratch (fsh = 256 * 9 c32)
    const int bpr = 256 / (F / 8);
    CHECK(bpr >= 1 && bpr * (F / 8) == 256, "F=%d", F);
    const size_t fsh = (size_t)256 * 9 * sizeof(c32);
    CHECK((size_t)bpr * fft_lds_points(F) * sizeof(c32) == fsh && fsh <= LDS_DEFAULT, "F=%d", F);
    if (fsh > lds_filter) lds_filter = fsh;
  }
}

// ---- k_sync, k_sync_exact: sync_params, launch_sync, rx_sync_exact (engine_rx.inc) ----------------------------------------
struct SyncClass {
  int wg, fixed, overlay, tps, small, keep, refused;
  bool operator!=(const SyncClass& o) const {
    return wg != o.wg || fixed != o.fixed || overlay != o.overlay || tps != o.tps || small != o.small || keep != o.keep || refused != o.refused;
  }
};

static void check_sync_layout(int N, int CP) {
  const int T = SYNC_TILE, HY = sync_hist_y(N), R = sync_ring_samples(HY);
  CHECK(HY == N && R == N + T && R % 8 == 0, "N=%d", N);  // (N is a multiple of 8)
  const SyncLds l = sync_lds_layout(R, CP);
  const size_t ys_end = up16((size_t)(sync_lp(R) + 2) * sizeof(c32));
  const size_t mt_bytes = (size_t)(sync_lp(T) + 2) * sizeof(float), mh_bytes = (size_t)(sync_lp(CP) + 2) * sizeof(float);
  CHECK(al16(l.ys) && al16(l.mt) && al16(l.mh) && al16(l.mh1) && al16(l.misc) && al16(l.total), "N=%d CP=%d", N, CP);
  if (sync_mt_overlay(R)) {
    // mt overlays the tile's own samples: it starts at the tile's first sample, ends inside the ring, and the part the
    // slide to the front still reads -- ys[T .. R) -- lies behind its end.  Only the fixed layout has the tile there.
    CHECK(R - T <= T, "N=%d: overlay needs the fixed layout", N);
    CHECK(l.mt == l.ys + (size_t)sync_lp(R - T) * sizeof(c32), "N=%d", N);
    CHECK(l.mt + mt_bytes <= l.ys + (size_t)sync_lp(T) * sizeof(c32), "N=%d: the slide reads what mt overwrote", N);
    CHECK(l.mt + mt_bytes <= ys_end && l.mh >= ys_end, "N=%d", N);
  } else {
    CHECK(l.mt >= ys_end && l.mh >= l.mt + mt_bytes, "N=%d CP=%d", N, CP);
  }
  CHECK(l.mh1 >= l.mh + mh_bytes && l.misc >= l.mh1 + mh_bytes && l.total == l.misc + 384, "N=%d CP=%d", N, CP);
  const SyncLaunch sl = sync_launch_choice(N, CP);
  CHECK(sl.lds == l.total && sl.fixed_layout == (R - T <= T), "N=%d CP=%d", N, CP);
  // the M history of a tile is the CP newest values of the one before: the receiver takes CP <= T (sync_params)
  if (CP <= T) {
    CHECK(sl.lds <= LDS_CU, "N=%d CP=%d: %zu bytes of LDS in k_sync", N, CP, sl.lds);
    CHECK(sl.wg >= 1 && sl.wg <= SYNC_MAX_WG && (size_t)sl.wg * sl.lds <= LDS_CU, "N=%d CP=%d wg=%d", N, CP, sl.wg);
    if (sl.lds > lds_sync) lds_sync = sl.lds;
  }
  const int tps = sync_tiles_per_seg(N, CP);
  CHECK(tps >= 32 && tps % 32 == 0 && (long)(tps / 32) * T >= N + CP && (long)(tps / 32 - 1) * T < N + CP, "N=%d CP=%d", N, CP);
  // k_sync_exact: the wave-sized launch passes its LDS without raising the limit; its ranges fit one allocation chunk
  // of 2048 candidates (CHUNK_C of the SMALL variant)
  const int es = sync_exact_small(CP, N / 2);
  CHECK(es >= 0 && es <= T && es <= 2048, "N=%d CP=%d", N, CP);
  CHECK((es > 0) == (N / 2 <= 256), "N=%d", N);
  for (int rmax : {T, es}) {
    const ExactLds e = exact_lds_layout(CP, rmax);
    CHECK(al16(e.me) && al16(e.ue) && al16(e.misc) && al16(e.total), "N=%d CP=%d", N, CP);
    CHECK(e.ue >= e.me + (size_t)(rmax + CP + 8) * sizeof(float) && e.misc >= e.ue + (size_t)(rmax + 8) * sizeof(float) &&
              e.total == e.misc + 512,
          "N=%d CP=%d", N, CP);
    CHECK(e.total == up16((size_t)(rmax + CP + 8) * 4) + up16((size_t)(rmax + 8) * 4) + 512, "N=%d CP=%d", N, CP);
    if (rmax == T) {
      CHECK(e.total <= LDS_CU, "N=%d CP=%d", N, CP);
      if (e.total > lds_exact) lds_exact = e.total;
    } else if (es > 0) {
      CHECK(e.total <= LDS_DEFAULT, "N=%d CP=%d: %zu bytes in the wave-sized k_sync_exact", N, CP, e.total);
      if (e.total > lds_exact_small) lds_exact_small = e.total;
    }
  }
  CHECK(sync_exact_keep(N) == (N == 4096), "N=%d", N);
}

static SyncClass sync_class(int N, int CP) {
  const SyncLaunch sl = sync_launch_choice(N, CP);
  SyncClass c;
  c.refused = CP > SYNC_TILE;
  c.wg = c.refused ? 0 : sl.wg;
  c.fixed = sl.fixed_layout;
  c.overlay = sync_mt_overlay(sync_ring_samples(sync_hist_y(N)));
  c.tps = sync_tiles_per_seg(N, CP);
  c.small = sync_exact_small(CP, N / 2) > 0;
  c.keep = sync_exact_keep(N);
  return c;
}

static void check_sync(int N) {
  int lo = 1;
  SyncClass run = sync_class(N, 1);
  for (int CP = 1; CP <= N + 1; CP++) {
    if (CP <= N) check_sync_layout(N, CP);
    const bool end = CP > N;
    SyncClass c = run;
    if (!end) c = sync_class(N, CP);
    if (end || c != run) {
      if (table)
        printf("sync %d %d %d wg=%d fixed=%d overlay=%d tps=%d small=%d keep=%d refused=%d\n", N, lo, CP - 1, run.wg, run.fixed,
               run.overlay, run.tps, run.small, run.keep, run.refused);
      lo = CP;
      run = c;
    }
  }
}

// ---- the fused front end: front_fused, launch_front (engine_rx.inc) -------------------------------------------------------
static void check_front_layout(int N, int CP, int ntaps) {
  const int T = SYNC_TILE, F = sync_filter_F(ntaps), B = F - ntaps + 1, R = sync_ring_samples(sync_hist_y(N));
  const FrontLds l = front_lds_layout(R, CP, B, F);
  CHECK(F <= 512 && CP <= T && sync_hist_y(N) + l.C <= T && l.C >= B && l.C % 8 == 0, "N=%d CP=%d ntaps=%d", N, CP, ntaps);
  CHECK(R - T <= T, "N=%d: the front end needs the fixed layout", N);
  CHECK(al16(l.ys) && al16(l.mt) && al16(l.mh0) && al16(l.mh1) && al16(l.tw) && al16(l.misc) && al16(l.total), "N=%d CP=%d ntaps=%d", N,
        CP, ntaps);
  const size_t mt_bytes = (size_t)(sync_lp(T) + 2) * sizeof(float), scb = (size_t)SYNC_THREADS * 9 * sizeof(c32);
  const size_t mh_bytes = (size_t)(sync_lp(CP) + 2) * sizeof(float);
  CHECK(l.mt >= l.ys + (size_t)(sync_lp(R + l.C) + 2) * sizeof(c32), "N=%d ntaps=%d", N, ntaps);
  CHECK(l.mh0 >= l.mt + mt_bytes && l.mh0 >= l.mt + scb, "N=%d ntaps=%d", N, ntaps);
  CHECK((size_t)(SYNC_THREADS / (F / 8)) * fft_lds_points(F) * sizeof(c32) == scb, "F=%d", F);
  CHECK(l.mh1 >= l.mh0 + mh_bytes && l.tw >= l.mh1 + mh_bytes, "N=%d CP=%d", N, CP);
  CHECK(l.misc >= l.tw + (size_t)fft_tw_lds_points(F) * sizeof(c32) && l.total == l.misc + 384, "N=%d ntaps=%d", N, ntaps);
  CHECK(3 * l.total <= LDS_CU, "N=%d CP=%d ntaps=%d", N, CP, ntaps);  // k_sync<3, true, F>
  if (l.total > lds_front) lds_front = l.total;
}

// the cyclic prefixes for which (N, ntaps) is eligible, as a list of runs in text form
static void front_runs(int N, int ntaps, char* out, size_t cap) {
  size_t n = 0;
  out[0] = 0;
  int lo = 0;
  for (int CP = 1; CP <= N + 1; CP++) {
    const bool e = CP <= N && front_eligible(N, CP, ntaps);
    if (e) check_front_layout(N, CP, ntaps);
    if (e && !lo) lo = CP;
    if (!e && lo) {
      n += (size_t)snprintf(out + n, cap - n, " %d-%d", lo, CP - 1);
      CHECK(n < cap, "front_runs");
      lo = 0;
    }
  }
  if (!out[0]) snprintf(out, cap, " none");
}

static void check_front(int N) {
  char run[256], cur[256];
  int lo = 1;
  front_runs(N, 1, run, sizeof(run));
  for (int ntaps = 2; ntaps <= MAX_TAPS + 1; ntaps++) {
    if (ntaps <= MAX_TAPS) front_runs(N, ntaps, cur, sizeof(cur));
    if (ntaps > MAX_TAPS || strcmp(cur, run) || sync_filter_F(ntaps) != sync_filter_F(lo)) {
      if (table) printf("front %d %d %d F=%d cp%s\n", N, lo, ntaps - 1, sync_filter_F(lo), run);
      lo = ntaps;
      strcpy(run, cur);
    }
  }
}

// ---- k_rx_demod: launch_demod (engine_rx.inc) -----------------------------------------------------------------------------
struct DemodClass {
  int twl, smap, refused;
  bool operator!=(const DemodClass& o) const { return twl != o.twl || smap != o.smap || refused != o.refused; }
};

static DemodClass demod_class(int N, int occ, int arity, int nbits, int shift, bool grid, bool csi, int nmap) {
  const DemodLaunch d = demod_launch_choice(N, occ, arity, nmap, nbits, shift, grid, csi);
  // the pieces are multiples of 16 bytes: the frames of a workgroup (N = 512) start aligned behind the shared tables
  const int shared = demod_lds_shared(N, d.twl, d.smap_lds, arity, nmap, grid), frame = demod_lds_frame(N, occ, nmap, nbits, shift, csi);
  CHECK(al16((size_t)shared) && al16((size_t)frame) && d.lds == (size_t)shared + (size_t)demod_fpw(N) * frame, "N=%d occ=%d", N, occ);
  CHECK(d.twl || fft_onebuf(N), "N=%d: up to N = 1024 the twiddles are always in LDS", N);
  CHECK(demod_hinv_len(N, occ, shift) >= occ && 2 * demod_hinv_len(N, occ, shift) >= occ + 2 * shift + 1, "N=%d occ=%d shift=%d", N, occ,
        shift);
  CHECK(demod_symbits_words(nmap, nbits) * 32 >= nmap * nbits + 8, "occ=%d", occ);
  // an extra is taken only where it costs no workgroup: with it the CU holds what it holds without
  const size_t base = (size_t)demod_lds_bytes(N, !fft_onebuf(N), false, occ, arity, nmap, nbits, shift, grid, csi);
  DemodClass c;
  c.twl = d.twl;
  c.smap = d.smap_lds;
  c.refused = d.lds > LDS_CU;  // "configuration needs more than 160 KiB of LDS in k_rx_demod"
  if (!c.refused) {
    CHECK(base <= LDS_CU && LDS_CU / d.lds >= 1, "N=%d occ=%d", N, occ);
    const int waves = demod_fpw(N) * ((N / 8 + WAVE - 1) / WAVE), cu = 4 * demod_waves_per_simd(N);
    const size_t by_waves = (size_t)(cu / waves > 1 ? cu / waves : 1);
    const size_t w_base = LDS_CU / base < by_waves ? LDS_CU / base : by_waves, w_now = LDS_CU / d.lds < by_waves ? LDS_CU / d.lds : by_waves;
    CHECK(w_now == w_base, "N=%d occ=%d arity=%d shift=%d: an LDS extra costs a workgroup", N, occ, arity, shift);
    if (d.lds > lds_demod) lds_demod = d.lds;
  } else {
    CHECK(base > LDS_CU && !d.smap_lds, "N=%d occ=%d: refused with an extra on", N, occ);  // no extra made it so
    demod_refused++;
  }
  demod_total++;
  return c;
}

static void check_demod(int N) {
  static const int ARITY[6] = {2, 4, 8, 16, 64, 256}, NBITS[6] = {1, 2, 3, 4, 6, 8}, SHIFT[5] = {1, 2, 4, 8, 64};
  for (int a = 0; a < 6; a++)
    for (int shift : SHIFT)
      for (int grid = 0; grid < 2; grid++)
        for (int csi = 0; csi < 2; csi++) {
          if (grid && ARITY[a] < 16) continue;  // (create_impl: a slicer grid needs sixteen points)
          int lo = 16;
          DemodClass run = {0, 0, 0};
          for (int occ = 16; occ <= N + 2; occ += 2) {
            DemodClass c = run;
            if (occ <= N) {
              // the built-in carrier map leaves two carriers of the occupied block empty; a custom one may fill it
              c = demod_class(N, occ, ARITY[a], NBITS[a], shift, grid, csi, occ - 2);
              demod_class(N, occ, ARITY[a], NBITS[a], shift, grid, csi, occ);
            }
            if (occ == 16) run = c;
            if (occ > N || c != run) {
              if (table)
                printf("demod %d arity=%d shift=%d grid=%d csi=%d %d %d twl=%d smap=%d refused=%d\n", N, ARITY[a], shift, grid, csi, lo,
                       occ - 2, run.twl, run.smap, run.refused);
              lo = occ;
              run = c;
            }
          }
        }
}

int main(int argc, char** argv) {
  table = argc > 1 && !strcmp(argv[1], "--table");
  static_assert(SYNC_TILE == 2048 && SYNC_THREADS == 256 && WAVE == 64, "the geometry this program was written for");
  check_filter();
  for (int N = 64; N <= 4096; N *= 2) {
    check_sync(N);
    check_front(N);
    check_demod(N);
  }
  printf("lds k_chan_filter %zu\nlds k_sync %zu\nlds k_front %zu\nlds k_sync_exact %zu\nlds k_sync_exact_wave %zu\nlds k_rx_demod %zu\n",
         lds_filter, lds_sync, lds_front, lds_exact, lds_exact_small, lds_demod);
  printf("refused k_rx_demod %ld of %ld\n", demod_refused, demod_total);
  printf("core_geom_check ok\n");
  return 0;
}
