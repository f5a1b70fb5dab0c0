// psd_plan_check.cpp -- the host arithmetic of the spectrum stage (ofdm_uhd_amd/csrc/psd_plan.h) as a program of its own:
// the segments a call completes, where they begin, what stays pending, the grid and every workgroup's share, and the
// index limits, swept over every (F, S) class and over call lengths around every boundary.  It walks the indices k_psd
// forms from a plan and checks each against the call's input and the carried history.  Needs no GPU and no HIP.  For
// a sanitizer run build it with
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include -o psd_plan_check tools/psd_plan_check.cpp
// tests/test_psd_host.py builds and runs it without the sanitizers.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../ofdm_uhd_amd/csrc/psd_plan.h"

#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #c); \
      exit(1);                                                    \
    }                                                             \
  } while (0)

// one call: the plan against the definition, and the indices the kernel reads and writes
static void check_call(uint64_t next, uint64_t nin, uint32_t F, uint32_t S) {
  PsdPlan p;
  CHECK(psd_plan(next, nin, F, S, &p));
  const uint64_t before = psd_segments(next, F, S), after = psd_segments(next + nin, F, S);
  CHECK(p.nseg == after - before);
  // the state: fewer than F samples pending, before and after, from the first incomplete segment on
  CHECK(psd_pending(next, F, S) < F && p.pending == psd_pending(next + nin, F, S) && p.pending < F);
  CHECK(p.first <= 0 && p.first > -(int64_t)F && (uint64_t)(-p.first) == psd_pending(next, F, S));
  CHECK(before * S + (uint64_t)(-p.first) == next);
  if (p.nseg == 0) {
    CHECK(p.grid == 0 && p.pending == psd_pending(next, F, S) + nin);
    return;
  }
  // every segment of the call ends inside the call's input and the last one brought in by its last samples
  const int64_t last = p.first + (int64_t)((p.nseg - 1) * S);
  CHECK(last + (int64_t)F <= (int64_t)nin);
  CHECK(last + (int64_t)F + (int64_t)S > (int64_t)nin);
  // the first segment's first sample lies in the history of F - 1 samples or in the call, and its last sample is one of
  // the call's (it was not complete before)
  CHECK(p.first + (int64_t)(F - 1) >= 0);
  // the grid: shares of whole rounds, every segment owned once, no empty workgroup, within the limits
  const uint32_t G = (uint32_t)psd_groups((int)F);
  CHECK(p.per >= G && p.per % G == 0 && p.grid >= 1 && p.grid <= psd_max_grid(F));
  CHECK((uint64_t)p.grid * p.per >= p.nseg && (uint64_t)(p.grid - 1) * p.per < p.nseg);
  CHECK((uint64_t)p.grid * F <= PSD_PART_BINS);
  CHECK((uint64_t)psd_threads((int)F) == (uint64_t)G * (F / 8) && psd_threads((int)F) >= 256 && psd_threads((int)F) <= 1024);
}

int main() {
  // segment counts by the definition
  CHECK(psd_segments(0, 64, 64) == 0 && psd_segments(63, 64, 1) == 0 && psd_segments(64, 64, 1) == 1 && psd_segments(65, 64, 1) == 2);
  CHECK(psd_segments(127, 64, 64) == 1 && psd_segments(128, 64, 64) == 2 && psd_segments(4096 + 19, 4096, 19) == 2);
  for (uint32_t F = PSD_MIN_FFT; F <= PSD_MAX_FFT; F *= 2) {
    CHECK(psd_fft_ok(F) && !psd_fft_ok(F + 1) && !psd_fft_ok(F - 1));
    const uint32_t G = (uint32_t)psd_groups((int)F);
    const uint32_t hops[] = {1, 2, 3, F / 4, F / 4 + 3, F / 2 - 1, F / 2, F / 2 + 1, F - 1, F};
    for (uint32_t S : hops) {
      // call lengths around every boundary: no segment, one, a round of G, a workgroup's share, the grid's cap
      std::vector<uint64_t> segs = {0, 1, 2, G - 1, G, G + 1, 2 * G, 2 * G + 1, 7 * G + 3};
      const uint64_t cap = psd_max_grid(F);
      for (uint64_t k : {cap * G - 1, cap * G, cap * G + 1, 2 * cap * G + 1, 3 * cap * G - 1}) segs.push_back(k);
      const uint64_t starts[] = {0, 1, S - 1, S, F - 1, F, F + 1, 5ull * F + 7, (1ull << 40) + 11};
      for (uint64_t next : starts)
        for (uint64_t k : segs) {
          // the shortest call that completes k segments from `next` on, one sample less and one more
          const uint64_t have = psd_segments(next, F, S);
          const uint64_t need = (have + k) == 0 ? 0 : (have + k - 1) * S + F;  // stream length with have + k segments
          const uint64_t nin = need > next ? need - next : 0;
          check_call(next, nin, F, S);
          if (nin) check_call(next, nin - 1, F, S);
          check_call(next, nin + 1, F, S);
          check_call(next, nin + S - 1, F, S);
        }
      // a stream in chunks: the plans add up to the stream in one call, whatever the cut
      uint64_t next = 0, total = 0, x = 12345;
      for (int i = 0; i < 200; i++) {
        x = x * 6364136223846793005ull + 1442695040888963407ull;
        const uint64_t sizes[] = {0, 1, S - 1, F + 1, F - 1, (x >> 33) % (3 * F)};
        const uint64_t nin = sizes[(x >> 20) % 6];
        PsdPlan p;
        CHECK(psd_plan(next, nin, F, S, &p));
        total += p.nseg;
        next += nin;
        CHECK(total == psd_segments(next, F, S) && p.pending == next - total * S);
      }
    }
  }
  CHECK(!psd_fft_ok(32) && !psd_fft_ok(8192) && !psd_fft_ok(0) && !psd_fft_ok(96));
  // index limits: the stream's length, and the segments of one call
  PsdPlan p;
  CHECK(psd_plan(PSD_MAX_INDEX - 5, 5, 64, 1, &p) && p.nseg == 5);
  CHECK(!psd_plan(PSD_MAX_INDEX - 5, 6, 64, 1, &p));
  CHECK(!psd_plan(PSD_MAX_INDEX + 1, 0, 64, 1, &p));
  CHECK(!psd_plan(0, ~0ull, 64, 1, &p));
  CHECK(psd_plan(100, PSD_MAX_CALL_SEGMENTS, 64, 1, &p) && p.nseg == PSD_MAX_CALL_SEGMENTS && (uint64_t)p.grid * p.per >= p.nseg);
  CHECK(!psd_plan(100, PSD_MAX_CALL_SEGMENTS + 1, 64, 1, &p) && p.nseg == PSD_MAX_CALL_SEGMENTS + 1);
  CHECK(psd_plan(0, 4096ull * PSD_MAX_CALL_SEGMENTS, 4096, 4096, &p) && p.nseg == PSD_MAX_CALL_SEGMENTS);
  CHECK(!psd_plan(0, 4096ull * (PSD_MAX_CALL_SEGMENTS + 1), 4096, 4096, &p));
  printf("psd_plan_check ok\n");
  return 0;
}
