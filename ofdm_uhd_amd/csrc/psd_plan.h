// psd_plan.h -- the host arithmetic of the spectrum stage (psd.h / engine_psd.inc): which segments of the stream a call
// completes, where they begin relative to the call's first sample, how many samples stay pending, and how the call's
// segments are dealt to workgroups.  Plain C++ without a HIP include, so that a stand-alone program can check it
// (tools/psd_plan_check.cpp).
//
// F is the transform length, S the hop (1 <= S <= F).  Segment j covers stream samples [j S, j S + F).  After T samples
// psd_segments(T) segments are complete; the first incomplete one begins at psd_segments(T) * S <= T, so fewer than F
// samples are pending and the stage's history of the last F - 1 samples (zeros before the stream start) holds them all.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define PSD_HD __host__ __device__
#else
#define PSD_HD
#endif

#define PSD_MIN_FFT 64u
#define PSD_MAX_FFT 4096u
#define PSD_MAX_INDEX (1ull << 62)           // stream samples since the reset: every product below stays inside 64 bits
#define PSD_MAX_CALL_SEGMENTS 0x7FFFFFFFull  // segments one call may complete: a workgroup's share counts in 32 bits
#define PSD_PART_BINS (1u << 21)             // bins of all workgroups' partials together: 24 MB of sums and maxima

PSD_HD static inline bool psd_fft_ok(uint32_t F) { return F >= PSD_MIN_FFT && F <= PSD_MAX_FFT && (F & (F - 1u)) == 0; }
// the workgroup of k_sense: F / 8 threads per transform, at least 256 threads, so G transforms side by side
PSD_HD constexpr int psd_threads(int F) { return F / 8 < 256 ? 256 : F / 8; }
PSD_HD constexpr int psd_groups(int F) { return psd_threads(F) / (F / 8); }

// segments complete after T samples of the stream
PSD_HD static inline uint64_t psd_segments(uint64_t T, uint32_t F, uint32_t S) { return T < F ? 0 : (T - F) / S + 1; }
// samples from the first incomplete segment on
PSD_HD static inline uint64_t psd_pending(uint64_t T, uint32_t F, uint32_t S) { return T - psd_segments(T, F, S) * S; }

// most workgroups of a launch: enough to fill the chip several times over, few enough that k_psd_reduce's walk over
// their partials stays short
PSD_HD static inline uint32_t psd_max_grid(uint32_t F) {
  const uint32_t g = PSD_PART_BINS / F;
  return g < 1024u ? g : 1024u;
}

struct PsdPlan {
  uint64_t nseg;    // segments the call completes
  int64_t first;    // where the first of them begins, relative to the call's first sample: in (-F, 0]
  uint64_t pending; // samples pending after the call
  uint32_t grid;    // workgroups (0: nothing to launch)
  uint32_t per;     // segments per workgroup, a multiple of G: workgroup b owns [b * per, min((b + 1) * per, nseg))
};

// a call of nin samples with `next` samples of the stream before it; false: refused (index limit, or too long for a grid)
PSD_HD static inline bool psd_plan(uint64_t next, uint64_t nin, uint32_t F, uint32_t S, PsdPlan* p) {
  p->nseg = 0;
  p->first = 0;
  p->pending = 0;
  p->grid = p->per = 0;
  if (next > PSD_MAX_INDEX || nin > PSD_MAX_INDEX - next) return false;
  const uint64_t before = psd_segments(next, F, S), after = psd_segments(next + nin, F, S);
  p->nseg = after - before;
  p->first = -(int64_t)(next - before * S);
  p->pending = next + nin - after * S;
  if (p->nseg > PSD_MAX_CALL_SEGMENTS) return false;
  if (p->nseg == 0) return true;
  const uint64_t G = (uint64_t)psd_groups((int)F);
  const uint64_t rounds_all = (p->nseg + G - 1) / G;  // rounds of G segments in the call
  const uint64_t cap = psd_max_grid(F);
  const uint64_t want = rounds_all < cap ? rounds_all : cap;
  const uint64_t rounds = (rounds_all + want - 1) / want;  // per workgroup
  p->per = (uint32_t)(rounds * G);
  p->grid = (uint32_t)((p->nseg + p->per - 1) / p->per);
  return true;
}
