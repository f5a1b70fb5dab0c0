// stream_stats.h -- the statistics of the stream stages that keep some (cfr.h, mempoly.h): counts, two maxima and float64
// sums since the stage was set or reset.  A thread adds its own terms in ascending order (StatAcc), a wave reduces by an
// xor butterfly, thread 0 adds the four waves' results in ascending order and writes the tile's partial (StatPartial);
// k_stat_reduce adds the partials of a call in a fixed order, in one or two levels, onto the running totals
// (StatTotals).  No float atomics: a call's sums depend on nothing but its samples and its length.
// A stage that has no term for a field (mempoly.h: sum_err, n_touched) leaves it at its 0.
#pragma once
#include "common.h"
#include "host_util.h"

constexpr int STAT_THREADS = 256;       // of a stage's compute kernel and of k_stat_reduce
constexpr int STAT_REDUCE_SPAN = 4096;  // partials one workgroup of k_stat_reduce adds

struct StatPartial {  // of one tile, or of STAT_REDUCE_SPAN tiles
  double sum_in, sum_out, sum_err;
  float peak_in, peak_out;
  uint32_t n_over, n_touched;
};
struct StatTotals {  // since the stage was set or reset
  double sum_in, sum_out, sum_err;
  float peak_in, peak_out;
  uint64_t n_over, n_touched;
};

// the float64 / float32 / uint32 reductions of one wave: every lane ends with the same value, in a fixed order
__device__ __forceinline__ double stat_wave_sum(double v) {
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) v += __shfl_xor(v, s, 64);
  return v;
}
__device__ __forceinline__ float stat_wave_max(float v) {
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) v = fmaxf(v, __shfl_xor(v, s, 64));
  return v;
}
__device__ __forceinline__ uint32_t stat_wave_count(uint32_t v) {
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) v += __shfl_xor(v, s, 64);
  return v;
}

struct StatAcc {  // a thread's statistics
  double sum_in = 0.0, sum_out = 0.0, sum_err = 0.0;
  float peak_in = 0.f, peak_out = 0.f;
  uint32_t n_over = 0, n_touched = 0;
};

// the workgroup's accumulators into one partial (thread 0 holds it on return); sh: one StatPartial per wave
template <int NW>
__device__ __forceinline__ StatPartial stat_block_reduce(const StatAcc& a, StatPartial* sh, int tid) {
  StatPartial p;
  p.sum_in = stat_wave_sum(a.sum_in);
  p.sum_out = stat_wave_sum(a.sum_out);
  p.sum_err = stat_wave_sum(a.sum_err);
  p.peak_in = stat_wave_max(a.peak_in);
  p.peak_out = stat_wave_max(a.peak_out);
  p.n_over = stat_wave_count(a.n_over);
  p.n_touched = stat_wave_count(a.n_touched);
  if ((tid & 63) == 0) sh[tid >> 6] = p;
  __syncthreads();
  if (tid == 0) {
    for (int i = 1; i < NW; i++) {
      p.sum_in += sh[i].sum_in;
      p.sum_out += sh[i].sum_out;
      p.sum_err += sh[i].sum_err;
      p.peak_in = fmaxf(p.peak_in, sh[i].peak_in);
      p.peak_out = fmaxf(p.peak_out, sh[i].peak_out);
      p.n_over += sh[i].n_over;
      p.n_touched += sh[i].n_touched;
    }
  }
  return p;
}

// The partials of a call into the totals, in a fixed order.  LAST = false: workgroup g adds in[g * SPAN .. ) (SPAN of
// them, fewer in the last) into out[g].  LAST = true: one workgroup adds all n (at most SPAN) onto *tot.
template <bool LAST>
__global__ void __launch_bounds__(STAT_THREADS) k_stat_reduce(const StatPartial* __restrict__ in, uint32_t n, StatPartial* __restrict__ out,
                                                              StatTotals* __restrict__ tot) {
  __shared__ StatPartial wpart[STAT_THREADS / 64];
  const int tid = threadIdx.x;
  const uint32_t lo = blockIdx.x * (uint32_t)STAT_REDUCE_SPAN;
  const uint32_t hi = min(n, lo + (uint32_t)STAT_REDUCE_SPAN);
  StatAcc a;
  for (uint32_t i = lo + tid; i < hi; i += STAT_THREADS) {
    const StatPartial p = in[i];
    a.sum_in += p.sum_in;
    a.sum_out += p.sum_out;
    a.sum_err += p.sum_err;
    a.peak_in = fmaxf(a.peak_in, p.peak_in);
    a.peak_out = fmaxf(a.peak_out, p.peak_out);
    a.n_over += p.n_over;
    a.n_touched += p.n_touched;
  }
  const StatPartial p = stat_block_reduce<STAT_THREADS / 64>(a, wpart, tid);
  if (tid != 0) return;
  if constexpr (LAST) {
    tot->sum_in += p.sum_in;
    tot->sum_out += p.sum_out;
    tot->sum_err += p.sum_err;
    tot->peak_in = fmaxf(tot->peak_in, p.peak_in);
    tot->peak_out = fmaxf(tot->peak_out, p.peak_out);
    tot->n_over += p.n_over;
    tot->n_touched += p.n_touched;
  } else {
    out[blockIdx.x] = p;
  }
}

// host side (engine_stage.inc: stage_stats_*): the samples counted, the partials of a call (one per tile; one per
// STAT_REDUCE_SPAN tiles where a call has more) and the totals
struct StatState {
  uint64_t n = 0;  // samples since the stage was set or reset
  DevBuf d_part, d_part2, d_tot;
  void release() {
    d_part.release();
    d_part2.release();
    d_tot.release();
  }
};
