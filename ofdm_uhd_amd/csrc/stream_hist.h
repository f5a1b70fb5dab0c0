// stream_hist.h -- the history kernels of the ten wideband stream stages: each keeps the last H input samples of its
// stream (ddc.h, ddc_bank.h, pfb.h, resamp.h, duc.h, tx_resamp.h), or of each of its streams (pfb_synth.h, duc_bank.h, tx_resamp_bank.h),
// for the next call's oldest taps.  (What the stages' compute kernels share is stream_tile.h.)
#pragma once
#include "common.h"

// the last H converted samples after this call, into the other history buffer: a call shorter than H keeps the tail
// of the old history, which is therefore never overwritten while it is read.  (XT = c32: `scale` is not used.)
template <typename XT>
__global__ void __launch_bounds__(256) k_stream_hist(const XT* __restrict__ x, uint64_t nin, const c32* __restrict__ old,
                                                     c32* __restrict__ nw, int H, float scale) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= H) return;
  const int64_t gi = (int64_t)nin - H + i;
  nw[i] = gi >= 0 ? iq_load(x, gi, scale) : old[(int64_t)i + (int64_t)nin];
}

// the same per row, for the stages that keep one stream per link (pfb_synth.h, duc_bank.h): row i = blockIdx.y of the
// call's input begins at x + i * stride, its H samples of history at old + i * H
__global__ void __launch_bounds__(256) k_stream_hist_rows(const c32* __restrict__ x, uint64_t stride, uint64_t nin,
                                                          const c32* __restrict__ old, c32* __restrict__ nw, int H) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= H) return;
  const int64_t i = blockIdx.y, gi = (int64_t)nin - H + k;
  nw[i * H + k] = gi >= 0 ? x[(uint64_t)i * stride + (uint64_t)gi] : old[i * H + k + (int64_t)nin];
}
