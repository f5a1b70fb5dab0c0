// stream_hist.h -- the history kernel of the five wideband stream stages (ddc.h, ddc_bank.h, duc.h, resamp.h,
// tx_resamp.h): each keeps the last H input samples of its stream for the next call's oldest taps.
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
