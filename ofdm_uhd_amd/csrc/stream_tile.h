// stream_tile.h -- what the tiles of the ten wideband stage kernels share on the device (ddc.h, ddc_bank.h, pfb.h,
// resamp.h, resamp_bank.h, duc.h, duc_bank.h, pfb_synth.h, tx_resamp.h, tx_resamp_bank.h): the two polyphase layouts a tile is staged in and the
// rotation by an NCO phase.  Small inlined functions only.  (The staging block and the transmit store stay in every
// kernel's own text: DESIGN.md, "The wideband stages share one host-side skeleton ...", says what a shared
// template of either did to the compiler's output and the measured times.)
#pragma once
#include "common.h"
#include "rx_demod.h"  // nco_radians, dexpj

typedef float ddc_f2 __attribute__((ext_vector_type(2)));
typedef float ddc_f4 __attribute__((ext_vector_type(4)));

// The two polyphase layouts a tile is staged in: sample u = cc N + rho (u / N = (u * magic) >> 32 for every u of a
// tile) goes to column cc of row rho (the resamplers: sample (J0 - QM + c) M + rho in row rho, column c) or of row
// N - 1 - rho (the decimators: sample (M0 + c) R - p in row p).  The row pitch W is odd.
__device__ __forceinline__ void polyphase_put(c32* xs, uint64_t magicM, int M, int W, int u, c32 v) {
  const int cc = (int)(((uint64_t)(uint32_t)u * magicM) >> 32);
  xs[(u - cc * M) * W + cc] = v;
}
__device__ __forceinline__ void ddc_put(c32* xs, uint64_t magic, int R, int W, int u, c32 v) {
  const int cc = (int)(((uint64_t)(uint32_t)u * magic) >> 32);
  const int p = R - 1 - (u - cc * R);
  xs[p * W + cc] = v;
}

// v times complex64(expj(2 pi phase / 2^64)): the float64 phasor rounded once, the gr_complex product (unfused)
__device__ __forceinline__ c32 nco_rotate(c32 v, uint64_t phase) {
  const dc r = dexpj(nco_radians(phase));
  return cmul(v, mk((float)r.re, (float)r.im));
}
