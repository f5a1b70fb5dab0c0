// psd.h -- the spectrum stage: an averaged-periodogram (Welch) estimator over any complex stream.  A stream stage that
// reads its input and changes nothing: per segment of F samples at hop S it forms the windowed power spectrum in
// float32 with k_sense's transform (same schedule, same bits), and keeps a float64 sum and a float32 maximum per bin
// since the last reset; the rows themselves go out where the caller asks for them.
//
// Definition (include/ofdm_hip.h), segment j over x[j S .. j S + F), w the window:
//   e[i]   = (x[jS + i].re * w[i], x[jS + i].im * w[i])
//   X      = fft_F(e)                       fft.h, the schedule of k_sense
//   P_j[k] = X[k].re * X[k].re + X[k].im * X[k].im
//   sum[k] = float64 sum over j of P_j[k];  peak[k] = max over j of P_j[k], from 0, a NaN not counted
//
// k_psd<F, XT>  k_sense's layout: F / 8 threads per transform, 8 points per thread in registers, G = psd_groups(F)
//               transforms side by side in a workgroup.  Workgroup b owns the call's segments [b per, (b + 1) per) and
//               walks them in rounds of G consecutive ones (group g takes segment b per + r G + g), the loads of round
//               r + 1 in flight while round r is transformed.  Consecutive segments overlap by F - S samples: the
//               groups of a round, and a workgroup's rounds, re-read them through the CU's L1 and the XCD's L2, never
//               from memory twice (what was measured of staging a run in LDS instead: DESIGN.md section 7).  A segment
//               that begins before the call's first sample reads those samples from the carried history.
//               Each thread keeps 8 float64 sums and 8 float32 maxima in registers over its rounds; lane t holds bins
//               t + m F / 8, so a wave's row store is contiguous.  The G groups are folded through LDS in ascending
//               group order into the workgroup's partial.
// k_psd_reduce  adds the workgroups' partials in ascending workgroup order onto the totals in the handle.
// No float atomics anywhere: the order of every float64 addition is fixed by the call's segment count (psd_plan.h).
#pragma once
#include "common.h"
#include "fft.h"
#include "host_util.h"
#include "psd_plan.h"
#include "sense.h"

struct PsdParams {
  const void* x;      // this call's samples (XT); x[0] is the stream's next sample
  const c32* hist;    // the F - 1 converted samples before x[0] (zeros before the stream start)
  const float* win;   // F window taps
  const c32* tw;      // F forward twiddles exp(-2 pi i k / F)
  float* rows;        // NULL, or [nseg][F]
  double* part_sum;   // [grid][F]
  float* part_peak;   // [grid][F]
  uint64_t nseg;      // segments of this call
  int64_t first;      // where segment 0 begins relative to x[0]: in (-F, 0]
  uint32_t hop;
  uint32_t per;       // segments per workgroup, a multiple of G
  float xscale;       // XT = sc16: sample = (float)int16 * xscale (common.h iq_load)
};

// the 8 samples of a thread: sample i = t + m TPT of the segment that begins at `off` relative to x[0]
template <int F, typename XT>
__device__ __forceinline__ void psd_load(c32 nx[8], const PsdParams& p, bool live, int64_t off, int t) {
  constexpr int TPT = F / 8;
  const XT* x = static_cast<const XT*>(p.x);
  if (!live) {
#pragma unroll
    for (int m = 0; m < 8; m++) nx[m] = mk(0.f, 0.f);
  } else if (off >= 0) {
#pragma unroll
    for (int m = 0; m < 8; m++) nx[m] = iq_load(x, off + t + m * TPT, p.xscale);
  } else {
    // (off > -F: the history index off + i + F - 1 is >= 0)
#pragma unroll
    for (int m = 0; m < 8; m++) {
      const int64_t i = off + t + m * TPT;
      nx[m] = i >= 0 ? iq_load(x, i, p.xscale) : p.hist[i + (F - 1)];
    }
  }
}

template <int F, typename XT = c32>
__global__ void __launch_bounds__(sense_threads(F), sense_lean(F) ? 2 : 1) k_psd(PsdParams p) {
  constexpr int TPT = F / 8;
  constexpr int G = sense_groups(F);
  constexpr int NT = sense_threads(F);
  constexpr bool LEAN = sense_lean(F);
  static_assert(G == psd_groups(F) && NT == psd_threads(F), "psd_plan.h restates k_sense's workgroup");
  extern __shared__ __align__(16) unsigned char smem_raw[];
  c32* lds = reinterpret_cast<c32*>(smem_raw);
  const int tid = threadIdx.x;
  const int g = tid / TPT, t = tid % TPT;

  float w[8], mx[8];
  double sm[8];
#pragma unroll
  for (int m = 0; m < 8; m++) {
    w[m] = p.win[t + m * TPT];
    mx[m] = 0.0f;
    sm[m] = 0.0;
  }
  c32* my = lds + (size_t)g * fft_lds_bufs(F) * fft_lds_points(F);
  FftTwRegs<LEAN ? 64 : F> twr;
  c32* twl = lds + (size_t)G * fft_lds_bufs(F) * fft_lds_points(F);  // (lean) the twiddle table
  if constexpr (LEAN) {
    for (int i = tid; i < fft_tw_used(F); i += NT) twl[lpad(i)] = p.tw[i];
    __syncthreads();
  } else {
    twr.load(p.tw, t);
  }

  // every group of every workgroup runs the same number of rounds (barriers inside fft_run): the segments behind the
  // call's last one are not live
  const uint32_t rounds = p.per / G;
  const uint64_t s0 = (uint64_t)blockIdx.x * p.per + (uint64_t)g;  // this group's segment in round 0
  c32 nx[8];
  psd_load<F, XT>(nx, p, s0 < p.nseg, p.first + (int64_t)(s0 * p.hop), t);
  for (uint32_t r = 0; r < rounds; r++) {
    const uint64_t s = s0 + (uint64_t)r * G;
    const bool live = s < p.nseg;
    c32 e[8];
#pragma unroll
    for (int m = 0; m < 8; m++) e[m] = mk(nx[m].re * w[m], nx[m].im * w[m]);
    {
      const uint64_t sn = s + G;
      const bool ln = (r + 1 < rounds) && sn < p.nseg;
      psd_load<F, XT>(nx, p, ln, p.first + (int64_t)(sn * p.hop), t);
    }
    if constexpr (LEAN) {
      int tt = t;  // opaque copy, renewed every round: keeps the passes' LDS addresses out of the registers (sense.h)
      asm volatile("" : "+v"(tt));
      fft_run_tw<F, false, FftBlockSync, SENSE_PK, FftTwLds>(e, tt, my, FftTwLds{twl}, FftBlockSync());
#pragma unroll
      for (int m = 0; m < 8; m++) w[m] = p.win[tt + m * TPT];
    } else if constexpr (TPT <= WAVE) {
      fft_run_tw<F, false, FftWaveSync, SENSE_PK, FftTwRegs<F>>(e, t, my, twr, FftWaveSync());
    } else {
      fft_run_tw<F, false, FftBlockSync, SENSE_PK, FftTwRegs<F>>(e, t, my, twr, FftBlockSync());
    }
    if (live) {
      float pw[8];
#pragma unroll
      for (int m = 0; m < 8; m++) {
        pw[m] = e[m].re * e[m].re + e[m].im * e[m].im;
        mx[m] = pw[m] > mx[m] ? pw[m] : mx[m];
        sm[m] += (double)pw[m];
      }
      if (p.rows) {
        float* row = p.rows + s * (uint64_t)F;
#pragma unroll
        for (int m = 0; m < 8; m++) row[t + m * TPT] = pw[m];
      }
    }
    if constexpr (TPT > WAVE) __syncthreads();  // LDS scratch is reused by the next round
  }

  double* ps = p.part_sum + (uint64_t)blockIdx.x * F;
  float* pp = p.part_peak + (uint64_t)blockIdx.x * F;
  if constexpr (G > 1) {
    // fold the G groups in ascending order: bin b of group g at fs[g * F + b] / fp[g * F + b], over the transform scratch
    double* fs = reinterpret_cast<double*>(smem_raw);
    float* fp = reinterpret_cast<float*>(smem_raw + sizeof(double) * (size_t)G * F);
    static_assert((sizeof(double) + sizeof(float)) * (size_t)G * F <= (size_t)G * fft_lds_bytes(F), "the fold fits the scratch");
    __syncthreads();
#pragma unroll
    for (int m = 0; m < 8; m++) {
      fs[g * F + t + m * TPT] = sm[m];
      fp[g * F + t + m * TPT] = mx[m];
    }
    __syncthreads();
    for (int b = tid; b < F; b += NT) {
      double v = fs[b];
      float u = fp[b];
      for (int q = 1; q < G; q++) {
        v += fs[q * F + b];
        u = fmaxf(u, fp[q * F + b]);
      }
      ps[b] = v;
      pp[b] = u;
    }
  } else {
#pragma unroll
    for (int m = 0; m < 8; m++) {
      ps[t + m * TPT] = sm[m];
      pp[t + m * TPT] = mx[m];
    }
  }
}

// one thread per bin: the partials of the call's workgroups, in ascending workgroup order, onto the totals
__global__ void __launch_bounds__(256) k_psd_reduce(const double* __restrict__ part_sum, const float* __restrict__ part_peak,
                                                    uint32_t nparts, uint32_t F, double* __restrict__ sum, float* __restrict__ peak) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= F) return;
  double v = sum[b];
  float u = peak[b];
  uint32_t i = 0;
  // 16 loads in flight per thread, added in order
  for (; i + 16 <= nparts; i += 16) {
    double a[16];
    float c[16];
#pragma unroll
    for (int k = 0; k < 16; k++) {
      a[k] = part_sum[(uint64_t)(i + k) * F + b];
      c[k] = part_peak[(uint64_t)(i + k) * F + b];
    }
#pragma unroll
    for (int k = 0; k < 16; k++) {
      v += a[k];
      u = fmaxf(u, c[k]);
    }
  }
  for (; i < nparts; i++) {
    v += part_sum[(uint64_t)i * F + b];
    u = fmaxf(u, part_peak[(uint64_t)i * F + b]);
  }
  sum[b] = v;
  peak[b] = u;
}

// host side (engine_psd.inc): StreamStage (host_util.h; hist = F - 1, `next` = samples since the reset) and the stage's own
struct PsdState : StreamStage {
  int F = 0, S = 0;
  int in_fmt = OFDM_IQ_FC32;
  float in_scale = 1.0f / 32768.0f;
  uint64_t nseg = 0;  // since ofdm_set_psd / ofdm_psd_reset
  DevBuf d_w, d_tw, d_sum, d_peak, d_psum, d_ppeak;
  void release() {
    d_w.release();
    d_tw.release();
    d_sum.release();
    d_peak.release();
    d_psum.release();
    d_ppeak.release();
    StreamStage::release();
  }
};
