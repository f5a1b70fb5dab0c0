// ddc.h -- wideband front end: frequency-translating decimating FIR (gr.freq_xlating_fir_filter_ccf) ahead of ofdm_rx.
//
// Definition (include/ofdm_hip.h):
//   v[m] = sum_k c[k] x[mR - k]           c[k] = complex64(h[k] exp(j 2 pi fc k)), float32 accumulation
//   y[m] = v[m] r[m]                      r[m] = complex64(expj(-2 pi Phi_m / 2^64)), Phi_m = m D mod 2^64
// x[n] is indexed from the last reset, zero before it.  The order of the additions inside v[m] is a function of k
// alone: tap k = qR + p belongs to chain q mod NG (NG fixed by R), a chain adds its taps in ascending k into two
// packed accumulators A += c.re * (x.re, x.im), B += c.im * (x.re, x.im), the chains are added in ascending order and
// v = (A.re - B.im, A.im + B.re).  Nothing depends on where a call, a chunk or a tile starts.
//
// One workgroup produces T consecutive outputs.  Its T R + ntaps - 1 inputs (rounded up to whole decimation periods)
// are staged into LDS de-interleaved into R polyphase rows: sample (M0 + c) R - p sits in row p, column c + Q
// (Q = (ntaps - 1) / R), so that for every tap the lanes that own consecutive outputs read consecutive 8-byte words --
// no bank conflict at any R.  The row pitch W is odd: the staging stores of consecutive samples (consecutive rows)
// spread over the banks as well.
#pragma once
#include "common.h"
#include "host_util.h"
#include "stream_tile.h"  // ddc_f2, ddc_f4, ddc_put, nco_rotate

constexpr int DDC_THREADS = 256;
constexpr int DDC_MAX_DECIM = 64;

struct DdcParams {
  const void* x;    // this call's samples in the handle's receive format; x[0] is stream sample a
  const c32* hist;  // the ntaps - 1 converted samples before x[0] (zeros before the stream start)
  const c32* tab;   // c[k]
  c32* out;         // out[0] is output m0
  uint64_t nin, a, m0, nout;
  uint64_t D;       // phase advance per output, 2^-64 turn
  uint64_t magic;   // floor(2^32 / R) + 1: u / R = (u * magic) >> 32 for every u of a tile
  int R, ntaps, Q, W;
  float scale;
};

// geometry per decimation: TJ lanes along the outputs, OPT outputs per thread (T = TJ * OPT), NG = 256 / TJ tap chains
struct DdcGeom {
  int opt, tj;
  int T() const { return opt * tj; }
  int NG() const { return DDC_THREADS / tj; }
};
static inline DdcGeom ddc_geom(int R) {
  if (R <= 4) return DdcGeom{4, 256};   // T = 1024, one chain
  if (R <= 16) return DdcGeom{4, 64};   // T = 256, four chains
  return DdcGeom{1, 64};                // T = 64, four chains
}
static inline int ddc_pitch(int T, int Q) { return (T + Q) | 1; }
static inline size_t ddc_lds_bytes(int R, int ntaps) {
  const DdcGeom g = ddc_geom(R);
  const int Q = (ntaps - 1) / R;
  const size_t samples = (size_t)R * ddc_pitch(g.T(), Q) * sizeof(c32);
  const size_t combine = g.NG() > 1 ? (size_t)g.NG() * g.T() * 4 * sizeof(float) : 0;
  return (size_t)((ntaps + 1) & ~1) * sizeof(c32) + (samples > combine ? samples : combine);
}

__device__ __forceinline__ void ddc_finish(const DdcParams& q, uint64_t m, ddc_f2 A, ddc_f2 B) {
  const uint64_t o = m - q.m0;
  if (o >= q.nout) return;
  q.out[o] = nco_rotate(mk(A.x - B.y, A.y + B.x), 0ull - m * q.D);
}

template <typename XT, int OPT, int TJ>
__global__ void __launch_bounds__(DDC_THREADS) k_ddc(DdcParams q) {
  constexpr int NT = DDC_THREADS, NG = NT / TJ, T = TJ * OPT;
  extern __shared__ __align__(16) unsigned char ddc_lds[];
  c32* tap = reinterpret_cast<c32*>(ddc_lds);
  c32* xs = tap + ((q.ntaps + 1) & ~1);
  const int tid = threadIdx.x;
  const int R = q.R, W = q.W, Q = q.Q, H = q.ntaps - 1;
  const XT* x = static_cast<const XT*>(q.x);
  const uint64_t M0 = q.m0 + (uint64_t)blockIdx.x * T;
  // the tile's first staged sample, relative to x[0]: (M0 - Q) R - (R - 1) - a
  const int64_t g0 = (int64_t)(M0 * (uint64_t)R - q.a) - (int64_t)Q * R - (R - 1);
  const int total = (T + Q) * R;

  for (int k = tid; k < q.ntaps; k += NT) tap[k] = q.tab[k];
  if (g0 >= 1 && g0 + total + 1 <= (int64_t)q.nin) {
    // interior tile: every sample comes from x, no per-sample test against the stream
    if constexpr (std::is_same<XT, c32>::value) {
      // 16 bytes per lane, on the 16-byte grid of the caller's buffer (the pair may begin one sample before the tile)
      const int e = (int)((((uintptr_t)x >> 3) + (uint64_t)g0) & 1u);
      for (int u = 2 * tid - e; u < total; u += 2 * NT) {
        const ddc_f4 v = *reinterpret_cast<const ddc_f4*>(x + (g0 + u));
        if (u >= 0) ddc_put(xs, q.magic, q.R, q.W, u, mk(v.x, v.y));
        if (u + 1 < total) ddc_put(xs, q.magic, q.R, q.W, u + 1, mk(v.z, v.w));
      }
    } else {
      for (int u = tid; u < total; u += NT) ddc_put(xs, q.magic, q.R, q.W, u, iq_load(x, g0 + u, q.scale));
    }
  } else {
    // first and last tiles: the carried history (zeros at the stream start) before x[0], zeros behind the call's end
    // (those feed only outputs the call does not have) and before the oldest tap
    for (int u = tid; u < total; u += NT) {
      const int64_t gi = g0 + u;
      c32 v = mk(0.f, 0.f);
      if (gi >= 0) {
        if (gi < (int64_t)q.nin) v = iq_load(x, gi, q.scale);
      } else if (gi + H >= 0) {
        v = q.hist[gi + H];
      }
      ddc_put(xs, q.magic, q.R, q.W, u, v);
    }
  }
  __syncthreads();

  const int tj = tid % TJ;
  const int g = __builtin_amdgcn_readfirstlane(tid / TJ);  // a wave lies in one chain: tap reads are broadcasts
  ddc_f2 A[OPT], B[OPT];
#pragma unroll
  for (int i = 0; i < OPT; i++) A[i] = B[i] = ddc_f2{0.f, 0.f};
  for (int qq = g; qq <= Q; qq += NG) {
    const int k0 = qq * R;
    const int np = min(R, q.ntaps - k0);
    const c32* col = xs + (tj + Q - qq);
    const c32* tp = tap + k0;
    for (int p = 0; p < np; p++) {
      const c32 c = tp[p];
      const ddc_f2 cr = {c.re, c.re}, ci = {c.im, c.im};
#pragma unroll
      for (int i = 0; i < OPT; i++) {
        const ddc_f2 s = *reinterpret_cast<const ddc_f2*>(col + p * W + i * TJ);
        A[i] = __builtin_elementwise_fma(cr, s, A[i]);
        B[i] = __builtin_elementwise_fma(ci, s, B[i]);
      }
    }
  }

  if constexpr (NG == 1) {
#pragma unroll
    for (int i = 0; i < OPT; i++) ddc_finish(q, M0 + (uint64_t)(tj + i * TJ), A[i], B[i]);
  } else {
    // the chains of an output, added in ascending chain order
    ddc_f4* cmb = reinterpret_cast<ddc_f4*>(xs);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < OPT; i++) cmb[g * T + tj + i * TJ] = ddc_f4{A[i].x, A[i].y, B[i].x, B[i].y};
    __syncthreads();
    for (int j = tid; j < T; j += NT) {
      ddc_f4 s = cmb[j];
#pragma unroll
      for (int c = 1; c < NG; c++) s = s + cmb[c * T + j];
      ddc_finish(q, M0 + (uint64_t)j, ddc_f2{s.x, s.y}, ddc_f2{s.z, s.w});
    }
  }
}

// (the history kernel is k_stream_hist, stream_hist.h, with H = ntaps - 1)

// host side (engine_ddc.inc): StreamStage (host_util.h) and the DDC's own
struct DdcState : StreamStage {
  int R = 1, ntaps = 1;
  double fc = 0.0;
  uint64_t D = 0;          // frac(fc R) in 2^-64 turn
  std::vector<c32> tab;    // the table the kernel multiplies with
  DevBuf d_tab;
  void release() {
    d_tab.release();
    StreamStage::release();
  }
};
