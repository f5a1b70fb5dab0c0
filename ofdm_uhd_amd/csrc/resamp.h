// resamp.h -- wideband front end for captures whose rate is no integer multiple of the modem's: rational-rate (L / M)
// polyphase resampler fused with the DDC's frequency translation (blks2.rational_resampler_ccf behind a tuner).
//
// Definition (include/ofdm_hip.h), output n at position n M on the L-times grid:
//   i_n = floor(n M / L), p_n = n M mod L
//   v[n] = sum over q >= 0 with p_n + q L < ntaps of c[p_n + q L] x[i_n - q]        float32
//   y[n] = v[n] r[n]                      r[n] = complex64(expj(-2 pi Phi_n / 2^64)), Phi_n = n D mod 2^64
// c[k] = complex64(h[k] exp(j 2 pi fc k / L)).  x[i] is indexed from the last reset, zero before it.  Tap q of an
// output belongs to chain q mod NG, a chain adds its taps in ascending q into two packed accumulators
// A += c.re * (x.re, x.im), B += c.im * (x.re, x.im) begun at +0, the chains are added in ascending order and
// v = (A.re - B.im, A.im + B.re).  NG is a function of (L, M) alone (resamp_geom).  Nothing depends on where a call, a
// chunk or a tile starts.
//
// A period is L outputs and M inputs: output n = J L + r (r in [0, L)) has i_n = J M + floor(r M / L) and
// p_n = r M mod L.  One workgroup produces TJ consecutive periods, on the absolute period grid.  A wave works on one
// phase class r at a time, its lanes on consecutive periods: p is wave-uniform (tap reads are broadcasts) and the
// input index advances by M per lane.  So the tile's inputs, with QM = ceil(Q / M) periods of history in front
// (Q = (ntaps - 1) / L), are staged into M rows: sample (J0 - QM + c) M + rho sits in row rho, column c, and for every
// tap the lanes read consecutive 8-byte words -- no bank conflict at any (L, M).  The row pitch W is odd, which spreads
// the staging stores (consecutive samples, consecutive rows) over the banks.  The sums go through LDS ([r][period],
// odd pitch) and leave in output order: every global store of a wave is one contiguous run.
#pragma once
#include "common.h"
#include "ddc.h"  // ddc_f2, ddc_f4, stream_tile.h
#include "host_util.h"
#include "stream_hist.h"  // k_stream_hist

constexpr int RESAMP_THREADS = 256;
constexpr int RESAMP_MAX_RATIO = 64;  // largest L and largest M

struct ResampParams {
  const void* x;    // this call's samples in the handle's receive format; x[0] is stream sample a
  const c32* hist;  // the Q converted samples before x[0] (zeros before the stream start)
  const c32* tab;   // c[k]
  c32* out;         // out[0] is output n0
  uint64_t nin, a, n0, nout;
  uint64_t J0;      // period of the first tile: n0 / L
  uint64_t D;       // phase advance per output, 2^-64 turn
  uint64_t magicM;  // floor(2^32 / M) + 1: u / M = (u * magicM) >> 32 for every u of a tile
  uint64_t magicL;  // the same for L
  int L, M, ntaps, Q, QM, W, TP, KC;
  float scale;
};

// geometry per (L, M): a tile is TJ = 64 KC periods (TJ L outputs from TJ M inputs); NG tap chains where one chain per
// output would leave waves without work (few phase classes and few periods)
struct ResampGeom {
  int kc, ng;
  int TJ() const { return WAVE * kc; }
};
static inline ResampGeom resamp_geom(int L, int M) {
  const int m = L > M ? L : M;
  const int kc = m <= 1 ? 16 : m <= 2 ? 8 : m <= 4 ? 4 : m <= 8 ? 2 : 1;
  return ResampGeom{kc, L * kc < RESAMP_THREADS / WAVE ? 4 : 1};
}
static inline int resamp_hist_periods(int Q, int M) { return (Q + M - 1) / M; }
static inline int resamp_pitch(int TJ, int QM) { return (TJ + QM) | 1; }
// LDS in c32 words: the table, the M staged rows, and the sums on their way out (NG > 1: A and B of every chain)
static inline size_t resamp_lds_bytes(int L, int M, int ntaps) {
  const ResampGeom g = resamp_geom(L, M);
  const int QM = resamp_hist_periods((ntaps - 1) / L, M);
  const size_t tab = (size_t)((ntaps + 1) & ~1);
  const size_t rows = ((size_t)M * resamp_pitch(g.TJ(), QM) + 1) & ~(size_t)1;
  const size_t sums = g.ng > 1 ? (size_t)g.ng * g.TJ() * L * 2 : (size_t)L * (g.TJ() | 1);
  return (tab + rows + sums) * sizeof(c32);
}

template <typename XT, int NG>
__global__ void __launch_bounds__(RESAMP_THREADS) k_resamp(ResampParams q) {
  constexpr int NT = RESAMP_THREADS, NW = NT / WAVE;
  extern __shared__ __align__(16) unsigned char resamp_lds[];
  c32* tap = reinterpret_cast<c32*>(resamp_lds);
  c32* xs = tap + ((q.ntaps + 1) & ~1);
  c32* ob = xs + ((q.M * q.W + 1) & ~1);
  const int tid = threadIdx.x;
  const int L = q.L, M = q.M, W = q.W, Q = q.Q, QM = q.QM, TJ = q.KC * WAVE, TO = TJ * L;
  const XT* x = static_cast<const XT*>(q.x);
  const uint64_t J0 = q.J0 + (uint64_t)blockIdx.x * (uint64_t)TJ;
  // the tile's first staged sample, relative to x[0]: (J0 - QM) M - a
  const int64_t g0 = ((int64_t)J0 - QM) * M - (int64_t)q.a;
  const int total = (TJ + QM) * M;

  for (int k = tid; k < q.ntaps; k += NT) tap[k] = q.tab[k];
  if (g0 >= 1 && g0 + total + 1 <= (int64_t)q.nin) {
    // interior tile: every sample comes from x, no per-sample test against the stream
    if constexpr (std::is_same<XT, c32>::value) {
      // 16 bytes per lane, on the 16-byte grid of the caller's buffer (the pair may begin one sample before the tile)
      const int e = (int)((((uintptr_t)x >> 3) + (uint64_t)g0) & 1u);
      for (int u = 2 * tid - e; u < total; u += 2 * NT) {
        const ddc_f4 v = *reinterpret_cast<const ddc_f4*>(x + (g0 + u));
        if (u >= 0) polyphase_put(xs, q.magicM, q.M, q.W, u, mk(v.x, v.y));
        if (u + 1 < total) polyphase_put(xs, q.magicM, q.M, q.W, u + 1, mk(v.z, v.w));
      }
    } else {
      for (int u = tid; u < total; u += NT) polyphase_put(xs, q.magicM, q.M, q.W, u, iq_load(x, g0 + u, q.scale));
    }
  } else {
    // first and last tiles: the carried history (zeros at the stream start) before x[0], zeros behind the call's end
    // (those feed only outputs the call does not have) and before the oldest sample the history holds
    for (int u = tid; u < total; u += NT) {
      const int64_t gi = g0 + u;
      c32 v = mk(0.f, 0.f);
      if (gi >= 0) {
        if (gi < (int64_t)q.nin) v = iq_load(x, gi, q.scale);
      } else if (gi + Q >= 0) {
        v = q.hist[gi + Q];
      }
      polyphase_put(xs, q.magicM, q.M, q.W, u, v);
    }
  }
  __syncthreads();

  // work item = (phase class r, 64 periods, chain g); a wave takes every NW-th one: all its indices are wave-uniform
  const int lane = tid & (WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
  const int nwork = L * q.KC * NG;
  for (int wi = wave; wi < nwork; wi += NW) {
    const int g = wi % NG, unit = wi / NG;
    const int r = unit / q.KC;
    const int t = (unit - r * q.KC) * WAVE + lane;
    const int rm = r * M, off = rm / L, p = rm - off * L;
    const int nq = p < q.ntaps ? (q.ntaps - 1 - p) / L + 1 : 0;
    // sample i - qq of period t: row (off - qq) mod M, column t + QM + floor((off - qq) / M)
    int row = off - g, col = QM;
    while (row < 0) {
      row += M;
      col--;
    }
    ddc_f2 A = {0.f, 0.f}, B = {0.f, 0.f};
    for (int qq = g; qq < nq; qq += NG) {
      const c32 c = tap[p + qq * L];
      const ddc_f2 s = *reinterpret_cast<const ddc_f2*>(xs + (row * W + col + t));
      A = __builtin_elementwise_fma(ddc_f2{c.re, c.re}, s, A);
      B = __builtin_elementwise_fma(ddc_f2{c.im, c.im}, s, B);
      row -= NG;
      while (row < 0) {
        row += M;
        col--;
      }
    }
    if constexpr (NG == 1) ob[r * q.TP + t] = mk(A.x - B.y, A.y + B.x);
    else reinterpret_cast<ddc_f4*>(ob)[g * TO + t * L + r] = ddc_f4{A.x, A.y, B.x, B.y};
  }
  __syncthreads();

  // in output order: the chains of an output added in ascending chain order, the rotation, one contiguous store
  for (int j = tid; j < TO; j += NT) {
    const uint64_t n = J0 * (uint64_t)L + (uint64_t)j;
    const uint64_t o = n - q.n0;  // (outputs before n0 wrap to huge values)
    if (o >= q.nout) continue;
    c32 v;
    if constexpr (NG == 1) {
      const int t = (int)(((uint64_t)(uint32_t)j * q.magicL) >> 32);
      v = ob[(j - t * L) * q.TP + t];
    } else {
      const ddc_f4* cmb = reinterpret_cast<const ddc_f4*>(ob);
      ddc_f4 s = cmb[j];
#pragma unroll
      for (int c = 1; c < NG; c++) s = s + cmb[c * TO + j];
      v = mk(s.x - s.w, s.y + s.z);
    }
    q.out[o] = nco_rotate(v, 0ull - n * q.D);
  }
}

// (the history kernel is k_stream_hist, stream_hist.h, with H = Q: the last Q converted samples after a call)

// host side (engine_resamp.inc): StreamStage (host_util.h; hist = Q) and the resampler's own
struct ResampState : StreamStage {
  int L = 1, M = 1, ntaps = 1;
  double fc = 0.0;
  uint64_t D = 0;          // frac(fc M / L) in 2^-64 turn
  std::vector<c32> tab;    // the table the kernel multiplies with
  DevBuf d_tab;
  void release() {
    d_tab.release();
    StreamStage::release();
  }
};
