// pfb.h -- wideband receive: critically sampled polyphase-FFT channeliser for links on the k/M grid.
//
// Definition (include/ofdm_hip.h): M channels at c/M cycles per input sample, decimation M, one
// real prototype h[0..ntaps):
//   u_p[m] = sum_{q >= 0, qM+p < ntaps} h[qM+p] x[(m-q)M - p]      p = 0..M-1: ONE chain of packed FMAs on (re, im),
//                                                                  ascending q, begun at +0
//   y_c[m] = sum_p u_p[m] w[(c p) mod M]                           w[j] = complex64(exp(+2 pi i j / M))
// x[n] is indexed from the last reset, zero before it.  The transform over p is the radix-2 decimation-in-time
// recursion  D_n(v)[c] = E[c] + t[c],  D_n(v)[c + n/2] = E[c] - t[c],  E = D_{n/2}(v even), O = D_{n/2}(v odd),
// t[c] = O[c] w[c M / n] (the unfused complex product; t[0] = O[0], index 0 is not multiplied), D_1(v) = v,
// y[m] = D_M(u[m]).  M <= 16 runs it in one thread per output index.  M = 32, 64 run it in two steps of the SAME
// recursion, M = M1 M2 with M1 = 8: first the M2 sub-transforms of size M1 (over p = r + M2 k), then the levels
// n = 2 M1 .. M, which only ever combine entries with equal c mod M1 -- the same operations on the same operands, so
// the bits are a function of (m, c) and (M, h) alone: never of the selected channels, their order or number, or of
// where a call, a chunk or a tile starts.  The whole transform is computed; only selected rows are stored.
//
// One workgroup produces T = 4096 / M consecutive output indices for all M channels.  The tile's (T + Q) M samples
// (Q = (ntaps - 1) / M) are staged once in k_ddc's polyphase layout (ddc_put: sample (M0 + c) M - p in row p, column
// c + Q, odd pitch W), the real taps and w behind them.  A thread forms 16 branch sums: lanes run along the output
// index (consecutive 8-byte LDS words), the branch p is the same in a whole wave (tap reads are broadcasts).  The
// sums go back into the sample rows (row p, column j), the transform reads a column of them, and every selected
// channel's outputs leave as one contiguous 512-byte run per wave.
#pragma once
#include "ddc.h"

#define PFB_MAX_CHANNELS 64  // = OFDM_PFB_MAX_CHANNELS

constexpr int PFB_THREADS = 256;
constexpr int PFB_TILE = 4096;  // T M: branch sums (and outputs over all channels) per workgroup

struct PfbParams {
  DdcParams b;        // k_ddc's staging parameters with R = M; b.out is the first selected channel's run; tab, D unused
  const float* taps;  // h[k]
  const c32* w;       // w[j], j in [0, M)
  uint64_t stride;    // selected channel i's run begins at b.out + i * stride
  // the positions in the selection that hold channel c: first[c], next[first[c]], ... until -1 (ascending)
  signed char first[PFB_MAX_CHANNELS], next[PFB_MAX_CHANNELS];
};

static inline int pfb_tile_outputs(int M) { return PFB_TILE / M; }
static inline size_t pfb_sample_words(int M, int ntaps) {
  const int Q = (ntaps - 1) / M;
  return ((size_t)M * ddc_pitch(pfb_tile_outputs(M), Q) + 1) & ~(size_t)1;
}
static inline size_t pfb_lds_bytes(int M, int ntaps) {
  return (pfb_sample_words(M, ntaps) + (size_t)M) * sizeof(c32) + (size_t)ntaps * sizeof(float);
}

// The levels of the recursion above over v[0], v[S], ..., v[(N - 1) S], in registers.  The twiddle of output c at
// this level is w[(c1 + m1 c) ws]: the first step has c1 = 0, m1 = 1, ws = M / N; the second works on the entries
// c = c1 (mod M1) with m1 = M1, ws = M2 / N.  FIRST: c1 is 0 at compile time.
template <int N, int S, bool FIRST>
__device__ __forceinline__ void pfb_dit(const c32* v, c32* out, const c32* w, int c1, int m1, int ws) {
  if constexpr (N == 1) {
    out[0] = v[0];
  } else {
    c32 e[N / 2], o[N / 2];
    pfb_dit<N / 2, 2 * S, FIRST>(v, e, w, c1, m1, 2 * ws);
    pfb_dit<N / 2, 2 * S, FIRST>(v + S, o, w, c1, m1, 2 * ws);
#pragma unroll
    for (int c = 0; c < N / 2; c++) {
      c32 t = o[c];
      if (c > 0) t = cmul(o[c], w[(c1 + m1 * c) * ws]);
      if (c == 0 && !FIRST) t = c1 == 0 ? o[0] : cmul(o[0], w[c1 * ws]);
      out[c] = mk(e[c].re + t.re, e[c].im + t.im);
      out[c + N / 2] = mk(e[c].re - t.re, e[c].im - t.im);
    }
  }
}

// channel c of output index M0 + j into every selected row that holds it (c is the same in a whole wave)
__device__ __forceinline__ void pfb_store(const PfbParams& q, int c, uint64_t o, c32 y) {
  if (o >= q.b.nout) return;
  for (int i = q.first[c]; i >= 0; i = q.next[i]) q.b.out[(uint64_t)i * q.stride + o] = y;
}

template <typename XT, int M>
__global__ void __launch_bounds__(PFB_THREADS, 4) k_pfb(PfbParams q) {
  constexpr int NT = PFB_THREADS, T = PFB_TILE / M, NB = PFB_TILE / NT, M1 = M <= 16 ? M : 8, M2 = M / M1;
  static_assert(T >= 64 && (T & (T - 1)) == 0, "a wave lies in one branch");
  extern __shared__ __align__(16) unsigned char pfb_lds[];
  const int tid = threadIdx.x;
  const int W = q.b.W, Q = q.b.Q, H = q.b.ntaps - 1;
  c32* xs = reinterpret_cast<c32*>(pfb_lds);
  c32* w = xs + (((size_t)M * W + 1) & ~(size_t)1);
  float* tap = reinterpret_cast<float*>(w + M);
  const XT* x = static_cast<const XT*>(q.b.x);
  const uint64_t O0 = (uint64_t)blockIdx.x * T;  // the tile's first output, relative to the call's
  const uint64_t M0 = q.b.m0 + O0;
  // the tile's first staged sample, relative to x[0]: (M0 - Q) M - (M - 1) - a
  const int64_t g0 = (int64_t)(M0 * (uint64_t)M - q.b.a) - (int64_t)Q * M - (M - 1);
  const int total = (T + Q) * M;

  for (int k = tid; k < q.b.ntaps; k += NT) tap[k] = q.taps[k];
  if (tid < M) w[tid] = q.w[tid];
  if (g0 >= 1 && g0 + total + 1 <= (int64_t)q.b.nin) {
    // interior tile: every sample comes from x, no per-sample test against the stream
    if constexpr (std::is_same<XT, c32>::value) {
      // 16 bytes per lane, on the 16-byte grid of the caller's buffer (the pair may begin one sample before the tile)
      const int e = (int)((((uintptr_t)x >> 3) + (uint64_t)g0) & 1u);
      for (int u = 2 * tid - e; u < total; u += 2 * NT) {
        const ddc_f4 v = *reinterpret_cast<const ddc_f4*>(x + (g0 + u));
        if (u >= 0) ddc_put(xs, q.b.magic, q.b.R, W, u, mk(v.x, v.y));
        if (u + 1 < total) ddc_put(xs, q.b.magic, q.b.R, W, u + 1, mk(v.z, v.w));
      }
    } else {
      for (int u = tid; u < total; u += NT) ddc_put(xs, q.b.magic, q.b.R, W, u, iq_load(x, g0 + u, q.b.scale));
    }
  } else {
    // first and last tiles: the carried history (zeros at the stream start) before x[0], zeros behind the call's end
    // (those feed only outputs the call does not have) and before the oldest tap
    for (int u = tid; u < total; u += NT) {
      const int64_t gi = g0 + u;
      c32 v = mk(0.f, 0.f);
      if (gi >= 0) {
        if (gi < (int64_t)q.b.nin) v = iq_load(x, gi, q.b.scale);
      } else if (gi + H >= 0) {
        v = q.b.hist[gi + H];
      }
      ddc_put(xs, q.b.magic, q.b.R, W, u, v);
    }
  }
  __syncthreads();

  // branch sums: sum i of this thread is branch p_i = (NT i) / T + p0 at column j_i = jb + (NT i) mod T
  const int p0 = T < NT ? __builtin_amdgcn_readfirstlane(tid / T) : 0;
  const int jb = tid & (T - 1);
  ddc_f2 acc[NB];
#pragma unroll
  for (int i = 0; i < NB; i++) acc[i] = ddc_f2{0.f, 0.f};
  for (int qq = 0; qq < Q; qq++) {
    const c32* col = xs + (jb + Q - qq);
    const float* tp = tap + qq * M + p0;
#pragma unroll
    for (int i = 0; i < NB; i++) {
      const int pc = (NT * i) / T, jc = (NT * i) & (T - 1);
      const float hk = tp[pc];
      const ddc_f2 s = *reinterpret_cast<const ddc_f2*>(col + (pc + p0) * W + jc);
      acc[i] = __builtin_elementwise_fma(ddc_f2{hk, hk}, s, acc[i]);
    }
  }
  {
    // the last row of taps: the branches with Q M + p < ntaps
    const c32* col = xs + jb;
    const float* tp = tap + Q * M + p0;
#pragma unroll
    for (int i = 0; i < NB; i++) {
      const int pc = (NT * i) / T, jc = (NT * i) & (T - 1);
      if (Q * M + pc + p0 < q.b.ntaps) {
        const float hk = tp[pc];
        const ddc_f2 s = *reinterpret_cast<const ddc_f2*>(col + (pc + p0) * W + jc);
        acc[i] = __builtin_elementwise_fma(ddc_f2{hk, hk}, s, acc[i]);
      }
    }
  }
  __syncthreads();  // every sample has been read: the sums take the rows' first T columns
#pragma unroll
  for (int i = 0; i < NB; i++) {
    const int pc = (NT * i) / T, jc = (NT * i) & (T - 1);
    xs[(pc + p0) * W + jb + jc] = mk(acc[i].x, acc[i].y);
  }
  __syncthreads();

  // the transform over p; M2 > 1: its first step in place (a thread owns rows r, r + M2, ... of its column)
#pragma unroll
  for (int it = 0; it < NB / M1; it++) {
    const int idx = tid + NT * it, j = idx & (T - 1), r = idx / T;
    c32 v[M1], y[M1];
#pragma unroll
    for (int k = 0; k < M1; k++) v[k] = xs[(r + M2 * k) * W + j];
    pfb_dit<M1, 1, true>(v, y, w, 0, 1, M2);
#pragma unroll
    for (int c = 0; c < M1; c++) {
      if constexpr (M2 == 1)
        pfb_store(q, c, O0 + (uint64_t)j, y[c]);
      else
        xs[(r + M2 * c) * W + j] = y[c];
    }
  }
  if constexpr (M2 > 1) {
    __syncthreads();
#pragma unroll
    for (int it = 0; it < NB / M2; it++) {
      const int idx = tid + NT * it, j = idx & (T - 1);
      const int c1 = __builtin_amdgcn_readfirstlane(idx / T);
      c32 v[M2], y[M2];
#pragma unroll
      for (int r = 0; r < M2; r++) v[r] = xs[(M2 * c1 + r) * W + j];
      pfb_dit<M2, 1, false>(v, y, w, c1, M1, 1);
#pragma unroll
      for (int c2 = 0; c2 < M2; c2++) pfb_store(q, c1 + M1 * c2, O0 + (uint64_t)j, y[c2]);
    }
  }
}

// (the history kernel is k_stream_hist, stream_hist.h, with H = ntaps - 1)

// host side (engine_pfb.inc): the stream state (StreamStage, host_util.h) is the channeliser's own
struct PfbState : StreamStage {
  int M = 2, ntaps = 1, K = 0;
  signed char sel_first[PFB_MAX_CHANNELS] = {}, sel_next[PFB_MAX_CHANNELS] = {};  // PfbParams::first, next
  DevBuf d_taps, d_w;
  void release() {
    d_taps.release();
    d_w.release();
    StreamStage::release();
  }
};
