// tx_resamp.h -- wideband transmit at a rate that is no integer multiple of the modem's: rational-rate (L / M) polyphase
// resampler followed by a frequency shift, behind ofdm_tx (the mirror image of resamp.h, the generalisation of duc.h).
//
// Definition (include/ofdm_hip.h), output n at position n M on the L-times grid:
//   i_n = floor(n M / L), p_n = n M mod L
//   v[n] = sum over q >= 0 with p_n + q L < ntaps of h[p_n + q L] x[i_n - q]     float32, real tap times complex sample
//   y[n] = v[n] r[n]                      r[n] = complex64(expj(+2 pi Phi_n / 2^64)), Phi_n = n D mod 2^64
//   out[n] = store(y[n] + add[n]) or store(y[n])
// x[i] is indexed from the last reset, zero before it.  v[n] is ONE chain of packed FMAs on the (re, im) pair in
// ascending q, begun at +0: a function of n alone, whatever the call, the chunk, the tile or the layout below.  With
// M = 1 the chain, the rotation and the store are k_duc's: the two kernels give the same bits.
//
// The geometry is k_resamp's.  A period is L outputs and M inputs: output n = J L + r (r in [0, L)) has
// i_n = J M + floor(r M / L) and p_n = r M mod L.  One workgroup produces TJ consecutive periods.  A wave works on one
// phase class r at a time, its lanes on consecutive periods: p is wave-uniform (the tap read is a broadcast) and the
// input index advances by M per lane.  The tile's inputs, with QM = ceil(Q / M) periods of history in front
// (Q = (ntaps - 1) / L), are read once and staged into M rows: sample (J0 - QM + c) M + rho sits in row rho, column c,
// so for every tap the lanes read consecutive 8-byte words -- no bank conflict at any (L, M).  The row pitch W is odd,
// which spreads the staging stores (consecutive samples, consecutive rows) over the banks.  The sums go through LDS
// ([r][period], odd pitch) and leave in output order: rotation, optional `add` load, one contiguous store per wave.
#pragma once
#include "common.h"
#include "ddc.h"  // ddc_f2, ddc_f4, stream_tile.h
#include "host_util.h"
#include "resamp.h"    // resamp_geom, resamp_hist_periods, resamp_pitch
#include "stream_hist.h"  // k_stream_hist

constexpr int TX_RESAMP_THREADS = 256;
constexpr int TX_RESAMP_MAX_RATIO = 64;       // largest L and largest M
constexpr int TX_RESAMP_WIDE_INPUTS = 4096;   // a tile is widened (below) only while it stages at most this many inputs

struct TxResampParams {
  const c32* x;     // this call's narrowband samples; x[0] is stream sample a
  const c32* hist;  // the Q samples before x[0] (zeros before the stream start)
  const float* taps;
  const c32* add;   // nout samples, or unused (ADD = false); may be `out` itself
  void* out;        // out[0] is output n0
  uint64_t nin, a, n0, nout;
  uint64_t J0;      // period of the first tile: n0 / L
  uint64_t D;       // phase advance per output, 2^-64 turn
  uint64_t magicM;  // floor(2^32 / M) + 1: u / M = (u * magicM) >> 32 for every u of a tile
  uint64_t magicL;  // the same for L
  int L, M, ntaps, Q, QM, W, TP, KC;
  float scale;      // sc16 output: full scale
};

// geometry per (L, M): a tile is TJ = 64 KC periods (TJ L outputs from TJ M inputs).  KC starts from k_resamp's; the
// work items of a tile are its L KC (phase class, 64 periods) pairs, and where those are fewer than the waves -- an
// output has one chain, it cannot be split as k_resamp splits it -- the tile takes more periods instead, as long as
// its inputs stay within TX_RESAMP_WIDE_INPUTS samples of LDS.
struct TxResampGeom {
  int kc;
  int TJ() const { return WAVE * kc; }
};
static inline TxResampGeom tx_resamp_geom(int L, int M) {
  int kc = resamp_geom(L, M).kc;
  while (L * kc < TX_RESAMP_THREADS / WAVE && 2 * kc * WAVE * M <= TX_RESAMP_WIDE_INPUTS) kc *= 2;
  return TxResampGeom{kc};
}
// LDS: the taps (float32, an even count: the rows stay 8-byte aligned), the M staged rows, the sums on their way out
static inline size_t tx_resamp_lds_bytes(int L, int M, int ntaps) {
  const TxResampGeom g = tx_resamp_geom(L, M);
  const int QM = resamp_hist_periods((ntaps - 1) / L, M);
  const size_t tap = (size_t)((ntaps + 1) & ~1) * sizeof(float);
  const size_t rows = ((size_t)M * resamp_pitch(g.TJ(), QM) + 1) & ~(size_t)1;
  const size_t sums = (size_t)L * (g.TJ() | 1);
  return tap + (rows + sums) * sizeof(c32);
}

template <typename OUT, bool ADD>
__global__ void __launch_bounds__(TX_RESAMP_THREADS) k_tx_resamp(TxResampParams q) {
  constexpr int NT = TX_RESAMP_THREADS, NW = NT / WAVE;
  extern __shared__ __align__(16) unsigned char tx_resamp_lds[];
  float* tap = reinterpret_cast<float*>(tx_resamp_lds);
  c32* xs = reinterpret_cast<c32*>(tap + ((q.ntaps + 1) & ~1));
  c32* ob = xs + ((q.M * q.W + 1) & ~1);
  const int tid = threadIdx.x;
  const int L = q.L, M = q.M, W = q.W, Q = q.Q, QM = q.QM, TJ = q.KC * WAVE, TO = TJ * L;
  const c32* x = q.x;
  const uint64_t J0 = q.J0 + (uint64_t)blockIdx.x * (uint64_t)TJ;
  // the tile's first staged sample, relative to x[0]: (J0 - QM) M - a
  const int64_t g0 = ((int64_t)J0 - QM) * M - (int64_t)q.a;
  const int total = (TJ + QM) * M;

  for (int k = tid; k < q.ntaps; k += NT) tap[k] = q.taps[k];
  if (g0 >= 1 && g0 + total + 1 <= (int64_t)q.nin) {
    // interior tile: every sample comes from x, no per-sample test against the stream.  16 bytes per lane, on the
    // 16-byte grid of the caller's buffer (the pair may begin one sample before the tile and end one behind it)
    const int e = (int)((((uintptr_t)x >> 3) + (uint64_t)g0) & 1u);
    for (int u = 2 * tid - e; u < total; u += 2 * NT) {
      const ddc_f4 v = *reinterpret_cast<const ddc_f4*>(x + (g0 + u));
      if (u >= 0) polyphase_put(xs, q.magicM, q.M, q.W, u, mk(v.x, v.y));
      if (u + 1 < total) polyphase_put(xs, q.magicM, q.M, q.W, u + 1, mk(v.z, v.w));
    }
  } else {
    // first and last tiles: the carried history (zeros at the stream start) before x[0], zeros behind the call's end
    // (those feed only outputs the call does not have) and before the oldest sample the history holds
    for (int u = tid; u < total; u += NT) {
      const int64_t gi = g0 + u;
      c32 v = mk(0.f, 0.f);
      if (gi >= 0) {
        if (gi < (int64_t)q.nin) v = x[gi];
      } else if (gi + Q >= 0) {
        v = q.hist[gi + Q];
      }
      polyphase_put(xs, q.magicM, q.M, q.W, u, v);
    }
  }
  __syncthreads();

  // work item = (phase class r, 64 periods); a wave takes every NW-th one: all its indices are wave-uniform
  const int lane = tid & (WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
  const int nwork = L * q.KC;
  for (int wi = wave; wi < nwork; wi += NW) {
    const int r = wi / q.KC;
    const int t = (wi - r * q.KC) * WAVE + lane;
    const int rm = r * M, off = rm / L, p = rm - off * L;
    const int nq = p < q.ntaps ? (q.ntaps - 1 - p) / L + 1 : 0;
    // sample i - qq of period t: row (off - qq) mod M, column t + QM + floor((off - qq) / M)
    int row = off, col = QM;
    const float* tp = tap + p;
    ddc_f2 A = {0.f, 0.f};
    for (int qq = 0; qq < nq; qq++) {
      const float h = tp[qq * L];
      const ddc_f2 s = *reinterpret_cast<const ddc_f2*>(xs + (row * W + col + t));
      A = __builtin_elementwise_fma(ddc_f2{h, h}, s, A);
      if (--row < 0) {
        row += M;
        col--;
      }
    }
    ob[r * q.TP + t] = mk(A.x, A.y);
  }
  __syncthreads();

  // in output order: the rotation, the band that is there, one contiguous store
  OUT* out = static_cast<OUT*>(q.out);
  for (int j = tid; j < TO; j += NT) {
    const uint64_t n = J0 * (uint64_t)L + (uint64_t)j;
    const uint64_t o = n - q.n0;  // (outputs before n0 wrap to huge values)
    if (o >= q.nout) continue;
    const int t = (int)(((uint64_t)(uint32_t)j * q.magicL) >> 32);
    c32 y = nco_rotate(ob[(j - t * L) * q.TP + t], n * q.D);
    if constexpr (ADD) y = cadd(y, q.add[o]);  // read before the store below: `add` may be `out`
    iq_store(out, (int64_t)o, y, q.scale);
  }
}

// (the history kernel is k_stream_hist<c32>, stream_hist.h, with H = Q: the last Q inputs after a call)

// host side (engine_tx_resamp.inc): StreamStage (host_util.h; hist = Q) and the stage's own
struct TxResampState : StreamStage {
  int L = 1, M = 1, ntaps = 1;
  int out_fmt = OFDM_IQ_FC32;
  float out_scale = 32768.0f;
  uint64_t D = 0;     // frac(fc) in 2^-64 turn
  DevBuf d_taps;
  void release() {
    d_taps.release();
    StreamStage::release();
  }
};
