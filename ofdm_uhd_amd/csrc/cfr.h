// cfr.h -- transmit crest-factor reduction by peak windowing: the last stage in front of a converter, behind ofdm_tx
// and the wideband transmit stages.  A stream stage with the propagation stage's call shape: nin samples in, nin out.
//
// Definition (include/ofdm_hip.h), n the stream index, A the threshold, w[0 .. 2H] the window:
//   m[n] = sqrtf(re * re + im * im)                  float32: two products, one addition, one square root
//   c[n] = m[n] > A ? 1.0f - A / m[n] : 0.0f         (a NaN magnitude gives 0; samples before the stream start are 0)
//   s[n] = sum over k in [0, 2H] of w[k] * c[n - k]  float32 product, then float32 addition, ascending k, from +0
//   b[n] = fmaxf(0.0f, 1.0f - s[n])
//   y[n] = (b[n] * x[n - H].re, b[n] * x[n - H].im)
//   out[n] = store(y[n])
// Every term is a function of the stream alone, whatever the call, the chunk or the tile.  All terms of s are >= +0:
// where every c of a window is 0, s is +0, b is 1 and y[n] is x[n - H] itself.
//
// One workgroup produces T = 256 * 4 consecutive outputs; thread t owns outputs t, t + 256, ...: every global store of
// a wave is one contiguous run (512 bytes of complex64, 256 bytes of 16-bit IQ), and so is the delayed load of
// x[n - H].  The tile stages c[] of its T + 2H inputs in LDS as float32 (at most 2046 words, 8 KB) and keeps, per
// 64 staged words (the words one wave stages in one step), one bit that says whether any of them is not 0.  The
// barrier that publishes the staged words is a __syncthreads_or of those bits:
//   fast path   no staged c of the tile is non-zero: the tile is a coalesced delayed copy.  In a tile that has peaks,
//               a wave whose 64 windows touch no marked group of 64 words does the same for its 64 outputs.
//   slow path   the (2H + 1)-tap sum from LDS: consecutive lanes read consecutive words (conflict-free), the window
//               comes from global memory at a uniform index (scalar loads).
// Both paths give the definition's bits: the fast path is the slow one with every term +0.
//
// Statistics (ofdm_cfr_stats): counts, the two maxima and three float64 sums, per thread, wave and tile and then per
// call in a fixed order (stream_stats.h, shared with mempoly.h): no float atomics.
#pragma once
#include "common.h"
#include "host_util.h"
#include "stream_stats.h"

constexpr int CFR_THREADS = STAT_THREADS;
constexpr int CFR_OPT = 4;  // outputs per thread: T = 1024
constexpr int CFR_TILE = CFR_THREADS * CFR_OPT;
constexpr int CFR_MAX_H = (OFDM_CFR_MAX_TAPS - 1) / 2;
constexpr int CFR_STAGED = CFR_TILE + 2 * CFR_MAX_H;  // 2046 words: 32 groups of 64
static_assert(CFR_STAGED <= 32 * 64, "one mask bit per 64 staged words");

struct CfrParams {
  const c32* x;     // this call's samples; x[0] is the stream's next sample
  const c32* hist;  // the 2H samples before x[0] (zeros before the stream start)
  void* out;
  StatPartial* part;  // one per tile
  uint64_t nin;
  float A;
  int H;
  float scale;  // sc16 output: full scale
};

template <typename OUT>
__global__ void __launch_bounds__(CFR_THREADS) k_cfr(CfrParams q, const float* __restrict__ w) {  // w: 2H + 1 window values
  constexpr int NT = CFR_THREADS, T = CFR_TILE;
  __shared__ float cs[CFR_STAGED];
  __shared__ uint32_t wmask[NT / 64];
  __shared__ StatPartial wpart[NT / 64];
  const int tid = threadIdx.x;
  const int H = q.H, H2 = 2 * q.H;
  const float A = q.A;
  const uint64_t off = (uint64_t)blockIdx.x * T;  // the tile's first output, relative to the call's
  const int64_t g0 = (int64_t)off - H2;           // the first staged sample, relative to x[0]
  const int total = T + H2;
  const int64_t nin = (int64_t)q.nin;
  const bool interior = g0 >= 0 && g0 + total <= nin;
  StatAcc acc;

  // c[] of the tile's inputs into LDS.  In step j a wave stages the 64 words of group 4 j + wave: `mine` gathers the
  // bits of this wave's groups with a non-zero word.  The tile's own inputs (u >= 2H, inside the call) are counted.
  uint32_t mine = 0;
  for (int u = tid, j = 0; u - (tid & 63) < total; u += NT, j++) {
    float c = 0.f;
    if (u < total) {
      const int64_t gi = g0 + u;
      c32 v = mk(0.f, 0.f);
      if (interior) {
        v = q.x[gi];
      } else if (gi >= 0) {
        // (zeros behind the call's end: they feed only outputs the call does not have)
        if (gi < nin) v = q.x[gi];
      } else {
        v = q.hist[gi + H2];  // (gi >= g0 >= -2H); zeros at the stream start
      }
      const float mm = v.re * v.re + v.im * v.im;
      const float m = sqrtf(mm);
      const bool over = m > A;
      if (over) c = 1.0f - A / m;
      cs[u] = c;
      if (u >= H2 && gi < nin) {
        acc.n_over += over ? 1u : 0u;
        acc.peak_in = fmaxf(acc.peak_in, mm);
        acc.sum_in += (double)mm;
      }
    }
    if (__ballot(c != 0.0f) != 0ull) mine |= 1u << (4 * j + (tid >> 6));
  }
  if ((tid & 63) == 0) wmask[tid >> 6] = mine;
  const int tile_any = __syncthreads_or(mine != 0u);
  uint32_t mask = 0;
  if (tile_any) mask = wmask[0] | wmask[1] | wmask[2] | wmask[3];

  OUT* out = static_cast<OUT*>(q.out);
#pragma unroll
  for (int i = 0; i < CFR_OPT; i++) {
    const int u = tid + i * NT;
    const int64_t o = (int64_t)off + u;
    if (o >= nin) continue;
    // x[n - H]: the call's own sample, or one of the carried history
    const int64_t xi = o - H;
    const c32 xd = xi >= 0 ? q.x[xi] : q.hist[xi + H2];
    // the wave's 64 windows lie in the staged words [ub, ub + 63 + 2H]: groups ub / 64 .. (ub + 63 + 2H) / 64
    const int ub = u & ~63;
    const int ga = ub >> 6, gb = (ub + 63 + H2) >> 6;
    const uint32_t window = (gb >= 31 ? 0xFFFFFFFFu : ((2u << gb) - 1u)) & ~((1u << ga) - 1u);
    c32 y = xd;
    if (mask & window) {
      const float* col = cs + (H2 + u);  // col[-k] is c[n - k]
      float s = 0.0f;
      for (int k = 0; k <= H2; k++) s = s + w[k] * col[-k];
      const float b = fmaxf(0.0f, 1.0f - s);
      y = mk(b * xd.re, b * xd.im);
      acc.n_touched += b < 1.0f ? 1u : 0u;
      const float er = y.re - xd.re, ei = y.im - xd.im;
      acc.sum_err += (double)(er * er + ei * ei);
    }
    const float yy = y.re * y.re + y.im * y.im;
    acc.peak_out = fmaxf(acc.peak_out, yy);
    acc.sum_out += (double)yy;
    iq_store(out, o, y, q.scale);
  }

  const StatPartial p = stat_block_reduce<NT / 64>(acc, wpart, tid);
  if (tid == 0) q.part[blockIdx.x] = p;
}

// (the history kernel is k_stream_hist<c32>, stream_hist.h, with H = 2H: the last 2H inputs after a call)

// host side (engine_cfr.inc): StreamStage (host_util.h; hist = 2H) and the stage's own
struct CfrState : StreamStage {
  int H = 0;
  float A = 0.f;
  int out_fmt = OFDM_IQ_FC32;
  float out_scale = 32768.0f;
  DevBuf d_w;
  StatState st;  // since ofdm_set_cfr / ofdm_cfr_reset
  void release() {
    d_w.release();
    st.release();
    StreamStage::release();
  }
};
