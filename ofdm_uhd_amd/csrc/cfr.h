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
// Statistics (ofdm_cfr_stats): counts, the two maxima and three float64 sums.  A thread adds its own terms in
// ascending order, a wave reduces by an xor butterfly, thread 0 adds the four waves' results in ascending order and
// writes the tile's partial; k_cfr_reduce adds the partials of a call in a fixed order, in one or two levels, onto the
// running totals.  No float atomics: a call's sums depend on nothing but its samples and its length.
#pragma once
#include "common.h"
#include "host_util.h"

constexpr int CFR_THREADS = 256;
constexpr int CFR_OPT = 4;  // outputs per thread: T = 1024
constexpr int CFR_TILE = CFR_THREADS * CFR_OPT;
constexpr int CFR_MAX_H = (OFDM_CFR_MAX_TAPS - 1) / 2;
constexpr int CFR_STAGED = CFR_TILE + 2 * CFR_MAX_H;  // 2046 words: 32 groups of 64
constexpr int CFR_REDUCE_SPAN = 4096;                  // partials one workgroup of k_cfr_reduce adds
static_assert(CFR_STAGED <= 32 * 64, "one mask bit per 64 staged words");

struct CfrPartial {  // of one tile, or of CFR_REDUCE_SPAN tiles
  double sum_in, sum_out, sum_err;
  float peak_in, peak_out;
  uint32_t n_over, n_touched;
};
struct CfrTotals {  // since ofdm_set_cfr / ofdm_cfr_reset
  double sum_in, sum_out, sum_err;
  float peak_in, peak_out;
  uint64_t n_over, n_touched;
};

struct CfrParams {
  const c32* x;     // this call's samples; x[0] is the stream's next sample
  const c32* hist;  // the 2H samples before x[0] (zeros before the stream start)
  void* out;
  CfrPartial* part;  // one per tile
  uint64_t nin;
  float A;
  int H;
  float scale;  // sc16 output: full scale
};

// the float64 / float32 / uint32 reductions of one wave: every lane ends with the same value, in a fixed order
__device__ __forceinline__ double cfr_wave_sum(double v) {
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) v += __shfl_xor(v, s, 64);
  return v;
}
__device__ __forceinline__ float cfr_wave_max(float v) {
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) v = fmaxf(v, __shfl_xor(v, s, 64));
  return v;
}
__device__ __forceinline__ uint32_t cfr_wave_count(uint32_t v) {
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) v += __shfl_xor(v, s, 64);
  return v;
}

struct CfrAcc {  // a thread's statistics
  double sum_in = 0.0, sum_out = 0.0, sum_err = 0.0;
  float peak_in = 0.f, peak_out = 0.f;
  uint32_t n_over = 0, n_touched = 0;
};

// the workgroup's accumulators into one partial (thread 0 holds it on return); sh: one CfrPartial per wave
template <int NW>
__device__ __forceinline__ CfrPartial cfr_block_reduce(const CfrAcc& a, CfrPartial* sh, int tid) {
  CfrPartial p;
  p.sum_in = cfr_wave_sum(a.sum_in);
  p.sum_out = cfr_wave_sum(a.sum_out);
  p.sum_err = cfr_wave_sum(a.sum_err);
  p.peak_in = cfr_wave_max(a.peak_in);
  p.peak_out = cfr_wave_max(a.peak_out);
  p.n_over = cfr_wave_count(a.n_over);
  p.n_touched = cfr_wave_count(a.n_touched);
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

template <typename OUT>
__global__ void __launch_bounds__(CFR_THREADS) k_cfr(CfrParams q, const float* __restrict__ w) {  // w: 2H + 1 window values
  constexpr int NT = CFR_THREADS, T = CFR_TILE;
  __shared__ float cs[CFR_STAGED];
  __shared__ uint32_t wmask[NT / 64];
  __shared__ CfrPartial wpart[NT / 64];
  const int tid = threadIdx.x;
  const int H = q.H, H2 = 2 * q.H;
  const float A = q.A;
  const uint64_t off = (uint64_t)blockIdx.x * T;  // the tile's first output, relative to the call's
  const int64_t g0 = (int64_t)off - H2;           // the first staged sample, relative to x[0]
  const int total = T + H2;
  const int64_t nin = (int64_t)q.nin;
  const bool interior = g0 >= 0 && g0 + total <= nin;
  CfrAcc acc;

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

  const CfrPartial p = cfr_block_reduce<NT / 64>(acc, wpart, tid);
  if (tid == 0) q.part[blockIdx.x] = p;
}

// The partials of a call into the totals, in a fixed order.  LAST = false: workgroup g adds in[g * SPAN .. ) (SPAN of
// them, fewer in the last) into out[g].  LAST = true: one workgroup adds all n (at most SPAN) onto *tot.
template <bool LAST>
__global__ void __launch_bounds__(CFR_THREADS) k_cfr_reduce(const CfrPartial* __restrict__ in, uint32_t n, CfrPartial* __restrict__ out,
                                                            CfrTotals* __restrict__ tot) {
  __shared__ CfrPartial wpart[CFR_THREADS / 64];
  const int tid = threadIdx.x;
  const uint32_t lo = blockIdx.x * (uint32_t)CFR_REDUCE_SPAN;
  const uint32_t hi = min(n, lo + (uint32_t)CFR_REDUCE_SPAN);
  CfrAcc a;
  for (uint32_t i = lo + tid; i < hi; i += CFR_THREADS) {
    const CfrPartial p = in[i];
    a.sum_in += p.sum_in;
    a.sum_out += p.sum_out;
    a.sum_err += p.sum_err;
    a.peak_in = fmaxf(a.peak_in, p.peak_in);
    a.peak_out = fmaxf(a.peak_out, p.peak_out);
    a.n_over += p.n_over;
    a.n_touched += p.n_touched;
  }
  const CfrPartial p = cfr_block_reduce<CFR_THREADS / 64>(a, wpart, tid);
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

// (the history kernel is k_stream_hist<c32>, stream_hist.h, with H = 2H: the last 2H inputs after a call)

// host side (engine_cfr.inc): StreamStage (host_util.h; hist = 2H) and the stage's own
struct CfrState : StreamStage {
  int H = 0;
  float A = 0.f;
  int out_fmt = OFDM_IQ_FC32;
  float out_scale = 32768.0f;
  uint64_t n = 0;          // samples since ofdm_set_cfr / ofdm_cfr_reset
  DevBuf d_w, d_part, d_part2, d_tot;
  void release() {
    d_w.release();
    d_part.release();
    d_part2.release();
    d_tot.release();
    StreamStage::release();
  }
};
