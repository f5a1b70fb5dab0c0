// mempoly.h -- a memory polynomial over the stream: with one coefficient table the behavioural model of a power
// amplifier (the air side, slot OFDM_MEMPOLY_PA), with another that amplifier's digital predistorter (the transmit side,
// slot OFDM_MEMPOLY_DPD, behind cfr.h and in front of the converter).  A stream stage with cfr.h's call shape: nin
// samples in, nin out, no delay.
//
// Definition (include/ofdm_hip.h), M taps of memory, K odd orders 1, 3, .., 2K - 1, a[m][k] the
// coefficients, n the stream index since the last reset, x zero before it; float32, every operation rounded once:
//   p[j]   = x[j].re * x[j].re + x[j].im * x[j].im      two products, one addition
//   h_m[j] = Horner in p[j] from the top: h = a[m][K-1]; for k = K-2 .. 0: h = (h.re * p + a[m][k].re, h.im * p + a[m][k].im)
//                                                        product, then addition: never an fmaf
//   t_m[n] = cmul(h_m[n - m], x[n - m])                  the gr_complex product (common.h)
//   y[n]   = t_0[n] + t_1[n] + .. + t_{M-1}[n]           float32 additions per part, ascending m, from t_0 (not from +0)
//   out[n] = store(y[n])
// Every term is a function of the stream alone, whatever the call, the chunk or the tile.
//
// One workgroup produces T = 256 * 4 consecutive outputs; thread t owns outputs t, t + 256, ..: every global store of a
// wave is one contiguous run (512 bytes of complex64, 256 bytes of 16-bit IQ).  The tile's T + M - 1 inputs are staged
// once in LDS (at most 1031 samples, 8248 bytes); the call's first tile takes its first M - 1 from the carried history.
// In the tap loop a wave reads 64 consecutive 8-byte words at the uniform offset -m: conflict-free.  p is formed again
// for each of the M uses of a sample (three operations) instead of being staged next to x: the term (m, j) is used by
// exactly one output, so nothing but p could be shared, and a second LDS array costs a read where this costs three
// operations of the 4 K + 7 a term has.  K is a template parameter (the Horner chain is unrolled and its length
// known); M is a run-time bound on an unrolled tap loop (a uniform exit) that runs outside the loop over the thread's
// four outputs, so a tap's coefficients a[m][k] are read once, at constant indices of the kernel's params: scalar
// loads into scalar registers.
//
// Statistics (ofdm_mempoly_stats) follow stream_stats.h: n_over counts outputs with |y|^2 > limit2 (the float32
// limit * limit; +inf: none), peak_in / sum_in are over p, peak_out / sum_out over |y|^2 = y.re * y.re + y.im * y.im.
#pragma once
#include "common.h"
#include "host_util.h"
#include "stream_stats.h"

constexpr int MPOLY_THREADS = STAT_THREADS;
constexpr int MPOLY_OPT = 4;  // outputs per thread: T = 1024
constexpr int MPOLY_TILE = MPOLY_THREADS * MPOLY_OPT;
constexpr int MPOLY_MAX_M = OFDM_MEMPOLY_MAX_MEMORY;
constexpr int MPOLY_MAX_K = OFDM_MEMPOLY_MAX_ORDERS;
constexpr int MPOLY_STAGED = MPOLY_TILE + MPOLY_MAX_M - 1;

struct MempolyParams {
  const c32* x;     // this call's samples; x[0] is the stream's next sample
  const c32* hist;  // the M - 1 samples before x[0] (zeros before the stream start)
  void* out;
  StatPartial* part;  // one per tile
  uint64_t nin;
  int M;
  float limit2;  // n_over counts |y|^2 above it
  float scale;   // sc16 output: full scale
  c32 a[MPOLY_MAX_M][MPOLY_MAX_K];
};

template <typename OUT, int K>
__global__ void __launch_bounds__(MPOLY_THREADS) k_mempoly(MempolyParams q) {
  constexpr int NT = MPOLY_THREADS, T = MPOLY_TILE;
  __shared__ c32 xs[MPOLY_STAGED];
  __shared__ StatPartial wpart[NT / 64];
  const int tid = threadIdx.x;
  const int M = q.M, M1 = q.M - 1;
  const uint64_t off = (uint64_t)blockIdx.x * T;  // the tile's first output, relative to the call's
  const int64_t g0 = (int64_t)off - M1;           // the first staged sample, relative to x[0]
  const int total = T + M1;
  const int64_t nin = (int64_t)q.nin;

  if (g0 >= 0 && g0 + total <= nin) {
    // interior tile: every sample comes from x, no per-sample test against the stream
    for (int u = tid; u < total; u += NT) xs[u] = q.x[g0 + u];
  } else {
    // first and last tiles: the carried history (zeros at the stream start) before x[0]; zeros behind the call's end
    // (they feed only outputs the call does not have)
    for (int u = tid; u < total; u += NT) {
      const int64_t gi = g0 + u;
      c32 v = mk(0.f, 0.f);
      if (gi >= 0) {
        if (gi < nin) v = q.x[gi];
      } else {
        v = q.hist[gi + M1];  // (gi >= g0 >= -(M - 1))
      }
      xs[u] = v;
    }
  }
  __syncthreads();

  // tap by tap over the thread's four outputs: a tap's K coefficients are read once (scalar loads at constant
  // offsets of the params) and feed four independent chains.  Outputs behind the call's end are formed from the
  // staged zeros and dropped.
  const c32* col = xs + (M1 + tid);  // col[i * NT - m] is x[n - m] of output i
  c32 y[MPOLY_OPT];
  float p0[MPOLY_OPT];
#pragma unroll
  for (int m = 0; m < MPOLY_MAX_M; m++) {
    if (m >= M) break;
#pragma unroll
    for (int i = 0; i < MPOLY_OPT; i++) {
      const c32 x = col[i * NT - m];
      const float p = x.re * x.re + x.im * x.im;
      c32 h = q.a[m][K - 1];
#pragma unroll
      for (int k = K - 2; k >= 0; k--) h = mk(h.re * p + q.a[m][k].re, h.im * p + q.a[m][k].im);
      const c32 t = cmul(h, x);
      if (m == 0) {
        y[i] = t;
        p0[i] = p;
      } else {
        y[i] = cadd(y[i], t);
      }
    }
  }

  StatAcc acc;
  OUT* out = static_cast<OUT*>(q.out);
#pragma unroll
  for (int i = 0; i < MPOLY_OPT; i++) {
    const int64_t o = (int64_t)off + tid + i * NT;
    if (o >= nin) continue;
    acc.peak_in = fmaxf(acc.peak_in, p0[i]);
    acc.sum_in += (double)p0[i];
    const float yy = y[i].re * y[i].re + y[i].im * y[i].im;
    acc.n_over += yy > q.limit2 ? 1u : 0u;
    acc.peak_out = fmaxf(acc.peak_out, yy);
    acc.sum_out += (double)yy;
    iq_store(out, o, y[i], q.scale);
  }

  const StatPartial p = stat_block_reduce<NT / 64>(acc, wpart, tid);
  if (tid == 0) q.part[blockIdx.x] = p;
}

// (the history kernel is k_stream_hist<c32>, stream_hist.h, with H = M - 1: the last M - 1 inputs after a call)

// host side (engine_mempoly.inc): StreamStage (host_util.h; hist = M - 1) and the stage's own.  A handle holds one per
// slot, each with its own history, statistics and timer.
struct MempolyState : StreamStage {
  int M = 1, K = 1;
  int out_fmt = OFDM_IQ_FC32;
  float out_scale = 32768.0f;
  float limit2 = 0.f;
  c32 a[MPOLY_MAX_M][MPOLY_MAX_K] = {};
  StatState st;  // since ofdm_set_mempoly / ofdm_mempoly_reset
  void release() {
    st.release();
    StreamStage::release();
  }
};
