// duc.h -- wideband transmit: polyphase interpolating FIR followed by a frequency shift, behind ofdm_tx (the mirror
// image of ddc.h; the reference leaves it to its radio: sink.set_interp / set_center_freq, usrp_transmit_path.py).
//
// Definition (include/ofdm_hip.h), output n = m L + p, p in [0, L):
//   v[n] = sum over q >= 0 with p + q L < ntaps of h[p + q L] x[m - q]       float32, real tap times complex sample
//   y[n] = v[n] r[n]                      r[n] = complex64(expj(+2 pi Phi_n / 2^64)), Phi_n = n D mod 2^64
//   out[n] = store(y[n] + add[n]) or store(y[n])
// x[m] is indexed from the last reset, zero before it.  v[n] is ONE chain of packed FMAs on the (re, im) pair in
// ascending q, begun at +0: a function of n alone, whatever the call, the chunk or the tile.
//
// One workgroup produces T = 256 * OPT consecutive outputs; thread t owns outputs t, t + 256, ...: consecutive lanes
// own consecutive outputs, so every global store of a wave is one contiguous run (512 bytes of complex64, 256 bytes
// of 16-bit IQ) and the `add` loads are the same runs.  The tile's inputs x[mb - Q .. mb + ceil((r0 + T) / L)) (mb,
// r0: quotient and remainder of the tile's first output index by L; Q = (ntaps - 1) / L) are staged once in LDS with
// the taps.  In the tap loop a 32-lane group reads
//   x:   consecutive 8-byte words, L lanes on each (broadcast): at most 32 / L + 2 distinct words, one bank pair each;
//   tap: the dword h[p + q L], p = n mod L: min(L, 32) distinct consecutive dwords (cyclically within the row of L).
// Both are conflict-free for L <= 32 and L = 64; for 32 < L < 64 the tap row wraps inside the group and up to
// 64 - L banks are hit twice.
#pragma once
#include "common.h"
#include "ddc.h"  // ddc_f2, stream_tile.h
#include "host_util.h"

constexpr int DUC_THREADS = 256;
constexpr int DUC_MAX_INTERP = 64;

struct DucParams {
  const c32* x;     // this call's narrowband samples; x[0] is stream sample a
  const c32* hist;  // the Q samples before x[0] (zeros before the stream start)
  const float* taps;
  const c32* add;   // nin L samples, or unused (ADD = false); may be `out` itself
  void* out;        // out[0] is output a L
  uint64_t nin, a, nout;
  uint64_t D;       // phase advance per output, 2^-64 turn
  uint64_t magic;   // floor(2^32 / L) + 1: u / L = (u * magic) >> 32 for every u of a tile
  int L, ntaps, Q;
  float scale;      // sc16 output: full scale
};

// geometry per interpolation: OPT outputs per thread, T = 256 * OPT outputs per workgroup.  The inner product has
// ceil(ntaps / L) steps per output whatever the tile; what a tile amortises is the Q staged samples of history and
// the taps, so long filters at small L take the larger tile.
struct DucGeom {
  int opt;
  int T() const { return opt * DUC_THREADS; }
};
static inline DucGeom duc_geom(int L) {
  if (L <= 2) return DucGeom{8};  // T = 2048 (Q up to 1023 staged samples per tile)
  return DucGeom{4};              // T = 1024
}
// staged samples of a tile: Q of history and the inputs of r0 + T outputs, r0 < L
static inline int duc_staged(int T, int L, int Q) { return Q + (T + 2 * L - 2) / L; }
static inline size_t duc_lds_bytes(int L, int ntaps) {
  const int Q = (ntaps - 1) / L;
  return (size_t)((ntaps + 1) & ~1) * sizeof(float) + (size_t)duc_staged(duc_geom(L).T(), L, Q) * sizeof(c32);
}

template <typename OUT, bool ADD, int OPT>
__global__ void __launch_bounds__(DUC_THREADS) k_duc(DucParams q) {
  constexpr int NT = DUC_THREADS, T = NT * OPT;
  extern __shared__ __align__(16) unsigned char duc_lds[];
  float* tap = reinterpret_cast<float*>(duc_lds);
  c32* xs = reinterpret_cast<c32*>(tap + ((q.ntaps + 1) & ~1));
  const int tid = threadIdx.x;
  const int L = q.L, Q = q.Q;
  // the tile's first output is a L + off: input mb = a + off / L, phase r0 = off % L
  const uint64_t off = (uint64_t)blockIdx.x * T;
  const uint64_t dq = off / (uint64_t)L;
  const int r0 = (int)(off - dq * (uint64_t)L);
  const int64_t g0 = (int64_t)dq - Q;  // the first staged sample, relative to x[0]
  const int total = Q + (r0 + T + L - 1) / L;

  for (int k = tid; k < q.ntaps; k += NT) tap[k] = q.taps[k];
  if (g0 >= 0 && g0 + total <= (int64_t)q.nin) {
    // interior tile: every sample comes from x, no per-sample test against the stream
    for (int u = tid; u < total; u += NT) xs[u] = q.x[g0 + u];
  } else {
    // first and last tiles: the carried history (zeros at the stream start) before x[0]; zeros behind the call's end
    // (they feed only outputs the call does not have) and before the oldest sample the history holds
    for (int u = tid; u < total; u += NT) {
      const int64_t gi = g0 + u;
      c32 v = mk(0.f, 0.f);
      if (gi >= 0) {
        if (gi < (int64_t)q.nin) v = q.x[gi];
      } else if (gi + Q >= 0) {
        v = q.hist[gi + Q];
      }
      xs[u] = v;
    }
  }
  __syncthreads();

  ddc_f2 A[OPT];
  const c32* col[OPT];
  const float* tp[OPT];
  int left[OPT];  // taps of this output's phase: q < left
#pragma unroll
  for (int i = 0; i < OPT; i++) {
    const int u = r0 + tid + i * NT;
    const int dm = (int)(((uint64_t)(uint32_t)u * q.magic) >> 32);
    const int p = u - dm * L;
    A[i] = ddc_f2{0.f, 0.f};
    col[i] = xs + (Q + dm);
    tp[i] = tap + p;
    left[i] = p < q.ntaps ? (q.ntaps - 1 - p) / L + 1 : 0;
  }
  for (int qq = 0; qq <= Q; qq++) {
#pragma unroll
    for (int i = 0; i < OPT; i++) {
      if (qq < left[i]) {
        const float h = tp[i][qq * L];
        const ddc_f2 s = *reinterpret_cast<const ddc_f2*>(col[i] - qq);
        A[i] = __builtin_elementwise_fma(ddc_f2{h, h}, s, A[i]);
      }
    }
  }

  OUT* out = static_cast<OUT*>(q.out);
#pragma unroll
  for (int i = 0; i < OPT; i++) {
    const uint64_t o = off + (uint64_t)(tid + i * NT);
    if (o >= q.nout) continue;
    const uint64_t n = q.a * (uint64_t)L + o;
    c32 y = nco_rotate(mk(A[i].x, A[i].y), n * q.D);
    if constexpr (ADD) y = cadd(y, q.add[o]);  // read before the store below: `add` may be `out`
    iq_store(out, (int64_t)o, y, q.scale);
  }
}

// (the history kernel is k_stream_hist<c32>, stream_hist.h, with H = Q: the last Q inputs after a call)

// host side (engine_duc.inc): StreamStage (host_util.h; hist = Q) and the DUC's own
struct DucState : StreamStage {
  int L = 1, ntaps = 1;
  int out_fmt = OFDM_IQ_FC32;
  float out_scale = 32768.0f;
  uint64_t D = 0;     // frac(fc) in 2^-64 turn
  DevBuf d_taps;
  void release() {
    d_taps.release();
    StreamStage::release();
  }
};
