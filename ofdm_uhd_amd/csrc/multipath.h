// multipath.h -- the propagation channel between ofdm_tx and ofdm_rx: delayed paths with complex gains and Doppler
// shifts, continuous tones, then ofdm_chan's carrier rotation and noise (the reference has a radio pair and the air
// there: usrp_transmit_path.py -> usrp_receive_path.py).  A stream stage with the DUC's call shape at L = 1.
//
// Definition (include/ofdm_hip.h), n the absolute stream index:
//   c_p[n] = g_p where D_p == 0, else g_p * complex64(expj(2 pi (n D_p mod 2^64) / 2^64))      gr_complex product
//   v[n]   = sum_p c_p[n] x[n - d_p]                  gr_complex products, float32 additions in ascending p from +0
//   t[n]   = sum_j a_j complex64(expj(2 pi ((Psi_j + n F_j) mod 2^64) / 2^64))                 ascending j from +0
//   z[n]   = channel_apply(v[n] + t[n], n, sigma, cfo, seed, stream_id)                        common.h
//   out[n] = store(z[n] + add[n]) or store(z[n])
// x[n] is indexed from the last reset, zero before it.  Every term is a function of n alone, whatever the call, the
// chunk or the tile: each phasor is nco_rotate's float64 evaluation at its own phase, nothing is advanced by a
// recurrence.
//
// One workgroup produces T = 256 * OPT consecutive outputs; thread t owns outputs t, t + 256, ...: consecutive lanes
// own consecutive outputs, so every global store of a wave is one contiguous run (512 bytes of complex64, 256 bytes
// of 16-bit IQ) and the `add` loads are the same runs.  The tile's inputs x[n0 - Dmax .. n0 + T) are staged once in
// LDS (at most 1023 + 1024 samples, 16 KB); in the path loop a wave reads 64 consecutive 8-byte words at the uniform
// offset -d_p: conflict-free.  The path parameters travel in the kernel's Params (scalar registers: p is uniform).
//
// PHASOR says whether any float64 phasor is evaluated (a Doppler path, a tone or a carrier offset), NOISE whether
// sigma > 0: a static profile is P loads from LDS and 4 P float32 multiplies per output and is bound by memory; with
// PHASOR each Doppler path and each tone costs one dexpj per output.
#pragma once
#include "common.h"
#include "host_util.h"
#include "stream_tile.h"  // nco_rotate's phasor: dexpj, nco_radians

constexpr int MP_THREADS = 256;
constexpr int MP_OPT = 4;  // outputs per thread: T = 1024
constexpr int MP_TILE = MP_THREADS * MP_OPT;
constexpr uint64_t MULTIPATH_MAX_INDEX = 1ull << 53;  // chan_rotate's double(cfo) * double(n) is exact up to here

struct MultipathParams {
  const c32* x;     // this call's samples; x[0] is stream sample a
  const c32* hist;  // the Dmax samples before x[0] (zeros before the stream start)
  const c32* add;   // nin samples, or unused (ADD = false); may be `out` itself
  void* out;        // out[0] is output a
  uint64_t nin, a;
  uint64_t seed, stream_id;
  uint64_t D[OFDM_MULTIPATH_MAX_PATHS];    // Doppler phase advance per sample, 2^-64 turn
  uint64_t F[OFDM_MULTIPATH_MAX_TONES];    // a tone's phase advance per sample ...
  uint64_t Psi[OFDM_MULTIPATH_MAX_TONES];  // ... and its phase at index 0
  c32 g[OFDM_MULTIPATH_MAX_PATHS];
  int d[OFDM_MULTIPATH_MAX_PATHS];
  float amp[OFDM_MULTIPATH_MAX_TONES];
  int P, J, Dmax;
  float sigma, cfo;
  float scale;      // sc16 output: full scale
};

static inline size_t multipath_lds_bytes(int Dmax) { return (size_t)(Dmax + MP_TILE) * sizeof(c32); }

// complex64(expj(2 pi phase / 2^64)): nco_rotate's phasor
__device__ __forceinline__ c32 mp_phasor(uint64_t phase) {
  const dc r = dexpj(nco_radians(phase));
  return mk((float)r.re, (float)r.im);
}

template <typename OUT, bool ADD, bool PHASOR, bool NOISE>
__global__ void __launch_bounds__(MP_THREADS) k_multipath(MultipathParams q) {
  constexpr int NT = MP_THREADS, T = MP_TILE;
  extern __shared__ __align__(16) unsigned char mp_lds[];
  c32* xs = reinterpret_cast<c32*>(mp_lds);
  const int tid = threadIdx.x;
  const int Dmax = q.Dmax;
  const uint64_t off = (uint64_t)blockIdx.x * T;  // the tile's first output, relative to the call's
  const int64_t g0 = (int64_t)off - Dmax;         // the first staged sample, relative to x[0]
  const int total = Dmax + T;

  if (g0 >= 0 && g0 + total <= (int64_t)q.nin) {
    // interior tile: every sample comes from x, no per-sample test against the stream
    for (int u = tid; u < total; u += NT) xs[u] = q.x[g0 + u];
  } else {
    // first and last tiles: the carried history (zeros at the stream start) before x[0]; zeros behind the call's end
    // (they feed only outputs the call does not have)
    for (int u = tid; u < total; u += NT) {
      const int64_t gi = g0 + u;
      c32 v = mk(0.f, 0.f);
      if (gi >= 0) {
        if (gi < (int64_t)q.nin) v = q.x[gi];
      } else if (gi + Dmax >= 0) {
        v = q.hist[gi + Dmax];
      }
      xs[u] = v;
    }
  }
  __syncthreads();

  OUT* out = static_cast<OUT*>(q.out);
#pragma unroll
  for (int i = 0; i < MP_OPT; i++) {
    const int u = tid + i * NT;
    const uint64_t o = off + (uint64_t)u;
    if (o >= q.nin) continue;
    const uint64_t n = q.a + o;
    const c32* col = xs + (Dmax + u);
    c32 v = mk(0.f, 0.f);
    for (int p = 0; p < q.P; p++) {
      c32 c = q.g[p];
      if constexpr (PHASOR) {
        if (q.D[p] != 0) c = cmul(c, mp_phasor(n * q.D[p]));
      }
      v = cadd(v, cmul(c, col[-q.d[p]]));
    }
    if constexpr (PHASOR) {
      if (q.J > 0) {
        c32 t = mk(0.f, 0.f);
        for (int j = 0; j < q.J; j++) {
          const c32 r = mp_phasor(q.Psi[j] + n * q.F[j]);
          t = cadd(t, mk(q.amp[j] * r.re, q.amp[j] * r.im));
        }
        v = cadd(v, t);
      }
    }
    c32 y = channel_apply(v, n, NOISE ? q.sigma : 0.0f, PHASOR ? q.cfo : 0.0f, q.seed, q.stream_id);
    if constexpr (ADD) y = cadd(y, q.add[o]);  // read before the store below: `add` may be `out`
    iq_store(out, (int64_t)o, y, q.scale);
  }
}

// (the history kernel is k_stream_hist<c32>, stream_hist.h, with H = Dmax: the last Dmax inputs after a call)

// host side (engine_multipath.inc): StreamStage (host_util.h; hist = Dmax) and the stage's own
struct MultipathState : StreamStage {
  int P = 1, J = 0;
  int out_fmt = OFDM_IQ_FC32;
  float out_scale = 32768.0f;
  float sigma = 0.f, cfo = 0.f;
  uint64_t seed = 0, stream_id = 0;
  bool phasor = false;  // a Doppler path, a tone or a carrier offset: float64 phasors are evaluated
  int d[OFDM_MULTIPATH_MAX_PATHS] = {0};
  c32 g[OFDM_MULTIPATH_MAX_PATHS] = {};
  uint64_t D[OFDM_MULTIPATH_MAX_PATHS] = {0};
  float amp[OFDM_MULTIPATH_MAX_TONES] = {0};
  uint64_t F[OFDM_MULTIPATH_MAX_TONES] = {0}, Psi[OFDM_MULTIPATH_MAX_TONES] = {0};
};
