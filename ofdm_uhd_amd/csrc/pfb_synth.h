// pfb_synth.h -- wideband transmit: polyphase-FFT synthesis bank for links on the c/M grid (the mirror image of pfb.h).
//
// Definition (include/ofdm_hip.h): M channels at c/M cycles per output sample, interpolation M,
// one real prototype h[0..ntaps), output n = m M + p:
//   V_p[m] = sum_c z_c[m] w[(c p) mod M]      z_c = the selected channel's input, (+0, +0) for a channel not selected
//   v[n]   = sum_{q >= 0, qM+p < ntaps} h[qM+p] V_p[m-q]          ONE chain of packed FMAs on (re, im), ascending q,
//                                                                begun at +0
//   out[n] = store(v[n] + add[n]) or store(v[n])
// V[m] = D_M(z[m]) is pfb.h's recursion pfb_dit with pfb.h's table w and pfb.h's schedule (M <= 16 whole; M = 32, 64
// in the two steps M = 8 M2), here over the channel index c: the whole transform, zeros included, so the bits of
// out[n] are a function of n, (M, h) and the M-vector of channel inputs alone -- never of the order of the selection
// or of where a call, a chunk or a tile starts.
//
// One workgroup takes T = 4096 / M consecutive input indices and produces their 4096 consecutive outputs.  The T + Q
// columns (Q = (ntaps - 1) / M; the Q history columns are transformed again by every tile rather than carried: at most
// about a quarter more transforms, and the state stays the plain inputs) are staged in LDS, channel c in row
// rho(c), column j = m - (M0 - Q), pitch P 8-byte words; rows of channels that are not selected are zeroed.
// rho(c) = c for M <= 16 and 8 (c mod M2) + c / M2 otherwise: the first step's thread (column j, r) then reads and
// writes rows 8 r .. 8 r + 7, the second step's (j, c1) reads and writes rows c1, c1 + 8, ..., both in place, and
// V_p ends in row p.  In both steps lanes run along j (consecutive words).
//
// Filter and store: thread t owns outputs t, t + 256, ... of the tile, so its phase p = t mod M is fixed (one tap read
// per q for its 16 outputs), consecutive lanes own consecutive outputs, and every global store and `add` load of a
// wave is one contiguous run (512 bytes of complex64, 256 bytes of 16-bit IQ).  In the tap loop a 32-lane group reads
//   V:   the 8-byte words p P + m' + const, p in [0, min(M, 32)), m' in [0, 32 / M) (M >= 32: one m): with
//        P = 32 / M (mod 32) for M < 32 these are p (32 / M) + m', all 32 residues mod 32; with P odd for M >= 32,
//        p P mod 32 over 32 consecutive p are all 32 residues: 32 distinct bank pairs, no conflict (ds_read_b64 banks
//        (a / 4) mod 64 over 32-lane groups);
//   tap: the dwords h[qM + p]: min(M, 32) consecutive dwords, M >= 32: one each, else 32 / M lanes on each (broadcast).
#pragma once
#include "pfb.h"

constexpr int PFS_THREADS = 256;

struct PfbSynthParams {
  const c32* x;     // selected channel i's inputs of this call begin at x + i * stride; x[0] is input index `next`
  const c32* hist;  // selected channel i's Q inputs before x[0] begin at hist + i * Q (zeros before the stream start)
  const float* taps;
  const c32* w;     // w[j], j in [0, M)
  const c32* add;   // nin M samples, or unused (ADD = false); may be `out` itself
  void* out;        // out[0] is output next * M
  uint64_t nin, stride, nout;
  int ntaps, Q, P;
  float scale;      // sc16 output: full scale
  signed char pos[PFB_MAX_CHANNELS];  // the place of channel c in the selection, -1: not selected
};

static inline int pfb_synth_tile_inputs(int M) { return PFB_TILE / M; }
// the smallest pitch that holds the T + Q columns and has the residue the filter's reads need (see above)
static inline int pfb_synth_pitch(int M, int Q) {
  const int W = pfb_synth_tile_inputs(M) + Q;
  if (M >= 32) return W | 1;
  return W + ((32 / M - W) & 31);
}
static inline size_t pfb_synth_lds_bytes(int M, int ntaps) {
  const int Q = (ntaps - 1) / M;
  return ((size_t)M * pfb_synth_pitch(M, Q) + (size_t)M) * sizeof(c32) + (size_t)ntaps * sizeof(float);
}

template <typename OUT, bool ADD, int M>
__global__ void __launch_bounds__(PFS_THREADS) k_pfb_synth(PfbSynthParams q) {
  constexpr int NT = PFS_THREADS, T = PFB_TILE / M, NB = PFB_TILE / NT, M1 = M <= 16 ? M : 8, M2 = M / M1;
  constexpr int LANES = M <= 16 ? NT : 64, GROUPS = NT / LANES;  // staging: threads along a row, rows side by side
  static_assert(NT % M == 0, "a thread keeps one phase");
  extern __shared__ __align__(16) unsigned char pfs_lds[];
  const int tid = threadIdx.x;
  const int Q = q.Q, P = q.P, W = T + Q;
  c32* xs = reinterpret_cast<c32*>(pfs_lds);
  c32* w = xs + (size_t)M * P;
  float* tap = reinterpret_cast<float*>(w + M);
  const uint64_t M0 = (uint64_t)blockIdx.x * T;  // the tile's first input index, relative to the call's
  const int64_t g0 = (int64_t)M0 - Q;            // the first staged column, relative to x[0]

  for (int k = tid; k < q.ntaps; k += NT) tap[k] = q.taps[k];
  if (tid < M) w[tid] = q.w[tid];
  // interior tile: every column comes from x (one sample to spare on either side for the 16-byte pairs)
  const bool interior = g0 >= 1 && g0 + W + 1 <= (int64_t)q.nin;
  {
    const int grp = tid / LANES, ln = tid % LANES;
    for (int c = grp; c < M; c += GROUPS) {
      c32* dst = xs + (M2 == 1 ? c : 8 * (c % M2) + c / M2) * P;
      const int i = q.pos[c];
      if (i < 0) {
        for (int j = ln; j < W; j += LANES) dst[j] = mk(0.f, 0.f);
        continue;
      }
      const c32* xr = q.x + (uint64_t)i * q.stride;
      if (interior) {
        // 16 bytes per lane, on the 16-byte grid of the caller's row (the pair may begin one sample before the tile)
        const int e = (int)((((uintptr_t)xr >> 3) + (uint64_t)g0) & 1u);
        for (int u = 2 * ln - e; u < W; u += 2 * LANES) {
          const ddc_f4 v = *reinterpret_cast<const ddc_f4*>(xr + (g0 + u));
          if (u >= 0) dst[u] = mk(v.x, v.y);
          if (u + 1 < W) dst[u + 1] = mk(v.z, v.w);
        }
      } else {
        // first and last tiles: the carried history (zeros at the stream start) before x[0], zeros behind the call's
        // end (those feed only outputs the call does not have)
        const c32* hr = q.hist + (int64_t)i * Q;
        for (int j = ln; j < W; j += LANES) {
          const int64_t gi = g0 + j;
          c32 v = mk(0.f, 0.f);
          if (gi >= 0) {
            if (gi < (int64_t)q.nin) v = xr[gi];
          } else {
            v = hr[gi + Q];  // gi + Q = M0 + j >= 0
          }
          dst[j] = v;
        }
      }
    }
  }
  __syncthreads();

  // the transform over c, per column, in place
  if constexpr (M2 == 1) {
    for (int j = tid; j < W; j += NT) {
      c32 v[M], y[M];
#pragma unroll
      for (int c = 0; c < M; c++) v[c] = xs[c * P + j];
      pfb_dit<M, 1, true>(v, y, w, 0, 1, 1);
#pragma unroll
      for (int p = 0; p < M; p++) xs[p * P + j] = y[p];
    }
  } else {
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), ln = tid & 63;
    // first step: sub-transform r of size 8 over the channels r + M2 k, which are rows 8 r + k
    for (int r = wv; r < M2; r += NT / 64) {
      c32* blk = xs + 8 * r * P;
      for (int j = ln; j < W; j += 64) {
        c32 v[M1], y[M1];
#pragma unroll
        for (int k = 0; k < M1; k++) v[k] = blk[k * P + j];
        pfb_dit<M1, 1, true>(v, y, w, 0, 1, M2);
#pragma unroll
        for (int c = 0; c < M1; c++) blk[c * P + j] = y[c];
      }
    }
    __syncthreads();
    // second step: the entries c1 of the M2 sub-transforms (rows c1 + 8 r) give the phases c1 + 8 c2
    for (int c1 = wv; c1 < M1; c1 += NT / 64) {
      c32* blk = xs + c1 * P;
      for (int j = ln; j < W; j += 64) {
        c32 v[M2], y[M2];
#pragma unroll
        for (int r = 0; r < M2; r++) v[r] = blk[8 * r * P + j];
        pfb_dit<M2, 1, false>(v, y, w, c1, M1, 1);
#pragma unroll
        for (int c2 = 0; c2 < M2; c2++) blk[8 * c2 * P + j] = y[c2];
      }
    }
  }
  __syncthreads();

  // the filter: output tid + NT i of the tile is phase p = tid mod M of input index mb + (NT / M) i
  const int p = tid & (M - 1), mb = tid / M;
  const c32* col = xs + p * P + Q + mb;
  const float* tp = tap + p;
  ddc_f2 acc[NB];
#pragma unroll
  for (int i = 0; i < NB; i++) acc[i] = ddc_f2{0.f, 0.f};
  for (int qq = 0; qq < Q; qq++) {
    const float hk = tp[qq * M];
#pragma unroll
    for (int i = 0; i < NB; i++) {
      const ddc_f2 s = *reinterpret_cast<const ddc_f2*>(col + i * (NT / M) - qq);
      acc[i] = __builtin_elementwise_fma(ddc_f2{hk, hk}, s, acc[i]);
    }
  }
  if (Q * M + p < q.ntaps) {
    // the last row of taps: the phases with Q M + p < ntaps
    const float hk = tp[Q * M];
#pragma unroll
    for (int i = 0; i < NB; i++) {
      const ddc_f2 s = *reinterpret_cast<const ddc_f2*>(col + i * (NT / M) - Q);
      acc[i] = __builtin_elementwise_fma(ddc_f2{hk, hk}, s, acc[i]);
    }
  }

  OUT* out = static_cast<OUT*>(q.out);
  const uint64_t O0 = (uint64_t)blockIdx.x * PFB_TILE;
#pragma unroll
  for (int i = 0; i < NB; i++) {
    const uint64_t o = O0 + (uint64_t)(tid + i * NT);
    if (o >= q.nout) continue;
    c32 y = mk(acc[i].x, acc[i].y);
    if constexpr (ADD) y = cadd(y, q.add[o]);  // read before the store below: `add` may be `out`
    iq_store(out, (int64_t)o, y, q.scale);
  }
}

// (the history kernel is k_stream_hist_rows, stream_hist.h: one row of Q inputs per selected channel)

// host side (engine_pfb_synth.inc): the stream state (StreamStage, host_util.h; hist = K Q) is the bank's own
struct PfbSynthState : StreamStage {
  int M = 2, ntaps = 1, K = 0, Q = 0;
  int out_fmt = OFDM_IQ_FC32;
  float out_scale = 32768.0f;
  signed char pos[PFB_MAX_CHANNELS] = {};  // PfbSynthParams::pos
  DevBuf d_taps, d_w;
  void release() {
    d_taps.release();
    d_w.release();
    StreamStage::release();
  }
};
