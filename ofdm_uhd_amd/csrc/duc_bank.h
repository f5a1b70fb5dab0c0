// duc_bank.h -- wideband transmit: K links at arbitrary centre frequencies onto one band in one pass (the transmit
// counterpart of ddc_bank.h; the two-channel transmitter of dual_channel/dual_channel.py, one sink.set_interp +
// set_center_freq per link, usrp_transmit_path.py:79-88).
//
// Definition (include/ofdm_hip.h), output n = m L + p, p in [0, L), tap k = p + q L:
//   xr_i[m] = x_i[m] r_i[m]           r_i[m] = complex64(expj(+2 pi (m E_i mod 2^64) / 2^64)), E_i = L D_i mod 2^64
//   A = fma(re c_i[p + q L], xr_i[m - q], A),  B = fma(im c_i[p + q L], xr_i[m - q], B)
//                                      ONE chain each of packed FMAs on (re, im), begun at +0: links in ascending i,
//                                      inside a link ascending q
//   v[n] = (A.re - B.im, A.im + B.re),  out[n] = store(v[n] + add[n]) or store(v[n])
// The shift sits on the INPUT side (h[k] x[m - q] e^{j 2 pi fc n} = (h[k] e^{j 2 pi fc k}) (x[m - q] e^{j 2 pi fc L (m - q)})):
// one float64 phasor per staged input sample and link where K passes of k_duc evaluate one per output and pass.
//
// One workgroup produces k_duc's tile, T = 256 * OPT consecutive outputs (duc_geom), thread t owning outputs t,
// t + 256, ...: consecutive lanes own consecutive outputs, so every global store and `add` load of a wave is one
// contiguous run.  The accumulators of the tile stay in registers over all links.  The links take turns in ONE LDS
// region -- link i's table c_i (ntaps words of 8 bytes) and the tile's samples of link i, rotated while they are staged
// (duc_staged words) -- between two barriers each: at most (1024 + 1023 + 2048) * 8 = 32760 bytes whatever K.  The
// rotation is a function of the absolute input index, so the history samples are rotated again by every tile and the
// state stays the raw inputs.  In the tap loop a 32-lane group reads
//   x:   consecutive 8-byte words, L lanes on each (broadcast), as in k_duc;
//   tap: the 8-byte words c[p + q L], p = n mod L: min(L, 32) distinct consecutive words, one bank pair each
// (ds_read_b64 banks (a / 4) mod 64 over 32-lane groups): conflict-free for L <= 32 and L = 64; for 32 < L < 64 the
// tap row wraps inside the group as k_duc's does.  The rows of taps that every phase has run without a per-output
// test; where L divides 256 a thread's outputs share their phase and one tap read serves all of them (OPT + 1 LDS
// reads for 2 OPT packed FMAs); the order of the additions is the same on both paths.
#pragma once
#include "duc.h"
#include "stream_hist.h"

#define DUC_BANK_MAX_LINKS 8  // = OFDM_DUC_BANK_MAX_LINKS

struct DucBankParams {
  const c32* x;     // link i's inputs of this call begin at x + i * stride; x[0] is input index a
  const c32* hist;  // link i's Q raw inputs before x[0] begin at hist + i * Q (zeros before the stream start)
  const c32* tab;   // link i's table c_i at tab + i * ntaps
  const c32* add;   // nin L samples, or unused (ADD = false); may be `out` itself
  void* out;        // out[0] is output a L
  uint64_t nin, stride, a, nout;
  uint64_t E[DUC_BANK_MAX_LINKS];  // phase advance per INPUT of each link, 2^-64 turn
  uint64_t magic;   // floor(2^32 / L) + 1: u / L = (u * magic) >> 32 for every u of a tile
  int L, ntaps, Q, K;
  float scale;      // sc16 output: full scale
};

// one link at a time: its table and its staged samples (k_duc's tile, k_duc's count)
static inline size_t duc_bank_lds_bytes(int L, int ntaps) {
  const int Q = (ntaps - 1) / L;
  return ((size_t)ntaps + (size_t)duc_staged(duc_geom(L).T(), L, Q)) * sizeof(c32);
}

template <typename OUT, bool ADD, int OPT>
__global__ void __launch_bounds__(DUC_THREADS) k_duc_bank(DucBankParams q) {
  constexpr int NT = DUC_THREADS, T = NT * OPT;
  extern __shared__ __align__(16) unsigned char duc_bank_lds[];
  c32* tap = reinterpret_cast<c32*>(duc_bank_lds);
  c32* xs = tap + q.ntaps;
  const int tid = threadIdx.x;
  const int L = q.L, Q = q.Q;
  // the tile's first output is a L + off: input mb = a + off / L, phase r0 = off % L
  const uint64_t off = (uint64_t)blockIdx.x * T;
  const uint64_t dq = off / (uint64_t)L;
  const int r0 = (int)(off - dq * (uint64_t)L);
  const int64_t g0 = (int64_t)dq - Q;       // the first staged sample, relative to x[0]
  const uint64_t m0 = q.a + (uint64_t)g0;   // its absolute index (wraps below 0 only where the sample is a zero)
  const int total = Q + (r0 + T + L - 1) / L;
  const bool interior = g0 >= 0 && g0 + total <= (int64_t)q.nin;

  // rows of taps every phase has (q < Qf), and the phases of the row behind them (q = Qf = Q, where ntaps is no
  // multiple of L): the tap loop runs without a per-output test, the last row under one
  const int Qf = q.ntaps / L, rem = q.ntaps - Qf * L;
  // L divides 256: the outputs t, t + 256, ... of a thread share their phase, and one tap read serves them all
  const bool samep = (NT % L) == 0;
  ddc_f2 A[OPT], B[OPT];
  const c32* col[OPT];
  int ph[OPT];
#pragma unroll
  for (int i = 0; i < OPT; i++) {
    const int u = r0 + tid + i * NT;
    const int dm = (int)(((uint64_t)(uint32_t)u * q.magic) >> 32);
    A[i] = B[i] = ddc_f2{0.f, 0.f};
    col[i] = xs + (Q + dm);
    ph[i] = u - dm * L;
  }

  for (int l = 0; l < q.K; l++) {
    if (l) __syncthreads();  // the link before has been read
    const c32* tab = q.tab + (size_t)l * q.ntaps;
    const c32* x = q.x + (uint64_t)l * q.stride;
    const uint64_t E = q.E[l];
    for (int k = tid; k < q.ntaps; k += NT) tap[k] = tab[k];
    if (interior) {
      // interior tile: every sample comes from x, no per-sample test against the stream
      for (int u = tid; u < total; u += NT) xs[u] = nco_rotate(x[g0 + u], (m0 + (uint64_t)u) * E);
    } else {
      // first and last tiles: the carried history (zeros at the stream start) before x[0]; zeros behind the call's end
      // (they feed only outputs the call does not have) and before the oldest sample the history holds
      const c32* hist = q.hist + (int64_t)l * Q;
      for (int u = tid; u < total; u += NT) {
        const int64_t gi = g0 + u;
        c32 v = mk(0.f, 0.f);
        if (gi >= 0) {
          if (gi < (int64_t)q.nin) v = x[gi];
        } else if (gi + Q >= 0) {
          v = hist[gi + Q];
        }
        xs[u] = nco_rotate(v, (m0 + (uint64_t)u) * E);
      }
    }
    __syncthreads();

    if (samep) {
      const c32* tp = tap + ph[0];
      for (int qq = 0; qq < Qf; qq++) {
        const c32 c = tp[qq * L];
        const ddc_f2 cr = {c.re, c.re}, ci = {c.im, c.im};
#pragma unroll
        for (int i = 0; i < OPT; i++) {
          const ddc_f2 s = *reinterpret_cast<const ddc_f2*>(col[i] - qq);
          A[i] = __builtin_elementwise_fma(cr, s, A[i]);
          B[i] = __builtin_elementwise_fma(ci, s, B[i]);
        }
      }
      if (ph[0] < rem) {
        const c32 c = tp[Qf * L];
        const ddc_f2 cr = {c.re, c.re}, ci = {c.im, c.im};
#pragma unroll
        for (int i = 0; i < OPT; i++) {
          const ddc_f2 s = *reinterpret_cast<const ddc_f2*>(col[i] - Qf);
          A[i] = __builtin_elementwise_fma(cr, s, A[i]);
          B[i] = __builtin_elementwise_fma(ci, s, B[i]);
        }
      }
    } else {
      for (int qq = 0; qq < Qf; qq++) {
#pragma unroll
        for (int i = 0; i < OPT; i++) {
          const c32 c = tap[ph[i] + qq * L];
          const ddc_f2 s = *reinterpret_cast<const ddc_f2*>(col[i] - qq);
          A[i] = __builtin_elementwise_fma(ddc_f2{c.re, c.re}, s, A[i]);
          B[i] = __builtin_elementwise_fma(ddc_f2{c.im, c.im}, s, B[i]);
        }
      }
#pragma unroll
      for (int i = 0; i < OPT; i++) {
        if (ph[i] < rem) {
          const c32 c = tap[ph[i] + Qf * L];
          const ddc_f2 s = *reinterpret_cast<const ddc_f2*>(col[i] - Qf);
          A[i] = __builtin_elementwise_fma(ddc_f2{c.re, c.re}, s, A[i]);
          B[i] = __builtin_elementwise_fma(ddc_f2{c.im, c.im}, s, B[i]);
        }
      }
    }
  }

  OUT* out = static_cast<OUT*>(q.out);
#pragma unroll
  for (int i = 0; i < OPT; i++) {
    const uint64_t o = off + (uint64_t)(tid + i * NT);
    if (o >= q.nout) continue;
    c32 y = mk(A[i].x - B[i].y, A[i].y + B[i].x);
    if constexpr (ADD) y = cadd(y, q.add[o]);  // read before the store below: `add` may be `out`
    iq_store(out, (int64_t)o, y, q.scale);
  }
}

// (the history kernel is k_stream_hist_rows, stream_hist.h, with H = Q: the last Q RAW inputs of every link)

// host side (engine_duc_bank.inc): the stream state (StreamStage, host_util.h; hist = K Q) is the bank's own
struct DucBankState : StreamStage {
  int L = 1, ntaps = 1, K = 0, Q = 0;
  int out_fmt = OFDM_IQ_FC32;
  float out_scale = 32768.0f;
  uint64_t E[DUC_BANK_MAX_LINKS] = {};
  std::vector<c32> tab;  // link i's table at tab[i * ntaps], as ofdm_duc_bank_taps returns it
  DevBuf d_tab;
  void release() {
    d_tab.release();
    StreamStage::release();
  }
};
