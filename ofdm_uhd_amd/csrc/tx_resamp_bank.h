// tx_resamp_bank.h -- wideband transmit at a rate that is no integer multiple of the modem's: K links at arbitrary
// centre frequencies onto one band in one pass through a rational-rate (L / M) resampler (the transmit counterpart of
// resamp_bank.h; what K passes of tx_resamp.h with `add` did before).
//
// Definition (include/ofdm_hip.h), output n at position n M on the L-times grid:
//   i_n = floor(n M / L), p = p_n = n M mod L
//   G_i = turns(fc_i / M), E_i = L G_i mod 2^64 (per input), D_i = M G_i mod 2^64 (per output)
//   xr_i[m] = x_i[m] r_i[m]           r_i[m] = complex64(expj(+2 pi (m E_i mod 2^64) / 2^64))
//   A = fma(re c_i[p + q L], xr_i[i_n - q], A),  B = fma(im c_i[p + q L], xr_i[i_n - q], B)
//                                      ONE chain each of packed FMAs on (re, im), begun at +0: links in ascending i,
//                                      inside a link ascending q while p + q L < ntaps
//   v[n] = (A.re - B.im, A.im + B.re),  out[n] = store(v[n] + add[n]) or store(v[n])
// c_i[k] = complex64(h[k] exp(j 2 pi fc_i k / M)).  The shift sits on the INPUT side: n M = (p + q L) + (i_n - q) L, so
// k G_i + m E_i = n D_i modulo 2^64 without rounding -- one float64 phasor per staged input sample and link (M / L per
// output) where K passes of k_tx_resamp evaluate one per output and pass.
//
// The tile is k_tx_resamp's (tx_resamp_geom: TJ periods per workgroup; M staged rows of odd pitch W; the sums leave
// through LDS in output order).  The links take turns, as in k_duc_bank, in ONE LDS region -- link i's table (ntaps
// words of 8 bytes) and the tile's samples of link i, rotated while they are staged -- between two barriers each.  The
// rotation is a function of the absolute input index, so the history is rotated again by every tile and the carried
// state stays the RAW inputs.  A and B of every output of the tile live in a 16-byte LDS cell ([r][period], odd pitch
// TP), read and written by the one thread that owns the output under every link: no barrier guards them, and the first
// link begins them at +0 without a read.
// A work item is (newest input `off` of the period, slot, 64 periods): the outputs r of a period with
// floor(r M / L) = off read the same samples, so up to TX_RESAMP_BANK_GROUP = 4 consecutive ones share every sample
// read (one 8-byte read for 2 x 4 packed FMAs where L >= 4 M; one output per item where L <= M).  Every index but the
// period is wave-uniform.  LDS reads in the tap loop, per wave:
//   x:    consecutive 8-byte words (lane = period, the row is wave-uniform): conflict-free at every (L, M);
//   tap:  one 8-byte word per output of the group for the whole wave (p is wave-uniform): broadcasts;
//   cell: consecutive 16-byte words, once per link: conflict-free.
// In the output pass consecutive lanes read cells TP apart (TP odd: 4 TP banks apart, the 16 lanes a ds_read_b128 serves
// together cover the 64 banks once) except where a wave crosses a period.  The order of the additions of an output is
// the definition's whatever the grouping.
#pragma once
#include "tx_resamp.h"

#define TX_RESAMP_BANK_MAX_LINKS 8  // = OFDM_TX_RESAMP_BANK_MAX_LINKS
constexpr size_t TX_RESAMP_BANK_MAX_LDS = 160 * 1024;
constexpr int TX_RESAMP_BANK_GROUP = 4;  // outputs of a period that share their sample reads, at most

struct TxResampBankParams {
  const c32* x;     // link i's inputs of this call begin at x + i * stride; x[0] is input index a
  const c32* hist;  // link i's Q raw inputs before x[0] begin at hist + i * Q (zeros before the stream start)
  const c32* tab;   // link i's table c_i at tab + i * ntaps
  const c32* add;   // nout samples, or unused (ADD = false); may be `out` itself
  void* out;        // out[0] is output n0
  uint64_t nin, stride, a, n0, nout;
  uint64_t J0;      // period of the first tile: n0 / L
  uint64_t E[TX_RESAMP_BANK_MAX_LINKS];  // phase advance per INPUT of each link, 2^-64 turn
  uint64_t magicM;  // floor(2^32 / M) + 1: u / M = (u * magicM) >> 32 for every u of a tile
  uint64_t magicL;  // the same for L
  int L, M, ntaps, Q, QM, W, TP, KC, K;
  float scale;      // sc16 output: full scale
};

// LDS: one link's table, its M staged rows (an even count of words: the cells stay 16-byte aligned), a cell per output
static inline size_t tx_resamp_bank_lds_bytes(int L, int M, int ntaps) {
  const TxResampGeom g = tx_resamp_geom(L, M);
  const int QM = resamp_hist_periods((ntaps - 1) / L, M);
  const size_t tab = (size_t)((ntaps + 1) & ~1);
  const size_t rows = ((size_t)M * resamp_pitch(g.TJ(), QM) + 1) & ~(size_t)1;
  const size_t cells = (size_t)L * (g.TJ() | 1);
  return (tab + rows + 2 * cells) * sizeof(c32);
}

// NG consecutive outputs of one period that share their newest input (phases p0, p0 + M, ... < L), one link: the
// chains of each continue from its cell (or begin at +0 under the first link) in ascending q.  Every sample is read
// once for the group.  The phases differ by less than L, so their tap counts differ by at most one: nqmin rows that
// every output has run without a test, the row behind them under one.
template <int NG>
__device__ __forceinline__ void tx_resamp_bank_group(const c32* tap, const c32* xp, ddc_f4* cell, int TP, bool first, int L, int M, int W,
                                                     int ntaps, int p0, int row) {
  ddc_f2 A[NG], B[NG];
#pragma unroll
  for (int g = 0; g < NG; g++) {
    A[g] = B[g] = ddc_f2{0.f, 0.f};
    if (!first) {
      const ddc_f4 c = cell[g * TP];
      A[g] = ddc_f2{c.x, c.y};
      B[g] = ddc_f2{c.z, c.w};
    }
  }
  const int pl = p0 + (NG - 1) * M;
  const int nqmin = pl < ntaps ? (ntaps - 1 - pl) / L + 1 : 0;
  const c32* tp = tap + p0;
  for (int qq = 0; qq < nqmin; qq++) {
    const ddc_f2 s = *reinterpret_cast<const ddc_f2*>(xp);
#pragma unroll
    for (int g = 0; g < NG; g++) {
      const c32 c = tp[g * M];
      A[g] = __builtin_elementwise_fma(ddc_f2{c.re, c.re}, s, A[g]);
      B[g] = __builtin_elementwise_fma(ddc_f2{c.im, c.im}, s, B[g]);
    }
    tp += L;
    if (--row < 0) {  // the row before row 0 is row M - 1 of the column before
      row += M;
      xp += M * W - 1;
    }
    xp -= W;
  }
  const int rem = ntaps - p0 - nqmin * L;  // the phases below it have one more tap
  if (rem > 0) {
    const ddc_f2 s = *reinterpret_cast<const ddc_f2*>(xp);
#pragma unroll
    for (int g = 0; g < NG; g++) {
      if (g * M < rem) {
        const c32 c = tp[g * M];
        A[g] = __builtin_elementwise_fma(ddc_f2{c.re, c.re}, s, A[g]);
        B[g] = __builtin_elementwise_fma(ddc_f2{c.im, c.im}, s, B[g]);
      }
    }
  }
#pragma unroll
  for (int g = 0; g < NG; g++) cell[g * TP] = ddc_f4{A[g].x, A[g].y, B[g].x, B[g].y};
}

template <typename OUT, bool ADD>
__global__ void __launch_bounds__(TX_RESAMP_THREADS) k_tx_resamp_bank(TxResampBankParams q) {
  constexpr int NT = TX_RESAMP_THREADS, NW = NT / WAVE;
  extern __shared__ __align__(16) unsigned char tx_resamp_bank_lds[];
  c32* tap = reinterpret_cast<c32*>(tx_resamp_bank_lds);
  c32* xs = tap + ((q.ntaps + 1) & ~1);
  ddc_f4* acc = reinterpret_cast<ddc_f4*>(xs + ((q.M * q.W + 1) & ~1));
  const int tid = threadIdx.x;
  const int L = q.L, M = q.M, W = q.W, Q = q.Q, QM = q.QM, TJ = q.KC * WAVE, TO = TJ * L;
  const uint64_t J0 = q.J0 + (uint64_t)blockIdx.x * (uint64_t)TJ;
  // the tile's first staged sample: its absolute index (wraps below 0 only where the sample is a zero) and its index
  // relative to x[0]
  const uint64_t m0 = (J0 - (uint64_t)QM) * (uint64_t)M;
  const int64_t g0 = ((int64_t)J0 - QM) * M - (int64_t)q.a;
  const int total = (TJ + QM) * M;
  const bool interior = g0 >= 0 && g0 + total <= (int64_t)q.nin;
  const int lane = tid & (WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
  const int slots = ((L + M - 1) / M + TX_RESAMP_BANK_GROUP - 1) / TX_RESAMP_BANK_GROUP;  // groups per newest input
  const int nwork = M * slots * q.KC;

  for (int l = 0; l < q.K; l++) {
    if (l) __syncthreads();  // the link before has been read
    const c32* tab = q.tab + (size_t)l * q.ntaps;
    const c32* x = q.x + (uint64_t)l * q.stride;
    const uint64_t E = q.E[l];
    for (int k = tid; k < q.ntaps; k += NT) tap[k] = tab[k];
    if (interior) {
      // interior tile: every sample comes from x, no per-sample test against the stream
      for (int u = tid; u < total; u += NT) polyphase_put(xs, q.magicM, M, W, u, nco_rotate(x[g0 + u], (m0 + (uint64_t)u) * E));
    } else {
      // first and last tiles: the carried history (zeros at the stream start) before x[0], zeros behind the call's end
      // (those feed only outputs the call does not have) and before the oldest sample the history holds
      const c32* hist = q.hist + (int64_t)l * Q;
      for (int u = tid; u < total; u += NT) {
        const int64_t gi = g0 + u;
        c32 v = mk(0.f, 0.f);
        if (gi >= 0) {
          if (gi < (int64_t)q.nin) v = x[gi];
        } else if (gi + Q >= 0) {
          v = hist[gi + Q];
        }
        polyphase_put(xs, q.magicM, M, W, u, nco_rotate(v, (m0 + (uint64_t)u) * E));
      }
    }
    __syncthreads();

    // work item = (newest input `off` of the period, slot, 64 periods); a wave takes every NW-th one, the same ones
    // under every link.  The outputs r of a period with floor(r M / L) = off read the same samples: up to
    // TX_RESAMP_BANK_GROUP of them, consecutive, share every sample read
    for (int wi = wave; wi < nwork; wi += NW) {
      const int unit = wi / q.KC;
      const int t = (wi - unit * q.KC) * WAVE + lane;
      const int off = unit / slots, slot = unit - off * slots;
      const int rb = (off * L + M - 1) / M + slot * TX_RESAMP_BANK_GROUP;   // the first r of the group
      const int re = min(((off + 1) * L + M - 1) / M, L);                  // one past the last r with this `off`
      const int ng = min(re - rb, TX_RESAMP_BANK_GROUP);
      if (ng <= 0) continue;
      // sample i - qq of period t: row (off - qq) mod M, column t + QM + floor((off - qq) / M)
      const c32* xp = xs + (off * W + QM + t);
      const int p0 = rb * M - off * L;
      ddc_f4* cell = acc + (rb * q.TP + t);
      switch (ng) {
        case 1: tx_resamp_bank_group<1>(tap, xp, cell, q.TP, l == 0, L, M, W, q.ntaps, p0, off); break;
        case 2: tx_resamp_bank_group<2>(tap, xp, cell, q.TP, l == 0, L, M, W, q.ntaps, p0, off); break;
        case 3: tx_resamp_bank_group<3>(tap, xp, cell, q.TP, l == 0, L, M, W, q.ntaps, p0, off); break;
        default: tx_resamp_bank_group<4>(tap, xp, cell, q.TP, l == 0, L, M, W, q.ntaps, p0, off); break;
      }
    }
  }
  __syncthreads();

  // in output order: the two chains combined, the band that is there, one contiguous store
  OUT* out = static_cast<OUT*>(q.out);
  for (int j = tid; j < TO; j += NT) {
    const uint64_t n = J0 * (uint64_t)L + (uint64_t)j;
    const uint64_t o = n - q.n0;  // (outputs before n0 wrap to huge values)
    if (o >= q.nout) continue;
    const int t = (int)(((uint64_t)(uint32_t)j * q.magicL) >> 32);
    const ddc_f4 s = acc[(j - t * L) * q.TP + t];
    c32 y = mk(s.x - s.w, s.y + s.z);
    if constexpr (ADD) y = cadd(y, q.add[o]);  // read before the store below: `add` may be `out`
    iq_store(out, (int64_t)o, y, q.scale);
  }
}

// (the history kernel is k_stream_hist_rows, stream_hist.h, with H = Q: the last Q RAW inputs of every link)

// host side (engine_tx_resamp_bank.inc): the stream state (StreamStage, host_util.h; hist = K Q) is the bank's own
struct TxResampBankState : StreamStage {
  int L = 1, M = 1, ntaps = 1, K = 0, Q = 0;
  int out_fmt = OFDM_IQ_FC32;
  float out_scale = 32768.0f;
  uint64_t E[TX_RESAMP_BANK_MAX_LINKS] = {};
  std::vector<c32> tab;  // link i's table at tab[i * ntaps], as ofdm_tx_resamp_bank_taps returns it
  DevBuf d_tab;
  void release() {
    d_tab.release();
    StreamStage::release();
  }
};
