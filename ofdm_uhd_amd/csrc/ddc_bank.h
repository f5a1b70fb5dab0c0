// ddc_bank.h -- wideband receive: K links of one capture in one pass (the DDC of ddc.h, K centre frequencies).
//
// Definition (include/ofdm_hip.h): link i is the DDC with (R, h, fc_i), bit for bit -- its table
// c_i, its phase step D_i, the same conversion of the input, the same output set, the same order of the additions
// (tap k = qR + p in chain q mod NG, ascending k inside a chain, chains added in ascending order) and the same unfused
// rotation.  Nothing depends on K, on a link's place in the list, or on where a call, a chunk or a tile starts.
//
// One workgroup produces the T consecutive outputs of k_ddc's tile (same geometry: ddc_geom) for EVERY link.  The
// tile's samples are staged into LDS once, in k_ddc's polyphase layout (row p, odd pitch W: conflict-free tap reads
// and staging stores at any R).  Behind the samples sit the K tables, link-minor: the entries of tap k for links
// l, l + 1 are one aligned 16-byte word, so the wave-uniform broadcast read of a tap serves two links.  The links are
// taken in groups of LG (as many as the accumulators leave registers for); for every tap a thread reads its OPT sample
// words once and issues the 2 LG OPT packed FMAs of the group on them: OPT + LG / 2 LDS reads for 2 LG OPT packed FMAs
// where k_ddc has OPT + 1 for 2 OPT.  With NG > 1 the chains of one link at a time meet in a combine buffer of their
// own behind the tables (the samples must outlive the group).
#pragma once
#include "ddc.h"

#define DDC_BANK_MAX_LINKS 8  // = OFDM_DDC_BANK_MAX_LINKS

struct DdcBankParams {
  DdcParams b;       // k_ddc's parameters; b.tab is the bank's table [ntaps][KP] (link-minor), b.out link 0's run, b.D unused
  uint64_t D[DDC_BANK_MAX_LINKS];  // phase advance per output of each link, 2^-64 turn
  uint64_t stride;   // link i's run begins at b.out + i * stride
  int K, KP;         // links, and K rounded up to even (the pitch of a tap's entries)
};

// links per pass over the staged tile: 4 outputs x 4 links x 4 accumulators, or 1 x 8 x 4
static inline int ddc_bank_group(int R) { return ddc_geom(R).opt == 4 ? 4 : 8; }
static inline size_t ddc_bank_sample_words(int R, int ntaps) {
  const int Q = (ntaps - 1) / R;
  return ((size_t)R * ddc_pitch(ddc_geom(R).T(), Q) + 1) & ~(size_t)1;  // the tables begin on a 16-byte boundary
}
static inline size_t ddc_bank_lds_bytes(int R, int ntaps, int K) {
  const DdcGeom g = ddc_geom(R);
  const int KP = (K + 1) & ~1;
  const size_t combine = g.NG() > 1 ? (size_t)g.NG() * g.T() * 4 * sizeof(float) : 0;
  return (ddc_bank_sample_words(R, ntaps) + (size_t)ntaps * KP) * sizeof(c32) + combine;
}

__device__ __forceinline__ void ddc_bank_finish(const DdcBankParams& q, int l, uint64_t m, ddc_f2 A, ddc_f2 B) {
  const uint64_t o = m - q.b.m0;
  if (o >= q.b.nout) return;
  q.b.out[(uint64_t)l * q.stride + o] = nco_rotate(mk(A.x - B.y, A.y + B.x), 0ull - m * q.D[l]);
}

// links [l0, l0 + LG) of the tile: l0 is even wherever LG > 1
template <int LG, int OPT, int TJ>
__device__ __forceinline__ void ddc_bank_pass(const DdcBankParams& q, const c32* xs, const c32* tap, ddc_f4* cmb, int l0,
                                              uint64_t M0, int tid) {
  constexpr int NT = DDC_THREADS, NG = NT / TJ, T = TJ * OPT;
  const int R = q.b.R, W = q.b.W, Q = q.b.Q, KP = q.KP;
  const int tj = tid % TJ;
  const int g = __builtin_amdgcn_readfirstlane(tid / TJ);  // a wave lies in one chain: tap reads are broadcasts
  ddc_f2 A[LG][OPT], B[LG][OPT];
#pragma unroll
  for (int l = 0; l < LG; l++)
#pragma unroll
    for (int i = 0; i < OPT; i++) A[l][i] = B[l][i] = ddc_f2{0.f, 0.f};
  for (int qq = g; qq <= Q; qq += NG) {
    const int k0 = qq * R;
    const int np = min(R, q.b.ntaps - k0);
    const c32* col = xs + (tj + Q - qq);
    const c32* tp = tap + (size_t)k0 * KP + l0;
    for (int p = 0; p < np; p++) {
      ddc_f2 s[OPT];
#pragma unroll
      for (int i = 0; i < OPT; i++) s[i] = *reinterpret_cast<const ddc_f2*>(col + p * W + i * TJ);
      c32 c[LG];
      if constexpr (LG == 1) {
        c[0] = tp[p * KP];
      } else {
#pragma unroll
        for (int l = 0; l < LG; l += 2) {
          const ddc_f4 cc = *reinterpret_cast<const ddc_f4*>(tp + p * KP + l);
          c[l] = mk(cc.x, cc.y);
          c[l + 1] = mk(cc.z, cc.w);
        }
      }
#pragma unroll
      for (int l = 0; l < LG; l++) {
        const ddc_f2 cr = {c[l].re, c[l].re}, ci = {c[l].im, c[l].im};
#pragma unroll
        for (int i = 0; i < OPT; i++) {
          A[l][i] = __builtin_elementwise_fma(cr, s[i], A[l][i]);
          B[l][i] = __builtin_elementwise_fma(ci, s[i], B[l][i]);
        }
      }
    }
  }

  if constexpr (NG == 1) {
#pragma unroll
    for (int l = 0; l < LG; l++)
#pragma unroll
      for (int i = 0; i < OPT; i++) ddc_bank_finish(q, l0 + l, M0 + (uint64_t)(tj + i * TJ), A[l][i], B[l][i]);
  } else {
    // the chains of an output, added in ascending chain order, one link at a time
#pragma unroll
    for (int l = 0; l < LG; l++) {
      __syncthreads();  // the link before has been read
#pragma unroll
      for (int i = 0; i < OPT; i++) cmb[g * T + tj + i * TJ] = ddc_f4{A[l][i].x, A[l][i].y, B[l][i].x, B[l][i].y};
      __syncthreads();
      for (int j = tid; j < T; j += NT) {
        ddc_f4 s = cmb[j];
#pragma unroll
        for (int c = 1; c < NG; c++) s = s + cmb[c * T + j];
        ddc_bank_finish(q, l0 + l, M0 + (uint64_t)j, ddc_f2{s.x, s.y}, ddc_f2{s.z, s.w});
      }
    }
  }
}

template <typename XT, int OPT, int TJ>
__global__ void __launch_bounds__(DDC_THREADS) k_ddc_bank(DdcBankParams q) {
  constexpr int NT = DDC_THREADS, T = TJ * OPT, MAXLG = OPT == 4 ? 4 : 8;
  extern __shared__ __align__(16) unsigned char ddc_bank_lds[];
  const int tid = threadIdx.x;
  const int R = q.b.R, Q = q.b.Q, H = q.b.ntaps - 1, K = q.K;
  c32* xs = reinterpret_cast<c32*>(ddc_bank_lds);
  c32* tap = xs + (((size_t)R * q.b.W + 1) & ~(size_t)1);
  ddc_f4* cmb = reinterpret_cast<ddc_f4*>(tap + (size_t)q.b.ntaps * q.KP);
  const XT* x = static_cast<const XT*>(q.b.x);
  const uint64_t M0 = q.b.m0 + (uint64_t)blockIdx.x * T;
  // the tile's first staged sample, relative to x[0]: (M0 - Q) R - (R - 1) - a
  const int64_t g0 = (int64_t)(M0 * (uint64_t)R - q.b.a) - (int64_t)Q * R - (R - 1);
  const int total = (T + Q) * R;

  {
    // ntaps KP is even: the tables move as 16-byte words
    const ddc_f4* src = reinterpret_cast<const ddc_f4*>(q.b.tab);
    ddc_f4* dst = reinterpret_cast<ddc_f4*>(tap);
    const int nw = q.b.ntaps * q.KP / 2;
    for (int k = tid; k < nw; k += NT) dst[k] = src[k];
  }
  if (g0 >= 1 && g0 + total + 1 <= (int64_t)q.b.nin) {
    // interior tile: every sample comes from x, no per-sample test against the stream
    if constexpr (std::is_same<XT, c32>::value) {
      // 16 bytes per lane, on the 16-byte grid of the caller's buffer (the pair may begin one sample before the tile)
      const int e = (int)((((uintptr_t)x >> 3) + (uint64_t)g0) & 1u);
      for (int u = 2 * tid - e; u < total; u += 2 * NT) {
        const ddc_f4 v = *reinterpret_cast<const ddc_f4*>(x + (g0 + u));
        if (u >= 0) ddc_put(xs, q.b.magic, q.b.R, q.b.W, u, mk(v.x, v.y));
        if (u + 1 < total) ddc_put(xs, q.b.magic, q.b.R, q.b.W, u + 1, mk(v.z, v.w));
      }
    } else {
      for (int u = tid; u < total; u += NT) ddc_put(xs, q.b.magic, q.b.R, q.b.W, u, iq_load(x, g0 + u, q.b.scale));
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
      ddc_put(xs, q.b.magic, q.b.R, q.b.W, u, v);
    }
  }
  __syncthreads();

  // the links in groups: MAXLG at a time, then what is left in groups of 4, 2, 1 (each group begins at an even link)
  int l0 = 0;
  for (; l0 + MAXLG <= K; l0 += MAXLG) ddc_bank_pass<MAXLG, OPT, TJ>(q, xs, tap, cmb, l0, M0, tid);
  if constexpr (MAXLG == 8) {
    if (K - l0 >= 4) {
      ddc_bank_pass<4, OPT, TJ>(q, xs, tap, cmb, l0, M0, tid);
      l0 += 4;
    }
  }
  if (K - l0 >= 2) {
    ddc_bank_pass<2, OPT, TJ>(q, xs, tap, cmb, l0, M0, tid);
    l0 += 2;
  }
  if (K - l0 >= 1) ddc_bank_pass<1, OPT, TJ>(q, xs, tap, cmb, l0, M0, tid);
}

// host side (engine_ddc_bank.inc): the stream state (StreamStage, host_util.h) is the bank's own, shared by its links
struct DdcBankState : StreamStage {
  int R = 1, ntaps = 1, K = 0;
  double fc[DDC_BANK_MAX_LINKS] = {};
  uint64_t D[DDC_BANK_MAX_LINKS] = {};
  std::vector<c32> tab;    // link i's table at tab[i * ntaps], as ofdm_ddc_bank_taps returns it
  DevBuf d_tab;
  void release() {
    d_tab.release();
    StreamStage::release();
  }
};
