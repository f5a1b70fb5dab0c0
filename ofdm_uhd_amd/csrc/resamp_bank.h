// resamp_bank.h -- wideband receive: K links of one capture in one pass at a rational rate (the resampler of resamp.h,
// K centre frequencies).
//
// Definition (include/ofdm_hip.h): link i is the resampler with (L, M, h, fc_i), bit for bit -- its
// table c_i, its phase step D_i, the same conversion of the input, the same output set, the same order of the
// additions (tap q in chain q mod NG, ascending q inside a chain, chains added in ascending order, NG = resamp_geom's)
// and the same unfused rotation.  Nothing depends on K, on a link's place in the list, or on where a call, a chunk or a
// tile starts.
//
// One workgroup produces the TJ periods of k_resamp's tile (same geometry: resamp_geom) for EVERY link.  The tile's
// samples are staged into LDS once, in k_resamp's layout (M rows, odd pitch W).  In front of them sit the K tables,
// link-minor: the entries of tap k for links l, l + 1 are one aligned 16-byte word, so the wave-uniform broadcast read
// of a tap serves two links.  A work item is k_resamp's (phase class r, 64 periods, chain g); the links are taken in
// groups of LG: per tap a lane reads its sample word once, the wave reads LG / 2 tap words and issues 2 LG packed FMAs,
// where k_resamp has one sample word and one tap word for 2.  The sums of a group leave through LDS in output order,
// link by link: every global store of a wave is one contiguous run.  The sum buffer holds NB links (the host's choice,
// resamp_bank_sum_links: what the LDS budget leaves); a group is never larger than NB, and at the largest shape
// (L = M = 64, 1024 taps, K = 8: 132 096 bytes with NB = 1) the links go through it one at a time.
#pragma once
#include "resamp.h"

#define RESAMP_BANK_MAX_LINKS 8  // = OFDM_RESAMP_BANK_MAX_LINKS

constexpr size_t RESAMP_BANK_LDS_MAX = 160 * 1024;  // LDS a workgroup may have on gfx950

struct ResampBankParams {
  ResampParams b;    // k_resamp's parameters; b.tab is the bank's table [ntaps][KP] (link-minor), b.out link 0's run, b.D unused
  uint64_t D[RESAMP_BANK_MAX_LINKS];  // phase advance per output of each link, 2^-64 turn
  uint64_t stride;   // link i's run begins at b.out + i * stride
  int K, KP;         // links, and K rounded up to even (the pitch of a tap's entries)
  int NB;            // links the sum buffer holds: 1, 2, 4 or 8
};

// c32 words of one link's sums on their way out (resamp_lds_bytes' last term)
static inline size_t resamp_bank_sum_words(int L, int M) {
  const ResampGeom g = resamp_geom(L, M);
  return g.ng > 1 ? (size_t)g.ng * g.TJ() * L * 2 : (size_t)L * (g.TJ() | 1);
}
static inline size_t resamp_bank_lds_bytes(int L, int M, int ntaps, int K, int NB) {
  const ResampGeom g = resamp_geom(L, M);
  const int KP = (K + 1) & ~1;
  const int QM = resamp_hist_periods((ntaps - 1) / L, M);
  const size_t tab = (size_t)ntaps * KP;  // even: the rows begin on a 16-byte boundary
  const size_t rows = ((size_t)M * resamp_pitch(g.TJ(), QM) + 1) & ~(size_t)1;
  return (tab + rows + (size_t)NB * resamp_bank_sum_words(L, M)) * sizeof(c32);
}
// links per sum buffer: the largest group (8, 4, 2, 1; no more than K) that leaves room for a second workgroup on the CU
// (half the LDS); where not even one link does, the largest that fits the workgroup's whole 160 KB
static inline int resamp_bank_sum_links(int L, int M, int ntaps, int K) {
  for (size_t budget : {RESAMP_BANK_LDS_MAX / 2, RESAMP_BANK_LDS_MAX})
    for (int nb = 8; nb >= 1; nb >>= 1)
      if (nb <= K && resamp_bank_lds_bytes(L, M, ntaps, K, nb) <= budget) return nb;
  return 1;
}

// links [l0, l0 + LG) of the tile: l0 is even wherever LG > 1.  Ends with the sum buffer free for the next group.
template <int LG, int NG>
__device__ __forceinline__ void resamp_bank_pass(const ResampBankParams& q, const c32* xs, const c32* tap, c32* ob, int l0,
                                                 uint64_t J0, int tid) {
  constexpr int NT = RESAMP_THREADS, NW = NT / WAVE;
  const int L = q.b.L, M = q.b.M, W = q.b.W, QM = q.b.QM, KP = q.KP, TP = q.b.TP, TJ = q.b.KC * WAVE, TO = TJ * L;
  const int SL = L * TP;  // NG == 1: one link's sums, [r][period]
  ddc_f4* cmb = reinterpret_cast<ddc_f4*>(ob);  // NG > 1: [link][chain][output] of (A, B)

  // work item = (phase class r, 64 periods, chain g), k_resamp's; a wave takes every NW-th one
  const int lane = tid & (WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
  const int nwork = L * q.b.KC * NG;
  for (int wi = wave; wi < nwork; wi += NW) {
    const int g = wi % NG, unit = wi / NG;
    const int r = unit / q.b.KC;
    const int t = (unit - r * q.b.KC) * WAVE + lane;
    const int rm = r * M, off = rm / L, p = rm - off * L;
    const int nq = p < q.b.ntaps ? (q.b.ntaps - 1 - p) / L + 1 : 0;
    int row = off - g, col = QM;
    while (row < 0) {
      row += M;
      col--;
    }
    ddc_f2 A[LG], B[LG];
#pragma unroll
    for (int l = 0; l < LG; l++) A[l] = B[l] = ddc_f2{0.f, 0.f};
    for (int qq = g; qq < nq; qq += NG) {
      const c32* tp = tap + (size_t)(p + qq * L) * KP + l0;
      const ddc_f2 s = *reinterpret_cast<const ddc_f2*>(xs + (row * W + col + t));
      c32 c[LG];
      if constexpr (LG == 1) {
        c[0] = tp[0];
      } else {
#pragma unroll
        for (int l = 0; l < LG; l += 2) {
          const ddc_f4 cc = *reinterpret_cast<const ddc_f4*>(tp + l);
          c[l] = mk(cc.x, cc.y);
          c[l + 1] = mk(cc.z, cc.w);
        }
      }
#pragma unroll
      for (int l = 0; l < LG; l++) {
        A[l] = __builtin_elementwise_fma(ddc_f2{c[l].re, c[l].re}, s, A[l]);
        B[l] = __builtin_elementwise_fma(ddc_f2{c[l].im, c[l].im}, s, B[l]);
      }
      row -= NG;
      while (row < 0) {
        row += M;
        col--;
      }
    }
#pragma unroll
    for (int l = 0; l < LG; l++) {
      if constexpr (NG == 1) ob[l * SL + r * TP + t] = mk(A[l].x - B[l].y, A[l].y + B[l].x);
      else cmb[(l * NG + g) * TO + t * L + r] = ddc_f4{A[l].x, A[l].y, B[l].x, B[l].y};
    }
  }
  __syncthreads();

  // in output order, link by link: the chains of an output added in ascending chain order, the rotation, one
  // contiguous store per wave and link
  for (int j = tid; j < TO; j += NT) {
    const uint64_t n = J0 * (uint64_t)L + (uint64_t)j;
    const uint64_t o = n - q.b.n0;  // (outputs before n0 wrap to huge values)
    if (o >= q.b.nout) continue;
    const int t = (int)(((uint64_t)(uint32_t)j * q.b.magicL) >> 32);
    const int at = (j - t * L) * TP + t;
#pragma unroll
    for (int l = 0; l < LG; l++) {
      c32 v;
      if constexpr (NG == 1) {
        v = ob[l * SL + at];
      } else {
        const ddc_f4* cl = cmb + (l * NG) * TO;
        ddc_f4 s = cl[j];
#pragma unroll
        for (int c = 1; c < NG; c++) s = s + cl[c * TO + j];
        v = mk(s.x - s.w, s.y + s.z);
      }
      q.b.out[(uint64_t)(l0 + l) * q.stride + o] = nco_rotate(v, 0ull - n * q.D[l0 + l]);
    }
  }
  if (l0 + LG < q.K) __syncthreads();  // the next group writes the buffer
}

template <typename XT, int NG>
__global__ void __launch_bounds__(RESAMP_THREADS) k_resamp_bank(ResampBankParams q) {
  constexpr int NT = RESAMP_THREADS;
  extern __shared__ __align__(16) unsigned char resamp_bank_lds[];
  c32* tap = reinterpret_cast<c32*>(resamp_bank_lds);
  c32* xs = tap + (size_t)q.b.ntaps * q.KP;
  c32* ob = xs + ((q.b.M * q.b.W + 1) & ~1);
  const int tid = threadIdx.x;
  const int M = q.b.M, Q = q.b.Q, QM = q.b.QM, TJ = q.b.KC * WAVE, K = q.K;
  const XT* x = static_cast<const XT*>(q.b.x);
  const uint64_t J0 = q.b.J0 + (uint64_t)blockIdx.x * (uint64_t)TJ;
  // the tile's first staged sample, relative to x[0]: (J0 - QM) M - a
  const int64_t g0 = ((int64_t)J0 - QM) * M - (int64_t)q.b.a;
  const int total = (TJ + QM) * M;

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
        if (u >= 0) polyphase_put(xs, q.b.magicM, q.b.M, q.b.W, u, mk(v.x, v.y));
        if (u + 1 < total) polyphase_put(xs, q.b.magicM, q.b.M, q.b.W, u + 1, mk(v.z, v.w));
      }
    } else {
      for (int u = tid; u < total; u += NT) polyphase_put(xs, q.b.magicM, q.b.M, q.b.W, u, iq_load(x, g0 + u, q.b.scale));
    }
  } else {
    // first and last tiles: the carried history (zeros at the stream start) before x[0], zeros behind the call's end
    // (those feed only outputs the call does not have) and before the oldest sample the history holds
    for (int u = tid; u < total; u += NT) {
      const int64_t gi = g0 + u;
      c32 v = mk(0.f, 0.f);
      if (gi >= 0) {
        if (gi < (int64_t)q.b.nin) v = iq_load(x, gi, q.b.scale);
      } else if (gi + Q >= 0) {
        v = q.b.hist[gi + Q];
      }
      polyphase_put(xs, q.b.magicM, q.b.M, q.b.W, u, v);
    }
  }
  __syncthreads();

  // the links in groups of 8, 4, 2, 1: the largest that the links left and the sum buffer allow (a group of more than
  // one begins at an even link: K - l0 and NB decide, and NB is a power of two)
  for (int l0 = 0; l0 < K;) {
    const int cap = min(K - l0, q.NB);
    if (cap >= 8) {
      resamp_bank_pass<8, NG>(q, xs, tap, ob, l0, J0, tid);
      l0 += 8;
    } else if (cap >= 4) {
      resamp_bank_pass<4, NG>(q, xs, tap, ob, l0, J0, tid);
      l0 += 4;
    } else if (cap >= 2) {
      resamp_bank_pass<2, NG>(q, xs, tap, ob, l0, J0, tid);
      l0 += 2;
    } else {
      resamp_bank_pass<1, NG>(q, xs, tap, ob, l0, J0, tid);
      l0 += 1;
    }
  }
}

// host side (engine_resamp_bank.inc): the stream state (StreamStage, host_util.h; hist = Q) is the bank's own, shared
// by its links
struct ResampBankState : StreamStage {
  int L = 1, M = 1, ntaps = 1, K = 0;
  double fc[RESAMP_BANK_MAX_LINKS] = {};
  uint64_t D[RESAMP_BANK_MAX_LINKS] = {};
  std::vector<c32> tab;    // link i's table at tab[i * ntaps], as ofdm_resamp_bank_taps returns it
  DevBuf d_tab;
  void release() {
    d_tab.release();
    StreamStage::release();
  }
};
