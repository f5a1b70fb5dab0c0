// rx_soft.h -- soft-decision receive (ofdm_set_rx_soft): per-bit reliabilities of the delivered packets, one int8 per
// payload bit in the order ofdm_fec_decode_soft reads (include/ofdm_hip.h, "soft-decision receive", has the definition).
//
// k_soft_demap works from what the receiver already computes: the slicer's inputs (the rows the tap pass of k_rx_demod
// writes for OFDM_TAP_RX_SINK), each frame's own equaliser row (the CSI instantiation's `eq`) and the deframer's packet
// list.  One workgroup per frame, keeping exactly the frames k_deframe_write keeps.  The chain's demapped carriers, in
// stream order, are walked in tiles of SOFT_TILE_CARRIERS, one carrier per thread: a tile begins on a frame byte
// (soft_plan.h), so each value has one writer and the tile's values, staged in LDS in output order, leave as whole
// 8-byte groups -- 16-byte stores with an 8-byte head / tail where the packet's place in the buffer asks for one.
#pragma once
#include "rx_deframe.h"
#include "soft_plan.h"

#define SOFT_THREADS 256
static_assert(SOFT_THREADS == SOFT_TILE_CARRIERS, "one carrier of the tile per thread");

struct SoftParams {
  const c32* sink;           // [sink_rows][occ]: sigrot of every sampled symbol the sink demapped (tap pass)
  uint64_t sink_rows;
  const uint64_t* sym_base;  // [npeaks] row of each flag's preamble
  const c32* eq;             // [nframes][eq_stride] hinv of the frame's own preamble
  int eq_stride;
  const int16_t* smap;  // [nmap] occupied index of sink column c
  const c32* cst;       // [arity]
  int occ, nmap, nbits, arity;
  float scale, dmin2;
  int8_t* out;  // value 8 * (payload offset) + index
};

__device__ __forceinline__ float soft_weight(c32 e) {
  const float m = cnorm(e);
  return (m > 0.0f && m <= 3.402823466e+38f) ? 1.0f / m : 0.0f;  // (NaN fails both comparisons)
}

// NB = bits per carrier (p.nbits): the per-bit minima and the value loop are unrolled to exactly that many
template <int NB>
__global__ void __launch_bounds__(SOFT_THREADS) k_soft_demap(DeframeParams q, SoftParams p) {
  extern __shared__ __align__(16) unsigned char soft_smem[];
  float* wL = reinterpret_cast<float*>(soft_smem);  // [nmap] weight of sink column c
  __shared__ c32 cstL[1u << SOFT_MAX_BITS];
  __shared__ uint8_t maskL[SOFT_TILE_MAX_BYTES];
  __shared__ __align__(16) int8_t stage[8 * SOFT_TILE_MAX_BYTES];
  __shared__ float gL;
  const int tid = threadIdx.x;
  const uint32_t f = blockIdx.x;
  // (every exit up to the first barrier is uniform across the workgroup)
  if (f >= dyn_nframes(q.dyn, q.nframes)) return;
  if (q.invalid[f]) return;
  const FrameResult r = q.res[f];
  if (r.status != FR_COMPLETE) return;
  const uint64_t pos = q.pos[f];
  const uint64_t ord = pos >> 40, boff = pos & ((1ull << 40) - 1);
  const uint32_t plen = r.packetlen >= 4 ? r.packetlen - 4 : 0;
  if (ord >= q.max_pkts || boff + plen > q.payload_cap) return;
  if (plen == 0) return;
  const uint32_t nmap = (uint32_t)p.nmap;
  constexpr uint32_t nbits = (uint32_t)NB;

  for (int j = tid; j < p.arity; j += SOFT_THREADS) cstL[j] = p.cst[j];
  const c32* eq = p.eq + (uint64_t)f * (uint64_t)p.eq_stride;
  for (uint32_t c = (uint32_t)tid; c < nmap; c += SOFT_THREADS) wL[c] = soft_weight(eq[p.smap[c]]);
  __syncthreads();
  if (tid == 0) {
    // the mean weight: one sequential float32 chain in carrier order, so that the result does not depend on a tree
    float acc = 0.0f;
    for (uint32_t c = 0; c < nmap; c++) acc = acc + wL[c];
    const float wbar = acc / (float)nmap;
    gL = (wbar > 0.0f && wbar <= 3.402823466e+38f) ? p.scale / (wbar * p.dmin2) : __builtin_nanf("");
  }
  __syncthreads();
  const float g = gL;
  const bool dead = g != g;  // mean weight 0 or not finite: every value of the packet is 0

  const uint64_t first_row = p.sym_base[dyn_j0(q.dyn, q.j0) + f] + 1;  // the preamble's row is not demapped
  const uint64_t ncar = soft_carriers(plen, nbits);
  int8_t* out = p.out + soft_values(boff);
  // a thread's two global reads of a tile: its carrier's slicer input and one whitening-mask byte.  They are issued one
  // tile ahead, in front of the tile's barriers and stores: a packet's tiles are a serial chain, and with the reads
  // inside it the kernel ran at their latency (two dependent round trips per tile)
  c32 xn = mk(0.f, 0.f);
  uint8_t mn = 0;
  // (symbol, column) of the thread's carrier in the tile being fetched, advanced by a tile's worth each time: no division
  // in the loop
  uint32_t sn = (uint32_t)tid / nmap, cn = (uint32_t)tid % nmap;
  const uint32_t ds = SOFT_TILE_CARRIERS / nmap, dc = SOFT_TILE_CARRIERS % nmap;
  auto fetch = [&](uint64_t t0) {
    if (t0) {
      sn += ds;
      cn += dc;
      if (cn >= nmap) {
        cn -= nmap;
        sn++;
      }
    }
    xn = mk(0.f, 0.f);
    if (t0 + (uint32_t)tid < ncar) {
      const uint64_t row = first_row + sn;
      if (row < p.sink_rows) xn = p.sink[row * (uint64_t)p.occ + cn];
    }
    const uint64_t fb = ((t0 * nbits) >> 3) + (uint32_t)tid;  // (a byte the tile does not have is not used)
    mn = (fb >= SOFT_HEADER_BYTES && fb - SOFT_HEADER_BYTES < plen) ? q.mask[fb - SOFT_HEADER_BYTES] : (uint8_t)0;
  };
  fetch(0);
  for (uint64_t t0 = 0; t0 < ncar; t0 += SOFT_TILE_CARRIERS) {
    const SoftTile tile = soft_tile(t0, nbits, plen);
    const c32 x = xn;
    const uint32_t c = cn;
    if ((uint32_t)tid < tile.nbytes) maskL[tid] = mn;
    if (t0 + SOFT_TILE_CARRIERS < ncar) fetch(t0 + SOFT_TILE_CARRIERS);
    __syncthreads();  // (also: the stores of the tile before have read the staging line)
    const uint64_t sc = t0 + (uint32_t)tid;
    if (sc < ncar) {
      // one pass over the table: the nearest point of either class of every bit
      float D0[NB], D1[NB];
#pragma unroll
      for (int b = 0; b < NB; b++) D0[b] = D1[b] = __builtin_inff();
      for (int j = 0; j < p.arity; j++) {
        const float d = cnorm(csub(x, cstL[j]));
#pragma unroll
        for (int b = 0; b < NB; b++) {
          if ((j >> b) & 1)
            D1[b] = d < D1[b] ? d : D1[b];
          else
            D0[b] = d < D0[b] ? d : D0[b];
        }
      }
      const float wg = wL[c] * g;
      const uint32_t bit0 = (uint32_t)tid * nbits;  // of the tile
#pragma unroll
      for (int b = 0; b < NB; b++) {
        const float l = (D0[b] - D1[b]) * wg;
        float v = rintf(l);
        v = (v == v) ? v : 0.0f;  // (before the clamp: fmaxf would turn NaN into the bound)
        v = fminf(fmaxf(v, -127.0f), 127.0f);
        int iv = dead ? 0 : (int)v;
        const uint32_t bt = bit0 + (uint32_t)b, byte = bt >> 3, e = bt & 7u;
        if ((maskL[byte] >> e) & 1u) iv = -iv;
        stage[8u * byte + 7u - e] = (int8_t)iv;
      }
    }
    __syncthreads();
    // ---- the packet's part of the tile to the buffer: 8-byte groups, paired into 16-byte stores where aligned ----
    if (tile.hi > tile.lo) {
      int8_t* og = out + tile.out0;  // 8-byte aligned: the buffer, 8 * boff and out0 all are
      const uint32_t n8 = (tile.hi - tile.lo) >> 3;
      const uint32_t head = (uint32_t)(((uintptr_t)og >> 3) & 1u) < n8 ? (uint32_t)(((uintptr_t)og >> 3) & 1u) : n8;
      const uint32_t n16 = (n8 - head) >> 1;
      const uint2* st = reinterpret_cast<const uint2*>(stage + tile.lo);
      uint2* o8 = reinterpret_cast<uint2*>(og);
      if (tid == 0 && head) o8[0] = st[0];
      uint4* o16 = reinterpret_cast<uint4*>(og + 8u * head);
      for (uint32_t k = (uint32_t)tid; k < n16; k += SOFT_THREADS) {
        const uint2 a = st[head + 2u * k], b = st[head + 2u * k + 1u];
        o16[k] = make_uint4(a.x, a.y, b.x, b.y);
      }
      if (tid == 0 && head + 2u * n16 < n8) o8[n8 - 1u] = st[n8 - 1u];
    }
  }
}
