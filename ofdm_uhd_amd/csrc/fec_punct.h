// fec_punct.h -- the punctured rates 2/3, 3/4 and 5/6 of the coded-link layer (fec.h): the layer that leaves coded bits
// out on the way to the air and puts erasures back in front of the decoder.  The encoder here forms only the kept
// parities, the decoder (k_fec_decode, unchanged) reads the expanded block as any other soft block.
// Definition: include/ofdm_hip.h ("punctured rates"), arithmetic: punct_plan.h, DESIGN.md section 7.
//
//   kept bit q   = mother bit punct_unrank(q), q < K; zero for K <= q < 8P
//   sent bit j   = kept bit (j mod R') * C' + j / R', R' = 8P / C'
#pragma once
#include "fec.h"
#include "punct_plan.h"

#define FEC_DEPUNCT_THREADS 256

// what the punctured rates keep on a handle next to FecState: nothing of it exists until a call at such a rate
struct FecPunctState {
  DevBuf d_pblk, d_mother;        // k_fec_depuncture's block table; the mother values of one slice
  std::vector<FecBlk> pblk;
  double last_ms = 0.0;
  bool timed = false;             // last_ms is of the last fec call
  void release() {
    d_pblk.release();
    d_mother.release();
  }
};

// ---------------------------------------------------------------------------------
// Punctured encoder: k_fec_encode's two passes (fec.h: fec_stage_info, fec_compose) with another bit source.  A sent bit
// is found through the C' interleaver and the pattern's unrank, and is one parity over seven info bits: the mother
// block is never formed, a dropped bit costs nothing.  blk: {payload offset, block offset, payload bytes}.
// ---------------------------------------------------------------------------------
template <uint32_t RATE>
__global__ void __launch_bounds__(FEC_ENC_THREADS) k_fec_puncture(const uint8_t* __restrict__ payloads, const FecBlk* __restrict__ blk,
                                                                  uint8_t* __restrict__ coded, const uint32_t* __restrict__ crc_table,
                                                                  const uint32_t* __restrict__ xp8, uint32_t lgC) {
  __shared__ uint8_t info[FEC_INFO_LDS];
  __shared__ uint32_t red[FEC_ENC_THREADS / WAVE];
  const FecBlk b = blk[blockIdx.x];
  const uint32_t n = b.len;  // <= OFDM_FEC_MAX_PAYLOAD (the host refuses longer ones)
  const int tid = threadIdx.x;
  fec_stage_info(info, red, payloads + b.in_off, n, tid, crc_table, xp8);
  const uint32_t K = punct_kept_bits<RATE>(n);
  const uint32_t nout = (K + 7u) >> 3;
  fec_compose(coded + b.out_off, info, nout, punct_log2_cols(lgC, nout), K, tid, [](uint32_t q) { return punct_unrank<RATE>(q); });
}

// ---------------------------------------------------------------------------------
// Depuncture: one workgroup per block.  Expands a punctured block into the 8 (2n + 10) int8 mother values, in coded
// order, that k_fec_decode<true> reads at one column.  Every thread owns whole 16-byte groups of the output: mother
// position i is zero where the pattern dropped it or the pad lies, else the value of kept bit rank(i), fetched from
// where the C' interleaver sent it; a group leaves in one 16-byte store.  The divisions by the period are by
// compile-time constants.  blk: {input offset (bytes hard, values soft), offset into the mother values, punctured
// bytes P, mother bytes 2n + 10 or 0}: a block whose length is no block at this rate (pad = 0) writes nothing, and the
// decoder's own table calls it no block.
// ---------------------------------------------------------------------------------
template <uint32_t RATE, bool SOFT>
__global__ void __launch_bounds__(FEC_DEPUNCT_THREADS) k_fec_depuncture(const uint8_t* __restrict__ in_all, const FecBlk* __restrict__ blk,
                                                                        int8_t* __restrict__ mother, uint32_t lgC) {
  const FecBlk b = blk[blockIdx.x];
  const uint32_t mlen = b.pad;
  if (mlen == 0) return;
  const uint32_t P = b.len;                // = punct_block_len<RATE>(n) (the host found n from it)
  const uint32_t ncoded = 8u * mlen - 4u;  // 2T; the four positions behind are the pad
  const uint32_t lgc = punct_log2_cols(lgC, P);
  const uint32_t R = (8u * P) >> lgc;
  const uint8_t* in = in_all + b.in_off;
  uint4* out = reinterpret_cast<uint4*>(mother + b.out_off);  // 16-byte aligned: the host's strides are multiples of 16
  const uint32_t ngroups = mlen >> 1;                          // 8 mlen / 16, mlen is even
  for (uint32_t g = threadIdx.x; g < ngroups; g += FEC_DEPUNCT_THREADS) {
    uint32_t w[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      uint32_t word = 0;
#pragma unroll
      for (int e = 0; e < 4; e++) {
        const uint32_t i = 16u * g + 4u * (uint32_t)k + (uint32_t)e;
        int v = 0;
        if (i < ncoded && punct_kept<RATE>(i)) {
          const uint32_t q = punct_rank<RATE>(i);                      // < K <= 8P
          const uint32_t j = (q & ((1u << lgc) - 1u)) * R + (q >> lgc);  // where kept bit q was sent, < 8P
          if (SOFT)
            v = (int)(int8_t)in[j];
          else
            v = ((in[j >> 3] >> (7u - (j & 7u))) & 1u) ? 1 : -1;
        }
        word |= ((uint32_t)v & 0xFFu) << (8 * e);
      }
      w[k] = word;
    }
    out[g] = make_uint4(w[0], w[1], w[2], w[3]);
  }
}
