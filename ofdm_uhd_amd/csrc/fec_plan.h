// fec_plan.h -- the host arithmetic of the coded-link layer (fec.h / engine_fec.inc): block lengths, the trellis
// geometry, the interleaver's column count and how a batch is cut into slices that share one bounded workspace.
// Plain C++ without a HIP include, so that a stand-alone program can check it (tools/fec_plan_check.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/ofdm_hip.h"

#ifdef __HIPCC__
#define FEC_HD __host__ __device__
#else
#define FEC_HD
#endif

// the decision workspace never grows past this: a larger batch is decoded in slices
constexpr uint64_t FEC_WS_MAX_BYTES = 512ull << 20;

// coded block of an n-byte payload: 2 (n + 4) info bytes + 12 tail bits + 4 pad bits
static inline int fec_coded_len(uint32_t payload_len, uint32_t* coded_len) {
  if (!coded_len || payload_len > OFDM_FEC_MAX_PAYLOAD) return OFDM_E_INVAL;
  *coded_len = 2u * payload_len + 10u;
  return OFDM_OK;
}

// lengths that are no block: odd, under 10, over OFDM_FEC_MAX_CODED
FEC_HD static inline bool fec_is_block(uint32_t coded_len) {
  return !(coded_len & 1u) && coded_len >= 10u && coded_len <= OFDM_FEC_MAX_CODED;
}

static inline int fec_payload_len(uint32_t coded_len, uint32_t* payload_len) {
  if (!payload_len || !fec_is_block(coded_len)) return OFDM_E_INVAL;
  *payload_len = (coded_len - 10u) / 2u;
  return OFDM_OK;
}

// trellis steps of a block, and the 64-step decision chunks that hold them
static inline uint32_t fec_steps(uint32_t coded_len) { return 4u * coded_len - 2u; }  // 8 (n + 4) + 6
static inline uint32_t fec_chunks(uint32_t coded_len) { return (fec_steps(coded_len) + 63u) / 64u; }

// log2 of the column count, -1 for a count outside {1, 2, 4, 8, 16}
static inline int fec_log2_cols(uint32_t cols) {
  for (int l = 0; l <= 4; l++)
    if (cols == (1u << l)) return l;
  return -1;
}

// Blocks per slice: every block of a slice owns `stride_words` 8-byte decision words of the workspace.  At least one,
// at most nblk, and never more than fit cap_bytes (one block always fits: 256 chunks * 512 bytes = 128 KiB).
static inline uint64_t fec_slice_blocks(uint64_t nblk, uint64_t stride_words, uint64_t cap_bytes) {
  if (nblk == 0) return 0;
  const uint64_t per = stride_words ? stride_words * 8u : 8u;
  uint64_t fit = cap_bytes / per;
  if (fit < 1) fit = 1;
  return fit < nblk ? fit : nblk;
}

// one block of a batch as the kernels see it
struct FecBlk {
  uint64_t in_off;   // into the input blob: bytes (payloads, hard blocks) or values (soft blocks)
  uint64_t out_off;  // into the output blob, bytes
  uint32_t len;      // encode: payload bytes; decode: coded bytes (any value: a length that is no block decodes to nothing)
  uint32_t pad;
};

// Layout of a decode batch: out_off[0..nblk] of the payloads (a length that is no block takes no room), the widest
// block's workspace stride in words and the bytes of input the valid blocks reach (`unit` input items per coded byte:
// 1 hard, 8 soft).  Returns the total payload bytes.
static inline uint64_t fec_plan_decode(const uint64_t* in_off, const uint32_t* coded_len, uint64_t nblk, uint64_t unit, FecBlk* blk,
                                       uint64_t* out_off, uint64_t* stride_words, uint64_t* in_extent) {
  uint64_t o = 0, stride = 0, ext = 0;
  for (uint64_t k = 0; k < nblk; k++) {
    blk[k].in_off = in_off[k];
    blk[k].out_off = o;
    blk[k].len = coded_len[k];
    blk[k].pad = 0;
    out_off[k] = o;
    if (fec_is_block(coded_len[k])) {
      o += (coded_len[k] - 10u) / 2u;
      const uint64_t w = 64ull * fec_chunks(coded_len[k]);
      if (w > stride) stride = w;
      const uint64_t e = in_off[k] + unit * coded_len[k];
      if (e > ext) ext = e;
    }
  }
  out_off[nblk] = o;
  *stride_words = stride;
  *in_extent = ext;
  return o;
}
