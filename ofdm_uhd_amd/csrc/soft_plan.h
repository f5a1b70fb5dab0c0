// soft_plan.h -- the host arithmetic of the soft-decision receive option (rx_soft.h / engine_soft.inc): where a packet's
// int8 values lie in the handle's buffer, how many carriers and symbols of the sink's rows they come from, the map
// between a stream bit of the frame sink and a value's place in the decoder's input order, and the tiles k_soft_demap
// walks.  Plain C++ without a HIP include, so that a stand-alone program can check it (tools/soft_plan_check.cpp).
//
// The frame sink packs LSB first: bit b of the point sliced on carrier c of the chain's demapped symbol s is stream bit
// beta = (s * nmap + c) * nbits + b, frame byte beta >> 3, bit weight e = beta & 7.  Frame bytes 0-3 are the header;
// message byte mb = (beta >> 3) - 4 of a packet with plen payload bytes (0 <= mb < plen) owns values 8 mb .. 8 mb + 7,
// MSB first: the value of bit weight e is at 8 mb + 7 - e.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define SOFT_HD __host__ __device__
#else
#define SOFT_HD
#endif

#define SOFT_HEADER_BYTES 4u
#define SOFT_TILE_CARRIERS 256u  // carriers per tile: a multiple of 8, so that every tile begins on a frame byte
#define SOFT_TILE_MAX_BYTES 256u  // frame bytes of a tile at 8 bits per carrier
#define SOFT_MAX_BITS 8u

// values of a packet, and where packet k's begin when the payloads begin at pay_off[k] bytes: 8 per payload byte
SOFT_HD static inline uint64_t soft_values(uint64_t plen) { return 8ull * plen; }

// value offsets of the call's packets from the payload offsets (npk + 1 entries each); returns the total
static inline uint64_t soft_plan_offsets(const uint64_t* pay_off, uint64_t npk, uint64_t* val_off) {
  for (uint64_t k = 0; k <= npk; k++) val_off[k] = soft_values(pay_off[k]);
  return npk ? val_off[npk] : 0;
}

// carriers of the chain (in stream order) whose bits reach the packet's last payload byte, and the symbols that hold them
SOFT_HD static inline uint64_t soft_carriers(uint32_t plen, uint32_t nbits) {
  if (plen == 0 || nbits == 0) return 0;
  return (8ull * (SOFT_HEADER_BYTES + (uint64_t)plen) + nbits - 1u) / nbits;
}
SOFT_HD static inline uint64_t soft_symbols(uint32_t plen, uint32_t nmap, uint32_t nbits) {
  if (nmap == 0) return 0;
  return (soft_carriers(plen, nbits) + nmap - 1u) / nmap;
}

// stream bit -> value index of the packet, -1 for a header bit, a CRC bit or anything behind the packet
SOFT_HD static inline int64_t soft_out_index(uint64_t beta, uint32_t plen) {
  const uint64_t byte = beta >> 3, e = beta & 7u;
  if (byte < SOFT_HEADER_BYTES || byte - SOFT_HEADER_BYTES >= plen) return -1;
  return (int64_t)(8u * (byte - SOFT_HEADER_BYTES) + 7u - e);
}
// and back (used by nothing but the checks)
SOFT_HD static inline uint64_t soft_beta(uint64_t index) {
  return 8u * ((index >> 3) + SOFT_HEADER_BYTES) + 7u - (index & 7u);
}

// One tile of k_soft_demap: carriers [first, first + SOFT_TILE_CARRIERS) of the chain fill frame bytes
// [byte0, byte0 + nbytes); their values are staged in output order, staging index i = 8 * (frame byte - byte0) + 7 - e.
// Of those, [lo, hi) belong to the packet and go to value index out0 + (i - lo); lo, hi and out0 are multiples of 8.
struct SoftTile {
  uint64_t byte0;
  uint32_t nbytes;
  uint32_t lo, hi;
  uint64_t out0;
};
SOFT_HD static inline SoftTile soft_tile(uint64_t first, uint32_t nbits, uint32_t plen) {
  SoftTile t;
  t.byte0 = (first * nbits) >> 3;  // exact: first is a multiple of SOFT_TILE_CARRIERS
  t.nbytes = (SOFT_TILE_CARRIERS / 8u) * nbits;
  const uint64_t m0 = SOFT_HEADER_BYTES, m1 = SOFT_HEADER_BYTES + (uint64_t)plen;  // the packet's frame bytes
  const uint64_t a = t.byte0 > m0 ? t.byte0 : m0;
  const uint64_t e = t.byte0 + t.nbytes < m1 ? t.byte0 + t.nbytes : m1;
  if (a >= e) {
    t.lo = t.hi = 0;
    t.out0 = 0;
    return t;
  }
  t.lo = (uint32_t)(8u * (a - t.byte0));
  t.hi = (uint32_t)(8u * (e - t.byte0));
  t.out0 = 8u * (a - m0);
  return t;
}
