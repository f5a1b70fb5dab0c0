// ldpc.h -- coded links: the quasi-cyclic LDPC codes (Z = 64, 24 columns, n = 1536; rate 1/2 with a 12 x 24 base matrix and
// k = 768, rates 2/3, 3/4 and 5/6 with 8, 6 and 4 rows) over the payload and their layered normalised min-sum decoder.  A second inner code next to fec.h, at the payload boundary: no
// modem kernel knows about it.  All arithmetic is integer: the result is defined bit for bit (include/ofdm_hip.h,
// "coded links: LDPC").
//
//   codeword bit 64 j + z = lane z of column j;  rot(x, s)[z] = x[(z + s) mod 64]
//   check (i, z): XOR over the row's entries (j, s) of rot(x_j, s)[z] = 0
//   block: info bytes payload | CRC-32 big-endian, KI per codeword (the last one shortened), each codeword sent as its
//   info bytes and then its PB parity bytes (KI / PB = 96 / 96, 128 / 64, 144 / 48, 160 / 32)
//
// A circulant is one wave: lane = z everywhere below, the shifts are compile-time constants (LDPC_TABLE_R<RATE>,
// ldpc_plan.h), so every row of the schedule is straight-line code with the rotation folded into its LDS addresses.
// The kernels are templates over the rate: another rate is another table, and the rate-1/2 instantiations are the code
// they were before the other rates came.
#pragma once
#include "common.h"
#include "host_util.h"
#include "ldpc_plan.h"

#include <utility>

#define LDPC_WAVES 4  // codewords per workgroup
#define LDPC_THREADS (LDPC_WAVES * WAVE)
#define LDPC_N (LDPC_COLS * LDPC_Z)
#define LDPC_HARD 16  // a hard bit as a decoder value

// host side (engine_ldpc.inc): CodecStage (host_util.h) and the code's own
struct LdpcState : CodecStage {
  DevBuf d_cw, d_res, d_rel;  // d_rel: host mode of the _rel calls only
  std::vector<LdpcBlk> blk;
  std::vector<uint32_t> cw;  // codeword -> block
  std::vector<LdpcRes> res;
  void release() {
    d_cw.release();
    d_res.release();
    d_rel.release();
    CodecStage::release();
  }
};

// The codeword's lanes talk through LDS that only their own wave touches: LDS operations of one wave complete in
// order, so all that is needed is that the compiler keeps the order, too.
__device__ __forceinline__ void ldpc_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// the codeword of this wave: its block and its place in it (all wave-uniform)
struct LdpcCw {
  uint32_t bi, w;
  LdpcBlk b;
};
__device__ __forceinline__ bool ldpc_my_codeword(const LdpcBlk* __restrict__ blk, const uint32_t* __restrict__ cw_blk, uint32_t ncw, LdpcCw& c) {
  const uint32_t ci = blockIdx.x * LDPC_WAVES + (uint32_t)__builtin_amdgcn_readfirstlane(wave_id());
  if (ci >= ncw) return false;
  c.bi = (uint32_t)__builtin_amdgcn_readfirstlane((int)cw_blk[ci]);
  c.b = blk[c.bi];
  c.w = ci - c.b.cw0;
  return true;
}

// ldpc_plan.h's block arithmetic with the rate as a compile-time constant
template <uint32_t RATE>
__device__ __forceinline__ uint32_t ldpc_cw_info_of(uint32_t k, uint32_t w) {
  constexpr uint32_t KI = ldpc_rate_info(RATE);
  const uint32_t left = k - KI * w;
  return left < KI ? left : KI;
}
template <uint32_t RATE>
__device__ __forceinline__ uint32_t ldpc_block_info_of(uint32_t coded_len) {
  constexpr uint32_t PB = ldpc_rate_parity(RATE);
  return coded_len - PB * ldpc_block_words(coded_len);
}

// ---------------------------------------------------------------------------------
// Encoder: one wave per codeword.  A column is one 64-bit word with lane z at bit 63 - z (the info bytes read big-endian),
// so rot(x, s) is a rotate left by s.  The kb info columns are wave-uniform; lambda_i and the parity recursion are
// straight-line scalar code (58 rotate-XORs at rate 1/2), then every lane composes whole output bytes: one writer per
// byte.
// ---------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t ldpc_rotl(uint64_t x, int s) { return s ? (x << s) | (x >> (64 - s)) : x; }
__device__ __forceinline__ uint64_t ldpc_rotr(uint64_t x, int s) { return s ? (x >> s) | (x << (64 - s)) : x; }

template <uint32_t RATE, int I, int J>
__device__ __forceinline__ uint64_t ldpc_info_term(const uint64_t (&x)[LDPC_TABLE_R<RATE>.kb]) {
  constexpr int s = LDPC_TABLE_R<RATE>.shift[I][J];
  if constexpr (s >= 0) return ldpc_rotl(x[J], s);
  return 0ull;
}
template <uint32_t RATE, int I, int... Js>
__device__ __forceinline__ uint64_t ldpc_lambda(const uint64_t (&x)[LDPC_TABLE_R<RATE>.kb], std::integer_sequence<int, Js...>) {
  return (ldpc_info_term<RATE, I, Js>(x) ^ ...);
}
template <uint32_t RATE, int... Is>
__device__ __forceinline__ void ldpc_lambdas(const uint64_t (&x)[LDPC_TABLE_R<RATE>.kb], uint64_t (&lam)[LDPC_TABLE_R<RATE>.mb],
                                             std::integer_sequence<int, Is...>) {
  ((lam[Is] = ldpc_lambda<RATE, Is>(x, std::make_integer_sequence<int, LDPC_TABLE_R<RATE>.kb>{})), ...);
}

template <uint32_t RATE>
__global__ void __launch_bounds__(LDPC_THREADS) k_ldpc_encode(const uint8_t* __restrict__ payloads, const LdpcBlk* __restrict__ blk,
                                                              const uint32_t* __restrict__ cw_blk, uint32_t ncw, uint8_t* __restrict__ coded,
                                                              const uint32_t* __restrict__ crc_table, const uint32_t* __restrict__ xp8) {
  constexpr int MB = LDPC_TABLE_R<RATE>.mb, KB = LDPC_TABLE_R<RATE>.kb, MID = LDPC_TABLE_R<RATE>.mid;
  constexpr uint32_t KI = ldpc_rate_info(RATE), PB = ldpc_rate_parity(RATE);
  // the block CRC's pieces, one per lane: 64 x 32 bytes reach the rate-1/2 payloads, 64 x 64 bytes the longer ones
  constexpr uint32_t PIECE = RATE == OFDM_LDPC_RATE_1_2 ? 32u : 64u;
  static_assert(WAVE * PIECE >= ldpc_rate_max_payload(RATE), "the pieces cover the longest payload");
  __shared__ __attribute__((aligned(8))) uint8_t s_info[LDPC_WAVES][KI];
  LdpcCw c;
  if (!ldpc_my_codeword(blk, cw_blk, ncw, c)) return;
  const int lane = lane_id();
  const uint32_t n = c.b.len, k = n + 4u;  // n <= the rate's largest payload (the host refuses longer ones)
  const uint32_t g0 = KI * c.w, kw = ldpc_cw_info_of<RATE>(k, c.w);
  const uint8_t* src = payloads + c.b.in_off;
  uint8_t* out = coded + c.b.out_off + (uint64_t)LDPC_CW_SENT * c.w;
  uint8_t* info = s_info[wave_id()];

  // the block's CRC-32, where this codeword holds some of its bytes: 64 pieces of PIECE bytes (crc_multmodp, common.h)
  uint32_t crc32 = 0;
  if (g0 + kw > n) {
    const uint32_t o = PIECE * (uint32_t)lane;
    if (o < n) {
      const uint32_t nb = (n - o < PIECE) ? (n - o) : PIECE;
      uint32_t crc = 0xFFFFFFFFu;
      for (uint32_t b = 0; b < nb; b++) crc = crc_table[(crc ^ src[o + b]) & 0xFFu] ^ (crc >> 8);
      crc32 = crc_multmodp(xp8[n - (o + nb)], crc ^ 0xFFFFFFFFu);
    }
#pragma unroll
    for (int d = WAVE / 2; d > 0; d >>= 1) crc32 ^= __shfl_xor(crc32, d, WAVE);
  }
#pragma unroll
  for (uint32_t m = (uint32_t)lane; m < KI; m += WAVE) {
    const uint32_t g = g0 + m;
    uint8_t v = 0;  // behind the block's info bytes: the shortened positions
    if (g < n)
      v = src[g];
    else if (g < k)
      v = (uint8_t)(crc32 >> (8u * (3u - (g - n))));  // struct.pack(">I", crc)
    info[m] = v;
    if (m < kw) out[m] = v;
  }
  ldpc_wave_sync();
  uint64_t mine = 0;
  if (lane < KB) mine = __builtin_bswap64(*reinterpret_cast<const uint64_t*>(info + 8 * lane));
  const int mlo = (int)(uint32_t)mine, mhi = (int)(uint32_t)(mine >> 32);
  uint64_t x[KB], lam[MB], p[MB];
#pragma unroll
  for (int j = 0; j < KB; j++)
    x[j] = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane(mhi, j) << 32) | (uint64_t)(uint32_t)__builtin_amdgcn_readlane(mlo, j);
  ldpc_lambdas<RATE>(x, lam, std::make_integer_sequence<int, MB>{});
  // p_0 = XOR of all lambda;  p_1 = lambda_0 ^ rot(p_0, 1);  p_{i+1} = lambda_i ^ p_i ^ (p_0 if i = mid)
  p[0] = 0;
#pragma unroll
  for (int i = 0; i < MB; i++) p[0] ^= lam[i];
  p[1] = lam[0] ^ ldpc_rotl(p[0], 1);
#pragma unroll
  for (int i = 1; i <= MB - 2; i++) p[i + 1] = lam[i] ^ p[i] ^ (i == MID ? p[0] : 0ull);
#pragma unroll
  for (uint32_t t = (uint32_t)lane; t < PB; t += WAVE) {
    const uint32_t col = t >> 3;
    uint64_t v = p[0];
#pragma unroll
    for (uint32_t q = 1; q < (uint32_t)MB; q++) v = (col == q) ? p[q] : v;
    out[kw + t] = (uint8_t)(v >> (56u - 8u * (t & 7u)));
  }
}

// ---------------------------------------------------------------------------------
// Decoder: one wave per codeword, lane = z, LDPC_WAVES codewords per workgroup.
//   P        24 x 64 int16 in LDS per codeword; entry (i, j, s) of lane z lives at 64 j + ((z + s) & 63).
//   R        per row and lane one word: the two smallest magnitudes already scaled (mu of the smallest and of the second
//            smallest), the entry that holds the smallest, and the signs of the row's messages.  R_e of an entry is mu2
//            where it held the minimum itself and mu1 elsewhere, with its sign: the messages are never stored.  At rate
//            1/2 (rows of up to 7 entries) the word has 32 bits; the longer rows of the other rates (up to 19 entries)
//            take 64: magnitudes and a 5-bit position in the low half, the signs in the high half.
//   stop     24 ballots of P > 0 make the hard decisions wave-uniform 64-bit columns; the syndrome is one scalar
//            rotate-XOR per entry (83 at rate 1/2) and the exit branch is uniform.
//   rel      (k_ldpc_decode_rel) in the epilogue the lane that forms info byte m from the eight int16 at P + 8 m also
//            takes the smallest of their magnitudes: the byte's reliability is min(127, that) + 128 where syn == 0.
// The rows of one iteration run in order 0 .. mb - 1; a row's entries lie in distinct columns, so its reads and writes of P
// never meet inside the row, and ldpc_wave_sync() stands between rows.
// ---------------------------------------------------------------------------------
template <bool SOFT, uint32_t RATE>
__device__ __forceinline__ int ldpc_value(const uint8_t* __restrict__ in, uint32_t kw, uint32_t b, bool& sent) {
  constexpr uint32_t KI = ldpc_rate_info(RATE);
  uint32_t at;
  sent = true;
  if (b < 8u * kw) {
    at = b;
  } else if (b < 8u * KI) {  // shortened: known to be 0, never on the air
    sent = false;
    return -127;
  } else {
    at = 8u * kw + (b - 8u * KI);
  }
  if (SOFT) {
    const int v = (int)(int8_t)in[at];
    return v < -127 ? -127 : v;
  }
  return ((in[at >> 3] >> (7u - (at & 7u))) & 1u) ? LDPC_HARD : -LDPC_HARD;
}

template <uint32_t RATE, int I, int E>
__device__ __forceinline__ int ldpc_at(int lane) {
  constexpr int j = LDPC_TABLE_R<RATE>.col[I][E], s = LDPC_TABLE_R<RATE>.sh[I][E];
  return LDPC_Z * j + ((lane + s) & (LDPC_Z - 1));
}

// R word: mu1 [0, 7), mu2 [7, 14), entry of the minimum behind them, bit SIGN + e set: R_e is positive.  Rate 1/2: a
// 3-bit entry [14, 17) and SIGN = 17 in 32 bits; the other rates: a 5-bit entry [14, 19) and SIGN = 32 in 64 bits.
template <uint32_t RATE>
struct LdpcRw {
  typedef uint64_t type;
  static constexpr int POS_BITS = 5, SIGN = 32;
};
template <>
struct LdpcRw<OFDM_LDPC_RATE_1_2> {
  typedef uint32_t type;
  static constexpr int POS_BITS = 3, SIGN = 17;
};

template <uint32_t RATE, int I, int... Es>
__device__ __forceinline__ void ldpc_row(int16_t* P, typename LdpcRw<RATE>::type& rw, int lane, std::integer_sequence<int, Es...>) {
  typedef typename LdpcRw<RATE>::type rw_t;
  constexpr int D = LDPC_TABLE_R<RATE>.deg[I], SIGN = LdpcRw<RATE>::SIGN;
  static_assert(D == (int)sizeof...(Es), "one index per entry of the row");
  static_assert(D <= (1 << LdpcRw<RATE>::POS_BITS) && SIGN + D <= 8 * (int)sizeof(rw_t) && 14 + LdpcRw<RATE>::POS_BITS <= SIGN, "the R word holds the row");
  const int at[D] = {ldpc_at<RATE, I, Es>(lane)...};
  int q[D];
  const int mu1o = (int)(rw & 127u), mu2o = (int)((rw >> 7) & 127u), poso = (int)((rw >> 14) & ((1u << LdpcRw<RATE>::POS_BITS) - 1u));
  int m1 = 255, m2 = 255, pos = 0;
  uint32_t beta = 0;
#pragma unroll
  for (int e = 0; e < D; e++) {
    const int mu = (e == poso) ? mu2o : mu1o;
    const int r = ((rw >> (SIGN + e)) & 1u) ? mu : -mu;
    int v = (int)P[at[e]] - r;
    v = v < -127 ? -127 : (v > 127 ? 127 : v);
    q[e] = v;
    beta |= (v > 0 ? 1u : 0u) << e;
    const int a = v < 0 ? -v : v;
    if (a < m1) {
      m2 = m1;
      m1 = a;
      pos = e;
    } else if (a < m2) {
      m2 = a;
    }
  }
  const int mu1 = (3 * m1) >> 2, mu2 = (3 * m2) >> 2;
  // R_e is positive where the XOR of the row's other signs is 1
  const uint32_t sg = ((__popc(beta) & 1) ? ~beta : beta) & ((1u << D) - 1u);
  rw = (rw_t)((uint32_t)mu1 | ((uint32_t)mu2 << 7) | ((uint32_t)pos << 14)) | ((rw_t)sg << SIGN);
#pragma unroll
  for (int e = 0; e < D; e++) {
    const int mu = (e == pos) ? mu2 : mu1;
    const int r = ((sg >> e) & 1u) ? mu : -mu;
    P[at[e]] = (int16_t)(q[e] + r);  // |P| <= 127 + 95
  }
}
template <uint32_t RATE, int... Is>
__device__ __forceinline__ void ldpc_iteration(int16_t* P, typename LdpcRw<RATE>::type (&rw)[LDPC_TABLE_R<RATE>.mb], int lane,
                                               std::integer_sequence<int, Is...>) {
  ((ldpc_row<RATE, Is>(P, rw[Is], lane, std::make_integer_sequence<int, LDPC_TABLE_R<RATE>.deg[Is]>{}), ldpc_wave_sync()), ...);
}

template <uint32_t RATE, int I, int... Es>
__device__ __forceinline__ uint64_t ldpc_check_row(const uint64_t (&X)[LDPC_COLS], std::integer_sequence<int, Es...>) {
  // lane z at bit z here: rot(x, s) is a rotate right by s
  return (ldpc_rotr(X[LDPC_TABLE_R<RATE>.col[I][Es]], LDPC_TABLE_R<RATE>.sh[I][Es]) ^ ...);
}
template <uint32_t RATE, int... Is>
__device__ __forceinline__ uint64_t ldpc_syndrome(const uint64_t (&X)[LDPC_COLS], std::integer_sequence<int, Is...>) {
  return (ldpc_check_row<RATE, Is>(X, std::make_integer_sequence<int, LDPC_TABLE_R<RATE>.deg[Is]>{}) | ...);
}

typedef int ldpc_i32x4 __attribute__((ext_vector_type(4), may_alias));

// The decoder's two entry points over one body (ldpc_decode_body.inc): k_ldpc_decode, and k_ldpc_decode_rel with one
// reliability byte per payload byte (include/ofdm_hip.h, "coded links: LDPC, reliabilities out").
template <bool SOFT, uint32_t RATE>
__global__ void __launch_bounds__(LDPC_THREADS) k_ldpc_decode(const uint8_t* __restrict__ in_all, const LdpcBlk* __restrict__ blk,
                                                              const uint32_t* __restrict__ cw_blk, uint32_t ncw, uint8_t* __restrict__ payloads,
                                                              LdpcRes* __restrict__ res, const uint32_t* __restrict__ crc_table,
                                                              const uint32_t* __restrict__ xp8, uint32_t max_iters) {
#define LDPC_DECODE_REL 0
#include "ldpc_decode_body.inc"
#undef LDPC_DECODE_REL
}

template <bool SOFT, uint32_t RATE>
__global__ void __launch_bounds__(LDPC_THREADS) k_ldpc_decode_rel(const uint8_t* __restrict__ in_all, const LdpcBlk* __restrict__ blk,
                                                                  const uint32_t* __restrict__ cw_blk, uint32_t ncw,
                                                                  uint8_t* __restrict__ payloads, uint8_t* __restrict__ rel,
                                                                  LdpcRes* __restrict__ res, const uint32_t* __restrict__ crc_table,
                                                                  const uint32_t* __restrict__ xp8, uint32_t max_iters) {
#define LDPC_DECODE_REL 1
#include "ldpc_decode_body.inc"
#undef LDPC_DECODE_REL
}
