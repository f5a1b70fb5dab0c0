// ldpc.h -- coded links: the rate-1/2 quasi-cyclic LDPC code (Z = 64, 12 x 24 base matrix, n = 1536, k = 768) over the
// payload and its layered normalised min-sum decoder.  A second inner code next to fec.h, at the payload boundary: no
// modem kernel knows about it.  All arithmetic is integer: the result is defined bit for bit (include/ofdm_hip.h,
// "coded links: LDPC").
//
//   codeword bit 64 j + z = lane z of column j;  rot(x, s)[z] = x[(z + s) mod 64]
//   check (i, z): XOR over the row's entries (j, s) of rot(x_j, s)[z] = 0
//   block: info bytes payload | CRC-32 big-endian, 96 per codeword (the last one shortened), each codeword sent as its
//   info bytes and then its 96 parity bytes
//
// A circulant is one wave: lane = z everywhere below, the shifts are compile-time constants (LDPC_TABLE, ldpc_plan.h),
// so every row of the schedule is straight-line code with the rotation folded into its LDS addresses.
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
  DevBuf d_cw, d_res;
  std::vector<LdpcBlk> blk;
  std::vector<uint32_t> cw;  // codeword -> block
  std::vector<LdpcRes> res;
  void release() {
    d_cw.release();
    d_res.release();
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

// ---------------------------------------------------------------------------------
// Encoder: one wave per codeword.  A column is one 64-bit word with lane z at bit 63 - z (the info bytes read big-endian),
// so rot(x, s) is a rotate left by s.  The twelve columns are wave-uniform; lambda_i and the parity recursion are
// straight-line scalar code (58 rotate-XORs), then every lane composes whole output bytes: one writer per byte.
// ---------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t ldpc_rotl(uint64_t x, int s) { return s ? (x << s) | (x >> (64 - s)) : x; }
__device__ __forceinline__ uint64_t ldpc_rotr(uint64_t x, int s) { return s ? (x >> s) | (x << (64 - s)) : x; }

template <int I, int J>
__device__ __forceinline__ uint64_t ldpc_info_term(const uint64_t (&x)[12]) {
  constexpr int s = LDPC_TABLE.shift[I][J];
  if constexpr (s >= 0) return ldpc_rotl(x[J], s);
  return 0ull;
}
template <int I, int... Js>
__device__ __forceinline__ uint64_t ldpc_lambda(const uint64_t (&x)[12], std::integer_sequence<int, Js...>) {
  return (ldpc_info_term<I, Js>(x) ^ ...);
}
template <int... Is>
__device__ __forceinline__ void ldpc_lambdas(const uint64_t (&x)[12], uint64_t (&lam)[12], std::integer_sequence<int, Is...>) {
  ((lam[Is] = ldpc_lambda<Is>(x, std::make_integer_sequence<int, 12>{})), ...);
}

__global__ void __launch_bounds__(LDPC_THREADS) k_ldpc_encode(const uint8_t* __restrict__ payloads, const LdpcBlk* __restrict__ blk,
                                                              const uint32_t* __restrict__ cw_blk, uint32_t ncw, uint8_t* __restrict__ coded,
                                                              const uint32_t* __restrict__ crc_table, const uint32_t* __restrict__ xp8) {
  __shared__ __attribute__((aligned(8))) uint8_t s_info[LDPC_WAVES][LDPC_CW_INFO];
  LdpcCw c;
  if (!ldpc_my_codeword(blk, cw_blk, ncw, c)) return;
  const int lane = lane_id();
  const uint32_t n = c.b.len, k = n + 4u;  // n <= OFDM_LDPC_MAX_PAYLOAD (the host refuses longer ones)
  const uint32_t g0 = LDPC_CW_INFO * c.w, kw = ldpc_cw_info(k, c.w);
  const uint8_t* src = payloads + c.b.in_off;
  uint8_t* out = coded + c.b.out_off + (uint64_t)LDPC_CW_SENT * c.w;
  uint8_t* info = s_info[wave_id()];

  // the block's CRC-32, where this codeword holds some of its bytes: 64 pieces of 32 bytes (crc_multmodp, common.h)
  uint32_t crc32 = 0;
  if (g0 + kw > n) {
    const uint32_t o = 32u * (uint32_t)lane;
    if (o < n) {
      const uint32_t nb = (n - o < 32u) ? (n - o) : 32u;
      uint32_t crc = 0xFFFFFFFFu;
      for (uint32_t b = 0; b < nb; b++) crc = crc_table[(crc ^ src[o + b]) & 0xFFu] ^ (crc >> 8);
      crc32 = crc_multmodp(xp8[n - (o + nb)], crc ^ 0xFFFFFFFFu);
    }
#pragma unroll
    for (int d = WAVE / 2; d > 0; d >>= 1) crc32 ^= __shfl_xor(crc32, d, WAVE);
  }
#pragma unroll
  for (uint32_t m = (uint32_t)lane; m < LDPC_CW_INFO; m += WAVE) {
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
  if (lane < 12) mine = __builtin_bswap64(*reinterpret_cast<const uint64_t*>(info + 8 * lane));
  const int mlo = (int)(uint32_t)mine, mhi = (int)(uint32_t)(mine >> 32);
  uint64_t x[12], lam[12], p[12];
#pragma unroll
  for (int j = 0; j < 12; j++)
    x[j] = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane(mhi, j) << 32) | (uint64_t)(uint32_t)__builtin_amdgcn_readlane(mlo, j);
  ldpc_lambdas(x, lam, std::make_integer_sequence<int, 12>{});
  // p_0 = XOR of all lambda;  p_1 = lambda_0 ^ rot(p_0, 1);  p_{i+1} = lambda_i ^ p_i ^ (p_0 if i = 6)
  p[0] = 0;
#pragma unroll
  for (int i = 0; i < 12; i++) p[0] ^= lam[i];
  p[1] = lam[0] ^ ldpc_rotl(p[0], 1);
#pragma unroll
  for (int i = 1; i <= 10; i++) p[i + 1] = lam[i] ^ p[i] ^ (i == 6 ? p[0] : 0ull);
#pragma unroll
  for (uint32_t t = (uint32_t)lane; t < LDPC_CW_PARITY; t += WAVE) {
    const uint32_t col = t >> 3;
    uint64_t v = p[0];
#pragma unroll
    for (uint32_t q = 1; q < 12; q++) v = (col == q) ? p[q] : v;
    out[kw + t] = (uint8_t)(v >> (56u - 8u * (t & 7u)));
  }
}

// ---------------------------------------------------------------------------------
// Decoder: one wave per codeword, lane = z, LDPC_WAVES codewords per workgroup.
//   P        24 x 64 int16 in LDS per codeword; entry (i, j, s) of lane z lives at 64 j + ((z + s) & 63).
//   R        per row and lane one word: the two smallest magnitudes already scaled (mu of the smallest and of the second
//            smallest), the entry that holds the smallest, and the signs of the row's messages.  R_e of an entry is mu2
//            where it held the minimum itself and mu1 elsewhere, with its sign: the 83 messages are never stored.
//   stop     24 ballots of P > 0 make the hard decisions wave-uniform 64-bit columns; the syndrome is 83 scalar
//            rotate-XORs and the exit branch is uniform.
// The rows of one iteration run in order 0 .. 11; a row's entries lie in distinct columns, so its reads and writes of P
// never meet inside the row, and ldpc_wave_sync() stands between rows.
// ---------------------------------------------------------------------------------
template <bool SOFT>
__device__ __forceinline__ int ldpc_value(const uint8_t* __restrict__ in, uint32_t kw, uint32_t b, bool& sent) {
  uint32_t at;
  sent = true;
  if (b < 8u * kw) {
    at = b;
  } else if (b < 8u * LDPC_CW_INFO) {  // shortened: known to be 0, never on the air
    sent = false;
    return -127;
  } else {
    at = 8u * kw + (b - 8u * LDPC_CW_INFO);
  }
  if (SOFT) {
    const int v = (int)(int8_t)in[at];
    return v < -127 ? -127 : v;
  }
  return ((in[at >> 3] >> (7u - (at & 7u))) & 1u) ? LDPC_HARD : -LDPC_HARD;
}

template <int I, int E>
__device__ __forceinline__ int ldpc_at(int lane) {
  constexpr int j = LDPC_TABLE.col[I][E], s = LDPC_TABLE.sh[I][E];
  return LDPC_Z * j + ((lane + s) & (LDPC_Z - 1));
}

// R word: mu1 [0, 7), mu2 [7, 14), entry of the minimum [14, 17), bit 17 + e set: R_e is positive
template <int I, int... Es>
__device__ __forceinline__ void ldpc_row(int16_t* P, uint32_t& rw, int lane, std::integer_sequence<int, Es...>) {
  constexpr int D = LDPC_TABLE.deg[I];
  static_assert(D == (int)sizeof...(Es), "one index per entry of the row");
  const int at[D] = {ldpc_at<I, Es>(lane)...};
  int q[D];
  const int mu1o = (int)(rw & 127u), mu2o = (int)((rw >> 7) & 127u), poso = (int)((rw >> 14) & 7u);
  int m1 = 255, m2 = 255, pos = 0;
  uint32_t beta = 0;
#pragma unroll
  for (int e = 0; e < D; e++) {
    const int mu = (e == poso) ? mu2o : mu1o;
    const int r = ((rw >> (17 + e)) & 1u) ? mu : -mu;
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
  rw = (uint32_t)mu1 | ((uint32_t)mu2 << 7) | ((uint32_t)pos << 14) | (sg << 17);
#pragma unroll
  for (int e = 0; e < D; e++) {
    const int mu = (e == pos) ? mu2 : mu1;
    const int r = ((sg >> e) & 1u) ? mu : -mu;
    P[at[e]] = (int16_t)(q[e] + r);  // |P| <= 127 + 95
  }
}
template <int... Is>
__device__ __forceinline__ void ldpc_iteration(int16_t* P, uint32_t (&rw)[LDPC_ROWS], int lane, std::integer_sequence<int, Is...>) {
  ((ldpc_row<Is>(P, rw[Is], lane, std::make_integer_sequence<int, LDPC_TABLE.deg[Is]>{}), ldpc_wave_sync()), ...);
}

template <int I, int... Es>
__device__ __forceinline__ uint64_t ldpc_check_row(const uint64_t (&X)[LDPC_COLS], std::integer_sequence<int, Es...>) {
  // lane z at bit z here: rot(x, s) is a rotate right by s
  return (ldpc_rotr(X[LDPC_TABLE.col[I][Es]], LDPC_TABLE.sh[I][Es]) ^ ...);
}
template <int... Is>
__device__ __forceinline__ uint64_t ldpc_syndrome(const uint64_t (&X)[LDPC_COLS], std::integer_sequence<int, Is...>) {
  return (ldpc_check_row<Is>(X, std::make_integer_sequence<int, LDPC_TABLE.deg[Is]>{}) | ...);
}

typedef int ldpc_i32x4 __attribute__((ext_vector_type(4), may_alias));

template <bool SOFT>
__global__ void __launch_bounds__(LDPC_THREADS) k_ldpc_decode(const uint8_t* __restrict__ in_all, const LdpcBlk* __restrict__ blk,
                                                              const uint32_t* __restrict__ cw_blk, uint32_t ncw, uint8_t* __restrict__ payloads,
                                                              LdpcRes* __restrict__ res, const uint32_t* __restrict__ crc_table,
                                                              const uint32_t* __restrict__ xp8, uint32_t max_iters) {
  __shared__ __attribute__((aligned(16))) int16_t s_P[LDPC_WAVES][LDPC_N];
  LdpcCw c;
  if (!ldpc_my_codeword(blk, cw_blk, ncw, c)) return;
  const int lane = lane_id();
  const uint32_t k = ldpc_block_info(c.b.len), n = k - 4u;  // (only blocks have codewords)
  const uint32_t g0 = LDPC_CW_INFO * c.w, kw = ldpc_cw_info(k, c.w);
  const uint8_t* in = in_all + c.b.in_off + (uint64_t)(SOFT ? 8u : 1u) * LDPC_CW_SENT * c.w;
  int16_t* P = s_P[wave_id()];

#pragma unroll
  for (int j = 0; j < LDPC_COLS; j++) {
    bool sent;
    P[LDPC_Z * j + lane] = (int16_t)ldpc_value<SOFT>(in, kw, (uint32_t)(LDPC_Z * j + lane), sent);
  }
  ldpc_wave_sync();

  uint32_t rw[LDPC_ROWS];
#pragma unroll
  for (int i = 0; i < LDPC_ROWS; i++) rw[i] = 0;  // R = 0
  uint32_t it = 0;
  uint64_t syn;
#pragma unroll 1
  do {
    it++;
    ldpc_iteration(P, rw, lane, std::make_integer_sequence<int, LDPC_ROWS>{});
    uint64_t X[LDPC_COLS];
#pragma unroll
    for (int j = 0; j < LDPC_COLS; j++) X[j] = __ballot(P[LDPC_Z * j + lane] > 0);
    syn = ldpc_syndrome(X, std::make_integer_sequence<int, LDPC_ROWS>{});
  } while (syn != 0ull && it < max_iters);

  // ---- the codeword's info bytes: payload out, its share of the block's CRC, the received CRC bytes ---------------
  uint8_t* out = payloads + c.b.out_off;
  uint32_t acc = 0, got = 0;
#pragma unroll
  for (uint32_t m = (uint32_t)lane; m < LDPC_CW_INFO; m += WAVE) {
    if (m >= kw) continue;
    const ldpc_i32x4 pk = *reinterpret_cast<const ldpc_i32x4*>(P + 8u * m);  // eight int16
    const uint32_t wd[4] = {(uint32_t)pk.x, (uint32_t)pk.y, (uint32_t)pk.z, (uint32_t)pk.w};
    uint32_t by = 0;
#pragma unroll
    for (int q = 0; q < 4; q++) {
      by = (by << 1) | ((int16_t)(wd[q] & 0xFFFFu) > 0 ? 1u : 0u);
      by = (by << 1) | ((int16_t)(wd[q] >> 16) > 0 ? 1u : 0u);
    }
    const uint32_t g = g0 + m;
    if (g < n) {
      out[g] = (uint8_t)by;
      // CRC-32 of the one byte, moved to its place: crc(A || B) = crc(A) x^(8 |B|) + crc(B)
      acc ^= crc_multmodp(xp8[n - (g + 1u)], crc_table[by ^ 0xFFu] ^ 0xFF000000u);
    } else {
      got |= by << (8u * (3u - (g - n)));
    }
  }
  // ---- corrected: sent positions that are no erasure and whose sign disagrees with the decision -------------------
  uint32_t bad = 0;
#pragma unroll
  for (int j = 0; j < LDPC_COLS; j++) {
    bool sent;
    const int v = ldpc_value<SOFT>(in, kw, (uint32_t)(LDPC_Z * j + lane), sent);
    const bool x = P[LDPC_Z * j + lane] > 0;
    bad += (sent && v != 0 && (v > 0) != x) ? 1u : 0u;
  }
#pragma unroll
  for (int d = WAVE / 2; d > 0; d >>= 1) {
    acc ^= __shfl_xor(acc, d, WAVE);
    got |= __shfl_xor(got, d, WAVE);
  }
  bad = wave_sum(bad);
  if (lane == 0) {  // the block's record starts at zero (the host clears it); its codewords meet in it
    LdpcRes* r = res + c.bi;
    atomicXor(&r->crc, acc);
    atomicOr(&r->got, got);
    atomicAdd(&r->corrected, bad);
    atomicMax(&r->iters, it);
    atomicAdd(&r->failed, syn != 0ull ? 1u : 0u);
  }
}
