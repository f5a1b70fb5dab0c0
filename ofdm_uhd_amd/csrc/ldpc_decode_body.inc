// ldpc_decode_body.inc -- the body of the LDPC decoder kernels (ldpc.h), included once into each of its two entry points:
// k_ldpc_decode with LDPC_DECODE_REL 0 and k_ldpc_decode_rel with LDPC_DECODE_REL 1.  The text stands in the kernel itself
// and not in a __device__ function behind it, because k_ldpc_decode has to stay the code it was: through an inlined
// function the same statements came out with other register counts (DESIGN.md section 7).  It sees the kernel's template
// parameters SOFT and RATE and its arguments; with LDPC_DECODE_REL also `rel`.
//
// LDPC_DECODE_REL: the lane that forms info byte m also takes the smallest of the byte's eight |P| and stores the
// reliability q = min(127, that) + 128 * (syn == 0) at rel + out_off + g for g < n: one writer per byte, no atomics.
  constexpr int MB = LDPC_TABLE_R<RATE>.mb;
  constexpr uint32_t KI = ldpc_rate_info(RATE);
  __shared__ __attribute__((aligned(16))) int16_t s_P[LDPC_WAVES][LDPC_N];
  LdpcCw c;
  if (!ldpc_my_codeword(blk, cw_blk, ncw, c)) return;
  const int lane = lane_id();
  const uint32_t k = ldpc_block_info_of<RATE>(c.b.len), n = k - 4u;  // (only blocks have codewords)
  const uint32_t g0 = KI * c.w, kw = ldpc_cw_info_of<RATE>(k, c.w);
  const uint8_t* in = in_all + c.b.in_off + (uint64_t)(SOFT ? 8u : 1u) * LDPC_CW_SENT * c.w;
  int16_t* P = s_P[wave_id()];

#pragma unroll
  for (int j = 0; j < LDPC_COLS; j++) {
    bool sent;
    P[LDPC_Z * j + lane] = (int16_t)ldpc_value<SOFT, RATE>(in, kw, (uint32_t)(LDPC_Z * j + lane), sent);
  }
  ldpc_wave_sync();

  typename LdpcRw<RATE>::type rw[MB];
#pragma unroll
  for (int i = 0; i < MB; i++) rw[i] = 0;  // R = 0
  uint32_t it = 0;
  uint64_t syn;
#pragma unroll 1
  do {
    it++;
    ldpc_iteration<RATE>(P, rw, lane, std::make_integer_sequence<int, MB>{});
    uint64_t X[LDPC_COLS];
#pragma unroll
    for (int j = 0; j < LDPC_COLS; j++) X[j] = __ballot(P[LDPC_Z * j + lane] > 0);
    syn = ldpc_syndrome<RATE>(X, std::make_integer_sequence<int, MB>{});
  } while (syn != 0ull && it < max_iters);

  // ---- the codeword's info bytes: payload out, its share of the block's CRC, the received CRC bytes ---------------
  uint8_t* out = payloads + c.b.out_off;
  uint32_t acc = 0, got = 0;
#pragma unroll
  for (uint32_t m = (uint32_t)lane; m < KI; m += WAVE) {
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
#if LDPC_DECODE_REL
      {
        int weakest = 127;  // min(127, the smallest |P| of the byte's eight bits)
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const int lo = (int16_t)(wd[q] & 0xFFFFu), hi = (int16_t)(wd[q] >> 16);
          const int alo = lo < 0 ? -lo : lo, ahi = hi < 0 ? -hi : hi;
          weakest = alo < weakest ? alo : weakest;
          weakest = ahi < weakest ? ahi : weakest;
        }
        rel[c.b.out_off + g] = (uint8_t)(weakest + (syn == 0ull ? 128 : 0));  // syn is wave-uniform
      }
#endif
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
    const int v = ldpc_value<SOFT, RATE>(in, kw, (uint32_t)(LDPC_Z * j + lane), sent);
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
