// rs_errors_only.inc -- the errors-only pass of the Reed-Solomon decoders (rs.h) over one codeword, from its syndromes
// on: Berlekamp-Massey, Lambda and Omega to every lane, roots, Forney, and the symbols changed in LDS.  Included once
// into k_rs_decode and once into k_rs_decode_rel, inside a block of its own.  The text stands in the kernels and not in
// a __device__ function behind them because k_rs_decode has to stay the code it was: through an inlined function the
// same statements took 131 registers for 127, one resident wave per SIMD less (DESIGN.md section 7).
//
// It sees, of the kernel's codeword loop: S (syndrome S_i in lane i of the half), i, k, W, w, kw, len (0: a half without
// a codeword), blkb.  It sets L, the locator's degree, and good, the verdict: degree 1 .. 16 with L roots found, and
// then the L symbols are changed.
  // ---- Berlekamp-Massey, inversion-free ----
  uint32_t lam = i == 0 ? 1u : 0u, B = lam, gam = 1;
  L = 0;
  for (uint32_t r = 0; r < OFDM_RS_PARITY; r++) {
    uint32_t sv = (uint32_t)__shfl((int)S, (int)((r - i) & 31u), 32);
    sv = i <= r ? sv : 0u;
    const uint32_t d = rs_half_xor(rs_mul(lam, sv));
    uint32_t Bs = (uint32_t)__shfl_up((int)B, 1, 32);
    if (i == 0) Bs = 0;
    const uint32_t T = rs_mul(gam, lam) ^ rs_mul(d, Bs);
    const bool upd = d != 0 && 2u * L <= r;
    B = upd ? lam : Bs;
    gam = upd ? d : gam;
    L = upd ? r + 1u - L : L;
    lam = T;
  }
  // every lane gets Lambda_0 .. Lambda_16 and Omega_0 .. Omega_15 of its half
  uint32_t lm[17], om[16];
#pragma unroll
  for (int j = 0; j < 17; j++) lm[j] = (uint32_t)__shfl((int)lam, j, 32);
  {
    uint32_t acc = 0;  // Omega_i = sum_{j <= i} Lambda_j S_(i - j), in lane i < 16
#pragma unroll
    for (int j = 0; j < 16; j++) {
      const uint32_t sv = (uint32_t)__shfl((int)S, (int)((i - (uint32_t)j) & 31u), 32);
      acc ^= (uint32_t)j <= i ? rs_mul(lm[j], sv) : 0u;
    }
#pragma unroll
    for (int j = 0; j < 16; j++) om[j] = (uint32_t)__shfl((int)acc, j, 32);
  }

  // ---- roots over the real positions, Forney ----
  const bool tryit = L >= 1u && L <= 16u;
  uint32_t err[8], nroot = 0;
#pragma unroll
  for (int q = 0; q < 8; q++) {
    err[q] = 0;
    const uint32_t p = i + 32u * (uint32_t)q;
    if (tryit && p < len) {
      const uint32_t deg = len - 1u - p;                    // the symbol's power of x: X = alpha^deg
      const uint32_t z = rs_tab.exp[deg ? 255u - deg : 0u];  // X^-1
      const RsCols cz = rs_cols(z);
      const RsCols cy = rs_cols(rs_mulc(cz, z));
      uint32_t E = lm[16], O = lm[15];
#pragma unroll
      for (int j = 6; j >= 0; j--) {
        E = rs_mulc(cy, E) ^ lm[2 * j + 2];
        O = rs_mulc(cy, O) ^ lm[2 * j + 1];
      }
      E = rs_mulc(cy, E) ^ lm[0];
      const uint32_t zO = rs_mulc(cz, O);
      if ((E ^ zO) == 0u) {
        nroot++;
        uint32_t v = om[15];
#pragma unroll
        for (int j = 14; j >= 0; j--) v = rs_mulc(cz, v) ^ om[j];
        err[q] = rs_mul(v, rs_inv(zO));
      }
    }
  }
  nroot = rs_half_sum(nroot);
  good = tryit && nroot == L;
  if (good) {
#pragma unroll
    for (int q = 0; q < 8; q++) {
      const uint32_t p = i + 32u * (uint32_t)q;
      if (err[q]) {  // (only where p < len) one writer per byte: position p of codeword w is this lane's alone
        const uint32_t at = p < kw ? p * W + w : k + (p - kw) * W + w;
        blkb[at] = (uint8_t)((uint32_t)blkb[at] ^ err[q]);
      }
    }
  }
