"""Decoding with reliabilities, the definition as NumPy: shared by test_rs_rel_host.py and test_gpu_rs_rel.py.  Restates
include/ofdm_hip.h ("outer code, decoding with reliabilities") on top of rs_cases (field, layout, first pass): the
threshold tau* by counting, the erased set J, and then the codeword that differs from the received word in e positions
outside J with 2 e + f <= 32, found without Berlekamp-Massey and without Forney: the error locator of each degree
e = 0, 1, ... by Gaussian elimination over GF(2^8) on the syndromes folded with the erasure locator, its roots by trying
every real position, the errata values by Gaussian elimination on the 32 syndrome equations, and a candidate is accepted
only when the corrected word's 32 syndromes are zero and the count holds: nothing of it is shared with the kernel.
Everything is integer arithmetic, so a GPU result is compared by equality."""
import numpy as np

import rs_cases as rc

DEFAULT_M = 28


# ---- linear algebra over GF(2^8) ---------------------------------------------------------------------------------------
def solve(A, b):
    """One solution x of A x = b (A: m x n integers, b: m), free unknowns 0; None where there is none."""
    A = np.array(A, np.int64).reshape(len(b), -1)
    m, n = A.shape
    aug = np.concatenate([A, np.asarray(b, np.int64).reshape(m, 1)], axis=1)
    piv, row = [], 0
    for col in range(n):
        nz = np.flatnonzero(aug[row:, col]) if row < m else []
        if len(nz) == 0:
            continue
        r = row + int(nz[0])
        aug[[row, r]] = aug[[r, row]]
        aug[row] = rc.gmul_v(aug[row], rc.ginv(int(aug[row, col])))
        for other in range(m):
            if other != row and aug[other, col]:
                aug[other] ^= rc.gmul_v(aug[row], int(aug[other, col]))
        piv.append(col)
        row += 1
    if aug[row:, n].any():
        return None
    x = np.zeros(n, np.int64)
    for r, col in enumerate(piv):
        x[col] = aug[r, n]
    return x


# ---- the threshold -----------------------------------------------------------------------------------------------------
def threshold(q, M):
    """tau* of reliabilities q (one per real position): the largest tau in 0 .. 254 with #{q <= tau} <= M, None where
    there is none (c(0) > M) or nothing would be erased (c(tau*) = 0)."""
    q = np.asarray(q, np.int64)
    best = None
    for tau in range(255):
        if int((q <= tau).sum()) <= M:
            best = tau
    if best is None or int((q <= best).sum()) == 0:
        return None
    return best


def erased(q, M):
    """The erased positions J (ascending), empty where there is no second pass."""
    tau = threshold(q, M)
    return np.zeros(0, np.int64) if tau is None else np.flatnonzero(np.asarray(q, np.int64) <= tau)


# ---- one codeword ------------------------------------------------------------------------------------------------------
def _locators(n):
    return rc.EXP[np.arange(n - 1, -1, -1) % 255]          # X_p = alpha^(n - 1 - p)


def second_pass(r, J):
    """The codeword that differs from r in e positions outside J with 2 e + |J| <= 32, or None."""
    r = np.asarray(r, np.uint8)
    n, f = len(r), len(J)
    if f == 0 or f > rc.PARITY:
        return None
    S = [int(s) for s in rc.syndromes(r)]
    X = _locators(n)
    gam = [1]                                               # Gamma(x) = prod (1 + X_j x), lowest degree first
    for p in J:
        xj = int(X[p])
        gam = [u ^ rc.gmul(v, xj) for u, v in zip(gam + [0], [0] + gam)]
    # folded syndromes: T_k = sum_j Gamma_j S_(k + f - j), k = 0 .. 31 - f; an error locator of degree e generates them
    T = []
    for k in range(rc.PARITY - f):
        t = 0
        for j in range(f + 1):
            t ^= rc.gmul(gam[j], S[k + f - j])
        T.append(t)
    inJ = np.zeros(n, bool)
    inJ[J] = True
    for e in range((rc.PARITY - f) // 2 + 1):
        # Lambda_1 .. Lambda_e with sum_{j = 1 .. e} Lambda_j T_(k + e - j) = T_(k + e) for every k the T reach
        rows = [[T[k + e - j] for j in range(1, e + 1)] for k in range(len(T) - e)]
        lam = solve(rows, [T[k + e] for k in range(len(T) - e)]) if e else (np.zeros(0, np.int64) if not any(T) else None)
        if lam is None:
            continue
        coef = [1] + [int(c) for c in lam]
        where = [p for p in range(n) if not inJ[p] and rc.poly_eval(coef[::-1], rc.ginv(int(X[p]))) == 0]
        if len(where) != e:
            continue
        pos = np.concatenate([np.asarray(J, np.int64), np.asarray(where, np.int64)])
        A = [[int(rc.EXP[(rc.LOG[int(X[p])] * i) % 255]) for p in pos] for i in range(rc.PARITY)]
        Y = solve(A, S)
        if Y is None:
            continue
        out = r.copy()
        out[pos] ^= Y.astype(np.uint8)
        outside = int((out != r)[~inJ].sum())
        if not rc.syndromes(out).any() and 2 * outside + f <= rc.PARITY:
            return out
    return None


def decode_cw(r, q, M=DEFAULT_M):
    """One received word and its reliabilities -> (word, corrected, failed, second)."""
    word, c, failed = rc.decode_cw(r)
    if not failed or q is None or M == 0:
        return word, c, failed, 0
    J = erased(q, M)
    out = second_pass(r, J)
    if out is None:
        return np.asarray(r, np.uint8), 0, 1, 0
    return out, int((out != np.asarray(r, np.uint8)).sum()), 0, 1


def decode(block, rel=None, M=DEFAULT_M):
    """One received block and one reliability byte per byte of it -> (ok, payload, corrected, failed, second)."""
    import struct
    import zlib
    block = bytes(block)
    n = rc.payload_len(len(block))
    if n is None:
        return (0, b"", 0, 0, 0)
    if rel is None or M == 0:
        return rc.decode(block) + (0,)
    q = np.frombuffer(bytes(rel), np.uint8) if isinstance(rel, (bytes, bytearray)) else np.asarray(rel, np.uint8)
    assert len(q) == len(block)
    k = n + 4
    buf = np.frombuffer(block, np.uint8).copy()
    corrected = failed = second = 0
    for w in range(rc.words(k)):
        pos = rc.positions(k, w)
        word, c, f, s = decode_cw(buf[pos], q[pos], M)
        buf[pos] = word
        corrected += c
        failed += f
        second += s
    payload = buf[:n].tobytes()
    crc = struct.unpack(">I", buf[n:k].tobytes())[0]
    return (int((zlib.crc32(payload) & 0xffffffff) == crc), payload, corrected, failed, second)


# ---- reliabilities from soft values ------------------------------------------------------------------------------------
def rel_from_values(values):
    """min |v| over the eight values of each byte, -128 read as 127, one Python integer at a time."""
    v = [int(x) for x in np.asarray(values, np.int8).reshape(-1)]
    assert len(v) % 8 == 0
    out = []
    for m in range(len(v) // 8):
        out.append(min(127 if x == -128 else abs(x) for x in v[8 * m:8 * m + 8]))
    return np.array(out, np.uint8)


# ---- damage with reliabilities -----------------------------------------------------------------------------------------
def spoil(block, w, f, e, rng, M=DEFAULT_M, erase_good=0, pin=()):
    """Codeword w of the block with e wrong symbols of reliability 200 and f symbols of reliability 0, of which
    ``erase_good`` stay correct and the others are wrong; ``pin``: symbol indices (negative from the end) that must be
    among the erased ones.  Every other symbol has reliability 200.  Returns (block, rel, erased symbol indices)."""
    k = rc.payload_len(len(block)) + 4
    pos = rc.positions(k, w)
    n = len(pos)
    pin = [p % n for p in pin]
    rest = [p for p in rng.permutation(n) if p not in pin]
    J = np.array(pin + rest[:f - len(pin)], np.int64)
    E = np.array(rest[f - len(pin):f - len(pin) + e], np.int64)
    wrong = np.concatenate([J[:len(J) - erase_good], E])
    out = rc.damage(block, pos[wrong], rng)
    rel = np.full(len(block), 200, np.uint8)
    rel[pos[J]] = 0
    return out, rel, np.sort(J)


# ---- the impaired link -------------------------------------------------------------------------------------------------
def link_on_the_cpu(orc, cfg, snr_db, seed=None, M=DEFAULT_M, scale=32.0):
    """The link of soft_cases with RS blocks straight on the transmitter, no inner code: RS blocks of
    soft_cases.link_payloads() -> oracle transmitter -> float64 channel model -> oracle receiver with its taps -> the soft
    model -> reliabilities -> the RS model without and with them.  Returns (plain, withrel) per packet:
    (ok, payload, corrected, failed) and (ok, payload, corrected, failed, second); (None, None) where the receiver's
    packet list is not the six packets, each from a frame of its own."""
    import multipath_cases as mpc
    import soft_cases as sc
    from ofdm_uhd_amd import _abi
    seed = sc.LINK_SEED if seed is None else seed
    pay = sc.link_payloads()
    iq = orc.tx(cfg, [rc.encode(p) for p in pay])
    psig = float(np.mean(np.abs(iq.astype(np.complex128)) ** 2))
    y, _ = mpc.model(sc.link_air(iq), sc.link_channel_cfg(snr_db, psig, seed), 0)
    res = orc.rx(cfg, y.astype(np.complex64), (1 << _abi.TAP_RX_FFT) | (1 << _abi.TAP_RX_SINK) | (1 << _abi.TAP_RX_FRAMES))
    pk = res.packets
    fft, sink, frames = res.tap(_abi.TAP_RX_FFT), res.tap(_abi.TAP_RX_SINK), res.tap(_abi.TAP_RX_FRAMES)
    smap, cst, mask = sc.smap_of(cfg), sc.cst_of(cfg), sc.mask_of(cfg)
    nbits = int(cfg.arity).bit_length() - 1
    if [len(blk) for _, blk in pk] != [rc.coded_len(len(p)) for p in pay] or len(frames) < len(pay):
        return None, None
    pre = np.concatenate([[0], np.cumsum(frames[:, 1].astype(np.int64) + 1)])[:-1]
    row, plain, withrel = 0, [], []
    for k, (ok, blk) in enumerate(pk):
        ns = -(-8 * (sc.HEADER + len(blk) + 4) // (len(smap) * nbits))
        if int(frames[k, 1]) < ns:
            return None, None
        x = sink[row:row + ns, :len(smap)]
        row += ns
        eq = sc.hinv_from_preamble(cfg, fft[pre[k]])
        v = sc.packet_values(x, eq, smap, cst, len(blk), mask, scale)
        plain.append(rc.decode(blk))
        withrel.append(decode(blk, rel_from_values(v), M))
    if row > len(sink):
        return None, None
    return plain, withrel


def link_summary(side, pay):
    """Per packet 0 / 1: decoded to the payload sent."""
    return "".join(str(int(bool(o[0]) and o[1] == p)) for o, p in zip(side, pay))
