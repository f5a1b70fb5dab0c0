"""The LDPC coded-link layer's definition as NumPy, shared by test_ldpc_host.py and test_gpu_ldpc.py: the rate-1/2
quasi-cyclic code (Z = 64, 12 x 24 base matrix, n = 1536, k = 768), its encoder, the block layout over a payload and the
layered normalised min-sum decoder, vectorised over the 64 lanes and over codewords.  Restates include/ofdm_hip.h
("coded links: LDPC"); everything is integer arithmetic, so a GPU result is compared by equality."""
import struct
import zlib

import numpy as np

Z = 64
ROWS, COLS = 12, 24
N_BITS, K_BITS = COLS * Z, (COLS - ROWS) * Z
CW_INFO = K_BITS // 8            # 96 info bytes per codeword
CW_PARITY = (N_BITS - K_BITS) // 8
MAX_PAYLOAD = 2012
MAX_CODED = 4032
DEFAULT_ITERS = 20
HARD = 16                        # a hard bit as a decoder value: +16 / -16

_ = -1
INFO_SHIFTS = (
    (_, 1, _, _, 25, _, _, 42, _, 59, _, 24),
    (_, _, _, 17, 48, _, _, _, 37, _, 21, 42),
    (2, _, _, _, _, _, 0, _, 56, _, 20, 50),
    (_, 52, _, _, _, 5, _, _, 45, 19, 45, _),
    (_, _, 34, _, _, _, 30, _, 29, 31, _, 55),
    (17, _, _, _, _, _, 5, _, 53, _, 21, 36),
    (_, _, _, _, _, _, 25, 16, _, 22, _, _),
    (_, _, 38, _, _, 54, _, 48, _, 56, 3, _),
    (_, 58, _, _, _, _, _, 7, 60, 36, _, 20),
    (_, _, _, 59, 35, _, _, _, _, 46, 38, 25),
    (40, _, _, 42, _, _, _, _, 24, 33, 16, _),
    (_, _, 46, _, _, 1, _, _, 51, _, 25, 5),
)
del _


def base_matrix():
    """The 12 x 24 table of shifts, -1 where there is no entry."""
    H = np.full((ROWS, COLS), -1, np.int64)
    H[:, :12] = np.array(INFO_SHIFTS)
    H[0, 12], H[6, 12], H[11, 12] = 1, 0, 1
    for i in range(11):
        H[i, 13 + i] = H[i + 1, 13 + i] = 0
    return H


H = base_matrix()
# per row: the (column, shift) pairs in column order
ROW_ENTRIES = tuple(tuple((j, int(H[i, j])) for j in range(COLS) if H[i, j] >= 0) for i in range(ROWS))
N_ENTRIES = sum(len(r) for r in ROW_ENTRIES)
_LANES = np.arange(Z)
# per row: index into the codeword's bits of every entry and lane, [degree, 64]
ROW_INDEX = tuple(np.array([Z * j + (_LANES + s) % Z for j, s in row]) for row in ROW_ENTRIES)


def rot(x, s):
    """rot(x, s)[z] = x[(z + s) mod 64] along the last axis."""
    return np.roll(x, -s, axis=-1)


def syndrome(bits):
    """bits [..., 1536] -> the 12 x 64 check sums [..., 12, 64]."""
    bits = np.asarray(bits, np.uint8)
    out = np.zeros(bits.shape[:-1] + (ROWS, Z), np.uint8)
    for i, idx in enumerate(ROW_INDEX):
        out[..., i, :] = np.bitwise_xor.reduce(bits[..., idx], axis=-2)
    return out


def encode_codeword(info):
    """768 info bits [..., 768] -> the codeword's 1536 bits."""
    info = np.asarray(info, np.uint8)
    x = info.reshape(info.shape[:-1] + (12, Z))
    lam = np.zeros_like(x)
    for i in range(ROWS):
        for j in range(12):
            if H[i, j] >= 0:
                lam[..., i, :] ^= rot(x[..., j, :], int(H[i, j]))
    p = np.zeros_like(x)
    p[..., 0, :] = np.bitwise_xor.reduce(lam, axis=-2)
    p[..., 1, :] = lam[..., 0, :] ^ rot(p[..., 0, :], 1)
    for i in range(1, 11):
        p[..., i + 1, :] = lam[..., i, :] ^ p[..., i, :]
        if i == 6:
            p[..., i + 1, :] ^= p[..., 0, :]
    return np.concatenate([x, p], axis=-2).reshape(info.shape[:-1] + (N_BITS,))


# ---- lengths and the block layout ------------------------------------------------------------------------------------
def codewords(k):
    return (k + CW_INFO - 1) // CW_INFO


def coded_len(n):
    """Coded bytes of an n-byte payload, None above MAX_PAYLOAD."""
    if n < 0 or n > MAX_PAYLOAD:
        return None
    return (n + 4) + CW_PARITY * codewords(n + 4)


def is_block(m):
    return 100 <= m <= MAX_CODED and (m - 1) % 192 >= 96


def payload_len(m):
    """Payload bytes of a coded block of m bytes, None for a length that is no block."""
    if not is_block(m):
        return None
    return m - CW_PARITY * ((m + 191) // 192) - 4


def cw_info_lens(k):
    """Info bytes of each codeword of a block with k info bytes."""
    return [min(CW_INFO, k - CW_INFO * w) for w in range(codewords(k))]


def encode(payload):
    payload = bytes(payload)
    assert len(payload) <= MAX_PAYLOAD
    info = payload + struct.pack(">I", zlib.crc32(payload) & 0xffffffff)
    kws = cw_info_lens(len(info))
    buf = np.zeros((len(kws), CW_INFO), np.uint8)
    for w, kw in enumerate(kws):
        buf[w, :kw] = np.frombuffer(info[CW_INFO * w:CW_INFO * w + kw], np.uint8)
    cw = np.packbits(encode_codeword(np.unpackbits(buf, axis=1)), axis=1)
    return b"".join(cw[w, :kw].tobytes() + cw[w, CW_INFO:].tobytes() for w, kw in enumerate(kws))


def hard_values(block):
    """A hard byte stream as decoder input: +16 / -16 per bit."""
    bits = np.unpackbits(np.frombuffer(bytes(block), np.uint8)).astype(np.int16)
    return (HARD * (2 * bits - 1)).astype(np.int8)


def flip(block, positions):
    bits = np.unpackbits(np.frombuffer(bytes(block), np.uint8)).copy()
    bits[np.asarray(positions, np.int64)] ^= 1
    return np.packbits(bits).tobytes()


# ---- decoder -----------------------------------------------------------------------------------------------------------
def decode_codewords(v, max_iters=DEFAULT_ITERS):
    """Layered normalised min-sum over codewords at once.  v [W, 1536] ints in [-127, 127] ->
    (bits uint8 [W, 1536], iters int [W], failed bool [W])."""
    v = np.asarray(v, np.int32)
    W = v.shape[0]
    P = v.copy()
    R = [np.zeros((W, len(row), Z), np.int32) for row in ROW_ENTRIES]
    bits = np.zeros((W, N_BITS), np.uint8)
    iters = np.zeros(W, np.int64)
    failed = np.ones(W, bool)
    act = np.arange(W)                       # codewords still iterating
    for it in range(1, max_iters + 1):
        if len(act) == 0:
            break
        Pa = P[act]
        for i, idx in enumerate(ROW_INDEX):
            d = len(idx)
            Q = np.clip(Pa[:, idx] - R[i][act], -127, 127)          # [A, d, 64]
            beta = Q > 0
            par = np.bitwise_xor.reduce(beta, axis=1)                # [A, 64]
            mag = np.abs(Q)
            order = np.sort(mag, axis=1)
            m1, m2 = order[:, 0], order[:, 1]
            pos = np.argmin(mag, axis=1)
            others = np.where(np.arange(d)[None, :, None] == pos[:, None, :], m2[:, None, :], m1[:, None, :])
            mu = (3 * others) >> 2
            Rn = np.where(par[:, None, :] ^ beta, mu, -mu)
            R[i][act] = Rn
            Pa[:, idx] = Q + Rn
        P[act] = Pa
        x = (Pa > 0).astype(np.uint8)
        bad = syndrome(x).reshape(len(act), -1).any(axis=1)
        bits[act] = x
        iters[act] = it
        failed[act] = bad
        act = act[bad]
    return bits, iters, failed


def block_values(v):
    """The values of one block (8 per sent byte) laid out per codeword, [W, 1536]: -128 reads as -127, shortened
    positions are -127.  Returns (V, sent) with sent the mask of the positions that were on the air."""
    v = np.maximum(np.asarray(v, np.int8).astype(np.int32), -127)
    m = len(v) // 8
    W = (m + 191) // 192
    k = m - CW_PARITY * W
    V = np.full((W, N_BITS), -127, np.int32)
    sent = np.zeros((W, N_BITS), bool)
    for w, kw in enumerate(cw_info_lens(k)):
        o = 8 * 192 * w
        V[w, :8 * kw] = v[o:o + 8 * kw]
        V[w, K_BITS:] = v[o + 8 * kw:o + 8 * kw + 8 * CW_PARITY]
        sent[w, :8 * kw] = True
        sent[w, K_BITS:] = True
    return V, sent, k


NO_BLOCK = (0, b"", 0, 0, 0)


def decode_values(v, max_iters=DEFAULT_ITERS):
    """One block from one signed value per sent bit -> (ok, payload, corrected, iters, cw_failed)."""
    v = np.asarray(v, np.int8)
    if len(v) % 8 or not is_block(len(v) // 8):
        return NO_BLOCK
    V, sent, k = block_values(v)
    bits, iters, failed = decode_codewords(V, max_iters)
    info = b"".join(np.packbits(bits[w, :8 * kw]).tobytes() for w, kw in enumerate(cw_info_lens(k)))
    payload, crc = info[:k - 4], struct.unpack(">I", info[k - 4:])[0]
    corrected = int(np.count_nonzero(sent & (V != 0) & ((V > 0) != (bits != 0))))
    return (int((zlib.crc32(payload) & 0xffffffff) == crc), payload, corrected, int(iters.max()), int(failed.sum()))


def decode(block, max_iters=DEFAULT_ITERS):
    """One hard block (bytes of any length) -> (ok, payload, corrected, iters, cw_failed)."""
    block = bytes(block)
    if not is_block(len(block)):
        return NO_BLOCK
    return decode_values(hard_values(block), max_iters)


def decode_many(values, max_iters=DEFAULT_ITERS):
    """decode_values over a list of blocks with all their codewords in one vectorised pass."""
    out = [None] * len(values)
    parts = []
    for i, v in enumerate(values):
        v = np.asarray(v, np.int8)
        if len(v) % 8 or not is_block(len(v) // 8):
            out[i] = NO_BLOCK
        else:
            parts.append((i,) + block_values(v))
    if not parts:
        return out
    bits, iters, failed = decode_codewords(np.concatenate([p[1] for p in parts]), max_iters)
    o = 0
    for i, V, sent, k in parts:
        W = len(V)
        b, it, f = bits[o:o + W], iters[o:o + W], failed[o:o + W]
        o += W
        info = b"".join(np.packbits(b[w, :8 * kw]).tobytes() for w, kw in enumerate(cw_info_lens(k)))
        payload, crc = info[:k - 4], struct.unpack(">I", info[k - 4:])[0]
        corrected = int(np.count_nonzero(sent & (V != 0) & ((V > 0) != (b != 0))))
        out[i] = (int((zlib.crc32(payload) & 0xffffffff) == crc), payload, corrected, int(it.max()), int(f.sum()))
    return out


# ---- the AWGN channel of the coding-gain measurement (BPSK, values = rint(4 LLR)) ---------------------------------------
def awgn_values(block, ebn0_db, rate, rng):
    """BPSK over AWGN at Eb/N0 (rate = info bits per sent bit): int8 values rint(4 LLR) clamped to +-127."""
    bits = np.unpackbits(np.frombuffer(bytes(block), np.uint8)).astype(np.float64)
    sigma2 = 1.0 / (2.0 * rate * 10.0 ** (ebn0_db / 10.0))
    y = (2.0 * bits - 1.0) + rng.normal(0.0, np.sqrt(sigma2), len(bits))
    return np.clip(np.rint(4.0 * 2.0 * y / sigma2), -127, 127).astype(np.int8)
