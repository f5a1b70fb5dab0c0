"""The LDPC coded-link layer's definition as NumPy at any of its four rates, shared by test_ldpc_rates_host.py,
test_gpu_ldpc_rates.py and tools/ldpc_gain.py: ldpc_cases.py with the table as a parameter.  ``code(rate)`` gives the
model of one rate ("1/2", "2/3", "3/4", "5/6"): the base matrix (Z = 64, 24 columns, mb rows), its encoder, the lengths
and block layout over a payload, and the layered normalised min-sum decoder, vectorised over the 64 lanes and over
codewords.  Restates include/ofdm_hip.h ("coded links: LDPC"); everything is integer arithmetic, so a GPU result is
compared by equality.  At rate 1/2 it is ldpc_cases.py (test_ldpc_rates_host.py holds the two against each other)."""
import functools
import struct
import zlib

import numpy as np

Z = 64
COLS = 24
N_BITS = COLS * Z
CW_SENT = N_BITS // 8            # a full codeword on the air: 192 bytes at every rate
MAX_CODED = 4032
MAX_WORDS = 21
DEFAULT_ITERS = 20
HARD = 16                        # a hard bit as a decoder value: +16 / -16
RATES = ("1/2", "2/3", "3/4", "5/6")
RATE_IDS = {r: i for i, r in enumerate(RATES)}
NO_BLOCK = (0, b"", 0, 0, 0)

_ = -1
INFO_SHIFTS = {
    "1/2": (
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
    ),
    "2/3": (
        (_, 1, 61, _, 10, _, _, 43, _, _, 15, _, _, 28, _, _),
        (7, 21, _, 32, _, 25, _, _, _, _, 60, _, 56, _, 16, _),
        (30, _, 37, _, 4, _, 12, _, 58, _, _, 14, _, _, 2, _),
        (34, _, _, 9, _, 4, 47, _, 9, _, _, _, 10, _, 23, _),
        (_, _, _, 14, _, 28, _, 47, _, 58, _, _, 5, _, _, 42),
        (_, 13, 43, _, _, 11, 13, _, _, _, 63, 36, _, 16, _, _),
        (_, 12, _, 61, 57, _, _, _, 0, 19, _, _, _, 35, _, 50),
        (0, _, 29, _, 16, _, _, 21, _, 12, _, 43, _, _, _, 41),
    ),
    "3/4": (
        (40, 21, 5, _, _, 7, 42, _, 18, _, _, 24, 0, _, 5, _, _, 40),
        (0, _, 58, _, 60, 1, 28, _, _, 27, 10, _, 27, _, 40, _, 61, _),
        (_, 1, 39, 26, _, 25, _, 23, 43, _, 29, _, _, 35, _, 52, _, 34),
        (_, 40, _, 13, 7, _, 52, _, _, 21, _, 51, 34, _, _, 2, 42, _),
        (8, _, 21, 37, 47, 6, _, 30, _, 5, _, _, _, 15, 6, _, 3, 36),
        (43, 17, _, 10, 32, _, _, 44, 5, _, 12, 50, _, 5, _, 58, _, _),
    ),
    "5/6": (
        (38, 18, 31, 40, 46, 13, _, 1, 40, 47, 43, _, 16, 0, 29, _, 33, 15, 49, _),
        (14, 30, 51, 26, 63, 0, 14, 0, _, 51, _, 5, 59, 39, _, 2, 27, _, 23, 55),
        (57, 40, 19, 23, _, 9, 34, _, 41, 52, 25, 62, _, _, 41, 7, 22, 0, 40, 27),
        (48, 42, 8, 33, 34, _, 33, 62, 15, _, 17, 30, 48, 59, 0, 61, _, 44, _, 14),
    ),
}
del _
_LANES = np.arange(Z)


def rot(x, s):
    """rot(x, s)[z] = x[(z + s) mod 64] along the last axis."""
    return np.roll(x, -s, axis=-1)


def hard_values(block):
    """A hard byte stream as decoder input: +16 / -16 per bit."""
    bits = np.unpackbits(np.frombuffer(bytes(block), np.uint8)).astype(np.int16)
    return (HARD * (2 * bits - 1)).astype(np.int8)


def flip(block, positions):
    bits = np.unpackbits(np.frombuffer(bytes(block), np.uint8)).copy()
    bits[np.asarray(positions, np.int64)] ^= 1
    return np.packbits(bits).tobytes()


def awgn_values(block, ebn0_db, rate, rng):
    """BPSK over AWGN at Eb/N0 (rate = info bits per sent bit, a number): int8 values rint(4 LLR) clamped to +-127."""
    bits = np.unpackbits(np.frombuffer(bytes(block), np.uint8)).astype(np.float64)
    sigma2 = 1.0 / (2.0 * rate * 10.0 ** (ebn0_db / 10.0))
    y = (2.0 * bits - 1.0) + rng.normal(0.0, np.sqrt(sigma2), len(bits))
    return np.clip(np.rint(4.0 * 2.0 * y / sigma2), -127, 127).astype(np.int8)


class Code:
    """The code of one rate."""

    def __init__(self, rate):
        self.rate = rate
        self.rate_id = RATE_IDS[rate]
        info = np.array(INFO_SHIFTS[rate])
        self.ROWS, self.KB = info.shape                       # mb, kb
        assert self.ROWS + self.KB == COLS
        self.MID = self.ROWS // 2
        self.K_BITS = self.KB * Z
        self.CW_INFO = self.K_BITS // 8                       # KI
        self.CW_PARITY = (N_BITS - self.K_BITS) // 8          # PB
        self.MAX_PAYLOAD = MAX_WORDS * self.CW_INFO - 4
        self.fraction = self.KB / float(COLS)                 # info bits per sent bit of a full codeword
        mb, kb = self.ROWS, self.KB
        H = np.full((mb, COLS), -1, np.int64)
        H[:, :kb] = info
        H[0, kb], H[self.MID, kb], H[mb - 1, kb] = 1, 0, 1
        for i in range(mb - 1):
            H[i, kb + 1 + i] = H[i + 1, kb + 1 + i] = 0
        self.H = H
        # per row: the (column, shift) pairs in column order
        self.ROW_ENTRIES = tuple(tuple((j, int(H[i, j])) for j in range(COLS) if H[i, j] >= 0) for i in range(mb))
        self.N_ENTRIES = sum(len(r) for r in self.ROW_ENTRIES)
        # per row: index into the codeword's bits of every entry and lane, [degree, 64]
        self.ROW_INDEX = tuple(np.array([Z * j + (_LANES + s) % Z for j, s in row]) for row in self.ROW_ENTRIES)

    # ---- the code ----------------------------------------------------------------------------------------------------
    def syndrome(self, bits):
        """bits [..., 1536] -> the mb x 64 check sums [..., mb, 64]."""
        bits = np.asarray(bits, np.uint8)
        out = np.zeros(bits.shape[:-1] + (self.ROWS, Z), np.uint8)
        for i, idx in enumerate(self.ROW_INDEX):
            out[..., i, :] = np.bitwise_xor.reduce(bits[..., idx], axis=-2)
        return out

    def encode_codeword(self, info):
        """64 kb info bits [..., 64 kb] -> the codeword's 1536 bits."""
        info = np.asarray(info, np.uint8)
        mb, kb, H = self.ROWS, self.KB, self.H
        x = info.reshape(info.shape[:-1] + (kb, Z))
        lam = np.zeros(info.shape[:-1] + (mb, Z), np.uint8)
        for i in range(mb):
            for j in range(kb):
                if H[i, j] >= 0:
                    lam[..., i, :] ^= rot(x[..., j, :], int(H[i, j]))
        p = np.zeros_like(lam)
        p[..., 0, :] = np.bitwise_xor.reduce(lam, axis=-2)
        p[..., 1, :] = lam[..., 0, :] ^ rot(p[..., 0, :], 1)
        for i in range(1, mb - 1):
            p[..., i + 1, :] = lam[..., i, :] ^ p[..., i, :]
            if i == self.MID:
                p[..., i + 1, :] ^= p[..., 0, :]
        return np.concatenate([x, p], axis=-2).reshape(info.shape[:-1] + (N_BITS,))

    # ---- lengths and the block layout ----------------------------------------------------------------------------------
    def codewords(self, k):
        return (k + self.CW_INFO - 1) // self.CW_INFO

    def coded_len(self, n):
        """Coded bytes of an n-byte payload, None above MAX_PAYLOAD."""
        if n < 0 or n > self.MAX_PAYLOAD:
            return None
        return (n + 4) + self.CW_PARITY * self.codewords(n + 4)

    def is_block(self, m):
        return self.CW_PARITY + 4 <= m <= MAX_CODED and (m - 1) % CW_SENT >= self.CW_PARITY

    def payload_len(self, m):
        """Payload bytes of a coded block of m bytes, None for a length that is no block."""
        if not self.is_block(m):
            return None
        return m - self.CW_PARITY * ((m + CW_SENT - 1) // CW_SENT) - 4

    def cw_info_lens(self, k):
        """Info bytes of each codeword of a block with k info bytes."""
        return [min(self.CW_INFO, k - self.CW_INFO * w) for w in range(self.codewords(k))]

    def encode(self, payload):
        payload = bytes(payload)
        assert len(payload) <= self.MAX_PAYLOAD
        KI = self.CW_INFO
        info = payload + struct.pack(">I", zlib.crc32(payload) & 0xffffffff)
        kws = self.cw_info_lens(len(info))
        buf = np.zeros((len(kws), KI), np.uint8)
        for w, kw in enumerate(kws):
            buf[w, :kw] = np.frombuffer(info[KI * w:KI * w + kw], np.uint8)
        cw = np.packbits(self.encode_codeword(np.unpackbits(buf, axis=1)), axis=1)
        return b"".join(cw[w, :kw].tobytes() + cw[w, KI:].tobytes() for w, kw in enumerate(kws))

    # ---- decoder -------------------------------------------------------------------------------------------------------
    def decode_codewords(self, v, max_iters=DEFAULT_ITERS):
        """Layered normalised min-sum over codewords at once.  v [W, 1536] ints in [-127, 127] ->
        (bits uint8 [W, 1536], iters int [W], failed bool [W])."""
        v = np.asarray(v, np.int32)
        W = v.shape[0]
        P = v.copy()
        R = [np.zeros((W, len(row), Z), np.int32) for row in self.ROW_ENTRIES]
        bits = np.zeros((W, N_BITS), np.uint8)
        iters = np.zeros(W, np.int64)
        failed = np.ones(W, bool)
        act = np.arange(W)                       # codewords still iterating
        for it in range(1, max_iters + 1):
            if len(act) == 0:
                break
            Pa = P[act]
            for i, idx in enumerate(self.ROW_INDEX):
                d = len(idx)
                Q = np.clip(Pa[:, idx] - R[i][act], -127, 127)          # [A, d, 64]
                beta = Q > 0
                par = np.bitwise_xor.reduce(beta, axis=1)                # [A, 64]
                mag = np.abs(Q)
                two = np.partition(mag, 1, axis=1)[:, :2]                # the two smallest, in order
                m1, m2 = two[:, 0], two[:, 1]
                pos = np.argmin(mag, axis=1)                             # the first entry that holds the smallest
                others = np.where(np.arange(d)[None, :, None] == pos[:, None, :], m2[:, None, :], m1[:, None, :])
                mu = (3 * others) >> 2
                Rn = np.where(par[:, None, :] ^ beta, mu, -mu)
                R[i][act] = Rn
                Pa[:, idx] = Q + Rn
            P[act] = Pa
            x = (Pa > 0).astype(np.uint8)
            bad = self.syndrome(x).reshape(len(act), -1).any(axis=1)
            bits[act] = x
            iters[act] = it
            failed[act] = bad
            act = act[bad]
        return bits, iters, failed

    def block_values(self, v):
        """The values of one block (8 per sent byte) laid out per codeword, [W, 1536]: -128 reads as -127, shortened
        positions are -127.  Returns (V, sent, k) with sent the mask of the positions that were on the air."""
        v = np.maximum(np.asarray(v, np.int8).astype(np.int32), -127)
        m = len(v) // 8
        W = (m + CW_SENT - 1) // CW_SENT
        k = m - self.CW_PARITY * W
        V = np.full((W, N_BITS), -127, np.int32)
        sent = np.zeros((W, N_BITS), bool)
        for w, kw in enumerate(self.cw_info_lens(k)):
            o = 8 * CW_SENT * w
            V[w, :8 * kw] = v[o:o + 8 * kw]
            V[w, self.K_BITS:] = v[o + 8 * kw:o + 8 * kw + 8 * self.CW_PARITY]
            sent[w, :8 * kw] = True
            sent[w, self.K_BITS:] = True
        return V, sent, k

    def _result(self, V, sent, k, bits, iters, failed):
        info = b"".join(np.packbits(bits[w, :8 * kw]).tobytes() for w, kw in enumerate(self.cw_info_lens(k)))
        payload, crc = info[:k - 4], struct.unpack(">I", info[k - 4:])[0]
        corrected = int(np.count_nonzero(sent & (V != 0) & ((V > 0) != (bits != 0))))
        return (int((zlib.crc32(payload) & 0xffffffff) == crc), payload, corrected, int(iters.max()), int(failed.sum()))

    def decode_values(self, v, max_iters=DEFAULT_ITERS):
        """One block from one signed value per sent bit -> (ok, payload, corrected, iters, cw_failed)."""
        return self.decode_many([v], max_iters)[0]

    def decode(self, block, max_iters=DEFAULT_ITERS):
        """One hard block (bytes of any length) -> (ok, payload, corrected, iters, cw_failed)."""
        block = bytes(block)
        if not self.is_block(len(block)):
            return NO_BLOCK
        return self.decode_values(hard_values(block), max_iters)

    def decode_many(self, values, max_iters=DEFAULT_ITERS):
        """decode_values over a list of blocks with all their codewords in one vectorised pass."""
        out = [None] * len(values)
        parts = []
        for i, v in enumerate(values):
            v = np.asarray(v, np.int8)
            if len(v) % 8 or not self.is_block(len(v) // 8):
                out[i] = NO_BLOCK
            else:
                parts.append((i,) + self.block_values(v))
        if not parts:
            return out
        bits, iters, failed = self.decode_codewords(np.concatenate([p[1] for p in parts]), max_iters)
        o = 0
        for i, V, sent, k in parts:
            W = len(V)
            out[i] = self._result(V, sent, k, bits[o:o + W], iters[o:o + W], failed[o:o + W])
            o += W
        return out

    def awgn_values(self, block, ebn0_db, rng):
        """awgn_values at this code's nominal rate kb / 24."""
        return awgn_values(block, ebn0_db, self.fraction, rng)


@functools.lru_cache(maxsize=None)
def code(rate):
    return Code(rate)
