"""The coded-link layer's definition as NumPy, shared by test_fec_host.py and test_gpu_fec.py: the rate-1/2, K = 7
convolutional encoder (133 / 171 octal, 802.11a arrangement), the block interleaver and a full-sequence
maximum-correlation Viterbi decoder, vectorised over the 64 states.  Restates include/ofdm_hip.h ("coded links");
everything is integer arithmetic, so a GPU result is compared with array_equal."""
import struct
import zlib

import numpy as np

MAX_PAYLOAD = 2040
MAX_CODED = 4090
COLS = (1, 2, 4, 8, 16)
TAPS_A = (0, 2, 3, 5, 6)        # A[t] = u[t]^u[t-2]^u[t-3]^u[t-5]^u[t-6]
TAPS_B = (0, 1, 2, 3, 6)        # B[t] = u[t]^u[t-1]^u[t-2]^u[t-3]^u[t-6]
UNREACHABLE = -(1 << 29)        # below every reachable metric (|metric| <= 2 * 16358 * 127)


def coded_len(n):
    return 2 * n + 10


def is_block(m):
    return m % 2 == 0 and 10 <= m <= MAX_CODED


def conv(u):
    """Info bits (tail included) -> interleaved-by-two coded bits c[2t] = A[t], c[2t+1] = B[t]."""
    u = np.asarray(u, np.uint8)
    T = len(u)
    z = np.concatenate([np.zeros(6, np.uint8), u])
    a = np.zeros(T, np.uint8)
    b = np.zeros(T, np.uint8)
    for k in TAPS_A:
        a ^= z[6 - k:6 - k + T]
    for k in TAPS_B:
        b ^= z[6 - k:6 - k + T]
    c = np.empty(2 * T, np.uint8)
    c[0::2], c[1::2] = a, b
    return c


def perm(B, C):
    """Index into the coded bits of every transmitted bit: sent[j] = c[perm[j]]."""
    R = B // C
    j = np.arange(B)
    return (j % R) * C + j // R


def info_bits(payload):
    info = bytes(payload) + struct.pack(">I", zlib.crc32(bytes(payload)) & 0xffffffff)
    return np.concatenate([np.unpackbits(np.frombuffer(info, np.uint8)), np.zeros(6, np.uint8)])


def encode(payload, C=16):
    payload = bytes(payload)
    assert len(payload) <= MAX_PAYLOAD and C in COLS
    c = np.concatenate([conv(info_bits(payload)), np.zeros(4, np.uint8)])
    assert len(c) == 16 * len(payload) + 80
    return np.packbits(c[perm(len(c), C)]).tobytes()


def hard_values(block):
    """A hard byte stream as decoder input: +1 / -1 per bit."""
    bits = np.unpackbits(np.frombuffer(bytes(block), np.uint8))
    return (2 * bits.astype(np.int8) - 1).astype(np.int8)


# per state s' (bit k = u[t-k] of the step's register once the input bit is in): sign of A and B on the branch from
# the predecessor with u[t-6] = 0; the other branch flips both (both generators tap u[t-6])
_S = np.arange(64)
_SA = np.array([2 * (sum((s >> k) & 1 for k in TAPS_A if k < 6) & 1) - 1 for s in _S], np.int32)
_SB = np.array([2 * (sum((s >> k) & 1 for k in TAPS_B if k < 6) & 1) - 1 for s in _S], np.int32)
_P0 = _S >> 1
_P1 = _P0 | 32


def decode_values(v, C=16):
    """One block from one signed value per transmitted bit -> (ok, payload, corrected)."""
    v = np.asarray(v, np.int8).astype(np.int32)
    if len(v) % 8 or not is_block(len(v) // 8):
        return (0, b"", 0)
    B = len(v)
    v = np.maximum(v, -127)
    n = (B // 8 - 10) // 2
    T = 8 * (n + 4) + 6
    d = np.empty(B, np.int32)
    d[perm(B, C)] = v                      # deinterleave: d[i] belongs to coded bit i
    vA, vB = d[0:2 * T:2], d[1:2 * T:2]
    metric = np.full(64, UNREACHABLE, np.int32)
    metric[0] = 0
    dec = np.empty((T, 64), bool)
    for t in range(T):
        bm = _SA * vA[t] + _SB * vB[t]
        m0 = metric[_P0] + bm
        m1 = metric[_P1] - bm
        dec[t] = m1 > m0                   # strictly larger only: a tie keeps the predecessor with u[t-6] = 0
        metric = np.where(dec[t], m1, m0)
    u = np.empty(T, np.uint8)
    cur = 0
    for t in range(T - 1, -1, -1):
        u[t] = cur & 1
        cur = (cur >> 1) | (int(dec[t, cur]) << 5)
    info = np.packbits(u[:8 * (n + 4)]).tobytes()
    payload, crc = info[:n], struct.unpack(">I", info[n:])[0]
    c = conv(u)
    dd = d[:2 * T]
    corrected = int(np.count_nonzero((dd != 0) & ((dd > 0) != (c != 0))))
    return (int((zlib.crc32(payload) & 0xffffffff) == crc), payload, corrected)


def decode(block, C=16):
    """One hard block (bytes of any length) -> (ok, payload, corrected)."""
    block = bytes(block)
    if not is_block(len(block)):
        return (0, b"", 0)
    return decode_values(hard_values(block), C)


def flip(block, positions):
    """The block with the transmitted bits at ``positions`` inverted."""
    bits = np.unpackbits(np.frombuffer(bytes(block), np.uint8)).copy()
    bits[np.asarray(positions, np.int64)] ^= 1
    return np.packbits(bits).tobytes()
