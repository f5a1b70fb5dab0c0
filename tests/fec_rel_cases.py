"""The soft-output decoder's definition as NumPy, on top of fec_cases: the forward and backward sweeps over the 64 states,
the per-bit metric gap Delta and the per-byte reliability q.  Restates include/ofdm_hip.h ("coded links, reliabilities
out"); everything is integer arithmetic, so a GPU result is compared with array_equal.  forced_alternative() is a second,
independent route to the same number (a Viterbi run with one bit forbidden) used only to check the first, and chain()
is the concatenated link on the CPU: RS block, inner encoder, BPSK over AWGN, both outer decoders."""
import struct
import zlib

import numpy as np

import fec_cases as fc
import punct_cases as pc
import rs_cases as rc
import rs_rel_cases as rr

_S = np.arange(64)
_N0 = (_S & 31) << 1            # successor with input bit 0; the one with input bit 1 is _N0 | 1
_N1 = _N0 | 1
_SIGN = np.where(_S < 32, 1, -1).astype(np.int64)   # a branch out of a state with u[t-6] = 1 has both signs flipped


def _mother(v, C):
    """(n, T, vA, vB) of one block's values, or None for a length that is no block."""
    v = np.asarray(v, np.int8).astype(np.int64)
    if len(v) % 8 or not fc.is_block(len(v) // 8):
        return None
    B = len(v)
    v = np.maximum(v, -127)
    n = (B // 8 - 10) // 2
    T = 8 * (n + 4) + 6
    d = np.empty(B, np.int64)
    d[fc.perm(B, C)] = v
    return n, T, d[0:2 * T:2], d[1:2 * T:2]


def sweeps(v, C=16):
    """(n, T, alpha, beta, u): alpha[t], beta[t] for t = 0 .. T (64 states each) and the decoded bits u[0 .. T), by the
    rule and the traceback of fec_cases.decode_values."""
    n, T, vA, vB = _mother(v, C)
    alpha = np.empty((T + 1, 64), np.int64)
    alpha[0] = fc.UNREACHABLE
    alpha[0, 0] = 0
    dec = np.empty((T, 64), bool)
    for t in range(T):
        bm = fc._SA * vA[t] + fc._SB * vB[t]
        m0 = alpha[t, fc._P0] + bm
        m1 = alpha[t, fc._P1] - bm
        dec[t] = m1 > m0
        alpha[t + 1] = np.where(dec[t], m1, m0)
    u = np.empty(T, np.uint8)
    cur = 0
    for t in range(T - 1, -1, -1):
        u[t] = cur & 1
        cur = (cur >> 1) | (int(dec[t, cur]) << 5)
    beta = np.empty((T + 1, 64), np.int64)
    beta[T] = fc.UNREACHABLE
    beta[T, 0] = 0
    for t in range(T - 1, -1, -1):
        bm = fc._SA * vA[t] + fc._SB * vB[t]          # indexed by the successor s'
        beta[t] = np.maximum(beta[t + 1, _N0] + _SIGN * bm[_N0], beta[t + 1, _N1] + _SIGN * bm[_N1])
    assert np.abs(alpha).max() < 2 ** 31 and np.abs(beta).max() < 2 ** 31       # "no sum leaves int32"
    return n, T, alpha, beta, u


def deltas(v, C=16):
    """(n, u, Delta): Delta_t = M* - A_t(1 - u[t]) for every info bit t < 8 (n + 4)."""
    n, T, alpha, beta, u = sweeps(v, C)
    best = int(alpha[T, 0])
    K = 8 * (n + 4)
    s = alpha[1:K + 1] + beta[1:K + 1]                # row t: alpha_{t+1} + beta_{t+1}
    assert np.abs(s).max() < 2 ** 31
    a = np.stack([s[:, 0::2].max(axis=1), s[:, 1::2].max(axis=1)], axis=1)      # A_t(0), A_t(1)
    t = np.arange(K)
    assert np.array_equal(a[t, u[:K]], np.full(K, best))                        # the decoded path has metric M*
    return n, u, best - a[t, 1 - u[:K]]


def forced_alternative(v, t, C=16):
    """A_t(1 - u[t]) by a Viterbi run of its own that forbids the states with (s' & 1) = u[t] after step t."""
    n, T, vA, vB = _mother(v, C)
    u = sweeps(v, C)[4]
    metric = np.full(64, fc.UNREACHABLE, np.int64)
    metric[0] = 0
    for k in range(T):
        bm = fc._SA * vA[k] + fc._SB * vB[k]
        metric = np.maximum(metric[fc._P0] + bm, metric[fc._P1] - bm)
        if k == t:
            metric[(_S & 1) == int(u[t])] = 4 * fc.UNREACHABLE               # below every path that avoids them
    return int(metric[0])


def decode_values(v, C=16):
    """One block from one signed value per transmitted bit -> (ok, payload, corrected, rel): fec_cases.decode_values's
    three fields and one uint8 per payload byte, q[m] = min(255, min over the byte's bits of Delta / 2)."""
    m = _mother(v, C)
    if m is None:
        return (0, b"", 0, np.zeros(0, np.uint8))
    n, u, d = deltas(v, C)
    info = np.packbits(u[:8 * (n + 4)]).tobytes()
    payload, crc = info[:n], struct.unpack(">I", info[n:])[0]
    dd = np.empty(2 * m[1], np.int64)
    dd[0::2], dd[1::2] = m[2], m[3]
    corrected = int(np.count_nonzero((dd != 0) & ((dd > 0) != (fc.conv(u) != 0))))
    assert (d >= 0).all() and not (d & 1).any()
    q = np.minimum(255, d[:8 * n].reshape(n, 8).min(axis=1) // 2).astype(np.uint8)
    return (int((zlib.crc32(payload) & 0xffffffff) == crc), payload, corrected, q)


def decode(block, C=16):
    """One hard block (bytes of any length) -> (ok, payload, corrected, rel)."""
    block = bytes(block)
    if not fc.is_block(len(block)):
        return (0, b"", 0, np.zeros(0, np.uint8))
    return decode_values(fc.hard_values(block), C)


def decode_values_rate(v, C=16, rate="1/2"):
    """The same at a punctured rate: punct_cases's mother values, then the model above."""
    if rate == "1/2":
        return decode_values(v, C)
    m = pc.mother_values(v, C, rate)
    if m is None:
        return (0, b"", 0, np.zeros(0, np.uint8))
    return decode_values(m, C)


def decode_rate(block, C=16, rate="1/2"):
    block = bytes(block)
    if rate == "1/2":
        return decode(block, C)
    if pc.payload_len(len(block), rate) is None:
        return (0, b"", 0, np.zeros(0, np.uint8))
    return decode_values_rate(fc.hard_values(block), C, rate)


def same(a, b):
    """Two (ok, payload, corrected, rel) results, field by field."""
    return (bool(a[0]) == bool(b[0]) and bytes(a[1]) == bytes(b[1]) and int(a[2]) == int(b[2])
            and np.asarray(a[3]).dtype == np.uint8 and np.array_equal(np.asarray(a[3]), np.asarray(b[3])))


# ---- inputs shared by the host and the GPU tests ------------------------------------------------------------------------
SIZES = (0, 3, 4, 11, 12, 219, 2040)    # T = 8 n + 38: a partial chunk, one nearly full, a tail-only last chunk, three, 256
KINDS = ("flips", "noisy", "zeros", "m128")
_CASES = {}
_MODEL = {}


def case_payload(n):
    return np.random.default_rng(2000 + n).integers(0, 256, n, dtype=np.uint8).tobytes()


def case(n, C, kind):
    """One decoder input: "flips" -> a hard block (bytes) with a few transmitted bits inverted (hard +-1 values tie all
    the time); the other kinds -> int8 values: noisy ones, noisy ones with runs of 0, noisy ones with -128 entries."""
    key = (n, C, kind)
    if key not in _CASES:
        rng = np.random.default_rng([n, C, KINDS.index(kind)])
        blk = fc.encode(case_payload(n), C)
        if kind == "flips":
            _CASES[key] = fc.flip(blk, rng.choice(8 * len(blk), min(3 + n // 8, 40), replace=False))
        else:
            x = fc.hard_values(blk).astype(np.float64)
            v = np.clip(np.rint(24.0 * x + 22.0 * rng.standard_normal(len(x))), -127, 127).astype(np.int8)
            if kind == "zeros":
                for at in rng.integers(0, len(v), 2 + len(v) // 500):
                    v[at:at + int(rng.integers(3, 40))] = 0
            if kind == "m128":
                v[rng.integers(0, 100, len(v)) < 3] = -128
            _CASES[key] = v
    return _CASES[key]


def case_model(n, C, kind):
    """The model's answer to case(n, C, kind), computed once."""
    key = (n, C, kind)
    if key not in _MODEL:
        x = case(n, C, kind)
        _MODEL[key] = decode(x, C) if kind == "flips" else decode_values(x, C)
    return _MODEL[key]


def clean_values(n, C, level):
    """A clean block at |v| = level."""
    return (fc.hard_values(fc.encode(case_payload(n), C)).astype(np.int32) * level).astype(np.int8)


# ---- the concatenated chain on the CPU ---------------------------------------------------------------------------------
def chain_payload(n, seed):
    return np.random.default_rng([seed, n, 1]).integers(0, 256, n, dtype=np.uint8).tobytes()


def chain_values(n, seed, ebn0_db, C=16, scale=32.0):
    """(payload, values): RS block of a seeded n-byte payload, rate-1/2 inner encoder with C columns, BPSK +-1 plus seeded
    Gaussian noise at ``ebn0_db`` (Eb/N0 of the whole concatenated rate), quantised rint(scale * y) clamped to +-127."""
    payload = chain_payload(n, seed)
    return payload, chain_channel(fc.encode(rc.encode(payload), C), n, seed, ebn0_db, scale)


def chain_channel(coded, n, seed, ebn0_db, scale=32.0):
    """The channel of chain_values on a coded block of an n-byte payload, wherever it was encoded."""
    x = fc.hard_values(coded).astype(np.float64)
    rate = 8.0 * n / len(x)
    sigma = np.sqrt(1.0 / (2.0 * rate * 10.0 ** (ebn0_db / 10.0)))
    y = x + sigma * np.random.default_rng([seed, n, 2]).standard_normal(len(x))
    return np.clip(np.rint(scale * y), -127, 127).astype(np.int8)


def chain_decode(values, C=16, M=rr.DEFAULT_M):
    """(inner, plain, with_rel): the inner model's result, rs_cases.decode of its payload, and rs_rel_cases.decode of it
    with the inner decoder's reliabilities."""
    inner = decode_values(values, C)
    return inner, rc.decode(inner[1]), rr.decode(inner[1], inner[3], M)


def chain_outcome(n, seed, ebn0_db, C=16, M=rr.DEFAULT_M):
    """(plain, with_rel, second): whether each outer decoder returned the payload sent, and the second-pass count."""
    payload, values = chain_values(n, seed, ebn0_db, C)
    _, plain, rel = chain_decode(values, C, M)
    return (int(bool(plain[0]) and plain[1] == payload), int(bool(rel[0]) and rel[1] == payload), int(rel[4]))
