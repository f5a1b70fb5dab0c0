"""The outer code's definition as NumPy, shared by test_rs_host.py and test_gpu_rs.py.  Restates include/ofdm_hip.h
("outer code"): GF(2^8) modulo 0x11d with alpha = 2, g(x) = prod_{i=0..31} (x - alpha^i), blocks of k = n + 4 info
bytes (payload | CRC-32 big-endian) byte-interleaved over W = ceil(k / 223) shortened RS(255, 223) codewords, parity
byte j of codeword w at k + j W + w, and bounded-distance decoding per codeword.  The model works on log / antilog
tables, divides by a generator matrix, runs the textbook Berlekamp-Massey with inverses and accepts a correction only
after evaluating the corrected word's 32 syndromes again: nothing of it is shared with the kernels.  Everything is
integer arithmetic, so a GPU result is compared by equality."""
import functools
import struct
import zlib

import numpy as np

PARITY = 32
T = 16
MAX_PAYLOAD = 3564
MAX_CODED = 4080
SIZES = (0, 1, 3, 218, 219, 220, 221, 442, 443, 1780, 3564)     # k = 223 / 224 / 225, one -> two codewords, uneven splits

# ---- the field --------------------------------------------------------------------------------------------------------
EXP = np.zeros(512, np.int64)
LOG = np.zeros(256, np.int64)
_v = 1
for _e in range(255):
    EXP[_e] = _v
    LOG[_v] = _e
    _v <<= 1
    if _v & 0x100:
        _v ^= 0x11d
EXP[255:510] = EXP[0:255]


def gmul(a, b):
    return 0 if a == 0 or b == 0 else int(EXP[LOG[a] + LOG[b]])


def ginv(a):
    assert a != 0
    return int(EXP[255 - LOG[a]])


def gmul_v(a, b):
    """Element-wise product of two integer arrays (broadcasting)."""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    return np.where((a == 0) | (b == 0), 0, EXP[LOG[a] + LOG[b]])


def poly_eval(p, x):
    """p[0] is the HIGHEST-degree coefficient."""
    y = 0
    for c in p:
        y = gmul(y, x) ^ int(c)
    return y


def _generator():
    g = [1]
    for i in range(PARITY):                    # times (x + alpha^i)
        a = int(EXP[i])
        g = [u ^ gmul(v, a) for u, v in zip(g + [0], [0] + g)]
    return g                                   # 33 coefficients, highest degree first, g[0] = 1


GEN = _generator()


@functools.lru_cache(maxsize=None)
def _parity_matrix():
    """Row r: the parity of the message that is 1 at symbol r of a full-length (223-symbol) word and 0 elsewhere,
    found by long division of x^(222 - r + 32) by g."""
    P = np.zeros((223, PARITY), np.int64)
    rem = [0] * PARITY
    rem[-1] = 1                                # x^0 ... then times x, 32 + 222 times
    rows = []
    for e in range(PARITY + 223):
        if e >= PARITY:
            rows.append(list(rem))             # x^e mod g, highest degree (x^31) first
        top = rem[0]
        rem = rem[1:] + [0]
        if top:
            rem = [c ^ gmul(top, gc) for c, gc in zip(rem, GEN[1:])]
    for r in range(223):
        P[r] = rows[222 - r]
    return P


def parity_of(msg):
    """The 32 parity bytes of one (shortened) message: byte j is the coefficient of x^(31 - j) of m(x) x^32 mod g(x)."""
    msg = np.asarray(msg, np.int64)
    assert 1 <= len(msg) <= 223
    P = _parity_matrix()[223 - len(msg):]
    return np.bitwise_xor.reduce(gmul_v(msg[:, None], P), axis=0).astype(np.uint8)


# ---- block layout -----------------------------------------------------------------------------------------------------
def words(k):
    return -(-k // 223)


def block_len(k):
    return k + PARITY * words(k)


def coded_len(n):
    assert 0 <= n <= MAX_PAYLOAD
    return block_len(n + 4)


@functools.lru_cache(maxsize=None)
def length_table():
    """{f(k): n} over every payload length."""
    return {block_len(n + 4): n for n in range(MAX_PAYLOAD + 1)}


def payload_len(m):
    """n of a block of m bytes, None for a length that is no block."""
    return length_table().get(m)


def cw_info(k, W, w):
    return -(-(k - w) // W)


def positions(k, w):
    """Where the symbols of codeword w lie in a block of k info bytes, first symbol first."""
    W = words(k)
    kw = cw_info(k, W, w)
    return np.concatenate([np.arange(kw) * W + w, k + np.arange(PARITY) * W + w])


def info_bytes(payload):
    payload = bytes(payload)
    return payload + struct.pack(">I", zlib.crc32(payload) & 0xffffffff)


def encode(payload):
    info = np.frombuffer(info_bytes(payload), np.uint8)
    k = len(info)
    W = words(k)
    out = np.zeros(block_len(k), np.uint8)
    out[:k] = info
    for w in range(W):
        pos = positions(k, w)
        out[pos[-PARITY:]] = parity_of(info[w::W])
    return out.tobytes()


# ---- decoding -----------------------------------------------------------------------------------------------------------
def syndromes(cw):
    """S_i = r(alpha^i), i = 0 .. 31, by direct evaluation of the polynomial (first symbol = highest degree)."""
    cw = np.asarray(cw, np.int64)
    deg = np.arange(len(cw) - 1, -1, -1)
    i = np.arange(PARITY)
    terms = np.where(cw[:, None] == 0, 0, EXP[(LOG[cw][:, None] + deg[:, None] * i[None, :]) % 255])
    return np.bitwise_xor.reduce(terms, axis=0)


def decode_cw(r):
    """One received word (k_w + 32 symbols) -> (word, corrected, failed).  Bounded distance: the codeword within 16
    symbol differences if there is one, else the received symbols and failed = 1."""
    r = np.asarray(r, np.uint8)
    n = len(r)
    S = [int(s) for s in syndromes(r)]
    if not any(S):
        return r, 0, 0
    # Berlekamp-Massey (Massey 1969): C the connection polynomial, lowest degree first
    Cp, Bp, L, m, b = [1], [1], 0, 1, 1
    for i in range(PARITY):
        d = S[i]
        for j in range(1, L + 1):
            if j < len(Cp):
                d ^= gmul(Cp[j], S[i - j])
        if d == 0:
            m += 1
            continue
        coef = gmul(d, ginv(b))
        Tp = list(Cp)
        Cp = Cp + [0] * max(0, len(Bp) + m - len(Cp))
        for j, c in enumerate(Bp):
            Cp[j + m] ^= gmul(coef, c)
        if 2 * L <= i:
            L, Bp, b, m = i + 1 - L, Tp, d, 1
        else:
            m += 1
    fail = (r, 0, 1)
    if L > T:
        return fail
    lam = (Cp + [0] * (L + 1))[:L + 1]
    if lam[L] == 0:
        return fail
    # roots among the real positions only: position p has X = alpha^(n - 1 - p)
    deg = np.arange(n - 1, -1, -1)
    val = np.zeros(n, np.int64)
    for j, c in enumerate(lam):                         # Lambda(X^-1) = sum c_j alpha^(-j deg)
        if c:
            val ^= EXP[(LOG[c] - j * deg) % 255]
    where = np.flatnonzero(val == 0)
    if len(where) != L:
        return fail
    omega = [0] * L                                     # S(x) Lambda(x) mod x^L
    for a in range(L):
        for j in range(a + 1):
            omega[a] ^= gmul(lam[j], S[a - j])
    out = r.copy()
    for p in where:
        X = int(EXP[deg[p] % 255])
        z = ginv(X)
        num = poly_eval(omega[::-1], z)
        den = 0                                         # Lambda'(z) = sum over odd j of c_j z^(j-1)
        for j in range(1, L + 1, 2):
            den ^= gmul(lam[j], int(EXP[(LOG[z] * (j - 1)) % 255]))
        if den == 0:
            return fail
        e = gmul(gmul(X, num), ginv(den))               # first root alpha^0: e = X Omega(z) / Lambda'(z)
        if e == 0:
            return fail
        out[p] ^= e
    if syndromes(out).any():                            # the definition's own test: it must BE a codeword
        return fail
    return out, L, 0


def decode(block):
    """One received block (bytes of any length) -> (ok, payload, corrected, failed)."""
    block = bytes(block)
    n = payload_len(len(block))
    if n is None:
        return (0, b"", 0, 0)
    k = n + 4
    buf = np.frombuffer(block, np.uint8).copy()
    corrected = failed = 0
    for w in range(words(k)):
        pos = positions(k, w)
        word, c, f = decode_cw(buf[pos])
        buf[pos] = word
        corrected += c
        failed += f
    payload = buf[:n].tobytes()
    crc = struct.unpack(">I", buf[n:k].tobytes())[0]
    return (int((zlib.crc32(payload) & 0xffffffff) == crc), payload, corrected, failed)


# ---- damage -------------------------------------------------------------------------------------------------------------
def damage(block, where, rng=None, xor=None):
    """The block with the bytes at ``where`` changed: XOR with ``xor`` (one value or one per position), or with random
    non-zero values."""
    b = np.frombuffer(bytes(block), np.uint8).copy()
    where = np.asarray(where, np.int64)
    if xor is None:
        xor = rng.integers(1, 256, len(where))
    b[where] ^= np.asarray(xor, np.uint8)
    return b.tobytes()


def errors_per_codeword(block, count, rng):
    """``count`` wrong symbols in every codeword of the block, at random places."""
    k = payload_len(len(block)) + 4
    where = np.concatenate([rng.choice(positions(k, w), count, replace=False) for w in range(words(k))])
    return damage(block, where, rng)


def miscorrection(block, w=0, seed=0):
    """The constructed miscorrection on codeword w: the weight-33 codeword 0 ... 0 1 | g_1 ... g_32 (the generator itself,
    on the last info symbol and the parity) has 33 non-zero symbols; adding 17 of them to a sent codeword leaves a word
    16 symbols from ANOTHER codeword (sent + that one), which a bounded-distance decoder must return."""
    k = payload_len(len(block)) + 4
    pos = positions(k, w)[-33:]
    assert all(GEN)                                     # every coefficient of g is non-zero: weight 33
    pick = np.sort(np.random.default_rng(seed).choice(33, 17, replace=False))
    return damage(block, pos[pick], xor=np.asarray(GEN, np.uint8)[pick]), damage(block, pos, xor=np.asarray(GEN, np.uint8))


# ---- the impaired link ------------------------------------------------------------------------------------------------
def link_on_the_cpu(orc, cfg, snr_db, rate, seed=None, scale=32.0):
    """punct_cases.link_on_the_cpu with the outer code around the payloads: RS blocks of soft_cases.link_payloads() ->
    model inner encoder at ``rate`` -> oracle transmitter -> float64 channel model -> oracle receiver with its taps ->
    the soft model -> both model inner decoders -> the RS model on what they return, whatever their CRC said.
    Returns (hard, soft), each per packet (inner (ok, bytes, corrected), outer (ok, payload, corrected, failed));
    (None, None) where the receiver's packet list is not the six packets, each from a frame of its own."""
    import multipath_cases as mpc
    import punct_cases as pc
    import soft_cases as sc
    from ofdm_uhd_amd import _abi
    seed = sc.LINK_SEED if seed is None else seed
    pay = sc.link_payloads()
    iq = orc.tx(cfg, [pc.encode(encode(p), 16, rate) for p in pay])
    psig = float(np.mean(np.abs(iq.astype(np.complex128)) ** 2))
    y, _ = mpc.model(sc.link_air(iq), sc.link_channel_cfg(snr_db, psig, seed), 0)
    res = orc.rx(cfg, y.astype(np.complex64), (1 << _abi.TAP_RX_FFT) | (1 << _abi.TAP_RX_SINK) | (1 << _abi.TAP_RX_FRAMES))
    pk = res.packets
    fft, sink, frames = res.tap(_abi.TAP_RX_FFT), res.tap(_abi.TAP_RX_SINK), res.tap(_abi.TAP_RX_FRAMES)
    smap, cst, mask = sc.smap_of(cfg), sc.cst_of(cfg), sc.mask_of(cfg)
    nbits = int(cfg.arity).bit_length() - 1
    # the six packets, in order, each from its own frame; a flag behind the last packet that delivers nothing (the
    # receiver raises one in the tail of some of these captures) leaves the list what it is
    want_len = [pc.coded_len(coded_len(len(p)), rate) for p in pay]
    if [len(blk) for _, blk in pk] != want_len or len(frames) < len(pay):
        return None, None
    pre = np.concatenate([[0], np.cumsum(frames[:, 1].astype(np.int64) + 1)])[:-1]
    row, hard, soft = 0, [], []
    for k, (ok, blk) in enumerate(pk):
        ns = -(-8 * (sc.HEADER + len(blk) + 4) // (len(smap) * nbits))
        if int(frames[k, 1]) < ns:
            return None, None
        x = sink[row:row + ns, :len(smap)]
        row += ns
        eq = sc.hinv_from_preamble(cfg, fft[pre[k]])
        v = sc.packet_values(x, eq, smap, cst, len(blk), mask, scale)
        h, s = pc.decode(blk, 16, rate), pc.decode_values(v, 16, rate)
        hard.append((h, decode(h[1])))
        soft.append((s, decode(s[1])))
    if row > len(sink):
        return None, None
    return hard, soft


def link_summary(side, pay):
    """(inner alone, concatenated) as strings of 0 / 1 per packet: decoded to the payload sent."""
    inner = "".join(str(int(bool(i[0]) and i[1] == encode(p))) for (i, _), p in zip(side, pay))
    outer = "".join(str(int(bool(o[0]) and o[1] == p)) for (_, o), p in zip(side, pay))
    return inner, outer
