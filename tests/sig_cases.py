"""The signal field restated in NumPy (include/ofdm_hip.h, "coded links: the signal field"), and the seeded cases the
host and GPU tests share: the codebook, the field's byte image, the maximum-likelihood decoder with its tie rule and
margin.  Nothing here loads the library."""
import functools

import numpy as np

GEN = 0xC75                 # x^11 + x^10 + x^6 + x^5 + x^4 + x^2 + 1
FIELD_BYTES, FIELD_BITS = 12, 96
NO_WORD = 0xFFFF
AWGN_SEED, AWGN_WORDS, AWGN_ESN0_DB = 20261021, 2048, -3.0


def codeword_bits(w):
    """The 24 codeword bits of word w, bit 0 first: 12 word bits MSB first, 11 bits of w x^11 mod g, overall parity."""
    r = w << 11
    for i in range(22, 10, -1):
        if (r >> i) & 1:
            r ^= GEN << (i - 11)
    bits = [(w >> (11 - j)) & 1 for j in range(12)] + [(r >> (10 - j)) & 1 for j in range(11)]
    return bits + [sum(bits) & 1]


@functools.lru_cache(maxsize=None)
def codebook():
    """uint8[4096, 24]: row w is the codeword of w."""
    cb = np.array([codeword_bits(w) for w in range(4096)], np.uint8)
    cb.setflags(write=False)
    return cb


@functools.lru_cache(maxsize=None)
def _signs():
    s = codebook().astype(np.int32) * 2 - 1
    s.setflags(write=False)
    return s


def word_fields(w):
    """(codec, rate, rs, log2 columns) of a valid word, None for any other 12-bit value -- stated on the table of the
    issue, not on the library's code."""
    if not 0 <= w < 4096 or (w & 0xF):
        return None
    codec, rate, rs, lg = w >> 10, (w >> 8) & 3, (w >> 7) & 1, (w >> 4) & 7
    if codec == 0 and rate == 0 and lg == 0:
        return codec, rate, rs, lg
    if codec == 1 and lg <= 4:
        return codec, rate, rs, lg
    if codec == 2 and lg == 0:
        return codec, rate, rs, lg
    return None


def valid_words():
    return [w for w in range(4096) if word_fields(w) is not None]


def field_bits(w):
    """The 96 field bits of word w: four copies of the codeword."""
    return np.tile(codebook()[w], 4)


def field_bytes(w):
    """The field's 12 bytes, field bit t MSB first within a byte."""
    return np.packbits(field_bits(w)).tobytes()


def encode(words, bodies):
    return [field_bytes(int(w)) + bytes(b) for w, b in zip(words, bodies)]


def values_of_bytes(block):
    """Hard input as the decoder sees it: +1 / -1 per bit, MSB first."""
    return (np.unpackbits(np.frombuffer(bytes(block), np.uint8)).astype(np.int8) * 2 - 1)


def decode_values(v):
    """(word, margin) of one packet's int8 values (any length; the first 96 are the field)."""
    v = np.asarray(v, np.int8).reshape(-1)
    if len(v) % 8 or len(v) < FIELD_BITS:
        return NO_WORD, 0
    x = np.maximum(v[:FIELD_BITS].astype(np.int32), -127)
    c = x.reshape(4, 24).sum(axis=0)
    m = _signs() @ c
    best = int(np.argmax(m))            # the first of equal maxima: the smallest word
    rest = np.delete(m, best)
    return best, int(m[best] - rest.max())


def decode_bytes(block):
    if len(block) < FIELD_BYTES:
        return NO_WORD, 0
    return decode_values(values_of_bytes(block))


def clean_values(w, amp=64):
    return ((field_bits(w).astype(np.int16) * 2 - 1) * amp).astype(np.int8)


def flipped(w, nflip, seed, amp=64):
    """The clean values of w with ``nflip`` of the 96 signs flipped at seeded positions."""
    v = clean_values(w, amp).copy()
    pos = np.random.default_rng(seed).choice(FIELD_BITS, nflip, replace=False)
    v[pos] = -v[pos]
    return v


def erased_copies(w, copies, amp=64):
    v = clean_values(w, amp).copy()
    for c in copies:
        v[24 * c:24 * c + 24] = 0
    return v


def tie_values():
    """Eight nonzero positions only: the first eight bits of copy 0 say "1".  Every word whose first eight bits are
    ones reaches the largest metric, 0xFF0 is the smallest of them, and the margin is 0."""
    v = np.zeros(FIELD_BITS, np.int8)
    v[:8] = 5
    return v


@functools.lru_cache(maxsize=None)
def awgn_set():
    """(words uint16[2048], values int8[2048, 96]): BPSK over AWGN at Es/N0 = -3 dB, values clip(rint(32 y), +-127)."""
    rng = np.random.default_rng(AWGN_SEED)
    words = rng.integers(0, 4096, AWGN_WORDS).astype(np.uint16)
    bits = np.tile(codebook()[words], (1, 4)).astype(np.float64)
    sigma = np.sqrt(0.5 / 10.0 ** (AWGN_ESN0_DB / 10.0))
    y = (2.0 * bits - 1.0) + sigma * rng.standard_normal(bits.shape)
    vals = np.clip(np.rint(32.0 * y), -127, 127).astype(np.int8)
    words.setflags(write=False)
    vals.setflags(write=False)
    return words, vals


def decode_many(vals):
    """decode_values over the rows of int8[n, 96], vectorised: (word int64[n], margin int64[n])."""
    x = np.maximum(np.asarray(vals, np.int8).astype(np.int32), -127)
    c = x.reshape(len(x), 4, 24).sum(axis=1)
    m = c @ _signs().T
    best = np.argmax(m, axis=1)
    top = m[np.arange(len(m)), best]
    m[np.arange(len(m)), best] = np.iinfo(np.int32).min
    return best, top - m.max(axis=1)
