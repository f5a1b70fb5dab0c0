"""Shared by test_channel_host.py and test_gpu_channel.py: the float64 model of the synthetic channel (the definition
in include/ofdm_hip.h: Philox-2x32-7 per PAIR of samples, word 0 for the even stream index and word 1 for the odd one,
16 bits of Box-Muller radius and 16 of angle, a carrier rotation by cfo * index), the two error bounds the tests hold
the oracle and the engine to, and the transmit cases both files run."""
import collections

import numpy as np

from helpers import make_cfg, make_payloads

EPS = 2.0 ** -24
BIG_SEED = (0x1234 << 32) | 77          # both halves of the seed enter the key
RAGGED = (300, 17, 250)                 # sym_pkt route; the symbols do not fill the last workgroup
UNIFORM = (250, 250, 250)               # uniform_spp route

Case = collections.namedtuple("Case", "name mod N occ CP lead sigma cfo_bins seed stream_id plens")
CASES = [
    # paired, LEAN, eight symbols in one wave: the lane swap must stay inside a symbol
    Case("n64_paired_lean", "qam16", 64, 48, 16, 128, 0.005, 0.0, BIG_SEED, 3, RAGGED),
    # paired, LEAN, one wave per symbol (the benchmark's shape)
    Case("n512_paired_lean", "qpsk", 512, 200, 128, 1024, 0.005, 0.0, 0xC0FFEE, 0, RAGGED),
    # paired, rotation: the full kernel
    Case("n512_paired_cfo", "qpsk", 512, 200, 128, 1024, 0.005, 0.05, BIG_SEED, 3, RAGGED),
    # odd lead: every symbol takes the per-sample route
    Case("n512_odd_lead_cfo", "qpsk", 512, 200, 128, 1025, 0.005, 0.05, BIG_SEED, 3, RAGGED),
    # odd CP: symbols alternate between the two routes (the stream id's high half enters the key)
    Case("n512_odd_cp", "qpsk", 512, 200, 127, 1024, 0.005, 0.0, 0xC0FFEE, (9 << 32) | 1, RAGGED),
    # rotation only, no noise
    Case("n512_cfo_only", "qpsk", 512, 200, 128, 1024, 0.0, 0.3, 0xC0FFEE, 0, RAGGED),
    # a symbol spans two waves
    Case("n1024_two_waves_cfo", "qam64", 1024, 600, 256, 2048, 0.002, 0.3, BIG_SEED, 3, RAGGED),
    # eight waves per symbol, odd lead
    Case("n4096_odd_lead", "qam16", 4096, 2400, 1024, 8193, 0.002, 0.0, BIG_SEED, 3, RAGGED),
    # the benchmark's shape again, equal lengths
    Case("n512_paired_lean_uniform", "qpsk", 512, 200, 128, 1024, 0.005, 0.0, BIG_SEED, 3, UNIFORM),
]
IDS = [c.name for c in CASES]

# the stand-alone call at its edges: more samples than k_channel's 2048 x 256 threads (the grid-stride loop wraps), an
# odd first index whose pair counter has a non-zero high word
STANDALONE = dict(n=524288 + 777, index0=2 ** 33 + 5, sigma=0.01, cfo=0.002, seed=BIG_SEED, stream_id=3)


def cfo_of(case):
    """radians per sample, as the float32 the ABI carries"""
    return float(np.float32(case.cfo_bins * 2.0 * np.pi / case.N))


def tail_of(case):
    return case.N + case.CP + 3


def cfg_of(case, **kw):
    return make_cfg(case.mod, case.N, case.occ, case.CP, **kw)


def payloads_of(case):
    return make_payloads(len(case.plens), list(case.plens))


def chan_args(case):
    return dict(sigma=case.sigma, cfo=cfo_of(case), seed=case.seed, stream_id=case.stream_id)


_REF = {}


def reference(orc, case):
    """(clean, ref): the oracle's transmit buffer with zeros for lead-in and tail, and the oracle's channel over the
    WHOLE of it -- lead-in, every body sample, every prefix copy and the tail, each at its own stream index.  Computed
    once per case, read-only."""
    if case.name not in _REF:
        clean = orc.tx(cfg_of(case), payloads_of(case), lead=case.lead, tail=tail_of(case))
        ref = orc.channel(clean.copy(), index0=0, **chan_args(case))
        for a in (clean, ref):
            a.setflags(write=False)
        _REF[case.name] = (clean, ref)
    return _REF[case.name]


def ramp(n):
    """The stand-alone call's input: amplitude rising from 0.01 to 0.25, seeded phases."""
    rng = np.random.default_rng(2033)
    ph = 2.0 * np.pi * rng.random(n)
    return (np.linspace(0.01, 0.25, n) * np.exp(1j * ph)).astype(np.complex64)


# ---- the model -------------------------------------------------------------------------------------------------------
def chan_key(seed, stream_id):
    seed, stream_id = int(seed), int(stream_id)
    m = 0xFFFFFFFF
    return ((seed & m) ^ (seed >> 32) ^ (((stream_id & m) * 0x9E3779B9 + (stream_id >> 32) * 0x85EBCA6B) & m)) & m


def philox(key, counter, rounds=7):
    """Philox-2x32 on an array of 64-bit counters: (word 0, word 1) as uint64 arrays holding 32-bit values."""
    ctr = np.atleast_1d(np.asarray(counter, dtype=np.uint64))
    m = np.uint64(0xFFFFFFFF)
    c0, c1 = ctr & m, ctr >> np.uint64(32)
    k = int(key) & 0xFFFFFFFF
    for _ in range(rounds):
        p = np.uint64(0xD256D193) * c0                      # < 2^64: both factors are below 2^32
        c0, c1 = (p >> np.uint64(32)) ^ np.uint64(k) ^ c1, p & m
        k = (k + 0x9E3779B9) & 0xFFFFFFFF
    return c0, c1


def words(seed, stream_id, idx):
    """The noise word of every stream index in idx: one call per pair, word 0 to the even index."""
    idx = np.asarray(idx, dtype=np.uint64)
    w0, w1 = philox(chan_key(seed, stream_id), idx >> np.uint64(1))
    return np.where((idx & np.uint64(1)) == 0, w0, w1)


def indices(n, index0):
    return np.uint64(index0) + np.arange(n, dtype=np.uint64)


def model(x, sigma, cfo, seed, stream_id, index0, word_index=None):
    """(y, rad): the channel on x in float64 and every sample's Box-Muller radius.  sigma and cfo are taken as the
    float32 values the ABI carries.  word_index (default: the samples' own stream indices) names the stream index whose
    noise word each sample uses -- the hook the mutated copies of test_channel_host.py go through."""
    sigma, cfo = float(np.float32(sigma)), float(np.float32(cfo))
    idx = indices(len(x), index0)
    y = np.asarray(x).astype(np.complex128)
    rad = np.zeros(len(y))
    if cfo != 0.0:
        ph = cfo * idx.astype(np.float64)                   # (indices below 2^53: exact)
        ph = ph - 2.0 * np.pi * np.floor(ph / (2.0 * np.pi) + 0.5)
        y = y * np.exp(1j * ph)
    if sigma > 0.0:
        w = words(seed, stream_id, idx if word_index is None else word_index)
        u1 = ((w >> np.uint64(16)).astype(np.float64) + 0.5) / 65536.0
        u2 = ((w & np.uint64(0xFFFF)).astype(np.float64) + 0.5) / 65536.0
        rad = np.sqrt(-2.0 * np.log(u1))
        y = y + (sigma / np.sqrt(2.0)) * rad * np.exp(2j * np.pi * u2)
    return y, rad


def parts(z):
    """[n, 2] real and imaginary parts in float64"""
    z = np.asarray(z).astype(np.complex128)
    return np.stack([z.real, z.imag], axis=1)


def oracle_bound(x, y, rad, sigma, cfo):
    """Per part, [n, 2]: how far the oracle's float32 evaluation may lie from the model's y (derivation: the docstring
    of test_channel_host.py).  18 eps (sigma / sqrt 2) rad for the noise term, 4 eps |x| for the rotation, eps |y_part|
    for the final addition."""
    sigma, cfo = float(np.float32(sigma)), float(np.float32(cfo))
    b = EPS * np.abs(parts(y))
    if sigma > 0.0:
        b = b + (18.0 * EPS * sigma / np.sqrt(2.0) * np.asarray(rad))[:, None]
    if cfo != 0.0:
        b = b + (4.0 * EPS * np.abs(np.asarray(x).astype(np.complex128)))[:, None]
    return b


def engine_bound(sigma, clean, ref):
    """Per sample: |engine - oracle| <= 1e-4 sigma + 4 * 2^-24 (|clean| + |ref|).  The first term is the accepted gap
    between the hardware's log2 / sqrt / sin / cos and libm (test_channel_parity: 1e-6 at sigma 0.01); the second covers
    the float32 roundings of the rotation and of the final addition.  A misplaced noise word misses by the order of
    sigma: ten thousand times the first term."""
    return 1e-4 * float(np.float32(sigma)) + 4.0 * EPS * (np.abs(clean).astype(np.float64) + np.abs(ref).astype(np.float64))


def prefix_mask(n, lead, tail, N, CP):
    """True at the cyclic-prefix samples of a transmit buffer of n samples"""
    L = N + CP
    assert (n - lead - tail) % L == 0
    k = np.arange(n) - lead
    return (k >= 0) & (k < n - lead - tail) & (k % L < CP)
