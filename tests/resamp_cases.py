"""Shared by test_resamp_host.py and test_gpu_resamp.py: the float64 model of the rational-rate front end (the
definition in include/ofdm_hip.h, restated in NumPy) and the wideband captures the end-to-end tests demodulate."""
import functools

import numpy as np

from helpers import make_cfg, make_payloads
from ofdm_uhd_amd import resample


def tile_inputs(L, M):
    """Inputs one workgroup of k_resamp consumes (resamp_geom in csrc/resamp.h: 64 KC periods of M inputs): the tests
    pick sizes around it.  A wrong value here only moves the sizes, it cannot make a wrong output pass."""
    m = max(L, M)
    kc = 16 if m <= 1 else 8 if m <= 2 else 4 if m <= 4 else 2 if m <= 8 else 1
    return 64 * kc * M


def phase_step(fc, L, M):
    """D of the definition, restated: frac(fc M / L) in units of 2^-64 turn, truncated; a fraction that rounds up to 1
    is 0."""
    t = float(fc) * int(M) / int(L)
    t -= np.floor(t)
    return int(t * 2.0 ** 64) if t < 1.0 else 0


def count(first, n, L, M):
    """Outputs m with first <= floor(m M / L) < first + n: ceil((first + n) L / M) - ceil(first L / M)."""
    return -(-(int(first) + int(n)) * int(L) // int(M)) - -(-int(first) * int(L) // int(M))


def _rotation(n0, nout, D):
    phi = (np.uint64(n0) + np.arange(nout, dtype=np.uint64)) * np.uint64(D)      # wraps modulo 2^64
    return np.exp(-2j * np.pi * (phi.astype(np.float64) / 2.0 ** 64))


def model_zero_stuffed(x, c, L, M, D, first=0):
    """y64[n], bound_sum[n] for the stream x (complex, x[0] has absolute index ``first``, zeros before it) and the
    table c, the convolution form: zero-stuff x by L, convolve with c, take the positions n M (relative to the stuffed
    stream's start first L), rotate by Phi_n; bound_sum is the same with |c| and |x|."""
    x = np.asarray(x).astype(np.complex128)
    c = np.asarray(c).astype(np.complex128)
    n0 = -(-first * L // M)
    nout = count(first, len(x), L, M)
    if nout == 0:
        return np.zeros(0, np.complex128), np.zeros(0)
    u = np.zeros(len(x) * L, np.complex128)
    u[::L] = x
    idx = (n0 + np.arange(nout, dtype=np.int64)) * M - first * L
    assert idx[0] >= 0 and idx[-1] < len(u)
    v = np.convolve(u, c)[idx]
    s = np.convolve(np.abs(u), np.abs(c))[idx]
    return v * _rotation(n0, nout, D), s


def model(x, c, L, M, D, first=0):
    """The same two results from the per-phase form of the definition, i_n = floor(n M / L), p_n = n M mod L,
    v[n] = sum_q c[p_n + q L] x[i_n - q]: one np.convolve of x with c[p::L] per phase p that occurs.  These are the
    sums of model_zero_stuffed without the terms that multiply a stuffed zero (test_resamp_host.py pins the two
    against each other), at 1 / L of the work -- which is what lets the GPU tests use L = 64 with 1024 taps."""
    x = np.asarray(x).astype(np.complex128)
    c = np.asarray(c).astype(np.complex128)
    n0 = -(-first * L // M)
    nout = count(first, len(x), L, M)
    if nout == 0:
        return np.zeros(0, np.complex128), np.zeros(0)
    pos = (n0 + np.arange(nout, dtype=np.int64)) * M
    i, p = pos // L - first, pos % L
    assert i[0] >= 0 and i[-1] < len(x)
    v, s = np.zeros(nout, np.complex128), np.zeros(nout)
    for ph in np.unique(p):
        sub = c[ph::L]
        if len(sub) == 0:
            continue                          # a phase without a tap: v = 0
        sel = p == ph
        v[sel] = np.convolve(x, sub)[i[sel]]
        s[sel] = np.convolve(np.abs(x), np.abs(sub))[i[sel]]
    return v * _rotation(n0, nout, D), s


def fft_resample(x, L, M):
    """Brick-wall resampling of a stream (length a multiple of L) to M / L times its rate: the whole stream's
    transform, zero-extended or cut to M / L times the band."""
    n = len(x)
    assert n % L == 0
    m = n // L * M
    X = np.fft.fft(np.asarray(x, np.complex128))
    Y = np.zeros(m, np.complex128)
    k = min(n, m)
    h = (k + 1) // 2
    Y[:h] = X[:h]
    Y[m - (k - h):] = X[n - (k - h):]
    return np.fft.ifft(Y) * (m / float(n))


# name -> modulation, N, occ, CP, L, M, link frequencies, payload bytes
CASES = {
    "qpsk512_2_5": ("qpsk", 512, 200, 128, 2, 5, (0.22, -0.21), 100),
    "qam16_512_4_3": ("qam16", 512, 200, 128, 4, 3, (0.05,), 100),
    "bpsk64_8_25": ("bpsk", 64, 48, 16, 8, 25, (0.3, -0.17), 40),
}


@functools.lru_cache(maxsize=None)
def _capture(name):
    from oracle import oracle as orc
    mod, N, occ, CP, L, M, freqs, plen = CASES[name]
    cfg = make_cfg(mod, N, occ, CP)
    pays = [make_payloads(4, plen, seed=s) for s in (11, 29)[:len(freqs)]]
    lead, tail, shift = 2 * N, 3 * N, 37
    nb = [orc.tx(cfg, p, lead=lead, tail=tail) for p in pays]
    P = float(np.mean(np.abs(nb[0][lead:len(nb[0]) - tail]) ** 2))
    streams = [np.concatenate([np.zeros(shift * i, np.complex64), x, np.zeros(shift * (len(nb) - 1 - i), np.complex64)])
               for i, x in enumerate(nb)]
    pad = -len(streams[0]) % L
    streams = [np.concatenate([x, np.zeros(pad, np.complex64)]) for x in streams]
    nw = len(streams[0]) // L * M
    n = np.arange(nw, dtype=np.float64)
    wide = np.zeros(nw, np.complex128)
    for x, f in zip(streams, freqs):
        wide += fft_resample(x, L, M) * np.exp(2j * np.pi * f * n)
    rng = np.random.default_rng(2024)
    sigma = np.sqrt(P * M / L / 1e3)           # 30 dB inside one link's band (L / M of the capture)
    wide += sigma * np.sqrt(0.5) * (rng.standard_normal(nw) + 1j * rng.standard_normal(nw))
    wide = wide.astype(np.complex64)
    wide.setflags(write=False)
    taps = resample.design(L, M, occ / float(N))
    return dict(cfg=cfg, L=L, M=M, freqs=freqs, payloads=pays, wide=wide, taps=taps, N=N, occ=occ, mod=mod, CP=CP)


def capture(name):
    """The wideband capture of one case (computed once per process, read-only)."""
    return _capture(name)
