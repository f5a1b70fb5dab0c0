"""Shared by test_ddc_host.py and test_gpu_ddc.py: the float64 model of the wideband front end (the definition in
include/ofdm_hip.h, restated in NumPy) and the two-link wideband captures the end-to-end tests demodulate."""
import functools

import numpy as np

from helpers import make_cfg, make_payloads
from ofdm_uhd_amd import ddc


def tile_outputs(R):
    """Outputs one workgroup of k_ddc produces (ddc_geom in csrc/ddc.h): the tests pick sizes around tile_outputs * R
    input samples.  A wrong value here only moves the sizes, it cannot make a wrong output pass."""
    return 1024 if R <= 4 else (256 if R <= 16 else 64)


def phase_step(fc, R):
    """D of the definition, restated: frac(fc R) in units of 2^-64 turn, truncated; a fraction that rounds up to 1 is 0."""
    t = float(fc) * int(R)
    t -= np.floor(t)
    return int(t * 2.0 ** 64) if t < 1.0 else 0


def count(first, n, R):
    """Outputs m with first <= m R < first + n: ceil((first + n) / R) - ceil(first / R)."""
    return -(-(int(first) + int(n)) // int(R)) - -(-int(first) // int(R))


def model(x, c, R, D, first=0):
    """y64[m], bound_sum[m] for the stream x (complex, x[0] has absolute index ``first``, zeros before it) and the
    table c: y = (sum_k c[k] x[mR - k]) expj(-2 pi (m D mod 2^64) / 2^64) in float64 over every m with
    first <= m R < first + len(x); bound_sum = sum_k |c[k]| |x[mR - k]|."""
    x = np.asarray(x).astype(np.complex128)
    c = np.asarray(c).astype(np.complex128)
    m0 = -(-first // R)
    nout = count(first, len(x), R)
    if nout == 0:
        return np.zeros(0, np.complex128), np.zeros(0)
    idx = (m0 + np.arange(nout, dtype=np.int64)) * R - first
    v = np.convolve(x, c)[idx]
    s = np.convolve(np.abs(x), np.abs(c))[idx]
    phi = (m0 + np.arange(nout, dtype=np.uint64)).astype(np.uint64) * np.uint64(D)   # wraps modulo 2^64
    return v * np.exp(-2j * np.pi * (phi.astype(np.float64) / 2.0 ** 64)), s


def interpolate(x, R):
    """Brick-wall interpolation by R: the whole stream's transform, zero-extended to R times the band."""
    n = len(x)
    X = np.fft.fft(np.asarray(x, np.complex128))
    Y = np.zeros(n * R, np.complex128)
    h = (n + 1) // 2
    Y[:h] = X[:h]
    Y[n * R - (n - h):] = X[h:]
    return np.fft.ifft(Y) * R


# name -> modulation, N, occ, CP, R, (fa, fb), transition, payload bytes
CASES = {
    "qpsk512_r4": ("qpsk", 512, 200, 128, 4, (0.25, -0.25), None, 100),
    "qam16_2048_r2": ("qam16", 2048, 1200, 512, 2, (0.0, 0.5), 0.1, 700),
    "bpsk64_r8": ("bpsk", 64, 48, 16, 8, (0.25, -0.25), None, 40),
    "qpsk512_r3": ("qpsk", 512, 200, 128, 3, (1.0 / 3.0, -1.0 / 3.0 + 0.013), None, 100),
}


@functools.lru_cache(maxsize=None)
def _capture(name):
    from oracle import oracle as orc
    mod, N, occ, CP, R, freqs, transition, plen = CASES[name]
    cfg = make_cfg(mod, N, occ, CP)
    pays = [make_payloads(4, plen, seed=11), make_payloads(4, plen, seed=29)]
    lead, tail, shift = 2 * N, 3 * N, 37
    nb = [orc.tx(cfg, p, lead=lead, tail=tail) for p in pays]
    P = float(np.mean(np.abs(nb[0][lead:len(nb[0]) - tail]) ** 2))
    xa = np.concatenate([nb[0], np.zeros(shift, np.complex64)])
    xb = np.concatenate([np.zeros(shift, np.complex64), nb[1]])
    n = np.arange(len(xa) * R, dtype=np.float64)
    wide = np.zeros(len(xa) * R, np.complex128)
    for x, f in zip((xa, xb), freqs):
        wide += interpolate(x, R) * np.exp(2j * np.pi * f * n)
    rng = np.random.default_rng(2024)
    sigma = np.sqrt(P * R / 1e3)           # 30 dB inside one link's band (1/R of the capture)
    wide += sigma * np.sqrt(0.5) * (rng.standard_normal(len(wide)) + 1j * rng.standard_normal(len(wide)))
    wide = wide.astype(np.complex64)
    wide.setflags(write=False)
    taps = ddc.design(R, occ / float(N), transition)
    return dict(cfg=cfg, R=R, freqs=freqs, payloads=pays, wide=wide, taps=taps, transition=transition, N=N, occ=occ,
                mod=mod, CP=CP)


def capture(name):
    """The wideband capture of one case (computed once per process, read-only)."""
    return _capture(name)
