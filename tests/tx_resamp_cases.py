"""Shared by test_tx_resamp_host.py and test_gpu_tx_resamp.py: the float64 model of the rational-rate transmit stage (the
definition in include/ofdm_hip.h, restated in NumPy), the error bound derived from it and the wideband bands of the
end-to-end tests -- the scenarios of resamp_cases built with the stage instead of the whole-stream FFT resampling."""
import numpy as np

from helpers import make_cfg, make_payloads
from ofdm_uhd_amd import resample, tx_resample

EPS = 2.0 ** -24
STAGGER = 37           # narrowband samples by which the second link trails the first (resamp_cases._capture's shift)


def tile_inputs(L, M):
    """Inputs one workgroup of k_tx_resamp consumes (tx_resamp_geom in csrc/tx_resamp.h: 64 KC periods of M inputs,
    KC doubled while there are fewer than 4 work items and the tile stays within 4096 inputs): the tests pick sizes
    around it.  A wrong value here only moves the sizes, it cannot make a wrong output pass."""
    m = max(L, M)
    kc = 16 if m <= 1 else 8 if m <= 2 else 4 if m <= 4 else 2 if m <= 8 else 1
    while L * kc < 4 and 2 * kc * 64 * M <= 4096:
        kc *= 2
    return 64 * kc * M


def phase_step(fc):
    """D of the definition, restated: frac(fc) in units of 2^-64 turn, truncated; a fraction that rounds up to 1 is 0."""
    t = float(fc)
    t -= np.floor(t)
    return int(t * 2.0 ** 64) if t < 1.0 else 0


def history(ntaps, L):
    return (int(ntaps) - 1) // int(L)


def count(first, n, L, M):
    """Outputs m with first <= floor(m M / L) < first + n: ceil((first + n) L / M) - ceil(first L / M)."""
    return -(-(int(first) + int(n)) * int(L) // int(M)) - -(-int(first) * int(L) // int(M))


def _rotation(n0, nout, D):
    phi = (np.uint64(n0) + np.arange(nout, dtype=np.uint64)) * np.uint64(D)      # wraps modulo 2^64
    return np.exp(2j * np.pi * (phi.astype(np.float64) / 2.0 ** 64))


def model_zero_stuffed(x, h, L, M, D, first=0):
    """y64[n], bound_sum[n] for the narrowband stream x (x[0] has absolute index ``first``, zeros before it) and the
    real taps h, the convolution form: zero-stuff x by L, convolve with h, take the positions n M (relative to the
    stuffed stream's start first L), rotate by +Phi_n; bound_sum is the same with |h| and |x|."""
    x = np.asarray(x).astype(np.complex128)
    h = np.asarray(h).astype(np.float64)
    n0 = -(-first * L // M)
    nout = count(first, len(x), L, M)
    if nout == 0:
        return np.zeros(0, np.complex128), np.zeros(0)
    u = np.zeros(len(x) * L, np.complex128)
    u[::L] = x
    idx = (n0 + np.arange(nout, dtype=np.int64)) * M - first * L
    assert idx[0] >= 0 and idx[-1] < len(u)
    v = np.convolve(u, h)[idx]
    s = np.convolve(np.abs(u), np.abs(h))[idx]
    return v * _rotation(n0, nout, D), s


def model(x, h, L, M, D, first=0):
    """The same two results from the per-phase form of the definition, i_n = floor(n M / L), p_n = n M mod L,
    v[n] = sum_q h[p_n + q L] x[i_n - q]: one np.convolve of x with h[p::L] per phase p that occurs.  These are the
    sums of model_zero_stuffed without the terms that multiply a stuffed zero (test_tx_resamp_host.py pins the two
    against each other), at 1 / L of the work -- which is what lets the GPU tests use L = 64 with 1024 taps."""
    x = np.asarray(x).astype(np.complex128)
    h = np.asarray(h).astype(np.float64)
    n0 = -(-first * L // M)
    nout = count(first, len(x), L, M)
    if nout == 0:
        return np.zeros(0, np.complex128), np.zeros(0)
    pos = (n0 + np.arange(nout, dtype=np.int64)) * M
    i, p = pos // L - first, pos % L
    assert i[0] >= 0 and i[-1] < len(x)
    v, s = np.zeros(nout, np.complex128), np.zeros(nout)
    for ph in np.unique(p):
        sub = h[ph::L]
        if len(sub) == 0:
            continue                          # a phase without a tap: v = 0
        sel = p == ph
        v[sel] = np.convolve(x, sub)[i[sel]]
        s[sel] = np.convolve(np.abs(x), np.abs(sub))[i[sel]]
    return v * _rotation(n0, nout, D), s


def bound(ntaps, L, s, add=None):
    """|y - y64| <= (ceil(ntaps / L) + 16) 2^-24 (s[n] + |add[n]|): an output is a float32 sum of at most
    ceil(ntaps / L) products, and 16 more roundings cover the rotation, the rounding of r and the optional ``add``
    (as duc_cases.bound)."""
    if add is not None:
        s = s + np.abs(np.asarray(add).astype(np.complex128))
    return (-(-int(ntaps) // int(L)) + 16) * EPS * s


# name -> modulation, N, occ, CP, L, M, link frequencies (cycles per wideband sample), payload bytes: the cases of
# resamp_cases with the ratio seen from the transmitter
CASES = {
    "qpsk512_5_2": ("qpsk", 512, 200, 128, 5, 2, (0.22, -0.21), 100),
    "qam16_512_3_4": ("qam16", 512, 200, 128, 3, 4, (0.05,), 100),
    "bpsk64_25_8": ("bpsk", 64, 48, 16, 25, 8, (0.3, -0.17), 40),
}


def links(name, orc=None, tx=None):
    """The narrowband streams of one case on a common time axis (link i trails link 0 by i STAGGER samples), from
    ``tx(cfg, payloads, lead, tail)`` (default: the oracle's transmitter), with the Q zeros that push the filter's
    tail out appended, and what goes with them."""
    mod, N, occ, CP, L, M, freqs, plen = CASES[name]
    cfg = make_cfg(mod, N, occ, CP)
    pays = [make_payloads(4, plen, seed=s) for s in (11, 29)[:len(freqs)]]
    lead, tail = 2 * N, 3 * N
    if tx is None:
        tx = lambda c, p, lead, tail: orc.tx(c, p, lead=lead, tail=tail)  # noqa: E731
    nb = [np.asarray(tx(cfg, p, lead, tail), np.complex64) for p in pays]
    P = float(np.mean(np.abs(nb[0][lead:len(nb[0]) - tail]) ** 2))
    tx_taps = tx_resample.design(L, M, occ / float(N))
    Q = history(len(tx_taps), L)
    x = [np.concatenate([np.zeros(STAGGER * i, np.complex64), s, np.zeros(STAGGER * (len(nb) - 1 - i) + Q, np.complex64)])
         for i, s in enumerate(nb)]
    return dict(cfg=cfg, L=L, M=M, freqs=freqs, payloads=pays, x=x, P=P, N=N, occ=occ, mod=mod, CP=CP,
                tx_taps=tx_taps, rx_taps=resample.design(M, L, occ / float(N)))


def noise(n, P, L, M):
    """The wideband noise of resamp_cases._capture: seed 2024, sigma = sqrt(P L / M / 1e3) -- 30 dB inside one link's
    band (M / L of the wideband one).  It is needed: a silent tail posts a spurious CRC-failed message."""
    rng = np.random.default_rng(2024)
    sigma = np.sqrt(P * L / M / 1e3)
    return sigma * np.sqrt(0.5) * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
