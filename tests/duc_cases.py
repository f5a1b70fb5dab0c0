"""Shared by test_duc_host.py and test_gpu_duc.py: the float64 model of the wideband transmit stage (the definition in
include/ofdm_hip.h, restated in NumPy), the error bound derived from it and the two-link scenario of ddc_cases built
with it instead of the whole-stream FFT interpolation."""
import numpy as np

import ddc_cases
from ofdm_uhd_amd import duc

EPS = 2.0 ** -24
STAGGER = 37           # narrowband samples by which the second link trails the first (ddc_cases._capture's shift)


def tile_outputs(L):
    """Outputs one workgroup of k_duc produces (duc_geom in csrc/duc.h): the tests pick sizes around it.  A wrong value
    here only moves the sizes, it cannot make a wrong output pass."""
    return 2048 if L <= 2 else 1024


def phase_step(fc):
    """D of the definition: frac(fc) in units of 2^-64 turn, truncated; a fraction that rounds up to 1 is 0."""
    return ddc_cases.phase_step(fc, 1)


def history(ntaps, L):
    return (int(ntaps) - 1) // int(L)


def model(x, h, L, D, first=0):
    """y64[n], bound_sum[n] for the narrowband stream x (x[0] has absolute index ``first``, zeros before it) and the
    real taps h: zero stuffing, np.convolve with the taps and the rotation expj(+2 pi (n D mod 2^64) / 2^64) in
    float64 over the len(x) L outputs n = first L ..; bound_sum[n] = sum_q |h[p + q L]| |x[m - q]|."""
    x = np.asarray(x).astype(np.complex128)
    h = np.asarray(h).astype(np.float64)
    L = int(L)
    nout = len(x) * L
    if nout == 0:
        return np.zeros(0, np.complex128), np.zeros(0)
    up = np.zeros(nout, np.complex128)
    up[::L] = x
    v = np.convolve(up, h)[:nout]
    s = np.convolve(np.abs(up), np.abs(h))[:nout]
    n = np.uint64(int(first) * L) + np.arange(nout, dtype=np.uint64)
    phi = n * np.uint64(D)                                                      # wraps modulo 2^64
    return v * np.exp(2j * np.pi * (phi.astype(np.float64) / 2.0 ** 64)), s


def bound(ntaps, L, s, add=None):
    """|y - y64| <= (Q + 1 + 16) 2^-24 s[n]: a float32 sum of at most Q + 1 products in any order, and 16 more roundings
    for the rotation, the rounding of r and the optional ``add``, whose magnitude then belongs to s."""
    if add is not None:
        s = s + np.abs(np.asarray(add).astype(np.complex128))
    return (history(ntaps, L) + 1 + 16) * EPS * s


def links(name, orc=None, tx=None):
    """The two narrowband streams of one ddc_cases case on a common time axis (the second trails by STAGGER samples),
    from ``tx(cfg, payloads, lead, tail)`` (default: the oracle's transmitter), and what goes with them."""
    mod, N, occ, CP, R, freqs, transition, plen = ddc_cases.CASES[name]
    from helpers import make_cfg, make_payloads
    cfg = make_cfg(mod, N, occ, CP)
    pays = [make_payloads(4, plen, seed=11), make_payloads(4, plen, seed=29)]
    lead, tail = 2 * N, 3 * N
    if tx is None:
        tx = lambda c, p, lead, tail: orc.tx(c, p, lead=lead, tail=tail)  # noqa: E731
    nb = [np.asarray(tx(cfg, p, lead, tail), np.complex64) for p in pays]
    P = float(np.mean(np.abs(nb[0][lead:len(nb[0]) - tail]) ** 2))
    xa = np.concatenate([nb[0], np.zeros(STAGGER, np.complex64)])
    xb = np.concatenate([np.zeros(STAGGER, np.complex64), nb[1]])
    return dict(cfg=cfg, R=R, freqs=freqs, payloads=pays, x=(xa, xb), P=P, N=N, occ=occ, mod=mod, CP=CP,
                tx_taps=duc.design(R, occ / float(N), transition),
                rx_taps=ddc_cases.ddc.design(R, occ / float(N), transition))


def noise(n, P, R):
    """The wideband noise of ddc_cases._capture: seed 2024, sigma = sqrt(P R / 1e3) -- 30 dB inside one link's band."""
    rng = np.random.default_rng(2024)
    sigma = np.sqrt(P * R / 1e3)
    return sigma * np.sqrt(0.5) * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
