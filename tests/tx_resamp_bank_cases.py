"""Shared by test_tx_resamp_bank_host.py and test_gpu_tx_resamp_bank.py: the float64 model of the transmit resampler
bank (the definition in include/ofdm_hip.h: the sum over the links of the single stage's model at the bank's phase step
per output), its derived error bound, a float32 NumPy emulation of the definition in its own order of operations, and
the shapes the tests use.

The bound.  |out[n] - out64[n]| <= (2 K (Q + 1) + 16) 2^-24 s[n], to first order in 2^-24, before a 16-bit store, with
s[n] = sum_i sum_q |h[p_n + q L]| |x_i[i_n - q]|, the sum of the links' tx_resamp_cases.model bound_sums, and
Q = (ntaps - 1) / L.  The derivation is duc_bank_cases' and carries over term for term (an output has at most Q + 1
taps per link whatever M is):
  - A and B are one chain each of K (Q + 1) packed fused multiply-adds at most; every one rounds once, relative to a
    partial sum whose magnitude sum |c| |xr| bounds, and |c_i[k]| |xr_i[m]| <= |h[k]| |x_i[m]| (1 + a few 2^-24):
    K (Q + 1) 2^-24 s[n] per chain and part;
  - the factor 2 covers combining two parts (A.re and B.im, A.im and B.re) into one complex error;
  - 16 covers what happens once per term or per output: the rounding of the phasor r and of the table entry c (one
    each), the input product x r (two products and one addition per part), the final combine of A and B and the
    optional `add` -- fewer than 16 roundings, each relative to something s[n] (plus |add[n]|) bounds.
The float64 model itself has no phase error against the definition: with n M = k + m L, k G + m E = n D modulo 2^64
exactly, so table angle plus input rotation is the model's rotation by n D (up to float64 rounding of the angles,
about 2^-50).  With ``add`` the magnitude |add[n]| joins s[n].  A 16-bit store adds half a step per part
(pfb_synth_cases.sc16_error).  The bound is wide (the emulation below stays under 0.1 of it); what pins the rotation,
the phase convention and the store are the bit-exact anchors of test_gpu_tx_resamp_bank.py."""
import numpy as np

import duc_bank_cases
import pfb_synth_cases
import tx_resamp_cases
from ofdm_uhd_amd import resample, tx_resample

EPS = 2.0 ** -24
MAX_LINKS = 8
# (K, L, M, ntaps): one link and two at the benchmark's short shape; the most links at its long one; L < M with sizes
# that divide nothing; no resampling at all; the largest ratio with the longest filter; decimation with a short filter;
# a ratio that is not coprime; phases without taps
HOST_SHAPES = [(1, 5, 2, 39), (2, 5, 2, 39), (8, 25, 8, 481), (3, 3, 4, 50), (8, 1, 1, 33), (2, 64, 63, 1024),
               (4, 2, 5, 25), (8, 4, 6, 31), (3, 7, 64, 200)]
FIRSTS = (0, 1000003, 2 ** 40 - 5)

tile_inputs = tx_resamp_cases.tile_inputs
history = tx_resamp_cases.history
count = tx_resamp_cases.count
freqs = duc_bank_cases.freqs
taps_for = duc_bank_cases.taps_for
sc16_error = pfb_synth_cases.sc16_error
_fma32 = duc_bank_cases._fma32
_cmul32v = duc_bank_cases._cmul32v


def stream_inputs(L, M):
    """Inputs per link for about 2 1/3 tiles: no multiple of the tile's inputs nor (M > 1) of the period's."""
    Ti, M = tile_inputs(L, M), int(M)
    n = 2 * Ti + Ti // 3 + 1
    while n % Ti == 0 or (M > 1 and n % M == 0):
        n += 1
    return n


def model_terms(x, h, L, M, fcs, first=0):
    """Per link what model() sums: (K, nout) complex128 and (K, nout) float64."""
    x = np.asarray(x)
    if x.ndim == 1:
        x = x[None]
    assert x.shape[0] == len(fcs)
    ys = [tx_resamp_cases.model(xi, h, L, M, tx_resample.bank_phase_steps(fc, L, M)[2], first) for xi, fc in zip(x, fcs)]
    return np.stack([y for y, _ in ys]), np.stack([s for _, s in ys])


def model(x, h, L, M, fcs, first=0):
    """out64[n], s[n]: the sum over the links of tx_resamp_cases.model(x_i, h, L, M, D_i, first), D_i from
    tx_resample.bank_phase_steps, and of its bound_sums."""
    y, s = model_terms(x, h, L, M, fcs, first)
    return y.sum(axis=0), s.sum(axis=0)


def bound(K, ntaps, L, s, add=None):
    """(2 K (Q + 1) + 16) 2^-24 s[n]; ``add`` joins s (its rounding is among the 16).  See the module docstring."""
    s = np.asarray(s)
    if add is not None:
        s = s + np.abs(np.asarray(add).astype(np.complex128))
    return (2 * int(K) * (history(ntaps, L) + 1) + 16) * EPS * s


def emulate(x, h, L, M, fcs, first=0, add=None):
    """The definition in float32, operation for operation: rotate every input with the once-rounded phasor at m E_i
    (the gr_complex product), then the A and B chains over the links in ascending order and, inside a link, ascending
    q while p_n + q L < ntaps, with the table c_i[k] = complex64(h[k] exp(j 2 pi fc_i k / M));
    v = (A.re - B.im, A.im + B.re); the optional add.  complex64, one sample per output of the call."""
    x = np.asarray(x, np.complex64)
    if x.ndim == 1:
        x = x[None]
    h = np.asarray(h, np.float32)
    L, M, first, ntaps, nin = int(L), int(M), int(first), len(h), x.shape[1]
    Q = history(ntaps, L)
    n0, nout = -(-first * L // M), count(first, nin, L, M)
    pos = [(n0 + j) * M for j in range(nout)]                         # Python integers: no overflow at first = 2^40
    i = np.array([p // L - first for p in pos], np.int64) + Q         # index into the stream with Q zeros in front
    p = np.array([p % L for p in pos], np.int64)
    A = np.zeros((2, nout), np.float32)
    B = np.zeros((2, nout), np.float32)
    m = np.uint64(first) + np.arange(nin, dtype=np.uint64)
    for xi, fc in zip(x, fcs):
        E = np.uint64(tx_resample.bank_phase_steps(fc, L, M)[1])
        ang = (m * E).astype(np.int64).astype(np.float64) * (2.0 * np.pi / 2.0 ** 64)    # wraps modulo 2^64
        r = (np.cos(ang).astype(np.float32) + 1j * np.sin(ang).astype(np.float32)).astype(np.complex64)
        xr = np.concatenate([np.zeros(Q, np.complex64), _cmul32v(xi, r)])
        c = resample.bandpass_taps(h, fc, M)
        for q in range(Q + 1):
            k = p + q * L
            sel = k < ntaps
            ck, col = c[k[sel]], xr[i[sel] - q]
            sre, sim = col.real.astype(np.float32), col.imag.astype(np.float32)
            cre, cim = ck.real.astype(np.float32), ck.imag.astype(np.float32)
            A[0, sel] = _fma32(cre, sre, A[0, sel])
            A[1, sel] = _fma32(cre, sim, A[1, sel])
            B[0, sel] = _fma32(cim, sre, B[0, sel])
            B[1, sel] = _fma32(cim, sim, B[1, sel])
    re, im = (A[0] - B[1]).astype(np.float32), (A[1] + B[0]).astype(np.float32)
    if add is not None:
        add = np.asarray(add, np.complex64)
        re, im = (re + add.real).astype(np.float32), (im + add.imag).astype(np.float32)
    return (re + 1j * im).astype(np.complex64)


def chunk_inputs(rng, nin, L, M, ntaps):
    """A segmentation of nin inputs per link: 0, 1, Q - 1, Q, Q + 1 and a tile's inputs +- 1 each once in front, then
    random sizes up to two tiles."""
    Q, Ti = history(ntaps, L), tile_inputs(L, M)
    must = [0] + [s for s in (1, Q - 1, Q, Q + 1, Ti - 1, Ti + 1) if s >= 1]
    out, left = [], int(nin)
    for s in must:
        s = min(s, left)
        out.append(s)
        left -= s
    while left:
        s = min(int(rng.integers(0, 2 * Ti + 2)), left)
        out.append(s)
        left -= s
    return out
