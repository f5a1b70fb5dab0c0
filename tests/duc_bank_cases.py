"""Shared by test_duc_bank_host.py and test_gpu_duc_bank.py: the float64 model of the DUC bank (the definition in
include/ofdm_hip.h: the sum over the links of the DUC's model), its derived error bound, a float32 NumPy emulation of
the definition in its own order of operations, and the shapes the tests use.

The bound.  |out[n] - out64[n]| <= (2 K (Q + 1) + 16) 2^-24 s[n], to first order in 2^-24, before a 16-bit store, with
s[n] = sum_i sum_q |h[p + q L]| |x_i[m - q]| (n = m L + p), the sum of the links' duc_cases.model bound_sums, and
Q = (ntaps - 1) / L:
  - A and B are one chain each of K (Q + 1) packed fused multiply-adds at most; every one rounds once, relative to a
    partial sum whose magnitude sum |c| |xr| bounds, and |c_i[k]| |xr_i[m]| <= |h[k]| |x_i[m]| (1 + a few 2^-24):
    K (Q + 1) 2^-24 s[n] per chain and part;
  - the factor 2 covers combining two parts (A.re and B.im, A.im and B.re) into one complex error;
  - 16 covers what happens once per term or per output: the rounding of the phasor r and of the table entry c (one
    each), the input product x r (two products and one addition per part), the final combine of A and B and the
    optional `add` -- fewer than 16 roundings, each relative to something s[n] (plus |add[n]|) bounds.
With ``add`` the magnitude |add[n]| joins s[n].  A 16-bit store adds half a step per part (pfb_synth_cases.sc16_error).
The bound is wide (the emulation below stays at or under 0.1 of it); what pins the rotation, the phase convention and
the store are the bit-exact anchors of test_gpu_duc_bank.py."""
import numpy as np

import duc_cases
import pfb_synth_cases
from ofdm_uhd_amd import ddc

EPS = 2.0 ** -24
MAX_LINKS = 8
# (K, L, ntaps): one link; a few; the most, with the long filter of the benchmarks; sizes that divide nothing; no
# interpolation; the largest L with the longest filter; a filter shorter than two rows
HOST_SHAPES = [(1, 4, 31), (3, 4, 31), (8, 8, 155), (5, 3, 50), (8, 1, 33), (2, 64, 1024), (8, 2, 25)]

tile_outputs = duc_cases.tile_outputs
history = duc_cases.history
phase_step = duc_cases.phase_step
sc16_error = pfb_synth_cases.sc16_error


def stream_inputs(L):
    """Inputs per link for about 2 1/3 tiles of outputs: the outputs are no multiple of the tile, the inputs (L > 1)
    none of L."""
    T, L = tile_outputs(L), int(L)
    n = (2 * T + T // 3) // L + 1
    while (n * L) % T == 0 or (L > 1 and n % L == 0):
        n += 1
    return n


def freqs(K):
    """K centre frequencies in [-0.5, 0.5]: off every grid, both signs, zero and an edge among them."""
    base = [0.1875 + 1e-3 / 3.0, -0.3141592653589793, 0.0, 0.5, -0.0625, 0.43, -0.5, 0.26 + 1e-9]
    return base[:int(K)]


def taps_for(rng, ntaps):
    """Real float32 taps of both signs whose magnitudes sum to about 1 per phase-free measure (a gain near 1)."""
    h = rng.standard_normal(int(ntaps)) * np.hamming(int(ntaps) + 2)[1:-1]
    return (h / max(np.sum(np.abs(h)), 1e-30) * 4.0).astype(np.float32)


def model_terms(x, h, L, fcs, first=0):
    """Per link what model() sums: (K, nin L) complex128 and (K, nin L) float64."""
    x = np.asarray(x)
    if x.ndim == 1:
        x = x[None]
    assert x.shape[0] == len(fcs)
    ys = [duc_cases.model(xi, h, L, phase_step(fc), first) for xi, fc in zip(x, fcs)]
    return np.stack([y for y, _ in ys]), np.stack([s for _, s in ys])


def model(x, h, L, fcs, first=0):
    """out64[n], s[n]: the sum over the links of duc_cases.model(x_i, h, L, phase_step(fc_i), first) and of its
    bound_sums."""
    y, s = model_terms(x, h, L, fcs, first)
    return y.sum(axis=0), s.sum(axis=0)


def bound(K, ntaps, L, s, add=None):
    """(2 K (Q + 1) + 16) 2^-24 s[n]; ``add`` joins s (its rounding is among the 16).  See the module docstring."""
    s = np.asarray(s)
    if add is not None:
        s = s + np.abs(np.asarray(add).astype(np.complex128))
    return (2 * int(K) * (history(ntaps, L) + 1) + 16) * EPS * s


def _fma32(a, b, c):
    """float32 fma(a, b, c): the product of two float32 is exact in float64; the sum is rounded to float64 and then to
    float32 (a double rounding that can differ from the fused operation by one float32 ulp in rare ties: far inside
    what the emulation is used for, a check of the bound)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def emulate(x, h, L, fcs, first=0, add=None):
    """The definition in float32, operation for operation: rotate every input with the once-rounded phasor (the
    gr_complex product), then the A and B chains over the links in ascending order and, inside a link, ascending q;
    v = (A.re - B.im, A.im + B.re); the optional add.  complex64 of nin L samples."""
    x = np.asarray(x, np.complex64)
    if x.ndim == 1:
        x = x[None]
    h = np.asarray(h, np.float32)
    L, ntaps, nin = int(L), len(h), x.shape[1]
    Q = history(ntaps, L)
    Are, Aim, Bre, Bim = (np.zeros((nin, L), np.float32) for _ in range(4))
    m = np.uint64(int(first)) + np.arange(nin, dtype=np.uint64)
    for xi, fc in zip(x, fcs):
        E = np.uint64((phase_step(fc) * L) % (1 << 64))
        ang = (m * E).astype(np.int64).astype(np.float64) * (2.0 * np.pi / 2.0 ** 64)    # wraps modulo 2^64
        r = (np.cos(ang).astype(np.float32) + 1j * np.sin(ang).astype(np.float32)).astype(np.complex64)
        xr = np.concatenate([np.zeros(Q, np.complex64), _cmul32v(xi, r)])
        c = ddc.bandpass_taps(h, fc)
        for q in range(Q + 1):
            np_ = min(L, ntaps - q * L)                       # the phases that have tap q
            ck = c[q * L:q * L + np_]
            col = xr[Q - q:Q - q + nin]
            sre, sim = col.real.astype(np.float32)[:, None], col.imag.astype(np.float32)[:, None]
            cre, cim = ck.real.astype(np.float32)[None, :], ck.imag.astype(np.float32)[None, :]
            Are[:, :np_] = _fma32(cre, sre, Are[:, :np_])
            Aim[:, :np_] = _fma32(cre, sim, Aim[:, :np_])
            Bre[:, :np_] = _fma32(cim, sre, Bre[:, :np_])
            Bim[:, :np_] = _fma32(cim, sim, Bim[:, :np_])
    re, im = (Are - Bim).astype(np.float32).reshape(-1), (Aim + Bre).astype(np.float32).reshape(-1)
    if add is not None:
        add = np.asarray(add, np.complex64)
        re, im = (re + add.real).astype(np.float32), (im + add.imag).astype(np.float32)
    return (re + 1j * im).astype(np.complex64)


def _cmul32v(a, b):
    """gr_complex product of two complex64 arrays: two products and one addition per part, separately rounded."""
    ar, ai, br, bi = (v.astype(np.float32) for v in (a.real, a.imag, b.real, b.imag))
    re = (ar * br).astype(np.float32) - (ai * bi).astype(np.float32)
    im = (ar * bi).astype(np.float32) + (ai * br).astype(np.float32)
    return (re.astype(np.float32) + 1j * im.astype(np.float32)).astype(np.complex64)


def chunk_inputs(rng, nin, L, ntaps):
    """A segmentation of nin inputs per link: 0, 1, Q - 1, Q, Q + 1 and the inputs of a tile of outputs +- 1 each once
    in front (as pfb_synth_cases.chunk_inputs has them), then random sizes up to two tiles."""
    Q, Ti = history(ntaps, L), max(tile_outputs(L) // int(L), 1)
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
