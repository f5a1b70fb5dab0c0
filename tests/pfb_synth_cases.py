"""Shared by test_pfb_synth_host.py and test_gpu_pfb_synth.py: the float64 model of the polyphase-FFT synthesis bank (the
definition in include/ofdm_hip.h, restated in NumPy in its direct form: one zero-stuffing interpolator and one rotation
per channel), its derived error bound and the shapes the tests use."""
import numpy as np

import pfb_cases

EPS = 2.0 ** -24
CHANNEL_COUNTS = pfb_cases.CHANNEL_COUNTS
TAP_GRID = pfb_cases.TAP_GRID
taps_for = pfb_cases.taps_for


def tile_inputs(M):
    """Input indices one workgroup of k_pfb_synth takes (PFB_TILE / M in csrc/pfb_synth.h; it produces 4096 outputs): the
    tests pick sizes around it.  A wrong value here only moves the sizes, it cannot make a wrong output pass."""
    return 4096 // int(M)


def history(ntaps, M):
    return (int(ntaps) - 1) // int(M)


def stream_inputs(M):
    """About 2 1/3 tiles of input indices per channel, a multiple of neither the tile nor (M > 2) of M."""
    T = tile_inputs(M)
    n = 2 * T + T // 3 + 1
    while n % T == 0 or (M > 2 and n % M == 0) or n % 2 == 0:
        n += 1
    return n


def model_terms(x, h, M, chans):
    """Per channel what model() sums: (K, nin M) complex128 and (K, nin M) float64."""
    x = np.asarray(x).astype(np.complex128)
    if x.ndim == 1:
        x = x[None]
    h = np.asarray(h).astype(np.float64)
    M = int(M)
    assert x.shape[0] == len(chans)
    nout = x.shape[1] * M
    y = np.zeros((len(chans), nout), np.complex128)
    s = np.zeros((len(chans), nout))
    if nout == 0:
        return y, s
    # output n = first M + j has n mod M = j mod M whatever the stream's first index: the rotation is periodic with M
    p = np.arange(nout) % M
    for i, (xc, c) in enumerate(zip(x, chans)):
        up = np.zeros(nout, np.complex128)
        up[::M] = xc
        y[i] = np.convolve(up, h)[:nout] * np.exp(2j * np.pi * (((int(c) % M) * p) % M) / M)
        s[i] = np.convolve(np.abs(up), np.abs(h))[:nout]
    return y, s


def model(x, h, M, chans):
    """out64[n], s[n] for the K narrowband streams x (shape (K, nin), zeros before their first sample) on the channels
    ``chans`` of M and the real prototype h, over the nin M outputs: per channel zero stuffing, np.convolve with h and
    the rotation exp(2 pi i c n / M), all in float64, summed over the channels;
    s[n] = sum_q |h[qM+p]| sum_c |x_c[m-q]|  (n = m M + p).  The stream's first absolute index does not enter: it moves
    n by a multiple of M."""
    y, s = model_terms(x, h, M, chans)
    return y.sum(axis=0), s.sum(axis=0)


def bound(ntaps, M, s, add=None):
    """|out - out64| <= (Q + 1 + 8 log2 M [+ 1]) 2^-24 s[n], to first order in 2^-24, before a 16-bit store.

    The transform: the M-point radix-2 recursion has log2 M levels; per level one complex product with a once-rounded
    twiddle and one addition, at most 5 roundings to first order, taken as 8 (pfb_cases.bound), each relative to a
    partial sum that sum_c |z_c[m]| bounds: |V_p[m] - V64_p[m]| <= 8 log2 M 2^-24 sum_c |x_c[m]|, and
    |V_p[m]| <= sum_c |x_c[m]|.  The filter: one float32 chain of at most Q + 1 fused multiply-adds per output, at most
    Q + 1 roundings each bounded by 2^-24 times the sum of the magnitudes of its terms, sum_q |h[qM+p]| |V_p[m-q]| <= s[n],
    and it carries the transform's error with weight |h|: together (Q + 1 + 8 log2 M) 2^-24 s[n].  With ``add`` one more
    rounding of a value whose magnitude s[n] + |add[n]| bounds, so |add| joins s.  A 16-bit store adds half a step per
    part: see sc16_error."""
    s = np.asarray(s)
    k = history(ntaps, M) + 1 + 8 * int(np.log2(M))
    if add is not None:
        s = s + np.abs(np.asarray(add).astype(np.complex128))
        k += 1
    return k * EPS * s


def sc16_error(out, want, scale):
    """(err, extra) for a 16-bit store: err[n] = max(|re error|, |im error|), the larger PART's error, and
    extra = 1 / (2 scale), half a step, to be added to bound() -- which bounds the complex error before the store and
    therefore each of its parts.  rint(part * scale) is off by at most half an integer; the scale the tests use is a
    power of two, so the product itself is exact.  (test_gpu_duc.py compares the DUC's 16-bit output the same way.)"""
    d = np.asarray(out).astype(np.complex128) - np.asarray(want).astype(np.complex128)
    return np.maximum(np.abs(d.real), np.abs(d.imag)), 0.5 / float(scale)


def dit(v, w, N=None):
    """The plain radix-2 decimation-in-time recursion of the definition over the last axis of v (length M, a power of
    two), in complex64 with separately rounded float32 operations: t[c] = O[c] w[c M / n] (index 0 not multiplied)."""
    v = np.asarray(v, np.complex64)
    M = len(w)
    n = v.shape[-1] if N is None else N
    if n == 1:
        return v.copy()
    E, Od = dit(v[..., 0::2], w, n // 2), dit(v[..., 1::2], w, n // 2)
    t = Od.copy()
    for c in range(1, n // 2):
        t[..., c] = cmul32(Od[..., c], w[c * M // n])
    return np.concatenate([cadd32(E, t), cadd32(E, -t)], axis=-1)


def cmul32(a, b):
    """gr_complex product: two products and one addition per part, separately rounded in float32."""
    a, b = np.asarray(a, np.complex64), np.complex64(b)
    ar, ai, br, bi = a.real.astype(np.float32), a.imag.astype(np.float32), np.float32(b.real), np.float32(b.imag)
    re = (ar * br).astype(np.float32) - (ai * bi).astype(np.float32)
    im = (ar * bi).astype(np.float32) + (ai * br).astype(np.float32)
    return (re.astype(np.float32) + 1j * im.astype(np.float32)).astype(np.complex64)


def cadd32(a, b):
    a, b = np.asarray(a, np.complex64), np.asarray(b, np.complex64)
    return ((a.real + b.real).astype(np.float32) + 1j * (a.imag + b.imag).astype(np.float32)).astype(np.complex64)


def dit_two_step(v, w):
    """The same transform in the schedule of M = 32, 64: the M2 = M / 8 sub-transforms of size 8 over the entries
    r + M2 k (twiddles w[c M2 ...], i.e. the size-8 recursion on the table w[::M2]), then for every c1 in [0, 8) the
    levels n = 16 .. M on the entries with equal c mod 8: a size-M2 recursion over r whose twiddle for output c2 at the
    level of size n2 is w[(c1 + 8 c) M2 / n2]."""
    v = np.asarray(v, np.complex64)
    M = len(w)
    M1, M2 = 8, M // 8
    sub = np.stack([dit(v[..., r::M2], w[::M2]) for r in range(M2)], axis=-2)      # [..., r, c1]
    out = np.zeros_like(v)
    for c1 in range(M1):
        y = _second(sub[..., :, c1], w, c1, M1, 1)
        for c2 in range(M2):
            out[..., c1 + M1 * c2] = y[..., c2]
    return out


def _second(v, w, c1, m1, ws):
    n = v.shape[-1]
    if n == 1:
        return v.copy()
    E, Od = _second(v[..., 0::2], w, c1, m1, 2 * ws), _second(v[..., 1::2], w, c1, m1, 2 * ws)
    t = Od.copy()
    for c in range(n // 2):
        k = (c1 + m1 * c) * ws
        if k:
            t[..., c] = cmul32(Od[..., c], w[k])
    return np.concatenate([cadd32(E, t), cadd32(E, -t)], axis=-1)


def table(M):
    a = 2.0 * np.pi * np.arange(M) / M
    return (np.cos(a).astype(np.float32) + 1j * np.sin(a).astype(np.float32)).astype(np.complex64)


def chunk_inputs(rng, nin, M, ntaps):
    """A segmentation of nin input indices: pfb_cases.chunk_sizes' sizes divided into input indices, with 0, 1, Q - 1, Q,
    Q + 1 and the tile's inputs +- 1 each once in front."""
    Q, T = history(ntaps, M), tile_inputs(M)
    must = [0] + [s for s in (1, Q - 1, Q, Q + 1, T - 1, T + 1) if s >= 1]
    rest = [s // M for s in pfb_cases.chunk_sizes(rng, max(nin - sum(must), 0) * M + M, M, ntaps)]
    out, left = [], nin
    for s in must + rest:
        s = min(s, left)
        out.append(s)
        left -= s
    if left:
        out.append(left)
    return out
