"""Shared by test_pfb_host.py and test_gpu_pfb.py: the float64 model of the polyphase-FFT channeliser (the definition in
include/ofdm_hip.h, restated in NumPy in its polyphase form), its derived error bound and the shapes the tests use."""
import numpy as np

import ddc_bank_cases

EPS = 2.0 ** -24
CHANNEL_COUNTS = (2, 4, 8, 16, 32, 64)
# ntaps per M: from {1, M - 1, M, M + 1, 31, 155, 1024}, at most three, 1024 wherever Q or the branch count is largest
TAP_GRID = {2: (1, 3, 1024), 4: (3, 4, 31), 8: (8, 9, 155), 16: (15, 17, 155), 32: (1, 31, 155), 64: (63, 65, 1024)}
# the ddc_cases captures whose two links sit on the grid of their decimation: name -> (M, channels)
ON_GRID = {"qpsk512_r4": (4, (1, 3)), "qam16_2048_r2": (2, (0, 1)), "bpsk64_r8": (8, (2, 6))}


def tile_outputs(M):
    """Output indices one workgroup of k_pfb produces (PFB_TILE / M in csrc/pfb.h): the tests pick sizes around
    tile_outputs * M input samples.  A wrong value here only moves the sizes, it cannot make a wrong output pass."""
    return 4096 // int(M)


def stream_length(M):
    """About 2 1/3 tiles of input, neither a multiple of M nor of the tile."""
    tile = tile_outputs(M) * M
    n = 2 * tile + tile // 3 + 5
    while n % M == 0 or n % tile == 0:
        n += 1
    return n


def count(first, n, M):
    """Outputs m with first <= m M < first + n: ceil((first + n) / M) - ceil(first / M)."""
    return -(-(int(first) + int(n)) // int(M)) - -(-int(first) // int(M))


def model(x, h, M, c, first=0):
    """y64[m], s[m] for the stream x (x[0] has absolute index ``first``, zeros before it), the real prototype h and
    channel c of M, over every m with first <= m M < first + len(x), in float64 and in the polyphase form of the
    definition: u_p[m] = sum_q h[qM+p] x[(m-q)M - p], y[m] = sum_p u_p[m] exp(2 pi i c p / M), which is
    sum_k h[k] exp(2 pi i c k / M) x[mM - k];  s[m] = sum_k |h[k]| |x[mM - k]|."""
    x = np.asarray(x).astype(np.complex128)
    h = np.asarray(h).astype(np.float64)
    M, first = int(M), int(first)
    nout = count(first, len(x), M)
    if nout == 0:
        return np.zeros(0, np.complex128), np.zeros(0)
    m0 = -(-first // M)
    Q = (len(h) - 1) // M
    lo = (m0 - Q) * M - (M - 1)                       # absolute index of the oldest sample any output reaches
    X = np.zeros((nout + Q) * M, np.complex128)       # absolute indices lo .. (m0 + nout - 1) M
    a, b = max(first, lo), min(first + len(x), lo + len(X))
    X[a - lo:b - lo] = x[a - first:b - first]
    y = np.zeros(nout, np.complex128)
    s = np.zeros(nout)
    for p in range(min(M, len(h))):
        xp = X[M - 1 - p::M]                          # xp[t] = x[(m0 - Q + t) M - p]
        hp = h[p::M]
        y += np.convolve(xp, hp)[Q:Q + nout] * np.exp(2j * np.pi * ((c * p) % M) / M)
        s += np.convolve(np.abs(xp), np.abs(hp))[Q:Q + nout]
    return y, s


def bound(ntaps, M, s):
    """|y - y64| <= (Q + 1 + 8 log2 M) 2^-24 s[m]: a float32 chain of at most Q + 1 products per branch; per radix-2
    level one complex product with a once-rounded twiddle and one addition, at most 5 roundings to first order, taken
    as 8; and sum_p |u_p| <= s."""
    Q = (int(ntaps) - 1) // int(M)
    return (Q + 1 + 8 * int(np.log2(M))) * EPS * np.asarray(s)


taps_for = ddc_bank_cases.taps_for


def chunk_sizes(rng, n, M, ntaps):
    """0, 1, M - 1, M, M + 1, ntaps - 2, ntaps - 1, ntaps, 997 and the tile's input +- 1, each once, then random draws."""
    tile = tile_outputs(M) * M
    sizes = [0] + [s for s in (1, M - 1, M, M + 1, ntaps - 2, ntaps - 1, ntaps, 997, tile - 1, tile + 1) if s >= 1]
    out, left, seq = [], n, list(sizes)
    while left > 0:
        s = min(seq.pop(0) if seq else int(rng.choice([v for v in sizes if v >= 16] or [M + 1])), left)
        out.append(s)
        left -= s
    return out
