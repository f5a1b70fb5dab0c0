"""Shared by test_mempoly_host.py and test_gpu_mempoly.py: the NumPy float32 model of the memory-polynomial stage (the
definition in include/ofdm_hip.h, operation by operation: NumPy's float32 product and sum are correctly rounded, as the
kernel's are), its statistics, the float64 model with the bound that holds the two together, a stand-in for the engine
that runs dpd.train on the float64 model, and the named cases both files run.

A case is a seeded complex Gaussian stream at rms 0.2 of N = 2 * 1024 + (M - 1) + 301 samples (two whole tiles, a
partial one and more than the history) and a seeded (M, K) table of coefficients of magnitude at most 1, for
(M, K) in {(1, 1), (1, 5), (2, 2), (3, 3), (8, 1), (8, 5)}, plus dpd.example_pa() on a (3, 3) stream.  Everything stays
finite: no NaN payloads are compared."""
import collections

import numpy as np

from ofdm_uhd_amd import dpd

TILE = 1024                       # outputs of one workgroup (csrc/mempoly.h: MPOLY_TILE)
SHAPES = ((1, 1), (1, 5), (2, 2), (3, 3), (8, 1), (8, 5))
RMS = 0.2
F32 = np.float32
EPS = 2.0 ** -24

Case = collections.namedtuple("Case", "name M K seed coef")


def stream(n, seed=1, rms=RMS):
    rng = np.random.default_rng(seed)
    s = rms / np.sqrt(2.0)
    return (s * rng.standard_normal(n) + 1j * s * rng.standard_normal(n)).astype(np.complex64)


def length(M):
    return 2 * TILE + (M - 1) + 301


def table(M, K, seed):
    """Seeded coefficients: magnitudes uniform in [0, 1], phases uniform."""
    rng = np.random.default_rng(seed)
    return (rng.uniform(0.0, 1.0, (M, K)) * np.exp(2j * np.pi * rng.uniform(0.0, 1.0, (M, K)))).astype(np.complex64)


def _cases():
    out = [Case("m%dk%d" % (M, K), M, K, 300 + 10 * M + K, table(M, K, 700 + 10 * M + K)) for M, K in SHAPES]
    out.append(Case("example_pa", 3, 3, 399, dpd.example_pa()))
    return collections.OrderedDict((c.name, c) for c in out)


CASES = _cases()
NAMES = list(CASES)


def input_of(name):
    c = CASES[name]
    return stream(length(c.M), c.seed)


def cfg_of(name, **kw):
    return dpd.mempoly_cfg(CASES[name].coef, **kw)


def _delayed(a, m):
    """a[n - m], zero (+0) before the stream's start"""
    return np.concatenate([np.zeros(m, a.dtype), a])[:len(a)] if m else a


Terms = collections.namedtuple("Terms", "y p yy")


def model(x, coef):
    """The definition on one whole stream (zero before its start): Terms of complex64 / float32 arrays, one entry per
    input.  Every line is one float32 operation per element."""
    x = np.ascontiguousarray(x, np.complex64)
    a = np.asarray(coef, np.complex64)
    M, K = a.shape
    ar, ai = a.real.astype(F32), a.imag.astype(F32)
    re, im = x.real.astype(F32), x.imag.astype(F32)
    rr = re * re
    ii = im * im
    p = rr + ii                                        # two products, one addition
    yr = yi = None
    for m in range(M):
        xr, xi, pm = _delayed(re, m), _delayed(im, m), _delayed(p, m)
        hr = np.full(len(x), ar[m, K - 1], F32)
        hi = np.full(len(x), ai[m, K - 1], F32)
        for k in range(K - 2, -1, -1):                 # Horner from the top: product, then addition
            hr = hr * pm
            hr = hr + ar[m, k]
            hi = hi * pm
            hi = hi + ai[m, k]
        a0, a1 = hr * xr, hi * xi                      # the gr_complex product
        tr = a0 - a1
        b0, b1 = hr * xi, hi * xr
        ti = b0 + b1
        if m == 0:
            yr, yi = tr, ti                            # from t_0, not from +0
        else:
            yr, yi = yr + tr, yi + ti
    assert yr.dtype == F32 and yi.dtype == F32 and p.dtype == F32
    y = np.empty(len(x), np.complex64)
    y.real, y.imag = yr, yi
    q0, q1 = yr * yr, yi * yi
    return Terms(y, p, q0 + q1)


def statistics(t, limit=float("inf")):
    """ofdm_mempoly_stats of the stream whose Terms are ``t``: counts, float32 maxima, float64 sums of the float32 terms."""
    with np.errstate(over="ignore"):
        limit2 = F32(limit) * F32(limit)
    return dict(n=len(t.y), n_over=int(np.sum(t.yy > limit2)),
                peak_in=float(np.fmax.reduce(t.p, initial=F32(0.0))), peak_out=float(np.fmax.reduce(t.yy, initial=F32(0.0))),
                sum_in=float(np.sum(t.p.astype(np.float64))), sum_out=float(np.sum(t.yy.astype(np.float64))))


def model_of(name):
    return model(input_of(name), CASES[name].coef)


def model64(x, coef):
    """The float64 model of the same complex64 inputs and coefficients."""
    return dpd.apply64(np.asarray(x, np.complex64), np.asarray(coef, np.complex64))


def bound(x, coef):
    """|model - model64| per output.  With u = 2^-24 and S_m = sum_k |a[m][k]| p^k |x| at sample n - m: p carries two
    roundings and enters a Horner chain of K - 1 products and K - 1 additions, so a part of h_m is off by at most
    (2 (K - 1) + 2 (K - 1)) u sum_k |a[m][k]| p^k; a part of the complex product adds two roundings of products and
    one of their sum or difference, (4 (K - 1) + 3) u S_m (|xr| + |xi|) / |x| in all; the M - 1 additions add
    (M - 1) u sum_m |t_m|.  With |xr| + |xi| <= sqrt(2) |x| per part and sqrt(2) again for the two parts:
    |error| <= 2 (4 K + M + 4) u sum_m S_m, first order in u with the slack in the constant."""
    x = np.asarray(x, np.complex128)
    a = np.abs(np.asarray(coef, np.complex128))
    M, K = a.shape
    mag, p = np.abs(x), np.abs(x) ** 2
    S = np.zeros(len(x))
    for m in range(M):
        s = sum(a[m, k] * p ** k for k in range(K)) * mag
        S += _delayed(s, m)
    return 2.0 * (4 * K + M + 4) * EPS * S


def polar_clip(x, threshold):
    """float64: magnitudes above the threshold pulled down to it (stands in for CFR where the modem's stream is not
    at hand)."""
    x = np.asarray(x, np.complex128)
    m = np.abs(x)
    return np.where(m > threshold, x * (threshold / np.maximum(m, 1e-300)), x)


class Model64Engine(object):
    """Stands in for Engine in dpd.train: the two slots as the float64 model, whole streams only (train resets the
    slots before every pass)."""

    def __init__(self, pa_coef):
        self.pa_cfg = dpd.mempoly_cfg(pa_coef)
        self.dpd_cfg = None

    def set_dpd(self, cfg):
        self.dpd_cfg = cfg

    def dpd_reset(self):
        pass

    def pa_reset(self):
        pass

    def dpd(self, x):
        return model64(x, dpd.coef_of(self.dpd_cfg)).astype(np.complex64)

    def pa(self, x):
        return model64(x, dpd.coef_of(self.pa_cfg)).astype(np.complex64)
