"""Shared by test_cfr_host.py and test_gpu_cfr.py: the NumPy float32 model of the crest-factor reduction stage (the
definition in include/ofdm_hip.h, operation by operation: NumPy's float32 product, sum, square root and quotient are
correctly rounded, as the kernel's are), its float64 statistics, and the named cases both files run.

A case is a seeded complex Gaussian stream of unit variance per part (rms sqrt(2)), N = 2 * 1024 + 2 H + 301 samples
(two whole tiles, a partial one and more than the longest history), a half-width H, the Hann window cfr.design(H) and a
threshold:
  none    1.5 times the stream's largest magnitude: nothing is touched
  papr7   7 dB over the rms: 0.7 % of the samples are over (exp(-10^0.7)); tiles with and without peaks, and waves
          without a peak inside tiles that have some
  under   3 dB under the rms, H = 16 only: 61 % are over, the windows overlap, s passes 1 and b clamps at 0
  all     1e-30: every sample is over"""
import collections

import numpy as np

from ofdm_uhd_amd import cfr

TILE = 1024                       # outputs of one workgroup (csrc/cfr.h: CFR_TILE)
HALF_WIDTHS = (0, 1, 16, 511)
F32 = np.float32

Case = collections.namedtuple("Case", "name H threshold seed")


def stream(n, seed=1):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)


def length(H):
    return 2 * TILE + 2 * H + 301


def rms(x):
    return float(np.sqrt(np.mean(np.abs(x.astype(np.complex128)) ** 2)))


def _cases():
    out = []
    for H in HALF_WIDTHS:
        x = stream(length(H), seed=100 + H)
        r, peak = rms(x), float(np.abs(x.astype(np.complex128)).max())
        out.append(Case("none_h%d" % H, H, 1.5 * peak, 100 + H))
        out.append(Case("papr7_h%d" % H, H, cfr.threshold_for(7.0, r), 100 + H))
        if H == 16:
            out.append(Case("under_h%d" % H, H, cfr.threshold_for(-3.0, r), 100 + H))
        out.append(Case("all_h%d" % H, H, 1e-30, 100 + H))
    return collections.OrderedDict((c.name, c) for c in out)


CASES = _cases()
NAMES = list(CASES)


def input_of(name):
    c = CASES[name]
    return stream(length(c.H), c.seed)


def cfg_of(name, **kw):
    c = CASES[name]
    return cfr.cfr_cfg(c.threshold, cfr.design(c.H), **kw)


Terms = collections.namedtuple("Terms", "y m mm c s b xd")


def model(x, threshold, window, skip_zero_terms=False):
    """The definition on one whole stream (zero before its start): Terms of float32 / complex64 arrays, one entry per
    input.  ``skip_zero_terms``: a term of s whose c is 0 is left out instead of added."""
    x = np.ascontiguousarray(x, np.complex64)
    w = np.asarray(window, F32)
    A = F32(threshold)
    n, H = len(x), (len(w) - 1) // 2
    re, im = x.real.astype(F32), x.imag.astype(F32)
    with np.errstate(all="ignore"):
        mm = re * re + im * im                     # two products, one addition
        m = np.sqrt(mm)
        over = m > A                               # (NaN: False)
        c = np.where(over, F32(1.0) - A / np.where(over, m, F32(1.0)), F32(0.0)).astype(F32)
        cp = np.concatenate([np.zeros(2 * H, F32), c])
        s = np.zeros(n, F32)                       # from +0, ascending k
        for k in range(2 * H + 1):
            ck = cp[2 * H - k:2 * H - k + n]       # c[n - k]
            t = w[k] * ck
            s = np.where(ck != 0, s + t, s) if skip_zero_terms else s + t
        b = np.fmax(F32(0.0), F32(1.0) - s)        # fmaxf
        xd = np.concatenate([np.zeros(H, np.complex64), x])[:n]     # x[n - H]
        y = np.empty(n, np.complex64)
        y.real = b * xd.real
        y.imag = b * xd.imag
    return Terms(y, m, mm, c, s, b, xd)


def statistics(t, threshold):
    """ofdm_cfr_stats of the stream whose Terms are ``t``: counts, float32 maxima, float64 sums of the float32 terms."""
    yr, yi = t.y.real.astype(F32), t.y.imag.astype(F32)
    yy = yr * yr + yi * yi
    er, ei = yr - t.xd.real.astype(F32), yi - t.xd.imag.astype(F32)
    ee = er * er + ei * ei
    return dict(n=len(t.y), n_over=int(np.sum(t.m > F32(threshold))), n_touched=int(np.sum(t.b < F32(1.0))),
                peak_in=float(np.fmax.reduce(t.mm, initial=F32(0.0))), peak_out=float(np.fmax.reduce(yy, initial=F32(0.0))),
                sum_in=float(np.sum(t.mm.astype(np.float64))), sum_out=float(np.sum(yy.astype(np.float64))),
                sum_err=float(np.sum(ee.astype(np.float64))))


def model_of(name):
    c = CASES[name]
    return model(input_of(name), c.threshold, cfr.design(c.H))


def peak_bound(threshold, x):
    """max |y| <= A (1 + 2^-22) + 2^-24 max |x| (include/ofdm_hip.h): four float32 roundings on the path m, A / m,
    1 - c, b x; the subtraction's error is absolute, hence the term in max |x|."""
    return float(F32(threshold)) * (1.0 + 2.0 ** -22) + 2.0 ** -24 * float(np.abs(np.asarray(x, np.complex128)).max())


def polar_clip(x, threshold):
    """H = 0 written out: y = x where |x| <= A, else (1 - (1 - A / m)) x, in float32."""
    x = np.ascontiguousarray(x, np.complex64)
    A = F32(threshold)
    re, im = x.real.astype(F32), x.imag.astype(F32)
    m = np.sqrt(re * re + im * im)
    over = m > A
    g = np.where(over, F32(1.0) - (F32(1.0) - A / np.where(over, m, F32(1.0))), F32(1.0)).astype(F32)
    y = np.empty(len(x), np.complex64)
    y.real, y.imag = g * re, g * im
    return y
