"""Transmit linearisation: a memory polynomial as digital predistorter (DPD) and as power-amplifier (PA) model.

Peaks are limited (cfr.py) because a power amplifier follows the converter, and an amplifier compresses.  The stage
``Engine.dpd`` / ``Engine.pa`` on the GPU (csrc/mempoly.h) is a memory polynomial over the stream,

    y[n] = sum over m < M, k < K of a[m][k] x[n - m] |x[n - m]|^(2 k)        (odd orders 1, 3, .., 2 K - 1)

With one table it is the usual behavioural model of an amplifier (the ``pa`` slot, the air side), with another that
amplifier's predistorter (the ``dpd`` slot, the transmit side, behind CFR and in front of the converter).  This module
holds the host side: the configuration struct, the float64 regressor matrix, the indirect-learning fit (a linear
least-squares problem), a training loop that runs the probe through both slots on the GPU, and the figures derived
from the statistics.

A predistorter holds for the drive level and the peak limit it was trained at: a polynomial amplifier has no inverse
past its compression point, so ``dpd=`` wants ``cfr=`` in front of it (without a peak limit the fit wanders at rms
0.2 and diverges from 0.25 on, against ``example_pa``).
"""
import math

import numpy as np

from . import _abi, iqio

MAX_MEMORY = _abi.OFDM_MEMPOLY_MAX_MEMORY
MAX_ORDERS = _abi.OFDM_MEMPOLY_MAX_ORDERS


def _table(coef):
    a = np.asarray(coef)
    if a.ndim != 2 or not (1 <= a.shape[0] <= MAX_MEMORY and 1 <= a.shape[1] <= MAX_ORDERS):
        raise ValueError("coef has shape (memory, orders) with memory in [1, %d] and orders in [1, %d]" % (MAX_MEMORY, MAX_ORDERS))
    a = a.astype(np.complex64)
    if not np.all(np.isfinite(a.real) & np.isfinite(a.imag)):
        raise ValueError("coef must be finite")
    return a


def mempoly_cfg(coef, out_format="fc32", out_scale=None, limit=None):
    """ofdm_mempoly_cfg for Engine.set_dpd / Engine.set_pa.  ``coef`` has shape (M, K): a[m][k] multiplies
    x[n - m] |x[n - m]|^(2 k); ``out_format`` is "fc32" or "sc16" (``out_scale`` None: 2^15); ``limit`` > 0 is the
    converter's full scale, against which the stage counts (and clamps nothing); None: +inf, nothing is counted.
    Raises ValueError for everything the library refuses."""
    a = _table(coef)
    lim = float("inf") if limit is None else float(np.float32(limit))
    if not lim > 0.0:                               # (NaN fails the comparison)
        raise ValueError("limit must be positive (None: nothing is counted)")
    cfg = _abi.ofdm_mempoly_cfg()
    cfg.struct_size = _abi.C.sizeof(cfg)
    cfg.memory, cfg.orders = a.shape
    cfg.out_format = iqio.FORMATS.index(iqio.check_format(out_format))
    cfg.out_scale = 0.0 if out_scale is None else iqio.check_scale(out_scale, iqio.TX_SCALE)
    cfg.limit = lim
    for m in range(a.shape[0]):
        for k in range(a.shape[1]):
            c = cfg.coef[m * MAX_ORDERS + k]
            c.re, c.im = float(a[m, k].real), float(a[m, k].imag)
    return cfg


def coef_of(cfg):
    """The (M, K) complex64 table of an ofdm_mempoly_cfg."""
    a = np.zeros((cfg.memory, cfg.orders), np.complex64)
    for m in range(cfg.memory):
        for k in range(cfg.orders):
            c = cfg.coef[m * MAX_ORDERS + k]
            a[m, k] = complex(c.re, c.im)
    return a


def identity(memory, orders):
    """The table that returns its input: a[0][0] = 1, every other entry 0."""
    a = np.zeros((int(memory), int(orders)), np.complex64)
    _table(a)
    a[0, 0] = 1.0
    return a


def example_pa():
    """A 3-tap amplifier model with orders 1, 3 and 5 of the kind the DPD literature uses (after Ding et al.): gain
    about 1.05, 1 dB into compression near |x| = 0.45."""
    return np.array([[1.0513 + 0.0904j, -0.0542 - 0.2900j, -0.9657 - 0.7028j],
                     [-0.0680 - 0.0023j, 0.2234 + 0.2317j, -0.2451 - 0.3735j],
                     [0.0289 - 0.0054j, -0.0621 - 0.0932j, 0.1229 + 0.1508j]], np.complex64)


def basis(x, memory, orders):
    """The float64 regressor matrix of a stream (zero before its start): len(x) rows, memory * orders columns, column
    m * orders + k holding x[n - m] |x[n - m]|^(2 k).  ``basis(x, M, K) @ coef.reshape(-1)`` is the float64 model."""
    x = np.asarray(x, np.complex128).reshape(-1)
    M, K = int(memory), int(orders)
    n = len(x)
    B = np.zeros((n, M * K), np.complex128)
    p = np.abs(x) ** 2
    for m in range(min(M, n)):
        col = x[:n - m].copy()
        for k in range(K):
            B[m:, m * K + k] = col
            col = col * p[:n - m]
    return B


def apply64(x, coef):
    """The float64 model of the stage on one whole stream."""
    a = np.asarray(coef, np.complex128)
    return basis(x, a.shape[0], a.shape[1]) @ a.reshape(-1)


def _gain_of(gain, pa_in, pa_out):
    if gain is None:                                # the least-squares complex gain of the amplifier
        den = np.vdot(pa_in, pa_in)
        if den == 0:
            raise ValueError("fit needs a signal")
        return complex(np.vdot(pa_in, pa_out) / den)
    g = np.asarray(gain)
    return complex(g[0, 0] if g.ndim == 2 else g)   # (an amplifier's table: its linear tap)


def fit(pa_in, pa_out, memory, orders, gain=None):
    """Indirect learning: the (memory, orders) table c of the post-inverse, the least-squares solution of
    basis(pa_out / gain) c = pa_in, which is then used as the predistorter.  ``gain`` is the linear gain the
    linearised amplifier is to have: a complex number, or an amplifier's table (its a[0][0]); None: the least-squares
    complex gain from pa_in to pa_out.  Returns complex64."""
    u = np.asarray(pa_in, np.complex128).reshape(-1)
    v = np.asarray(pa_out, np.complex128).reshape(-1)
    if len(u) != len(v):
        raise ValueError("pa_in and pa_out are the same stream before and behind the amplifier")
    M, K = int(memory), int(orders)
    _table(np.zeros((M, K)))
    if len(u) < M * K:
        raise ValueError("fit needs at least memory * orders samples")
    g = _gain_of(gain, u, v)
    c = np.linalg.lstsq(basis(v / g, M, K), u, rcond=None)[0]
    return c.reshape(M, K).astype(np.complex64)


def nmse_db(y, ref):
    """10 log10(sum |y - ref|^2 / sum |ref|^2), in float64."""
    y = np.asarray(y, np.complex128).reshape(-1)
    ref = np.asarray(ref, np.complex128).reshape(-1)
    num, den = float(np.sum(np.abs(y - ref) ** 2)), float(np.sum(np.abs(ref) ** 2))
    if den <= 0.0:
        raise ValueError("nmse_db needs a reference with power")
    return 10.0 * math.log10(num / den) if num > 0.0 else float("-inf")


def train(engine, probe, memory=3, orders=3, iterations=2, gain=None):
    """Fit a predistorter for the amplifier in ``engine``'s ``pa`` slot (Engine.set_pa, complex64 out) on the
    complex64 stream ``probe``: the probe runs through the ``dpd`` slot and the ``pa`` slot on the GPU, fit() on the
    host gives the next table from the amplifier's input and output, the table is loaded, and so ``iterations`` times,
    beginning with identity().  ``gain`` None: the amplifier table's a[0][0].  Returns (coef, nmse): the last table,
    which is left loaded in the ``dpd`` slot (complex64 out, no limit), and for each iteration the NMSE in dB of the
    amplifier's output against gain * probe with that iteration's table in force.  The table holds for the probe's
    level and peak limit."""
    if engine.pa_cfg is None:
        raise ValueError("train() needs the amplifier: Engine.set_pa()")
    if engine.pa_cfg.out_format != _abi.OFDM_IQ_FC32:
        raise ValueError("train() needs the amplifier's output in complex64")
    probe = np.ascontiguousarray(probe, np.complex64).reshape(-1)
    g = _gain_of(coef_of(engine.pa_cfg) if gain is None else gain, None, None)

    def through(coef):
        engine.set_dpd(mempoly_cfg(coef))
        engine.pa_reset()
        u = engine.dpd(probe)
        return u, engine.pa(u)
    coef = identity(memory, orders)
    u, v = through(coef)
    nmse = []
    for _ in range(int(iterations)):
        coef = fit(u, v, memory, orders, g)
        u, v = through(coef)
        nmse.append(nmse_db(v, g * probe.astype(np.complex128)))
    engine.dpd_reset()
    engine.pa_reset()
    return coef, nmse


def _db(ratio):
    return 10.0 * math.log10(ratio) if ratio > 0.0 else float("-inf")


def report(stats):
    """Figures of Engine.dpd_stats() / Engine.pa_stats(): ``gain_db`` the power gain sum_out / sum_in,
    ``peak_expansion_db`` the peak power out over the peak power in (a predistorter expands peaks, an amplifier
    compresses them), ``share_over`` the fraction of outputs above ``limit``."""
    n = int(stats["n"])
    if n == 0:
        raise ValueError("no samples since the statistics were reset")
    return {
        "gain_db": _db(stats["sum_out"] / stats["sum_in"]) if stats["sum_in"] > 0.0 else float("nan"),
        "peak_expansion_db": _db(stats["peak_out"] / stats["peak_in"]) if stats["peak_in"] > 0.0 else float("nan"),
        "share_over": stats["n_over"] / float(n),
    }


def load_coef(path):
    """A coefficient table from a .npy file of shape (M, K) (the command lines' --dpd / --pa FILE.npy)."""
    return _table(np.load(path, allow_pickle=False))
