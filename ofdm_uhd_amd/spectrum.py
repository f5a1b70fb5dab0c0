"""Spectrum measurement: Welch power spectral density on the GPU and the figures a transmitter is held to.

``Engine.psd`` (csrc/psd.h) runs an averaged periodogram over any complex stream: windowed segments of ``nfft`` samples
at hop ``hop``, k_sense's float32 transform, a float64 sum and a float32 maximum per bin.  This module holds the host
side: the configuration struct and, in float64 and plain NumPy (no engine needed), what is read off the average -- the
density, the power of a band, the adjacent-channel leakage ratio (ACLR), the occupied bandwidth and the margin to an
emission mask.

Frequencies are in cycles per sample and cyclic.  Arrays are in FFT order unless said otherwise: bin k of F is the
frequency k / F (mod 1) and covers [(k - 1/2) / F, (k + 1/2) / F).  ``ascending`` turns an array into ascending
frequency, -1/2 first, for plots and files.

As a program it measures a file::

    python -m ofdm_uhd_amd.spectrum --from-file x.dat [--sc16] --nfft 1024 [--hop 512] [--channel FC,BW --spacing F]
"""
import math
import sys

import numpy as np

from . import _abi, iqio, window as _window

MAX_FFT = _abi.OFDM_PSD_MAX_FFT
MIN_FFT = 64
WINDOWS = ("blackmanharris", "hanning", "hamming", "rectangular")


def window_taps(window, nfft):
    """``nfft`` float32 taps: a name from window.py or an array of that length."""
    if isinstance(window, str):
        if window not in WINDOWS:
            raise ValueError("window must be one of %s or an array, not %r" % (", ".join(WINDOWS), window))
        w = np.asarray(getattr(_window, window)(nfft), np.float64)
    else:
        w = np.asarray(window, np.float64).reshape(-1)
    if len(w) != nfft:
        raise ValueError("a window has nfft taps")
    w = w.astype(np.float32)
    if not np.all(np.isfinite(w)):
        raise ValueError("a window's taps must be finite")
    if not np.any(w != 0.0):
        raise ValueError("a window's taps must not all be zero")
    return w


def psd_cfg(nfft, hop=None, window="blackmanharris", in_format="fc32", in_scale=None):
    """ofdm_psd_cfg for Engine.set_psd.  ``nfft`` is a power of two in [64, 4096]; ``hop`` in [1, nfft] (None:
    nfft // 2); ``window`` a name from window.py or nfft taps; ``in_format`` "fc32" or "sc16" (``in_scale`` None:
    2^-15).  Raises ValueError for everything the library refuses."""
    if int(nfft) != nfft or not MIN_FFT <= int(nfft) <= MAX_FFT or int(nfft) & (int(nfft) - 1):
        raise ValueError("nfft must be a power of two in [%d, %d]" % (MIN_FFT, MAX_FFT))
    nfft = int(nfft)
    hop = nfft // 2 if hop is None else hop
    if int(hop) != hop or not 1 <= int(hop) <= nfft:
        raise ValueError("hop must be an integer in [1, nfft]")
    w = window_taps(window, nfft)
    cfg = _abi.ofdm_psd_cfg()
    cfg.struct_size = _abi.C.sizeof(cfg)
    cfg.nfft = nfft
    cfg.hop = int(hop)
    cfg.in_format = iqio.FORMATS.index(iqio.check_format(in_format))
    cfg.in_scale = 0.0 if in_scale is None else iqio.check_scale(in_scale, iqio.RX_SCALE)
    cfg.taps[:nfft] = [float(v) for v in w]
    return cfg


def taps_of(cfg):
    return np.array(cfg.taps[:cfg.nfft], np.float32)


def segments(n, nfft, hop):
    """Segments complete after ``n`` samples of a stream."""
    return 0 if n < nfft else (n - nfft) // hop + 1


# ---- host-side figures: float64, plain NumPy ---------------------------------------------------------------------------

def density(sum_, nseg, taps):
    """sum / (nseg * sum of w^2): the power per unit of bandwidth, the whole band being 1 -- white noise of power
    sigma^2 reads sigma^2 in every bin, and the mean over the bins is the stream's power."""
    if int(nseg) < 1:
        raise ValueError("no segment since the accumulators were reset")
    w2 = float(np.sum(np.asarray(taps, np.float64) ** 2))
    return np.asarray(sum_, np.float64) / (float(nseg) * w2)


def ascending(a):
    """The half swap: FFT order -> ascending frequency (-1/2 first), along the last axis."""
    a = np.asarray(a)
    return np.roll(a, a.shape[-1] // 2, axis=-1)


def freqs(nfft, order="fft"):
    """The bins' centre frequencies in cycles per sample: FFT order, or ``order="ascending"``."""
    f = np.fft.fftfreq(int(nfft))
    return f if order == "fft" else ascending(f)


def _bins(d):
    d = np.asarray(d, np.float64).reshape(-1)
    if len(d) < 1:
        raise ValueError("an empty density")
    return d


def band_power(density, f_lo, f_hi):
    """The power in [f_lo, f_hi): every bin counts by the fraction of its width [(k - 1/2) / F, (k + 1/2) / F) that the
    band covers.  Frequencies are cyclic (a band may pass 1/2 or lie anywhere on the axis); a band wider than 1, or with
    f_hi < f_lo, is refused."""
    d = _bins(density)
    F = len(d)
    f_lo, f_hi = float(f_lo), float(f_hi)
    if not (math.isfinite(f_lo) and math.isfinite(f_hi)) or f_hi < f_lo or f_hi - f_lo > 1.0 + 1e-12:
        raise ValueError("a band is [f_lo, f_hi) with f_lo <= f_hi <= f_lo + 1")
    u_lo, u_hi = f_lo * F + 0.5, f_hi * F + 0.5         # in bins: bin k covers [k, k + 1)
    k = np.arange(math.floor(u_lo), max(math.ceil(u_hi), math.floor(u_lo) + 1))
    frac = np.clip(np.minimum(k + 1.0, u_hi) - np.maximum(k.astype(np.float64), u_lo), 0.0, 1.0)
    return float(np.sum(d[np.mod(k, F)] * frac)) / F


def _db(ratio):
    return 10.0 * math.log10(ratio) if ratio > 0.0 else (float("-inf") if ratio == 0.0 else float("nan"))


def aclr_db(density, center, bandwidth, spacing):
    """(lower, upper): the channel's power over that of the adjacent bands, in dB.  The channel is ``bandwidth`` wide
    around ``center``; the adjacent bands have the same width and lie at center -/+ spacing.  Refused where an adjacent
    band reaches the channel, directly (spacing < bandwidth) or around the axis (spacing + bandwidth > 1)."""
    c, bw, sp = float(center), float(bandwidth), float(spacing)
    if not (bw > 0.0 and sp >= bw and sp + bw <= 1.0 + 1e-12):
        raise ValueError("aclr_db needs 0 < bandwidth <= spacing and spacing + bandwidth <= 1")
    ch = band_power(density, c - bw / 2, c + bw / 2)
    lo = band_power(density, c - sp - bw / 2, c - sp + bw / 2)
    hi = band_power(density, c + sp - bw / 2, c + sp + bw / 2)
    return (_db(ch / lo) if lo > 0.0 else float("inf"), _db(ch / hi) if hi > 0.0 else float("inf"))


def occupied_band(density, share=0.99, center=None):
    """(f_lo, f_hi): the band that holds ``share`` of the power, (1 - share) / 2 of it lying below and as much above.
    The axis is cut opposite ``center`` (None: at -/+ 1/2, centre 0) and the power taken as evenly spread inside a
    bin."""
    d = _bins(density)
    F = len(d)
    if not 0.0 < float(share) < 1.0:
        raise ValueError("share must be in (0, 1)")
    c = 0.0 if center is None else float(center)
    # bins in ascending frequency from c - 1/2: the cut lies at u0 in bin units, the first bin may be a part
    u0 = (c - 0.5) * F + 0.5
    k0 = math.floor(u0)
    k = np.arange(k0, k0 + F + 1)
    lo = np.maximum(k.astype(np.float64), u0)
    hi = np.minimum(k + 1.0, u0 + F)
    wdt = np.clip(hi - lo, 0.0, 1.0)
    p = d[np.mod(k, F)] * wdt
    tot = float(np.sum(p))
    if not tot > 0.0:
        raise ValueError("no power")
    cum = np.concatenate([[0.0], np.cumsum(p)])

    def at(target):
        i = int(np.searchsorted(cum, target, side="right")) - 1
        i = min(max(i, 0), len(p) - 1)
        while p[i] <= 0.0 and i + 1 < len(p):
            i += 1
        inside = (target - cum[i]) / p[i] if p[i] > 0.0 else 0.0
        return (lo[i] + inside * wdt[i] - 0.5) / F

    tail = 0.5 * (1.0 - float(share)) * tot
    return at(tail), at(tot - tail)


def occupied_bandwidth(density, share=0.99, center=None):
    """The width of ``occupied_band``."""
    f_lo, f_hi = occupied_band(density, share, center)
    return f_hi - f_lo


def mask_margin_db(density, mask, center, bandwidth):
    """The smallest margin to an emission mask and where it occurs: (margin_db, at).  ``mask`` is a list of
    ``(offset_lo, offset_hi, limit_dbc)``: between center + offset_lo and center + offset_hi (signed offsets, a segment
    on either side listed separately) the density must stay ``limit_dbc`` (a negative number) relative to the channel's
    mean in-band density.  A segment's worst bin, among those whose centre lies in it, is compared with its limit;
    margin = limit - level, positive inside the mask.  ``at`` = dict(segment=, freq=, level_dbc=, limit_dbc=)."""
    d = _bins(density)
    F = len(d)
    c, bw = float(center), float(bandwidth)
    if not 0.0 < bw <= 1.0:
        raise ValueError("bandwidth must be in (0, 1]")
    ref = band_power(d, c - bw / 2, c + bw / 2) / bw
    if not ref > 0.0:
        raise ValueError("no power in the channel")
    best = None
    for i, (o_lo, o_hi, limit) in enumerate(mask):
        o_lo, o_hi = float(o_lo), float(o_hi)
        if not o_lo < o_hi or o_hi - o_lo > 1.0:
            raise ValueError("a mask segment is (offset_lo, offset_hi, limit_dbc) with offset_lo < offset_hi <= offset_lo + 1")
        k = np.arange(math.ceil((c + o_lo) * F - 1e-9), math.ceil((c + o_hi) * F - 1e-9))   # centres k / F in [lo, hi)
        if len(k) == 0:
            continue
        v = d[np.mod(k, F)]
        j = int(np.argmax(v))
        level = _db(float(v[j]) / ref)
        margin = float(limit) - level
        if best is None or margin < best[0]:
            f = float(k[j]) / F
            best = (margin, dict(segment=i, freq=f - math.floor(f + 0.5), level_dbc=level, limit_dbc=float(limit)))
    if best is None:
        raise ValueError("no bin lies in any mask segment")
    return best


def report(read, cfg, center=None, bandwidth=None, spacing=None, mask=None, share=0.99):
    """The figures of ``Engine.psd_read()`` under the configuration ``cfg`` (an ofdm_psd_cfg, or the window's taps):
    ``density`` and ``peak`` (the max-hold on the density's scale) in FFT order, ``nseg``, ``obw`` (with ``center``
    where given); with ``center`` and ``bandwidth`` the channel's power ``channel_power``; with ``spacing`` too
    ``aclr_db`` = (lower, upper); with ``mask`` ``mask_margin_db`` and ``mask_at``."""
    taps = taps_of(cfg) if hasattr(cfg, "nfft") else np.asarray(cfg, np.float32)
    nseg = int(read["nseg"])
    den = density(read["sum"], nseg, taps)
    w2 = float(np.sum(taps.astype(np.float64) ** 2))
    out = {"density": den, "peak": np.asarray(read["peak"], np.float64) / w2, "nseg": nseg, "nfft": len(den),
           "power": float(np.mean(den)), "obw": occupied_bandwidth(den, share, center)}
    if center is not None and bandwidth is not None:
        out["center"], out["bandwidth"] = float(center), float(bandwidth)
        out["channel_power"] = band_power(den, center - bandwidth / 2.0, center + bandwidth / 2.0)
        if spacing is not None:
            out["aclr_db"] = aclr_db(den, center, bandwidth, spacing)
        if mask is not None:
            out["mask_margin_db"], out["mask_at"] = mask_margin_db(den, mask, center, bandwidth)
    return out


def welch(iq, nfft, hop=None, window="blackmanharris"):
    """The estimator on the host in float64 (numpy.fft): {"sum", "peak", "nseg"} as Engine.psd_read() returns them,
    for streams too short to be worth a GPU and as a cross-check."""
    x = np.asarray(iq, np.complex128).reshape(-1)
    hop = nfft // 2 if hop is None else int(hop)
    w = window_taps(window, nfft).astype(np.float64)
    n = segments(len(x), nfft, hop)
    s, pk = np.zeros(nfft), np.zeros(nfft)
    for a in range(0, n, 256):
        idx = (np.arange(a, min(a + 256, n)) * hop)[:, None] + np.arange(nfft)[None, :]
        P = np.abs(np.fft.fft(x[idx] * w, axis=1)) ** 2
        s += P.sum(axis=0)
        pk = np.maximum(pk, P.max(axis=0))
    return {"sum": s, "peak": pk, "nseg": n}


def main(argv=None):
    import argparse

    from . import engine, options as _options

    ap = argparse.ArgumentParser(prog="python -m ofdm_uhd_amd.spectrum", description="Welch power spectrum of an IQ file on the GPU")
    ap.add_argument("--from-file", required=True, help="IQ samples: complex64, or int16 I,Q pairs with --sc16")
    ap.add_argument("--sc16", action="store_true")
    ap.add_argument("--nfft", type=int, default=1024)
    ap.add_argument("--hop", type=int, default=None)
    ap.add_argument("--window", default="blackmanharris", choices=WINDOWS)
    ap.add_argument("--channel", default=None, metavar="FC,BW", help="the channel's centre and width in cycles per sample")
    ap.add_argument("--spacing", type=float, default=None, help="with --channel: the adjacent channels' distance (ACLR)")
    ap.add_argument("--chunk-samples", type=int, default=1 << 22)
    ap.add_argument("--out", default=None, metavar="FILE.npy", help="the density in ascending frequency")
    a = ap.parse_args(argv)
    try:
        cfg = psd_cfg(a.nfft, a.hop, a.window, "sc16" if a.sc16 else "fc32")
        center = bandwidth = None
        if a.channel is not None:
            center, bandwidth = (float(v) for v in a.channel.split(","))
        if a.spacing is not None and a.channel is None:
            raise ValueError("--spacing needs --channel")
        if a.chunk_samples < 1:
            raise ValueError("--chunk-samples must be positive")
    except ValueError as e:
        ap.error(str(e))
    raw = np.fromfile(a.from_file, np.int16 if a.sc16 else np.complex64)
    if a.sc16:
        raw = raw[:len(raw) // 2 * 2].reshape(-1, 2)
    e = engine.Engine(_options.default_options())
    try:
        e.set_psd(cfg)
        for i in range(0, len(raw), a.chunk_samples):
            e.psd(raw[i:i + a.chunk_samples])
        read = e.psd_read()
    finally:
        e.close()
    if read["nseg"] == 0:
        sys.stderr.write("spectrum: the file holds fewer than nfft samples\n")
        return None
    r = report(read, cfg, center, bandwidth, a.spacing)
    print("segments %d  power %.6g  occupied bandwidth (99%%) %.6f" % (r["nseg"], r["power"], r["obw"]))
    if "channel_power" in r:
        print("channel power %.6g" % r["channel_power"])
    if "aclr_db" in r:
        print("ACLR lower %.2f dB  upper %.2f dB" % r["aclr_db"])
    if a.out:
        np.save(a.out, ascending(r["density"]))
    return r


if __name__ == "__main__":
    main()
