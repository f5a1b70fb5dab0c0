"""The spectrum stage's float64 model, seeded streams, case list and error bound (csrc/psd.h),
shared by test_psd_host.py and test_gpu_psd.py.

The bound.  A float32 row is compared with the float64 row of the same complex64 samples and float32 taps (both exact in
float64), bin by bin: with X the float64 transform of e = w * x and u = 2^-24,

    D = C * log2(F) * u * ||e||_2,        |P32[k] - P64[k]| <= 2 |X[k]| D + D^2.

The form is that of a transform whose every radix-2 stage adds an error of a few u times the energy that reaches a bin
(for a signal spread over the band, ||e||_2 per stage), the stages' errors added linearly.  C counts the roundings of
csrc/fft.h per radix-2 stage, in its most expensive pass, the twiddled radix-8 pass (three stages):
    twiddle product cmul_f       the table entry rounded from float64 (1 u), then fmaf(a.re, w.re, -(a.im * w.im)): the
                                 inner product and the fused result round once each, 2 u of |a| |w| per part        3 u
    dft8, three levels of cadd / csub, each rounding its result once                                                  3 u
    the odd branch's factor h = float32(sqrt(1/2)) (1 u) and the product by it (1 u)                                  2 u
8 u per three stages: 8/3 u per stage.  The leading radix-2 and radix-4 passes of the lengths that are no power of 8 have
no twiddles and no h: 1 u per stage, below that.  Outside the transform there are three more roundings per bin.  The
window product is 1 u of |e[i]| per part, carried through the transform like an input error: 1 u once, 1/6 u per stage
over the shortest transform's six stages.  The two products and one addition of |X|^2 are 2 u of P, an error of u |X[k]|
in the units of D: one more u per stage covers it as long as |X[k]| <= log2(F) ||e||_2.  ``check_spread`` asserts that of
every modelled row, so a stream for which the form does not hold is refused, not passed.  Rounded up,

    C = 8/3 + 1/6 + 1 -> 4.

The constant was not fitted to the kernel: a complex64 transform of scipy measures 0.64 .. 0.79 of u log2(F) ||e||_2 in
its worst bin, a fifth of this bound, the distance between errors added linearly and in quadrature over 6 to 12 stages.
The kernel's worst error / bound per case is printed by test_gpu_psd.py and recorded in DESIGN.md section 7."""
import numpy as np

from ofdm_uhd_amd import dpd, spectrum, window

U = 2.0 ** -24
C = 4.0
MAX_GRID_BINS = 1 << 21         # csrc/psd_plan.h PSD_PART_BINS


def groups(F):
    """Transforms side by side in one workgroup (sense_groups)."""
    return max(256, F // 8) // (F // 8)


def max_grid(F):
    return min(MAX_GRID_BINS // F, 1024)


def plan(nseg, F):
    """(grid, per): csrc/psd_plan.h restated -- workgroups of a call of ``nseg`` segments and each one's share."""
    G = groups(F)
    if nseg == 0:
        return 0, 0
    rounds_all = -(-nseg // G)
    want = min(rounds_all, max_grid(F))
    per = -(-rounds_all // want) * G
    return -(-nseg // per), per


def samples_for(nseg, F, S):
    """The shortest stream with ``nseg`` segments; F - 1 samples for none."""
    return F - 1 if nseg == 0 else (nseg - 1) * S + F


def welch64(x, F, S, w):
    """The definition in float64: rows (nseg, F), their sum and maximum, nseg.  ``x`` complex, ``w`` the F taps."""
    x = np.asarray(x, np.complex128).reshape(-1)
    w = np.asarray(w, np.float64)
    n = spectrum.segments(len(x), F, S)
    rows = np.zeros((n, F))
    X = np.zeros((n, F), np.complex128)
    norm = np.zeros(n)
    for a in range(0, n, 1024):
        idx = (np.arange(a, min(a + 1024, n)) * S)[:, None] + np.arange(F)[None, :]
        e = x[idx] * w
        X[a:a + len(e)] = np.fft.fft(e, axis=1)
        norm[a:a + len(e)] = np.sqrt(np.sum(np.abs(e) ** 2, axis=1))
    rows = np.abs(X) ** 2
    return {"rows": rows, "X": np.abs(X), "norm": norm, "sum": rows.sum(axis=0), "peak": rows.max(axis=0) if n else np.zeros(F),
            "nseg": n}


def bound(F, absX, norm):
    """The per-bin bound of float32 rows against float64: ``absX`` (nseg, F) the float64 |X|, ``norm`` (nseg,) ||w x||_2."""
    D = (C * np.log2(F) * U * np.asarray(norm, np.float64))[:, None]
    return 2.0 * np.asarray(absX, np.float64) * D + D * D


def check_spread(F, absX, norm):
    """The condition the bound's derivation states: no bin holds more than log2(F) ||e||_2."""
    lim = np.log2(F) * np.asarray(norm, np.float64)[:, None]
    assert np.all(np.asarray(absX) <= lim), "the stream concentrates its energy beyond what the bound's form covers"


def stream(n, seed, fmt="fc32"):
    """Seeded noise of power 1/8 with a tone 20 dB below it off any bin centre; "sc16": int16 (n, 2) at about a quarter
    of full scale.  Returns (what the engine is fed, the same samples as complex64)."""
    rng = np.random.default_rng(seed)
    x = 0.25 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    x = x + 0.035 * np.exp(2j * np.pi * (0.1234567 * np.arange(n) + 0.3))
    if fmt == "sc16":
        q = np.clip(np.rint(np.stack([x.real, x.imag], axis=1) * 8192.0), -32768, 32767).astype(np.int16)
        return q, (q.astype(np.float32) * np.float32(2.0 ** -15)).view(np.complex64).reshape(-1)
    x = x.astype(np.complex64)
    return x, x


def taps(F, seed=None):
    """The sensor's Blackman-Harris window as float32; with a seed, a random positive window (no symmetry to hide a
    reversed index behind)."""
    if seed is None:
        return np.asarray(window.blackmanharris(F), np.float64).astype(np.float32)
    return np.random.default_rng(seed).uniform(0.1, 1.0, F).astype(np.float32)


def _cases():
    out = []
    for F in (64, 512, 1024, 2048, 4096):
        G = groups(F)
        hops = [F, F // 2, F // 4 + 3] + ([1] if F == 64 else [])
        for S in hops:
            counts = sorted({0, 1, G - 1, G, G + 1, 3 * G + 1})
            for nseg in counts:
                out.append((F, S, nseg))
        # one more than a whole number of shares where a workgroup has more than one round: past the grid's cap
        S = 1 if F == 64 else F // 4 + 3
        nseg = 2 * max_grid(F) * G + 1
        assert plan(nseg, F)[1] > G and (nseg - 1) % plan(nseg - 1, F)[1] == 0
        out.append((F, S, nseg))
    return out


CASES = _cases()
CASE_IDS = ["F%d-S%d-n%d" % c for c in CASES]


# ---- the amplifier chain of the issue: what the transmit chain is for, in ACLR ----------------------------------------
PA_NFFT, PA_HOP, PA_SEGMENTS = 1024, 512, 127
PA_BW, PA_SPACING = 0.2, 0.22          # adjacent bands of the channel's width, 0.02 away


def pa_probe(seed=11):
    """Band-limited Gaussian noise 0.2 cycles/sample wide at rms 0.2, polar-clipped at 7 dB: 127 segments of 1024 at hop
    512."""
    n = samples_for(PA_SEGMENTS, PA_NFFT, PA_HOP)
    rng = np.random.default_rng(seed)
    Xf = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    Xf[np.abs(np.fft.fftfreq(n)) >= PA_BW / 2] = 0.0
    x = np.fft.ifft(Xf)
    x *= 0.2 / np.sqrt(np.mean(np.abs(x) ** 2))
    A = 0.2 * 10.0 ** (7.0 / 20.0)
    m = np.abs(x)
    return (x * np.minimum(1.0, A / np.maximum(m, 1e-300))).astype(np.complex64)


def aclr_of(x):
    """(lower, upper) ACLR in dB of a stream by the float64 model."""
    w = taps(PA_NFFT)
    r = welch64(x, PA_NFFT, PA_HOP, w)
    return spectrum.aclr_db(spectrum.density(r["sum"], r["nseg"], w), 0.0, PA_BW, PA_SPACING)


def fit64(x, pa, rounds=2, memory=3, orders=3):
    """Two rounds of indirect learning in float64 (dpd.train's loop on the host models): the predistorter table."""
    coef = dpd.identity(memory, orders)
    for _ in range(rounds):
        u = dpd.apply64(x, coef)
        v = dpd.apply64(u, pa)
        coef = dpd.fit(u, v, memory, orders, pa)
    return coef
