"""Shared by test_slicer_cases_host.py and test_gpu_slicer.py: captures that drive the receiver's slicer into each of
its three paths and into both of its fall-throughs, the classification of the frame sink's points by the path the
engine takes for them, and a float32 NumPy statement of the engine's three rules next to the full search the oracle runs.

The engine's slicer (csrc/rx_demod.h, the demapper loop) decides a point x = sigrot by one of
  sign   BPSK / QPSK: the signs of the parts index the table directly -- taken while |re| > eps (QPSK: and |im| > eps)
         and both |re|, |im| < bound;
  grid   QAM of arity >= 16: of the four table entries whose levels bracket the two parts the one with the smallest
         distance, ties to the lowest table index -- taken while |re|, |im| <= 64 amax;
  full   8PSK, and whatever the two tests above reject: the first minimum of |x - pos[j]|^2 over the table,
which is what the oracle (sink_slicer) always does.  The constants are those of csrc/engine.hip:421-467:
  sign:  level = |pos[0].re| (QPSK: min(|pos[0].re|, |pos[0].im|)), eps = level * (1/512),
         bound = 8 * max(|pos[0].re|, |pos[0].im|);
  grid:  lr / li the distinct real / imaginary parts in ascending order, amax the largest |part|, bound = 64 amax,
         and the grid is used only while dmin^2 > 2 bound^2 2^-23 (dmin the smallest level spacing);
all of them float32 values.

A capture is made from orc.tx and orc.channel alone, by seed.  Three impairments, each on a whole packet, a clean packet
between impaired ones and one at the end:
  notch   the upper quarter of the occupied carriers is removed from the packet's preamble body (float64 FFT, bins
          zeroed, IFFT, prefix rebuilt), so the equaliser of those carriers is noise^-1, of order 1e2..1e3: points far
          beyond either bound, all finite, and a packet whose CRC fails;
  noisy   white noise 6 dB below the signal over everything behind the second data symbol: the header parses, every
          symbol is demapped, and the points lie anywhere -- near the axes, outside the table, next to midpoints;
  atten   the preamble symbol at 1/20: every point of the packet 20 times the table, beyond the sign slicer's bound.
"""
import collections

import numpy as np

from helpers import make_cfg, make_payloads
from ofdm_uhd_amd import _abi

Row = collections.namedtuple("Row", "mod N occ CP seed plen step plan")
# (the attenuated preamble leads the capture: behind full-scale data the timing metric, normalised by the energy of its
#  later half-window alone, peaks before the weak preamble has begun, and behind a stretch of silence the detector's
#  average is still up from the burst's end -- either way the packet is lost before a point of it reaches the slicer)
SIGN_PLAN = ("atten", "clean", "notch", "clean", "noisy", "clean")
TABLE_PLAN = ("notch", "clean", "noisy", "clean", "noisy", "clean")
# mod, N / occ / CP, seed, payload bytes of packet 0, bytes less per later packet, plan -- the smallest geometry that reaches each code path
ROWS = [
    Row("bpsk", 128, 64, 32, 1, 200, 13, SIGN_PLAN),          # sign_kind 1; a 64-lane wave for 16 threads of work
    Row("qpsk", 512, 200, 128, 2, 300, 13, SIGN_PLAN),        # sign_kind 2, several one-wave frames per workgroup
    Row("qpsk", 64, 48, 16, 3, 500, 13, SIGN_PLAN),           # 8 threads per symbol
    Row("8psk", 256, 120, 64, 4, 300, 13, TABLE_PLAN),        # full search; 3-bit chunks straddle bytes, with wrong bits
    Row("qam16", 256, 120, 64, 5, 300, 13, TABLE_PLAN),       # 4 x 4 grid: nr - 2 = 2, the clamp on every outer point
    Row("qam64", 128, 96, 32, 6, 300, 13, TABLE_PLAN),        # 8 x 8 grid
    Row("qam256", 64, 48, 16, 7, 400, 13, TABLE_PLAN),        # 16 x 16 grid: the SlicerGrid arrays are full
    Row("qam256", 512, 200, 128, 8, 400, 13, TABLE_PLAN),     # the grid with several frames per workgroup
    Row("qam16", 2048, 1200, 512, 9, 600, 0, ("notch", "clean", "noisy", "clean")),  # both twiddle instantiations
]
IDS = ["%s-%d" % (r.mod, r.N) for r in ROWS]

NOISE_DB = 70.0          # the channel's noise below the signal, whole capture
NOISY_DB = 6.0           # the noisy packets' own
ATTEN = 1.0 / 20.0
CLEAN_SYMBOLS = 2        # data symbols of a noisy packet left alone (the header sits in the first)


def row(mod, N):
    return ROWS[IDS.index("%s-%d" % (mod, N))]


def _noise(orc, n, sigma, seed):
    z = np.zeros(n, np.complex64)
    orc.channel(z, sigma=sigma, seed=seed)
    return z


def build_capture(orc, cfg, payloads, plan, seed, cfo_bins=0.0):
    """The capture of `payloads` with plan[i] applied to packet i."""
    N, CP, occ = cfg.fft_length, cfg.cp_length, cfg.occupied_tones
    L = N + CP
    lead, tail = 2 * N, L + 2 * N
    x = orc.tx(cfg, payloads, lead=lead, tail=tail)
    psig = float(np.mean(np.abs(x[lead:len(x) - tail]) ** 2))
    start = lead
    for i, (p, what) in enumerate(zip(payloads, plan)):
        nsym = len(orc.tx(cfg, [p])) // L               # preamble + data symbols of this packet
        end = start + nsym * L
        if what == "notch":
            body = np.fft.fftshift(np.fft.fft(x[start + CP:start + L].astype(np.complex128)))
            zl = (N - occ) // 2
            body[zl + 3 * occ // 4:zl + occ + 3] = 0.0
            body = np.fft.ifft(np.fft.ifftshift(body)).astype(np.complex64)
            x[start + CP:start + L] = body
            x[start:start + CP] = body[N - CP:]
        elif what == "noisy":
            # (a packet of two data symbols -- N = 2048 -- keeps the first, which holds the header)
            a = start + (1 + min(CLEAN_SYMBOLS, max(nsym - 2, 1))) * L
            assert a < end
            x[a:end] += _noise(orc, end - a, float(np.sqrt(psig / 10 ** (NOISY_DB / 10.0))), seed * 1000 + i)
        elif what == "atten":
            x[start:start + L] *= np.float32(ATTEN)
        else:
            assert what == "clean"
        start = end
    assert start == len(x) - tail
    orc.channel(x, sigma=float(np.sqrt(psig / 10 ** (NOISE_DB / 10.0))), cfo=cfo_bins * 2 * np.pi / N, seed=seed)
    return x


def impaired_capture(orc, mod, N, occ, CP, seed):
    """(cfg, x, payloads) of the row: everything from the seed."""
    r = row(mod, N)
    assert (r.occ, r.CP) == (occ, CP)
    cfg = make_cfg(mod, N, occ, CP)
    if mod == "bpsk":
        # The stock table is (1 + 0j, -1 + 1.2246469e-16j): psk.py's exp(j pi) keeps the rounding of sin(pi), and
        # ofdm_create recognises a two-point table as a sign table only when both imaginary parts are exactly zero
        # (engine.hip:444).  With the stock table BPSK is therefore decided by the full search (the BPSK rows of
        # test_gpu_parity.CASES cover that); this row hands both sides the exact table, which is what sign_kind 1 serves.
        cfg.constellation[1].im = 0.0
    pay = make_payloads(len(r.plan), [r.plen - r.step * i for i in range(len(r.plan))], seed=seed)
    return cfg, build_capture(orc, cfg, pay, r.plan, seed), pay


RX_TAPS = (_abi.TAP_RX_CHAN_FILT, _abi.TAP_RX_METRIC, _abi.TAP_RX_PRESEL, _abi.TAP_RX_FFT, _abi.TAP_RX_ACQ, _abi.TAP_RX_SINK,
           _abi.TAP_RX_PACKETS)
_REF = {}


def reference(orc, r):
    """(cfg, x, payloads, ro): the row's capture and the oracle's result on it with the taps of test_gpu_parity._check_rx.
    Computed once per row, read-only."""
    key = IDS[ROWS.index(r)]
    if key not in _REF:
        cfg, x, pay = impaired_capture(orc, r.mod, r.N, r.occ, r.CP, r.seed)
        x.setflags(write=False)
        _REF[key] = (cfg, x, pay, orc.rx(cfg, x, sum(1 << t for t in RX_TAPS)))
    return _REF[key]


# ---- the engine's constants and rules, float32 ------------------------------------------------------------------------
F32 = np.float32
Slicer = collections.namedtuple("Slicer", "pos sign_kind sign_idx sign_eps sign_bound grid lr li idx bound")


def table(cfg):
    n = int(cfg.arity)
    return np.array([complex(F32(cfg.constellation[i].re), F32(cfg.constellation[i].im)) for i in range(n)], np.complex64)


def slicer_of(cfg):
    """What ofdm_create derives from the table (engine.hip:391-467), restated."""
    pos = table(cfg)
    re, im = pos.real, pos.imag
    n = len(pos)
    kind, sidx, eps, sbound = 0, None, F32(0), F32(0)
    if n == 2 and im[0] == 0 and im[1] == 0 and re[0] == -re[1] and re[0] != 0:
        kind, sidx = 1, [0, 0, 0, 0]
        sidx[1 if re[0] > 0 else 0] = 0
        sidx[1 if re[1] > 0 else 0] = 1
    elif n == 4:
        a, b = abs(re[0]), abs(im[0])
        ok4, seen, sidx = bool(a > 0 and b > 0), 0, [0, 0, 0, 0]
        for i in range(4):
            if abs(re[i]) != a or abs(im[i]) != b:
                ok4 = False
            ix = (2 if re[i] > 0 else 0) | (1 if im[i] > 0 else 0)
            if seen & (1 << ix):
                ok4 = False
            seen |= 1 << ix
            sidx[ix] = i
        kind = 2 if ok4 else 0
    if kind:
        lvl = abs(re[0]) if kind == 1 else min(abs(re[0]), abs(im[0]))
        eps = F32(lvl) * F32(1.0 / 512.0)
        sbound = F32(8.0) * F32(max(abs(re[0]), abs(im[0])))
    lr, li = np.unique(re), np.unique(im)
    grid = n >= 16 and 2 <= len(lr) <= 16 and 2 <= len(li) <= 16 and len(lr) * len(li) == n
    idx, bound = None, F32(0)
    if grid:
        idx = np.full((len(lr), len(li)), -1, np.int64)
        for i in range(n):
            a, b = int(np.searchsorted(lr, re[i])), int(np.searchsorted(li, im[i]))
            grid = grid and idx[a, b] < 0
            idx[a, b] = i
        amax = F32(max(np.abs(re).max(), np.abs(im).max()))
        bound = F32(64.0) * amax
        dmin = F32(min(np.diff(lr).min(), np.diff(li).min()))
        grid = bool(grid and dmin * dmin > F32(2.0) * bound * bound * F32(1.1920929e-7))
    return Slicer(pos, kind, sidx, eps, sbound, bool(grid), lr, li, idx, bound)


def _dist(x, p):
    """|x - p|^2 as cnorm(csub(x, p)) of csrc/common.h evaluates it: float32, one rounding per operation."""
    dr = x.real.astype(F32) - F32(p.real)
    di = x.imag.astype(F32) - F32(p.imag)
    return dr * dr + di * di


def full_search(s, x):
    """sink_slicer of the oracle: the first minimum of the float32 distances over the table."""
    x = np.asarray(x, np.complex64)
    best = np.zeros(len(x), np.int64)
    with np.errstate(all="ignore"):
        bestd = _dist(x, s.pos[0])
        for j in range(1, len(s.pos)):
            dd = _dist(x, s.pos[j])
            lt = dd < bestd
            bestd = np.where(lt, dd, bestd)
            best = np.where(lt, j, best)
    return best


def paths(s, x):
    """0 = full search, 1 = sign slicer, 2 = grid slicer for every point, by the engine's own tests."""
    x = np.asarray(x, np.complex64)
    with np.errstate(all="ignore"):
        sre, sim = np.abs(x.real), np.abs(x.imag)
        sign = np.zeros(len(x), bool)
        if s.sign_kind:
            sign = (sre > s.sign_eps) & (sre < s.sign_bound) & (sim < s.sign_bound)
            if s.sign_kind == 2:
                sign &= sim > s.sign_eps
        grid = np.zeros(len(x), bool)
        if s.grid:
            grid = ~sign & (sre <= s.bound) & (sim <= s.bound)
    return np.where(sign, 1, np.where(grid, 2, 0))


def engine_rule(s, x, tie_low=True, bounded=True):
    """The engine's decision for every point.  tie_low / bounded exist for the host test's own mutated copies: the
    tie-break turned round, the bound tests taken out."""
    x = np.asarray(x, np.complex64)
    path = paths(s, x)
    if not bounded:
        with np.errstate(all="ignore"):
            sre, sim = np.abs(x.real), np.abs(x.imag)
            if s.sign_kind:
                ok = sre > s.sign_eps
                if s.sign_kind == 2:
                    ok &= sim > s.sign_eps
                path = np.where(ok, 1, 0)
            elif s.grid:
                path = np.where(np.isnan(sre) | np.isnan(sim), 0, 2)
    out = full_search(s, x)
    if s.sign_kind:
        rp, ip = x.real > 0, x.imag > 0
        si = np.asarray(s.sign_idx)
        pick = si[np.where(rp, 1, 0)] if s.sign_kind == 1 else si[np.where(rp, 2, 0) | np.where(ip, 1, 0)]
        out = np.where(path == 1, pick, out)
    if s.grid:
        nr, ni = len(s.lr), len(s.li)
        with np.errstate(all="ignore"):
            ka = np.zeros(len(x), np.int64)
            kb = np.zeros(len(x), np.int64)
            for a in range(1, nr - 1):
                ka += x.real >= s.lr[a]
            for b in range(1, ni - 1):
                kb += x.imag >= s.li[b]
            best = s.idx[ka, kb]
            bestd = _dist_to(s, x, best)
            for c4 in range(1, 4):
                cand = s.idx[ka + (c4 >> 1), kb + (c4 & 1)]
                dd = _dist_to(s, x, cand)
                take = (dd < bestd) | ((dd == bestd) & ((cand < best) if tie_low else (cand > best)))
                bestd = np.where(take, dd, bestd)
                best = np.where(take, cand, best)
        out = np.where(path == 2, best, out)
    return out


def _dist_to(s, x, j):
    p = s.pos[j]
    dr = x.real.astype(F32) - p.real.astype(F32)
    di = x.imag.astype(F32) - p.imag.astype(F32)
    return dr * dr + di * di


def midpoint_near(s, x, frac=0.01):
    """True where a part lies within frac of the level spacing of a decision midpoint of the grid."""
    near = np.zeros(len(x), bool)
    for lv, part in ((s.lr, x.real), (s.li, x.imag)):
        for a in range(len(lv) - 1):
            mid, sp = 0.5 * (float(lv[a]) + float(lv[a + 1])), float(lv[a + 1]) - float(lv[a])
            near |= np.abs(part.astype(np.float64) - mid) <= frac * sp
    return near


def classify(cfg, sink):
    """Counts of the non-zero points of the oracle's TAP_RX_SINK array by what the engine's slicer does with them
    (constants: csrc/engine.hip:421-467, restated in slicer_of):
      n              non-zero points            nonfinite      of them, with a part that is not finite
      sign           on the sign path           sign_eps       rejected for a part inside eps (and inside the bound)
      sign_beyond    rejected for a part at or beyond 8 levels
      grid_inside    on the grid path, both parts within the outermost levels
      grid_outside   on the grid path, a part outside the outermost level
      grid_midpoint  on the grid path, a part within 1 % of a spacing of a decision midpoint
      grid_beyond    rejected by the grid for a part beyond 64 amax
      full           decided by the full search (8PSK: all; otherwise the rejected ones)."""
    s = slicer_of(cfg)
    x = np.asarray(sink, np.complex64).ravel()
    x = x[(x.real != 0) | (x.imag != 0)]
    path = paths(s, x)
    with np.errstate(all="ignore"):
        sre, sim = np.abs(x.real), np.abs(x.imag)
        out = dict.fromkeys(("sign", "sign_eps", "sign_beyond", "grid_inside", "grid_outside", "grid_midpoint", "grid_beyond"), 0)
        out["n"] = len(x)
        out["nonfinite"] = int((~np.isfinite(x.real) | ~np.isfinite(x.imag)).sum())
        out["full"] = int((path == 0).sum())
        if s.sign_kind:
            beyond = ~((sre < s.sign_bound) & (sim < s.sign_bound))
            out["sign"] = int((path == 1).sum())
            out["sign_beyond"] = int(beyond.sum())
            out["sign_eps"] = int(((path != 1) & ~beyond).sum())
        if s.grid:
            on = path == 2
            outer = (x.real < s.lr[0]) | (x.real > s.lr[-1]) | (x.imag < s.li[0]) | (x.imag > s.li[-1])
            out["grid_inside"] = int((on & ~outer).sum())
            out["grid_outside"] = int((on & outer).sum())
            out["grid_midpoint"] = int((on & midpoint_near(s, x)).sum())
            out["grid_beyond"] = int((path == 0).sum())
    return out
