"""A seeded, class-stratified sweep of the core modem (k_tx_mod, k_chan_filter, k_sync, k_sync_exact, k_peak, k_rx_demod,
the deframer) over the geometry ofdm_create accepts.  No GPU and no engine in here: the cases, the classes they are drawn
for, the captures and the reference's own conditioning.  tests/test_core_sweep_cases_host.py holds the module to its
conditions on the CPU, tests/test_gpu_core_sweep.py runs the engine on every case, tests/test_core_geom_host.py compares
the class functions below with what the headers' own functions give (tools/core_geom_check.cpp --table).

Classes.  Every launch decision the host takes from the geometry is a class, restated here from the formulas (filter_F,
sync_class, front_eligible, demod_class); required(N) lists what the cases of one fft_length must hold, check_classes asserts it:
  filter     F = 256 / 512 / 1024 from options at both ends of the band of occupied_tones that gives it (F.lo, F.hi);
             F = 64 and 128 -- and the other three -- with hand-set taps (a Hamming low-pass of exactly ntaps taps
             that passes the occupied band; ntaps = 1 is the tap 1.0) at ntaps = p2/2 + 1 and p2, the largest and the
             smallest block B = F - ntaps + 1 (F.Bmax, F.Bmin); captures shorter than one block, than one round of
             256 / (F / 8) blocks, than two rounds, and longer
  sync       every workgroup count of k_sync<W, fixed> the formulas give for that N (wgW) on both sides of the cyclic
             prefix where it changes; fixed | ring layout, overlay | none, every tiles_per_seg, k_sync_exact's wave-sized
             variant on | off, KEEP on | off; CP = 1, in 2..7, a multiple of 8 and not, N/4, above N/2, N (at N = 4096
             the largest the receiver takes, 2048: the edge itself is in test_gpu_core_sweep.py)
  demod      occupied_tones at the smallest and largest value make_cfg accepts, occ - 16 = 0 and 4 (mod 8: the carrier map
             takes multiples of four only, 2 and 6 are refused by make_cfg -- the host test pins that), all seven modulations, max_fft_shift_len 1, 2, 4, 8, and from N = 2048 on every (twl, smap_lds) the formulas choose
  transmit   symbol counts on both sides of one k_tx_mod workgroup (512 / (N / 8) symbols) where three packets allow it
             (N <= 512), one 0-byte payload in every case
  mix        detector parameters away from their defaults in every fifth case, RANDOM fully random shapes on top

Reference conditioning.  A case's capture is the first step of LADDER[modulation] -- three SNRs times three channel seeds
-- at which the oracle agrees with the float64 model within test_oracle.py's bounds (_tx_against_model,
_rx_against_model, unchanged).  Where no step does, the case is replaced by the next draw of the same geometry (other
payloads).  The choice is made on the reference pair alone; the frozen table below records it (draw, step), and
test_core_sweep_cases_host.py asserts that it is what the ladder gives, that at most 5 % of the cases were replaced, that
the oracle returns a CRC-good packet in at least 90 % of them and a flag and a frame in every one.

Frozen table (PYTHONPATH=. python tests/core_sweep_cases.py prints it): name | draw step | samples flags frames packets crc-good
%(TABLE)s
"""
import numpy as np

from helpers import loopback_stream, make_cfg, make_payloads
from ofdm_uhd_amd import config

SEED = 0x5EED51
NS = (64, 128, 256, 512, 1024, 2048, 4096)
MODS = ("bpsk", "qpsk", "8psk", "qam8", "qam16", "qam64", "qam256")
SHIFTS = (1, 2, 4, 8)
RANDOM = 16
MAX_SAMPLES = 72000
CHANNEL_SEEDS = (0xC0FFEE, 0xBEEF, 0xF00D)
# The ladder goes DOWN from the SNR the constellation works at: what leaves a capture ill-conditioned is a stretch whose
# energy window holds noise alone while the FFT filter's block (up to 1024 samples, rounding relative to its largest
# sample) still holds signal -- test_oracle.py's remark on its WIDE rows -- and a higher noise floor is what cures it.
_SNR0 = {"bpsk": 20.0, "qpsk": 20.0, "8psk": 26.0, "qam8": 26.0, "qam16": 30.0, "qam64": 38.0, "qam256": 45.0}
LADDER = {m: tuple((s - k * max(6.0, (s - 20.0) / 2.0), seed) for k in range(3) for seed in CHANNEL_SEEDS) for m, s in _SNR0.items()}
# detector thresholds (rise, fall) of tests/soak/fuzz_parity.py's draws; the last one raises junk flags by the dozen
DET_RISE_FALL = ((0.1, 0.1), (0.1, 0.2), (0.1, 0.4), (0.3, 0.4), (0.3, 0.2))
_LOW, _HIGH = MODS[:4], MODS[4:]

# ---- the launch decisions, restated (csrc/rx_sync.h, csrc/rx_demod.h) ---------------------------------------------------
TILE, LDS_CU, MAX_WG, GRID_BYTES = 2048, 160 * 1024, 5, 396


def _lp(i):
    return i + (i >> 3)


def _up16(b):
    return (b + 15) & ~15


def filter_F(ntaps):
    p2 = 1
    while p2 < ntaps:
        p2 *= 2
    return max(64, 2 * p2)


def filter_bpr(F):
    return 256 // (F // 8)


def options_ntaps(N, occ):
    """len(config.channel_filter_taps(N, occ)) without designing the filter."""
    from ofdm_uhd_amd import firdes
    bw = (float(occ) / float(N)) / 2.0
    return firdes.compute_ntaps(1.0, bw * 0.08)


def sync_lds(N, CP):
    o = _up16((_lp(N + TILE) + 2) * 8)
    if N > 1000:                                     # no overlay: the tile's M values have a region of their own
        o += _up16((_lp(TILE) + 2) * 4)
    return o + 2 * _up16((_lp(CP) + 2) * 4) + 384


def sync_class(N, CP):
    refused = CP > TILE
    return dict(wg=0 if refused else min(MAX_WG, LDS_CU // sync_lds(N, CP)), fixed=int(N <= TILE), overlay=int(N <= 1000),
                tps=32 * (-(-(N + CP) // TILE)), small=int(N // 2 <= 256), keep=int(N // 2 >= 2048), refused=int(refused))


def _tw_points(n):
    u = 7 * (n // 8 - 1) + 1
    return u + u // 8 + 1


def front_eligible(N, CP, ntaps):
    F = filter_F(ntaps)
    B = F - ntaps + 1
    C = (B + 7) // 8 * 8
    if F > 512 or N + C > TILE or CP > TILE:
        return False
    o = _up16((_lp(N + TILE + C) + 2) * 8) + max(_up16((_lp(TILE) + 2) * 4), 256 * 9 * 8)
    o += 2 * _up16((_lp(CP) + 2) * 4) + _up16(_tw_points(F) * 8) + 384
    return o <= LDS_CU // 3


def demod_lds(N, twl, smap, occ, arity, nmap, nbits, shift, grid, csi):
    shared = _up16((_tw_points(N) if twl else 0) * 8 + arity * 8 + (GRID_BYTES if grid else 0) + (((nmap * 2 + 3) & ~3) if smap else 0))
    hinv = max((occ + 2 * shift + 3) // 2, occ)
    words = (nmap * nbits + 8 + 31) // 32 + 2
    frame = _up16((N + N // 8) * 8 + (hinv + occ) * 8 + (0 if N == 512 else 64) * 4 + ((words + 3) & ~3) * 4 + (2 * occ * 4 if csi else 0))
    return shared + (4 if N == 512 else 1) * frame


def demod_class(N, occ, arity, shift, grid, csi, nmap=None):
    nmap = occ - 2 if nmap is None else nmap
    nbits = (arity - 1).bit_length()
    waves = (4 if N == 512 else 1) * (-(-(N // 8) // 64))

    def lds(twl, smap):
        return demod_lds(N, twl, smap, occ, arity, nmap, nbits, shift, grid, csi)

    def wgs(b):
        return max(1, min(max(1, 16 // waves), LDS_CU // b))
    base = N < 2048
    w0 = wgs(lds(base, False))
    twl = base or (wgs(lds(True, False)) == w0 and lds(True, False) <= LDS_CU)
    smap = wgs(lds(twl, True)) == w0 and lds(twl, True) <= LDS_CU
    return dict(twl=int(twl), smap=int(smap), refused=int(lds(twl, smap) > LDS_CU))


def has_grid(mod):
    return config.MODS[mod] >= 16


# ---- geometry -----------------------------------------------------------------------------------------------------------
_ACCEPTED = {}


def accepted_occ(N):
    """The even occupied_tones make_cfg takes at this fft_length, ascending."""
    if N not in _ACCEPTED:
        out = []
        for occ in range(16, N + 1, 2):
            if options_ntaps(N, occ) > 512:
                continue
            try:
                config.carrier_map(occ, N, "FE7F", sink=False)
                config.carrier_map(occ, occ, "FE7F", sink=True)
            except ValueError:
                continue
            out.append(occ)
        # (the filter design fails where the cut-off passes half the sample rate: find the top by trying)
        while out:
            try:
                make_cfg("bpsk", N, out[-1], 1)
                break
            except ValueError:
                out.pop()
        _ACCEPTED[N] = out
    return _ACCEPTED[N]


def bands(N):
    """{F: (lowest, highest accepted even occupied_tones whose filter from options has that transform length)}"""
    out = {}
    for occ in accepted_occ(N):
        F = filter_F(options_ntaps(N, occ))
        lo, hi = out.get(F, (occ, occ))
        out[F] = (min(lo, occ), max(hi, occ))
    return out


def hand_taps(N, occ, ntaps):
    """A Hamming-windowed low-pass of exactly ntaps taps, unit gain at 0: the cut-off one transition width (what that many
    taps resolve, firdes' rule read backwards) above the occupied band's edge, below half the sample rate."""
    if ntaps == 1:
        return [1.0]
    bw = occ / float(N) / 2.0
    fc = min(bw + 53.0 / (22.0 * ntaps), 0.5 * (bw + 0.5))
    n = np.arange(ntaps) - (ntaps - 1) / 2.0
    h = 2.0 * fc * np.sinc(2.0 * fc * n) * (0.54 - 0.46 * np.cos(2.0 * np.pi * np.arange(ntaps) / (ntaps - 1)))
    return [float(v) for v in (h / h.sum()).astype(np.float32)]


def case_cfg(c):
    cfg = make_cfg(c["mod"], c["N"], c["occ"], c["CP"])
    cfg.max_fft_shift_len = c["shift"]
    if c["ntaps"] is not None:
        taps = hand_taps(c["N"], c["occ"], c["ntaps"])
        cfg.ntaps = len(taps)
        for i in range(len(cfg.taps)):
            cfg.taps[i] = taps[i] if i < len(taps) else 0.0
    if c["det"] is not None:
        cfg.peak_rise, cfg.peak_fall, cfg.peak_alpha, cfg.sampler_timeout = c["det"]
    return cfg


def case_ntaps(c):
    return c["ntaps"] if c["ntaps"] is not None else options_ntaps(c["N"], c["occ"])


def _ncar(c):
    return len(config.carrier_map(c["occ"], c["N"], "FE7F", sink=False))


def packet_symbols(c, size):
    """Preamble + data symbols of one packet (header 4 + payload + CRC 4 + the trailing byte; test_oracle checks the count)."""
    bits = _ncar(c) * (config.MODS[c["mod"]] - 1).bit_length()
    return 1 + -(-8 * (size + 9) // bits)


def case_sizes(c, draw=0):
    """Three or four payloads of 0 .. 300 bytes, one of them empty; shortened until the capture stays below MAX_SAMPLES."""
    rng = np.random.default_rng([SEED, c["index"], draw])
    n = c.get("npkt") or int(rng.integers(3, 5))
    sizes = [int(v) for v in rng.integers(0, c.get("maxlen", 300) + 1, n)]
    sizes[int(rng.integers(0, n))] = 0
    L = c["N"] + c["CP"]
    room = MAX_SAMPLES - (2 * c["N"] + L + 2 * c["N"])
    while sum(packet_symbols(c, s) for s in sizes) * L > room and max(sizes) > 0:
        sizes[int(np.argmax(sizes))] //= 2
    return sizes


def case_payloads(c, draw=0):
    sizes = case_sizes(c, draw)
    return make_payloads(len(sizes), sizes, seed=int(np.random.default_rng([SEED, c["index"], draw, 1]).integers(0, 1 << 30)))


def capture(orc, c, draw, step):
    """(cfg, payloads, x) of the case at one step of its modulation's ladder."""
    cfg, pay = case_cfg(c), case_payloads(c, draw)
    snr, seed = LADDER[c["mod"]][step]
    x = loopback_stream(orc, cfg, pay, snr_db=snr, cfo_bins=c["cfo"], seed=seed)
    x.setflags(write=False)
    return cfg, pay, x


def conditioned(orc, cfg, pay, x):
    """The oracle agrees with the float64 model on this capture, within test_oracle.py's bounds."""
    import test_oracle
    try:
        test_oracle._tx_against_model(orc, cfg, pay)
        test_oracle._rx_against_model(orc, cfg, x)
    except AssertionError:
        return False
    return True


def condition(orc, c, max_draws=3):
    """(draw, step) of the first conditioned capture, None if max_draws draws hold none."""
    for draw in range(max_draws):
        for step in range(len(LADDER[c["mod"]])):
            if conditioned(orc, *capture(orc, c, draw, step)):
                return draw, step
    return None


# ---- the list -----------------------------------------------------------------------------------------------------------
def _occ_near(N, target, residue):
    """The accepted occupied_tones nearest target with occ - 16 = residue (mod 8)."""
    ok = [o for o in accepted_occ(N) if (o - 16) % 8 == residue]
    return min(ok, key=lambda o: (abs(o - target), o))


def _cp_list(N):
    top = min(N, TILE)
    cps = [1, 2 + (N // 64) % 6, N // 4, N // 4 + 3, min(N // 2 + 5, top), top]
    for cp in range(1, top):                         # both sides of every change of k_sync's workgroup count
        if sync_class(N, cp)["wg"] != sync_class(N, cp + 1)["wg"]:
            cps += [cp, cp + 1]
    return cps


_HAND_SMALL, _HAND_128, _HAND_BIG = (1, 17, 32), (33, 64), (65, 128, 129, 256, 257, 512)


def _make_cases():
    rng = np.random.default_rng(SEED)
    cases = []

    def add(kind, N, occ, CP, mod, shift, ntaps=None, det=None, cfo=0.0, **kw):
        c = dict(index=len(cases), kind=kind, N=N, occ=occ, CP=CP, mod=mod, shift=shift, ntaps=ntaps, det=det, cfo=cfo, **kw)
        c["name"] = "%s-%d-%d-%d-%s-s%d%s" % (kind, N, occ, CP, mod, shift, "" if ntaps is None else "-t%d" % ntaps)
        cases.append(c)
        return c

    for k, N in enumerate(NS):
        filt = []
        for F, (lo, hi) in sorted(bands(N).items()):
            filt += [(lo, None), (hi, None)]
        mid = int(0.4 * N)
        filt += [(None, _HAND_SMALL[k % 3]), (None, _HAND_128[k % 2]), (None, _HAND_BIG[k % 6])]
        if N == 64:
            filt.append((None, 64))                   # (seven lengths, six slots: the seventh F = 128 case goes here)
        cps = _cp_list(N)
        short = 0
        for i in range(max(len(filt), len(cps), len(MODS))):
            occ, ntaps = filt[i % len(filt)]
            if occ is None:
                occ = _occ_near(N, mid, 4 * (i % 2))
            det = None
            if i % 5 == 3:                            # detector / sampler parameters as tests/soak/fuzz_parity.py draws them
                det = DET_RISE_FALL[int(rng.integers(0, len(DET_RISE_FALL)))] + (
                    float(rng.choice([0.0003, 0.001, 0.002, 0.005])), int(rng.choice([1000, 7, 2])))
            kw = dict(maxlen=2) if i == 0 else {}     # (three or four packets inside one k_tx_mod workgroup where that can be)
            # a filter block four symbols long and more: the constellations that work at 20 .. 26 dB (the remark at LADDER);
            # the others go to the shorter blocks first
            if filter_F(ntaps if ntaps is not None else options_ntaps(N, occ)) >= 4 * N:
                mod = _LOW[(i + k) % len(_LOW)]
            else:
                mod = (_HIGH + _LOW)[short % len(MODS)]
                short += 1
            add("grid", N, occ, cps[i % len(cps)], mod, SHIFTS[(i + k) % 4], ntaps, det,
                cfo=float((0.0, 0.03, -0.2, 0.05)[i % 4]), **kw)
        if N >= 2048:                                 # every (twl, smap_lds) the formulas choose by themselves
            for want in ((1, 1), (1, 0), (0, 1), (0, 0)):
                for j, occ in enumerate(accepted_occ(N)):
                    mod, shift = MODS[(j + k) % len(MODS)], SHIFTS[j % 4]
                    d = demod_class(N, occ, config.MODS[mod], shift, has_grid(mod), False)
                    if (d["twl"], d["smap"]) == want:
                        add("lds%d%d" % want, N, occ, N // 4 + 8 * len(cases) % 64, mod, shift)
                        break
    # captures shorter than one filter block, than one round, than two (N = 64: nothing longer fits below a block)
    add("short", 64, 40, 16, "qpsk", 2, 257, npkt=1, maxlen=0)
    add("short", 64, 40, 5, "bpsk", 4, 257, npkt=3, maxlen=20)
    add("short", 64, 40, 16, "qam8", 4, 257, npkt=4, maxlen=60)
    for _ in range(RANDOM):
        N = int(rng.choice(NS))
        occ = int(rng.choice(accepted_occ(N)))
        add("rand", N, occ, int(rng.integers(1, min(N, TILE) + 1)), str(rng.choice(MODS)), int(rng.choice(SHIFTS)),
            cfo=float(rng.choice([0.0, 0.0, 0.03, -0.2, 0.45])))
    return cases


def labels(c, nsamples=None):
    """The classes a case belongs to (nsamples: its capture's length, for the filter's round classes)."""
    N, occ, CP, nt = c["N"], c["occ"], c["CP"], case_ntaps(c)
    F = filter_F(nt)
    out = ["F%d" % F, c["mod"], "shift%d" % c["shift"], "occ%%8=%d" % ((occ - 16) % 8)]
    if c["ntaps"] is None:
        lo, hi = bands(N)[F]
        out += [t for t, v in (("F%d.lo" % F, lo), ("F%d.hi" % F, hi)) if occ == v]
    else:
        p2 = F // 2
        out += [t for t, v in (("F%d.Bmax" % F, p2 // 2 + 1), ("F%d.Bmin" % F, p2), ("nt1", 1)) if nt == v]
    acc = accepted_occ(N)
    out += [t for t, v in (("occmin", acc[0]), ("occmax", acc[-1])) if occ == v]
    s = sync_class(N, CP)
    out += ["wg%d" % s["wg"], "fixed" if s["fixed"] else "ring", "overlay" if s["overlay"] else "nooverlay", "tps%d" % s["tps"],
            "small" if s["small"] else "nosmall", "keep" if s["keep"] else "nokeep"]
    out += [t for t, on in (("cp1", CP == 1), ("cp2-7", 2 <= CP <= 7), ("cp%8=0", CP % 8 == 0), ("cp%8!=0", CP % 8 != 0),
                            ("cp=N/4", CP == N // 4), ("cp>N/2", CP > N // 2), ("cp=top", CP == min(N, TILE))) if on]
    d = demod_class(N, occ, config.MODS[c["mod"]], c["shift"], has_grid(c["mod"]), False)
    out.append("twl%dsmap%d" % (d["twl"], d["smap"]))
    out.append("front" if front_eligible(N, CP, nt) else "nofront")
    nsym = sum(packet_symbols(c, s) for s in case_sizes(c, c.get("draw", 0)))
    out.append("tx<=wg" if nsym <= 512 // (N // 8) else "tx>wg")
    if c["det"] is not None:
        out.append("det")
    if nsamples is not None:
        B = F - nt + 1
        rnd = filter_bpr(F) * B
        out.append("len<B" if nsamples < B else "len<round" if nsamples < rnd else "len<2rounds" if nsamples < 2 * rnd else "rounds>2")
    return out


def required(N):
    """What the cases of one fft_length must hold."""
    need = {"occmin", "occmax", "occ%8=0", "occ%8=4", "cp1", "cp2-7", "cp%8=0", "cp%8!=0", "cp=N/4", "cp=top",
            "F64", "F128"}
    if N < 4096:                                     # (at N = 4096 the receiver takes no cyclic prefix above N/2)
        need.add("cp>N/2")
    need |= set(MODS) | {"shift%d" % s for s in SHIFTS}
    for F in bands(N):
        need |= {"F%d.lo" % F, "F%d.hi" % F}
    top = min(N, TILE)
    for cp in range(1, top + 1):
        s = sync_class(N, cp)
        need |= {"wg%d" % s["wg"], "tps%d" % s["tps"]}
    s = sync_class(N, 1)
    need |= {"fixed" if s["fixed"] else "ring", "overlay" if s["overlay"] else "nooverlay", "small" if s["small"] else "nosmall",
             "keep" if s["keep"] else "nokeep"}
    if N >= 2048:
        need |= {"twl1smap1", "twl1smap0", "twl0smap1", "twl0smap0"}
    if N <= 512:
        need |= {"tx<=wg", "tx>wg"}
    need |= {"front", "nofront"} if N <= 1024 else {"nofront"}
    return need


# over the whole list: both block sizes of every transform length, and the four capture lengths
REQUIRED_ANYWHERE = {"F%d.%s" % (F, e) for F in (64, 128, 256, 512, 1024) for e in ("Bmax", "Bmin")} | {
    "nt1", "det", "len<B", "len<round", "len<2rounds", "rounds>2"}


def check_classes(cases, table):
    """Every class present; both sides of every change of k_sync's workgroup count."""
    have_all = set()
    for N in NS:
        have = set()
        for c in cases:
            if c["N"] == N:
                have |= set(labels(c, table[c["name"]]["samples"] if table else None))
        missing = required(N) - have
        assert not missing, (N, sorted(missing))
        cps = {c["CP"] for c in cases if c["N"] == N}
        for cp in range(1, min(N, TILE)):
            if sync_class(N, cp)["wg"] != sync_class(N, cp + 1)["wg"]:
                assert {cp, cp + 1} <= cps, (N, cp)
        have_all |= have
    if table:
        assert not REQUIRED_ANYWHERE - have_all, sorted(REQUIRED_ANYWHERE - have_all)


CASES = _make_cases()
_KEYS = ("draw", "step", "samples", "flags", "frames", "packets", "crc_good")


def _parse_table(text):
    out = {}
    for line in text.splitlines():
        f = line.split()
        if len(f) == len(_KEYS) + 3 and f[1] == "|" and f[4] == "|":
            out[f[0]] = dict(zip(_KEYS, (int(v) for v in f[2:4] + f[5:])))
    return out


TABLE = """
grid-64-32-1-bpsk-s1 | 0 0 | 1101 5 5 0 0
grid-64-56-3-qpsk-s2 | 0 0 | 3204 5 5 4 3
grid-64-16-16-8psk-s4 | 0 2 | 8896 6 5 1 0
grid-64-28-19-qam8-s8 | 0 0 | 6979 4 4 3 3
grid-64-24-37-qam16-s1-t1 | 0 0 | 5811 4 4 3 3
grid-64-28-64-qam64-s2-t33 | 0 2 | 2560 4 4 3 3
grid-64-24-1-8psk-s4-t65 | 0 0 | 1166 4 4 2 2
grid-64-28-3-qam256-s8-t64 | 0 6 | 1998 5 5 1 0
grid-128-64-1-qam16-s2 | 0 0 | 1673 5 5 4 4
grid-128-116-4-qam64-s4 | 0 0 | 1832 5 5 4 4
grid-128-32-32-qam8-s8 | 0 1 | 9152 4 4 2 2
grid-128-60-35-bpsk-s1 | 0 0 | 10781 23 23 0 0
grid-128-16-69-qpsk-s2 | 0 5 | 27107 4 4 2 1
grid-128-28-128-8psk-s4 | 0 0 | 15616 4 4 3 2
grid-128-48-1-qam256-s8-t17 | 0 5 | 3092 7 7 4 3
grid-128-52-4-bpsk-s1-t64 | 0 0 | 12260 5 5 3 3
grid-128-48-32-qpsk-s2-t128 | 0 0 | 2592 3 3 2 2
grid-256-124-1-qam16-s4 | 0 2 | 2823 6 6 3 3
grid-256-236-6-qam64-s8 | 0 2 | 3382 5 5 3 3
grid-256-64-64-qam256-s1 | 0 3 | 3904 4 4 3 2
grid-256-120-67-bpsk-s2 | 0 0 | 16528 5 5 1 1
grid-256-32-133-8psk-s4 | 0 0 | 23975 5 5 4 4
grid-256-60-256-qam8-s8 | 0 0 | 10240 4 4 3 3
grid-256-104-1-qpsk-s1-t32 | 0 0 | 9505 10 10 2 2
grid-256-100-6-8psk-s2-t33 | 0 0 | 4954 6 6 3 3
grid-256-104-64-qam8-s4-t129 | 0 0 | 6784 5 5 3 3
grid-512-244-1-qam16-s8 | 0 0 | 5639 8 8 3 3
grid-512-472-4-qam64-s1 | 0 0 | 5660 5 5 3 2
grid-512-124-128-qam256-s2 | 0 3 | 7808 4 4 3 2
grid-512-240-131-bpsk-s4 | 0 0 | 8478 4 4 3 3
grid-512-64-261-qpsk-s8 | 0 0 | 22919 5 5 4 4
grid-512-120-512-8psk-s1 | 0 0 | 15360 4 4 3 3
grid-512-200-1-qam8-s2-t1 | 0 0 | 8204 6 6 2 2
grid-512-204-4-qam16-s4-t64 | 0 0 | 5660 4 4 3 3
grid-512-200-128-qam64-s8-t256 | 0 2 | 9728 18 18 4 4
grid-1024-484-1-qam16-s1 | 0 0 | 11271 6 6 3 3
grid-1024-948-6-qam64-s2 | 0 1 | 13366 7 7 4 3
grid-1024-244-256-qam256-s4 | 0 0 | 15616 5 5 3 3
grid-1024-480-259-bpsk-s8 | 0 0 | 16926 3 3 3 3
grid-1024-124-517-qpsk-s1 | 0 0 | 42621 5 5 4 4
grid-1024-240-1024-8psk-s2 | 0 0 | 24576 4 4 3 3
grid-1024-408-407-qam8-s4-t17 | 0 0 | 18406 4 4 4 3
grid-1024-412-408-qam16-s8-t33 | 0 0 | 16984 5 5 4 4
grid-1024-408-1-qam64-s1-t257 | 0 1 | 11271 48 48 1 0
grid-2048-964-1-qam16-s2 | 0 0 | 26633 23 23 3 3
grid-2048-1896-4-qam64-s4 | 0 0 | 22556 7 7 3 2
grid-2048-484-512-qam256-s8 | 0 3 | 26112 4 4 3 2
grid-2048-960-515-bpsk-s1 | 0 0 | 41511 4 4 4 4
grid-2048-244-1029-qpsk-s2 | 0 0 | 48193 4 4 3 3
grid-2048-480-2048-8psk-s4 | 0 3 | 40960 3 3 3 3
grid-2048-816-898-qam8-s8-t32 | 0 0 | 28814 3 3 3 2
grid-2048-820-899-qam16-s1-t64 | 0 0 | 28821 3 3 3 3
grid-2048-816-1-qam64-s2-t512 | 0 3 | 26633 11 11 4 3
lds11-2048-244-552-qam64-s1 | 0 0 | 26392 4 4 3 3
lds10-2048-300-560-qam64-s4 | 0 1 | 34272 5 5 4 4
lds01-2048-248-568-qam256-s2 | 0 0 | 26504 4 4 2 2
lds00-2048-1060-512-qam256-s1 | 0 0 | 26112 4 4 3 3
grid-4096-1928-1-qam16-s4 | 0 0 | 53257 30 30 4 4
grid-4096-3792-6-qam64-s8 | 0 0 | 53302 7 7 4 4
grid-4096-964-1024-qam256-s1 | 0 0 | 62464 5 5 4 3
grid-4096-1924-1027-bpsk-s2 | 0 0 | 62491 3 3 3 3
grid-4096-484-2048-qpsk-s4 | 0 3 | 71680 4 4 3 3
grid-4096-960-2048-8psk-s8 | 0 0 | 59392 4 4 3 3
grid-4096-1640-1887-qam8-s1-t1 | 0 0 | 58265 3 3 2 2
grid-4096-1636-1888-qam16-s2-t33 | 0 0 | 58272 3 3 3 3
grid-4096-1640-1-qam64-s4-t65 | 0 0 | 45063 190 190 1 0
lds11-4096-484-1040-qam256-s1 | 0 4 | 62608 5 5 4 4
lds10-4096-540-1048-qam256-s4 | 0 0 | 62680 5 5 4 4
lds01-4096-624-1056-qam256-s8 | 0 1 | 52448 4 4 3 2
lds00-4096-2248-1064-qam256-s2 | 0 0 | 62824 5 5 4 4
short-64-40-16-qpsk-s2-t257 | 0 1 | 496 2 1 1 1
short-64-40-5-bpsk-s4-t257 | 2 4 | 1084 2 1 1 1
short-64-40-16-qam8-s4-t257 | 0 7 | 1776 4 4 3 1
rand-1024-448-413-qam64-s2 | 0 0 | 14155 4 4 2 2
rand-128-64-123-qam64-s4 | 0 1 | 4277 4 4 2 2
rand-4096-496-1238-qam16-s4 | 0 0 | 53722 4 4 3 3
rand-128-44-78-qam16-s4 | 0 0 | 6692 5 5 3 3
rand-256-140-117-qam16-s1 | 0 0 | 5873 5 5 4 4
rand-4096-3448-1668-qam8-s4 | 0 0 | 68260 4 4 4 4
rand-64-44-62-qam16-s8 | 0 0 | 2902 4 4 3 2
rand-512-416-338-qam16-s1 | 0 0 | 8848 4 4 2 2
rand-128-56-54-qpsk-s2 | 0 0 | 6336 4 4 3 2
rand-64-36-42-qam8-s2 | 0 0 | 2270 4 4 2 2
rand-2048-352-1107-bpsk-s2 | 0 0 | 71292 5 5 4 4
rand-512-448-356-qam64-s4 | 0 0 | 8124 4 4 2 2
rand-512-472-327-qam8-s2 | 0 0 | 11277 4 4 4 4
rand-512-356-6-8psk-s8 | 0 0 | 7228 7 7 4 4
rand-256-224-85-qam16-s8 | 0 1 | 5798 5 5 3 3
rand-4096-1044-1878-8psk-s2 | 0 1 | 70150 5 5 3 3
"""
PRECHECK = _parse_table(TABLE)
__doc__ = __doc__.replace("%(TABLE)s", TABLE.strip("\n"))
for _c in CASES:
    if _c["name"] in PRECHECK:
        _c["draw"] = PRECHECK[_c["name"]]["draw"]
assert len({c["name"] for c in CASES}) == len(CASES)
if PRECHECK:
    assert set(PRECHECK) == {c["name"] for c in CASES}, "the frozen table is not this list's"
    check_classes(CASES, PRECHECK)

_REF = {}


def reference(orc, c):
    """(cfg, payloads, x, oracle result with test_gpu_parity's taps) at the frozen draw and step, computed once."""
    if c["name"] not in _REF:
        from test_gpu_parity import oracle_rx
        row = PRECHECK[c["name"]]
        cfg, pay, x = capture(orc, c, row["draw"], row["step"])
        _REF[c["name"]] = (cfg, pay, x, oracle_rx(orc, cfg, x))
    return _REF[c["name"]]


def row_of(ro, x, draw, step):
    good = sum(1 for ok, _ in ro.packets if ok)
    return dict(draw=draw, step=step, samples=len(x), flags=int(ro.stats["peaks"]), frames=int(ro.stats["frames"]),
                packets=len(ro.packets), crc_good=good)


def class_counts(cases, table):
    n = {}
    for c in cases:
        for t in labels(c, table[c["name"]]["samples"] if table else None):
            n[t] = n.get(t, 0) + 1
    return n


if __name__ == "__main__":
    import time
    from oracle import oracle as _orc
    t0 = time.time()
    tab = {}
    for c in CASES:
        got = condition(_orc, c)
        if got is None:
            print("# %s: no conditioned capture" % c["name"])
            continue
        c["draw"] = got[0]
        cfg, pay, x = capture(_orc, c, *got)
        tab[c["name"]] = row_of(_orc.rx(cfg, x, 0), x, *got)
        r = tab[c["name"]]
        print("%s | %d %d | %d %d %d %d %d" % ((c["name"],) + tuple(r[k] for k in _KEYS)))
    print("# %d cases, %.1f s" % (len(CASES), time.time() - t0))
    if len(tab) == len(CASES):
        check_classes(CASES, tab)
        cnt = class_counts(CASES, tab)
        print("# " + ", ".join("%s %d" % kv for kv in sorted(cnt.items())))
