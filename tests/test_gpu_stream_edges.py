"""Stream cuts where ofdm_demod.feed()'s own arithmetic sits, against the ORACLE on the whole capture.

a. ofdm_rx_set_origin directly: a call on x[o:] with the origin at o gives the whole capture's filtered stream bit for
   bit from the first block of the absolute overlap-save grid whose input window lies inside the call (the first
   multiple of B at or after o + ntaps - 1); in front of it only the missing history differs.

b. feed() over chosen cuts: the packets, and the sequence of flags that became final -- read after every call from
   engine().rx_nco_state() and the call's base (ofdm_demod.stream_position()) -- equal orc.rx's packets and
   OFDM_TAP_RX_PEAKS on the whole capture, every flag exactly once.  (test_gpu_stream.py compares feed() with work();
   here neither side of the comparison is the engine.)  QPSK 64/48/16: span = 33 137 and lookback = 77 824 samples, so
   captures of 150 .. 300 k samples make the carried buffer move."""
import math

import numpy as np
import pytest

import np_model as npm
from helpers import make_cfg, make_payloads, noise_capture
from ofdm_uhd_amd import _abi, config, engine, iqio, ofdm, options

pytestmark = pytest.mark.gpu

GEOM = dict(modulation="qpsk", fft_length=64, occupied_tones=48, cp_length=16)
N, CP, L, T = 64, 16, 80, 2048
SPAN, LOOKBACK = 33137, 77824


def _geometry(cfg):
    """ofdm_demod._stream_geometry restated: one maximum-length packet plus margins, and the detector's look-back."""
    n, ll = cfg.fft_length, cfg.fft_length + cfg.cp_length
    nbits = max(1, int(math.ceil(math.log(cfg.arity, 2))))
    ncar = len(config.carrier_map(cfg.occupied_tones, cfg.occupied_tones, cfg.carrier_map.decode("ascii") or "FE7F"))
    sym_max = int(math.ceil(8.0 * (4 + 4095 + 17) / (ncar * nbits))) + 1
    return (sym_max + 3) * ll + 2 * T + int(cfg.ntaps), (34 + 3 + (ll + T - 1) // T) * T


# ---- a. the origin, directly -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mod,n,occ,cp,fmt", [("qpsk", 64, 48, 16, "fc32"), ("qpsk", 512, 200, 128, "fc32"),
                                              ("qpsk", 512, 200, 128, "sc16")])
def test_origin_keeps_the_filter_grid(orc, mod, n, occ, cp, fmt):
    cfg = make_cfg(mod, n, occ, cp)
    npkt = 6 if n == 64 else 2
    x = orc.tx(cfg, make_payloads(npkt, 150, seed=n), lead=2 * n, tail=3 * n)
    orc.channel(x, sigma=0.005, cfo=0.05 * 2 * np.pi / n, seed=n)
    nt = int(cfg.ntaps)
    B = orc.filter_fft_len(nt) - nt + 1
    origins = (1, B - 1, B, B + 1, 2048, 2049, 3 * B + 7)
    assert len(x) > max(origins) + 2 * B + nt
    eng = engine.Engine(cfg=cfg)
    q = None
    if fmt == "sc16":
        eng.set_rx_iq_format("sc16")
        q = iqio.to_sc16(x)
        x = iqio.from_sc16(q)                        # both sides get the quantised values
    ro = orc.rx(cfg, x, 1 << _abi.TAP_RX_CHAN_FILT)
    whole = ro.tap(_abi.TAP_RX_CHAN_FILT)
    eng.set_taps(_abi.TAP_RX_CHAN_FILT)
    for o in origins:
        eng.set_origin(o)
        eng.rx(x[o:] if q is None else q[o:])
        y = eng.tap(_abi.TAP_RX_CHAN_FILT)
        assert len(y) == len(x) - o
        first = -(-(o + nt - 1) // B) * B            # first block boundary whose window x[m - (ntaps - 1) ..] lies in the call
        assert o + nt - 1 <= first < o + nt - 1 + B
        assert np.array_equal(y[first - o:], whole[first:]), o
        # in front of it: the same filter on a stream that begins at o (zero history), float64
        ref = npm.chan_filter(cfg, x[o:])
        assert np.abs(y[:first - o] - ref[:first - o]).max() <= 1e-5, o
        if o % B:                                    # (and the grid really is the capture's: with origin 0 the bits differ)
            eng.set_origin(0)
            eng.rx(x[o:] if q is None else q[o:])
            assert not np.array_equal(eng.tap(_abi.TAP_RX_CHAN_FILT)[first - o:], whole[first:]), o
    eng.set_origin(0)
    eng.rx(x if q is None else q)
    assert np.array_equal(eng.tap(_abi.TAP_RX_CHAN_FILT), whole)
    eng.close()
    ro.close()


# ---- b. feed() against the oracle ---------------------------------------------------------------------------------------
def _bursts(orc, cfg, seed, n_target, cfo=0.05, snr=30.0, lead=1500, gaps=(200, 4000), sizes=(20, 300)):
    """Bursts of 1 .. 4 packets of mixed sizes separated by silences, AWGN + CFO, at least n_target samples."""
    rng = np.random.default_rng(seed)
    parts, n, k = [np.zeros(lead, np.complex64)], lead, 0
    while n < n_target:
        m = int(rng.integers(1, 5))
        parts.append(orc.tx(cfg, make_payloads(m, rng.integers(sizes[0], sizes[1], m), seed=seed * 1000 + k)))
        parts.append(np.zeros(int(rng.integers(*gaps)), np.complex64))
        n += len(parts[-1]) + len(parts[-2])
        k += 1
    x = np.concatenate(parts)
    psig = float(np.mean(np.abs(parts[1]) ** 2))
    orc.channel(x, sigma=float(np.sqrt(psig / 10 ** (snr / 10))), cfo=cfo * 2 * np.pi / cfg.fft_length, seed=seed)
    return x


_CAPTURES = {}


def _capture(orc, key, make):
    """(cfg, x, ro): a capture and the oracle's result on the whole of it, made once per key, read-only."""
    if key not in _CAPTURES:
        cfg, x = make()
        x.setflags(write=False)
        _CAPTURES[key] = (cfg, x, orc.rx(cfg, iqio.from_sc16(x) if x.dtype == np.int16 else x, 0))
    return _CAPTURES[key]


def _mixed(orc, cfo=0.05, seed=1):
    return _capture(orc, ("mixed", cfo, seed), lambda: (make_cfg("qpsk", N, 48, CP), _bursts(orc, make_cfg("qpsk", N, 48, CP), seed, 250000, cfo)))


def _demod(cfg=None, **kw):
    """An ofdm_demod at 64/48/16.  cfg: a configuration with other detector settings -- ofdm_demod's options do not carry
    them, so the test puts an engine made from it in the place of the demodulator's own."""
    d = ofdm.ofdm_demod(options.default_options(**GEOM), **kw)
    if cfg is not None:
        d.engine().close()
        d._engine = engine.Engine(cfg=cfg)
        d.reset_stream()
    return d


def _feed(d, x, cuts):
    """Feeds x cut at `cuts` (ascending chunk ends; equal neighbours give empty chunks), then flushes.  Returns the
    packets, the flags in the order they became final -- (flag, NCO phase in 2^-64 turn, NCO step, swallowed mark) -- and
    per call (base, total, horizon, start, ran) as feed() must
    have had them -- restated here, and checked against stream_position() after every call."""
    span, lookback = _geometry(d.engine().cfg)
    got, finals, log, a = [], [], [], 0
    assert list(cuts) == sorted(cuts) and cuts[-1] == len(x)
    for b in list(cuts) + [None]:
        flush = b is None
        chunk = x[:0] if flush else x[a:b]
        base, carried, final = d.stream_position()
        total = base + carried + len(chunk)
        assert total == (len(x) if flush else b)
        horizon = total if flush else total - span
        got += d.flush() if flush else d.feed(chunk)
        ran = total > base and horizon > final
        if ran:
            fl, phi, st, sw = d.engine().rx_nco_state()
            fl = fl.astype(np.int64) + base
            assert np.all(np.diff(fl) > 0)
            finals += [(int(fl[j]), int(phi[j]), float(st[j]), int(sw[j])) for j in range(len(fl)) if final < fl[j] <= horizon]
        start = max(base, ((horizon - lookback - span) // T) * T) if horizon > 0 else base
        if not flush:
            assert d.stream_position() == (start, total - start, max(final, horizon) if ran else final)
            a = b
        log.append((base, total, horizon, start, ran))
    assert d.stream_position() == (0, 0, -1)             # flush() ends the stream
    return got, finals, log


def _nco_turns(x):
    """nco_turns of csrc/rx_demod.h: a phase advance in radians as a fraction of a turn in units of 2^-64."""
    t = x * 0.15915494309189533577
    t -= math.floor(t)
    return int(t * 18446744073709551616.0)


def _check(d, x, ro, cuts, marks=None):
    """marks: the swallowed marks one call on the whole capture gives the flags (the oracle does not report them)."""
    got, rows, log = _feed(d, x, cuts)
    finals = [r[0] for r in rows]
    want = ro.tap(_abi.TAP_RX_PEAKS).tolist()
    assert len(finals) == len(set(finals)), "a flag became final twice: %r" % sorted(f for f in set(finals) if finals.count(f) > 1)
    assert finals == want, sorted(set(finals) ^ set(want))[:8]
    assert got == ro.packets
    assert d.n_packets == len(ro.packets) and d.n_ok == sum(ok for ok, _ in ro.packets)
    # the NCO each final flag was settled with, from the oracle's angles: step = float32(-2 / N) * angle, and the phase
    # before flag j + 1 = phase before flag j + turns(step_j * (p_j+1 - p_j)) in integer turns, 0 before the first flag --
    # whichever call settled it, whatever predecessor and filter grid that call was given
    sens = np.float32(-2.0 / d.engine().cfg.fft_length)
    steps = (sens * ro.tap(_abi.TAP_RX_ANGLES).astype(np.float32)).astype(np.float64).tolist()
    assert [r[2] for r in rows] == steps
    phase, phases = 0, []
    for j in range(len(want)):
        phases.append(phase)
        if j + 1 < len(want):
            phase = (phase + _nco_turns(steps[j] * float(int(want[j + 1]) - int(want[j])))) % (1 << 64)
    assert [r[1] for r in rows] == phases
    if marks is not None:
        assert [r[3] for r in rows] == list(marks)
    return log


def _steps(n, step, first=()):
    """Chunk ends: `first`, then every `step` samples up to n."""
    cuts = sorted(first)
    at = cuts[-1] if cuts else 0
    while at + step < n:
        at += step
        cuts.append(at)
    return cuts + [n]


def _flag_near(ro, where):
    pk = ro.tap(_abi.TAP_RX_PEAKS).astype(np.int64)
    return int(pk[np.argmin(np.abs(pk - where))])


def test_stream_geometry_restated(orc):
    cfg = make_cfg("qpsk", N, 48, CP)
    d = _demod()
    assert _geometry(cfg) == (SPAN, LOOKBACK) == tuple(d._stream_geometry()[1:]) and d._stream_geometry()[0] == T
    cfg, x, ro = _mixed(orc)
    assert ro.stats["peaks"] > 100 and ro.stats["chained_frames"] > 0 and ro.stats["crc_ok"] > 30


@pytest.mark.parametrize("d_cut", [-1, 0, 1, 2])
def test_chunk_ends_at_a_flag(orc, d_cut):
    """A chunk ends at p - 1, p, p + 1, p + 2: the flag is the last sample but one, the last, the first of the next chunk
    -- and, carried, is found again with its correlator history in the next call."""
    cfg, x, ro = _mixed(orc)
    p = _flag_near(ro, 180000)
    log = _check(_demod(), x, ro, _steps(len(x), 50000, first=(60000, 120000, p + d_cut)))
    assert log[2][1] == p + d_cut and log[2][3] > 0            # (the carried buffer no longer starts at sample 0)


@pytest.mark.parametrize("d_h", [-1, 0, 1])
def test_horizon_at_a_flag(orc, d_h):
    """The call's horizon is exactly p - 1, p, p + 1: p <= horizon decides whether the flag and its packet are final in
    this call or in the next -- once either way."""
    cfg, x, ro = _mixed(orc)
    p = _flag_near(ro, 100000)
    assert p in [int(f[0]) for f in ro.tap(_abi.TAP_RX_FRAMES)]
    end = p + d_h + SPAN
    log = _check(_demod(), x, ro, _steps(len(x), 40000, first=(50000, end)))
    assert log[1][2] == p + d_h and log[1][4]


def _silence(orc):
    def make():
        cfg = make_cfg("qpsk", N, 48, CP)
        a = orc.tx(cfg, make_payloads(5, [60, 200, 120, 30, 250], seed=31), lead=1500, tail=0)
        b = orc.tx(cfg, make_payloads(4, [100, 40, 220, 90], seed=32), lead=0, tail=40000)
        x = np.concatenate([a, np.zeros(130000, np.complex64), b])
        orc.channel(x, sigma=float(np.sqrt(np.mean(np.abs(a[1500:]) ** 2) / 1000.0)), cfo=0.05 * 2 * np.pi / N, seed=33)
        return cfg, x
    return _capture(orc, "silence", make)


def test_silence_longer_than_the_time_out(orc):
    """Two bursts 130 000 samples apart, chunks of 30 000: the first burst's last frame runs into the sampler's time-out
    (1001 data symbols), the second burst's flags are found on the NO_SIG grid behind it, and by then the last flag
    before them has left the carried buffer -- it reaches the engine only as the history's predecessor."""
    cfg, x, ro = _silence(orc)
    fr = ro.tap(_abi.TAP_RX_FRAMES).astype(np.int64)
    assert (cfg.sampler_timeout + 1) * L < 130000 and fr[:, 1].max() == cfg.sampler_timeout + 1
    gap = int(np.argmax(fr[:, 1]))
    last_a, first_b = int(fr[gap, 0]), int(fr[gap + 1, 0])
    assert first_b - last_a > 130000 and sum(ok for ok, _ in ro.packets) >= 6
    log = _check(_demod(), x, ro, _steps(len(x), 30000))
    assert any(ran and base > last_a and horizon >= first_b for base, total, horizon, start, ran in log)


def test_settled_flag_in_the_first_window_of_a_carried_buffer(orc):
    """The carried buffer starts on the tile grid; a settled flag less than N samples behind that start is one the
    sampler of the next call cannot see (p < N: the engine's n_lo > 0), while the stream has long delivered it."""
    cfg, x, ro = _mixed(orc)
    pk = ro.tap(_abi.TAP_RX_PEAKS).astype(np.int64)
    low = [int(p) for p in pk if p % T < N and 2 * T < p < len(x) - SPAN - LOOKBACK - SPAN - 3 * T]
    assert low, "no flag in the first N samples of a tile: another seed"
    f = low[0]
    # horizon - lookback - span in [tile of f, tile of f + T): start = the tile of f
    total = (f // T) * T + LOOKBACK + SPAN + 100 + SPAN
    log = _check(_demod(), x, ro, _steps(len(x), 45000, first=(total,)))
    base, _, horizon, start, ran = log[0]
    assert ran and start == (f // T) * T and 0 <= f - start < N and f <= horizon
    assert log[1][0] == start and log[1][4]                    # the next call ran on that buffer


def test_coarse_offset_stream(orc):
    """1.3 bins: every frame's equaliser carries the coarse-offset term across the cuts."""
    cfg, x, ro = _mixed(orc, cfo=1.3)
    assert sum(ok for ok, _ in ro.packets) > 20
    _check(_demod(), x, ro, _steps(len(x), 45000))


@pytest.mark.parametrize("side", ["before", "behind"])
def test_swallowed_flag_at_a_cut(orc, side):
    """0.3 bins: first packets of bursts are lost and bogus headers chain frames.  A flag swallowed by an unfinished
    packet lies just before / just behind a cut: the mark travels with the settled history."""
    cfg, x, ro = _mixed(orc, cfo=0.3)
    assert ro.stats["chained_frames"] > 0
    d = _demod()
    one = d.work(x)                                              # (the whole capture once, to learn which flags are swallowed)
    fl, _, _, sw = d.engine().rx_nco_state()
    assert one == ro.packets and fl.tolist() == ro.tap(_abi.TAP_RX_PEAKS).tolist() and sw.any()
    marked = fl[sw != 0].astype(np.int64)
    q = int(marked[np.argmin(np.abs(marked - 170000))])
    d.n_packets = d.n_ok = 0
    _check(d, x, ro, _steps(len(x), 50000, first=(60000, 120000, q + 3 if side == "before" else q - 3)), marks=sw.tolist())


def test_noise_flags_and_a_long_history(orc):
    """peak_alpha 0.0003 with rise / fall 0.8 / 0.6 on noise plus two bursts: runs of u > theta come from the noise alone,
    hundreds of flags settle and every call splices a long history (set_flag_history, trust_after, pred)."""
    def make():
        cfg = make_cfg("qpsk", N, 48, CP)
        cfg.peak_rise, cfg.peak_fall, cfg.peak_alpha = 0.8, 0.6, 0.0003
        x = noise_capture(orc, ntiles=100)
        for at, seed in ((30000, 41), (150000, 42)):
            b = orc.tx(cfg, make_payloads(4, [80, 200, 40, 150], seed=seed))
            x[at:at + len(b)] += b
        return cfg, x
    cfg, x, ro = _capture(orc, "noise", make)
    assert ro.stats["peaks"] > 150
    _check(_demod(cfg), x, ro, _steps(len(x), 40000))


def test_tiny_and_empty_chunks(orc):
    """Chunks of 1, 2, 7 and 0 samples at the start of the stream and in the middle of it."""
    cfg, x, ro = _mixed(orc)
    p = _flag_near(ro, 160000)
    cuts = [1, 3, 10, 10, 70000, 140000, p - 4, p - 3, p - 1, p - 1, p + 6, p + 6, p + 7, 200000, 200000, len(x)]
    _check(_demod(), x, ro, cuts)


def test_sc16_stream(orc):
    def make():
        cfg, x, _ = _mixed(orc)
        return cfg, iqio.to_sc16(x)
    cfg, q, ro = _capture(orc, "sc16", make)
    assert q.dtype == np.int16 and ro.stats["crc_ok"] > 30
    _check(_demod(iq_format="sc16"), q, ro, _steps(len(q), 70000, first=(33333,)))


def test_quality_and_csi_records(orc):
    """Link quality and channel state on: the stream's records are those of one work() call (which
    test_gpu_link_quality.test_stream_records_equal_one_call and test_gpu_csi hold to their models), packets and flags
    the oracle's."""
    cfg, x, ro = _mixed(orc)
    one = ofdm.ofdm_demod(options.default_options(**GEOM), quality_callback=lambda ok, p, q: None, csi=True)
    assert one.work(x) == ro.packets
    want_q, want_c = one.last_quality.copy(), {k: v.copy() for k, v in one.last_csi.items()}
    d = _demod(quality_callback=lambda ok, p, q: None, csi=True)
    got_q, got_c = [], []
    feed = d.feed

    def keep(out):
        got_q.append(d.last_quality.copy())
        got_c.append({k: v.copy() for k, v in d.last_csi.items()})
        return out
    d.feed = lambda chunk, flush=False: keep(feed(chunk, flush=flush))       # (flush() goes through feed)
    _check(d, x, ro, _steps(len(x), 60000, first=(45000,)))
    got_q = np.concatenate(got_q)
    assert len(got_q) == len(want_q) == len(ro.packets)
    for f in engine.QUALITY_DTYPE.names:
        assert np.array_equal(got_q[f], want_q[f], equal_nan=True), f
    for k in want_c:
        assert np.array_equal(np.concatenate([c[k] for c in got_c]), want_c[k], equal_nan=True), k
