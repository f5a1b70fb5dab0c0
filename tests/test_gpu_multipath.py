"""The propagation channel stage on the GPU (csrc/multipath.h, ofdm_set_multipath / ofdm_multipath): against the float64
model within the derived bound (multipath_cases; test_multipath_host.py shows the bound attainable and sharp), bit for
bit across any chunking, at its anchors (the unit profile is the identity and, with sigma and cfo, the flat channel),
through `add`, the refusals, device pointers, and end to end: a selective channel between Engine.tx and Engine.rx, a
primary user in front of the spectrum sensor, the streaming object and the command line.

CPU pre-checks of the two end-to-end scenarios (the float64 model's output fed to the oracle on the CPU):
  selective channel  two_ray at 30 dB, noise seeds 7, 0xC0FFEE and 31: the oracle's receiver decodes 12 of 12 packets with
                     each; the test uses seed 7.
  primary user       sigma 1e-4, one tone of amplitude 0.01 at the centre of sensor bin 40 of 256, 10 messages averaged,
                     dwell 1: the oracle's sensor gives every bin within +-2 of the tone a mean >= 3.3e-2, 25.2 dB above
                     the 1e-4 threshold, and every bin more than 8 away a mean <= 1.39e-6, 18.6 dB below it.  The second
                     margin is the noise's alone (mean bin power sigma^2 sum(w^2) = 6.7e-7, 21.8 dB below; the largest of
                     243 ten-message means lies 3 dB above that) and no amplitude changes it; amplitudes 0.02 and 0.05
                     raise the first to 31 and 39 dB."""
import ctypes as C

import numpy as np
import pytest

import chan_cases
import multipath_cases as mc
import stage_harness as sh
from helpers import make_cfg, make_payloads
from ofdm_uhd_amd import _abi, benchmark_ofdm_rx, benchmark_ofdm_tx, channel_sim, config, csi, engine, iqio, multipath
from stage_harness import eng  # noqa: F401  (the module's engine)

pytestmark = pytest.mark.gpu

N = 2 * mc.TILE + 1023 + 301          # longer than two tiles plus the longest history
STARTS = (0, sh.START, sh.FAR)
TWO53 = 1 << 53


def _run(eng, name, x, first=0, add=None, **kw):
    eng.set_multipath(mc.cfg_of(name, **kw))
    if first:
        eng.multipath_reset(first)
    return eng.multipath(x, add=add)


# ---- 1. the model ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["fc32", "sc16"])
@pytest.mark.parametrize("name", mc.NAMES)
def test_every_profile_lies_within_the_bound_of_the_model(eng, name, fmt):
    x = mc.stream(N, seed=3)
    try:
        worst = [mc.check(_run(eng, name, x, first, out_format=fmt), x, mc.cfg_of(name), first, fmt,
                          "%s %s first %d" % (name, fmt, first)) for first in STARTS]
        assert max(worst) <= 1.0
    finally:
        eng.set_multipath(None)


# ---- 2. segmentation ---------------------------------------------------------------------------------------------------
def _chunk_sizes(dmax):
    return [1, 2, dmax - 1, dmax, dmax + 1, 997, mc.TILE - 1, mc.TILE + 1]


@pytest.mark.parametrize("name,with_add,fmt", [("everything", False, "fc32"), ("everything", True, "fc32"),
                                                 ("everything", True, "sc16"), ("late_only", False, "fc32"),
                                                 ("late_only", True, "fc32"), ("late_only", False, "sc16")])
def test_a_stream_in_chunks_is_the_stream_in_one_call_bit_for_bit(eng, name, with_add, fmt):
    sizes = _chunk_sizes(mc.dmax_of(name))
    n = sum(sizes)
    assert n > 2 * mc.TILE + mc.dmax_of(name)
    x = mc.stream(n, seed=5)
    w = mc.stream(n, seed=6) if with_add else None
    try:
        for first, order in ((sh.START, sizes), (0, sizes[::-1])):
            whole = _run(eng, name, x, first, add=w, out_format=fmt).copy()
            mc.check(whole, x, mc.cfg_of(name), first, fmt, "%s %s whole, first %d" % (name, fmt, first), add=w)
            eng.multipath_reset(first)
            parts, a = [], 0
            for s in order:
                parts.append(eng.multipath(x[a:a + s], add=None if w is None else w[a:a + s]).copy())
                assert len(eng.multipath(x[:0], add=None if w is None else w[:0])) == 0      # a call of no samples in between
                a += s
            got = np.concatenate(parts)
            assert a == n and got.shape == whole.shape
            assert np.array_equal(sh.bits(got), sh.bits(whole)), "%s first %d: chunked differs" % (name, first)
    finally:
        eng.set_multipath(None)


# ---- 3. anchors --------------------------------------------------------------------------------------------------------
def test_the_unit_profile_returns_its_input_and_with_noise_the_flat_channel(eng):
    x = sh.tx_stream(np.random.default_rng(1), 5000)
    try:
        assert np.array_equal(_run(eng, "unit", x), x)
        kw = dict(sigma=0.01, cfo=0.002, seed=chan_cases.BIG_SEED, stream_id=3)
        for first in (0, sh.START, 2 ** 33 + 5):
            want = eng.channel(x, index0=first, **kw)
            assert np.array_equal(_run(eng, "unit", x, first, **kw), want), first
        for kw in (dict(sigma=0.01), dict(cfo=-0.3)):        # the noise-only and the rotation-only kernels
            assert np.array_equal(_run(eng, "unit", x, 77, **kw), eng.channel(x, index0=77, **kw)), kw
    finally:
        eng.set_multipath(None)


# ---- 4. add ------------------------------------------------------------------------------------------------------------
def test_add_is_one_float32_addition_per_part_and_the_16_bit_store_is_the_librarys(eng):
    x, w = mc.stream(N, seed=8), mc.stream(N, seed=9)
    try:
        for name in ("two_ray", "everything"):
            plain = _run(eng, name, x).copy()
            want = sh.part_sum(w, plain)
            eng.multipath_reset(0)
            assert np.array_equal(eng.multipath(x, add=w), want)
            mc.check(want, x, mc.cfg_of(name), 0, "fc32", "add %s" % name, add=w)
            q = _run(eng, name, x, add=w, out_format="sc16")
            assert q.dtype == np.int16 and np.array_equal(q, iqio.to_sc16(want))
            eng.multipath_reset(0)
            assert np.array_equal(eng.multipath(x), iqio.to_sc16(plain))
            # an `add` of another length is refused without moving the stream
            eng.multipath_reset(0)
            half = eng.multipath(x[:1500], add=w[:1500]).copy()
            for bad in (w[:-1], np.concatenate([w, w[:1]])):
                with pytest.raises(ValueError):
                    eng.multipath(x[1500:], add=bad)
            rest = eng.multipath(x[1500:], add=w[1500:])
            assert np.array_equal(np.concatenate([half, rest]), q)
    finally:
        eng.set_multipath(None)


# ---- 5. refusals -------------------------------------------------------------------------------------------------------
NAN, INF = float("nan"), float("inf")


def _arr(field, i, v):
    def put(c):
        if field == "gain":
            c.gain[i].re, c.gain[i].im = v
        else:
            getattr(c, field)[i] = v
    return put


BAD = [
    ("struct_size", lambda c: setattr(c, "struct_size", 12)),
    ("npaths 0", lambda c: setattr(c, "npaths", 0)),
    ("npaths 17", lambda c: setattr(c, "npaths", 17)),
    ("ntones 5", lambda c: setattr(c, "ntones", 5)),
    ("delay 1024", _arr("delay", 3, 1024)),
    ("gain inf", _arr("gain", 2, (INF, 0.0))),
    ("gain nan", _arr("gain", 15, (0.0, NAN))),
    ("doppler above", _arr("doppler", 1, 0.5000001)),
    ("doppler nan", _arr("doppler", 0, NAN)),
    ("tone_amp negative", _arr("tone_amp", 1, -1e-3)),
    ("tone_amp nan", _arr("tone_amp", 3, NAN)),
    ("tone_freq above", _arr("tone_freq", 0, -0.51)),
    ("tone_freq nan", _arr("tone_freq", 2, NAN)),
    ("tone_phase inf", _arr("tone_phase", 2, INF)),
    ("sigma negative", lambda c: setattr(c, "sigma", -1e-3)),
    ("sigma inf", lambda c: setattr(c, "sigma", INF)),
    ("cfo nan", lambda c: setattr(c, "cfo", NAN)),
    ("out_format", lambda c: setattr(c, "out_format", 2)),
    ("out_scale negative", lambda c: (setattr(c, "out_format", 1), setattr(c, "out_scale", -1.0))),
    ("out_scale inf", lambda c: (setattr(c, "out_format", 1), setattr(c, "out_scale", INF))),
]
# one message per refused field: struct_size, npaths, ntones, delay, gain, doppler, tone_amp, tone_freq, tone_phase,
# sigma, cfo, out_format, out_scale
MESSAGES = 13


def _bad_cfg(change):
    c = mc.cfg_of("everything")
    change(c)
    return c


def test_every_bad_field_is_refused_with_its_own_message_and_leaves_what_is_in_force(eng):
    x = mc.stream(N, seed=11)
    msgs = {}
    try:
        # none in force: none afterwards
        eng.set_multipath(None)
        with pytest.raises(ValueError, match="without"):
            eng.multipath(x)
        with pytest.raises(ValueError, match="without ofdm_set_multipath"):
            eng.multipath_reset(0)
        for what, change in BAD:
            with pytest.raises(ValueError) as e:
                eng.set_multipath(_bad_cfg(change))
            msgs[what] = str(e.value)
            assert eng.multipath_cfg is None
            with pytest.raises(ValueError, match="without ofdm_set_multipath"):
                eng.multipath_reset(0)
        assert len(set(msgs.values())) == MESSAGES, sorted(set(msgs.values()))
        # one in force: it stays in force, mid-stream
        whole = _run(eng, "everything", x, sh.START).copy()
        eng.multipath_reset(sh.START)
        parts = [eng.multipath(x[:1501]).copy()]
        for what, change in BAD:
            with pytest.raises(ValueError) as e:
                eng.set_multipath(_bad_cfg(change))
            assert str(e.value) == msgs[what]
        parts.append(eng.multipath(x[1501:]))
        assert np.array_equal(sh.bits(np.concatenate(parts)), sh.bits(whole))
    finally:
        eng.set_multipath(None)


def test_entries_beyond_npaths_and_ntones_are_not_looked_at(eng):
    x = mc.stream(N, seed=12)
    try:
        want = _run(eng, "two_ray", x).copy()
        c = mc.cfg_of("two_ray")
        for p in range(2, 16):
            c.delay[p], c.doppler[p] = 5000, 7.0
            c.gain[p].re, c.gain[p].im = NAN, INF
        for j in range(4):
            c.tone_amp[j], c.tone_freq[j], c.tone_phase[j] = -1.0, NAN, INF
        eng.set_multipath(c)
        assert np.array_equal(sh.bits(eng.multipath(x)), sh.bits(want))
    finally:
        eng.set_multipath(None)


def _raw(eng, x_ptr, nin, out_ptr, cap, add_ptr=None):
    nn = C.c_uint64(0)
    rc = _abi.load().ofdm_multipath(eng._h, C.c_void_p(x_ptr), nin, None if add_ptr is None else C.c_void_p(add_ptr),
                                    C.c_void_p(out_ptr), cap, C.byref(nn))
    return rc, nn.value


def test_pointers_capacity_and_the_index_limit(eng):
    n = 3000
    x = mc.stream(n, seed=13)
    buf = np.zeros(2 * n + 8, np.complex64)
    buf[:n] = x
    out = np.zeros(n + 1, np.complex64)
    q = np.zeros((n + 1, 2), np.int16)
    xp, bp, op, qp = x.ctypes.data, buf.ctypes.data, out.ctypes.data, q.ctypes.data
    try:
        whole = _run(eng, "everything", x, 5).copy()
        eng.multipath_reset(5)
        # misaligned float buffers (in, add, out), then a misaligned 16-bit output
        for args in ((xp + 4, n - 1, op, n), (xp, n, op + 4, n), (xp, n, op, n, xp + 4)):
            assert _raw(eng, *args)[0] == _abi.OFDM_E_INVAL
        eng.set_multipath(mc.cfg_of("everything", out_format="sc16"))
        assert _raw(eng, xp, n, qp + 2, n)[0] == _abi.OFDM_E_INVAL
        assert _raw(eng, xp, n, qp + 4, n)[0] == _abi.OFDM_OK
        eng.set_multipath(mc.cfg_of("everything"))
        eng.multipath_reset(5)
        # input and output may not share a byte (next to each other they may lie: below)
        for i, o in ((bp, bp), (bp, bp + 8 * (n - 1)), (bp + 8 * n, bp + 8)):
            assert _raw(eng, i, n, o, n)[0] == _abi.OFDM_E_INVAL
            assert "overlaps" in eng._lib.ofdm_last_error(eng._h).decode()
        # capacity one short: *nout says what is needed, the stream has not moved, and the retried call continues
        assert _raw(eng, xp, 1000, op, 1000) == (_abi.OFDM_OK, 1000)
        first = out[:1000].copy()
        assert _raw(eng, xp + 8000, n - 1000, op, n - 1001) == (_abi.OFDM_E_CAPACITY, n - 1000)
        assert _raw(eng, bp + 8000, n - 1000, bp + 8 * n, n - 1000) == (_abi.OFDM_OK, n - 1000)      # adjacent buffers
        assert np.array_equal(sh.bits(np.concatenate([first, buf[n:2 * n - 1000]])), sh.bits(whole))
        # the stream index stays at or below 2^53
        eng.multipath_reset(TWO53)
        assert len(eng.multipath(x[:0])) == 0
        with pytest.raises(ValueError, match="2\\^53"):
            eng.multipath(x[:1])
        with pytest.raises(ValueError, match="2\\^53"):
            eng.multipath_reset(TWO53 + 1)
        assert len(eng.multipath(x[:0])) == 0                      # the refused reset left the stream where it was
        eng.multipath_reset(TWO53 - 10)
        with pytest.raises(ValueError, match="2\\^53"):
            eng.multipath(x[:11])
        y = eng.multipath(x[:10])
        mc.check(y, x[:10], mc.cfg_of("everything"), TWO53 - 10, "fc32", "the last ten indices below 2^53")
        with pytest.raises(ValueError, match="2\\^53"):
            eng.multipath(x[:1])
    finally:
        eng.set_multipath(None)


# ---- 6. device pointers ------------------------------------------------------------------------------------------------
def test_device_pointers_two_halves_and_add_aliasing_the_output(eng):
    torch = pytest.importorskip("torch")
    x, w = mc.stream(N, seed=14), mc.stream(N, seed=15)
    dev = engine.Engine(cfg=make_cfg(device_ptrs=True))
    d_x = torch.from_numpy(x).cuda()
    d_out = torch.zeros(N, dtype=torch.complex64, device="cuda")
    d_q = torch.zeros((N, 2), dtype=torch.int16, device="cuda")
    try:
        want = _run(eng, "everything", x, sh.START).copy()
        eng.multipath_reset(sh.START)
        want_add = eng.multipath(x, add=w).copy()
        want_q = _run(eng, "everything", x, sh.START, out_format="sc16").copy()
        dev.set_multipath(mc.cfg_of("everything"))
        dev.multipath_reset(sh.START)
        dev.prof_enable(True)
        with pytest.raises(ValueError):
            dev.multipath_last_ms()                                # no profiled call yet
        h = 1601
        assert dev.multipath_device(d_x.data_ptr(), h, d_out.data_ptr(), N) == h
        assert dev.multipath_last_ms() > 0.0
        assert dev.multipath_device(d_x.data_ptr() + 8 * h, N - h, d_out.data_ptr() + 8 * h, N - h) == N - h
        assert np.array_equal(sh.bits(d_out.cpu().numpy()), sh.bits(want))
        # `add` aliasing the output: each sample is read before it is written
        d_out.copy_(torch.from_numpy(w))
        torch.cuda.synchronize()
        dev.multipath_reset(sh.START)
        assert dev.multipath_device(d_x.data_ptr(), N, d_out.data_ptr(), N, add_ptr=d_out.data_ptr()) == N
        assert np.array_equal(sh.bits(d_out.cpu().numpy()), sh.bits(want_add))
        # the input overlapping the output is refused
        with pytest.raises(ValueError, match="overlaps"):
            dev.multipath_device(d_x.data_ptr(), N, d_x.data_ptr(), N)
        dev.set_multipath(mc.cfg_of("everything", out_format="sc16"))
        dev.multipath_reset(sh.START)
        assert dev.multipath_device(d_x.data_ptr(), N, d_q.data_ptr(), N) == N
        assert np.array_equal(d_q.cpu().numpy(), want_q)
    finally:
        eng.set_multipath(None)
        dev.close()
        sh.release(torch, d_x, d_out, d_q)


def test_a_handle_that_dropped_the_stage_receives_as_one_that_never_saw_it():
    cfg = make_cfg()
    pays = make_payloads(4, 100, seed=11)
    a, b = engine.Engine(cfg=cfg), engine.Engine(cfg=cfg)
    try:
        b.set_multipath(mc.cfg_of("everything"))
        b.prof_enable(True)
        assert len(b.multipath(mc.stream(3000))) == 3000 and b.multipath_last_ms() > 0.0
        b.set_multipath(None)
        with pytest.raises(ValueError):
            b.multipath_last_ms()
        for e in (a, b):
            e.set_channel(sigma=0.01, lead=1024, tail=1536)
            e.prof_enable(True)
            e.prof_reset()
        xa, xb = a.tx(pays), b.tx(pays)
        assert np.array_equal(xa, xb)
        pa, pb = a.rx(xa), b.rx(xb)
        assert pa == pb and [p for ok, p in pa if ok] == pays
        ca, cb = sh.launches(a), sh.launches(b)
        assert ca == cb and sum(ca.values()) > 0
        assert len(ca) == _abi.K_COUNT == 11 and not any("multipath" in k for k in ca)
        # with the stage configured and used, the kernel table still counts only what it counted
        b.set_multipath(mc.cfg_of("two_ray"))
        b.prof_reset()
        b.multipath(xb)
        assert np.array_equal(b.tx(pays), xa) and b.rx(xa) == pa
        assert sh.launches(b) == ca
    finally:
        a.close()
        b.close()


# ---- 7. a selective channel end to end -----------------------------------------------------------------------------------
def test_gain_follows_the_two_ray_profile_from_tx_to_rx_on_the_device():
    """The scenario of test_gpu_csi.test_gain_follows_a_two_path_channel with the channel on the device.  (The oracle's
    receiver decodes 12 of 12 packets of the float64 model's output with this seed: the file's docstring.)"""
    torch = pytest.importorskip("torch")
    Nf, occ, CP = 512, 200, 128
    cfg = make_cfg("qpsk", Nf, occ, CP, device_ptrs=True)
    pay = make_payloads(12, 800, seed=31)
    dev = engine.Engine(cfg=cfg)
    blob, offs, lens = engine.pack_payloads(pay)
    dev.set_channel(sigma=0.0, lead=2 * Nf, tail=3 * Nf)
    _, nsamp = dev.tx_frame_count(lens)
    d_pay = torch.from_numpy(blob.copy()).cuda()
    d_tx = torch.zeros(nsamp, dtype=torch.complex64, device="cuda")
    d_rx = torch.zeros(nsamp, dtype=torch.complex64, device="cuda")
    d_got = torch.zeros(16 * 1024, dtype=torch.uint8, device="cuda")
    try:
        assert dev.tx_device(d_pay.data_ptr(), offs, lens, d_tx.data_ptr(), nsamp) == nsamp
        psig = float(torch.mean(torch.abs(d_tx[2 * Nf:nsamp - 3 * Nf]).double() ** 2).item())
        mcfg = mc.cfg_of("two_ray", sigma=multipath.sigma_for_snr(30.0, psig), seed=7)
        dev.set_multipath(mcfg)
        assert dev.multipath_device(d_tx.data_ptr(), nsamp, d_rx.data_ptr(), nsamp) == nsamp
        dev.set_rx_csi(True)
        npk, off, ln, ok = dev.rx_device(d_rx.data_ptr(), nsamp, d_got.data_ptr(), d_got.numel(), 32)
        print("selective channel: %d packets, %d pass the CRC" % (npk, int(ok.sum())))
        assert int(ok.sum()) >= 10
        rep = csi.carrier_report(dev.rx_csi_summary(), cfg)
        k = (np.arange(occ) + config.zeros_on_left(Nf, occ) - Nf // 2) % Nf      # FFT bin of occupied carrier i
        H = 20 * np.log10(np.abs(multipath.frequency_response(mcfg, Nf)[k]))
        got = rep["gain_db"]
        assert np.isfinite(got).all()
        dev_db = (got - got.mean()) - (H - H.mean())
        print("selective channel: gain_db follows the profile within %.3f dB" % np.abs(dev_db).max())
        assert np.abs(dev_db).max() <= 1.0, np.abs(dev_db).max()
    finally:
        dev.close()
        sh.release(torch, d_pay, d_tx, d_rx, d_got)


# ---- 8. a primary user end to end ----------------------------------------------------------------------------------------
def test_the_sensor_finds_a_tone_of_the_stage_and_nothing_else(eng):
    """Noise (sigma 1e-4) and one tone of amplitude 0.01 at the centre of sensor bin 40 of 256.  (Margins of the oracle's
    sensor on the float64 model: 25.2 dB on the occupied side, 18.6 dB on the free side: the file's docstring.)"""
    S = 256
    sc = config.make_sense_cfg(S, 0, 1, 10, 1, threshold=1e-4)
    n = S * 11 + S
    try:
        eng.set_multipath(paths=[(0, 1.0)], tones=[(0.01, 40.0 / S)], sigma=1e-4)
        got = eng.sense(sc, eng.multipath(np.zeros(n, np.complex64)))
        assert len(got["bits"]) == 1
        bits, mean = got["bits"][0], got["mean"][0]
        dist = np.abs(np.arange(S) - (40 + S // 2) % S)          # the ascending-frequency map: bin k at (k + S/2) % S
        print("primary user: occupied side min %.3g, free side max %.3g (threshold 1e-4)" % (
            mean[dist <= 2].min(), mean[dist > 8].max()))
        assert (bits[dist <= 2] == 0).all() and (bits[dist > 8] == 1).all()
    finally:
        eng.set_multipath(None)


# ---- 9. the streaming object ---------------------------------------------------------------------------------------------
def test_channel_work_is_feed_in_chunks_plus_flush_and_a_stream_after_work_starts_afresh():
    x = mc.stream(N, seed=16)
    cfg = mc.cfg_of("everything", out_format="fc32")
    ch, fresh = multipath.channel(cfg), multipath.channel(cfg)
    try:
        whole = ch.work(x)
        assert whole.dtype == np.complex64 and len(whole) == N + 1023 == N + ch.dmax
        mc.check(whole, np.concatenate([x, np.zeros(1023, np.complex64)]), cfg, 0, "fc32", "channel.work")

        def chunks(c):
            return np.concatenate([c.feed(x[a:a + 700]) for a in range(0, N, 700)] + [c.flush()])
        assert np.array_equal(sh.bits(chunks(ch)), sh.bits(whole))            # a stream after work() starts afresh
        assert np.array_equal(sh.bits(chunks(fresh)), sh.bits(whole))
        assert np.array_equal(sh.bits(chunks(ch)), sh.bits(whole))            # ... and one after a flush
        ch.feed(x[:1234])
        assert np.array_equal(sh.bits(ch.work(x)), sh.bits(whole))            # ... and work() after an unfinished one
    finally:
        ch.close()
        fresh.close()


# ---- 10. the command line ------------------------------------------------------------------------------------------------
def test_channel_sim_sits_between_the_two_benchmark_programs(tmp_path):
    tx, rx1, rx2 = (str(tmp_path / f) for f in ("tx.dat", "rx1.dat", "rx2.dat"))
    npk = benchmark_ofdm_tx.main(["-m", "qpsk", "--to-file", tx, "-M", "9e-6"])
    assert npk == 4
    wide = iqio.read_complex_binary(tx)
    # silence around the packets: --snr measures the non-zero samples only
    sh.write_capture(tx, np.concatenate([np.zeros(4096, np.complex64), wide, np.zeros(8192, np.complex64)]))
    flags = ["--from-file", tx, "--paths", multipath.format_paths(mc.PROFILES["two_ray"].paths), "--snr", "30"]
    cfg = channel_sim.main(flags + ["--to-file", rx1])
    assert multipath.paths_of(cfg) == multipath.paths_of(mc.cfg_of("two_ray"))
    psig = float(np.mean(np.abs(wide[wide != 0].astype(np.complex128)) ** 2))
    assert cfg.sigma == pytest.approx(multipath.sigma_for_snr(30.0, psig), rel=1e-6)
    channel_sim.main(flags + ["--to-file", rx2, "--chunk-samples", "5000"])
    y1, y2 = iqio.read_complex_binary(rx1), iqio.read_complex_binary(rx2)
    assert len(y1) == 4096 + len(wide) + 8192 + 4 and np.array_equal(sh.bits(y1), sh.bits(y2))
    for f in (rx1, rx2):
        acct = benchmark_ofdm_rx.main(["-m", "qpsk", "--from-file", f, "--to-file", str(tmp_path / "rx.txt")])
        print("channel_sim: n_rcvd %d n_right %d" % (acct.n_rcvd, acct.n_right))
        assert acct.n_rcvd >= npk - 1 and acct.n_right >= acct.n_rcvd - 1
