"""The spectrum stage on the GPU (csrc/psd.h, ofdm_set_psd / ofdm_psd): every case of psd_cases against the float64 model
within the derived bound, bit for bit against the oracle-pinned sensor where the two compute the same thing, across any
chunking, in both input formats and both pointer modes, through the refusals, and end to end from ofdm_mod(spectrum=)
and the amplifier chain.

The figures of ofdm_mod.last_spectrum are compared with those the float64 model gives for the very samples flush()
returned, to 0.01 dB.  That tolerance follows from the bound: a band's power is a sum over segments and bins whose
errors are at most 2 |X| D + D^2 each; summed over a band whose density lies 40 dB below the channel's, with
D = 4 * 10 * 2^-24 ||e||_2 = 2.4e-6 ||e||_2 and |X| about 1e-2 ||e||_2 there, the relative error of the band's power is at
most 2 D / |X| = 5e-4, 0.002 dB, and the channel's own is a hundred times smaller."""
import ctypes as C

import numpy as np
import pytest

import psd_cases as pc
import stage_harness as sh
from helpers import make_cfg, make_payloads
from ofdm_uhd_amd import _abi, config, dpd, engine, iqio, ofdm, options, spectrum
from stage_harness import eng  # noqa: F401  (the module's engine)

pytestmark = pytest.mark.gpu


def _err(eng):
    return (eng._lib.ofdm_last_error(eng._h) or b"").decode()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- 1. every case against the model -----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pc.CASES, ids=pc.CASE_IDS)
def test_every_case_is_the_model_within_its_bound(eng, case):
    F, S, nseg = case
    n = pc.samples_for(nseg, F, S)
    raw, x = pc.stream(n, seed=F + S + nseg)
    w = pc.taps(F, seed=F + 1)
    eng.set_psd(spectrum.psd_cfg(F, S, w))
    try:
        assert eng.psd_count(n) == nseg
        rows = eng.psd(raw, rows=True)
        got = eng.psd_read()
        assert rows.shape == (nseg, F) and rows.dtype == np.float32 and got["nseg"] == nseg
        m = pc.welch64(x, F, S, w)
        assert m["nseg"] == nseg
        if nseg == 0:
            assert not got["sum"].any() and not got["peak"].any()
            return
        pc.check_spread(F, m["X"], m["norm"])
        b = pc.bound(F, m["X"], m["norm"])
        err = np.abs(rows.astype(np.float64) - m["rows"])
        print("F=%d S=%d nseg=%d: worst row error / bound = %.3g" % (F, S, nseg, float(np.max(err / b))))
        assert np.all(err <= b)
        # the sums: within the rows' bounds and the float64 rounding of nseg additions
        assert np.all(np.abs(got["sum"] - m["sum"]) <= b.sum(axis=0) + nseg * 2.0 ** -53 * m["sum"])
        # ... and they are the float64 sums of the GPU's own rows, the maxima their maxima bit for bit
        own = rows.astype(np.longdouble).sum(axis=0)          # (extended precision: the reference sum has no rounding to speak of)
        assert np.all(np.abs(got["sum"] - own) <= nseg * 2.0 ** -53 * own)
        assert np.array_equal(_bits(got["peak"]), _bits(rows.max(axis=0)))
    finally:
        eng.set_psd(None)


# ---- 2. the oracle-pinned sensor ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["fc32", "sc16"])
@pytest.mark.parametrize("F", [256, 2048])
def test_at_hop_F_the_rows_are_the_sensors_messages_bit_for_bit(eng, F, fmt):
    """tune_delay = 0, dwell_delay = 1: a message of k_sense is the max-hold over one vector, the vector's spectrum."""
    nseg = 37
    raw, _ = pc.stream(nseg * F + 5, seed=F, fmt=fmt)
    sc = config.make_sense_cfg(F, 0, 1, 1, 0)
    eng.set_rx_iq_format(fmt)
    try:
        msgs = eng.sense(sc, raw)["msgs"]
        eng.set_psd(spectrum.psd_cfg(F, F, "blackmanharris", in_format=fmt))
        rows = eng.psd(raw, rows=True)
        assert msgs.shape == rows.shape == (nseg, F) and rows.any()
        assert np.array_equal(_bits(rows), _bits(msgs))
    finally:
        eng.set_rx_iq_format("fc32")
        eng.set_psd(None)


# ---- 3. chunks -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("F,S", [(64, 1), (64, 19), (512, 512), (1024, 259), (4096, 2048)])
def test_a_stream_in_chunks_is_the_stream_in_one_call(eng, F, S, reverse):
    rng = np.random.default_rng(F + S)
    chunks = [0, 1, S - 1, F + 1, F - 1, S, 2 * F + 3, 1, 0, 5 * F + 1] + [int(v) for v in rng.integers(0, 3 * F, 6)]
    if reverse:
        chunks = chunks[::-1]
    raw, _ = pc.stream(sum(chunks), seed=7)
    eng.set_psd(spectrum.psd_cfg(F, S, pc.taps(F, seed=3)))
    try:
        whole = eng.psd(raw, rows=True).copy()
        want = eng.psd_read()
        assert want["nseg"] == len(whole) == spectrum.segments(len(raw), F, S) > 0
        eng.psd_reset()
        zero = eng.psd_read()
        assert zero["nseg"] == 0 and not zero["sum"].any() and not zero["peak"].any()
        parts, a = [], 0
        for n in chunks:
            assert eng.psd_count(n) == spectrum.segments(a + n, F, S) - spectrum.segments(a, F, S)
            parts.append(eng.psd(raw[a:a + n], rows=True))
            a += n
        assert any(len(p) == 0 for p in parts)
        assert np.array_equal(_bits(np.concatenate(parts)), _bits(whole))
        got = eng.psd_read()
        assert got["nseg"] == want["nseg"] and np.array_equal(_bits(got["peak"]), _bits(want["peak"]))
        assert np.all(np.abs(got["sum"] - want["sum"]) <= want["nseg"] * 2.0 ** -52 * want["sum"])   # two orders of the same terms
        # without rows the accumulators are the same
        eng.psd_reset()
        a = 0
        for i, n in enumerate(chunks):
            assert eng.psd(raw[a:a + n]) == len(parts[i])
            a += n
        again = eng.psd_read()
        assert again["nseg"] == got["nseg"] and np.array_equal(again["sum"], got["sum"]) and np.array_equal(again["peak"], got["peak"])
    finally:
        eng.set_psd(None)


def test_equal_call_sequences_give_bit_equal_sums(eng):
    F, S = 1024, 259
    raw, _ = pc.stream(pc.samples_for(2 * pc.max_grid(F) * pc.groups(F) + 1, F, S), seed=5)
    cuts = [0, 100000, 100001, 377777, len(raw)]
    eng.set_psd(spectrum.psd_cfg(F, S))
    try:
        reads = []
        for _ in range(2):
            eng.psd_reset()
            for a, b in zip(cuts[:-1], cuts[1:]):
                eng.psd(raw[a:b])
            reads.append(eng.psd_read())
        assert reads[0]["nseg"] == reads[1]["nseg"] == spectrum.segments(len(raw), F, S)
        assert np.array_equal(reads[0]["sum"].view(np.uint64), reads[1]["sum"].view(np.uint64))
        assert np.array_equal(_bits(reads[0]["peak"]), _bits(reads[1]["peak"]))
    finally:
        eng.set_psd(None)


# ---- 4. formats and pointer modes ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,S", [(64, 19), (512, 256), (2048, 515)])
def test_sc16_input_is_the_converted_samples_bit_for_bit(eng, F, S):
    q, x = pc.stream(9 * F + 7, seed=F, fmt="sc16")
    w = pc.taps(F, seed=2)
    try:
        eng.set_psd(spectrum.psd_cfg(F, S, w, in_format="sc16"))
        rq = eng.psd(q[:F + 3], rows=True), eng.psd(q[F + 3:], rows=True)     # (a cut: the history is converted samples)
        got = eng.psd_read()
        with pytest.raises(ValueError):
            eng.psd(x)
        eng.set_psd(spectrum.psd_cfg(F, S, w))
        rx = eng.psd(x, rows=True)
        want = eng.psd_read()
        with pytest.raises(ValueError):
            eng.psd(q)
        assert len(rx) > 0 and np.array_equal(_bits(np.concatenate(rq)), _bits(rx))
        assert np.array_equal(_bits(got["peak"]), _bits(want["peak"])) and got["nseg"] == want["nseg"]
        # another scale is the samples at that scale
        eng.set_psd(spectrum.psd_cfg(F, S, w, in_format="sc16", in_scale=1.0 / 1024))
        r2 = eng.psd(q, rows=True)
        eng.set_psd(spectrum.psd_cfg(F, S, w))
        assert np.array_equal(_bits(r2), _bits(eng.psd(iqio.from_sc16(q, 1.0 / 1024), rows=True)))
    finally:
        eng.set_psd(None)


@pytest.mark.parametrize("fmt", ["fc32", "sc16"])
def test_device_pointers_give_what_host_mode_gives(eng, fmt):
    torch = pytest.importorskip("torch")
    F, S = 1024, 259
    raw, _ = pc.stream(40 * F + 11, seed=9, fmt=fmt)
    cfg = spectrum.psd_cfg(F, S, pc.taps(F, seed=4), in_format=fmt)
    eng.set_psd(cfg)
    devE = engine.Engine(cfg=make_cfg(device_ptrs=True))
    x = rows = s = p = None
    try:
        want_rows = eng.psd(raw, rows=True)
        want = eng.psd_read()
        devE.set_psd(cfg)
        dev = torch.device("cuda", 0)
        x = torch.from_numpy(np.array(raw)).to(dev)
        nseg = len(want_rows)
        rows = torch.full((nseg + 2, F), -1.0, dtype=torch.float32, device=dev)
        half = len(raw) // 2 + 1
        ss = 4 if fmt == "sc16" else 8
        n1 = devE.psd_device(x.data_ptr(), half, rows.data_ptr(), nseg + 2)
        n2 = devE.psd_device(x.data_ptr() + ss * half, len(raw) - half, rows.data_ptr() + 4 * F * n1, nseg + 2 - n1)
        assert n1 + n2 == nseg and 0 < n1 < nseg
        s = torch.zeros(F, dtype=torch.float64, device=dev)
        p = torch.zeros(F, dtype=torch.float32, device=dev)
        assert devE.psd_read_device(s.data_ptr(), p.data_ptr()) == nseg
        torch.cuda.synchronize()
        out = rows.cpu().numpy()
        assert np.array_equal(_bits(out[:nseg]), _bits(want_rows)) and np.all(out[nseg:] == -1.0)
        assert np.array_equal(_bits(p.cpu().numpy()), _bits(want["peak"]))
        assert np.all(np.abs(s.cpu().numpy() - want["sum"]) <= nseg * 2.0 ** -52 * want["sum"])
        # without rows; rows that overlap the input are refused and move nothing
        more = spectrum.segments(len(raw) + F, F, S) - nseg
        assert devE.psd_device(x.data_ptr(), F) == more > 0
        n = C.c_uint64(0)
        rc = devE._lib.ofdm_psd(devE._h, C.c_void_p(x.data_ptr()), 3 * F, C.c_void_p(x.data_ptr() + 64), 100, C.byref(n))
        assert rc == _abi.OFDM_E_INVAL and "overlaps" in _err(devE)
        assert devE.psd_read_device() == nseg + more
    finally:
        eng.set_psd(None)
        keep = [t for t in (x, rows, s, p) if t is not None]
        sh.release(torch, *keep)
        devE.close()


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------
def test_a_short_rows_buffer_leaves_the_state_and_the_accumulators(eng):
    F, S = 512, 131
    raw, _ = pc.stream(30 * F, seed=1)
    eng.set_psd(spectrum.psd_cfg(F, S, pc.taps(F, seed=5)))
    try:
        whole = eng.psd(raw, rows=True).copy()
        want = eng.psd_read()
        eng.psd_reset()
        first = eng.psd(raw[:7 * F + 5], rows=True).copy()
        before = eng.psd_read()
        rest = np.ascontiguousarray(raw[7 * F + 5:])
        need = eng.psd_count(len(rest))
        assert need == len(whole) - len(first) > 1
        out = np.full((need, F), -3.0, np.float32)
        n = C.c_uint64(0)
        rc = eng._lib.ofdm_psd(eng._h, C.c_void_p(rest.ctypes.data), len(rest), C.c_void_p(out.ctypes.data), need - 1, C.byref(n))
        assert rc == _abi.OFDM_E_CAPACITY and n.value == need and "rows too small" in _err(eng)
        assert np.all(out == -3.0) and eng.psd_count(len(rest)) == need
        after = eng.psd_read()
        assert after["nseg"] == before["nseg"] and np.array_equal(after["sum"], before["sum"]) and np.array_equal(after["peak"], before["peak"])
        # the retried call continues the stream bit for bit; a NULL rows ignores rows_cap
        assert np.array_equal(_bits(np.concatenate([first, eng.psd(rest, rows=True)])), _bits(whole))
        got = eng.psd_read()
        assert got["nseg"] == want["nseg"] and np.array_equal(_bits(got["peak"]), _bits(want["peak"]))
        rc = eng._lib.ofdm_psd(eng._h, C.c_void_p(rest.ctypes.data), len(rest), None, 0, C.byref(n))
        assert rc == _abi.OFDM_OK and n.value == eng.psd_read()["nseg"] - got["nseg"] > 0
    finally:
        eng.set_psd(None)


def test_every_refusal_has_its_message_and_leaves_the_configuration_in_force(eng):
    F, S = 256, 67
    raw, _ = pc.stream(20 * F, seed=8)
    w = pc.taps(F, seed=6)
    good = spectrum.psd_cfg(F, S, w)
    eng.set_psd(good)
    try:
        whole = eng.psd(raw, rows=True).copy()
        want = eng.psd_read()
        eng.psd_reset()
        half = 9 * F + 1
        first = eng.psd(raw[:half], rows=True).copy()

        def changed(**kw):
            cfg = spectrum.psd_cfg(F, S, w)
            for k, v in kw.items():
                if k == "tap":
                    cfg.taps[v[0]] = v[1]
                elif k == "zero":
                    for i in range(F):
                        cfg.taps[i] = 0.0
                else:
                    setattr(cfg, k, v)
            return cfg
        nan, inf = float("nan"), float("inf")
        bad = [(changed(struct_size=good.struct_size - 4), "struct_size"), (changed(nfft=32), "nfft"), (changed(nfft=8192), "nfft"),
               (changed(nfft=384), "nfft"), (changed(nfft=0), "nfft"), (changed(hop=0), "hop"), (changed(hop=F + 1), "hop"),
               (changed(tap=(3, nan)), "finite"), (changed(tap=(F - 1, inf)), "finite"), (changed(zero=True), "all be zero"),
               (changed(in_format=2), "in_format"), (changed(in_format=_abi.OFDM_IQ_SC16, in_scale=-1.0), "in_scale"),
               (changed(in_format=_abi.OFDM_IQ_SC16, in_scale=inf), "in_scale"), (changed(in_format=_abi.OFDM_IQ_SC16, in_scale=nan), "in_scale")]
        for cfg, word in bad:
            rc = eng._lib.ofdm_set_psd(eng._h, C.byref(cfg))
            assert rc == _abi.OFDM_E_INVAL and word in _err(eng), (word, _err(eng))
            with pytest.raises(ValueError):
                eng.set_psd(cfg)
            assert eng.psd_cfg is good
        eng.set_psd(changed(tap=(F, nan)))      # an entry beyond nfft is not looked at ...
        eng.set_psd(good)                       # (... but a configuration that is accepted starts the stage afresh)
        first = eng.psd(raw[:half], rows=True).copy()
        for cfg, _ in bad[:4]:
            with pytest.raises(ValueError):
                eng.set_psd(cfg)
        # refused calls: misaligned pointers, and they move nothing
        buf = np.zeros(4 * F + 2, np.complex64)
        out = np.zeros((8, F), np.float32)
        sums = np.zeros(F + 1, np.float64)
        n = C.c_uint64(0)
        rc = eng._lib.ofdm_psd(eng._h, C.c_void_p(buf.ctypes.data + 4), 2 * F, C.c_void_p(out.ctypes.data), 8, C.byref(n))
        assert rc == _abi.OFDM_E_INVAL and "8-byte aligned" in _err(eng)
        rc = eng._lib.ofdm_psd(eng._h, C.c_void_p(buf.ctypes.data), 2 * F, C.c_void_p(out.ctypes.data + 2), 8, C.byref(n))
        assert rc == _abi.OFDM_E_INVAL and "4-byte aligned" in _err(eng)
        rc = eng._lib.ofdm_psd_read(eng._h, C.c_void_p(sums.ctypes.data + 4), None, C.byref(n))
        assert rc == _abi.OFDM_E_INVAL and "8-byte aligned" in _err(eng)
        rc = eng._lib.ofdm_psd(eng._h, None, 5, None, 0, C.byref(n))
        assert rc == _abi.OFDM_E_INVAL and "null iq_in" in _err(eng)
        rc = eng._lib.ofdm_psd(eng._h, C.c_void_p(buf.ctypes.data), 1 << 63, None, 0, C.byref(n))
        assert rc == _abi.OFDM_E_INVAL and "split it" in _err(eng)
        rc = eng._lib.ofdm_psd_count(eng._h, (1 << 31) * S + F, C.byref(n))
        assert rc == _abi.OFDM_E_INVAL and "split it" in _err(eng) and n.value > (1 << 31) - 1
        assert eng._lib.ofdm_psd_read(eng._h, None, None, C.byref(n)) == _abi.OFDM_OK and n.value == len(first)
        # the stream continues as if none of these calls had been made
        assert np.array_equal(_bits(np.concatenate([first, eng.psd(raw[half:], rows=True)])), _bits(whole))
        got = eng.psd_read()
        assert got["nseg"] == want["nseg"] and np.array_equal(_bits(got["peak"]), _bits(want["peak"]))
        # a misaligned 16-bit pointer
        eng.set_psd(spectrum.psd_cfg(F, S, w, in_format="sc16"))
        q = np.zeros(2 * F + 2, np.int16)
        rc = eng._lib.ofdm_psd(eng._h, C.c_void_p(q.ctypes.data + 2), F, None, 0, C.byref(n))
        assert rc == _abi.OFDM_E_INVAL and "ofdm_sc16" in _err(eng) and eng.psd_count(F) == 1
    finally:
        eng.set_psd(None)


def test_calls_without_a_configuration_are_refused(eng):
    eng.set_psd(None)
    assert eng.psd_cfg is None
    n = C.c_uint64(0)
    x = np.zeros(128, np.complex64)
    rc = eng._lib.ofdm_psd(eng._h, C.c_void_p(x.ctypes.data), 128, None, 0, C.byref(n))
    assert rc == _abi.OFDM_E_INVAL and "without ofdm_set_psd" in _err(eng)
    for fn, args in ((eng._lib.ofdm_psd_reset, ()), (eng._lib.ofdm_psd_count, (128, C.byref(n))),
                     (eng._lib.ofdm_psd_read, (None, None, C.byref(n)))):
        assert fn(eng._h, *args) == _abi.OFDM_E_INVAL and "without ofdm_set_psd" in _err(eng)
    for call in (lambda: eng.psd(x), eng.psd_reset, eng.psd_read, eng.psd_last_ms, lambda: eng.psd_count(5)):
        with pytest.raises(ValueError):
            call()
    # ... and after a configuration was dropped
    eng.set_psd(nfft=64)
    assert eng.psd(x) == 3
    eng.set_psd(None)
    with pytest.raises(ValueError):
        eng.psd(x)


def test_a_handle_that_never_set_the_stage_launches_what_it_launched_before():
    """Two handles transmit and receive the same packets: one never saw the stage, the other measured another stream
    and dropped it.  Same samples, same packets, same per-kernel launch counts; the kernel table has no entry for the
    stage, which reports its own time."""
    cfg = make_cfg()
    a, b = engine.Engine(cfg=cfg), engine.Engine(cfg=cfg)
    try:
        raw, _ = pc.stream(5000, seed=2)
        b.set_psd(nfft=256, hop=64)
        b.psd(raw)
        b.set_psd(None)
        for e in (a, b):
            e.prof_enable(True)
            e.prof_reset()
        pay = make_payloads(4, 300, seed=1)
        ia, ib = a.tx(pay), b.tx(pay)
        assert np.array_equal(ia, ib)
        pad = np.zeros(2048, np.complex64)
        assert a.rx(np.concatenate([pad, ia, pad])) == b.rx(np.concatenate([pad, ib, pad]))
        ca, cb = sh.launches(a), sh.launches(b)
        assert ca == cb and sum(ca.values()) > 0 and len(ca) == _abi.K_COUNT == 11 and not any("psd" in k for k in ca)
        b.set_psd(nfft=256, hop=64)
        b.prof_reset()
        with pytest.raises(ValueError):
            b.psd_last_ms()                      # no profiled call yet
        assert b.psd(raw[:100]) == 0
        with pytest.raises(ValueError):
            b.psd_last_ms()                      # a call that completed no segment has no kernel time
        assert b.psd(raw) > 0 and b.psd_last_ms() > 0.0
        assert sum(sh.launches(b).values()) == 0
    finally:
        a.close()
        b.close()


# ---- 6. end to end -------------------------------------------------------------------------------------------------------
def _options():
    return options.default_options(modulation="qpsk", fft_length=512, occupied_tones=200, cp_length=128)


def _figures(samples, fmt, F, S, center, bw, spacing, mask):
    x = iqio.from_sc16(samples) if fmt == "sc16" else samples
    w = pc.taps(F)
    m = pc.welch64(x, F, S, w)
    return spectrum.report({"sum": m["sum"], "peak": m["peak"], "nseg": m["nseg"]}, w, center, bw, spacing, mask)


@pytest.mark.parametrize("fmt", ["fc32", "sc16"])
def test_ofdm_mod_reports_the_spectrum_of_what_it_hands_out(fmt):
    opt = _options()
    sent = make_payloads(6, 400, seed=3)
    front = dict(interpolation=4, center_freq=0.125)
    coef = dpd.identity(3, 3)
    coef[0, 1] = 0.05 - 0.02j                   # (a mild expansion: the table's content is not the point here)
    mask = [(0.06, 0.2, -30.0), (-0.2, -0.06, -30.0)]
    kw = dict(pad_for_usrp=False, iq_format=fmt, duc=front, cfr=dict(papr_db=7.0, half_width=16), dpd=dict(coef=coef))
    tx = ofdm.ofdm_mod(opt, spectrum=dict(nfft=1024, hop=512, window="blackmanharris", spacing=0.25, mask=mask), **kw)
    plain = ofdm.ofdm_mod(opt, **kw)
    try:
        assert tx.last_spectrum is None and plain.last_spectrum is None and tx.flush(end=True) is None
        for m in (tx, plain):
            m.engine().set_tx_amplitude(0.1)
            m.set_cfr_amplitude(0.1)
            for p in sent[:3]:
                m.send_pkt(p)
        parts, ref = [tx.flush()], [plain.flush()]
        running = tx.last_spectrum
        assert running is not None and running["nseg"] == spectrum.segments(len(parts[0]), 1024, 512)
        for m in (tx, plain):
            for p in sent[3:]:
                m.send_pkt(p)
        parts.append(tx.flush(end=True))
        ref.append(plain.flush(end=True))
        iq, want = np.concatenate(parts), np.concatenate(ref)
        # without spectrum= the returned samples are bit-equal
        assert iq.dtype == want.dtype and np.array_equal(iq, want)
        r = tx.last_spectrum
        assert r["center"] == 0.125 and r["bandwidth"] == pytest.approx(200 / 512.0 / 4) and r["nfft"] == 1024
        f = _figures(iq, fmt, 1024, 512, 0.125, 200 / 512.0 / 4, 0.25, mask)
        print("ofdm_mod %s: nseg %d, obw %.5f, ACLR %.2f / %.2f dB, mask margin %.2f dB" % (
            fmt, r["nseg"], r["obw"], r["aclr_db"][0], r["aclr_db"][1], r["mask_margin_db"]))
        assert r["nseg"] == f["nseg"] == spectrum.segments(len(iq), 1024, 512) > 20
        for side in (0, 1):
            assert r["aclr_db"][side] > 25.0 and abs(r["aclr_db"][side] - f["aclr_db"][side]) < 0.01
        assert abs(r["mask_margin_db"] - f["mask_margin_db"]) < 0.01 and r["mask_at"]["segment"] == f["mask_at"]["segment"]
        assert abs(10 * np.log10(r["channel_power"] / f["channel_power"])) < 0.01
        assert r["obw"] == pytest.approx(f["obw"], abs=1e-5) and 0.08 < r["obw"] < 0.2
        assert np.allclose(r["density"], f["density"], rtol=1e-3, atol=1e-6 * float(np.max(f["density"])))
        # a second stream starts afresh: the same samples, the same figures
        for p in sent[:3]:
            tx.send_pkt(p)
        again = [tx.flush()]
        for p in sent[3:]:
            tx.send_pkt(p)
        again.append(tx.flush(end=True))
        assert np.array_equal(np.concatenate(again), iq)
        r2 = tx.last_spectrum
        assert r2["nseg"] == r["nseg"] and r2["aclr_db"] == pytest.approx(r["aclr_db"], abs=1e-6)
    finally:
        tx.engine().close()
        plain.engine().close()


def test_the_modulator_alone_and_the_command_lines(tmp_path):
    """spectrum= without a wideband stage: the channel fills the band, there is no adjacent channel and no ACLR.  The
    same through transmit_path's options, benchmark_ofdm_tx --psd and python -m ofdm_uhd_amd.spectrum on the file."""
    from ofdm_uhd_amd import benchmark_ofdm_tx, transmit_path
    opt = _options()
    tx = ofdm.ofdm_mod(opt, pad_for_usrp=False, spectrum=dict(nfft=256))
    try:
        for p in make_payloads(3, 200, seed=1):
            tx.send_pkt(p)
        iq = tx.flush(end=True)
        r = tx.last_spectrum
        assert r["nseg"] == spectrum.segments(len(iq), 256, 128) and "aclr_db" not in r
        assert r["bandwidth"] == pytest.approx(200 / 512.0) and 0.3 < r["obw"] < 0.5
        with pytest.raises(ValueError):
            ofdm.ofdm_mod(opt, spectrum=dict(nfft=100))
        with pytest.raises(ValueError):
            ofdm.ofdm_mod(opt, spectrum=dict(nfft=256, overlap=3))
    finally:
        tx.engine().close()
    o = _options()
    o.psd, o.psd_spacing, o.duc_interp, o.duc_freq = "512,128", 0.25, 4, -0.125
    tp = transmit_path.transmit_path(o)
    try:
        assert tp.ofdm_tx.engine().psd_cfg.nfft == 512 and tp.ofdm_tx.engine().psd_cfg.hop == 128
        tp.send_pkt(b"x" * 300)
        tp.send_pkt(eof=True)
        assert tp.ofdm_tx.last_spectrum["center"] == -0.125 and len(tp.ofdm_tx.last_spectrum["aclr_db"]) == 2
    finally:
        tp.ofdm_tx.engine().close()
    f, d = str(tmp_path / "tx.dat"), str(tmp_path / "psd.npy")
    assert benchmark_ofdm_tx.main(["-m", "qpsk", "-M", "0.02", "--to-file", f, "--duc-interp", "4", "--duc-freq", "0.125",
                                   "--psd", "1024", "--psd-out", d]) > 0
    den = np.load(d)
    assert den.shape == (1024,) and abs(int(np.argmax(den)) - (512 + 128)) < 60       # ascending frequency: 0.125 is bin 640
    r = spectrum.main(["--from-file", f, "--nfft", "1024", "--channel", "0.125,%r" % (200 / 512.0 / 4), "--spacing", "0.25",
                       "--chunk-samples", "50001"])
    assert np.allclose(spectrum.ascending(r["density"]), den, rtol=1e-9, atol=0.0) and r["aclr_db"][0] > 25.0
    for bad in (["--psd", "100"], ["--psd", "1024,0"], ["--psd", "a"], ["--psd-spacing", "0.2"]):
        with pytest.raises(SystemExit):
            benchmark_ofdm_tx.main(["-m", "qpsk", "-M", "0.02", "--to-file", f] + bad)


def test_the_amplifier_chain_on_the_gpu(eng):
    """e.dpd, e.pa, dpd.train, then e.psd: the ordering of test_psd_host.py's float64 chain, and the GPU's ACLR within
    0.01 dB of the float64 model's on the GPU's own streams."""
    x = pc.pa_probe()
    pa = dpd.example_pa()
    eng.set_psd(spectrum.psd_cfg(pc.PA_NFFT, pc.PA_HOP))
    eng.set_pa(dpd.mempoly_cfg(pa))
    try:
        def aclr(stream):
            eng.psd_reset()
            assert eng.psd(stream) == pc.PA_SEGMENTS
            got = spectrum.report(eng.psd_read(), eng.psd_cfg, 0.0, pc.PA_BW, pc.PA_SPACING)["aclr_db"]
            want = pc.aclr_of(stream)
            assert abs(got[0] - want[0]) < 0.01 and abs(got[1] - want[1]) < 0.01
            return got
        a_in = aclr(x)
        eng.pa_reset()
        a_pa = aclr(eng.pa(x))
        coef, nmse = dpd.train(eng, x, memory=3, orders=3, iterations=2)
        eng.dpd_reset()
        eng.pa_reset()
        a_dpd = aclr(eng.pa(eng.dpd(x)))
        print("GPU ACLR lower / upper: input %.2f / %.2f, amplifier %.2f / %.2f, predistorted %.2f / %.2f dB; NMSE %.1f dB" % (
            a_in + a_pa + a_dpd + (nmse[-1],)))
        for side in (0, 1):
            assert a_pa[side] < a_in[side] - 1.0 and a_dpd[side] > a_pa[side] + 1.0
    finally:
        eng.set_psd(None)
        eng.set_pa(None)
        eng.set_dpd(None)
