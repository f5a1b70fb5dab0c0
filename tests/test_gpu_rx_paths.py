"""ofdm_rx's two count paths, its capacity errors and its profiler spans.

The default path keeps frame and packet counts on the device (two host round trips); OFDM_RX_SYNCS=1 reads them back
as it goes (four).  Both must hand the caller exactly the same thing; a call whose buffers are too small must say so
without touching a byte behind the capacities it was given and without leaving anything behind on the handle; and
every exit must close the profiler spans it opened (the launch counts below are decided by the code, not measured)."""
import ctypes as C

import numpy as np
import pytest

from helpers import loopback_stream, make_cfg, make_payloads
from ofdm_uhd_amd import _abi, config, engine, options

pytestmark = pytest.mark.gpu

GUARD = 256          # elements behind every declared capacity
FILL = 0xA5          # the byte they are filled with


def _c2(orc, dev):
    cfg = make_cfg("qpsk", device_ptrs=dev)
    return cfg, loopback_stream(orc, cfg, make_payloads(24, 1026, seed=5), snr_db=30.0, cfo_bins=0.05)


def _chained(orc, dev):      # the cfo = 0.3 row of test_gpu_parity.CASES: first packet lost, chained frames
    cfg = make_cfg("qpsk", 512, 200, 128, device_ptrs=dev)
    return cfg, loopback_stream(orc, cfg, make_payloads(6, 1026), snr_db=30.0, cfo_bins=0.3)


def _long_symbols(orc, dev):
    cfg = make_cfg("qam16", 2048, 1200, 512, device_ptrs=dev)
    return cfg, loopback_stream(orc, cfg, make_payloads(3, 4091), snr_db=30.0)


def _noise(orc, dev):
    x = np.zeros(40000, np.complex64)
    orc.channel(x, sigma=0.05, seed=11)
    return make_cfg("qpsk", device_ptrs=dev), x


def _empty(orc, dev):
    return make_cfg("qpsk", device_ptrs=dev), np.zeros(0, np.complex64)


STREAMS = {"c2": _c2, "chained": _chained, "n2048": _long_symbols, "noise": _noise, "empty": _empty}


def _guarded(n, dtype):
    a = np.empty(n + GUARD, dtype)
    a.view(np.uint8)[:] = FILL
    return a


def _intact(a, n):
    return bool((a[n:].view(np.uint8) == FILL).all())


def _engine(cfg, instr):
    eng = engine.Engine(cfg=cfg)
    if instr:
        eng.set_rx_quality(True)
        eng.set_rx_csi(True)
    return eng


def _rx(eng, x, max_pkts, payload_cap, instr=False):
    """ofdm_rx through ctypes with a guard region behind every caller buffer.  Returns everything the call and the
    accessors behind it hand out, as plain Python values that compare with ==."""
    n = len(x)
    off, ln, ok = _guarded(max_pkts + 1, np.uint64), _guarded(max_pkts, np.uint32), _guarded(max_pkts, np.uint8)
    npk, st = C.c_int(-1), _abi.ofdm_stats()
    if eng.device_ptrs:
        import torch
        xd = torch.from_numpy(x.view(np.float32).copy()).cuda()
        payd = torch.full((payload_cap + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        iq_p, pay_p = C.c_void_p(xd.data_ptr() if n else None), C.c_void_p(payd.data_ptr())
    else:
        pay = _guarded(payload_cap, np.uint8)
        iq_p, pay_p = (x.ctypes.data_as(C.c_void_p) if n else None), pay.ctypes.data_as(C.c_void_p)
    rc = eng._lib.ofdm_rx(eng._h, iq_p, n, pay_p, payload_cap, off.ctypes.data_as(C.POINTER(C.c_uint64)),
                          ln.ctypes.data_as(C.POINTER(C.c_uint32)), ok.ctypes.data_as(C.POINTER(C.c_uint8)), max_pkts,
                          C.byref(npk), C.byref(st))
    if eng.device_ptrs:
        torch.cuda.synchronize()
        pay = payd.cpu().numpy()
    assert _intact(off, max_pkts + 1), "payload_off written behind max_pkts + 1 entries"
    assert _intact(ln, max_pkts), "payload_len written behind max_pkts entries"
    assert _intact(ok, max_pkts), "crc_ok written behind max_pkts entries"
    assert _intact(pay, payload_cap), "payload written behind payload_cap"
    out = {"rc": rc, "npkt": npk.value, "stats": st.as_dict(),
           "err": (eng._lib.ofdm_last_error(eng._h) or b"").decode() if rc != _abi.OFDM_OK else ""}
    if rc != _abi.OFDM_OK:
        return out
    k = npk.value
    out["off"] = off[:k + 1].tolist()
    out["len"] = ln[:k].tolist()
    out["ok"] = ok[:k].tolist()
    out["payload"] = pay[:int(off[k]) if k else 0].tobytes()
    out["pos"] = eng.rx_packet_pos().tolist()
    out["nco"] = [a.tobytes() for a in eng.rx_nco_state()]
    if instr:
        q = eng.rx_quality()
        out["quality"] = {f: q[f].tobytes() for f in q.dtype.names}      # (field by field: no padding bytes)
        csi = eng.rx_csi()
        out["csi"] = {key: (v.shape, v.tobytes()) for key, v in csi.items()}
    return out


def _room(cfg, x):
    max_pkts = len(x) // (cfg.fft_length + cfg.cp_length) + 16
    return max_pkts, max_pkts * 64 + len(x)


def _fresh(cfg, x, instr=False):
    eng = _engine(cfg, instr)
    r = _rx(eng, x, *_room(cfg, x), instr=instr)
    eng.close()
    return r


# ---- a. the default path against OFDM_RX_SYNCS=1 ------------------------------------------------------------------
@pytest.mark.parametrize("instr", [False, True], ids=["plain", "quality+csi"])
@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("stream", sorted(STREAMS))
def test_default_path_matches_rx_syncs(orc, monkeypatch, stream, dev, instr):
    cfg, x = STREAMS[stream](orc, dev)
    monkeypatch.delenv("OFDM_RX_SYNCS", raising=False)
    a = _fresh(cfg, x, instr)
    monkeypatch.setenv("OFDM_RX_SYNCS", "1")
    b = _fresh(cfg, x, instr)
    assert a["rc"] == _abi.OFDM_OK
    for key in sorted(set(a) | set(b)):
        assert a[key] == b[key], key
    # the inputs are what their names say
    st = a["stats"]
    assert st["samples"] == len(x) and st["overflow"] == 0 and st["packets"] == a["npkt"] == len(a["pos"])
    if stream == "c2":
        assert a["npkt"] == 24 and st["crc_ok"] == 24
    elif stream == "chained":
        assert st["chained_frames"] >= 1 and st["frames"] > st["packets"] >= 1
        assert any(np.frombuffer(a["nco"][3], np.uint8))          # a swallowed flag
    elif stream == "n2048":
        assert a["npkt"] == 3 and st["crc_ok"] == 3
    else:
        assert st["peaks"] == 0 and a["npkt"] == 0 and a["off"] == [0] and a["payload"] == b""


# ---- b. capacity errors ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("syncs", [False, True], ids=["default", "rx_syncs"])
@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
def test_capacity_errors(orc, monkeypatch, dev, syncs):
    if syncs:
        monkeypatch.setenv("OFDM_RX_SYNCS", "1")
    else:
        monkeypatch.delenv("OFDM_RX_SYNCS", raising=False)
    cfg, x = _c2(orc, dev)
    want = _fresh(cfg, x)
    npk, nbytes = want["npkt"], len(want["payload"])
    assert want["rc"] == _abi.OFDM_OK and npk == 24 and nbytes == 24 * 1026
    room_pkts, room_bytes = _room(cfg, x)
    eng = _engine(cfg, False)
    for max_pkts, cap in ((npk - 1, room_bytes), (room_pkts, nbytes - 1), (npk - 1, nbytes - 1)):
        r = _rx(eng, x, max_pkts, cap)               # (the guards behind max_pkts / cap are checked in there)
        assert r["rc"] == _abi.OFDM_E_CAPACITY, (max_pkts, cap)
        assert r["npkt"] == npk
        assert r["err"]
    assert _rx(eng, x, npk, nbytes) == want          # exactly enough room, on the handle that has just failed
    assert _rx(eng, x, room_pkts, room_bytes) == want
    eng.close()


# ---- c. every exit closes its spans ------------------------------------------------------------------------------------
KERNELS = ("k_frame_pack", "k_tx_mod", "k_channel", "k_sync", "k_peak", "k_rx_demod", "k_deframe", "k_sense",
           "k_chan_filter", "k_sync_exact", "k_front")


def _launches(**kw):
    return {k: kw.get(k, 0) for k in KERNELS}


FRONT = dict(k_chan_filter=1, k_sync=1, k_sync_exact=1, k_peak=1)
SPANS = {
    "normal": _launches(k_rx_demod=1, k_deframe=1, **FRONT),
    "no_flag": _launches(**FRONT),
    "capacity": _launches(k_rx_demod=1, k_deframe=1, **FRONT),
    "fixed": _launches(k_peak=1, k_rx_demod=1, k_deframe=1),
    "sense": _launches(k_rx_demod=1, k_deframe=1, k_sense=1, **FRONT),
}


@pytest.mark.parametrize("case", sorted(SPANS))
def test_spans_close(orc, monkeypatch, case):
    monkeypatch.delenv("OFDM_RX_SYNCS", raising=False)
    cfg, x = (_noise if case == "no_flag" else _c2)(orc, False)
    max_pkts, cap = _room(cfg, x)
    want_rc = _abi.OFDM_OK
    if case == "capacity":
        max_pkts, want_rc = 23, _abi.OFDM_E_CAPACITY
    if case == "fixed":
        N, CP = 512, 128
        pay = make_payloads(6, 500, seed=21)
        nsym = len(orc.tx(cfg, pay[:1])) // (N + CP)
        cfg = config.make_cfg(options.default_options(modulation="qpsk", fft_length=N, occupied_tones=200, cp_length=CP,
                                                      sync="fixed", sync_nsymbols=nsym, sync_freq_offset=0.0))
        x = loopback_stream(orc, cfg, pay, snr_db=30.0, lead=0, tail=700)
    eng = _engine(cfg, False)
    if case == "sense":
        eng.set_rx_sense(config.make_sense_cfg(256, 1, 6, 3, 1, threshold=0.05))
    eng.prof_enable(True)
    for _ in range(2):                               # the second call starts from whatever the first one left
        eng.prof_reset()
        r = _rx(eng, x, max_pkts, cap)
        assert r["rc"] == want_rc
        got = {k: v[1] for k, v in eng.prof().items()}
        assert got == SPANS[case]
    if case == "fixed":
        assert r["npkt"] == 6
    eng.close()


def test_overflow_retry_reports_no_overflow():
    """A carrier long enough that the first attempt's sparse candidate storage (1/16 of the samples plus a fixed slack
    of about 17 M) overflows: k_sync_exact and the detector run a second time with room for every sample, find no flag,
    and the call returns as for any input without a frame -- stats.overflow is 0, both attempts' spans are closed."""
    cfg = make_cfg("qpsk")
    x = np.ones(24 << 20, np.complex64)
    eng = _engine(cfg, False)
    eng.prof_enable(True)
    eng.prof_reset()
    r = _rx(eng, x, 64, 1 << 16)
    assert r["rc"] == _abi.OFDM_OK and r["npkt"] == 0
    assert r["stats"]["samples"] == len(x) and r["stats"]["peaks"] == 0 and r["stats"]["overflow"] == 0, r["stats"]
    got = {k: v[1] for k, v in eng.prof().items()}
    assert got == _launches(k_chan_filter=1, k_sync=1, k_sync_exact=2, k_peak=2), got      # (2: the retry ran)
    eng.close()
