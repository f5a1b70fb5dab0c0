"""Per-subcarrier channel state (ofdm_set_rx_csi / ofdm_rx_csi / ofdm_rx_csi_summary) on the host side: the entry points,
the inverse of the carrier-map rule, the per-carrier report and the map it suggests, and an oracle loopback on such a
map.  No GPU needed."""
import ctypes

import numpy as np
import pytest

from helpers import loopback_stream, make_cfg, make_payloads
from ofdm_uhd_amd import _abi, config, csi

SIZES = [(48, 64), (64, 128), (100, 128), (120, 256), (180, 256), (196, 256), (200, 512), (204, 512), (600, 1024),
         (1200, 2048), (2400, 4096)]


def test_csi_entry_points_exported():
    lib = _abi.load()
    for name in ("ofdm_set_rx_csi", "ofdm_rx_csi", "ofdm_rx_csi_summary"):
        assert name in _abi.EXPORTS
        assert hasattr(lib, name), name
    assert lib.ofdm_abi_version() == _abi.OFDM_ABI_VERSION == 6


def test_csi_calls_refuse_a_null_handle():
    lib = _abi.load()
    n = ctypes.c_int(-1)
    npk = ctypes.c_uint32(7)
    assert lib.ofdm_set_rx_csi(None, 1) == _abi.OFDM_E_INVAL
    assert lib.ofdm_rx_csi(None, 0, 0, None, None, None, None, ctypes.byref(n)) == _abi.OFDM_E_INVAL
    assert lib.ofdm_rx_csi_summary(None, 1, ctypes.byref(npk), None, None, None, None, None) == _abi.OFDM_E_INVAL


def _both_rules(occ, N, hx, want):
    zl = config.zeros_on_left(N, occ)
    assert hx == hx.upper()
    assert config.carrier_map(occ, occ, hx, sink=True) == sorted(want)
    assert config.carrier_map(occ, N, hx, sink=False) == [c + zl for c in sorted(want)]


@pytest.mark.parametrize("occ,N", SIZES)
def test_carrier_map_hex_round_trip(occ, N):
    # the default map's carriers come back as a string that selects the same carriers
    d = config.carrier_map(occ, occ, "FE7F", sink=True)
    _both_rules(occ, N, config.carrier_map_hex(occ, N, d), d)
    rng = np.random.default_rng(occ)
    nok = 0
    for trial in range(40):
        want = set(np.flatnonzero(rng.random(occ) < rng.uniform(0.3, 0.95)).tolist()) or {occ // 2}
        # a set that excludes a carrier the growth rule forces on raises and names it; adding the named carriers
        # back ends in a set that maps
        for _ in range(occ):
            try:
                hx = config.carrier_map_hex(occ, N, sorted(want))
            except ValueError as e:
                c = int(str(e).split("forces carrier ")[1].split()[0])
                assert 0 <= c < occ and c not in want
                want.add(c)
                continue
            _both_rules(occ, N, hx, want)
            nok += 1
            break
        else:
            raise AssertionError("no map for %r" % sorted(want))
    assert nok == 40


def test_carrier_map_hex_grown_form():
    # N = 512 / occ = 204: a full-length 51-digit string would put the mapper's block at bin 152 and the sink's at 154;
    # the grown form with partial nibbles agrees, and its edge carriers are forced on
    hx = config.carrier_map_hex(204, 512, range(204))
    assert len(hx) == 50
    _both_rules(204, 512, hx, range(204))
    with pytest.raises(ValueError, match="forces carrier 0 "):
        config.carrier_map_hex(204, 512, range(1, 204))
    with pytest.raises(ValueError, match="forces carrier 202 "):
        config.carrier_map_hex(204, 512, [c for c in range(204) if c != 202])
    with pytest.raises(ValueError):
        config.carrier_map_hex(200, 512, [])
    with pytest.raises(ValueError):
        config.carrier_map_hex(200, 512, [200])


class _Cfg(object):
    def __init__(self, N=512, occ=200, carriers=b""):
        self.fft_length, self.occupied_tones, self.carrier_map = N, occ, carriers


def _summary(P, npkt=10, err=None, ref=None, inv=None):
    occ = len(P)
    return {"npkt": npkt, "pre_power": np.asarray(P, np.float64) * npkt,
            "err": np.full(occ, 1.0) if err is None else err, "ref": np.full(occ, 100.0) if ref is None else ref,
            "inv_gain": np.full(occ, 4.0 * npkt) if inv is None else inv, "ninv": np.full(occ, npkt, np.uint32)}


def _pilots(N, occ):
    return np.asarray(config.make_ksfreq(N, occ)) != 0


def test_carrier_report_flat_spectrum():
    N, occ = 512, 200
    pil = _pilots(N, occ)
    S, Nn = 50.0, 0.5
    rep = csi.carrier_report(_summary(np.where(pil, S + Nn, Nn)), _Cfg(N, occ))
    np.testing.assert_allclose(rep["snr_preamble_db"], 10 * np.log10(S / Nn), rtol=1e-12)
    used = np.zeros(occ, bool)
    used[config.carrier_map(occ, occ, "FE7F", sink=True)] = True
    np.testing.assert_allclose(rep["snr_decision_db"][used], 20.0, rtol=1e-12)
    assert np.isnan(rep["snr_decision_db"][~used]).all() and (~used).sum() >= 2
    np.testing.assert_allclose(rep["gain_db"], 10 * np.log10(4.0), rtol=1e-12)


def test_carrier_report_noise_bump():
    N, occ = 512, 200
    pil = _pilots(N, occ)
    S, Nn, B = 50.0, 0.5, 5000.0
    base = np.where(pil, S + Nn, Nn)
    nul = np.flatnonzero(~pil)
    a, b = int(nul[40]), int(nul[44])               # a band from null bin to null bin
    P = base.copy()
    P[a:b + 1] += B
    ref = csi.carrier_report(_summary(base), _Cfg(N, occ))["snr_preamble_db"]
    got = csi.carrier_report(_summary(P), _Cfg(N, occ))["snr_preamble_db"]
    drop = ref - got
    hit = set(range(a, b + 1)) | {a - 1, b + 1}      # the band and its pilot neighbours
    assert pil[a - 1] and pil[b + 1]
    assert {i for i in range(occ) if drop[i] > 3.02} == hit
    assert (drop[sorted(hit)] > 10).all()
    # (a null bin next to a pilot neighbour borrows that pilot's signal estimate: at most 3 dB lower); nothing else moves
    far = [i for i in range(occ) if i < a - 2 or i > b + 2]
    assert np.array_equal(got[far], ref[far])


def test_carrier_report_band_edges():
    for N, occ in ((512, 200), (256, 120), (128, 100)):
        pil = _pilots(N, occ)
        rng = np.random.default_rng(occ)
        P = np.where(pil, 40.0, 0.0) + rng.uniform(0.2, 2.0, occ)
        rep = csi.carrier_report(_summary(P), _Cfg(N, occ))["snr_preamble_db"]
        for i, nb in ((0, 1), (occ - 1, occ - 2)):
            if pil[i]:     # one null neighbour only
                want = 10 * np.log10(max(P[i] - P[nb], 0) / P[nb])
            else:          # one pilot neighbour only, whose noise is the mean of the nulls on both of its sides
                j = nb
                nh = (P[j - 1] + P[j + 1]) / 2 if 0 < j < occ - 1 else P[i]
                want = 10 * np.log10(max(P[j] - nh, 0) / P[i])
            np.testing.assert_allclose(rep[i], want, rtol=1e-12)


def test_suggest_keeps_the_current_maps_exclusions():
    N, occ = 512, 200
    pil = _pilots(N, occ)
    rep = csi.carrier_report(_summary(np.where(pil, 50.5, 0.5)), _Cfg(N, occ))
    cur = config.carrier_map(occ, occ, "FE7F", sink=True)
    off = sorted(set(range(occ)) - set(cur))
    assert off                                        # "FE7F" leaves the carriers around DC off
    hx = csi.suggest_carrier_map(rep, _Cfg(N, occ), 10.0)
    assert config.carrier_map(occ, occ, hx, sink=True) == cur
    hx_all = csi.suggest_carrier_map(rep, _Cfg(N, occ), 10.0, respect_current=False)
    assert config.carrier_map(occ, occ, hx_all, sink=True) == list(range(occ))
    # a bad stretch is left out
    rep2 = dict(rep)
    rep2["snr_preamble_db"] = rep["snr_preamble_db"].copy()
    rep2["snr_preamble_db"][60:70] = 3.0
    got = config.carrier_map(occ, occ, csi.suggest_carrier_map(rep2, _Cfg(N, occ), 10.0), sink=True)
    assert got == [c for c in cur if not 60 <= c < 70]


def test_oracle_loopback_on_a_suggested_map(orc):
    N, occ = 512, 200
    zl = config.zeros_on_left(N, occ)
    want = [c for c in config.carrier_map(occ, occ, "FE7F", sink=True) if not 120 <= c < 128]
    hx = config.carrier_map_hex(occ, N, want)
    cfg = make_cfg("qpsk", N, occ, 128, carriers=hx)
    pay = make_payloads(4, 500, seed=5)
    iq, freq, _ = orc.tx(cfg, pay, want_taps=True)
    used = np.flatnonzero(np.abs(freq[1]) > 0)
    assert used.tolist() == [c + zl for c in want]
    x = loopback_stream(orc, cfg, pay)
    r = orc.rx(cfg, x)
    assert r.packets == [(True, p) for p in pay]
