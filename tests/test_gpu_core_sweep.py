"""The core modem against the oracle over the whole geometry ofdm_create accepts: every case of core_sweep_cases.py (the
classes it is stratified by, the reference's own conditioning and the frozen counts are there) through transmit, the
tapped receive pass and the tap-free one, bit for bit, in both sample formats; link quality and channel state on at every
fft_length; the fused front end wherever the geometry admits it; the filter's block grid at every transform length; and
the edge of the accepted space (fft_length 4096 with a cyclic prefix of 2048, 2049 and 4096; ntaps 0 and 513)."""
import numpy as np
import pytest

import core_sweep_cases as cs
import np_model as npm
from ofdm_uhd_amd import _abi, engine, iqio
from test_gpu_parity import _check_rx, _check_tx, check_rx_tap_free, check_rx_untapped, oracle_rx
from test_gpu_rx_paths import _room, _rx
from test_gpu_slicer import KNOBS

pytestmark = pytest.mark.gpu

CP_ERROR = "cyclic prefix longer than a k_sync tile"


def _defaults(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def _counts(eng, row):
    """The engine's counts of its last receive call against the frozen table's."""
    st = eng.last_stats
    assert (st["samples"], st["peaks"], st["frames"], st["packets"], st["crc_ok"]) == (
        row["samples"], row["flags"], row["frames"], row["packets"], row["crc_good"])
    assert st["overflow"] == 0


@pytest.mark.parametrize("fmt", ["fc32", "sc16"])
@pytest.mark.parametrize("N", cs.NS)
def test_sweep_parity(orc, monkeypatch, N, fmt):
    _defaults(monkeypatch)
    mine = [c for c in cs.CASES if c["N"] == N]
    assert len(mine) >= 7
    for c in mine:
        cfg, pay, x, ro = cs.reference(orc, c)
        assert orc.filter_fft_len(int(cfg.ntaps)) == cs.filter_F(cs.case_ntaps(c)), c["name"]
        eng = engine.Engine(cfg=cfg)
        _check_tx(orc, cfg, eng, pay)
        xin = x
        if fmt == "sc16":                            # both sides get the quantised values
            eng.set_rx_iq_format("sc16")
            xin = iqio.to_sc16(x)
            ro = oracle_rx(orc, cfg, iqio.from_sc16(xin))
        else:
            row = cs.PRECHECK[c["name"]]
            assert cs.row_of(ro, x, row["draw"], row["step"]) == row, c["name"]
        _check_rx(orc, cfg, eng, xin, ro)
        if fmt == "fc32":
            _counts(eng, cs.PRECHECK[c["name"]])
        check_rx_tap_free(eng, xin, ro, eng.rx_packet_pos().tolist())
        if fmt == "fc32":
            _counts(eng, cs.PRECHECK[c["name"]])
        if fmt == "sc16":
            ro.close()
        eng.close()


@pytest.mark.parametrize("N", cs.NS)
def test_sweep_quality_and_csi(orc, monkeypatch, N):
    """Link quality and per-subcarrier channel state on (the INSTR and the CSI instantiation decide), no tap: the same
    oracle result, at an odd geometry of every fft_length."""
    _defaults(monkeypatch)
    c = [c for c in cs.CASES if c["N"] == N and c["CP"] % 8 and cs.PRECHECK[c["name"]]["crc_good"]][-1]
    cfg, pay, x, ro = cs.reference(orc, c)
    eng = engine.Engine(cfg=cfg)
    _check_rx(orc, cfg, eng, x, ro)
    pos = eng.rx_packet_pos().tolist()
    eng.set_taps()
    eng.set_rx_quality(True)
    check_rx_untapped(eng, x, ro, pos)
    eng.set_rx_csi(True)
    check_rx_untapped(eng, x, ro, pos)
    eng.close()


def _front_cases():
    """One front-eligible case per (fft_length, transform length), and one case the front end does not take."""
    pick = {}
    for c in cs.CASES:
        if "front" in cs.labels(c):
            pick.setdefault((c["N"], cs.filter_F(cs.case_ntaps(c))), c)
    return [pick[k] for k in sorted(pick)]


FRONT = _front_cases()


@pytest.mark.parametrize("c", FRONT, ids=[c["name"] for c in FRONT])
def test_sweep_fused_front_end(orc, monkeypatch, c):
    """OFDM_FRONT=1 at every (N, F) that is eligible by itself, F = 64 and 128 included: every tap array_equal, and it is
    the fused kernel that ran."""
    _defaults(monkeypatch)
    monkeypatch.setenv("OFDM_FRONT", "1")
    cfg, pay, x, ro = cs.reference(orc, c)
    eng = engine.Engine(cfg=cfg)
    eng.prof_enable(True)
    eng.prof_reset()
    _check_rx(orc, cfg, eng, x, ro)
    prof = eng.prof()
    assert prof["k_front"][1] >= 1 and prof["k_chan_filter"][1] == 0 and prof["k_sync"][1] == 0, prof
    eng.close()


def test_front_end_coverage():
    got = {(c["N"], cs.filter_F(cs.case_ntaps(c))) for c in FRONT}
    for N in (64, 128, 256, 512, 1024):
        assert {(N, 64), (N, 128)} <= got, N
    assert {F for _, F in got} == {64, 128, 256, 512}


def test_sweep_front_end_ineligible(orc, monkeypatch):
    """A geometry the front end does not take (F = 1024) under OFDM_FRONT=1: the two-kernel path runs, same bits."""
    _defaults(monkeypatch)
    monkeypatch.setenv("OFDM_FRONT", "1")
    c = [c for c in cs.CASES if c["N"] == 512 and "nofront" in cs.labels(c)][0]
    cfg, pay, x, ro = cs.reference(orc, c)
    eng = engine.Engine(cfg=cfg)
    eng.prof_enable(True)
    eng.prof_reset()
    _check_rx(orc, cfg, eng, x, ro)
    prof = eng.prof()
    assert prof["k_front"][1] == 0 and prof["k_chan_filter"][1] >= 1 and prof["k_sync"][1] >= 1, prof
    eng.close()


# ---- the filter's block grid at every transform length ------------------------------------------------------------------------
def _grid_case(F):
    """A case of that transform length whose capture is long enough for the largest origin."""
    for c in cs.CASES:
        nt = cs.case_ntaps(c)
        B = cs.filter_F(nt) - nt + 1
        if cs.filter_F(nt) == F and cs.PRECHECK[c["name"]]["samples"] > 3 * B + 7 + 2 * B + nt and c["N"] <= 1024:
            return c
    raise AssertionError(F)


@pytest.mark.parametrize("fmt", ["fc32", "sc16"])
@pytest.mark.parametrize("F", [64, 128, 256, 512, 1024])
def test_origin_keeps_the_filter_grid_at_every_length(orc, monkeypatch, F, fmt):
    """test_gpu_stream_edges.test_origin_keeps_the_filter_grid's assertion: y from the first whole block on is the whole
    capture's, and within 1e-5 of the float64 filter in front of it."""
    _defaults(monkeypatch)
    c = _grid_case(F)
    cfg, pay, x, ro = cs.reference(orc, c)
    nt = int(cfg.ntaps)
    B = F - nt + 1
    eng = engine.Engine(cfg=cfg)
    q = None
    if fmt == "sc16":
        eng.set_rx_iq_format("sc16")
        q = iqio.to_sc16(x)
        x = iqio.from_sc16(q)
        whole = orc.rx(cfg, x, 1 << _abi.TAP_RX_CHAN_FILT).tap(_abi.TAP_RX_CHAN_FILT)
    else:
        whole = ro.tap(_abi.TAP_RX_CHAN_FILT)
    eng.set_taps(_abi.TAP_RX_CHAN_FILT)
    for o in (1, B - 1, B, B + 1, 3 * B + 7):
        if o < 1:
            continue                                 # (B = 1: no origin inside the first block)
        eng.set_origin(o)
        eng.rx(x[o:] if q is None else q[o:])
        y = eng.tap(_abi.TAP_RX_CHAN_FILT)
        assert len(y) == len(x) - o
        first = -(-(o + nt - 1) // B) * B            # first block boundary whose window lies in the call
        assert o + nt - 1 <= first < o + nt - 1 + B
        assert np.array_equal(y[first - o:], whole[first:]), o
        ref = npm.chan_filter(cfg, x[o:])
        if first > o:
            assert np.abs(y[:first - o] - ref[:first - o]).max() <= 1e-5, o
    eng.set_origin(0)
    eng.rx(x if q is None else q)
    assert np.array_equal(eng.tap(_abi.TAP_RX_CHAN_FILT), whole)
    eng.close()


# ---- the edge of the accepted space -------------------------------------------------------------------------------------------
def _edge_case(CP):
    c = dict(index=9000 + CP, kind="edge", N=4096, occ=2400, CP=CP, mod="qpsk", shift=4, ntaps=None, det=None, cfo=0.0, npkt=3,
             maxlen=40)
    c["name"] = "edge-4096-%d" % CP
    return c


def test_longest_cyclic_prefix_the_receiver_takes(orc, monkeypatch):
    """N = 4096, CP = 2048: one k_sync tile of M history, tiles_per_seg 96 -- received like any other case."""
    _defaults(monkeypatch)
    c = _edge_case(2048)
    cfg, pay, x = cs.capture(orc, c, 0, 0)
    ro = oracle_rx(orc, cfg, x)
    assert ro.stats["peaks"] >= 1 and ro.stats["frames"] >= 1
    eng = engine.Engine(cfg=cfg)
    _check_tx(orc, cfg, eng, pay)
    _check_rx(orc, cfg, eng, x, ro)
    check_rx_tap_free(eng, x, ro, eng.rx_packet_pos().tolist())
    eng.close()


@pytest.mark.parametrize("CP", [2049, 4096])
def test_cyclic_prefix_beyond_a_tile_is_refused_by_rx_only(orc, monkeypatch, CP):
    """ofdm_create takes it and transmit equals the oracle; every ofdm_rx returns OFDM_E_INVAL in these words, writes
    nothing behind the caller's capacities, and the handle transmits the same bits afterwards."""
    _defaults(monkeypatch)
    c = _edge_case(CP)
    cfg, pay, x = cs.capture(orc, c, 0, 0)
    eng = engine.Engine(cfg=cfg)
    _check_tx(orc, cfg, eng, pay)
    eng.set_taps()
    iq0 = eng.tx(pay)
    for _ in range(2):
        out = _rx(eng, x, *_room(cfg, x))
        assert out["rc"] == _abi.OFDM_E_INVAL and CP_ERROR in out["err"], out
    with pytest.raises(ValueError, match=CP_ERROR):
        eng.rx(x)
    assert np.array_equal(eng.tx(pay), iq0)
    _check_tx(orc, cfg, eng, pay)
    eng.close()


@pytest.mark.parametrize("ntaps", [0, 513])
def test_ntaps_outside_the_table_is_refused(ntaps):
    cfg = cs.case_cfg(cs.CASES[0])
    cfg.ntaps = ntaps
    with pytest.raises(ValueError, match="ntaps"):
        engine.Engine(cfg=cfg)
