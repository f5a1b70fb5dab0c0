"""The engine against the oracle on every capture of capture_edge_cases.py: capture ends around the sampler's acceptance
test and each step of its symbol count, captures shorter than every window the receiver has, starts inside the first
preamble, flags and capture ends on k_sync's tile and segment boundaries.  (What each family is for, and that the oracle
and the float64 model agree on every case: test_capture_edges_host.py.)

No tolerance anywhere.  The two exhaustive sweeps at 64/48/16 run the tap-free default path -- the lean kernel with the
frame counts n_lo / n_hi left on the device: packets (the failed ones byte for byte), flags, frames, the eight counters,
packet positions.  The structured subsets run four ways: every tap array_equal (test_gpu_parity._check_rx), tap-free,
OFDM_RX_SYNCS=1, and the fused front end (N <= 512); SHORT and the END subsets also as 16-bit samples, and the END
subsets from a device buffer of exactly the capture's length."""
import numpy as np
import pytest

import capture_edge_cases as cc
from ofdm_uhd_amd import _abi
from test_gpu_parity import STAT_KEYS, _check_rx, check_rx_tap_free, check_rx_untapped

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engines():
    """One engine per geometry (and per input format / pointer mode), module scope."""
    from ofdm_uhd_amd import engine
    from helpers import make_cfg
    made = {}

    def get(geom, fmt=None, dev=False):
        if (geom, fmt, dev) not in made:
            g = cc.GEOMS[geom]
            e = engine.Engine(cfg=make_cfg(g.mod, g.N, g.occ, g.CP, device_ptrs=True) if dev else cc.cfg_of(geom))
            if fmt:
                e.set_rx_iq_format(fmt)
            made[(geom, fmt, dev)] = e
        return made[(geom, fmt, dev)]
    yield get
    for e in made.values():
        e.close()


@pytest.fixture(autouse=True)
def _default_paths(monkeypatch):
    monkeypatch.delenv("OFDM_RX_SYNCS", raising=False)
    monkeypatch.delenv("OFDM_FRONT", raising=False)


@pytest.mark.parametrize("i", range(cc.NCHUNKS))
@pytest.mark.parametrize("family", cc.EXHAUSTIVE)
def test_sweep_tap_free(orc, engines, family, i):
    """Every length e of the END sweep, every offset s of the FRONT sweep."""
    eng = engines(cc.geom_of(family))
    for case in cc.chunk(orc, family, i):
        try:
            check_rx_tap_free(eng, case[2], cc.reference(orc, case, taps=False), cc.packet_positions(case))
        except AssertionError as err:
            raise AssertionError("%s: %s" % (case[0], err))
        cc.release(case)


def _four_ways(orc, monkeypatch, eng, case):
    cid, cfg, x = case
    ro = cc.reference(orc, case)
    pos = cc.packet_positions(case)
    _check_rx(orc, cfg, eng, x, ro)                              # every tap
    assert eng.rx_packet_pos().tolist() == pos
    check_rx_tap_free(eng, x, ro, pos)                           # the lean kernel, counts on the device
    monkeypatch.setenv("OFDM_RX_SYNCS", "1")
    check_rx_untapped(eng, x, ro, pos)                           # the counts read back as the call goes
    monkeypatch.delenv("OFDM_RX_SYNCS")
    if cfg.fft_length <= 512:
        monkeypatch.setenv("OFDM_FRONT", "1")
        eng.prof_enable(True)
        eng.prof_reset()
        _check_rx(orc, cfg, eng, x, ro)
        prof = eng.prof()
        eng.prof_enable(False)
        monkeypatch.delenv("OFDM_FRONT")
        assert prof["k_chan_filter"][1] == 0 and prof["k_sync"][1] == 0 and prof["k_front"][1] == (1 if len(x) else 0), prof


@pytest.mark.parametrize("family", cc.STRUCTURED)
def test_structured_four_ways(orc, monkeypatch, engines, family):
    eng = engines(cc.geom_of(family))
    for case in cc.cases(orc, family):
        try:
            _four_ways(orc, monkeypatch, eng, case)
        except AssertionError as err:
            raise AssertionError("%s: %s" % (case[0], err))


def test_multi_wave_end_cuts(orc, engines):
    """16-QAM 2048/1200/512 (frames of several waves): the END cuts, every tap and tap-free."""
    eng = engines("qam16-2048")
    for case in cc.cases(orc, "end-qam16-2048"):
        cid, cfg, x = case
        ro = cc.reference(orc, case)
        try:
            _check_rx(orc, cfg, eng, x, ro)
            check_rx_tap_free(eng, x, ro, cc.packet_positions(case))
        except AssertionError as err:
            raise AssertionError("%s: %s" % (cid, err))


@pytest.mark.parametrize("family", cc.SC16)
def test_sc16(orc, engines, family):
    """SHORT and the END subsets as 16-bit samples: the engine converts as it loads, the oracle gets the same values."""
    eng = engines(cc.geom_of(family), "sc16")
    for case in cc.sc16_cases(orc, family):
        cid, cfg, q = case
        assert q.dtype == np.int16 and q.shape == (len(q), 2)
        ro = cc.reference(orc, case)
        try:
            _check_rx(orc, cfg, eng, q, ro)
            check_rx_tap_free(eng, q, ro, cc.packet_positions(case))
        except AssertionError as err:
            raise AssertionError("%s: %s" % (cid, err))


@pytest.mark.parametrize("geom", cc.SUBSET)
def test_end_cuts_from_device_buffer(orc, engines, geom):
    """Device-pointer mode: the capture in a torch buffer of exactly e samples (nothing behind the last one belongs to
    the call), tap-free."""
    import torch
    eng = engines(geom, dev=True)
    eng.set_taps()
    L = cc.GEOMS[geom].N + cc.GEOMS[geom].CP
    for case in cc.cases(orc, "end-" + geom):
        cid, cfg, x = case
        ro = cc.reference(orc, case)
        n = len(x)
        xd = torch.from_numpy(x.view(np.float32).copy()).cuda()
        assert xd.numel() == 2 * n
        max_pkts = n // L + 16
        cap = max_pkts * 64 + n
        payd = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        npk, off, ln, ok = eng.rx_device(xd.data_ptr(), n, payd.data_ptr(), cap, max_pkts)
        torch.cuda.synchronize()
        pay = payd.cpu().numpy()
        pk = [(bool(ok[k]), pay[int(off[k]):int(off[k]) + int(ln[k])].tobytes()) for k in range(npk)]
        assert pk == ro.packets, cid
        assert eng.tap(_abi.TAP_RX_PEAKS).tolist() == ro.tap(_abi.TAP_RX_PEAKS).tolist(), cid
        assert eng.tap(_abi.TAP_RX_FRAMES).tolist() == ro.tap(_abi.TAP_RX_FRAMES).tolist(), cid
        for k in STAT_KEYS:
            assert eng.last_stats[k] == ro.stats[k], (cid, k)
        assert eng.last_stats["overflow"] == 0
        assert eng.rx_packet_pos().tolist() == cc.packet_positions(case), cid
