"""The receiver against the oracle where the clean captures of test_gpu_parity do not reach: points that leave the sign
and the grid slicer through their fall-throughs (slicer_cases.py: what the captures are and which classes of points
test_slicer_cases_host.py shows them to hold), with taps (packets from the lean kernel's pass, counts read back as the
call goes, symbol taps from a second, instrumented pass), without any (the lean kernel alone, counts kept on the device)
and with link quality and channel state on (the instrumented and CSI instantiations decide), and every launch variant an LDS-fit formula chooses between, forced both ways through the knob that exists for
it (OFDM_DEMOD_LDS, OFDM_SYNC_W, OFDM_SYNC_STATIC, OFDM_EXACT_SMALL: csrc/engine_rx.inc).  The oracle always runs the
full search and has no variants: one result per capture, computed once, is what every setting is compared with."""
import numpy as np
import pytest

import slicer_cases as sc
from helpers import make_cfg, make_payloads
from ofdm_uhd_amd import _abi
from test_gpu_parity import _check_rx, check_rx_tap_free, check_rx_untapped

pytestmark = pytest.mark.gpu

KNOBS = ("OFDM_DEMOD_LDS", "OFDM_SYNC_W", "OFDM_SYNC_STATIC", "OFDM_EXACT_SMALL", "OFDM_RX_SYNCS", "OFDM_FRONT",
         "OFDM_SENSE_SPLIT")
LDS_ERROR = "configuration needs more than 160 KiB of LDS in k_rx_demod"


def _engine(cfg):
    from ofdm_uhd_amd import engine
    return engine.Engine(cfg=cfg)


def _defaults(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def _both_kernels(orc, cfg, eng, x, ro):
    """_check_rx with its seven taps, then the same capture without any."""
    _check_rx(orc, cfg, eng, x, ro)
    pos = eng.rx_packet_pos().tolist()
    check_rx_tap_free(eng, x, ro, pos)
    return pos


# ---- a. every row: with taps, without, with link quality and channel state -------------------------------------------------
@pytest.mark.parametrize("r", sc.ROWS, ids=sc.IDS)
def test_impaired_payload_parity(orc, monkeypatch, r):
    _defaults(monkeypatch)
    cfg, x, pay, ro = sc.reference(orc, r)
    assert any(ok for ok, _ in ro.packets) and not all(ok for ok, _ in ro.packets)      # (the bytes of a failed packet count)
    eng = _engine(cfg)
    pos = _both_kernels(orc, cfg, eng, x, ro)
    # instrumentation moves no decision, still no tap: link quality on (the instrumented instantiation decides), then
    # channel state as well (the CSI one)
    eng.set_rx_quality(True)
    check_rx_untapped(eng, x, ro, pos)
    eng.set_rx_csi(True)
    check_rx_untapped(eng, x, ro, pos)
    eng.close()


# ---- b. the demodulator's LDS extras, forced both ways --------------------------------------------------------------------
# bit 0: twiddles in LDS (an instantiation of its own from N = 2048 on, no effect below), bit 1: the carrier map in LDS
LDS_VARIANTS = [(i, v) for i in ("qpsk-512", "qam256-64", "8psk-256", "qam16-2048")
                for v in ((0, 1, 2, 3) if i == "qam16-2048" else (0, 2))]


@pytest.mark.parametrize("rid,v", LDS_VARIANTS, ids=["%s-lds%d" % iv for iv in LDS_VARIANTS])
def test_demod_lds_variants(orc, monkeypatch, rid, v):
    _defaults(monkeypatch)
    cfg, x, pay, ro = sc.reference(orc, sc.ROWS[sc.IDS.index(rid)])
    eng = _engine(cfg)
    # the default never lacks LDS
    eng.set_taps()
    assert eng.rx(x) == ro.packets
    monkeypatch.setenv("OFDM_DEMOD_LDS", str(v))
    try:
        _both_kernels(orc, cfg, eng, x, ro)
    except ValueError as e:
        # a forced extra that does not fit is refused, in these words, and nothing else is an accepted failure
        assert LDS_ERROR in str(e)
    eng.close()


# ---- c. k_sync's instantiations and k_sync_exact's split point ------------------------------------------------------------
SYNC_TAPS = (_abi.TAP_RX_CHAN_FILT, _abi.TAP_RX_METRIC, _abi.TAP_RX_PRESEL)
_SYNC_REF = {}


def _sync_reference(orc, which):
    """(cfg, x, ro) of the two captures of test_sync_variants, computed once."""
    if which not in _SYNC_REF:
        if which == "n512":
            cfg, pay = make_cfg("qpsk", 512, 200, 128), make_payloads(3, 300, seed=31)
        elif which == "n1024":
            cfg, pay = make_cfg("qpsk", 1024, 600, 256), make_payloads(2, 300, seed=34)
        else:       # history longer than a tile: the ring layout by itself
            cfg, pay = make_cfg("8psk", 4096, 2456, 1440), make_payloads(1, 300, seed=32)
        x = sc.build_capture(orc, cfg, pay, ("clean",) * len(pay), 33, cfo_bins=0.05)
        x.setflags(write=False)
        _SYNC_REF[which] = (cfg, x, orc.rx(cfg, x, sum(1 << t for t in SYNC_TAPS)))
    return _SYNC_REF[which]


def _check_sync(eng, x, ro):
    eng.set_taps(*SYNC_TAPS)
    assert eng.rx(x) == ro.packets
    for t in SYNC_TAPS + (_abi.TAP_RX_ANGLES,):
        assert np.array_equal(eng.tap(t), ro.tap(t)), t
    assert eng.tap(_abi.TAP_RX_PEAKS).tolist() == ro.tap(_abi.TAP_RX_PEAKS).tolist()


# OFDM_SYNC_STATIC=0 asks for the ring layout where the fixed one would do.  At N = 512 the tile's M values overlay its
# samples in LDS, which only the fixed layout allows: the knob is without effect there (before this test existed it
# ran the ring on the overlaid layout, and the pre-selection came out wrong).  N = 1024 is where it does force the ring.
SYNC_SETTINGS = ([("n512", {"OFDM_SYNC_W": w, "OFDM_SYNC_STATIC": s}) for w in (2, 3, 4, 5, 6) for s in (0, 1)] +
                 [("n512", {"OFDM_EXACT_SMALL": e}) for e in (0, 1, 2048)] +
                 [("n1024", {"OFDM_SYNC_W": w, "OFDM_SYNC_STATIC": s}) for w in (2, 4) for s in (0, 1)] +
                 [("n4096", {"OFDM_SYNC_W": w, "OFDM_SYNC_STATIC": s}) for w in (2, 3) for s in (0, 1)])
NPKT = {"n512": 3, "n1024": 2, "n4096": 1}


@pytest.mark.parametrize("which,env", SYNC_SETTINGS,
                         ids=["%s-%s" % (w, "-".join("%s%d" % (k[5:].lower(), e[k]) for k in sorted(e))) for w, e in SYNC_SETTINGS])
def test_sync_variants(orc, monkeypatch, which, env):
    _defaults(monkeypatch)
    cfg, x, ro = _sync_reference(orc, which)
    assert all(ok for ok, _ in ro.packets) and len(ro.packets) == NPKT[which]
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    eng = _engine(cfg)
    _check_sync(eng, x, ro)
    eng.close()
