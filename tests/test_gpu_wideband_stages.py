"""The eight wideband stream stages (DDC, DDC bank, receive resampler, DUC, transmit resampler, channeliser, synthesis
bank, DUC bank) live on ONE handle.  They share one host-side skeleton (StreamStage, csrc/engine_stage.inc); each must
still own its history buffers, its staging buffers, its stream position and its HIP-event pair.  The per-stage files
check the receive stages together and the transmit stages together; this is the only place that has all eight
interleaved."""
import numpy as np
import pytest

from helpers import make_cfg
from ofdm_uhd_amd import ddc, duc, engine, pfb, resample, tx_resample

pytestmark = pytest.mark.gpu

STAGES = ("ddc", "ddc_bank", "resamp", "duc", "tx_resamp", "pfb", "pfb_synth", "duc_bank")
# the stages whose output is (K, nout), and those whose input is (K, nin)
ROWS_OUT = ("ddc_bank", "pfb")
ROWS_IN = ("pfb_synth", "duc_bank")
# samples of history a stage carries from call to call: ntaps - 1 (DDC, bank, channeliser), (ntaps - 1) // L (the
# others; the synthesis bank and the DUC bank per row, L = M for the synthesis bank)
HISTORY = {"ddc": 6, "ddc_bank": 6, "resamp": 5, "duc": 2, "tx_resamp": 5, "pfb": 6, "pfb_synth": 5, "duc_bank": 2}
# chunk 2 is shorter than the stage's history (the history roll keeps the tail of the old one), and still long enough
# that the call has outputs at the position chunk 1 leaves the stream in (so that it is timed)
CHUNKS = {"ddc": (1500, 3, 1400), "ddc_bank": (1200, 4, 1801), "resamp": (1001, 3, 2000), "duc": (1300, 1, 900),
          "tx_resamp": (999, 4, 1600), "pfb": (1202, 3, 1500), "pfb_synth": (700, 2, 500), "duc_bank": (900, 1, 700)}


def _configs():
    rng = np.random.default_rng(21)
    t7 = lambda: (rng.standard_normal(7) / 3.0).astype(np.float32)
    t23 = lambda: (rng.standard_normal(23) / 3.0).astype(np.float32)
    return {"ddc": ddc.ddc_cfg(3, 0.21, taps=t7()),
            "ddc_bank": ddc.bank_cfg(3, [-0.3, 0.12], taps=t7()),
            "resamp": resample.resamp_cfg(4, 3, -0.17, taps=t23()),
            "duc": duc.duc_cfg(3, 0.25, taps=t7()),
            "tx_resamp": tx_resample.tx_resamp_cfg(4, 3, -0.2, taps=t23()),
            "pfb": pfb.pfb_cfg(4, channels=[1, 3], taps=t7()),
            "pfb_synth": pfb.synth_cfg(4, [1, 3], taps=t23()),
            "duc_bank": duc.bank_cfg(3, [-0.3, 0.12], taps=t7())}


def _chunks(name):
    """The stage's own stream (a seed per stage; one stream per row for the two transmit banks), cut into its three
    chunks."""
    n = CHUNKS[name]
    rng = np.random.default_rng(100 + STAGES.index(name))
    shape = (2, sum(n)) if name in ROWS_IN else (sum(n),)
    x = (0.1 * (rng.standard_normal(shape) + 1j * rng.standard_normal(shape))).astype(np.complex64)
    return [x[..., :n[0]], x[..., n[0]:n[0] + n[1]], x[..., n[0] + n[1]:]]


def _join(name, parts):
    return np.concatenate(parts, axis=1 if name in ROWS_OUT else 0)


def _readable(eng, name):
    try:
        return getattr(eng, name + "_last_ms")() >= 0.0
    except ValueError:
        return False


def test_eight_stages_interleaved_on_one_handle():
    cfgs = _configs()
    chunks = {s: _chunks(s) for s in STAGES}
    for s in STAGES:
        assert 1 <= chunks[s][1].shape[-1] < HISTORY[s]

    # what each stage gives for its chunks on a handle that has nothing else configured
    want = {}
    for s in STAGES:
        e = engine.Engine(cfg=make_cfg())
        try:
            getattr(e, "set_" + s)(cfgs[s])
            want[s] = _join(s, [getattr(e, s)(c).copy() for c in chunks[s]])
        finally:
            e.close()

    eng = engine.Engine(cfg=make_cfg())
    try:
        for s in STAGES:
            getattr(eng, "set_" + s)(cfgs[s])
        got = {s: [] for s in STAGES}
        # round 1, not profiled: no stage has a time
        for s in STAGES:
            got[s].append(getattr(eng, s)(chunks[s][0]).copy())
        assert not any(_readable(eng, s) for s in STAGES)
        # round 2, profiled: the event pairs are created one after the other while every stage is live, and a stage's
        # time becomes readable with its own call, not with another stage's
        eng.prof_enable(True)
        for i, s in enumerate(STAGES):
            assert [_readable(eng, t) for t in STAGES] == [j < i for j in range(len(STAGES))], s
            y = getattr(eng, s)(chunks[s][1]).copy()
            assert y.size > 0, s
            got[s].append(y)
            assert _readable(eng, s), s
        # round 3, not profiled again: a call clears its own stage's time and nobody else's
        eng.prof_enable(False)
        for i, s in enumerate(STAGES):
            assert [_readable(eng, t) for t in STAGES] == [j >= i for j in range(len(STAGES))], s
            got[s].append(getattr(eng, s)(chunks[s][2]).copy())
        assert not any(_readable(eng, s) for s in STAGES)
        for s in STAGES:
            y = _join(s, got[s])
            assert y.shape == want[s].shape and np.array_equal(y, want[s]), s
    finally:
        eng.close()
