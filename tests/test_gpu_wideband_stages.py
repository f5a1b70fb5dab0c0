"""The eight wideband stream stages (DDC, DDC bank, receive resampler, DUC, transmit resampler, channeliser, synthesis
bank, DUC bank) live on ONE handle.  They share one host-side skeleton (StreamStage, csrc/engine_stage.inc); each must
still own its history buffers, its staging buffers, its stream position and its HIP-event pair.  The per-stage files
check the receive stages together and the transmit stages together; this is the only place that has all eight
interleaved.  The last test is about a buffer that StreamStage holds for the five transmit stages: the host-mode copy
of the band a call adds onto."""
import numpy as np
import pytest

import duc_cases
import pfb_synth_cases
import tx_resamp_cases
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


# (stage, L, M): the five transmit stages, the resamplers on both sides of 1
ADD_CASES = [("duc", 4, 1), ("duc_bank", 4, 1), ("pfb_synth", 4, 1), ("tx_resamp", 3, 2), ("tx_resamp", 2, 3),
             ("tx_resamp_bank", 3, 2), ("tx_resamp_bank", 2, 3)]


def _add_case(stage, L, M, rng):
    """(cfg, rows, inputs of one workgroup tile, count(eng, nin)) of a transmit stage with 9 taps, K = 3 for the
    banks; the tile is the stage's own geometry as its test module restates it."""
    h = (rng.standard_normal(9) / 3.0).astype(np.float32)
    fcs = [0.21, -0.3, 0.0]
    fixed = lambda eng, n: n * L
    if stage == "duc":
        return duc.duc_cfg(L, fcs[0], taps=h), None, duc_cases.tile_outputs(L) // L, fixed
    if stage == "duc_bank":
        return duc.bank_cfg(L, fcs, taps=h), 3, duc_cases.tile_outputs(L) // L, fixed
    if stage == "pfb_synth":
        return pfb.synth_cfg(L, [1, 3, 0], taps=h), 3, pfb_synth_cases.tile_inputs(L), fixed
    counted = lambda eng, n: getattr(eng, stage + "_count")(n)
    if stage == "tx_resamp":
        return tx_resample.tx_resamp_cfg(L, M, fcs[0], taps=h), None, tx_resamp_cases.tile_inputs(L, M), counted
    return tx_resample.bank_cfg(L, M, fcs, taps=h), 3, tx_resamp_cases.tile_inputs(L, M), counted


@pytest.mark.parametrize("stage,L,M", ADD_CASES)
def test_add_after_reconfiguration_sees_no_stale_band(stage, L, M):
    """Host mode with ``add``: the band reaches the kernel through the stage's own device copy (StreamStage::d_add).
    On a handle that has added onto a long band, was switched off (set_<stage>(None)) and configured afresh, nothing
    of that band reaches the kernel with a shorter one: the stream in segments of 1, 0 and 3 samples and the rest
    gives, bit for bit, what a handle that never saw the first band gives in one call.  (Whether the copy's memory is
    reused cannot be seen from here.)  The stream begins at index 2, where at L < M the one-sample call completes no
    output (the history rolls, nothing is launched or copied back), and spans two workgroup tiles and a ragged
    tail."""
    rng = np.random.default_rng(300 + 10 * ADD_CASES.index((stage, L, M)))
    cfg, rows, tile, count = _add_case(stage, L, M, rng)
    call = lambda e, what, *args, **kw: getattr(e, what % stage)(*args, **kw)
    n1, n2 = 3 * tile + 101, 2 * tile + 37
    shape = lambda n: (n,) if rows is None else (rows, n)
    draw = lambda sh: (0.1 * (rng.standard_normal(sh) + 1j * rng.standard_normal(sh))).astype(np.complex64)
    x1, x2 = draw(shape(n1)), draw(shape(n2))

    fresh = engine.Engine(cfg=make_cfg())
    try:
        call(fresh, "set_%s", cfg)
        call(fresh, "%s_reset", 2)
        band2 = draw((count(fresh, n2),))
        want = call(fresh, "%s", x2, add=band2).copy()
    finally:
        fresh.close()
    assert len(want) == len(band2) > 2 * tile * L // M

    eng = engine.Engine(cfg=make_cfg())
    try:
        call(eng, "set_%s", cfg)
        band1 = draw((count(eng, n1),)) + np.complex64(8.0)              # a stale band would show
        assert len(call(eng, "%s", x1, add=band1)) == len(band1) > len(band2)
        call(eng, "set_%s", None)
        call(eng, "set_%s", cfg)
        call(eng, "%s_reset", 2)
        parts, a, o, empty = [], 0, 0, 0
        for n in (1, 0, 3, n2 - 4):
            cnt = count(eng, n)
            y = call(eng, "%s", x2[..., a:a + n], add=band2[o:o + cnt])
            assert len(y) == cnt
            empty += n > 0 and cnt == 0
            parts.append(y.copy())
            a, o = a + n, o + cnt
        assert empty == (1 if L < M else 0)
        got = np.concatenate(parts)
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes()
    finally:
        eng.close()
