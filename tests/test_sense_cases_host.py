"""What sense_cases.py promises, without a GPU: the launch geometry each case is for (restated from sense_enqueue), the
oracle against the float64 model on every capture, that every round and every lane of every case decides part of every
message -- otherwise test_gpu_sense_geometry.py could pass with a round or a lane skipped -- and the oracle's decisions
against the float64 message-order sum at every (avg, skip)."""
import numpy as np
import pytest

import sense_cases as sn
from ofdm_uhd_amd import predictive_sense


@pytest.mark.parametrize("c", sn.CASES, ids=sn.ids(sn.CASES))
def test_geometry(c):
    """The natural cases run with split=None: what they reach depends on the 2048 in the restatement alone."""
    geo = sn.case_geometry(c)
    assert geo.G == {64: 32, 128: 16, 256: 8, 512: 4, 1024: 2, 2048: 1, 4096: 1}[c.S]
    assert geo.stride == geo.nsplit * geo.G and geo.rounds == c.rounds and geo.nsplit == len(c.last)
    assert (c.split is None) == (c in sn.NATURAL)
    if c.split is not None:
        assert geo.nsplit == c.split
    if c.id == "two-launches":
        # one vector per message: the launch offset is what this one is for
        assert (geo.rounds, geo.launches, c.nmsgs - sn.MAX_GRID_Y) == (1, 2, 2)
    else:
        assert geo.rounds >= 2 and geo.launches == 1
    # every accrued vector has a slot of its own, inside the grid
    assert len({tuple(s) for s in geo.slots.tolist()}) == c.dwell
    assert geo.slots[:, 1].max() < geo.nsplit and geo.slots[:, 2].max() < geo.G
    live = sn.live_groups(geo)
    assert (live[:-1] == geo.G).all()                  # full until the last round
    assert tuple(live[-1].tolist()) == c.last
    assert int(live.sum()) == c.dwell


def test_table():
    """The rows the cases are for: per S, three rounds with dead groups, a last round with one live group in the second
    workgroup, one with nothing dead, one with two dead workgroups; per = 1, 2, 3 of the decision kernel at every S."""
    assert len(sn.FORCED) == 4 * len(sn.SIZES) + 1 and len(set(sn.ids(sn.CASES))) == len(sn.CASES)
    for S in sn.SIZES:
        rows = [c for c in sn.FORCED if c.S == S and "c5" not in c.id]
        G = sn.case_geometry(rows[0]).G
        assert [(c.split, c.dwell) for c in rows] == [(1, 2 * G + max(1, G // 4)), (2, 3 * G + 1), (2, 4 * G), (3, 3 * G + 1)]
        assert sorted((c.avg, c.skip) for c in rows) == sorted(sn.AVG_SKIP)
        assert all(c.nmsgs == 3 for c in rows)
        if G > 1:
            assert rows[0].last[0] < G                                  # dead groups inside the only workgroup
    assert {c.tune for c in sn.FORCED} == {0, 1, 2}
    c5 = sn.BY_ID["s4096-c5-15-rounds"]
    assert (c5.S, c5.tune, c5.dwell, c5.split, c5.nmsgs, c5.rounds) == (4096, 2, 15, 1, 2, 15)
    assert [(c.S, c.rx_scale is None) for c in sn.SC16] == [(64, True), (512, True), (1024, False), (2048, True), (4096, False)]
    assert max(len(sn.built(c)[1]) for c in sn.FORCED if "c5" not in c.id) < 80000                 # "about 70 k samples"


@pytest.mark.parametrize("c", sn.CASES, ids=sn.ids(sn.CASES))
def test_oracle_vs_model_and_nothing_idle(orc, c):
    sc, x, ref = sn.reference(orc, c)
    xf = sn.built(c)[2]
    geo = sn.case_geometry(c)
    pw = sn.np_sense_powers(sc, xf)
    model = pw.max(axis=1)
    assert ref["msgs"].shape == model.shape == (c.nmsgs, c.S)
    # the bar of test_oracle_vs_numpy_model (north star)
    err = float(np.max(np.abs(ref["msgs"] - model)))
    print("%s: max |oracle - model| = %.3g of the peak" % (c.id, err / model.max()))
    assert err <= 1e-5 * model.max()
    # the message without one round, and without one (workgroup, group) lane: every message differs from the full one
    # after rounding to float32 (a vector that alone holds a bin's maximum is missed when it goes)
    winner = sn.sole_winners(pw)
    f = np.arange(c.dwell)
    by_round = sn.decides(winner, f // geo.stride, geo.rounds)
    assert by_round.all(), np.argwhere(~by_round)[:8]
    lanes = min(geo.stride, c.dwell)
    by_lane = sn.decides(winner, f % geo.stride, lanes)
    if lanes <= c.S:
        assert by_lane.all(), np.argwhere(~by_lane)[:8]
    else:
        # more lanes than bins (S = 64, three workgroups: 96 on 64): no message can be decided by all of them.  Every
        # message is decided by as many lanes as it can be short of one, every lane decides one of the messages
        assert (by_lane.sum(axis=1) >= c.S - 1).all() and by_lane.any(axis=0).all()
    if c.dwell <= c.S:
        # here every single vector decides its bin
        assert sn.decides(winner, f, c.dwell).all()
    # nothing of the tune delay or the tail got in: the loudest accrued bin stays far below their tone
    assert ref["msgs"].max() < 2.0e-3 * sc.threshold / sn.THRESHOLD
    if geo.launches > 1:
        # what a second launch without its offset would leave: nothing, or the first messages again
        for m in range(sn.MAX_GRID_Y, c.nmsgs):
            assert ref["msgs"][m].min() > 0 and not np.array_equal(ref["msgs"][m], ref["msgs"][m - sn.MAX_GRID_Y])


@pytest.mark.parametrize("c", sn.CASES, ids=sn.ids(sn.CASES))
def test_oracle_decisions(orc, c):
    sc, x, ref = sn.reference(orc, c)
    nd = c.nmsgs // (c.avg + c.skip)
    assert nd >= 1 and len(ref["hex"]) == nd and ref["mean"].shape == ref["bits"].shape == (nd, c.S)
    mean, bits = sn.np_sense_decide(sc, ref["msgs"])
    assert np.array_equal(ref["mean"], mean) and np.array_equal(ref["bits"], bits)
    assert ref["hex"] == [predictive_sense.hex_conv(b.tolist()) for b in bits]
    # both decisions occur: the threshold lies inside the tones' range
    assert 0 < int(bits.sum()) < bits.size


def test_windows():
    """The forced cases' windows are asymmetric (tap t + m * TPT is not tap S - 1 - t - m * TPT, nor the default's
    mirror S - 2 - i), and differ from case to case."""
    seen = set()
    for c in sn.FORCED:
        w = np.array(sn.case_window(c))
        assert w.min() >= 0.5 and w.max() < 1.5
        assert np.abs(w - w[::-1]).max() > 0.5 and np.abs(w[:-1] - w[:-1][::-1]).max() > 0.5
        seen.add(w.tobytes())
    assert len(seen) == len(sn.FORCED)
