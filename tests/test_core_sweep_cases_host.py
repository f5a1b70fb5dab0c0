"""The conditions core_sweep_cases.py sets itself, on the CPU: the list comes from its seed alone, every class is present on
both sides, the frozen table is what the ladder of (SNR, channel seed) gives on the reference pair -- the oracle against the
float64 model within test_oracle.py's bounds, which also holds the oracle itself at filter transform lengths 64, 128 and
1024 -- and the shares the module promises hold.  No engine anywhere."""
import pytest

import core_sweep_cases as cs
from helpers import make_cfg

REPLACED_MAX, GOOD_MIN = 0.05, 0.90


def test_the_list_is_its_seed():
    again = cs._make_cases()
    assert [c["name"] for c in again] == [c["name"] for c in cs.CASES]
    assert set(cs.PRECHECK) == {c["name"] for c in cs.CASES}
    assert len([c for c in cs.CASES if c["kind"] == "rand"]) == cs.RANDOM


def test_every_class_on_both_sides():
    cs.check_classes(cs.CASES, cs.PRECHECK)
    cnt = cs.class_counts(cs.CASES, cs.PRECHECK)
    print("cases per class: " + ", ".join("%s %d" % kv for kv in sorted(cnt.items())))
    for N in cs.NS:
        for mod in cs.MODS:
            assert any(c["N"] == N and c["mod"] == mod for c in cs.CASES), (N, mod)
    # every case carries an empty payload, three or four packets (the short captures fewer), 0 .. 300 bytes
    for c in cs.CASES:
        sizes = cs.case_sizes(c, cs.PRECHECK[c["name"]]["draw"])
        assert 0 in sizes and max(sizes) <= 300 and (len(sizes) in (3, 4) or c["kind"] == "short"), c["name"]
        assert cs.PRECHECK[c["name"]]["samples"] <= cs.MAX_SAMPLES, c["name"]


def test_residues_the_carrier_map_refuses():
    """occupied_tones - 16 = 2 or 6 (mod 8) is outside the accepted space: the sweep cannot hold it."""
    for N in cs.NS:
        assert {(o - 16) % 8 for o in cs.accepted_occ(N)} == {0, 4}
        for occ in (N // 2 + 2, N // 2 + 6):
            assert (occ - 16) % 8 in (2, 6)
            with pytest.raises(ValueError):
                make_cfg("qpsk", N, occ, N // 4)


def test_filter_lengths(orc):
    seen = set()
    for c in cs.CASES:
        cfg = cs.case_cfg(c)
        assert int(cfg.ntaps) == cs.case_ntaps(c), c["name"]
        F = orc.filter_fft_len(int(cfg.ntaps))
        assert F == cs.filter_F(int(cfg.ntaps)) and "F%d" % F in cs.labels(c), c["name"]
        seen.add((c["N"], F))
    assert {F for _, F in seen} == {64, 128, 256, 512, 1024}
    for N in cs.NS:
        assert {(N, 64), (N, 128), (N, 1024)} <= seen, N


@pytest.mark.parametrize("N", cs.NS)
def test_frozen_table_is_what_the_ladder_gives(orc, N):
    """Every case: the frozen (draw, step) is the first conditioned capture -- so the oracle agrees with the float64 model
    on it -- and the oracle's counts on it are the frozen ones."""
    for c in cs.CASES:
        if c["N"] != N:
            continue
        row = cs.PRECHECK[c["name"]]
        assert cs.condition(orc, c) == (row["draw"], row["step"]), c["name"]
        cfg, pay, x = cs.capture(orc, c, row["draw"], row["step"])
        ro = orc.rx(cfg, x, 0)
        assert cs.row_of(ro, x, row["draw"], row["step"]) == row, c["name"]
        assert row["flags"] >= 1 and row["frames"] >= 1, c["name"]
        ro.close()


def test_shares():
    rows = cs.PRECHECK
    replaced = sorted(n for n, r in rows.items() if r["draw"] > 0)
    print("replaced by a later draw: %s" % replaced)
    assert len(replaced) <= REPLACED_MAX * len(rows)
    good = sum(1 for r in rows.values() if r["crc_good"] >= 1)
    print("cases with a CRC-good packet: %d of %d; first ladder step: %d" % (
        good, len(rows), sum(1 for r in rows.values() if (r["draw"], r["step"]) == (0, 0))))
    assert good >= GOOD_MIN * len(rows)
