"""The coded-stream captures on the CPU (tests/coded_stream_cases.py): the levels and seeds its docstring records really
give every configuration's model chain something to do, the capture has the length the streamed tests need, and the
chunkings are what they are named."""
import numpy as np
import pytest

import coded_stream_cases as cs


@pytest.mark.parametrize("name", cs.IDS)
def test_the_models_meet_the_conditions_on_the_cpu(orc, name):
    c = cs.precheck(name)
    print("%s: %s" % (name, " ".join("%s %d" % kv for kv in c.items())))
    cs.nontrivial(name, c)
    assert c["right"] == c["ok"]                                   # no decoder reported ok for a payload that was not sent
    assert 4 * cs.span_of() <= c["samples"] <= cs.MAX_SAMPLES and 24 <= c["sent"] <= 40
    assert c == cs.PRECHECK[name]


def test_payloads_and_layout():
    pay, _ = cs.payloads_of(cs.CONFIGS["ldpc-soft"]["seed"])
    sizes = [len(p) for p in pay]
    assert set(cs.ALWAYS) <= set(sizes) and max(sizes) == 300 and len(set(pay)) == len(pay)
    assert all(p[2:4] == b"\0\0" and int.from_bytes(p[:2], "big") == i for i, p in enumerate(pay) if len(p) >= 4)
    pay2, x = cs.capture_on_the_cpu("ldpc-soft")
    assert pay2 == pay and x.dtype == np.complex64 and not x.flags.writeable
    assert np.count_nonzero(x[:cs.LEAD] == 0) == 0                 # noise everywhere, the lead included


def test_chunkings():
    n = 250001
    assert cs.chunks("one", n) == [(0, n)]
    for name in ("40000", "7000"):
        cuts = cs.chunks(name, n)
        assert cuts[0][0] == 0 and cuts[-1][1] == n and all(a[1] == b[0] for a, b in zip(cuts, cuts[1:]))
        assert {b - a for a, b in cuts[:-1]} == {int(name)}
    cuts = cs.chunks("random", n)
    assert cuts == cs.chunks("random", n) and cuts[-1][1] == n and all(1 <= b - a <= 90000 for a, b in cuts)
    assert len({b - a for a, b in cuts}) > 2
