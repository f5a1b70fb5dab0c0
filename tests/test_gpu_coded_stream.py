"""Coded links across stream cuts: ofdm_demod.feed() over chunks == one work() on the whole capture, in EVERY field --
the returned packets, last_fec, last_ldpc, last_rs, last_rs_second, last_fec_rel, last_soft, the callback's sequence,
n_packets and n_ok -- for the ten configurations of tests/coded_stream_cases.py, each on its own capture of more than
four spans, so that a streamed call really delivers a strict interior subset of the packets its rx() returned: some in
front were delivered by an earlier call, some behind are held back for the next, and the decoders that work on the
handle's device-resident soft values (rx_fec_decode_soft, rx_fec_decode_soft_rel, rx_ldpc_decode_soft) decode all of them
before ofdm.py picks.  All comparisons are equalities.

The reference, one work() per configuration, is held against the NumPy models first (coded_stream_cases.model_chain: the
hard paths from what an uncoded ofdm_demod returns on the same capture, the soft paths from the reference's own
last_soft) and must meet the non-triviality conditions of coded_stream_cases.nontrivial, which that file's docstring
shows the models to meet on the CPU; it is computed once and shared by the chunkings."""
import functools

import numpy as np
import pytest

import coded_stream_cases as cs
from ofdm_uhd_amd import benchmark_ofdm_rx, engine, fec, iqio, ofdm

pytestmark = pytest.mark.gpu

LISTS = ("last_fec", "last_ldpc", "last_rs", "last_rs_second")       # plain values per packet
ARRAYS = ("last_fec_rel", "last_soft")                               # one array per packet
FIELDS = LISTS + ARRAYS


def _demod(name=None, **kw):
    return ofdm.ofdm_demod(cs.options_of(), **dict(cs.CONFIGS[name]["rx"] if name else {}, **kw))


def _fields(dem):
    out = {k: list(getattr(dem, k)) for k in LISTS}
    out.update({k: [np.array(v) for v in getattr(dem, k)] for k in ARRAYS})
    return out


def _same_fields(got, want, tag):
    for k in LISTS:
        assert got[k] == want[k], (tag, k)
    for k in ARRAYS:
        assert len(got[k]) == len(want[k]), (tag, k, len(got[k]), len(want[k]))
        for i, (a, b) in enumerate(zip(got[k], want[k])):
            assert a.dtype == b.dtype and np.array_equal(a, b), (tag, k, i)


@functools.lru_cache(maxsize=None)
def reference(name):
    """One work() of ofdm_demod(**rx) on the configuration's capture, every field; trusted only after it equals the
    models and is not trivial."""
    rx = cs.CONFIGS[name]["rx"]
    pay, x = cs.capture(name)
    assert 4 * cs.span_of() <= len(x) <= cs.MAX_SAMPLES
    fired = []
    ref, plain = _demod(name, callback=lambda ok, p: fired.append((ok, p))), _demod()
    try:
        assert ref._stream_geometry()[1] == cs.span_of()
        pkts = ref.work(x)
        got = _fields(ref)
        pos = ref.engine().rx_packet_pos().astype(np.int64)
        n = (ref.n_packets, ref.n_ok)
        raw = plain.work(x)
        assert np.array_equal(plain.engine().rx_packet_pos().astype(np.int64), pos)
    finally:
        ref.engine().close()
        plain.engine().close()
    assert len(raw) == len(pkts) == len(pos) and fired == pkts and n == (len(pkts), sum(ok for ok, _ in pkts))
    if rx.get("soft"):
        assert [len(v) for v in got["last_soft"]] == [8 * len(p) for _, p in raw]
    else:
        assert got["last_soft"] == []
    want = cs.model_chain(rx, raw, got["last_soft"] if rx.get("soft") else None)
    c = cs.counts(rx, raw, dict(got, pkts=pkts))
    print("%s: %s" % (name, " ".join("%s %d" % kv for kv in c.items())))
    assert pkts == want["pkts"], name
    _same_fields(got, dict(want, last_soft=got["last_soft"]), name)
    cs.nontrivial(name, c)
    assert c == {k: cs.PRECHECK[name][k] for k in c}, name                # what the models gave on the CPU
    assert all(p in pay for ok, p in pkts if ok)                          # no ok for a payload that was not sent
    return dict(pkts=pkts, raw=raw, pos=pos, n=n, fields=got)


def _stream(dem, x, chunking):
    """feed() over the chunks, then flush(); per call what it returned, every field behind it and where the stream stood."""
    span = dem._stream_geometry()[1]
    pieces = [(x[a:b], chunking == "one") for a, b in cs.chunks(chunking, len(x))] + [(x[:0], True)]
    calls = []
    for piece, flush in pieces:
        base, carried, final = dem.stream_position()
        out = dem.feed(piece, flush=flush)
        total = base + carried + len(piece)
        horizon = total if flush else total - span
        call = dict(out=out, fields=_fields(dem), flush=flush, final_before=final, final_after=max(final, horizon),
                    ran=carried + len(piece) > 0 and horizon > final, engine_pos=None)
        if not flush:
            assert dem.stream_position()[2] == call["final_after"]
        if call["ran"]:
            call["engine_pos"] = dem.engine().rx_packet_pos().astype(np.int64) + base
        calls.append(call)
    return calls


def _concat(calls):
    out = {k: [] for k in FIELDS}
    for c in calls:
        for k in FIELDS:
            out[k] += c["fields"][k]
    return [p for c in calls for p in c["out"]], out


@pytest.mark.parametrize("chunking", cs.CHUNKINGS)
@pytest.mark.parametrize("name", cs.IDS)
def test_feed_equals_work_in_every_field(name, chunking):
    ref = reference(name)
    _, x = cs.capture(name)
    # the stitching itself, at these noise levels: an uncoded receiver streams what it returns in one call
    plain = _demod()
    try:
        got_raw, _ = _concat(_stream(plain, x, chunking))
    finally:
        plain.engine().close()
    assert got_raw == ref["raw"]
    fired = []
    dem = _demod(name, callback=lambda ok, p: fired.append((ok, p)))
    try:
        calls = _stream(dem, x, chunking)
        n = (dem.n_packets, dem.n_ok)
    finally:
        dem.engine().close()
    pkts, got = _concat(calls)
    assert [len(c["out"]) for c in calls if not c["ran"]] == [0] * sum(not c["ran"] for c in calls)
    live = [k for k in FIELDS if ref["fields"][k]]                        # the fields this configuration fills
    for i, c in enumerate(calls):
        for k in FIELDS:
            assert len(c["fields"][k]) == (len(c["out"]) if k in live else 0), (i, k)     # one entry per delivered packet
    assert pkts == ref["pkts"]
    assert fired == ref["pkts"]
    _same_fields(got, ref["fields"], (name, chunking))
    assert n == ref["n"]
    # the delivered packets are those of the call's rx() between the two horizons, where work() found them
    k, interior = 0, 0
    for c in calls:
        if not c["ran"]:
            continue
        pos = c["engine_pos"]
        now = (pos > c["final_before"]) & (pos <= c["final_after"])
        assert int(now.sum()) == len(c["out"]) and np.array_equal(pos[now], ref["pos"][k:k + len(c["out"])])
        k += len(c["out"])
        skipped, held = int((pos <= c["final_before"]).sum()), int((pos > c["final_after"]).sum())
        assert skipped + len(c["out"]) + held == len(pos)
        interior += bool(skipped and held and len(c["out"]))
    assert k == len(ref["pos"])
    before_flush = [c for c in calls if not c["flush"]]
    if chunking == "40000":
        assert sum(len(c["out"]) > 0 for c in before_flush) >= 3
        assert interior >= 1                                      # sel was a strict interior subset of the engine's list
    if chunking == "7000":
        idle = [c for c in before_flush if not c["out"]]
        assert idle and all(not c["fields"][k] for c in idle for k in FIELDS)
    if chunking == "one":
        assert calls[0]["out"] == ref["pkts"] and not calls[1]["out"] and not any(calls[1]["fields"][k] for k in FIELDS)


def test_decoding_on_the_handle_leaves_its_values_alone():
    """feed() and work() read the values before they decode, and a second decode of a call's values is legal: each of
    the three decoders that work on the handle, twice, on a capture of its own."""
    def rel(dec):
        return [(bool(d[0]), d[1], d[2], d[3].tobytes()) for d in dec]

    def plain(dec):
        return [(bool(d[0]),) + tuple(d[1:]) for d in dec]

    cases = (("fec-soft-rs", lambda e: plain(e.rx_fec_decode_soft())),
             ("fec34-soft", lambda e: rel(e.rx_fec_decode_soft_rel(fec.as_cfg(dict(rate="3/4"))))),
             ("ldpc-soft", lambda e: plain(e.rx_ldpc_decode_soft())))
    eng = engine.Engine(cs.options_of())
    try:
        eng.set_rx_soft(True)
        for name, decode in cases:
            _, x = cs.capture(name)
            pk = eng.rx(x)
            before = eng.rx_soft()
            first = decode(eng)
            between = eng.rx_soft()
            second = decode(eng)
            after = eng.rx_soft()
            assert len(pk) == len(first) == len(before) >= 20, name
            assert first == second, name
            assert any(d[0] for d in first) and sum(d[2] > 0 for d in first) >= 10, name           # there was something to decode
            for a, b, c in zip(before, between, after):
                assert np.array_equal(a, b) and np.array_equal(a, c), name
    finally:
        eng.close()


def test_quality_and_csi_follow_the_decoded_packets():
    name = "ldpc-soft"
    ref = reference(name)
    _, x = cs.capture(name)
    seen = {"one": [], "fed": []}
    one = _demod(name, quality_callback=lambda ok, p, q: seen["one"].append((ok, p, q.copy())), csi=True)
    fed = _demod(name, quality_callback=lambda ok, p, q: seen["fed"].append((ok, p, q.copy())), csi=True)
    try:
        assert one.work(x) == ref["pkts"]
        want_q, want_csi = one.last_quality.copy(), {k: v.copy() for k, v in one.last_csi.items()}
        recs, rows, delivering = [], {k: [] for k in want_csi}, 0
        for a, b in cs.chunks("40000", len(x)):
            out = fed.feed(x[a:b])
            delivering += bool(out)
            assert len(fed.last_quality) == len(out) and all(len(v) == len(out) for v in fed.last_csi.values())
            recs += list(fed.last_quality)
            for k in rows:
                rows[k].append(fed.last_csi[k].copy())
        out = fed.flush()
        recs += list(fed.last_quality)
        for k in rows:
            rows[k].append(fed.last_csi[k].copy())
    finally:
        one.engine().close()
        fed.engine().close()
    assert delivering >= 3
    for tag in ("one", "fed"):
        assert [(ok, p) for ok, p, _ in seen[tag]] == ref["pkts"]                   # the decoded verdicts and payloads
    assert len(recs) == len(want_q) == len(ref["pkts"])
    for f in ("flag", "first_symbol"):
        assert [int(r[f]) for r in recs] == [int(v) for v in want_q[f]], f
        assert [int(q[f]) for _, _, q in seen["fed"]] == [int(v) for v in want_q[f]], f
    assert [int(v) for v in want_q["flag"]] == ref["pos"].tolist()
    for k, v in want_csi.items():
        got = np.concatenate(rows[k])
        assert got.shape == v.shape and np.array_equal(got.view(np.uint32), v.view(np.uint32)), k


def test_command_line_chunked_equals_one_call(tmp_path):
    """benchmark_ofdm_rx --chunk-samples with the coded links' flags: the same file out, the same accounting."""
    for name, flags in (("ldpc-soft", ["--ldpc-soft"]), ("fec-soft-rs", ["--fec-soft", "--rs"])):
        ref = reference(name)
        _, x = cs.capture(name)
        iqf = str(tmp_path / (name + ".dat"))
        iqio.file_sink(iqf).write(np.array(x))
        want = benchmark_ofdm_rx.rx_accounting(verbose=False)
        for ok, p in ref["pkts"]:
            want.rx_callback(ok, p)
        res = []
        for tag, extra in (("one", []), ("chunked", ["--chunk-samples", "40000"])):
            out = str(tmp_path / ("%s.%s.txt" % (name, tag)))
            acct = benchmark_ofdm_rx.main(["-m", cs.MOD, "--from-file", iqf, "--to-file", out] + flags + extra)
            res.append(((acct.n_rcvd, acct.n_right), open(out, "rb").read()))
        assert res[0] == res[1], name
        assert res[0][0] == (want.n_rcvd, want.n_right) and want.n_right >= 10 and len(res[0][1]) > 0, name
