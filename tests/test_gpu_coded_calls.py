"""Every codec call of the coded links (the K = 7 code at rate 1/2 and punctured, its soft-output decoder, Reed-Solomon
with and without reliabilities, LDPC) on ONE handle.  They share one host-side skeleton (CodecStage, csrc/engine_codec.inc):
the staging buffers, the block table and the HIP-event pair of a call come from one base, and the Viterbi decoders share
one per-slice event vector.  A mistake there shows only when calls interleave; the per-codec files run each codec on a
handle of its own.  The last test is about the preamble the three ofdm_rx_*_decode_soft* calls share."""
import ctypes as C
import functools

import numpy as np
import pytest

import fec_cases as fc
import fec_rel_cases as fr
import ldpc_cases as lc
import punct_cases as pc
import rs_cases as rc
import rs_rel_cases as rr
from helpers import make_cfg
from ofdm_uhd_amd import _abi, engine, options

pytestmark = pytest.mark.gpu

# the empty block, the smallest, a generic one, and one past a codeword boundary of both block codes (223 + 4 info bytes:
# two RS codewords, three LDPC codewords)
SIZES = (0, 1, 100, 223)
R34 = dict(rate="3/4")
TIMERS = ("fec", "fec_punct", "rs", "rs_rel", "ldpc")


def _damage(block):
    """The block with two bytes inverted."""
    b = bytearray(block)
    for at in (len(b) // 3, (2 * len(b)) // 3):
        b[at] ^= 0xFF
    return bytes(b)


def _weak_values(block, sent):
    """+-40 per bit of a received block, +-3 over the bytes that differ from what was sent."""
    v = (40 * fc.hard_values(block).astype(np.int16)).reshape(-1, 8)
    wrong = np.frombuffer(block, np.uint8) != np.frombuffer(sent, np.uint8)
    v[wrong] = np.sign(v[wrong]) * 3
    return v.reshape(-1).astype(np.int8)


@functools.lru_cache(maxsize=None)
def model():
    """The inputs of every call and the models' results, computed once (no GPU)."""
    rng = np.random.default_rng(77)
    m = {}
    m["pay"] = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in SIZES]
    m["rs_encode"] = [rc.encode(p) for p in m["pay"]]
    m["fec_in"] = m["pay"] + m["rs_encode"]                       # the payloads, and the outer code's blocks (a concatenated link)
    m["fec_encode"] = [fc.encode(p, 16) for p in m["fec_in"]]
    m["fec_encode_34"] = [pc.encode(p, 16, "3/4") for p in m["pay"]]
    m["ldpc_encode"] = [lc.encode(p) for p in m["pay"]]
    m["d12"] = [_damage(b) for b in m["fec_encode"]]
    m["v34"] = [fc.hard_values(_damage(b)) for b in m["fec_encode_34"]]
    m["dl"] = [_damage(b) for b in m["ldpc_encode"]]
    m["vl"] = [lc.hard_values(b) for b in m["dl"]]
    m["drs"] = [_damage(b) for b in m["rs_encode"]]
    m["vrs"] = [_weak_values(d, b) for d, b in zip(m["drs"], m["rs_encode"])]
    m["fec_decode"] = [fc.decode(b, 16) for b in m["d12"]]
    m["fec_decode_soft_34"] = [pc.decode_values(v, 16, "3/4") for v in m["v34"]]
    m["fec_decode_rel"] = [fr.decode(b, 16) for b in m["d12"]]
    m["ldpc_decode"] = [lc.decode(b) for b in m["dl"]]
    m["ldpc_decode_soft"] = [lc.decode_values(v) for v in m["vl"]]
    m["rs_decode"] = [rc.decode(b) for b in m["drs"]]
    m["rs_rel_from_soft"] = [rr.rel_from_values(v) for v in m["vrs"]]
    m["rs_decode_rel_soft"] = [rr.decode(b, q) for b, q in zip(m["drs"], m["rs_rel_from_soft"])]
    # what the inner decoder made of the outer code's blocks, with its reliabilities
    m["rs_from_fec"] = [d[1] for d in m["fec_decode_rel"][len(SIZES):]]
    m["rel_from_fec"] = [d[3] for d in m["fec_decode_rel"][len(SIZES):]]
    m["rs_decode_rel_fec"] = [rr.decode(b, q) for b, q in zip(m["rs_from_fec"], m["rel_from_fec"])]
    return m


# (name, the call, the timers it sets, the timers it leaves refusing), in the order of a round; m is model().  The timers
# are what the test_last_ms tests of the per-codec files document for the call.
CALLS = [
    ("rs_encode", lambda e, m: e.rs_encode(m["pay"]), ("rs",), ()),
    ("fec_encode", lambda e, m: e.fec_encode(m["fec_in"]), ("fec",), ("fec_punct",)),
    ("fec_encode_34", lambda e, m: e.fec_encode(m["pay"], R34), ("fec_punct",), ()),
    ("ldpc_encode", lambda e, m: e.ldpc_encode(m["pay"]), ("ldpc",), ()),
    ("fec_decode", lambda e, m: e.fec_decode(m["d12"]), ("fec",), ("fec_punct",)),
    ("fec_decode_soft_34", lambda e, m: e.fec_decode_soft(m["v34"], R34), ("fec", "fec_punct"), ()),
    ("fec_decode_rel", lambda e, m: e.fec_decode_rel(m["d12"]), ("fec",), ("fec_punct",)),
    ("ldpc_decode", lambda e, m: e.ldpc_decode(m["dl"]), ("ldpc",), ()),
    ("ldpc_decode_soft", lambda e, m: e.ldpc_decode_soft(m["vl"]), ("ldpc",), ()),
    ("rs_decode", lambda e, m: e.rs_decode(m["drs"]), ("rs",), ()),
    ("rs_rel_from_soft", lambda e, m: e.rs_rel_from_soft(m["vrs"]), ("rs_rel",), ()),
    ("rs_decode_rel_fec", lambda e, m: e.rs_decode_rel(m["rs_from_fec"], m["rel_from_fec"]), ("rs",), ()),
    ("rs_decode_rel_soft", lambda e, m: e.rs_decode_rel(m["drs"], m["rs_rel_from_soft"]), ("rs",), ()),
]


def same(a, b):
    """Two results, field by field: lists and tuples element by element, arrays by dtype and content, ok as a truth
    value (the models say 0 / 1)."""
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.dtype == b.dtype and np.array_equal(a, b)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return type(a) in (bool, int, bytes) and a == b


def run(e, name, call, timed, refused):
    got = call(e, model())
    for t in timed:
        assert getattr(e, t + "_last_ms")() > 0.0, (name, t)
    for t in refused:
        with pytest.raises(ValueError):
            getattr(e, t + "_last_ms")()
    return got


def _engine():
    e = engine.Engine(options.default_options(modulation="qpsk"))
    e.prof_enable(True)
    return e


@functools.lru_cache(maxsize=None)
def rounds():
    """Two rounds of every call on one handle."""
    e = _engine()
    try:
        return tuple({name: run(e, name, call, timed, refused) for name, call, timed, refused in CALLS} for _ in range(2))
    finally:
        e.close()


def test_the_cases_are_what_they_are_meant_to_be():
    m = model()
    assert [len(p) for p in m["pay"]] == list(SIZES)
    assert [rc.words(n + 4) for n in SIZES] == [1, 1, 1, 2] and [lc.codewords(n + 4) for n in SIZES] == [1, 1, 2, 3]
    assert all(a != b and len(a) == len(b) for k, d in (("fec_encode", "d12"), ("ldpc_encode", "dl"), ("rs_encode", "drs"))
               for a, b in zip(m[k], m[d]))
    # the damage is within the outer code's reach and leaves the inner codes something to do
    assert [r[:2] for r in m["rs_decode"]] == [(1, p) for p in m["pay"]] and all(r[2] == 2 for r in m["rs_decode"])
    assert any(r[2] > 0 for r in m["fec_decode"]) and any(r[2] > 0 for r in m["ldpc_decode"])
    assert all(len(q) == len(b) for q, b in zip(m["rel_from_fec"], m["rs_from_fec"]))


def test_round_two_equals_round_one():
    one, two = rounds()
    assert list(one) == list(two) == [c[0] for c in CALLS]
    for name in one:
        assert same(one[name], two[name]), name


@pytest.mark.parametrize("name", [c[0] for c in CALLS])
def test_a_call_among_the_others_equals_the_call_alone_and_the_model(name):
    m = model()
    among = rounds()[0][name]
    e = _engine()
    try:
        for t in TIMERS:
            with pytest.raises(ValueError):
                getattr(e, t + "_last_ms")()            # a fresh handle has timed nothing
        alone = run(e, *[c for c in CALLS if c[0] == name][0])
    finally:
        e.close()
    assert same(among, alone), name
    assert len(among) == len(m[name])
    for i, (g, w) in enumerate(zip(among, m[name])):
        w = w if isinstance(w, (bytes, np.ndarray)) else (bool(w[0]),) + tuple(w[1:])
        assert same(g, w), (name, i)


# ---- the receiver's own values: ofdm_rx_fec_decode_soft, ofdm_rx_fec_decode_soft_rel, ofdm_rx_ldpc_decode_soft ------------
def test_the_three_rx_decode_calls_through_the_abi():
    """One burst of two short packets at the smallest geometry of test_gpu_soft.GEOMS: a block of the K = 7 code, which
    is no LDPC block, and an LDPC block, which is no block of the K = 7 code."""
    cfg = make_cfg("bpsk", 64, 48, 16)
    N, L = 64, 80
    pkts = [fc.encode(b"abc"), lc.encode(b"abc")]
    assert [len(p) for p in pkts] == [16, 103] and lc.is_block(103) and not lc.is_block(16) and not fc.is_block(103)
    lib = _abi.load()
    u64p, u32p, vp = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.c_void_p
    SLOTS = 8
    out, rel = np.zeros(4096, np.uint8), np.zeros(4096, np.uint8)
    poff, ok, corr = np.zeros(SLOTS + 1, np.uint64), np.zeros(SLOTS, np.uint8), np.zeros(SLOTS, np.uint32)
    iters, failed = np.zeros(SLOTS, np.uint8), np.zeros(SLOTS, np.uint32)
    n = C.c_int(-1)
    head = (out.ctypes.data_as(vp), len(out), poff.ctypes.data_as(u64p), ok.ctypes.data_as(vp), corr.ctypes.data_as(u32p))

    def results(*cols):
        return [(bool(ok[i]), out[int(poff[i]):int(poff[i + 1])].tobytes(), int(corr[i])) + tuple(c(i) for c in cols) for i in range(n.value)]

    e = engine.Engine(cfg=cfg)
    try:
        h = e._h
        three = [
            (lambda k: lib.ofdm_rx_fec_decode_soft(h, None, *head, k, C.byref(n)),
             lambda: results(), lambda v: fc.decode_values(v, 16)),
            (lambda k: lib.ofdm_rx_fec_decode_soft_rel(h, None, *head, rel.ctypes.data_as(vp), len(rel), k, C.byref(n)),
             lambda: results(lambda i: rel[int(poff[i]):int(poff[i + 1])].copy()), lambda v: fr.decode_values(v, 16)),
            (lambda k: lib.ofdm_rx_ldpc_decode_soft(h, None, *head, iters.ctypes.data_as(vp), failed.ctypes.data_as(u32p), k, C.byref(n)),
             lambda: results(lambda i: int(iters[i]), lambda i: int(failed[i])), lambda v: lc.decode_values(v)),
        ]
        x = np.concatenate([np.zeros(2 * N, np.complex64), e.tx(pkts), np.zeros(L + 2 * N, np.complex64)])
        e.set_rx_soft(True)
        assert e.rx(x) == [(True, p) for p in pkts]
        vals = e.rx_soft()
        assert [len(v) for v in vals] == [8 * 16, 8 * 103]
        for call, got, want in three:
            n.value = -1
            assert call(1) == _abi.OFDM_E_CAPACITY and n.value == 2         # one slot for two packets: refused, *n says how many
            n.value = -1
            assert call(2) == _abi.OFDM_OK and n.value == 2
            g, w = got(), [want(v) for v in vals]
            assert same(g, [(bool(r[0]),) + tuple(r[1:]) for r in w]), (g, w)
        assert [bool(fc.decode_values(v, 16)[0]) for v in vals] == [True, False]
        assert [bool(lc.decode_values(v)[0]) for v in vals] == [False, True]
        e.set_rx_soft(None)
        assert e.rx(x) == [(True, p) for p in pkts]
        for call, _, _ in three:
            assert call(2) == _abi.OFDM_E_INVAL                              # the last ofdm_rx ran without soft values
    finally:
        e.close()
