"""Decoding with reliabilities on the GPU (csrc/rs.h: k_rs_decode_rel, k_rs_rel_soft).  Everything is integer arithmetic,
so every result is compared with the NumPy model of tests/rs_rel_cases.py by equality, in every field: damage on the line
2 e + f = 32 and one past it in every geometry, the first pass's precedence, the threshold rule, batches, every alignment,
refusals, the device-pointer chain, the timing accessors, the reliabilities from soft values, and the layer on a link.

Sizes: the smallest that reach every geometry: n = 0 (k = 4, a 36-symbol codeword), 219 (one full 255-symbol codeword),
220 (W = 2, uneven split), 1780 (W = 8, all halves busy), 1781 (W = 9, two passes), 3564 (W = 16).

The issue's list of damage asks for (f, e) = (1, 15) among cases "built so that the first pass fails (e + f >= 17)"; one
erased and fifteen other wrong symbols are 16 wrong symbols, which the first pass corrects.  The case is kept as listed
and its result is the first pass's (second = 0), as the definition says.

The issue also expects (32, 1) to "stay failed and unchanged".  No decoder can do that and decode (32, 0) as well: 32
erased symbols use all 32 parity symbols, so EVERY received word agrees, outside J, with exactly one codeword (e = 0,
2 * 0 + 32 <= 32), which by the definition is the output.  With one more wrong symbol outside J that codeword is not the
one sent; nothing is left to notice it but the CRC-32 inside the block.  The case is kept and asserts what the definition
gives: equality with the model, second = 1, failed = 0, a payload that is not the one sent and ok = 0.  (This is why the
default M is 28, not 32.)

CPU pre-check of the impaired link (rs_rel_cases.link_on_the_cpu: RS blocks straight on the oracle's transmitter, no
inner code, the float64 channel model of multipath_cases, the oracle's receiver with its taps, the soft model at scale
32, reliabilities by the rule, the RS models without and with them at M = 28): 16-QAM, N 512 / occ 200 / CP 128, the
packets and paths of soft_cases.  The grid, its counts and the points taken are listed at LINK_CASES below."""
import ctypes as C
import functools

import numpy as np
import pytest

import rs_cases as rc
import rs_rel_cases as rr
import soft_cases as sc
from ofdm_uhd_amd import _abi, engine, ofdm, options, rs

pytestmark = pytest.mark.gpu

SIZES = (0, 219, 220, 1780, 1781, 3564)
LINE = ((32, 0), (30, 1), (16, 8), (2, 15), (31, 0), (1, 15))       # 2 e + f = 32, and 31
PAST = ((17, 8), (32, 1))                                           # 2 e + f = 33, 34


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(options.default_options(modulation="qpsk"))
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def payload(n):
    return np.random.default_rng(1000 + n).integers(0, 256, n, dtype=np.uint8).tobytes()


@functools.lru_cache(maxsize=None)
def block(n):
    return rc.encode(payload(n))


_MODEL = {}


def model(b, rel, M):
    """The model's answer, computed once per distinct input."""
    key = (bytes(b), None if rel is None else bytes(np.asarray(rel, np.uint8)), M)
    if key not in _MODEL:
        _MODEL[key] = rr.decode(b, rel, M)
    return _MODEL[key]


def check(eng, batch, rels, M=rr.DEFAULT_M):
    got = [(int(ok), p, c, f, s) for ok, p, c, f, s in eng.rs_decode_rel(batch, rels, dict(max_erasures=M))]
    want = [model(b, r, M) for b, r in zip(batch, rels)]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, len(batch[i]), g[0], g[2:], w[0], w[2:])
    return want


def pins(f):
    """Erased symbols that must be there: the first and the last position, and both sides of the info / parity boundary."""
    return (0, -1, -33, -32)[:f] if f >= 4 else (0, -1)[:f]


# ---- 1. damage on the line 2 e + f = 32 and one past it ------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_damage_on_the_line_and_past_it(eng, n):
    b, k = block(n), n + 4
    W = rc.words(k)
    rng = np.random.default_rng(n)
    batch, rels, kinds = [], [], []
    for j, (f, e) in enumerate(LINE + PAST):
        w = (j * 5 + W - 1) % W                                             # the last codeword first: the shorter ones, the second pass of W = 9
        good = 3 if f >= 16 else 0                                          # erased, but already correct
        d, rel, J = rr.spoil(b, w, f, e, rng, erase_good=good, pin=pins(f))
        assert {0, len(rc.positions(k, w)) - 1}.issubset(set(J.tolist())) or f < 2
        batch.append(d)
        rels.append(rel)
        kinds.append((f, e, good))
    want = check(eng, batch, rels, 32)                                      # (M = 32: f = 32 is erased whole)
    for (f, e, good), got in zip(kinds, want):
        if (f, e) == (17, 8):
            assert got[0] == 0 and got[2:] == (0, 1, 0), (f, e, got[2:])    # failed, unchanged
        elif (f, e) == (32, 1):
            assert got[0] == 0 and (got[1] != payload(n) or n == 0) and got[3:] == (0, 1), (f, e, got[2:])      # see the docstring
        elif (f, e) == (1, 15):
            assert got == (1, payload(n), 16, 0, 0)                         # 16 wrong symbols: the first pass's
        else:
            assert got == (1, payload(n), f - good + e, 0, 1), (f, e, got[2:])


def test_20_wrong_bytes_of_reliability_0_come_back(eng):
    """Fails before this feature: that codeword is `failed`."""
    for n in (219, 1780):
        b = block(n)
        rng = np.random.default_rng(20)
        d, rel, _ = rr.spoil(b, 0, 20, 0, rng)
        assert rc.decode(d)[2:] == (0, 1)                                   # errors only: one codeword fails
        got = eng.rs_decode_rel([d], [rel])                                 # the default: at most 28 erasures
        assert got == [(True, payload(n), 20, 0, 1)] and model(d, rel, 28) == (1, payload(n), 20, 0, 1)


# ---- 2. the first pass decides where it decodes ----------------------------------------------------------------------------
def adversarial(sent, got):
    """Reliability 0 on every correct byte, 200 on the wrong ones."""
    a, b = np.frombuffer(sent, np.uint8), np.frombuffer(got, np.uint8)
    return np.where(a == b, 0, 200).astype(np.uint8)


def test_first_pass_is_sovereign(eng):
    rng = np.random.default_rng(3)
    sent, batch = [], []
    for n in (3, 219, 443, 1780):
        b = rc.encode(payload(n))
        for percent in (1, 10):
            where = np.flatnonzero(rng.integers(0, 100, len(b)) < percent)
            sent.append(b)
            batch.append(rc.damage(b, where, rng))
        sent.append(b)
        batch.append(rc.errors_per_codeword(b, 16, rng))
        m, _ = rc.miscorrection(b, w=0, seed=n)
        sent.append(b)
        batch.append(m)
    b = rc.encode(payload(443))                                             # k = 447, W = 3: bursts
    for s in (0, 100, 447, len(b) - 46):
        sent.append(b)
        batch.append(rc.damage(b, np.arange(s, s + 46), xor=0xFF))
    rels = [adversarial(s, g) for s, g in zip(sent, batch)]
    want = check(eng, batch, rels)
    today = eng.rs_decode(batch)
    n_first = 0
    for w, t in zip(want, today):
        if w[4] == 0:                                                       # (a 36-symbol word may have few enough correct bytes to erase)
            assert (bool(w[0]),) + w[1:4] == t
            n_first += 1
    assert n_first >= len(batch) - 2 and any(t[2] for t in today) and any(t[3] for t in today)


def test_no_reliabilities_no_erasures_and_all_255_are_rs_decode(eng):
    rng = np.random.default_rng(4)
    batch = []
    for n in SIZES:
        b = block(n)
        batch += [b, rc.errors_per_codeword(b, 9, rng), rc.errors_per_codeword(b, 17, rng), rc.damage(b, rng.choice(len(b), 30, False), rng)]
    batch += [bytes(35), bytes(256)]
    today = eng.rs_decode(batch)
    zeros = [np.zeros(len(b), np.uint8) for b in batch]
    assert eng.rs_decode_rel(batch, None) == [t + (0,) for t in today]
    assert eng.rs_decode_rel(batch, zeros, dict(max_erasures=0)) == [t + (0,) for t in today]
    for M in (28, 32):
        assert eng.rs_decode_rel(batch, [np.full(len(b), 255, np.uint8) for b in batch], dict(max_erasures=M)) == [t + (0,) for t in today]
    assert any(t[3] for t in today) and any(t[2] for t in today)


# ---- 3. the threshold ----------------------------------------------------------------------------------------------------
def cw_case(n, w, wrong, rel_of, rng, default=200):
    """Codeword w of block(n): the symbols ``wrong`` changed, reliabilities ``rel_of`` {symbol: value}, others ``default``."""
    b, k = block(n), n + 4
    pos = rc.positions(k, w)
    d = rc.damage(b, pos[np.asarray(wrong, np.int64)], rng)
    rel = np.full(len(b), default, np.uint8)
    for s, v in rel_of.items():
        rel[pos[s]] = v
    return d, rel


def test_threshold_rule(eng):
    rng = np.random.default_rng(5)
    sym = [int(s) for s in rng.permutation(255)]
    z28, z29, one5 = sym[:28], sym[:29], sym[29:34]
    cases = {
        # 28 at reliability 0 and 5 at 1: tau* = 0, f = 28; two of the five are wrong: 2 * 2 + 28 = 32
        "tie across the cap": (cw_case(219, 0, z28 + one5[:2], {**{s: 0 for s in z28}, **{s: 1 for s in one5}}, rng), 28, (1, 30, 0, 1)),
        # 29 at reliability 0: c(0) > M, no second pass
        "c(0) > M": (cw_case(219, 0, z29[:20], {s: 0 for s in z29}, rng), 28, (0, 0, 1, 0)),
        # 24 at 0 and 5 at 1: c(1) = 29 > 28, so tau* = 0 and f = 24; the wrong ones among the five are errors: 2 * 4 + 24 = 32
        "tie below the cap": (cw_case(219, 0, sym[:24] + one5[:4], {**{s: 0 for s in sym[:24]}, **{s: 1 for s in one5}}, rng), 28, (1, 28, 0, 1)),
        # the same with all five wrong: 2 * 5 + 24 = 34
        "tie below the cap, past the line": (cw_case(219, 0, sym[:24] + one5, {**{s: 0 for s in sym[:24]}, **{s: 1 for s in one5}}, rng), 28,
                                             (0, 0, 1, 0)),
        # tau* = 254: everything that is not 255 is erased
        "tau* = 254": (cw_case(219, 0, sym[:25], {s: 254 for s in sym[:25]}, rng, default=255), 28, (1, 25, 0, 1)),
        # 255 is never erased, even at M = 32: 20 wrong, none to erase
        "255 never": (cw_case(219, 0, sym[:20], {}, rng, default=255), 32, (0, 0, 1, 0)),
        # ten of the 20 wrong at 0, ten at 255: f = 10, e = 10, 30 <= 32
        "255 as errors": (cw_case(219, 0, sym[:20], {s: 0 for s in sym[:10]}, rng, default=255), 32, (1, 20, 0, 1)),
        # nothing to erase at all: c(tau*) = 0 needs every reliability at 255 (above)
    }
    for name, ((d, rel), M, (ok, corr, fail, sec)) in cases.items():
        want = check(eng, [d], [rel], M)[0]
        assert (want[0],) + want[2:] == (ok, corr, fail, sec), (name, want[0], want[2:])
        assert rr.threshold(rel[rc.positions(223, 0)], M) == {"tau* = 254": 254, "255 as errors": 254, "255 never": None, "c(0) > M": None}.get(name, 0), name


def test_second_counts_per_block(eng):
    """W = 2: one codeword clean and one needing the second pass; and both needing it."""
    rng = np.random.default_rng(6)
    b = block(220)
    one0, rel0, _ = rr.spoil(b, 0, 22, 1, rng)
    one1, rel1, _ = rr.spoil(b, 1, 22, 1, rng)
    both = np.frombuffer(one0, np.uint8) ^ np.frombuffer(one1, np.uint8) ^ np.frombuffer(b, np.uint8)
    want = check(eng, [one0, one1, both.tobytes(), b], [rel0, rel1, np.minimum(rel0, rel1), rel0])
    assert [w[2:] for w in want] == [(23, 0, 1), (23, 0, 1), (46, 0, 2), (0, 0, 0)] and all(w[:2] == (1, payload(220)) for w in want)


# ---- 4. batches and alignment --------------------------------------------------------------------------------------------
def test_a_few_hundred_mixed_blocks(eng):
    rng = np.random.default_rng(7)
    kinds = []
    for n in SIZES + (3, 443):
        b = block(n) if n in SIZES else rc.encode(payload(n))
        W = rc.words(n + 4)
        kinds.append((b, np.full(len(b), 9, np.uint8)))
        kinds.append(rr.spoil(b, W - 1, 20, 2, rng)[:2])
        kinds.append(rr.spoil(b, 0, 26, 4, rng)[:2])                         # past the line
        d = rc.errors_per_codeword(b, 17, rng)
        kinds.append((d, rng.integers(0, 256, len(b), dtype=np.uint8)))     # random reliabilities on a failing block
    for m in (0, 35, 256, 4081):
        kinds.append((bytes(m), np.zeros(m, np.uint8)))                     # no blocks
    order = rng.integers(0, len(kinds), 320)
    want = check(eng, [kinds[i][0] for i in order], [kinds[i][1] for i in order])
    assert sum(w[4] for w in want) > 50 and sum(w[3] for w in want) > 50 and sum(1 for w in want if w == (0, b"", 0, 0, 0)) > 10


def test_every_alignment_of_block_and_reliabilities(eng):
    rng = np.random.default_rng(8)
    d, rel, _ = rr.spoil(block(220), 1, 24, 3, rng)
    want = model(d, rel, 28)
    assert want[2:] == (27, 0, 1)
    L = len(d)
    offs = np.array([r * 320 + r for r in range(16)], np.uint64)            # every residue mod 16
    roffs = np.array([r * 320 + (7 * r + 3) % 16 for r in range(16)], np.uint64)
    blob = np.full(16 * 320 + 64, 0xEE, np.uint8)
    rblob = np.full(16 * 320 + 64, 0, np.uint8)                             # (0 around the blocks: reading past an edge would erase)
    for r in range(16):
        blob[int(offs[r]):int(offs[r]) + L] = np.frombuffer(d, np.uint8)
        rblob[int(roffs[r]):int(roffs[r]) + L] = rel
    lens = np.full(16, L, np.uint32)
    out = np.full(16 * 220 + 32, 0xEE, np.uint8)
    poff, ok, corr, fail, sec = eng._rs_decode_rel(rs.rs_cfg(), engine._ptr(blob), offs, lens, engine._ptr(rblob), roffs, engine._ptr(out), 16 * 220)
    assert poff.tolist() == [220 * i for i in range(17)] and (out[16 * 220:] == 0xEE).all()
    for r in range(16):
        assert (int(ok[r]), out[220 * r:220 * r + 220].tobytes(), int(corr[r]), int(fail[r]), int(sec[r])) == want, r


# ---- 5. refusals, timing ---------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable(eng):
    lib, h = eng._lib, eng._h
    u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
    blob, offs, lens = engine.pack_payloads([rc.encode(b"abc"), rc.encode(b"defgh")])
    relb = np.full(len(blob), 7, np.uint8)
    pay = np.zeros(16, np.uint8)
    poff = np.full(3, 77, np.uint64)
    ok, corr, fail, sec = np.zeros(2, np.uint8), np.zeros(2, np.uint32), np.zeros(2, np.uint32), np.full(2, 9, np.uint32)
    cfg = rs.rs_cfg()
    args = [h, C.byref(cfg), blob.ctypes.data, offs.ctypes.data_as(u64p), lens.ctypes.data_as(u32p), 2, relb.ctypes.data, None,
            pay.ctypes.data, 16, poff.ctypes.data_as(u64p), ok.ctypes.data, corr.ctypes.data_as(u32p), fail.ctypes.data_as(u32p),
            sec.ctypes.data_as(u32p)]
    for null in (2, 3, 4, 8, 10, 11, 12, 13):
        a = list(args)
        a[null] = None
        assert lib.ofdm_rs_decode_rel(*a) == _abi.OFDM_E_INVAL, null
    for bad in (_abi.ofdm_rs_rel_cfg(struct_size=28, max_erasures=28), _abi.ofdm_rs_rel_cfg(struct_size=32, max_erasures=33),
                _abi.ofdm_rs_rel_cfg(struct_size=32, max_erasures=28, reserved=(0, 0, 0, 0, 0, 1))):
        a = list(args)
        a[1] = C.byref(bad)
        assert lib.ofdm_rs_decode_rel(*a) == _abi.OFDM_E_INVAL
    with pytest.raises(ValueError):
        rs.rs_cfg(33)
    a = list(args)
    a[9] = 7
    assert lib.ofdm_rs_decode_rel(*a) == _abi.OFDM_E_CAPACITY and poff.tolist() == [0, 3, 8]
    for a in (list(args), args[:1] + [None] + args[2:], args[:14] + [None]):                 # cfg == NULL: M = 28; second may be NULL
        pay[:] = 0
        assert lib.ofdm_rs_decode_rel(*a) == _abi.OFDM_OK
        assert pay[:8].tobytes() == b"abcdefgh" and ok.tolist() == [1, 1] and corr.tolist() == [0, 0] and fail.tolist() == [0, 0]
    assert sec.tolist() == [0, 0]
    # reliabilities from values
    vals = np.zeros(8 * 5, np.int8)
    voff, vlen = np.array([0, 16], np.uint64), np.array([2, 3], np.uint32)
    rel = np.full(8, 0xEE, np.uint8)
    roff = np.full(3, 77, np.uint64)
    rargs = [h, vals.ctypes.data, voff.ctypes.data_as(u64p), vlen.ctypes.data_as(u32p), 2, rel.ctypes.data, 5, roff.ctypes.data_as(u64p)]
    for null in (1, 2, 3, 5, 7):
        a = list(rargs)
        a[null] = None
        assert lib.ofdm_rs_rel_from_soft(*a) == _abi.OFDM_E_INVAL, null
    a = list(rargs)
    a[6] = 4
    assert lib.ofdm_rs_rel_from_soft(*a) == _abi.OFDM_E_CAPACITY and roff.tolist() == [0, 2, 5]
    a = list(rargs)
    a[2] = np.array([0, 12], np.uint64).ctypes.data_as(u64p)
    assert lib.ofdm_rs_rel_from_soft(*a) == _abi.OFDM_E_INVAL
    assert lib.ofdm_rs_rel_from_soft(*rargs) == _abi.OFDM_OK and rel.tolist() == [0] * 5 + [0xEE] * 3
    assert lib.ofdm_rs_decode_rel(None, *args[1:]) == _abi.OFDM_E_INVAL and lib.ofdm_rs_rel_from_soft(None, *rargs[1:]) == _abi.OFDM_E_INVAL
    rng = np.random.default_rng(9)
    check(eng, *zip(*[rr.spoil(block(219), 0, 20, 3, rng)[:2], (block(0), np.zeros(36, np.uint8))]))


def test_both_last_ms():
    e = engine.Engine(options.default_options(modulation="qpsk"))
    try:
        e.prof_enable(True)
        with pytest.raises(ValueError):
            e.rs_rel_last_ms()
        rel = e.rs_rel_from_soft([np.zeros(8 * 36, np.int8)])
        assert e.rs_rel_last_ms() > 0.0
        with pytest.raises(ValueError):
            e.rs_last_ms()                              # no decode yet
        e.rs_decode_rel([block(0)], rel)
        assert e.rs_last_ms() > 0.0 and e.rs_rel_last_ms() > 0.0
        e.rs_decode_rel([bytes(35)], [np.zeros(35, np.uint8)])      # no block: nothing launched
        with pytest.raises(ValueError):
            e.rs_last_ms()
        e.rs_rel_from_soft([])
        with pytest.raises(ValueError):
            e.rs_rel_last_ms()
        assert len(e.prof()) == _abi.K_COUNT            # the kernel table is what it was
    finally:
        e.close()


# ---- 6. reliabilities from soft values -------------------------------------------------------------------------------------
def test_rel_from_soft_equals_the_model(eng):
    rng = np.random.default_rng(10)
    lens = [1, 3, 4, 5, 31, 32, 33, 0, 2, 36, 255, 1190, 7, 4080, 6]        # bytes; the running sum visits every alignment
    vals = []
    for m in lens:
        v = rng.integers(-128, 128, 8 * m).astype(np.int8)
        v[rng.integers(0, 100, 8 * m) < 3] = -128
        v[rng.integers(0, 100, 8 * m) < 3] = 0
        if m >= 2:
            v[:8] = [-128, 127, -128, 127, -127, 127, -128, -128]           # 127, with -128 among the values
            v[-8:] = [5, -4, 3, -128, 9, 100, -100, 7]
        vals.append(v)
    got = eng.rs_rel_from_soft(vals)
    for g, v, m in zip(got, vals, lens):
        want = rr.rel_from_values(v)
        assert g.dtype == np.uint8 and len(g) == m and np.array_equal(g, want) and np.array_equal(rs.rel_from_values(v), want), m
    assert got[5][0] == 127 and got[5][-1] == 3 and max(int(g.max()) for g in got if len(g)) <= 127
    assert eng.rs_rel_from_soft([]) == []
    with pytest.raises(ValueError):
        eng.rs_rel_from_soft([np.zeros(7, np.int8)])


# ---- 7. device pointers ------------------------------------------------------------------------------------------------------
def test_the_device_chain_from_the_receiver():
    """rx_device -> rx_soft_device -> rs_rel_from_soft_device -> rs_decode_rel_device: no host copy of values or
    reliabilities; guards behind every buffer stay what they were."""
    torch = pytest.importorskip("torch")
    from ofdm_uhd_amd import config
    N, CP = 64, 16
    opt = options.default_options(modulation="qpsk", fft_length=N, occupied_tones=48, cp_length=CP)
    rng = np.random.default_rng(11)
    pay = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (59, 180, 1, 0)]
    mod = ofdm.ofdm_mod(opt, pad_for_usrp=False, rs=True)
    dev = engine.Engine(cfg=config.make_cfg(opt, device_ptrs=True))
    try:
        for p in pay:
            mod.send_pkt(p)
        x = np.concatenate([np.zeros(2 * N, np.complex64), mod.flush(), np.zeros(N + CP, np.complex64)])
        dev.set_rx_soft(True)
        xd = torch.from_numpy(x.view(np.float32).copy()).cuda()
        cap = 4096
        blk = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        npk, off, ln, ok = dev.rx_device(xd.data_ptr(), len(x), blk.data_ptr(), cap, 16)
        assert npk == len(pay) and ln.tolist() == [rc.coded_len(len(p)) for p in pay]
        total = int(ln.astype(np.int64).sum())
        vd = torch.full((8 * total + 64,), 99, dtype=torch.int8, device="cuda")
        voff = dev.rx_soft_device(vd.data_ptr(), 8 * total)
        rd = torch.full((total + 64,), 0xEE, dtype=torch.uint8, device="cuda")
        ln32 = ln.astype(np.uint32)
        roff = dev.rs_rel_from_soft_device(vd.data_ptr(), voff[:npk].copy(), ln32, rd.data_ptr(), total)
        v, r = vd.cpu().numpy(), rd.cpu().numpy()
        assert roff.tolist() == np.concatenate([[0], np.cumsum(ln)]).tolist() and (r[total:] == 0xEE).all()
        assert np.array_equal(r[:total], rr.rel_from_values(v[:8 * total])) and int(r[:total].min()) > 0
        with pytest.raises(engine.EngineError):
            dev.rs_rel_from_soft_device(vd.data_ptr(), voff[:npk].copy(), ln32, rd.data_ptr(), total - 1)
        # damage on the device: 20 bytes of packet 1 wrong, their reliabilities 0
        b = blk.cpu().numpy()
        at = int(off[1]) + np.arange(20) * 3
        b[at] ^= 0x5A
        r[int(roff[1]) + np.arange(20) * 3] = 0
        blk.copy_(torch.from_numpy(b))
        rd.copy_(torch.from_numpy(r))
        n_pay = sum(len(p) for p in pay)
        out = torch.full((n_pay + 64,), 0xEE, dtype=torch.uint8, device="cuda")
        o64 = off.astype(np.uint64)
        poff, dok, corr, fail, sec = dev.rs_decode_rel_device(blk.data_ptr(), o64[:npk].copy(), ln32, rd.data_ptr(), roff[:npk].copy(),
                                                              out.data_ptr(), n_pay)
        o = out.cpu().numpy()
        got = [(int(dok[i]), o[int(poff[i]):int(poff[i + 1])].tobytes(), int(corr[i]), int(fail[i]), int(sec[i])) for i in range(npk)]
        want = [rr.decode(b[int(off[i]):int(off[i]) + int(ln[i])].tobytes(), r[int(roff[i]):int(roff[i + 1])], 28) for i in range(npk)]
        assert got == want == [(1, pay[0], 0, 0, 0), (1, pay[1], 20, 0, 1), (1, pay[2], 0, 0, 0), (1, pay[3], 0, 0, 0)]
        assert (o[n_pay:] == 0xEE).all()
        with pytest.raises(engine.EngineError):
            dev.rs_decode_rel_device(blk.data_ptr(), o64[:npk].copy(), ln32, rd.data_ptr(), roff[:npk].copy(), out.data_ptr(), n_pay - 1)
        # without reliabilities: rs_decode's result
        assert [x.tolist() for x in dev.rs_decode_rel_device(blk.data_ptr(), o64[:npk].copy(), ln32, None, None, out.data_ptr(), n_pay)[1:]] == \
            [x.tolist() for x in dev.rs_decode_device(blk.data_ptr(), o64[:npk].copy(), ln32, out.data_ptr(), n_pay)[1:]] + [[0] * npk]
    finally:
        mod.engine().close()
        dev.close()


# ---- 8. on a link ------------------------------------------------------------------------------------------------------------
def test_clean_loopback_and_the_arguments():
    N, CP = 64, 16
    opt = options.default_options(modulation="qpsk", fft_length=N, occupied_tones=48, cp_length=CP)
    rng = np.random.default_rng(147)
    pay = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (59, 180, 1, 148, 0)]
    for bad in (dict(rs=dict(erasures=True)), dict(rs=dict(erasures=True), soft=True, fec=True), dict(rs=dict(max_erasures=3), soft=True),
                dict(rs=dict(erasures=True, max_erasures=33), soft=True)):
        with pytest.raises(ValueError):
            ofdm.ofdm_demod(opt, **bad)
    mod = ofdm.ofdm_mod(opt, pad_for_usrp=False, rs=True)
    seen = []
    dem = ofdm.ofdm_demod(opt, callback=lambda ok, p: seen.append((ok, p)), soft=True, rs=dict(erasures=True))
    try:
        for p in pay:
            mod.send_pkt(p)
        x = np.concatenate([np.zeros(2 * N, np.complex64), mod.flush(), np.zeros(N + CP, np.complex64)])
        assert dem.work(x) == [(True, p) for p in pay] == seen
        assert dem.last_rs == [(True, 0, 0)] * len(pay) and dem.last_rs_second == [0] * len(pay)
        assert [len(v) for v in dem.last_soft] == [8 * rc.coded_len(len(p)) for p in pay]
        half = len(x) // 2
        assert dem.feed(x[:half]) + dem.feed(x[half:]) + dem.flush() == [(True, p) for p in pay]
    finally:
        for o in (mod, dem):
            o.engine().close()


def test_the_command_line_takes_rs_erasures(tmp_path):
    from ofdm_uhd_amd import benchmark_ofdm_rx, benchmark_ofdm_tx, iqio
    src = tmp_path / "tx.bin"
    data = np.random.default_rng(0).integers(0, 256, 20000, dtype=np.uint8).tobytes()
    src.write_bytes(data)
    iqf = str(tmp_path / "tx.dat")
    npk = benchmark_ofdm_tx.main(["--from-file", str(src), "--to-file", iqf, "-M", "1.0", "-s", "1024", "--rs"])
    iq = iqio.read_complex_binary(iqf)
    rng = np.random.default_rng(1)
    x = np.concatenate([np.zeros(1024, np.complex64), iq, np.zeros(2048, np.complex64)])
    x += ((rng.standard_normal(len(x)) + 1j * rng.standard_normal(len(x))) * 1e-3).astype(np.complex64)
    iqio.file_sink(iqf).write(x)
    for extra in (["--rs-erasures"], ["--rs-erasures", "24"]):
        out = str(tmp_path / ("rx%d.bin" % len(extra)))
        acct = benchmark_ofdm_rx.main(["--from-file", iqf, "--to-file", out] + extra)
        assert acct.n_rcvd == npk and acct.n_right == npk
        assert open(out, "rb").read() == data
    with pytest.raises(SystemExit):
        benchmark_ofdm_rx.main(["--from-file", iqf, "--to-file", str(tmp_path / "x.bin"), "--rs-erasures", "--fec"])


# ---- 9. the impaired link ------------------------------------------------------------------------------------------------
# The grid, searched on the CPU with rs_rel_cases.link_on_the_cpu: noise seeds 7 .. 12, 16 .. 22 dB in 1 dB steps (errors-
# only RS goes from losing every packet to keeping all six between 16 and 21 dB), M = 28: 42 points, at every one the
# receiver's packet list is the six packets.  Packets decoded to the payload sent, errors only > with reliabilities:
#   seed    16 dB            17 dB            18 dB            19 dB            20 dB            21 dB            22 dB
#    7   000000 > 100011  100001 > 110011  110011 > 111011  110011 > 111011  110011 > 111011  111111 > 111111  111111 > 111111
#    8   000000 > 100000  000000 > 100100  101000 > 111111  all six either way from 19 dB on
#    9   000000 > 100000  000000 > 110011  010010 > 110011  010010 > 110011  110011 > 110011  111011 > 111011  111011 > 111011
#   10   000000 > 111000  100000 > 111001  111001 > 111011  111011 > 111011  111011 > 111011  111011 > 111011  111011 > 111111
#   11   001010 > 011011  011011 > 111111  011011 > 111111  all six either way from 19 dB on
#   12   100000 > 101001  101000 > 101011  111000 > 111101  111011 > 111111  all six either way from 20 dB on
# Of 36 packets per level: 3 > 15, 9 > 24, 19 > 31, 28 > 32, 31 > 32, 34 > 34, 34 > 35; 158 > 203 of 252 in all.  At
# every point decoding with reliabilities returned every packet that errors-only decoding returned, and no decoder
# reported ok for a wrong payload.  At 21 of the 42 points errors-only loses at least two of six and reliabilities return
# more.  Taken: seed 7 at 16 dB (none > three), seed 8 at 18 dB (two > six) and seed 9 at 17 dB (none > four).
# Per packet: errors only (ok, corrected, failed), then with reliabilities (ok, corrected, failed, second).
LINK_CASES = {
    (7, 16.0): (((0, 0, 2), (0, 15, 1), (0, 0, 2), (0, 0, 2), (0, 0, 2), (0, 15, 1)),
                ((1, 34, 0, 2), (0, 15, 1, 0), (0, 0, 2, 0), (0, 0, 2, 0), (1, 41, 0, 2), (1, 32, 0, 1))),
    (8, 18.0): (((1, 32, 0), (0, 0, 2), (1, 30, 0), (0, 13, 1), (0, 14, 1), (0, 13, 1)),
                ((1, 32, 0, 0), (1, 34, 0, 2), (1, 30, 0, 0), (1, 32, 0, 1), (1, 34, 0, 1), (1, 33, 0, 1))),
    (9, 17.0): (((0, 0, 2), (0, 15, 1), (0, 0, 2), (0, 0, 2), (0, 0, 2), (0, 0, 2)),
                ((1, 40, 0, 2), (1, 33, 0, 1), (0, 0, 2, 0), (0, 0, 2, 0), (1, 38, 0, 2), (1, 42, 0, 2))),
}


@pytest.mark.parametrize("seed,snr_db", sorted(LINK_CASES), ids=["seed%d-%.0fdB" % c for c in sorted(LINK_CASES)])
def test_impaired_link(seed, snr_db):
    """Exact, twice.  Against the models fed with the same call's packets and soft values: ofdm_demod(rs=True) equals the
    RS model, ofdm_demod(soft=True, rs=dict(erasures=True)) equals the model with the reliabilities of last_soft, in
    every field.  Against the CPU pre-check: per packet the outcome listed at LINK_CASES; reliabilities never return
    fewer packets, and every ok payload is the one sent."""
    opt = options.default_options(modulation=sc.LINK_MOD, fft_length=sc.LINK_N, occupied_tones=sc.LINK_OCC, cp_length=sc.LINK_CP)
    pay = list(sc.link_payloads())
    mod = ofdm.ofdm_mod(opt, pad_for_usrp=False, rs=True)
    plain = ofdm.ofdm_demod(opt, rs=True)
    wrel = ofdm.ofdm_demod(opt, soft=True, rs=dict(erasures=True, max_erasures=28))
    raw = ofdm.ofdm_demod(opt, soft=True)
    try:
        for p in pay:
            mod.send_pkt(p)
        iq = mod.flush()
        psig = float(np.mean(np.abs(iq.astype(np.complex128)) ** 2))
        ch = mod.engine()
        ch.set_multipath(sc.link_channel_cfg(snr_db, psig, seed))
        y = ch.multipath(sc.link_air(iq))
        pk = raw.work(y)
        vals = list(raw.last_soft)
        got_p, got_r = plain.work(y), wrel.work(y)
        rs_p, rs_r, second = list(plain.last_rs), list(wrel.last_rs), list(wrel.last_rs_second)
        n_ok = (plain.n_ok, wrel.n_ok)
    finally:
        for o in (mod, plain, wrel, raw):
            o.engine().close()
    assert [len(b) for _, b in pk] == [rc.coded_len(len(p)) for p in pay]                              # the six packets
    m_p = [rc.decode(b) for _, b in pk]
    m_r = [rr.decode(b, rr.rel_from_values(v), 28) for (_, b), v in zip(pk, vals)]
    print("link seed %d at %.0f dB: packet CRC %s, errors only ok %s corrected %s failed %s, with reliabilities ok %s corrected %s "
          "failed %s second %s" % (seed, snr_db, [int(ok) for ok, _ in pk], [o[0] for o in m_p], [o[2] for o in m_p], [o[3] for o in m_p],
                                    [o[0] for o in m_r], [o[2] for o in m_r], [o[3] for o in m_r], [o[4] for o in m_r]))
    assert got_p == [(bool(o[0]), o[1]) for o in m_p] and got_r == [(bool(o[0]), o[1]) for o in m_r]
    assert rs_p == [(bool(ok), o[2], o[3]) for (ok, _), o in zip(pk, m_p)]
    assert rs_r == [(bool(ok), o[2], o[3]) for (ok, _), o in zip(pk, m_r)] and second == [o[4] for o in m_r]
    want_p, want_r = LINK_CASES[(seed, snr_db)]
    assert tuple((o[0], o[2], o[3]) for o in m_p) == want_p and tuple((o[0],) + o[2:] for o in m_r) == want_r
    for o_p, o_r, sent in zip(m_p, m_r, pay):
        assert (not o_p[0] or o_p[1] == sent) and (not o_r[0] or o_r[1] == sent)                       # no ok for a wrong payload
        assert o_r[0] >= o_p[0]                                                                         # never fewer
    assert n_ok == (sum(w[0] for w in want_p), sum(w[0] for w in want_r))
    assert n_ok[0] <= 4 and n_ok[1] > n_ok[0]                                                           # loses at least two; more come back
