"""The soft-output Viterbi decoder on the GPU (csrc/fec_rel.h: k_fec_decode_rel; ofdm_fec_decode_rel /
ofdm_fec_decode_soft_rel / ofdm_rx_fec_decode_soft_rel).  Everything is integer arithmetic, so every field -- payload,
verdict, corrected count and the reliability bytes -- is compared with the NumPy model of tests/fec_rel_cases.py by
equality, and the first three also with the plain decoder on the same handle: every chunk shape of the trellis, hard, soft
and tied input, the clamp, the punctured rates, batches wider than one workspace slice with lengths that are no block
among them, refusals, the device-pointer chain into ofdm_rs_decode_rel, the receiver's own values, the timing accessor,
the concatenated chain over a noisy channel, and ofdm_demod(rs=dict(erasures=True, source="fec")).

The seeds of the concatenated chain were chosen on the CPU with the models alone (fec_rel_cases.chain_outcome: n = 219,
one RS codeword, rate 1/2, C = 16, BPSK over AWGN at Eb/N0 = 2.0 dB of the whole concatenated rate, scale 32, M = 28).
Of the seeds 0 .. 199 there, rs_cases.decode returns 135 payloads and the chain with reliabilities 143; the eight it
gains are 4, 7, 41, 98, 133, 141, 151, 196, and none is lost.  The list below: (plain, with reliabilities, second)
    seed 0: (0, 0, 0)    seed 1: (1, 1, 0)    seed 2: (1, 1, 0)    seed 4: (0, 1, 1)
    seed 6: (0, 0, 0)    seed 7: (0, 1, 1)    seed 41: (0, 1, 1)
"""
import ctypes as C
import functools

import numpy as np
import pytest

import fec_cases as fc
import fec_rel_cases as fr
import punct_cases as pc
import rs_cases as rc
import rs_rel_cases as rr
from ofdm_uhd_amd import _abi, config, engine, ofdm, options

pytestmark = pytest.mark.gpu

SLICE_BLOCKS = (512 << 20) // (256 * 64 * 8)    # fec_plan.h: FEC_WS_MAX_BYTES over the widest block's 256 chunks of 64 words
CHAIN_SEEDS = {0: (0, 0, 0), 1: (1, 1, 0), 2: (1, 1, 0), 4: (0, 1, 1), 6: (0, 0, 0), 7: (0, 1, 1), 41: (0, 1, 1)}
CHAIN_DB = 2.0
NOTHING = (0, b"", 0, np.zeros(0, np.uint8))


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(options.default_options(modulation="qpsk"))
    yield e
    e.close()


def agree(got, want, tag=None):
    assert len(got) == len(want), tag
    for i, (g, w) in enumerate(zip(got, want)):
        assert isinstance(g[3], np.ndarray) and g[3].dtype == np.uint8, (tag, i)
        assert fr.same(g, w), (tag, i, int(g[0]), int(w[0]), g[2], w[2], len(g[1]), len(w[1]), g[3][:16].tolist(), np.asarray(w[3])[:16].tolist())


def plain(dec):
    return [(bool(ok), p, c) for ok, p, c in dec]


def first_three(dec):
    return [(bool(d[0]), d[1], d[2]) for d in dec]


# ---- 1. every chunk shape, hard, soft and tied input ----------------------------------------------------------------------
@pytest.mark.parametrize("C_", [1, 16])
@pytest.mark.parametrize("n", fr.SIZES)
def test_every_chunk_shape(eng, n, C_):
    hard = fr.case(n, C_, "flips")
    got = eng.fec_decode_rel([hard], C_)
    agree(got, [fr.case_model(n, C_, "flips")], "flips")
    assert first_three(got) == plain(eng.fec_decode([hard], C_))
    kinds = [k for k in fr.KINDS if k != "flips"]
    vals = [fr.case(n, C_, k) for k in kinds] + [fc.hard_values(hard)]
    got = eng.fec_decode_soft_rel(vals, C_)
    agree(got, [fr.case_model(n, C_, k) for k in kinds] + [fr.case_model(n, C_, "flips")], "soft")
    assert first_three(got) == plain(eng.fec_decode_soft(vals, C_))
    assert all(len(g[3]) == n for g in got)


@pytest.mark.parametrize("C_", [1, 16])
def test_saturation(eng, C_):
    """Free distance 10: 250 at |v| = 25, the clamp 255 at |v| = 26 and at 127; all-zero values tie everywhere."""
    for n in (4, 219):
        vals = [fr.clean_values(n, C_, lv) for lv in (25, 26, 127)] + [np.zeros(8 * fc.coded_len(n), np.int8)]
        got = eng.fec_decode_soft_rel(vals, C_)
        agree(got, [fr.decode_values(v, C_) for v in vals], n)
        assert [sorted(set(g[3].tolist())) for g in got] == [[250], [255], [255], [0]]
        assert first_three(got)[:3] == [(True, fr.case_payload(n), 0)] * 3 and got[3][1] == bytes(n)


# ---- 2. punctured rates ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", pc.RATES)
def test_punctured_rates(eng, rate):
    odd = next(n for n in range(5, 60) if pc.coded_len(n, rate) % 2)
    rng = np.random.default_rng(pc.RATE_ID[rate])
    cfg = dict(rate=rate)
    hard, vals = [], []
    for n in (4, 219, odd):
        blk = pc.encode(fr.case_payload(n), 16, rate)
        assert len(blk) == pc.coded_len(n, rate)
        hard.append(fc.flip(blk, rng.choice(8 * len(blk), 1 + n // 100, replace=False)))
        v = np.clip(np.rint(30.0 * fc.hard_values(blk) + 14.0 * rng.standard_normal(8 * len(blk))), -127, 127).astype(np.int8)
        v[rng.integers(0, 100, len(v)) < 2] = -128
        v[5:9] = 0
        vals.append(v)
    gap = next(m for m in range(8, 60) if pc.payload_len(m, rate) is None)
    hard.append(bytes(gap))
    vals.append(np.ones(8 * gap, np.int8))
    got = eng.fec_decode_rel(hard, cfg)
    agree(got, [fr.decode_rate(b, 16, rate) for b in hard], "hard")
    assert first_three(got) == plain(eng.fec_decode(hard, cfg)) and fr.same(got[-1], NOTHING)
    got = eng.fec_decode_soft_rel(vals, cfg)
    agree(got, [fr.decode_values_rate(v, 16, rate) for v in vals], "soft")
    assert first_three(got) == plain(eng.fec_decode_soft(vals, cfg))
    assert [len(g[3]) for g in got] == [4, 219, odd, 0]


# ---- 3. batches --------------------------------------------------------------------------------------------------------------
def test_mixed_lengths_and_every_alignment(eng):
    """Payload lengths 0 .. 12 and lengths that are no block between them: the payload / reliability offsets visit every
    alignment; a no-block entry takes no room in either blob."""
    batch, want = [], []
    for n in list(range(13)) + [3, 0, 7, 219, 5]:
        batch.append(fr.case(n, 16, "noisy") if n in fr.SIZES else
                     np.clip(24 * fc.hard_values(fc.encode(fr.case_payload(n), 16)).astype(np.int32) + (np.arange(16 * n + 80) % 37) - 18,
                             -127, 127).astype(np.int8))
        want.append(fr.decode_values(batch[-1], 16))
        if n % 3 == 0:
            for m in (7, 8, fc.MAX_CODED + 2):
                batch.append(np.ones(8 * m, np.int8))
                want.append(NOTHING)
    batch.append(np.ones(83, np.int8))                  # no multiple of 8
    want.append(NOTHING)
    got = eng.fec_decode_soft_rel(batch, 16)
    agree(got, want)
    assert first_three(got) == plain(eng.fec_decode_soft(batch, 16))
    assert eng.fec_decode_rel([], 16) == [] and eng.fec_decode_soft_rel([], 16) == []
    agree(eng.fec_decode_rel([b"", bytes(9), bytes(4091)]), [NOTHING] * 3)     # not one block: no launch


@pytest.mark.parametrize("rate,soft", [("1/2", False), ("1/2", True), ("3/4", True)])
def test_a_batch_wider_than_the_workspace_goes_in_slices(eng, rate, soft):
    """One 2040-byte payload makes every block's share of the decision workspace 128 KiB (and 64 KiB of checkpoints):
    SLICE_BLOCKS blocks fill its 512 MiB, the rest of the batch is a second launch over the same memory."""
    assert SLICE_BLOCKS == 4096
    enc = lambda n: pc.encode(fr.case_payload(n), 16, rate)
    small = [enc(n) for n in (0, 3, 4, 12)]
    small[1] = fc.flip(small[1], [5])
    wide = enc(2040)
    gap = next(m for m in range(7, 60) if pc.payload_len(m, rate) is None)
    batch = [small[i % 4] for i in range(SLICE_BLOCKS + 104)]
    batch[7], batch[SLICE_BLOCKS + 1] = bytes(gap), bytes(gap)                  # no block in either slice
    batch[SLICE_BLOCKS - 1], batch[SLICE_BLOCKS], batch[-1] = wide, small[1], wide
    cfg = dict(rate=rate)
    if soft:
        got = eng.fec_decode_soft_rel([fc.hard_values(b) for b in batch], cfg)
    else:
        got = eng.fec_decode_rel(batch, cfg)
    model = functools.lru_cache(maxsize=None)(lambda b: fr.decode_rate(b, 16, rate))
    agree(got, [model(b) for b in batch])
    assert got[-1][:3] == (True, fr.case_payload(2040), 0) and len(got[-1][3]) == 2040
    assert got[SLICE_BLOCKS][:3] == (True, fr.case_payload(3), 1) and fr.same(got[SLICE_BLOCKS + 1], NOTHING)


# ---- 4. refusals, timing ---------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable(eng):
    lib, h = eng._lib, eng._h
    u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
    blocks = [fc.encode(b"abc", 16), fc.encode(b"defgh", 16)]
    blob, offs, lens = engine.pack_payloads(blocks)
    pay, rel = np.zeros(16, np.uint8), np.full(16, 0xEE, np.uint8)
    poff = np.full(3, 77, np.uint64)
    ok, corr = np.zeros(2, np.uint8), np.zeros(2, np.uint32)
    cfg = _abi.ofdm_fec_cfg(struct_size=C.sizeof(_abi.ofdm_fec_cfg), interleave_cols=16)
    args = [h, C.byref(cfg), blob.ctypes.data, offs.ctypes.data_as(u64p), lens.ctypes.data_as(u32p), 2, pay.ctypes.data, 16,
            poff.ctypes.data_as(u64p), ok.ctypes.data, corr.ctypes.data_as(u32p), rel.ctypes.data, 16]
    for fn in (lib.ofdm_fec_decode_rel, lib.ofdm_fec_decode_soft_rel):
        for null in (2, 3, 4, 8, 9, 10, 11):                                # 11: a null rel
            a = list(args)
            a[null] = None
            assert fn(*a) == _abi.OFDM_E_INVAL, null
        for bad in (_abi.ofdm_fec_cfg(struct_size=12, interleave_cols=16), _abi.ofdm_fec_cfg(struct_size=32, interleave_cols=3),
                    _abi.ofdm_fec_cfg(struct_size=32, interleave_cols=16, rate=4)):
            a = list(args)
            a[1] = C.byref(bad)
            assert fn(*a) == _abi.OFDM_E_INVAL
        assert fn(None, *args[1:]) == _abi.OFDM_E_INVAL
    poff[:] = 77
    a = list(args)
    a[12] = 7                                                               # rel_cap one byte short
    assert lib.ofdm_fec_decode_rel(*a) == _abi.OFDM_E_CAPACITY and poff.tolist() == [0, 3, 8]
    poff[:] = 77
    a = list(args)
    a[7] = 7                                                                # payload_cap one byte short
    assert lib.ofdm_fec_decode_rel(*a) == _abi.OFDM_E_CAPACITY and poff.tolist() == [0, 3, 8]
    assert (rel == 0xEE).all() and not pay.any()
    for a in (list(args), args[:1] + [None] + args[2:], args[:12] + [8]):   # cfg == NULL: 16 columns; rel_cap exact
        pay[:], rel[:] = 0, 0xEE
        assert lib.ofdm_fec_decode_rel(*a) == _abi.OFDM_OK
        assert pay[:8].tobytes() == b"abcdefgh" and ok.tolist() == [1, 1] and corr.tolist() == [0, 0]
        assert rel.tolist() == [10] * 8 + [0xEE] * 8                        # clean +-1 values: Delta / 2 = 10
    # the receiver's form: without soft values of a last ofdm_rx it is refused, as ofdm_rx_fec_decode_soft is
    n = C.c_int(-1)
    assert lib.ofdm_rx_fec_decode_soft_rel(h, None, pay.ctypes.data, 16, poff.ctypes.data_as(u64p), ok.ctypes.data, corr.ctypes.data_as(u32p),
                                           rel.ctypes.data, 16, 2, C.byref(n)) == _abi.OFDM_E_INVAL
    agree(eng.fec_decode_rel(blocks), [fr.decode(b) for b in blocks])


def test_last_ms():
    e = engine.Engine(options.default_options(modulation="qpsk"))
    try:
        e.prof_enable(True)
        with pytest.raises(ValueError):
            e.fec_last_ms()                             # no fec call yet
        blk = fc.encode(b"abcd", 16)
        e.fec_decode_rel([blk])
        assert e.fec_last_ms() > 0.0
        with pytest.raises(ValueError):
            e.fec_punct_last_ms()                       # rate 1/2 launches no depuncture
        e.fec_decode_rel([bytes(9)])                    # no block: nothing launched, no time to report
        with pytest.raises(ValueError):
            e.fec_last_ms()
        e.fec_decode_soft_rel([fc.hard_values(pc.encode(b"abcd", 16, "3/4"))], dict(rate="3/4"))
        assert e.fec_last_ms() > 0.0 and e.fec_punct_last_ms() > 0.0
        e.prof_enable(False)
        e.fec_decode_rel([blk])
        with pytest.raises(ValueError):
            e.fec_last_ms()                             # the last call ran without profiling
        assert len(e.prof()) == _abi.K_COUNT            # the kernel table is what it was
    finally:
        e.close()


# ---- 5. device pointers, the receiver's own values ---------------------------------------------------------------------------
def test_the_device_chain_into_the_outer_decoder(eng):
    """fec_decode_rel_device(soft=True) -> rs_decode_rel_device(rel_offs=None): payloads, reliabilities and offsets go
    from one layer to the next as they lie; the result equals the host-mode result; guards stay what they were."""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(21)
    pay = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (59, 219, 1, 0)]
    # (the noise level of the 219-byte chain at 2.5 dB on every block, whatever its length)
    vals = [fr.chain_channel(fc.encode(rc.encode(p), 16), 219, 5 + i, 2.5) for i, p in enumerate(pay)]
    vals.insert(2, np.ones(8 * 9, np.int8))             # no block between them
    real = [0, 1, 3, 4]
    host = eng.fec_decode_soft_rel(vals, 16)
    host_rs = eng.rs_decode_rel([d[1] for d in host], [d[3] for d in host])
    dev = engine.Engine(cfg=config.make_cfg(options.default_options(modulation="qpsk"), device_ptrs=True))
    try:
        lens = np.array([len(v) // 8 for v in vals], np.uint32)
        offs = np.concatenate([[0], np.cumsum([len(v) for v in vals[:-1]])]).astype(np.uint64)
        d_in = torch.from_numpy(np.concatenate(vals)).cuda()
        total = sum(len(d[1]) for d in host)
        d_pay = torch.full((total + 64,), 0xEE, dtype=torch.uint8, device="cuda")
        d_rel = torch.full((total + 64,), 0xEE, dtype=torch.uint8, device="cuda")
        with pytest.raises(engine.EngineError):
            dev.fec_decode_rel_device(d_in.data_ptr(), offs, lens, d_pay.data_ptr(), total, d_rel.data_ptr(), total - 1, 16, soft=True)
        poff, ok, corr = dev.fec_decode_rel_device(d_in.data_ptr(), offs, lens, d_pay.data_ptr(), total, d_rel.data_ptr(), total, 16, soft=True)
        p, r = d_pay.cpu().numpy(), d_rel.cpu().numpy()
        got = [(bool(ok[i]), p[int(poff[i]):int(poff[i + 1])].tobytes(), int(corr[i]), r[int(poff[i]):int(poff[i + 1])]) for i in range(len(vals))]
        agree(got, host)
        assert (p[total:] == 0xEE).all() and (r[total:] == 0xEE).all() and int(poff[-1]) == total
        blen = np.diff(poff).astype(np.uint32)
        n_out = sum(len(q) for q in pay)
        d_out = torch.full((n_out + 64,), 0xEE, dtype=torch.uint8, device="cuda")
        qoff, rok, rcorr, rfail, rsec = dev.rs_decode_rel_device(d_pay.data_ptr(), poff[:-1].copy(), blen, d_rel.data_ptr(), None,
                                                                 d_out.data_ptr(), n_out)
        o = d_out.cpu().numpy()
        got_rs = [(bool(rok[i]), o[int(qoff[i]):int(qoff[i + 1])].tobytes(), int(rcorr[i]), int(rfail[i]), int(rsec[i])) for i in range(len(vals))]
        assert got_rs == host_rs == [tuple([bool(w[0])] + list(w[1:])) for w in (rr.decode(d[1], d[3]) for d in host)]
        assert got_rs[2] == (False, b"", 0, 0, 0) and any(got_rs[i][0] for i in real)
        assert all(got_rs[i][1] == q for i, q in zip(real, pay) if got_rs[i][0]) and (o[n_out:] == 0xEE).all()
    finally:
        dev.close()


def test_the_receivers_own_values():
    """rx_fec_decode_soft_rel after one rx() == fec_decode_soft_rel on rx_soft(), host and device pointers."""
    torch = pytest.importorskip("torch")
    N, CP = 64, 16
    opt = options.default_options(modulation="qpsk", fft_length=N, occupied_tones=48, cp_length=CP)
    rng = np.random.default_rng(22)
    pay = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (40, 0, 13)]
    mod = ofdm.ofdm_mod(opt, pad_for_usrp=False, fec=True)
    eng = engine.Engine(opt)
    dev = engine.Engine(cfg=config.make_cfg(opt, device_ptrs=True))
    try:
        for p in pay:
            mod.send_pkt(p)
        x = np.concatenate([np.zeros(2 * N, np.complex64), mod.flush(), np.zeros(N + CP, np.complex64)])
        with pytest.raises(ValueError):
            eng.rx_fec_decode_soft_rel()                # no rx yet
        eng.set_rx_soft(True)
        assert len(eng.rx(x)) == 3
        vals = eng.rx_soft()
        got = eng.rx_fec_decode_soft_rel()
        agree(got, eng.fec_decode_soft_rel(vals), "engine")
        agree(got, [fr.decode_values(v) for v in vals], "model")
        assert first_three(got) == plain(eng.rx_fec_decode_soft()) == [(True, p, 0) for p in pay]
        assert all(int(g[3].min()) > 0 for g in got if len(g[3]))
        dev.set_rx_soft(True)
        xd = torch.from_numpy(x.view(np.float32).copy()).cuda()
        blk = torch.zeros(4096, dtype=torch.uint8, device="cuda")
        assert dev.rx_device(xd.data_ptr(), len(x), blk.data_ptr(), 4096, 16)[0] == 3
        total = sum(len(p) for p in pay)
        d_pay = torch.full((total + 8,), 0xEE, dtype=torch.uint8, device="cuda")
        d_rel = torch.full((total + 8,), 0xEE, dtype=torch.uint8, device="cuda")
        poff, ok, corr = dev.rx_fec_decode_soft_rel_device(d_pay.data_ptr(), total, d_rel.data_ptr(), total)
        p, r = d_pay.cpu().numpy(), d_rel.cpu().numpy()
        agree([(bool(ok[i]), p[int(poff[i]):int(poff[i + 1])].tobytes(), int(corr[i]), r[int(poff[i]):int(poff[i + 1])]) for i in range(3)], got)
        assert (p[total:] == 0xEE).all() and (r[total:] == 0xEE).all()
    finally:
        for e in (mod.engine(), eng, dev):
            e.close()


# ---- 6. the concatenated chain ----------------------------------------------------------------------------------------------
def test_the_concatenated_chain_exact_and_useful(eng):
    """rs_encode -> fec_encode -> the seeded AWGN channel of fec_rel_cases -> fec_decode_soft_rel -> rs_decode_rel on the
    GPU, against the models in every field, with the outcome per seed the module docstring lists: three blocks the plain
    outer decoder fails come back with reliabilities, two stay lost, two need none."""
    n = 219
    pay = [fr.chain_payload(n, s) for s in CHAIN_SEEDS]
    outer = eng.rs_encode(pay)
    coded = eng.fec_encode(outer, 16)
    assert outer == [rc.encode(p) for p in pay] and coded == [fc.encode(b, 16) for b in outer]
    vals = [fr.chain_channel(c, n, s, CHAIN_DB) for c, s in zip(coded, CHAIN_SEEDS)]
    for v, s in zip(vals, CHAIN_SEEDS):
        assert np.array_equal(v, fr.chain_values(n, s, CHAIN_DB)[1])
    inner = eng.fec_decode_soft_rel(vals, 16)
    want = [fr.chain_decode(v) for v in vals]
    agree(inner, [w[0] for w in want])
    blocks, rel = [d[1] for d in inner], [d[3] for d in inner]
    with_rel = eng.rs_decode_rel(blocks, rel, dict(max_erasures=28))
    without = eng.rs_decode(blocks)
    assert [(int(a), b, c, d, e) for a, b, c, d, e in with_rel] == [w[2] for w in want]
    assert [(int(a), b, c, d) for a, b, c, d in without] == [w[1] for w in want]
    for (s, outcome), p, a, b in zip(CHAIN_SEEDS.items(), pay, without, with_rel):
        assert (int(a[0] and a[1] == p), int(b[0] and b[1] == p), b[4]) == outcome, s
        assert (not a[0] or a[1] == p) and (not b[0] or b[1] == p), s       # every ok payload is the one sent
    gained = [s for s, o in CHAIN_SEEDS.items() if o[:2] == (0, 1)]
    assert len(gained) >= 2 and all(CHAIN_SEEDS[s][2] >= 1 for s in gained) and any(o[:2] == (0, 0) for o in CHAIN_SEEDS.values())


# ---- 7. ofdm_demod -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("soft", [True, False], ids=["soft", "hard"])
def test_ofdm_demod_end_to_end(soft):
    N, CP = 64, 16
    opt = options.default_options(modulation="qpsk", fft_length=N, occupied_tones=48, cp_length=CP)
    for bad in (dict(rs=dict(erasures=True, source="fec")), dict(rs=dict(erasures=True, source="fec"), soft=True),
                dict(rs=dict(erasures=True, source="soft"), soft=True, fec=True), dict(rs=dict(erasures=True), soft=True, fec=True)):
        with pytest.raises(ValueError):
            ofdm.ofdm_demod(opt, **bad)
    rng = np.random.default_rng(23)
    pay = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (59, 180, 1, 148, 0)]
    mod = ofdm.ofdm_mod(opt, pad_for_usrp=False, fec=True, rs=True)
    seen = []
    kw = dict(soft=True) if soft else {}
    dem = ofdm.ofdm_demod(opt, callback=lambda ok, p: seen.append((ok, p)), fec=True, rs=dict(erasures=True, source="fec"), **kw)
    raw = ofdm.ofdm_demod(opt)
    try:
        for p in pay:
            mod.send_pkt(p)
        x = np.concatenate([np.zeros(2 * N, np.complex64), mod.flush(), np.zeros(N + CP, np.complex64)])
        at = 2 * N + (len(x) - 3 * N) * np.array([0.23, 0.41, 0.43, 0.77])
        x[at.astype(np.int64)] += np.complex64(1.8 - 1.2j) * np.abs(x).max()        # a few corrupted samples
        got = dem.work(x)
        if soft:
            inner = [fr.decode_values(v) for v in dem.last_soft]
        else:
            inner = [fr.decode(p) for _, p in raw.work(x)]
        assert len(got) == len(inner) == len(pay) == len(dem.last_fec_rel)
        for q, w in zip(dem.last_fec_rel, inner):
            assert q.dtype == np.uint8 and np.array_equal(q, w[3])
        outer = [rr.decode(w[1], w[3], 28) for w in inner]
        assert got == [(bool(o[0]), o[1]) for o in outer] == seen
        assert dem.last_rs == [(bool(w[0]), o[2], o[3]) for w, o in zip(inner, outer)]
        assert dem.last_rs_second == [o[4] for o in outer]
        assert [c for _, c in dem.last_fec] == [w[2] for w in inner]
        assert [p for ok, p in got if ok] == [p for (ok, _), p in zip(got, pay) if ok] and sum(ok for ok, _ in got) >= 3
        half = len(x) // 2
        assert dem.feed(x[:half]) + dem.feed(x[half:]) + dem.flush() == got
    finally:
        for o in (mod, dem, raw):
            o.engine().close()
