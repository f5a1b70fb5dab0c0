"""The LDPC decoder's byte reliabilities on the GPU (csrc/ldpc.h: k_ldpc_decode_rel<SOFT, RATE>; ofdm_ldpc_decode_rel,
ofdm_ldpc_decode_soft_rel, ofdm_rx_ldpc_decode_soft_rel) and the concatenated link above them,
ofdm_demod(ldpc=, rs=dict(erasures=True, source="ldpc")).  Everything is integer arithmetic: every result is compared with
the model of tests/ldpc_rel_cases.py by equality, the reliabilities with array_equal.

The impaired link (test_link_*): 16-QAM, N 512 / occ 200 / CP 128, four packets of 880, 300, 700 and 1748 bytes (rng 2026)
as RS blocks in rate-1/2 LDPC blocks, noise only through the channel stage.  The point was searched on the CPU as
coded_stream_cases.py describes for its own captures (model encoders, the oracle's transmitter, the float64 channel model of
multipath_cases, the oracle's receiver and the frame sink restated over its taps, soft_cases' values, the model decoder
and the RS model), noise seeds 1 .. 8 at 12.5, 13, 13.5 and 14 dB: at 13.5 dB, noise seed 8, all four packets come back;
from the soft values 7 of the first packet's 11 codewords and 4 of the third's 9 fail and the other two packets decode
in 3 and 1 iterations; RS returns the second and the fourth with and without reliabilities, and one RS codeword of the
third takes the second pass; from the hard bytes 8 and 6 codewords fail.  (The failures there are bursts: the same
packets fail at every level of the grid, so this link shows the format on the air, not a gain.)  The test asserts on what
the GPU receiver delivers that some packet has failed codewords and some packet has none."""
import ctypes as C
import functools

import numpy as np
import pytest

import ldpc_rate_cases as lr
import ldpc_rel_cases as lc
import rs_cases as rc
import rs_rel_cases as rr
import soft_cases as sc
from ofdm_uhd_amd import _abi, config, engine, ldpc, multipath, ofdm, options

pytestmark = pytest.mark.gpu

LINK_SNR_DB, LINK_NOISE_SEED = 13.5, 8
LINK_SIZES = (880, 300, 700, 1748)
SOFT_LEVELS = {"1/2": 1.25, "2/3": 2.0, "3/4": 2.5, "5/6": 3.25}    # Eb/N0 dB of item 1's values: near each rate's threshold
NO_BLOCK_LEN = 193                  # (193 - 1) mod 192 = 0 < PB: no block at any rate


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(options.default_options(modulation="qpsk"))
    yield e
    e.close()


def cfg_of(rate, max_iters=20):
    return dict(rate=rate, max_iters=max_iters)


def as_model(res):
    return [(int(r[0]),) + tuple(r[1:]) for r in res]


def lengths(rate):
    """Item 1's payload lengths: the block CRC inside, at the end of and straddling the first codeword, two codewords,
    a shortened last codeword, one more one-codeword block (the codeword count is then no multiple of 4), the largest."""
    c = lc.code(rate)
    KI = c.CW_INFO
    return (0, 1, KI - 5, KI - 4, KI - 3, 2 * KI - 4, 2 * KI + 7, 40, c.MAX_PAYLOAD)


@functools.lru_cache(maxsize=None)
def batch(rate, soft):
    """(inputs, the model's results) of item 1's batch: hard blocks with 1 % of their bits flipped, or values from an AWGN
    channel near the rate's threshold; a length that is no block in the middle."""
    c = lc.code(rate)
    rng = np.random.default_rng(71 + lr.RATE_IDS[rate])
    blks = [c.encode(rng.integers(0, 256, n, dtype=np.uint8).tobytes()) for n in lengths(rate)]
    ncw = sum(c.codewords(n + 4) for n in lengths(rate))
    assert ncw % 4 != 0, ncw
    if soft:
        ins = [c.awgn_values(b, SOFT_LEVELS[rate], rng) for b in blks]
        ins.insert(4, np.ones(8 * NO_BLOCK_LEN, np.int8))
        want = c.decode_many_rel(ins)
    else:
        ins = []
        for b in blks:
            bits = np.unpackbits(np.frombuffer(b, np.uint8))
            ins.append(np.packbits(bits ^ (rng.random(len(bits)) < 0.01)).tobytes())
        ins.insert(4, bytes(NO_BLOCK_LEN))
        want = c.decode_many_rel([lr.hard_values(b) if len(b) != NO_BLOCK_LEN else np.zeros(8 * NO_BLOCK_LEN, np.int8) for b in ins])
    return tuple(ins), tuple(want)


def raw_call(eng, rate, ins, soft, rel, rel_cap, max_iters=20, payload_cap=None):
    """One of the two batch entry points called through ctypes on a host-mode handle: returns (rc, payload blob, payload
    offsets, ok, corrected, iters, cw_failed); ``rel`` is the caller's uint8 array or None."""
    lib, h = eng._lib, eng._h
    u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
    p = lambda a, t=C.c_void_p: None if a is None else a.ctypes.data_as(t)
    blob, offs, lens = engine._pack_values(list(ins)) if soft else engine.pack_payloads(list(ins))
    n = len(lens)
    out = np.full(max(int(lens.astype(np.int64).sum()), 1), 0x5A, np.uint8)
    poff = np.full(n + 1, 77, np.uint64)
    ok, it = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    corr, failed = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    fn = lib.ofdm_ldpc_decode_soft_rel if soft else lib.ofdm_ldpc_decode_rel
    cfg = ldpc.ldpc_cfg(max_iters, rate)
    r = fn(h, C.byref(cfg), p(blob), p(offs, u64p), p(lens, u32p), n, p(out, C.POINTER(C.c_uint8)), len(out) if payload_cap is None else payload_cap,
           p(poff, u64p), p(ok), p(corr, u32p), p(it), p(failed, u32p), p(rel, C.POINTER(C.c_uint8)), rel_cap)
    return r, out, poff, ok, corr, it, failed


# ---- 1. payload lengths, per rate, hard and soft, one batch per rate ---------------------------------------------------------
@pytest.mark.parametrize("soft", [False, True], ids=["hard", "soft"])
@pytest.mark.parametrize("rate", lc.RATES)
def test_one_batch_of_every_length(eng, rate, soft):
    ins, want = batch(rate, soft)
    got = (eng.ldpc_decode_soft_rel if soft else eng.ldpc_decode_rel)(list(ins), cfg_of(rate))
    assert lc.same(as_model(got), list(want))
    assert [len(g[5]) for g in got] == [len(g[1]) for g in got] == list(lengths(rate)[:4]) + [0] + list(lengths(rate)[4:])
    assert len(got[0][5]) == 0 and got[4][:5] == (False, b"", 0, 0, 0)         # a payload of 0 bytes, and the length that is no block
    q = np.concatenate([w[5] for w in want])
    assert (q >= 128).any() and len(set(q.tolist())) > 20                         # (the batch visits many values)
    if soft:
        assert (q < 128).any() and any(w[4] for w in want)                       # and some codeword failed
    # the blobs as the C call leaves them: 0xA5 outside the blocks' ranges, the offsets those of the payloads
    rel = np.full(sum(lengths(rate)) + 64, 0xA5, np.uint8)
    r, out, poff, ok, corr, it, failed = raw_call(eng, rate, ins, soft, rel, len(rel))
    assert r == _abi.OFDM_OK
    total = int(poff[-1])
    assert total == sum(lengths(rate)) and poff[4] == poff[5]                     # the no-block entry has no bytes
    assert np.array_equal(rel[:total], q) and (rel[total:] == 0xA5).all()
    assert [(int(ok[i]), out[int(poff[i]):int(poff[i + 1])].tobytes(), int(corr[i]), int(it[i]), int(failed[i])) for i in range(len(ins))] == \
        [tuple(w[:5]) for w in want]


def test_device_blob_is_written_only_inside_the_blocks():
    """Device-pointer mode, rates 1/2 and 5/6, soft: the kernel's own stores into a rel blob pre-filled with 0xA5, with the
    no-block entry in the middle and slack behind the last block."""
    torch = pytest.importorskip("torch")
    dev = engine.Engine(options.default_options(modulation="qpsk"), device_ptrs=True)
    try:
        for rate in ("1/2", "5/6"):
            ins, want = batch(rate, True)
            blob, offs, lens = engine._pack_values(list(ins))
            d_in = torch.from_numpy(blob.copy()).cuda()
            total = sum(lengths(rate))
            d_out = torch.full((total + 100,), 0xEE, dtype=torch.uint8, device="cuda")
            d_rel = torch.full((total + 100,), 0xA5, dtype=torch.uint8, device="cuda")
            poff, ok, corr, it, failed = dev.ldpc_decode_rel_device(d_in.data_ptr(), offs, lens, d_out.data_ptr(), d_out.numel(), d_rel.data_ptr(),
                                                                    d_rel.numel(), cfg_of(rate), soft=True)
            out, rel = d_out.cpu().numpy(), d_rel.cpu().numpy()
            assert int(poff[-1]) == total and poff[4] == poff[5]
            assert np.array_equal(rel[:total], np.concatenate([w[5] for w in want])) and (rel[total:] == 0xA5).all()
            assert out[:total].tobytes() == b"".join(w[1] for w in want) and (out[total:] == 0xEE).all()
            assert [(int(ok[i]), int(corr[i]), int(it[i]), int(failed[i])) for i in range(len(ins))] == [(w[0],) + tuple(w[2:5]) for w in want]
    finally:
        dev.close()


# ---- 2. mixed workgroups: conv must not leak between the waves of a workgroup ----------------------------------------------
@pytest.mark.parametrize("rate", lc.RATES)
def test_failed_codewords_next_to_clean_ones(eng, rate):
    c = lc.code(rate)
    KI = c.CW_INFO
    rng = np.random.default_rng(5)
    spoiled = (1, 4, 5, 7, 10)                                                    # among 11 one-codeword blocks: workgroups 0 1 0 0 | 1 1 0 1 | 0 0 1
    blks = [c.encode(rng.integers(0, 256, KI - 4, dtype=np.uint8).tobytes()) for _ in range(11)]
    three = c.encode(rng.integers(0, 256, 3 * KI - 4, dtype=np.uint8).tobytes())  # and a block whose middle codeword is the spoiled one
    ins = [lc.spoil(b, [0]) if i in spoiled else b for i, b in enumerate(blks)] + [lc.spoil(three, [1])]
    one = eng.ldpc_decode_rel(ins, cfg_of(rate, 1))
    assert lc.same(as_model(one), [c.decode_rel(b, 1) for b in ins])
    for i, g in enumerate(one[:11]):
        assert (g[5].max() < 128 and g[4] == 1) if i in spoiled else (g[5].min() >= 128 and g[4] == 0), i
    q = one[11][5]
    assert q[:KI].min() >= 128 and q[KI:2 * KI].max() < 128 and q[2 * KI:].min() >= 128 and one[11][4] == 1
    many = eng.ldpc_decode_rel(ins, cfg_of(rate, 20))                              # the same flips with iterations to spare
    assert lc.same(as_model(many), [c.decode_rel(b, 20) for b in ins])
    for g in many:
        assert g[0] and g[4] == 0 and g[5].min() >= 128
    assert {g[3] for g in many} != {1}                                            # (the spoiled ones took more than one)


# ---- 3. the ends of the range ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", lc.RATES)
def test_range_ends(eng, rate):
    c = lc.code(rate)
    KI = c.CW_INFO
    pay = np.random.default_rng(6).integers(0, 256, 2 * KI - 4, dtype=np.uint8).tobytes()
    blk = c.encode(pay)
    hard = lr.hard_values(blk)
    strong = (hard.astype(np.int16) * 127 // 16).astype(np.int8)                  # clean values at +-127
    zero = hard.copy()
    zero[:8 * lr.CW_SENT] = 0                                                     # a codeword whose values are all 0
    erased = lr.hard_values(lc.spoil(blk, [0])).copy()
    erased[8 * 17 + 3] = 0                                                        # one erased bit in byte 17 of a codeword that fails
    ins = [strong, zero, erased]
    got = eng.ldpc_decode_soft_rel(ins, cfg_of(rate, 1))
    assert lc.same(as_model(got), lc.code(rate).decode_many_rel(ins, 1))
    assert got[0][:2] == (True, pay) and (got[0][5] == 255).all()
    assert (got[1][5][:KI] == 128).all() and got[1][5][KI:].min() > 128 and got[1][4] == 0
    assert got[2][4] == 1 and got[2][5][:KI].max() < 128 <= got[2][5][KI:].min()


# ---- 4. the other fields are the plain decoder's ---------------------------------------------------------------------------
@pytest.mark.parametrize("rate", lc.RATES)
def test_the_other_fields_equal_the_plain_calls(eng, rate):
    for soft in (False, True):
        ins = list(batch(rate, soft)[0])
        plain = (eng.ldpc_decode_soft if soft else eng.ldpc_decode)(ins, cfg_of(rate))
        withrel = (eng.ldpc_decode_soft_rel if soft else eng.ldpc_decode_rel)(ins, cfg_of(rate))
        assert [g[:5] for g in withrel] == plain
        assert all(g[5].dtype == np.uint8 and len(g[5]) == len(g[1]) for g in withrel)


def _air(iq, N=512, CP=128):
    return np.concatenate([np.zeros(2 * N, np.complex64), iq, np.zeros(N + CP + 2 * N, np.complex64)])


def test_the_receivers_own_values():
    """rx_ldpc_decode_soft_rel after one rx() == ldpc_decode_soft_rel on rx_soft(), host and device pointers."""
    torch = pytest.importorskip("torch")
    N, CP = 64, 16
    opt = options.default_options(modulation="qpsk", fft_length=N, occupied_tones=48, cp_length=CP)
    c = lc.code("1/2")
    rng = np.random.default_rng(8)
    pay = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (0, 92, 93, 300)]
    mod = ofdm.ofdm_mod(opt, pad_for_usrp=False, ldpc=True)
    e = engine.Engine(opt)
    dev = engine.Engine(cfg=config.make_cfg(opt, device_ptrs=True))
    try:
        for p in pay:
            mod.send_pkt(p)
        x = np.concatenate([np.zeros(2 * N, np.complex64), mod.flush(), np.zeros(N + CP, np.complex64)])
        x += ((rng.standard_normal(len(x)) + 1j * rng.standard_normal(len(x))) * 1e-3).astype(np.complex64)
        with pytest.raises(ValueError):
            e.rx_ldpc_decode_soft_rel()                                           # no rx yet
        e.set_rx_soft(True)
        assert len(e.rx(x)) == len(pay)
        vals = e.rx_soft()
        got = e.rx_ldpc_decode_soft_rel()
        assert lc.same(as_model(got), as_model(e.ldpc_decode_soft_rel(vals)))
        assert lc.same(as_model(got), c.decode_many_rel(vals))
        assert [g[:5] for g in got] == e.rx_ldpc_decode_soft() == [(True, p, 0, 1, 0) for p in pay]
        assert all(int(g[5].min()) >= 128 for g in got if len(g[5]))
        dev.set_rx_soft(True)
        xd = torch.from_numpy(x.view(np.float32).copy()).cuda()
        blk = torch.zeros(8192, dtype=torch.uint8, device="cuda")
        assert dev.rx_device(xd.data_ptr(), len(x), blk.data_ptr(), 8192, 16)[0] == len(pay)
        total = sum(len(p) for p in pay)
        d_pay = torch.full((total + 8,), 0xEE, dtype=torch.uint8, device="cuda")
        d_rel = torch.full((total + 8,), 0xA5, dtype=torch.uint8, device="cuda")
        poff, ok, corr, it, failed = dev.rx_ldpc_decode_soft_rel_device(d_pay.data_ptr(), total, d_rel.data_ptr(), total)
        p_, r_ = d_pay.cpu().numpy(), d_rel.cpu().numpy()
        assert lc.same([(int(ok[i]), p_[int(poff[i]):int(poff[i + 1])].tobytes(), int(corr[i]), int(it[i]), int(failed[i]),
                         r_[int(poff[i]):int(poff[i + 1])]) for i in range(len(pay))], as_model(got))
        assert (p_[total:] == 0xEE).all() and (r_[total:] == 0xA5).all()
        with pytest.raises(engine.EngineError):
            dev.rx_ldpc_decode_soft_rel_device(d_pay.data_ptr(), total, d_rel.data_ptr(), total - 1)
    finally:
        for o in (mod.engine(), e, dev):
            o.close()


# ---- 5. errors, and the device-pointer chain into the outer decoder ----------------------------------------------------------
def test_error_codes(eng):
    ins, want = batch("1/2", False)
    total = sum(lengths("1/2"))
    r, _, poff, *_ = raw_call(eng, "1/2", ins, False, None, 1 << 20)
    assert r == _abi.OFDM_E_INVAL                                                 # a null rel
    rel = np.full(total, 0xA5, np.uint8)
    r, _, poff, *_ = raw_call(eng, "1/2", ins, False, rel, total - 1)
    assert r == _abi.OFDM_E_CAPACITY and int(poff[-1]) == total and poff[0] == 0  # the offsets are set first
    assert np.array_equal(np.diff(poff.astype(np.int64)), [len(w[1]) for w in want]) and (rel == 0xA5).all()
    r, _, poff, *_ = raw_call(eng, "1/2", ins, False, rel, total, payload_cap=total - 1)
    assert r == _abi.OFDM_E_CAPACITY and int(poff[-1]) == total and (rel == 0xA5).all()
    lib, h = eng._lib, eng._h
    assert lib.ofdm_rx_ldpc_decode_soft_rel(h, None, None, 0, None, None, None, None, None, None, 0, 0, None) == _abi.OFDM_E_INVAL
    with pytest.raises(ValueError):
        eng.rx_ldpc_decode_soft_rel()                                             # no rx() with soft values before it
    r, *_ = raw_call(eng, "1/2", ins, False, rel, total)
    assert r == _abi.OFDM_OK and np.array_equal(rel, np.concatenate([w[5] for w in want]))   # the handle stays usable


def test_last_ms_reports_the_rel_kernel(eng):
    ins = list(batch("1/2", False)[0])
    eng.prof_enable(True)
    try:
        eng.ldpc_decode_rel(ins)
        assert eng.ldpc_last_ms() > 0.0
        eng.ldpc_decode_rel([bytes(NO_BLOCK_LEN)])                                # nothing launched: no time to report
        with pytest.raises(ValueError):
            eng.ldpc_last_ms()
        assert len(eng.prof()) == _abi.K_COUNT                                    # the kernel table is what it was
    finally:
        eng.prof_enable(False)


def test_device_pointers_chain_into_the_outer_decoder(eng):
    """ldpc_decode_rel_device -> rs_decode_rel_device with rel_offs=None, no host copy between, equals the host calls."""
    torch = pytest.importorskip("torch")
    ch = lc.chain(tuple(range(16, 24)))
    vals = [v for _, v, _, _, _ in ch]
    host_inner = eng.ldpc_decode_soft_rel(vals)
    host_outer = eng.rs_decode_rel([g[1] for g in host_inner], [g[5] for g in host_inner], dict(max_erasures=lc.CHAIN_M))
    dev = engine.Engine(options.default_options(modulation="qpsk"), device_ptrs=True)
    try:
        blob, offs, lens = engine._pack_values(vals)
        d_in = torch.from_numpy(blob.copy()).cuda()
        cap = int(lens.astype(np.int64).sum())
        d_mid = torch.full((cap,), 0xEE, dtype=torch.uint8, device="cuda")
        d_rel = torch.full((cap,), 0xA5, dtype=torch.uint8, device="cuda")
        d_out = torch.full((cap,), 0xEE, dtype=torch.uint8, device="cuda")
        poff, ok, corr, it, failed = dev.ldpc_decode_rel_device(d_in.data_ptr(), offs, lens, d_mid.data_ptr(), cap, d_rel.data_ptr(), cap, soft=True)
        mlen = np.diff(poff.astype(np.int64)).astype(np.uint32)
        res = dev.rs_decode_rel_device(d_mid.data_ptr(), poff[:-1].copy(), mlen, d_rel.data_ptr(), None, d_out.data_ptr(), cap,
                                       dict(max_erasures=lc.CHAIN_M))
        out = d_out.cpu().numpy()
        got = [(bool(res[1][i]), out[int(res[0][i]):int(res[0][i + 1])].tobytes()) + tuple(int(col[i]) for col in res[2:]) for i in range(len(vals))]
        assert got == host_outer
        assert [(bool(ok[i]), int(corr[i]), int(it[i]), int(failed[i])) for i in range(len(vals))] == [(g[0],) + g[2:5] for g in host_inner]
    finally:
        dev.close()


# ---- 6. the seeded chain -----------------------------------------------------------------------------------------------------
def test_the_chain_on_seeds_16_to_31(eng):
    """ldpc_decode_soft_rel -> rs_decode_rel equals the model block by block; seeds 20 and 28 come back only with the
    reliabilities."""
    seeds = tuple(range(16, 32))
    ch = lc.chain(seeds)
    vals = [v for _, v, _, _, _ in ch]
    inner = eng.ldpc_decode_soft_rel(vals)
    assert lc.same(as_model(inner), [d for _, _, d, _, _ in ch])
    outer = eng.rs_decode_rel([g[1] for g in inner], [g[5] for g in inner], dict(max_erasures=lc.CHAIN_M))
    assert as_model(outer) == [tuple(o) for _, _, _, _, o in ch]
    alone = eng.rs_decode([g[1] for g in inner])
    assert as_model(alone) == [tuple(o) for _, _, _, o, _ in ch]
    for s in (20, 28):
        i = seeds.index(s)
        assert outer[i][0] and outer[i][1] == ch[i][0] and outer[i][4] == 1 and not alone[i][0], s
    for (p, _, _, _, _), a, o in zip(ch, alone, outer):
        assert (not a[0] or (o[0] and o[1] == p)) and (not o[0] or o[1] == p)     # nothing lost, nothing wrong accepted


# ---- 7. on a link --------------------------------------------------------------------------------------------------------------
def _opt():
    return options.default_options(modulation="qam16", fft_length=512, occupied_tones=200, cp_length=128)


@functools.lru_cache(maxsize=None)
def link_payloads():
    rng = np.random.default_rng(2026)
    return tuple(rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in LINK_SIZES)


@functools.lru_cache(maxsize=None)
def link_capture(impaired):
    mod = ofdm.ofdm_mod(_opt(), pad_for_usrp=False, ldpc=True, rs=True)
    try:
        for p in link_payloads():
            mod.send_pkt(p)
        iq = mod.flush()
        y = np.concatenate([np.zeros(2 * 512, np.complex64), iq, np.zeros(512 + 128, np.complex64)])      # clean: one symbol of silence behind
        if impaired:
            y = sc.link_air(iq)
            psig = float(np.mean(np.abs(iq.astype(np.complex128)) ** 2))
            ch = mod.engine()
            ch.set_multipath(multipath.multipath_cfg(sigma=multipath.sigma_for_snr(LINK_SNR_DB, psig), seed=LINK_NOISE_SEED))
            y = ch.multipath(y)
    finally:
        mod.engine().close()
    y.setflags(write=False)
    return y


def _fields(dem):
    return dict(last_fec=list(dem.last_fec), last_ldpc=list(dem.last_ldpc), last_rs=list(dem.last_rs), last_rs_second=list(dem.last_rs_second),
                last_ldpc_rel=[np.array(q) for q in dem.last_ldpc_rel], last_soft=[np.array(v) for v in dem.last_soft])


def _same_fields(a, b):
    for k in ("last_fec", "last_ldpc", "last_rs", "last_rs_second"):
        assert a[k] == b[k], k
    for k in ("last_ldpc_rel", "last_soft"):
        assert len(a[k]) == len(b[k]) and all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a[k], b[k])), k


def _model_fields(raw, inner, M=rr.DEFAULT_M):
    """ofdm_demod's fields from the uncoded receiver's packets and the model's inner results."""
    outer = [rr.decode(d[1], d[5], M) for d in inner]
    return [(bool(o[0]), o[1]) for o in outer], dict(
        last_fec=[(bool(ok), d[2]) for (ok, _), d in zip(raw, inner)], last_ldpc=[(d[3], d[4]) for d in inner],
        last_rs=[(bool(d[0]), o[2], o[3]) for d, o in zip(inner, outer)], last_rs_second=[o[4] for o in outer],
        last_ldpc_rel=[d[5] for d in inner])


def test_link_through_noise_equals_the_model_and_feed_equals_work():
    """13.5 dB, noise seed 8 (the file's docstring): the soft path.  Every field of ofdm_demod is the model's on the
    engine's own soft values; feed() in two cuts plus flush() equals work(), every field."""
    c = lc.code("1/2")
    y = link_capture(True)
    kw = dict(ldpc=True, soft=True, rs=dict(erasures=True, source="ldpc"))
    fired = {"one": [], "fed": []}
    one = ofdm.ofdm_demod(_opt(), callback=lambda ok, p: fired["one"].append((ok, p)), **kw)
    fed = ofdm.ofdm_demod(_opt(), callback=lambda ok, p: fired["fed"].append((ok, p)), **kw)
    plain = ofdm.ofdm_demod(_opt())
    try:
        raw = plain.work(y)
        got = one.work(y)
        have = _fields(one)
        inner = c.decode_many_rel(have["last_soft"])
        want, want_f = _model_fields(raw, inner)
        print("link %.1f dB seed %d: packets %s, packet CRC %s, cw_failed %s, iters %s, rs ok %s, second %s" % (
            LINK_SNR_DB, LINK_NOISE_SEED, [len(p) for _, p in raw], [int(ok) for ok, _ in raw], [d[4] for d in inner], [d[3] for d in inner],
            [int(ok) for ok, _ in want], want_f["last_rs_second"]))
        assert got == want == fired["one"] and len(got) >= 2
        want_f["last_soft"] = have["last_soft"]
        _same_fields(have, want_f)
        assert any(f > 0 for _, f in have["last_ldpc"]) and any(f == 0 for _, f in have["last_ldpc"])      # a codeword failed, a packet had none
        assert any(q.size and q.min() < 128 for q in have["last_ldpc_rel"]) and any(q.size and q.min() >= 128 for q in have["last_ldpc_rel"])
        assert all(p in link_payloads() for ok, p in got if ok) and (one.n_packets, one.n_ok) == (len(got), sum(ok for ok, _ in got))
        half = len(y) // 2
        out, acc = [], dict((k, []) for k in have)
        for call in (lambda: fed.feed(y[:half]), lambda: fed.feed(y[half:]), fed.flush):
            part = call()
            out += part
            f = _fields(fed)
            assert all(len(f[k]) == len(part) for k in f)
            for k in f:
                acc[k] += f[k]
        assert out == got and fired["fed"] == fired["one"]
        _same_fields(acc, have)
        assert (fed.n_packets, fed.n_ok) == (one.n_packets, one.n_ok)
    finally:
        for o in (one, fed, plain):
            o.engine().close()


def test_link_hard_path_on_noise_and_on_a_clean_capture():
    """The hard path (``soft`` left out).  Through the same noise: the model on what an uncoded receiver returns.  On a clean
    capture: all packets, no second pass, every reliability at least 128."""
    c = lc.code("1/2")
    dem = ofdm.ofdm_demod(_opt(), ldpc=True, rs=dict(erasures=True, source="ldpc", max_erasures=24))
    plain = ofdm.ofdm_demod(_opt())
    try:
        y = link_capture(True)
        raw = plain.work(y)
        got = dem.work(y)
        want, want_f = _model_fields(raw, [c.decode_rel(p) for _, p in raw], 24)
        want_f["last_soft"] = []
        assert got == want
        _same_fields(_fields(dem), want_f)
        assert any(f > 0 for _, f in dem.last_ldpc)
        x = link_capture(False)
        assert dem.work(x) == [(True, p) for p in link_payloads()]
        assert dem.last_rs_second == [0] * 4 and dem.last_rs == [(True, 0, 0)] * 4 and dem.last_fec == [(True, 0)] * 4
        assert dem.last_ldpc == [(1, 0)] * 4 and dem.last_soft == []
        assert [len(q) for q in dem.last_ldpc_rel] == [rc.coded_len(n) for n in LINK_SIZES] and all(q.min() >= 128 for q in dem.last_ldpc_rel)
    finally:
        dem.engine().close()
        plain.engine().close()


# ---- 8. the command line ---------------------------------------------------------------------------------------------------------
def test_the_command_line_takes_rs_erasures_with_ldpc(tmp_path):
    from ofdm_uhd_amd import benchmark_ofdm_rx, benchmark_ofdm_tx, iqio
    src = tmp_path / "tx.bin"
    data = np.random.default_rng(0).integers(0, 256, 6000, dtype=np.uint8).tobytes()
    src.write_bytes(data)
    iqf = str(tmp_path / "tx.dat")
    npk = benchmark_ofdm_tx.main(["--from-file", str(src), "--to-file", iqf, "-M", "1.0", "-s", "1024", "--ldpc", "--rs"])
    iq = iqio.read_complex_binary(iqf)
    rng = np.random.default_rng(1)
    x = np.concatenate([np.zeros(1024, np.complex64), iq, np.zeros(2048, np.complex64)])
    x += ((rng.standard_normal(len(x)) + 1j * rng.standard_normal(len(x))) * 1e-3).astype(np.complex64)
    iqio.file_sink(iqf).write(x)
    for extra in (["--ldpc", "--rs-erasures"], ["--ldpc-soft", "--rs-erasures", "24"]):
        out = str(tmp_path / ("rx%d.bin" % len(extra)))
        acct = benchmark_ofdm_rx.main(["--from-file", iqf, "--to-file", out] + extra)
        assert acct.n_rcvd == npk and acct.n_right == npk
        assert open(out, "rb").read() == data
    with pytest.raises(SystemExit):
        benchmark_ofdm_rx.main(["--from-file", iqf, "--to-file", str(tmp_path / "x.bin"), "--fec", "--rs-erasures"])
