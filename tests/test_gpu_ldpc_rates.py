"""LDPC coded links at rates 2/3, 3/4 and 5/6 on the GPU (csrc/ldpc.h: k_ldpc_encode<RATE>, k_ldpc_decode<SOFT, RATE>; the
rate is the word behind max_iters in ofdm_ldpc_cfg).  Everything is integer arithmetic, so every result is compared with
the NumPy model of tests/ldpc_rate_cases.py by equality, in every field: the encoder's blocks, the decoder's payloads,
verdicts, corrected counts, iteration counts and failed codewords on clean, flipped, soft, erased and full-scale input,
lengths that are a block at another rate only, batches of many workgroups, the device-pointer forms, the error codes,
and the layer on a link: ofdm_mod(ldpc=dict(rate=)) -> ofdm_demod(ldpc=dict(rate=)), clean and through noise, hard and
soft, under rs=True and across a stream cut.

Soft input (test_decode_soft_from_a_gaussian_channel): 64 one-codeword blocks (payloads of KI - 4 bytes) per rate, BPSK
over AWGN at the rate's nominal Eb/N0, values rint(4 LLR), seed 61 (the values of the higher level: seed 1061).  Checked on
the CPU in the model first, seeds 60 .. 74: at 2.25 / 2.75 / 3.5 dB (rates 2/3, 3/4, 5/6) seed 61 leaves 11 / 5 / 3 blocks
failed and 53 / 59 / 61 decoded, of which 6 / 1 / 4 took more than 10 iterations; 1.5 dB higher all 64 decode within 4 / 3
/ 3 iterations.  The test asserts these properties of the model before it compares.

CPU pre-check of the impaired links (the float64 channel model of multipath_cases, noise only, fed to the oracle's
receiver, the soft-demapper model of soft_cases behind it and the model decoder of the rate behind that): QPSK, N 512 /
occ 200 / CP 128, four packets of KI - 4, KI - 3, 300 and 2 KI - 4 bytes (rng 2025), noise seeds 1 .. 12 at 9.5 and
10.5 dB.  As at rate 1/2 the receiver's synchroniser sets the floor: most seeds lose or gain a flag at either level.
  2/3 at 10.5 dB, noise seed 5: the raw packets show 1.3, 0, 0 and 0.03 % bit errors, the packet CRC fails on two; the
  model decodes all four from the hard bytes in 3, 1, 1 and 1 iterations and from the soft values in 1 each.
  3/4 at 10.5 dB, noise seed 5: 1.17 % bit errors in the first packet, whose CRC fails; the model decodes all four, hard in
  3, 1, 1 and 1 iterations, soft in 2, 1, 1 and 1.
  5/6 at 10.5 dB, noise seed 4: 0.07, 0, 0 and 0.03 % bit errors, the packet CRC fails on two; the model decodes all four
  in one iteration, hard and soft.
The tests assert the pre-check's properties on what the GPU receiver delivers: at least one packet's hard bytes fail their
CRC before decoding, and the model returns every packet."""
import ctypes as C
import functools

import numpy as np
import pytest

import ldpc_rate_cases as rc
from ofdm_uhd_amd import _abi, engine, ldpc, multipath, ofdm, options, rs

pytestmark = pytest.mark.gpu

RATES = ("2/3", "3/4", "5/6")
SOFT_LEVELS = {"2/3": 2.25, "3/4": 2.75, "5/6": 3.5}         # Eb/N0 dB at which some blocks fail; the other level is 1.5 dB up
SOFT_SEED = 61
LINK_LEVELS = {"2/3": (10.5, 5), "3/4": (10.5, 5), "5/6": (10.5, 4)}       # (SNR dB, noise seed): the docstring's pre-check


def sizes(rate):
    """k = n + 4 either side of one codeword and of two, and the rate's largest payload (21 full codewords)."""
    KI = rc.code(rate).CW_INFO
    return (0, 1, KI - 5, KI - 4, KI - 3, 2 * KI - 4, 2 * KI - 3, rc.code(rate).MAX_PAYLOAD)


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(options.default_options(modulation="qpsk"))
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def payloads(rate):
    rng = np.random.default_rng(41)
    return tuple(rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in sizes(rate))


@functools.lru_cache(maxsize=None)
def blocks(rate):
    return tuple(rc.code(rate).encode(p) for p in payloads(rate))


def as_model(res):
    return [(int(r[0]),) + tuple(r[1:]) for r in res]


def cfg_of(rate, max_iters=20):
    return dict(rate=rate, max_iters=max_iters)


@functools.lru_cache(maxsize=None)
def damaged(rate, flips):
    rng = np.random.default_rng(int(flips * 1000))
    out = []
    for b in blocks(rate):
        bits = np.unpackbits(np.frombuffer(b, np.uint8))
        out.append(np.packbits(bits ^ (rng.random(len(bits)) < flips)).tobytes())
    return tuple(out)


@functools.lru_cache(maxsize=None)
def gaussian(rate, up):
    """64 one-codeword blocks through the AWGN channel at the rate's level, or 1.5 dB above it."""
    c = rc.code(rate)
    rng = np.random.default_rng(SOFT_SEED)
    pay = [rng.integers(0, 256, c.CW_INFO - 4, dtype=np.uint8).tobytes() for _ in range(64)]
    blks = [c.encode(p) for p in pay]
    if up:
        rng = np.random.default_rng(SOFT_SEED + 1000)
    return tuple(c.awgn_values(b, SOFT_LEVELS[rate] + (1.5 if up else 0.0), rng) for b in blks)


@functools.lru_cache(maxsize=None)
def model_soft(rate, up, max_iters=20):
    return tuple(rc.code(rate).decode_many(list(gaussian(rate, up)), max_iters))


# ---- 1. encoder --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", RATES)
def test_encode_one_mixed_batch_and_alone(eng, rate):
    pay, want = list(payloads(rate)), list(blocks(rate))
    assert eng.ldpc_encode(pay, cfg_of(rate)) == want
    assert eng.ldpc_encode([], cfg_of(rate)) == []
    for p, b in zip(pay, want):
        assert eng.ldpc_encode([p], cfg_of(rate)) == [b]
    assert eng.ldpc_encode(pay, ldpc.ldpc_cfg(3, rate)) == want                  # the encoder ignores max_iters
    assert [len(b) for b in want] == [ldpc.coded_len(n, rate) for n in sizes(rate)]
    assert eng.ldpc_encode(pay[:5]) != want[:5]                                  # (rate 1/2 is another code)


# ---- 2. decoder --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", RATES)
def test_decode_clean(eng, rate):
    c, pay, blks = rc.code(rate), payloads(rate), list(blocks(rate))
    got = as_model(eng.ldpc_decode(blks, cfg_of(rate)))
    assert got == [(1, p, 0, 1, 0) for p in pay]
    assert got == [c.decode(b) for b in blks]
    for i in (0, 3, 4, 7):
        assert as_model(eng.ldpc_decode([blks[i]], cfg_of(rate))) == [(1, pay[i], 0, 1, 0)]
    assert as_model(eng.ldpc_decode_soft([rc.hard_values(b) for b in blks], cfg_of(rate))) == got
    assert eng.ldpc_decode([], cfg_of(rate)) == []


@pytest.mark.parametrize("flips", [0.01, 0.03])
@pytest.mark.parametrize("rate", RATES)
def test_decode_hard_with_flips_equals_the_model_in_every_field(eng, rate, flips):
    c = rc.code(rate)
    blks = list(damaged(rate, flips))
    got = as_model(eng.ldpc_decode(blks, cfg_of(rate)))
    want = [c.decode(b) for b in blks]
    print("%s flips %.2f: ok %s corrected %s iters %s failed %s" % (rate, flips, [w[0] for w in want], [w[2] for w in want],
                                                                     [w[3] for w in want], [w[4] for w in want]))
    assert got == want
    assert max(w[3] for w in want) > 1
    assert as_model(eng.ldpc_decode([blks[4]], cfg_of(rate))) == [want[4]]


@pytest.mark.parametrize("up", [False, True], ids=["threshold", "plus1.5dB"])
@pytest.mark.parametrize("rate", RATES)
def test_decode_soft_from_a_gaussian_channel(eng, rate, up):
    vals = list(gaussian(rate, up))
    want = list(model_soft(rate, up))
    print("%s soft %s: ok %d of 64, failed blocks %d, iters %s" % (rate, "up" if up else "threshold", sum(w[0] for w in want),
                                                                  sum(w[4] > 0 for w in want), sorted({w[3] for w in want})))
    if up:
        assert all(w[0] == 1 and w[4] == 0 for w in want)
    else:      # the level and seed the docstring chose on the CPU: failures, successes and late stops, in the model
        assert any(w[4] > 0 and w[0] == 0 for w in want) and any(w[0] == 1 for w in want)
        assert any(w[0] == 1 and w[4] == 0 and w[3] > 10 for w in want)
    assert as_model(eng.ldpc_decode_soft(vals, cfg_of(rate))) == want
    assert as_model(eng.ldpc_decode_soft([vals[5]], cfg_of(rate))) == [want[5]]


@pytest.mark.parametrize("rate", RATES)
def test_max_iters_1_and_64(eng, rate):
    c = rc.code(rate)
    vals = list(gaussian(rate, False))
    for it in (1, 64):
        want = list(model_soft(rate, False, it))
        assert as_model(eng.ldpc_decode_soft(vals, cfg_of(rate, it))) == want
        assert max(w[3] for w in want) == it
    assert all(w[3] == 1 for w in model_soft(rate, False, 1))
    hard = list(damaged(rate, 0.03))
    for it in (1, 64):
        assert as_model(eng.ldpc_decode(hard, ldpc.ldpc_cfg(it, rate))) == [c.decode(b, it) for b in hard]


@pytest.mark.parametrize("rate", RATES)
def test_all_erasures_and_minus_128(eng, rate):
    c, pay, blks = rc.code(rate), payloads(rate), blocks(rate)
    # all-zero values: erasures only; every check holds for the zero word after one iteration, and its CRC field is wrong
    # (but for the empty payload, whose CRC-32 is 0)
    zeros = [np.zeros(8 * len(b), np.int8) for b in blks]
    want = c.decode_many(zeros)
    assert want == [(int(n == 0), bytes(n), 0, 1, 0) for n in sizes(rate)]
    assert as_model(eng.ldpc_decode_soft(zeros, cfg_of(rate))) == want
    # a block of -128s: reads as -127 everywhere, the zero word again, and every sent bit agrees with it
    low = [np.full(8 * len(b), -128, np.int8) for b in blks]
    want = c.decode_many(low)
    assert want == [(int(n == 0), bytes(n), 0, 1, 0) for n in sizes(rate)]
    assert as_model(eng.ldpc_decode_soft(low, cfg_of(rate))) == want
    # -128 for every 0 bit of a clean block, and sprinkled over noisy ones
    loud = [np.where(rc.hard_values(b) > 0, 127, -128).astype(np.int8) for b in blks]
    assert as_model(eng.ldpc_decode_soft(loud, cfg_of(rate))) == [(1, p, 0, 1, 0) for p in pay] == c.decode_many(loud)
    rng = np.random.default_rng(43)
    mixed = []
    for v in gaussian(rate, False)[:16]:
        v = v.copy()
        v[rng.random(len(v)) < 0.05] = -128
        v[rng.random(len(v)) < 0.1] = 0
        mixed.append(v)
    assert as_model(eng.ldpc_decode_soft(mixed, cfg_of(rate))) == c.decode_many(mixed)


@pytest.mark.parametrize("rate", RATES)
def test_lengths_that_are_a_block_at_another_rate_only(eng, rate):
    c = rc.code(rate)
    PB = c.CW_PARITY
    good = blocks(rate)
    for m in (PB + 3, 192 + PB, 4033):
        assert ldpc.payload_len(m, rate) is None
        # (a block at the rates with less parity; 5/6 has the least, and 4033 is too long for all)
        assert any(ldpc.payload_len(m, q) is not None for q in rc.RATES) == (m != 4033 and rate != "5/6")
        assert as_model(eng.ldpc_decode([bytes(m)], cfg_of(rate))) == [rc.NO_BLOCK]
        assert as_model(eng.ldpc_decode_soft([np.ones(8 * m, np.int8)], cfg_of(rate))) == [rc.NO_BLOCK]
    if rate != "5/6":       # 225 bytes: a codeword and one info byte at rate 5/6, nothing here
        assert ldpc.payload_len(225, "5/6") == 157 and ldpc.payload_len(225, rate) is None
        assert as_model(eng.ldpc_decode([bytes(225)], cfg_of(rate))) == [rc.NO_BLOCK]
    # 192 + PB + 1 is one: the codeword's parity and one info byte behind a full codeword
    short = c.encode(payloads(rate)[4][:c.CW_INFO - 3])
    assert len(short) == 192 + PB + 1 and as_model(eng.ldpc_decode([short], cfg_of(rate))) == [c.decode(short)] == [(1, payloads(rate)[4], 0, 1, 0)]
    # one batch mixing lengths: blocks of every size among lengths that are none
    batch = [good[5], bytes(PB + 3), good[7], bytes(192 + PB), b"", good[4], bytes(4033), good[1], good[0]]
    got = as_model(eng.ldpc_decode(batch, cfg_of(rate)))
    for i in (1, 3, 4, 6):
        assert got[i] == rc.NO_BLOCK
    for i, j in ((0, 5), (2, 7), (5, 4), (7, 1), (8, 0)):
        assert got[i] == (1, payloads(rate)[j], 0, 1, 0)
    assert got == [c.decode(b) for b in batch]
    assert as_model(eng.ldpc_decode([bytes(PB + 3), b"", bytes(4033)], cfg_of(rate))) == [rc.NO_BLOCK] * 3      # not one block: no launch
    # a block of this rate read at rate 1/2 (the default) is another code's: same lengths where both have them, no payload back
    assert as_model(eng.ldpc_decode([good[3]]))[0][:2] != (1, payloads(rate)[3])


@pytest.mark.parametrize("rate", RATES)
def test_a_batch_of_1000_one_codeword_blocks(eng, rate):
    """250 workgroups of four one-wave codewords, and 999 blocks whose last workgroup holds three; eight distinct blocks,
    clean and damaged, so the waves of one workgroup stop at different iterations."""
    c = rc.code(rate)
    KI = c.CW_INFO
    rng = np.random.default_rng(47)
    small = []
    for n, flips in ((0, 0.0), (KI - 4, 0.0), (40, 0.01), (KI - 4, 0.015), (KI - 5, 0.02), (1, 0.03), (KI - 4, 0.05), (60, 0.5)):
        b = c.encode(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
        bits = np.unpackbits(np.frombuffer(b, np.uint8))
        small.append(np.packbits(bits ^ (rng.random(len(bits)) < flips)).tobytes())
    want8 = [c.decode(b) for b in small]
    assert len({w[3] for w in want8}) >= 3 and want8[0][3] == 1 and want8[-1][:1] == (0,)
    order = rng.integers(0, 8, 1000)
    got = as_model(eng.ldpc_decode([small[i] for i in order], cfg_of(rate)))
    assert got == [want8[i] for i in order]
    got = as_model(eng.ldpc_decode([small[i] for i in order[:999]], cfg_of(rate)))
    assert got == [want8[i] for i in order[:999]]


# ---- 3. error codes and device pointers ------------------------------------------------------------------------------------
def test_error_codes(eng):
    lib, h = eng._lib, eng._h
    u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
    p = lambda a, t=C.c_void_p: None if a is None else a.ctypes.data_as(t)
    pay = np.zeros(8192, np.uint8)
    out = np.zeros(16384, np.uint8)
    coff = np.full(3, 77, np.uint64)

    def enc(cfg, lens):
        lens = np.array(lens, np.uint32)
        return lib.ofdm_ldpc_encode(h, C.byref(cfg), p(pay), p(np.array([0, 4000], np.uint64), u64p), p(lens, u32p), 2, p(out), len(out),
                                    p(coff, u64p))

    for rate in rc.RATES:
        c = rc.code(rate)
        cfg = ldpc.ldpc_cfg(rate=rate)
        assert enc(cfg, [100, c.MAX_PAYLOAD]) == _abi.OFDM_OK and coff.tolist() == [0, c.coded_len(100), c.coded_len(100) + 4032]
        assert enc(cfg, [100, c.MAX_PAYLOAD + 1]) == _abi.OFDM_E_INVAL          # a payload one byte above the rate's largest
        with pytest.raises(ValueError):
            eng.ldpc_encode([b"a", bytes(c.MAX_PAYLOAD + 1)], cfg)
        assert eng.ldpc_encode([b"a"], cfg) == [c.encode(b"a")]                  # the handle stays usable
    four = ldpc.ldpc_cfg()
    four.rate = 4                                                                # no such rate
    tail = ldpc.ldpc_cfg(rate="3/4")
    tail.reserved[1] = 1                                                         # a reserved word behind the rate
    blk = np.frombuffer(rc.code("3/4").encode(bytes(140)), np.uint8).copy()
    pout, poff = np.zeros(512, np.uint8), np.full(2, 77, np.uint64)
    ok, it = np.zeros(1, np.uint8), np.zeros(1, np.uint8)
    corr, failed = np.zeros(1, np.uint32), np.zeros(1, np.uint32)

    def dec(cfg, fn):
        return fn(h, C.byref(cfg), p(blk), p(np.zeros(1, np.uint64), u64p), p(np.array([192], np.uint32), u32p), 1, p(pout), 512, p(poff, u64p),
                  p(ok), p(corr, u32p), p(it), p(failed, u32p))

    for cfg in (four, tail):
        assert enc(cfg, [100, 60]) == _abi.OFDM_E_INVAL
        assert dec(cfg, lib.ofdm_ldpc_decode) == _abi.OFDM_E_INVAL
        assert dec(cfg, lib.ofdm_ldpc_decode_soft) == _abi.OFDM_E_INVAL
        with pytest.raises(ValueError):
            eng.ldpc_encode([b"a"], cfg)
        with pytest.raises(ValueError):
            eng.ldpc_decode([blk.tobytes()], cfg)
    assert dec(ldpc.ldpc_cfg(rate="3/4"), lib.ofdm_ldpc_decode) == _abi.OFDM_OK and ok.tolist() == [1] and poff.tolist() == [0, 140]
    with pytest.raises(ValueError):
        eng.ldpc_encode([b"a"], dict(rate="7/8"))


def test_device_pointers():
    torch = pytest.importorskip("torch")
    dev = engine.Engine(options.default_options(modulation="qpsk"), device_ptrs=True)
    try:
        for rate in RATES:
            cfg = ldpc.ldpc_cfg(rate=rate)
            idx = (0, 3, 4, 7)
            pay = [payloads(rate)[i] for i in idx]
            blob, offs, lens = engine.pack_payloads(pay)
            d_pay = torch.from_numpy(blob.copy()).cuda()
            d_coded = torch.zeros(8192, dtype=torch.uint8, device="cuda")
            coff = dev.ldpc_encode_device(d_pay.data_ptr(), offs, lens, d_coded.data_ptr(), d_coded.numel(), cfg)
            coded = d_coded.cpu().numpy()
            want = [blocks(rate)[i] for i in idx]
            assert [coded[int(coff[i]):int(coff[i + 1])].tobytes() for i in range(4)] == want
            assert not coded[int(coff[4]):].any()                                   # nothing behind the last block
            with pytest.raises(engine.EngineError):
                dev.ldpc_encode_device(d_pay.data_ptr(), offs, lens, d_coded.data_ptr(), int(coff[4]) - 1, cfg)
            clen = np.diff(coff).astype(np.uint32)
            d_out = torch.full((8192,), 0xEE, dtype=torch.uint8, device="cuda")
            poff, ok, corr, it, failed = dev.ldpc_decode_device(d_coded.data_ptr(), coff[:4].copy(), clen, d_out.data_ptr(), d_out.numel(), cfg)
            out = d_out.cpu().numpy()
            assert ok.tolist() == [1] * 4 and corr.tolist() == [0] * 4 and it.tolist() == [1] * 4 and failed.tolist() == [0] * 4
            assert [out[int(poff[i]):int(poff[i + 1])].tobytes() for i in range(4)] == pay
            assert (out[int(poff[4]):] == 0xEE).all()                               # nothing written past the payloads
            vals = list(gaussian(rate, False)[:8])
            d_soft = torch.from_numpy(np.concatenate(vals)).cuda()
            soff = (np.arange(8, dtype=np.uint64) * np.uint64(8 * 192))
            res = dev.ldpc_decode_device(d_soft.data_ptr(), soff, np.full(8, 192, np.uint32), d_out.data_ptr(), d_out.numel(), cfg, soft=True)
            out = d_out.cpu().numpy()
            got = [(int(res[1][i]), out[int(res[0][i]):int(res[0][i + 1])].tobytes(), int(res[2][i]), int(res[3][i]), int(res[4][i]))
                   for i in range(8)]
            assert got == list(model_soft(rate, False)[:8])
    finally:
        dev.close()


# ---- 4. on a link ------------------------------------------------------------------------------------------------------
def _air(iq, tail=512 + 128 + 2 * 512, N=512):
    """The burst with silence around it, as the receiver's tests embed one."""
    return np.concatenate([np.zeros(2 * N, np.complex64), iq, np.zeros(tail, np.complex64)])


@functools.lru_cache(maxsize=None)
def link_payloads(rate, impaired=False):
    KI = rc.code(rate).CW_INFO
    rng = np.random.default_rng(2025)
    return tuple(rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (KI - 4, KI - 3, 300) + ((2 * KI - 4,) if impaired else ()))


def _close(*objs):
    for o in objs:
        o.engine().close()


@pytest.mark.parametrize("rate", RATES)
def test_clean_loopback_hard_and_soft(rate):
    c = rc.code(rate)
    opt = options.default_options(modulation="qpsk")                  # N 512 / occ 200 / CP 128
    pay = list(link_payloads(rate))
    mod = ofdm.ofdm_mod(opt, pad_for_usrp=False, ldpc=dict(rate=rate))
    seen = []
    hard = ofdm.ofdm_demod(opt, callback=lambda ok, payload: seen.append((ok, payload)), ldpc=dict(rate=rate))
    soft = ofdm.ofdm_demod(opt, ldpc=dict(rate=rate, max_iters=20), soft=True)
    plain = ofdm.ofdm_demod(opt)
    try:
        for p in pay:
            mod.send_pkt(p)
        x = _air(mod.flush(), tail=512 + 128)
        assert hard.work(x) == [(True, p) for p in pay] == seen
        assert hard.last_fec == [(True, 0)] * 3 and hard.last_ldpc == [(1, 0)] * 3 and (hard.n_packets, hard.n_ok) == (3, 3)
        assert plain.work(x) == [(True, c.encode(p)) for p in pay]    # exactly the model's coded blocks on the air
        got = soft.work(x)
        want = c.decode_many(soft.last_soft)
        assert got == [(True, p) for p in pay] == [(bool(w[0]), w[1]) for w in want]
        assert soft.last_fec == [(True, w[2]) for w in want] and soft.last_ldpc == [(w[3], w[4]) for w in want] == [(1, 0)] * 3
    finally:
        _close(mod, hard, soft, plain)


@functools.lru_cache(maxsize=None)
def impaired_capture(rate):
    """The impaired link of the file's docstring: the four packets through the channel stage at the pre-check's level and
    noise seed."""
    snr_db, seed = LINK_LEVELS[rate]
    mod = ofdm.ofdm_mod(options.default_options(modulation="qpsk"), pad_for_usrp=False, ldpc=dict(rate=rate))
    try:
        for p in link_payloads(rate, True):
            mod.send_pkt(p)
        iq = mod.flush()
        psig = float(np.mean(np.abs(iq.astype(np.complex128)) ** 2))
        ch = mod.engine()
        ch.set_multipath(multipath.multipath_cfg(sigma=multipath.sigma_for_snr(snr_db, psig), seed=seed))
        y = ch.multipath(_air(iq))
    finally:
        _close(mod)
    y.setflags(write=False)
    return y


@pytest.mark.parametrize("rate", RATES)
def test_impaired_link_equals_the_model_and_every_packet_comes_back(rate):
    """Noise only, at the level and seed the file's docstring derives on the CPU.  Exact part: the hard result is the model
    applied to what ofdm_demod without a code returns, the soft result is the model applied to the engine's own last_soft
    values, in every field of last_fec and last_ldpc.  Physical part, the pre-check's: at least one packet's hard bytes
    fail their CRC before decoding, and every packet comes back, hard and soft."""
    c = rc.code(rate)
    opt = options.default_options(modulation="qpsk")
    pay = list(link_payloads(rate, True))
    hard = ofdm.ofdm_demod(opt, ldpc=dict(rate=rate))
    soft = ofdm.ofdm_demod(opt, ldpc=dict(rate=rate), soft=True)
    plain = ofdm.ofdm_demod(opt)
    try:
        y = impaired_capture(rate)
        raw = plain.work(y)
        assert len(raw) == len(pay)
        want = [c.decode(p) for _, p in raw]
        assert hard.work(y) == [(bool(w[0]), w[1]) for w in want]
        assert hard.last_fec == [(bool(ok), w[2]) for (ok, _), w in zip(raw, want)]
        assert hard.last_ldpc == [(w[3], w[4]) for w in want]
        got = soft.work(y)
        swant = c.decode_many(soft.last_soft)
        print("impaired %s: outer ok %s, hard ok %s corrected %s iters %s, soft ok %s corrected %s iters %s" % (
            rate, [int(ok) for ok, _ in raw], [w[0] for w in want], [w[2] for w in want], [w[3] for w in want], [w[0] for w in swant],
            [w[2] for w in swant], [w[3] for w in swant]))
        assert got == [(bool(w[0]), w[1]) for w in swant]
        assert soft.last_fec == [(bool(ok), w[2]) for (ok, _), w in zip(raw, swant)]
        assert soft.last_ldpc == [(w[3], w[4]) for w in swant]
        assert not all(ok for ok, _ in raw)                           # a packet CRC failed before decoding
        assert [(w[0], w[1]) for w in want] == [(1, p) for p in pay]  # the model returns every packet from the hard bytes
        assert got == [(True, p) for p in pay] and soft.n_ok == len(pay)
    finally:
        _close(hard, soft, plain)


@pytest.mark.parametrize("rate", RATES)
def test_rs_above_ldpc_clean(rate):
    opt = options.default_options(modulation="qpsk")
    limit = rs.max_payload_under(ldpc.max_payload(rate))
    assert limit == {"2/3": 2328, "3/4": 2632, "5/6": 2904}[rate]
    KI = rc.code(rate).CW_INFO
    rng = np.random.default_rng(53)
    pay = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (0, KI - 4, KI - 3, limit)]
    mod = ofdm.ofdm_mod(opt, pad_for_usrp=False, ldpc=dict(rate=rate), rs=True)
    dem = ofdm.ofdm_demod(opt, ldpc=dict(rate=rate), rs=True)
    try:
        for p in pay[:2]:
            mod.send_pkt(p)
        with pytest.raises(ValueError):
            mod.send_pkt(bytes(limit + 1))                              # the RS block would not fit the inner code at this rate
        for p in pay[2:]:
            mod.send_pkt(p)
        x = _air(mod.flush(), tail=512 + 128)
        assert dem.work(x) == [(True, p) for p in pay]
        assert dem.last_fec == [(True, 0)] * 4 and dem.last_rs == [(True, 0, 0)] * 4
        assert [it for it, _ in dem.last_ldpc] == [1] * 4 and [f for _, f in dem.last_ldpc] == [0] * 4
    finally:
        _close(mod, dem)


@pytest.mark.parametrize("soft", [False, True], ids=["hard", "soft"])
def test_feed_in_two_cuts_equals_work_at_rate_3_4(soft):
    """The impaired capture of rate 3/4 in one work() and as feed(), feed(), flush() cut in the middle: the packets, last_fec,
    last_ldpc, last_soft, the callback's sequence and the counters."""
    opt = options.default_options(modulation="qpsk")
    kw = dict(ldpc=dict(rate="3/4"), soft=True) if soft else dict(ldpc=dict(rate="3/4"))
    y = impaired_capture("3/4")
    fired = {"one": [], "fed": []}
    one = ofdm.ofdm_demod(opt, callback=lambda ok, p: fired["one"].append((ok, p)), **kw)
    fed = ofdm.ofdm_demod(opt, callback=lambda ok, p: fired["fed"].append((ok, p)), **kw)
    try:
        want = one.work(y)
        want_f = (list(one.last_fec), list(one.last_ldpc), [np.array(v) for v in one.last_soft])
        assert len(want) == 4 and any(c > 0 for _, c in want_f[0])    # (there was something to correct)
        half = len(y) // 2
        got, got_f = [], ([], [], [])
        for call in (lambda: fed.feed(y[:half]), lambda: fed.feed(y[half:]), fed.flush):
            out = call()
            got += out
            assert len(fed.last_fec) == len(fed.last_ldpc) == len(out) and len(fed.last_soft) == (len(out) if soft else 0)
            got_f[0].extend(fed.last_fec)
            got_f[1].extend(fed.last_ldpc)
            got_f[2].extend(np.array(v) for v in fed.last_soft)
        assert got == want and fired["fed"] == fired["one"] == want
        assert got_f[0] == want_f[0] and got_f[1] == want_f[1]
        assert len(got_f[2]) == len(want_f[2]) == (4 if soft else 0)
        assert all(np.array_equal(a, b) for a, b in zip(got_f[2], want_f[2]))
        assert (fed.n_packets, fed.n_ok) == (one.n_packets, one.n_ok) == (4, 4)
    finally:
        _close(one, fed)


def test_value_errors_of_the_link_objects():
    opt = options.default_options(modulation="qpsk")
    with pytest.raises(ValueError):
        ofdm.ofdm_mod(opt, pad_for_usrp=False, ldpc=dict(rate="4/5"))
    with pytest.raises(ValueError):
        ofdm.ofdm_demod(opt, ldpc=dict(rate=4))
    with pytest.raises(ValueError):
        ofdm.ofdm_demod(opt, ldpc=dict(rate="3/4"), fec=True)
    for rate in RATES:
        n = ldpc.max_payload(rate)
        mod = ofdm.ofdm_mod(opt, pad_for_usrp=False, ldpc=dict(rate=rate))
        both = ofdm.ofdm_mod(opt, pad_for_usrp=False, ldpc=dict(rate=rate), rs=True)
        try:
            mod.send_pkt(bytes(n))
            with pytest.raises(ValueError):
                mod.send_pkt(bytes(n + 1))                                  # payload above the rate's largest, the offending packet only
            assert len(mod.flush()) > 0
            both.send_pkt(bytes(rs.max_payload_under(n)))
            with pytest.raises(ValueError):
                both.send_pkt(bytes(rs.max_payload_under(n) + 1))           # an RS block that does not fit
            assert len(both.flush()) > 0
        finally:
            _close(mod, both)
