"""LDPC coded links on the GPU (csrc/ldpc.h, ofdm_ldpc_encode / ofdm_ldpc_decode / ofdm_ldpc_decode_soft /
ofdm_rx_ldpc_decode_soft): everything is integer arithmetic, so every result is compared with the NumPy model of
tests/ldpc_cases.py by equality -- the encoder's blocks, the decoder's payloads, verdicts, corrected counts, iteration
counts and failed codewords on clean, damaged, soft, hopeless, erased and tie-ridden input, lengths that are no block, a
batch of many workgroups, the device-pointer forms, the error codes, and the layer on a link:
ofdm_mod(ldpc=) -> ofdm_demod(ldpc=) clean and through noise, hard and soft.

Soft input (test_decode_soft_from_a_gaussian_channel): BPSK over AWGN, values rint(4 LLR), seed 61, the eight payload
sizes below.  Checked on the CPU in the model first: at Eb/N0 = 3.0 dB every block decodes within 6 iterations; at
1.5 dB the model's blocks take up to 20 iterations, several codewords stop late (block iteration counts above 5) and
codewords fail (cw_failed > 0 in at least one block).  The test asserts both properties of the model before it compares.

CPU pre-check of the impaired link (the float64 channel model of multipath_cases, noise only, fed to the oracle's
receiver, the soft-demapper model of soft_cases behind it and the model decoders behind that): N 512 / occ 200 / CP 128,
four packets of 92, 93, 300 and 188 bytes (rng 2025).
  16-QAM at 12 dB, noise seed 7: the raw packets show 0.7, 1.5, 1.5 and 1.6 % bit errors and the packet CRC fails on all four; the LDPC
  model decodes all four from the soft values in 1, 2, 2 and 2 iterations and from the hard bytes in 1, 2, 2 and 2
  (max_iters / 2 = 10).  The same payloads under fec_cases at the same level and seed: the packet CRC fails on all four
  as well (the K = 7 model also decodes them: at this level the synchroniser, not the code, is what gives up first --
  at 11 dB and below the oracle's receiver loses or gains a flag, with either code).
  QPSK at 9.5 dB, noise seed 12: the packet CRC fails on all four; the LDPC model decodes all four in 1 iteration, soft
  and hard.  Under fec_cases the packet CRC fails on two of the four and the K = 7 model decodes all four.  (Of the
  noise seeds 1 .. 12 at 9.5 dB the other eleven lose or gain a flag or leave a packet CRC intact; at 9 dB all do.)
So on this noise-only link the coding gain does not show: the receiver's synchroniser sets the floor, not either code.
The gain itself is measured on the models."""
import ctypes as C
import functools

import numpy as np
import pytest

import ldpc_cases as lc
from ofdm_uhd_amd import _abi, engine, ldpc, multipath, ofdm, options

pytestmark = pytest.mark.gpu

# k = n + 4: 95 / 96 / 97 either side of one codeword, 192 / 193 either side of two, 2016 = 21 full codewords
SIZES = [0, 1, 91, 92, 93, 188, 189, 2012]
LINK_SIZES = (92, 93, 300, 188)
LINK_LEVELS = {"qpsk": (9.5, 12), "qam16": (12.0, 7)}        # (SNR dB, noise seed): the docstring's pre-check


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(options.default_options(modulation="qpsk"))
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def payloads():
    rng = np.random.default_rng(41)
    return tuple(rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in SIZES)


@functools.lru_cache(maxsize=None)
def blocks():
    return tuple(lc.encode(p) for p in payloads())


def as_model(res):
    return [(int(r[0]),) + tuple(r[1:]) for r in res]


@functools.lru_cache(maxsize=None)
def damaged(rate):
    rng = np.random.default_rng(int(rate * 1000))
    out = []
    for b in blocks():
        bits = np.unpackbits(np.frombuffer(b, np.uint8))
        out.append(np.packbits(bits ^ (rng.random(len(bits)) < rate)).tobytes())
    return tuple(out)


@functools.lru_cache(maxsize=None)
def gaussian(ebn0_db):
    rng = np.random.default_rng(61)
    return tuple(lc.awgn_values(b, ebn0_db, 0.5, rng) for b in blocks())


@functools.lru_cache(maxsize=None)
def model_soft(ebn0_db, max_iters=20):
    return tuple(lc.decode_many(list(gaussian(ebn0_db)), max_iters))


# ---- 1. encoder --------------------------------------------------------------------------------------------------------
def test_encode_one_mixed_batch_and_alone(eng):
    assert eng.ldpc_encode(list(payloads())) == list(blocks())
    assert eng.ldpc_encode([]) == []
    for i in (0, 3, 4, 7):
        assert eng.ldpc_encode([payloads()[i]]) == [blocks()[i]]
    assert eng.ldpc_encode(list(payloads()), dict(max_iters=3)) == list(blocks())     # the encoder ignores max_iters
    assert [len(b) for b in blocks()] == [ldpc.coded_len(n) for n in SIZES]


# ---- 2. decoder --------------------------------------------------------------------------------------------------------
def test_decode_clean(eng):
    got = as_model(eng.ldpc_decode(list(blocks())))
    assert got == [(1, p, 0, 1, 0) for p in payloads()]
    assert got == [lc.decode(b) for b in blocks()]
    for i in (0, 3, 4, 7):
        assert as_model(eng.ldpc_decode([blocks()[i]])) == [(1, payloads()[i], 0, 1, 0)]
    assert as_model(eng.ldpc_decode_soft([lc.hard_values(b) for b in blocks()])) == got
    assert eng.ldpc_decode([]) == []


@pytest.mark.parametrize("rate", [0.02, 0.05])
def test_decode_hard_with_flips_equals_the_model_in_every_field(eng, rate):
    blks = list(damaged(rate))
    got = as_model(eng.ldpc_decode(blks))
    want = [lc.decode(b) for b in blks]
    print("flips %.2f: ok %s corrected %s iters %s failed %s" % (rate, [w[0] for w in want], [w[2] for w in want],
                                                                  [w[3] for w in want], [w[4] for w in want]))
    assert got == want
    assert max(w[3] for w in want) > 1
    if rate == 0.02:
        assert [w[:2] for w in want] == [(1, p) for p in payloads()]
    assert as_model(eng.ldpc_decode([blks[4]])) == [want[4]]


@pytest.mark.parametrize("ebn0_db", [3.0, 1.5])
def test_decode_soft_from_a_gaussian_channel(eng, ebn0_db):
    vals = list(gaussian(ebn0_db))
    want = list(model_soft(ebn0_db))
    print("soft %.1f dB: ok %s corrected %s iters %s failed %s" % (ebn0_db, [w[0] for w in want], [w[2] for w in want],
                                                                   [w[3] for w in want], [w[4] for w in want]))
    if ebn0_db == 1.5:     # the level the docstring chose on the CPU: late stops and failures, in the model
        assert sum(w[3] > 5 for w in want) >= 2 and any(w[4] > 0 for w in want) and any(w[0] for w in want)
    else:
        assert all(w[0] == 1 and w[4] == 0 for w in want)
    assert as_model(eng.ldpc_decode_soft(vals)) == want
    assert as_model(eng.ldpc_decode_soft([vals[5]])) == [want[5]]


def test_max_iters_1_and_64_and_a_stop_exactly_at_the_limit(eng):
    vals = list(gaussian(1.5))
    for it in (1, 64):
        want = list(model_soft(1.5, it))
        assert as_model(eng.ldpc_decode_soft(vals, it)) == want
        assert max(w[3] for w in want) == it
    assert all(w[3] == 1 for w in model_soft(1.5, 1))
    # a block whose last codeword meets its checks after exactly t > 2 iterations: with max_iters = t it stops there
    # with no codeword failed, with t - 1 it is cut off one iteration short
    full = model_soft(1.5, 64)
    i, t = next((i, w[3]) for i, w in enumerate(full) if w[4] == 0 and w[3] > 2)
    at, short = lc.decode_values(vals[i], t), lc.decode_values(vals[i], t - 1)
    assert at == full[i] and at[3] == t and short[3] == t - 1 and short[4] >= 1
    assert as_model(eng.ldpc_decode_soft([vals[i]], t)) == [at]
    assert as_model(eng.ldpc_decode_soft([vals[i]], dict(max_iters=t - 1))) == [short]
    hard = list(damaged(0.05))
    for it in (1, 64):
        assert as_model(eng.ldpc_decode(hard, ldpc.ldpc_cfg(it))) == [lc.decode(b, it) for b in hard]


def test_hopeless_zero_minus_128_and_ties(eng):
    rng = np.random.default_rng(43)
    # random values: nothing to find, every codeword runs to the limit
    noise = [rng.integers(-128, 128, 8 * len(b), dtype=np.int16).astype(np.int8) for b in blocks()]
    for it in (5, 20):
        want = lc.decode_many(noise, it)
        assert all(w[0] == 0 and w[3] == it and w[4] >= 1 for w in want)
        assert as_model(eng.ldpc_decode_soft(noise, it)) == want
    rnd = [rng.integers(0, 256, len(b), dtype=np.uint8).tobytes() for b in blocks()]
    want = [lc.decode(b) for b in rnd]
    assert all(w[0] == 0 for w in want) and want[-1][3] == 20    # (a short block's few sent bits can meet all checks)
    assert as_model(eng.ldpc_decode(rnd)) == want
    # all-zero values: erasures only; every check holds for the zero word after one iteration, and its CRC field is wrong
    # (but for the empty payload, whose CRC-32 is 0)
    zeros = [np.zeros(8 * len(b), np.int8) for b in blocks()]
    want = lc.decode_many(zeros)
    assert want == [want_zero(i) for i in range(len(SIZES))]
    assert as_model(eng.ldpc_decode_soft(zeros)) == want
    # -128 reads as -127: full-scale clean values, and -128 sprinkled over noisy ones
    loud = [np.where(lc.hard_values(b) > 0, 127, -128).astype(np.int8) for b in blocks()]
    assert as_model(eng.ldpc_decode_soft(loud)) == [(1, p, 0, 1, 0) for p in payloads()] == lc.decode_many(loud)
    mixed = []
    for v in gaussian(1.5):
        v = v.copy()
        v[rng.random(len(v)) < 0.05] = -128
        v[rng.random(len(v)) < 0.1] = 0
        mixed.append(v)
    assert as_model(eng.ldpc_decode_soft(mixed)) == lc.decode_many(mixed)
    # many exact ties: values from {-1, 0, 1} (Q = 0 and equal minima everywhere), and a scale up where mu is not 0
    for scale in (1, 2, 5):
        ties = [(scale * rng.integers(-1, 2, 8 * len(b))).astype(np.int8) for b in blocks()]
        assert as_model(eng.ldpc_decode_soft(ties)) == lc.decode_many(ties)
    weak = [(lc.hard_values(b) // 16 * rng.integers(0, 3, 8 * len(b))).astype(np.int8) for b in blocks()]   # right signs, 0 / 1 / 2
    want = lc.decode_many(weak)
    assert as_model(eng.ldpc_decode_soft(weak)) == want and any(w[0] for w in want)
    # a length that is no multiple of 8 values is no block
    assert as_model(eng.ldpc_decode_soft([np.ones(801, np.int8), zeros[1]])) == [lc.NO_BLOCK, want_zero(1)]


def want_zero(i):
    return (int(SIZES[i] == 0), bytes(SIZES[i]), 0, 1, 0)


def test_lengths_that_are_no_block_alone_and_inside_a_batch(eng):
    good = blocks()
    for m in (99, 193, 288, 4033):
        assert ldpc.payload_len(m) is None
        assert as_model(eng.ldpc_decode([bytes(m)])) == [lc.NO_BLOCK]
        assert as_model(eng.ldpc_decode_soft([np.ones(8 * m, np.int8)])) == [lc.NO_BLOCK]
    batch = [good[5], bytes(99), good[7], bytes(193), b"", good[4], bytes(288), bytes(4033), good[1]]
    got = as_model(eng.ldpc_decode(batch))
    for i in (1, 3, 4, 6, 7):
        assert got[i] == lc.NO_BLOCK
    for i, j in ((0, 5), (2, 7), (5, 4), (8, 1)):
        assert got[i] == (1, payloads()[j], 0, 1, 0)
    assert got == [lc.decode(b) for b in batch]
    assert as_model(eng.ldpc_decode([bytes(99), b"", bytes(4033)])) == [lc.NO_BLOCK] * 3          # not one block: no launch


def test_a_batch_of_3000_one_codeword_blocks(eng):
    """750 workgroups of four one-wave codewords; eight distinct blocks, clean and damaged, so the waves of one
    workgroup stop at different iterations."""
    rng = np.random.default_rng(47)
    small = []
    for n, rate in ((0, 0.0), (92, 0.0), (40, 0.03), (92, 0.05), (91, 0.06), (1, 0.08), (92, 0.12), (60, 0.5)):
        b = lc.encode(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
        bits = np.unpackbits(np.frombuffer(b, np.uint8))
        small.append(np.packbits(bits ^ (rng.random(len(bits)) < rate)).tobytes())
    want8 = [lc.decode(b) for b in small]
    assert len({w[3] for w in want8}) >= 4 and want8[0][3] == 1 and want8[-1][:1] == (0,)
    order = rng.integers(0, 8, 3000)
    got = as_model(eng.ldpc_decode([small[i] for i in order]))
    assert got == [want8[i] for i in order]


def test_last_ms(eng):
    eng.prof_enable(False)
    eng.ldpc_encode([b"abc"])
    with pytest.raises(ValueError):
        eng.ldpc_last_ms()                      # the last call ran without profiling
    eng.prof_enable(True)
    try:
        eng.ldpc_encode([b"abc"])
        assert eng.ldpc_last_ms() > 0.0
        eng.ldpc_decode([blocks()[3]])
        assert eng.ldpc_last_ms() > 0.0
        eng.ldpc_decode_soft([lc.hard_values(blocks()[3])])
        assert eng.ldpc_last_ms() > 0.0
        eng.ldpc_decode([bytes(99)])            # nothing launched: no time to report
        with pytest.raises(ValueError):
            eng.ldpc_last_ms()
        assert len(eng.prof()) == _abi.K_COUNT  # the kernel table is what it was
    finally:
        eng.prof_enable(False)


# ---- 3. error codes ------------------------------------------------------------------------------------------------------
def test_error_codes(eng):
    lib, h = eng._lib, eng._h
    u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
    pay = np.frombuffer(bytes(range(200)), np.uint8).copy()
    off = np.array([0, 100], np.uint64)
    ln = np.array([100, 60], np.uint32)
    out = np.zeros(1024, np.uint8)
    coff = np.full(3, 77, np.uint64)

    def enc(cfg, payloads=pay, offs=off, lens=ln, n=2, coded=out, cap=1024, coded_off=coff):
        return lib.ofdm_ldpc_encode(h, C.byref(cfg) if cfg is not None else None,
                                                None if payloads is None else payloads.ctypes.data_as(C.c_void_p),
                                                None if offs is None else offs.ctypes.data_as(u64p),
                                                None if lens is None else lens.ctypes.data_as(u32p), n,
                                                None if coded is None else coded.ctypes.data_as(C.c_void_p), cap,
                                                None if coded_off is None else coded_off.ctypes.data_as(u64p))

    good = ldpc.ldpc_cfg()
    assert enc(good) == _abi.OFDM_OK and coff.tolist() == [0, 296, 456]
    assert enc(None) == _abi.OFDM_OK                                             # cfg NULL: the defaults
    bad_size = _abi.ofdm_ldpc_cfg(struct_size=8, max_iters=20)
    zero, over = ldpc.ldpc_cfg(), ldpc.ldpc_cfg()
    zero.max_iters, over.max_iters = 0, 65
    for cfg in (bad_size, zero, over):
        assert enc(cfg) == _abi.OFDM_E_INVAL
    assert enc(good, lens=np.array([100, 2013], np.uint32)) == _abi.OFDM_E_INVAL  # payload 2013
    for kw in (dict(payloads=None), dict(offs=None), dict(lens=None), dict(coded_off=None), dict(coded=None), dict(n=-1)):
        assert enc(good, **kw) == _abi.OFDM_E_INVAL, kw
    coff[:] = 77
    assert enc(good, cap=455) == _abi.OFDM_E_CAPACITY and coff.tolist() == [0, 296, 456]      # offsets set before the check

    coded = np.frombuffer(blocks()[3] + blocks()[4], np.uint8).copy()
    doff = np.array([0, 192], np.uint64)
    dlen = np.array([192, 289], np.uint32)
    pout = np.zeros(512, np.uint8)
    poff = np.full(3, 77, np.uint64)
    ok, it = np.zeros(2, np.uint8), np.zeros(2, np.uint8)
    corr, failed = np.zeros(2, np.uint32), np.zeros(2, np.uint32)

    def dec(cfg, fn=None, blob=coded, offs=doff, lens=dlen, n=2, pay_out=pout, cap=512, pay_off=poff, ok_=ok, corr_=corr, it_=it,
            failed_=failed):
        p = lambda a, t=C.c_void_p: None if a is None else a.ctypes.data_as(t)
        return (fn or lib.ofdm_ldpc_decode)(h, C.byref(cfg) if cfg is not None else None, p(blob), p(offs, u64p),
                                                        p(lens, u32p), n, p(pay_out), cap, p(pay_off, u64p), p(ok_), p(corr_, u32p),
                                                        p(it_), p(failed_, u32p))

    assert dec(good) == _abi.OFDM_OK and poff.tolist() == [0, 92, 185] and ok.tolist() == [1, 1] and it.tolist() == [1, 1]
    assert pout[:185].tobytes() == payloads()[3] + payloads()[4] and not pout[185:].any()
    assert dec(None) == _abi.OFDM_OK
    for cfg in (bad_size, zero, over):
        assert dec(cfg) == _abi.OFDM_E_INVAL
        assert dec(cfg, fn=lib.ofdm_ldpc_decode_soft) == _abi.OFDM_E_INVAL
    for kw in (dict(blob=None), dict(offs=None), dict(lens=None), dict(pay_off=None), dict(ok_=None), dict(corr_=None),
               dict(it_=None), dict(failed_=None), dict(pay_out=None), dict(n=-1)):
        assert dec(good, **kw) == _abi.OFDM_E_INVAL, kw
    poff[:] = 77
    assert dec(good, cap=184) == _abi.OFDM_E_CAPACITY and poff.tolist() == [0, 92, 185]
    assert lib.ofdm_rx_ldpc_decode_soft(h, None, None, 0, None, None, None, None, None, 0, None) == _abi.OFDM_E_INVAL
    assert lib.ofdm_ldpc_last_ms(h, None) == _abi.OFDM_E_INVAL
    # through the Python layer: the same refusals as exceptions, and the handle stays usable
    with pytest.raises(ValueError):
        eng.ldpc_encode([b"a", bytes(2013)])
    with pytest.raises(ValueError):
        eng.ldpc_encode([b"a"], bad_size)
    with pytest.raises(ValueError):
        eng.ldpc_decode([blocks()[0]], over)
    with pytest.raises(ValueError):
        eng.rx_ldpc_decode_soft()               # no rx() with soft values before it
    assert eng.ldpc_encode([b"a"]) == [lc.encode(b"a")]


def test_device_pointers():
    torch = pytest.importorskip("torch")
    dev = engine.Engine(options.default_options(modulation="qpsk"), device_ptrs=True)
    try:
        idx = (0, 3, 4, 7)
        pay = [payloads()[i] for i in idx]
        blob, offs, lens = engine.pack_payloads(pay)
        d_pay = torch.from_numpy(blob.copy()).cuda()
        d_coded = torch.zeros(8192, dtype=torch.uint8, device="cuda")
        coff = dev.ldpc_encode_device(d_pay.data_ptr(), offs, lens, d_coded.data_ptr(), d_coded.numel())
        coded = d_coded.cpu().numpy()
        want = [blocks()[i] for i in idx]
        assert [coded[int(coff[i]):int(coff[i + 1])].tobytes() for i in range(4)] == want
        assert not coded[int(coff[4]):].any()                                   # nothing behind the last block
        with pytest.raises(engine.EngineError):
            dev.ldpc_encode_device(d_pay.data_ptr(), offs, lens, d_coded.data_ptr(), int(coff[4]) - 1)
        clen = np.diff(coff).astype(np.uint32)
        d_out = torch.full((4096,), 0xEE, dtype=torch.uint8, device="cuda")
        poff, ok, corr, it, failed = dev.ldpc_decode_device(d_coded.data_ptr(), coff[:4].copy(), clen, d_out.data_ptr(), d_out.numel())
        out = d_out.cpu().numpy()
        assert ok.tolist() == [1] * 4 and corr.tolist() == [0] * 4 and it.tolist() == [1] * 4 and failed.tolist() == [0] * 4
        assert [out[int(poff[i]):int(poff[i + 1])].tobytes() for i in range(4)] == pay
        assert (out[int(poff[4]):] == 0xEE).all()                               # nothing written past the payloads
        vals = [gaussian(1.5)[i] for i in idx]
        d_soft = torch.from_numpy(np.concatenate(vals)).cuda()
        res = dev.ldpc_decode_device(d_soft.data_ptr(), (8 * coff[:4]).astype(np.uint64), clen, d_out.data_ptr(), d_out.numel(),
                                     soft=True)
        out = d_out.cpu().numpy()
        got = [(int(res[1][i]), out[int(res[0][i]):int(res[0][i + 1])].tobytes(), int(res[2][i]), int(res[3][i]), int(res[4][i]))
               for i in range(4)]
        assert got == [model_soft(1.5)[i] for i in idx]
    finally:
        dev.close()


# ---- 4. on a link ------------------------------------------------------------------------------------------------------
def _air(iq, tail=512 + 128 + 2 * 512, N=512):
    """The burst with silence around it, as the receiver's tests embed one."""
    return np.concatenate([np.zeros(2 * N, np.complex64), iq, np.zeros(tail, np.complex64)])


@functools.lru_cache(maxsize=None)
def link_payloads():
    rng = np.random.default_rng(2025)
    return tuple(rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in LINK_SIZES)


def _close(*objs):
    for o in objs:
        o.engine().close()


@pytest.mark.parametrize("mod_name", ["qpsk", "qam16"])
def test_clean_loopback_hard_and_soft(mod_name):
    opt = options.default_options(modulation=mod_name)                # N 512 / occ 200 / CP 128
    pay = list(link_payloads())
    mod = ofdm.ofdm_mod(opt, pad_for_usrp=False, ldpc=True)
    seen = []
    hard = ofdm.ofdm_demod(opt, callback=lambda ok, payload: seen.append((ok, payload)), ldpc=True)
    soft = ofdm.ofdm_demod(opt, ldpc=dict(max_iters=20), soft=True)
    plain = ofdm.ofdm_demod(opt)
    try:
        for p in pay:
            mod.send_pkt(p)
        x = _air(mod.flush(), tail=512 + 128)
        assert hard.work(x) == [(True, p) for p in pay] == seen
        assert hard.last_fec == [(True, 0)] * 4 and hard.last_ldpc == [(1, 0)] * 4 and (hard.n_packets, hard.n_ok) == (4, 4)
        assert plain.work(x) == [(True, lc.encode(p)) for p in pay]   # exactly the model's coded blocks on the air
        assert plain.last_fec == [] and plain.last_ldpc == []
        got = soft.work(x)
        want = lc.decode_many(soft.last_soft)
        assert got == [(True, p) for p in pay] == [(bool(w[0]), w[1]) for w in want]
        assert soft.last_fec == [(True, w[2]) for w in want] and soft.last_ldpc == [(w[3], w[4]) for w in want] == [(1, 0)] * 4
        # the chunked path decodes what it delivers, too
        half = len(x) // 2
        assert hard.feed(x[:half]) + hard.feed(x[half:]) + hard.flush() == [(True, p) for p in pay]
        assert soft.feed(x[:half]) + soft.feed(x[half:]) + soft.flush() == [(True, p) for p in pay]
    finally:
        _close(mod, hard, soft, plain)


@pytest.mark.parametrize("mod_name", ["qpsk", "qam16"])
def test_impaired_link_equals_the_model_and_every_packet_comes_back(mod_name):
    """Noise only, at the level and seed the file's docstring derives on the CPU.  Exact part: the hard result is the model
    applied to what ofdm_demod without a code returns, the soft result is the model applied to the engine's own last_soft
    values, in every field.  Physical part: every packet comes back ok from the soft values, though the packet CRC
    failed (the pre-check)."""
    snr_db, seed = LINK_LEVELS[mod_name]
    opt = options.default_options(modulation=mod_name)
    pay = list(link_payloads())
    mod = ofdm.ofdm_mod(opt, pad_for_usrp=False, ldpc=True)
    hard = ofdm.ofdm_demod(opt, ldpc=True)
    soft = ofdm.ofdm_demod(opt, ldpc=True, soft=True)
    plain = ofdm.ofdm_demod(opt)
    try:
        for p in pay:
            mod.send_pkt(p)
        iq = mod.flush()
        psig = float(np.mean(np.abs(iq.astype(np.complex128)) ** 2))
        ch = mod.engine()
        ch.set_multipath(multipath.multipath_cfg(sigma=multipath.sigma_for_snr(snr_db, psig), seed=seed))
        y = ch.multipath(_air(iq))
        raw = plain.work(y)
        assert len(raw) == len(pay)
        want = [lc.decode(p) for _, p in raw]
        assert hard.work(y) == [(bool(w[0]), w[1]) for w in want]
        assert hard.last_fec == [(bool(ok), w[2]) for (ok, _), w in zip(raw, want)]
        assert hard.last_ldpc == [(w[3], w[4]) for w in want]
        got = soft.work(y)
        swant = lc.decode_many(soft.last_soft)
        print("impaired %s: outer ok %s, hard ok %s iters %s, soft ok %s corrected %s iters %s" % (
            mod_name, [int(ok) for ok, _ in raw], [w[0] for w in want], [w[3] for w in want], [w[0] for w in swant],
            [w[2] for w in swant], [w[3] for w in swant]))
        assert got == [(bool(w[0]), w[1]) for w in swant]
        assert soft.last_fec == [(bool(ok), w[2]) for (ok, _), w in zip(raw, swant)]
        assert soft.last_ldpc == [(w[3], w[4]) for w in swant]
        assert got == [(True, p) for p in pay]                        # every packet comes back
        assert all(w[3] <= 10 for w in swant) and soft.n_ok == len(pay)
    finally:
        _close(mod, hard, soft, plain)


def test_rs_above_ldpc_clean():
    opt = options.default_options(modulation="qpsk")
    rng = np.random.default_rng(53)
    pay = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (0, 92, 93, 1752)]
    mod = ofdm.ofdm_mod(opt, pad_for_usrp=False, ldpc=True, rs=True)
    dem = ofdm.ofdm_demod(opt, ldpc=True, rs=True)
    try:
        for p in pay[:2]:
            mod.send_pkt(p)
        with pytest.raises(ValueError):
            mod.send_pkt(bytes(1753))                                   # the RS block would not fit the inner code
        for p in pay[2:]:
            mod.send_pkt(p)
        x = _air(mod.flush(), tail=512 + 128)
        assert dem.work(x) == [(True, p) for p in pay]
        assert dem.last_fec == [(True, 0)] * 4 and dem.last_rs == [(True, 0, 0)] * 4
        assert [it for it, _ in dem.last_ldpc] == [1] * 4 and [f for _, f in dem.last_ldpc] == [0] * 4
    finally:
        _close(mod, dem)


def test_value_errors_of_the_link_objects():
    opt = options.default_options(modulation="qpsk")
    with pytest.raises(ValueError):
        ofdm.ofdm_mod(opt, pad_for_usrp=False, ldpc=True, fec=True)
    with pytest.raises(ValueError):
        ofdm.ofdm_demod(opt, ldpc=True, fec=True)
    with pytest.raises(ValueError):
        ofdm.ofdm_demod(opt, ldpc=True, soft=True, rs=dict(erasures=True))
    with pytest.raises(ValueError):
        ofdm.ofdm_demod(opt, ldpc=True, rs=dict(erasures=True, source="fec"))
    with pytest.raises(ValueError):
        ofdm.ofdm_mod(opt, pad_for_usrp=False, ldpc=dict(max_iters=0))
    mod = ofdm.ofdm_mod(opt, pad_for_usrp=False, ldpc=True)
    try:
        mod.send_pkt(bytes(2012))
        with pytest.raises(ValueError):
            mod.send_pkt(bytes(2013))                                   # payload too long, the offending packet only
        assert len(mod.flush()) > 0
    finally:
        _close(mod)
