"""The outer code on the GPU (csrc/rs.h: k_rs_encode, k_rs_decode).  Everything is integer arithmetic, so every result
is compared with the NumPy model of tests/rs_cases.py by equality, in every field: the encoder's blocks; the decoder's
payloads, verdicts, corrected and failed counts on clean, damaged, miscorrecting and hopeless input; lengths that are no
block; batches with many more codewords than one workgroup holds; the device-pointer forms with a guard region and the
chained ofdm_fec_decode -> ofdm_rs_decode call; refusals; the timing accessor; and the layer on a link: clean loopbacks
at N = 64, the two command-line tools with --rs, and the impaired link of soft_cases.

CPU pre-check of the impaired link (rs_cases.link_on_the_cpu: RS blocks inside the model's punctured blocks through the
oracle's transmitter, the float64 channel model of multipath_cases, the oracle's receiver with its taps, the soft model,
the model inner decoders at the rate, the RS model on what they return): 16-QAM, N 512 / occ 200 / CP 128, packets of
300, 301, 257, 400, 333, 300 bytes (RS blocks of 368, 369, 325, 468, 401, 368), paths (0, 1.0) and (9, 0.8 exp(2.1j)),
scale 32.  The grid searched, the points taken and the outcome per packet are listed at LINK_CASES below."""
import ctypes as C
import functools

import numpy as np
import pytest

import punct_cases as pc
import rs_cases as rc
import soft_cases as sc
from ofdm_uhd_amd import _abi, engine, ofdm, options, rs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(options.default_options(modulation="qpsk"))
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def payloads():
    rng = np.random.default_rng(255)
    return tuple(rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in rc.SIZES)


@functools.lru_cache(maxsize=None)
def blocks():
    return tuple(rc.encode(p) for p in payloads())


@functools.lru_cache(maxsize=None)
def model_decode(block):
    """The model's answer, computed once per distinct block."""
    return rc.decode(block)


def as_model(res):
    return [(int(ok), p, c, f) for ok, p, c, f in res]


def check(eng, batch):
    got = as_model(eng.rs_decode(batch))
    want = [model_decode(b) for b in batch]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, len(batch[i]), g[0], g[2:], w[0], w[2:])
    return want


# ---- 1. encoder ---------------------------------------------------------------------------------------------------------
def test_encode_equals_the_model(eng):
    got = eng.rs_encode(list(payloads()))
    assert [len(b) for b in got] == [rs.coded_len(n) for n in rc.SIZES]
    for g, w, p in zip(got, blocks(), payloads()):
        assert g == w and g[:len(p)] == p                                   # the model's block; systematic
    assert eng.rs_encode([]) == []
    # the same payloads at other places of the blob: every source and destination alignment of the 16-byte staging
    rev = list(payloads())[::-1] + [b"x", b"yz"] + list(payloads()[2:5])
    assert eng.rs_encode(rev) == [rc.encode(p) for p in rev]


# ---- 2. decoder ---------------------------------------------------------------------------------------------------------
def test_decode_clean(eng):
    want = check(eng, list(blocks()))
    assert want == [(1, p, 0, 0) for p in payloads()]


@pytest.mark.parametrize("percent", [1, 10])
def test_decode_seeded_byte_errors(eng, percent):
    rng = np.random.default_rng(percent)
    batch = []
    for b in blocks():
        where = np.flatnonzero(rng.integers(0, 100, len(b)) < percent)
        batch.append(rc.damage(b, where, rng))
    want = check(eng, batch)
    print("%d %%: ok %s corrected %s failed %s" % (percent, [w[0] for w in want], [w[2] for w in want], [w[3] for w in want]))
    if percent == 1:
        assert all(w[0] == 1 for w in want) and sum(w[2] for w in want) > 50
    else:
        assert any(w[3] for w in want) and any(w[2] for w in want)          # 25 of 255 is past t: most long words fail


@pytest.mark.parametrize("count", [16, 17])
def test_decode_errors_per_codeword(eng, count):
    rng = np.random.default_rng(count)
    batch = [rc.errors_per_codeword(b, count, rng) for b in blocks()]
    want = check(eng, batch)
    for w, p, sent, got in zip(want, payloads(), blocks(), batch):
        k = len(p) + 4
        W = rc.words(k)
        if count == 16:
            assert w == (1, p, 16 * W, 0)
        else:                                                               # every codeword fails, the bytes stay
            assert w == (int(got[:k] == sent[:k]), got[:len(p)], 0, W)


def test_decode_the_constructed_miscorrection(eng):
    batch, others = [], []
    for i, b in enumerate(blocks()):
        W = rc.words(len(payloads()[i]) + 4)
        m, other = rc.miscorrection(b, w=i % W, seed=i)
        batch.append(m)
        others.append(other)
    want = check(eng, batch)
    for w, o in zip(want, others):
        assert (w[0], w[2], w[3]) == (0, 16, 0) and w[1] == o[:len(w[1])]  # the OTHER codeword's bytes, CRC failing


def test_decode_bursts(eng):
    b = blocks()[rc.SIZES.index(443)]                                       # k = 447, W = 3, 543 bytes
    k, W = 447, 3
    batch = [rc.damage(b, np.arange(s, s + 15 * W + 1), xor=0xFF) for s in range(0, len(b) - 15 * W, 7)]
    batch += [rc.damage(b, np.arange(s, s + 16 * W), xor=0x5A) for s in (0, 100, k - 16 * W, k, len(b) - 16 * W)]
    n_ok = len(batch)
    batch += [rc.damage(b, np.arange(s, s + 16 * W + 1), xor=0x01) for s in (0, 200, k - 16 * W - 1)]
    want = check(eng, batch)
    assert all(w[:2] == (1, payloads()[rc.SIZES.index(443)]) and w[3] == 0 for w in want[:n_ok])
    assert all(w[3] == 1 and w[0] == 0 for w in want[n_ok:])               # exactly one codeword fails
    big = blocks()[-1]                                                      # W = 16: 241 bytes in a row
    assert check(eng, [rc.damage(big, np.arange(s, s + 241), xor=0x80) for s in (0, 1777, 3500, len(big) - 241)]) == \
        [(1, payloads()[-1], 241, 0)] * 4


def test_decode_garbage_and_zeros(eng):
    rng = np.random.default_rng(99)
    lens = [len(b) for b in blocks()] + [36, 37, 40, 50, 64, 100] * 8
    batch = [rng.integers(0, 256, m, dtype=np.uint8).tobytes() for m in lens]
    want = check(eng, batch)
    assert all(w[0] == 0 for w in want)
    assert sum(w[3] for w in want) >= sum(rc.words(rc.payload_len(m) + 4) for m in lens) - 2     # (nearly) every word fails
    short = want[len(blocks()):]
    assert sum(w[3] for w in short) >= len(short) - 1                       # the shortened region refuses them
    zeros = [bytes(len(b)) for b in blocks()]
    # all zeros is a codeword whose CRC fails (but for n = 0: the CRC-32 of nothing is 0)
    assert check(eng, zeros) == [(int(n == 0), bytes(n), 0, 0) for n in rc.SIZES]


def test_lengths_that_are_no_block(eng):
    rng = np.random.default_rng(5)
    junk = [rng.integers(0, 256, m, dtype=np.uint8).tobytes() for m in (0, 1, 35, 256, 287, 2041, 2072, 4081, 4091)]
    good = blocks()
    batch = [good[3], junk[0], good[10], junk[1], junk[2], good[0], junk[3], junk[4], good[8], junk[5], junk[6], junk[7], junk[8], good[5]]
    want = check(eng, batch)
    for i in (1, 3, 4, 6, 7, 9, 10, 11, 12):
        assert want[i] == (0, b"", 0, 0)
    assert want[0] == (1, payloads()[3], 0, 0) and want[13] == (1, payloads()[5], 0, 0)
    assert as_model(eng.rs_decode(junk)) == [(0, b"", 0, 0)] * len(junk)    # not one block: no launch
    assert eng.rs_decode([]) == []


def test_many_blocks_in_one_call(eng):
    """5 000 blocks of n = 3 and 600 of n = 1 780 (W = 8: one full pass of a workgroup's eight halves): many more
    codewords than one workgroup's waves; some clean, some damaged, some hopeless."""
    rng = np.random.default_rng(12)
    small = rc.encode(b"abc")
    kinds_s = [small, rc.damage(small, [0, 5, 38], rng), rc.errors_per_codeword(small, 16, rng), rc.errors_per_codeword(small, 17, rng)]
    big = blocks()[rc.SIZES.index(1780)]
    kinds_b = [big, rc.errors_per_codeword(big, 5, rng), rc.damage(big, np.arange(700, 700 + 8 * 15 + 1), rng),
               rc.errors_per_codeword(big, 17, rng)]
    batch = [kinds_s[i % 4] for i in range(5000)] + [kinds_b[(i * 7) % 4] for i in range(600)]
    got = as_model(eng.rs_decode(batch))
    assert got == [model_decode(b) for b in batch]
    assert got[0] == (1, b"abc", 0, 0) and got[1] == (1, b"abc", 3, 0) and got[5000] == (1, payloads()[rc.SIZES.index(1780)], 0, 0)
    enc = eng.rs_encode([b"abc"] * 5000 + [payloads()[rc.SIZES.index(1780)]] * 600)
    assert enc[:5000] == [small] * 5000 and enc[5000:] == [big] * 600


# ---- 3. device pointers ---------------------------------------------------------------------------------------------------
def test_device_pointers_and_the_chain_with_the_inner_code():
    torch = pytest.importorskip("torch")
    dev = engine.Engine(options.default_options(modulation="qpsk"), device_ptrs=True)
    try:
        idx = (0, 2, 4, 7, 9)
        pay = [payloads()[i] for i in idx]
        want = [blocks()[i] for i in idx]
        blob, offs, lens = engine.pack_payloads(pay)
        d_pay = torch.from_numpy(blob.copy()).cuda()
        total = sum(len(b) for b in want)
        d_rs = torch.full((total + 64,), 0xEE, dtype=torch.uint8, device="cuda")
        coff = dev.rs_encode_device(d_pay.data_ptr(), offs, lens, d_rs.data_ptr(), total)
        got = d_rs.cpu().numpy()
        assert [got[int(coff[i]):int(coff[i + 1])].tobytes() for i in range(len(idx))] == want
        assert int(coff[-1]) == total and (got[total:] == 0xEE).all()      # the guard behind the blocks is untouched
        with pytest.raises(engine.EngineError):
            dev.rs_encode_device(d_pay.data_ptr(), offs, lens, d_rs.data_ptr(), total - 1)
        # encode side of the chain: the RS blob and its offsets are the inner encoder's payloads
        rlen = np.diff(coff).astype(np.uint32)
        fcfg = dict(rate="3/4")
        d_air = torch.zeros(2 * total + 64, dtype=torch.uint8, device="cuda")
        aoff = dev.fec_encode_device(d_rs.data_ptr(), coff[:len(idx)].copy(), rlen, d_air.data_ptr(), d_air.numel(), fcfg)
        air = d_air.cpu().numpy()
        assert [air[int(aoff[i]):int(aoff[i + 1])].tobytes() for i in range(len(idx))] == [pc.encode(b, 16, "3/4") for b in want]
        # damage on the air that the inner code cannot take (runs of 3 and 8 inverted bytes: the interleaver spreads them,
        # the Viterbi decoder returns 18 and 48 wrong bytes), and some it can (one bit)
        air[int(aoff[3]) + 20:int(aoff[3]) + 23] ^= 0xFF
        air[int(aoff[4]) + 20:int(aoff[4]) + 28] ^= 0xFF
        air[int(aoff[1]) + 7] ^= 0x10
        d_air.copy_(torch.from_numpy(air))
        alen = np.diff(aoff).astype(np.uint32)
        d_mid = torch.full((total + 64,), 0xEE, dtype=torch.uint8, device="cuda")
        moff, ok_in, corr_in = dev.fec_decode_device(d_air.data_ptr(), aoff[:len(idx)].copy(), alen, d_mid.data_ptr(), total, fcfg)
        inner = [pc.decode(air[int(aoff[i]):int(aoff[i + 1])].tobytes(), 16, "3/4") for i in range(len(idx))]
        assert ok_in.tolist() == [w[0] for w in inner] == [1, 1, 1, 0, 0] and corr_in.tolist()[1] == 1
        # decode side of the chain: the inner decoder's output blob and offsets go straight in; no host copy between
        n_pay = sum(len(p) for p in pay)
        d_out = torch.full((n_pay + 64,), 0xEE, dtype=torch.uint8, device="cuda")
        poff, ok, corr, fail = dev.rs_decode_device(d_mid.data_ptr(), moff[:len(idx)].copy(), np.diff(moff).astype(np.uint32),
                                                    d_out.data_ptr(), n_pay)
        out = d_out.cpu().numpy()
        model = [rc.decode(w[1]) for w in inner]
        assert [(int(ok[i]), out[int(poff[i]):int(poff[i + 1])].tobytes(), int(corr[i]), int(fail[i])) for i in range(len(idx))] == model
        assert model == [(1, pay[0], 0, 0), (1, pay[1], 0, 0), (1, pay[2], 0, 0), (1, pay[3], 18, 0), (1, pay[4], 48, 0)]
        assert (out[n_pay:] == 0xEE).all() and (d_mid.cpu().numpy()[total:] == 0xEE).all()      # guards untouched
        with pytest.raises(engine.EngineError):
            dev.rs_decode_device(d_mid.data_ptr(), moff[:len(idx)].copy(), np.diff(moff).astype(np.uint32), d_out.data_ptr(), n_pay - 1)
    finally:
        dev.close()


# ---- 4. refusals, timing ----------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable(eng):
    lib, h = eng._lib, eng._h
    with pytest.raises(ValueError):
        eng.rs_encode([b"ok", bytes(3565)])
    assert eng.rs_encode([bytes(3564)]) == [rc.encode(bytes(3564))]
    blob, offs, lens = engine.pack_payloads([b"abc", b"defgh"])
    u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
    out = np.zeros(200, np.uint8)
    coff = np.zeros(3, np.uint64)
    args = [h, blob.ctypes.data, offs.ctypes.data_as(u64p), lens.ctypes.data_as(u32p), 2, out.ctypes.data, 200, coff.ctypes.data_as(u64p)]
    for null in (1, 2, 3, 5, 7):
        a = list(args)
        a[null] = None
        assert lib.ofdm_rs_encode(*a) == _abi.OFDM_E_INVAL
    a = list(args)
    a[6] = 79                                                               # 39 + 41 = 80 needed
    assert lib.ofdm_rs_encode(*a) == _abi.OFDM_E_CAPACITY and coff.tolist() == [0, 39, 80]
    assert lib.ofdm_rs_encode(*args) == _abi.OFDM_OK
    assert out[:80].tobytes() == rc.encode(b"abc") + rc.encode(b"defgh")
    clen = np.array([39, 41], np.uint32)
    pay = np.zeros(16, np.uint8)
    poff = np.full(3, 77, np.uint64)
    ok, corr, fail = np.zeros(2, np.uint8), np.zeros(2, np.uint32), np.zeros(2, np.uint32)
    dargs = [h, out.ctypes.data, coff.ctypes.data_as(u64p), clen.ctypes.data_as(u32p), 2, pay.ctypes.data, 16, poff.ctypes.data_as(u64p),
             ok.ctypes.data, corr.ctypes.data_as(u32p), fail.ctypes.data_as(u32p)]
    for null in (1, 2, 3, 5, 7, 8, 9, 10):
        a = list(dargs)
        a[null] = None
        assert lib.ofdm_rs_decode(*a) == _abi.OFDM_E_INVAL
    a = list(dargs)
    a[6] = 7
    assert lib.ofdm_rs_decode(*a) == _abi.OFDM_E_CAPACITY and poff.tolist() == [0, 3, 8]
    assert lib.ofdm_rs_decode(*dargs) == _abi.OFDM_OK
    assert pay[:8].tobytes() == b"abcdefgh" and ok.tolist() == [1, 1] and corr.tolist() == [0, 0] and fail.tolist() == [0, 0]
    assert lib.ofdm_rs_encode(None, *args[1:]) == _abi.OFDM_E_INVAL
    check(eng, list(blocks()[:4]))


def test_rs_last_ms():
    e = engine.Engine(options.default_options(modulation="qpsk"))
    try:
        e.prof_enable(True)
        with pytest.raises(ValueError):
            e.rs_last_ms()                              # no rs call yet
        blk = e.rs_encode([b"abc"])
        assert e.rs_last_ms() > 0.0
        e.rs_decode([bytes(35)])                        # 35 is no block: nothing launched, no time to report
        with pytest.raises(ValueError):
            e.rs_last_ms()
        e.rs_decode(blk)
        assert e.rs_last_ms() > 0.0
        e.prof_enable(False)
        e.rs_decode(blk)
        with pytest.raises(ValueError):
            e.rs_last_ms()                              # the last call ran without profiling
        assert len(e.prof()) == _abi.K_COUNT            # the kernel table is what it was
    finally:
        e.close()


# ---- 5. on a link -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fcfg,soft", [(None, False), (True, False), (dict(rate="3/4"), True)], ids=["rs", "rs+fec", "rs+fec34+soft"])
def test_clean_loopback(fcfg, soft):
    N, CP = 64, 16
    opt = options.default_options(modulation="qpsk", fft_length=N, occupied_tones=48, cp_length=CP)
    rng = np.random.default_rng(147)
    pay = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (59, 180, 1, 148, 0)]
    mod = ofdm.ofdm_mod(opt, pad_for_usrp=False, fec=fcfg, rs=True)
    seen = []
    dem = ofdm.ofdm_demod(opt, callback=lambda ok, p: seen.append((ok, p)), fec=fcfg, soft=soft, rs=True)
    plain = ofdm.ofdm_demod(opt)
    try:
        for p in pay[:2]:
            mod.send_pkt(p)
        with pytest.raises(ValueError):
            mod.send_pkt(bytes(1781 if fcfg else 3565))                     # the offending packet only
        for p in pay[2:]:
            mod.send_pkt(p)
        x = np.concatenate([np.zeros(2 * N, np.complex64), mod.flush(), np.zeros(N + CP, np.complex64)])
        blocks_ = [rc.encode(p) for p in pay]
        if fcfg:
            blocks_ = [pc.encode(b, 16, "3/4" if isinstance(fcfg, dict) else "1/2") for b in blocks_]
        assert plain.work(x) == [(True, b) for b in blocks_]                # outer, then inner, then the modulator
        assert dem.work(x) == [(True, p) for p in pay] == seen
        assert dem.last_rs == [(True, 0, 0)] * len(pay) and (dem.n_packets, dem.n_ok) == (len(pay), len(pay))
        if fcfg:
            assert dem.last_fec == [(True, 0)] * len(pay)
        half = len(x) // 2                                                  # the chunked path decodes what it delivers, too
        assert dem.feed(x[:half]) + dem.feed(x[half:]) + dem.flush() == [(True, p) for p in pay]
    finally:
        for o in (mod, dem, plain):
            o.engine().close()


def test_the_command_line_takes_rs(tmp_path):
    """benchmark_ofdm_tx --rs --fec-rate 3/4 -> file -> benchmark_ofdm_rx --rs --fec-rate 3/4, hard and with --fec-soft."""
    from ofdm_uhd_amd import benchmark_ofdm_rx, benchmark_ofdm_tx, iqio
    src = tmp_path / "tx.bin"
    data = np.random.default_rng(0).integers(0, 256, 20000, dtype=np.uint8).tobytes()
    src.write_bytes(data)
    iqf, plain_iqf = str(tmp_path / "tx.dat"), str(tmp_path / "tx_norss.dat")
    npk = benchmark_ofdm_tx.main(["--from-file", str(src), "--to-file", iqf, "-M", "1.0", "-s", "1024", "--rs", "--fec-rate", "3/4"])
    assert npk == benchmark_ofdm_tx.main(["--from-file", str(src), "--to-file", plain_iqf, "-M", "1.0", "-s", "1024", "--fec-rate", "3/4"])
    iq = iqio.read_complex_binary(iqf)
    assert len(iqio.read_complex_binary(plain_iqf)) < len(iq) < 1.25 * len(iqio.read_complex_binary(plain_iqf))
    rng = np.random.default_rng(1)                                               # a noise floor and a tail, as the receiver needs
    x = np.concatenate([np.zeros(1024, np.complex64), iq, np.zeros(2048, np.complex64)])
    x += ((rng.standard_normal(len(x)) + 1j * rng.standard_normal(len(x))) * 1e-3).astype(np.complex64)
    iqio.file_sink(iqf).write(x)
    for extra in ([], ["--fec-soft"]):
        out = str(tmp_path / ("rx%d.bin" % len(extra)))
        acct = benchmark_ofdm_rx.main(["--from-file", iqf, "--to-file", out, "--rs", "--fec-rate", "3/4"] + extra)
        assert acct.n_rcvd == npk and acct.n_right == npk
        assert open(out, "rb").read() == data


# ---- 6. the impaired link -------------------------------------------------------------------------------------------------
# The grid, searched on the CPU with rs_cases.link_on_the_cpu and bounded as follows: noise seeds 7 .. 12, 10 .. 20 dB in
# 1 dB steps, rates 1/2, 2/3 and 3/4, hard and soft: 198 points, at 193 of them the receiver's packet list is the six
# packets (not at seed 9 rate 2/3 10 dB, seed 11 rates 1/2 and 2/3 10 dB, seed 12 rate 1/2 10 and 11 dB).  Packets decoded
# to the payload sent, inner code alone > concatenated, noise seed 7:
#            hard                                            soft
#   1/2  10 dB 010000 > 110101   11 dB 110000 > 111101       10 dB 111101 > 111101   11 dB 111101 > 111111
#        12 dB 110101 > 111111   13 dB 111101 > 111111       12 dB on: all six either way
#        14 dB on: all six either way
#   2/3  10 dB 000000 > 000000   11 dB 000000 > 001000       10 dB 001000 > 111001   11 dB 101011 > 111011
#        12 dB 000000 > 101000   13 dB 000000 > 101011       12 dB 101011 > 111111   13 dB 111011 > 111111
#        14 dB 101000 > 101111   15 dB 101000 > 111111       14 dB on: all six either way
#        16 .. 20 dB 101110 > 111111
#   3/4  10 .. 12 dB 000000 > 000000                         10 dB 000000 > 101000   11 dB 101000 > 101000
#        13 dB 000000 > 100000   14 dB 000000 > 101000       12 dB 101000 > 101100   13 dB 101100 > 101101
#        15 dB 100000 > 101001   16 dB 100000 > 101101       14 dB 101101 > 111101   15 dB 101101 > 111111
#        17, 18 dB 100001 > 101111                           16, 17 dB 101111 > 111111
#        19 dB 100101 > 101111   20 dB 100111 > 101111       18 dB on: all six either way
# Over all six seeds the concatenation never returned fewer packets than the inner code alone, and no decoder reported
# ok for a wrong payload; 38 points are "hard points" (the inner code alone loses at least two, the concatenation
# returns all six) and 11 are "soft points" (seeds 7 .. 11, rates 2/3 and 3/4, 10 .. 15 dB).
# Taken: the hard point rate 2/3, 15 dB (wrong bytes behind the inner decoder: 0, 30, 0, 6, 7, 10: all corrected); the
# soft point rate 3/4, 15 dB (soft: 0, 23, 0, 0, 17, 0 wrong bytes, corrected; hard there: 0, 164, 19, 52, 56, 24, three
# packets lose two codewords each); and rate 3/4, 17 dB, where hard packet 1 (159 wrong bytes) loses both its codewords
# and comes back ok = 0 with the inner decoder's bytes, while soft (12 wrong bytes) corrects it.
# Per packet: (inner ok, concatenated ok, symbols corrected, codewords failed), hard then soft.
LINK_CASES = {
    (15.0, "2/3"): (((1, 1, 0, 0), (0, 1, 30, 0), (1, 1, 0, 0), (0, 1, 6, 0), (0, 1, 7, 0), (0, 1, 10, 0)),
                    ((1, 1, 0, 0),) * 6),
    (15.0, "3/4"): (((1, 1, 0, 0), (0, 0, 0, 2), (0, 1, 19, 0), (0, 0, 0, 2), (0, 0, 0, 2), (0, 1, 24, 0)),
                    ((1, 1, 0, 0), (0, 1, 23, 0), (1, 1, 0, 0), (1, 1, 0, 0), (0, 1, 17, 0), (1, 1, 0, 0))),
    (17.0, "3/4"): (((1, 1, 0, 0), (0, 0, 0, 2), (0, 1, 7, 0), (0, 1, 9, 0), (0, 1, 18, 0), (1, 1, 0, 0)),
                    ((1, 1, 0, 0), (0, 1, 12, 0), (1, 1, 0, 0), (1, 1, 0, 0), (1, 1, 0, 0), (1, 1, 0, 0))),
}
TAPS = (_abi.TAP_RX_FFT, _abi.TAP_RX_SINK, _abi.TAP_RX_DEMAPPED)


@functools.lru_cache(maxsize=None)
def link_case(snr_db, rate, seed=sc.LINK_SEED):
    """The link of soft_cases at one level and rate with the outer code around the payloads: one receive call with
    everything the soft model needs, and what ofdm_demod(fec=, rs=True) returns hard and soft."""
    opt = options.default_options(modulation=sc.LINK_MOD, fft_length=sc.LINK_N, occupied_tones=sc.LINK_OCC, cp_length=sc.LINK_CP)
    pay = list(sc.link_payloads())
    fcfg = dict(rate=rate)
    mod = ofdm.ofdm_mod(opt, pad_for_usrp=False, fec=fcfg, rs=True)
    hard = ofdm.ofdm_demod(opt, fec=fcfg, rs=True)
    soft = ofdm.ofdm_demod(opt, fec=fcfg, soft=True, rs=True)
    eng = engine.Engine(opt)
    try:
        for p in pay:
            mod.send_pkt(p)
        iq = mod.flush()
        psig = float(np.mean(np.abs(iq.astype(np.complex128)) ** 2))
        ch = mod.engine()
        ch.set_multipath(sc.link_channel_cfg(snr_db, psig, seed))
        y = ch.multipath(sc.link_air(iq))
        eng.set_taps(*TAPS)
        eng.set_rx_quality(True)
        eng.set_rx_csi(True)
        eng.set_rx_soft(True)
        pk = eng.rx(y)
        vals = sc.call_values(eng.cfg, pk, eng.rx_quality(), eng.rx_csi()["eq"], eng.tap(_abi.TAP_RX_SINK), eng.tap(_abi.TAP_RX_DEMAPPED))
        got_h, got_s = hard.work(y), soft.work(y)
        return dict(pay=pay, nsamp=len(iq), pk=pk, vals=vals, got_h=got_h, got_s=got_s, fec_h=list(hard.last_fec), fec_s=list(soft.last_fec),
                    rs_h=list(hard.last_rs), rs_s=list(soft.last_rs), n_ok=(hard.n_ok, soft.n_ok))
    finally:
        for o in (mod, hard, soft):
            o.engine().close()
        eng.close()


@pytest.mark.parametrize("snr_db,rate", sorted(LINK_CASES), ids=["%.0f-%s" % c for c in sorted(LINK_CASES)])
def test_impaired_link(snr_db, rate):
    """Exact, twice.  Against the models fed with the same call's packets and soft values: ofdm_demod(fec=, rs=True), hard
    and soft, equals the inner model decoder followed by the RS model in every field (payloads, last_fec, last_rs).
    Against the CPU pre-check: per packet the outcome listed at LINK_CASES, and every ok payload is the one sent."""
    r = link_case(snr_db, rate)
    pk, pay = r["pk"], r["pay"]
    assert [len(p) for _, p in pk] == [pc.coded_len(rc.coded_len(len(p)), rate) for p in pay]          # the six packets
    for side, inner, key in (("hard", [pc.decode(p, 16, rate) for _, p in pk], "h"),
                             ("soft", [pc.decode_values(v, 16, rate) for v in r["vals"]], "s")):
        outer = [rc.decode(i[1]) for i in inner]
        print("link at %.0f dB rate %s %s: %d samples, packet CRC %s, inner ok %s corrected %s, outer ok %s corrected %s failed %s" % (
            snr_db, rate, side, r["nsamp"], [int(ok) for ok, _ in pk], [i[0] for i in inner], [i[2] for i in inner],
            [o[0] for o in outer], [o[2] for o in outer], [o[3] for o in outer]))
        assert r["got_" + key] == [(bool(o[0]), o[1]) for o in outer]
        assert r["fec_" + key] == [(bool(ok), i[2]) for (ok, _), i in zip(pk, inner)]
        assert r["rs_" + key] == [(bool(i[0]), o[2], o[3]) for i, o in zip(inner, outer)]
        want = LINK_CASES[(snr_db, rate)][0 if key == "h" else 1]
        assert tuple((i[0], o[0], o[2], o[3]) for i, o in zip(inner, outer)) == want
        for o, sent in zip(outer, pay):
            assert not o[0] or o[1] == sent
    assert r["n_ok"] == tuple(sum(w[1] for w in side) for side in LINK_CASES[(snr_db, rate)])


def test_impaired_link_the_outer_code_returns_what_the_inner_code_loses():
    hard, soft = LINK_CASES[(15.0, "2/3")], LINK_CASES[(15.0, "3/4")]
    r = link_case(15.0, "2/3")
    inner_ok = sum(1 for ok, _, _ in r["rs_h"] if ok)
    assert inner_ok == sum(w[0] for w in hard[0]) == 2 and r["got_h"] == [(True, p) for p in r["pay"]]   # two of six become six of six
    r = link_case(15.0, "3/4")
    assert sum(1 for ok, _, _ in r["rs_s"] if ok) == sum(w[0] for w in soft[1]) == 4 and r["got_s"] == [(True, p) for p in r["pay"]]
    r = link_case(17.0, "3/4")                                             # a codeword that fails: ok = 0, the inner decoder's bytes
    inner = pc.decode(r["pk"][1][1], 16, "3/4")
    assert r["got_h"][1] == (False, inner[1][:len(r["pay"][1])]) and r["rs_h"][1] == (False, 0, 2) and r["got_s"][1] == (True, r["pay"][1])
