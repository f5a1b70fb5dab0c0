"""Punctured rates of the coded links on the GPU (csrc/fec_punct.h: k_fec_puncture, k_fec_depuncture in front of the
unchanged k_fec_decode; ofdm_fec_cfg.rate).  Everything is integer arithmetic, so every result is compared with the
NumPy model of tests/punct_cases.py by equality, in every field: the encoder's blocks, the decoder's payloads, verdicts
and corrected counts on clean, damaged and hopeless input, soft input with zeros, ties and -128, lengths that are no
block at the rate, a batch wider than one workspace slice, the device-pointer forms, rate 1/2 through the new field,
the timing accessor, and the layer on a link: clean loopbacks at N = 64, the two command-line tools with --fec-rate, and
the impaired link of soft_cases.

CPU pre-check of the impaired link (punct_cases.link_on_the_cpu: the punctured blocks through the oracle's transmitter,
the float64 channel model of multipath_cases, the oracle's receiver with its taps, the soft model, the model decoders at
the rate): 16-QAM, N 512 / occ 200 / CP 128, packets of 300, 301, 257, 400, 333, 300 bytes, paths (0, 1.0) and
(9, 0.8 exp(2.1j)), noise seed 7, scale 32.  Packets decoded to the payload sent, hard | soft:
    13 dB  rate 1/2  101101 | 111111  (31 360 samples on the air)
    13 dB  rate 2/3  000000 | 110111  (24 960)
    13 dB  rate 3/4  000000 | 000000  (23 040)
    17 dB  rate 3/4  100000 | 111111
(no decoder reported ok for a wrong payload).  At rate 5/6 the receiver's packet list on this capture is not the six
packets at any level from 14 to 24 dB with noise seed 7.  A bounded search with the same chain and channel -- noise
seeds 7 .. 12, 14 .. 24 dB in 1 dB steps, these lengths and two further sets of six (250, 399, 312, 275, 350, 288 and
400, 260, 377, 301, 264, 345) -- found 41 of the 198 points at which the oracle delivers the six packets; soft decoding
returned at least as many as hard at every one of them, and no decoder reported ok for a wrong payload.  With the
lengths above:
    seed 8   14, 15 dB        000000 | 100101, 100111
    seed 10  14 .. 18 dB      000000 | 100101 (14 .. 16), 101111 (17, 18)
    seed 12  14 .. 19 dB      000000 | 110001, 110101, 111101 (16 .. 18); 19 dB 010000 | 111101
    seeds 7, 9, 11            no level
(the second set has two points, both at 14 dB; the third has 26, among them seed 9 at 16 .. 23 dB with all six soft).
The case taken is seed 12 at 17 dB with the lengths of the other cases: the middle of three levels with the same result,
hard 0 of 6, soft 5 of 6.  From 20 dB up the packet list is not the six packets there."""
import ctypes as C
import functools

import numpy as np
import pytest

import fec_cases as fc
import punct_cases as pc
import soft_cases as sc
from ofdm_uhd_amd import _abi, engine, fec, ofdm, options

pytestmark = pytest.mark.gpu

# 0 .. 3 and 5: the shortest blocks, P odd and even at every rate; 16 / 17 and 255: more than one thread's share of
# groups, T either side of chunk boundaries; 2040: the longest block (more output bytes and groups than threads)
SIZES = (0, 1, 2, 3, 5, 16, 17, 255, 2040)
COLS = (1, 8, 16)
TAPS = (_abi.TAP_RX_FFT, _abi.TAP_RX_SINK, _abi.TAP_RX_DEMAPPED)


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(options.default_options(modulation="qpsk"))
    yield e
    e.close()


def cfg_of(C_, rate):
    return dict(interleave=C_, rate=rate)


@functools.lru_cache(maxsize=None)
def payloads():
    rng = np.random.default_rng(141)
    return tuple(rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in SIZES)


@functools.lru_cache(maxsize=None)
def blocks(C_, rate):
    return tuple(pc.encode(p, C_, rate) for p in payloads())


@functools.lru_cache(maxsize=None)
def model_decode(block, C_, rate):
    """The model's answer, computed once per distinct block."""
    return pc.decode(block, C_, rate)


def as_model(res):
    return [(int(ok), p, c) for ok, p, c in res]


def damaged(C_, rate, flips):
    rng = np.random.default_rng(int(flips * 1000) + 17 * C_ + pc.RATE_ID[rate])
    out = []
    for b in blocks(C_, rate):
        bits = np.unpackbits(np.frombuffer(b, np.uint8))
        out.append(np.packbits(bits ^ (rng.random(len(bits)) < flips)).tobytes())
    return out


# ---- 1. encoder --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", pc.RATES)
def test_encode_one_mixed_batch(eng, rate):
    lens = [len(b) for b in blocks(16, rate)]
    assert any(n % 2 for n in lens) and not all(n % 2 for n in lens)       # odd P: C' = 8 under 16 columns, and even P
    assert lens == [fec.coded_len(n, rate) for n in SIZES]
    for C_ in COLS:
        assert eng.fec_encode(list(payloads()), cfg_of(C_, rate)) == list(blocks(C_, rate))
    assert eng.fec_encode(list(payloads()), dict(rate=rate)) == list(blocks(16, rate))      # the default is 16 columns
    assert eng.fec_encode([], dict(rate=rate)) == []
    for C_ in (2, 4):
        assert eng.fec_encode([payloads()[6]], cfg_of(C_, rate)) == [pc.encode(payloads()[6], C_, rate)]


def test_encode_refusals(eng):
    bad = _abi.ofdm_fec_cfg(struct_size=C.sizeof(_abi.ofdm_fec_cfg), interleave_cols=16, rate=4)
    for call in (lambda: eng.fec_encode([b"a"], bad), lambda: eng.fec_decode([bytes(10)], bad),
                 lambda: eng.fec_decode_soft([np.ones(80, np.int8)], bad)):
        with pytest.raises(ValueError):
            call()
    for rate in pc.RATES:
        with pytest.raises(ValueError):
            eng.fec_encode([b"a", bytes(2041)], dict(rate=rate))
        bad = _abi.ofdm_fec_cfg(struct_size=C.sizeof(_abi.ofdm_fec_cfg), interleave_cols=3, rate=pc.RATE_ID[rate])
        with pytest.raises(ValueError):
            eng.fec_encode([b"a"], bad)
        assert eng.fec_encode([b"a"], dict(rate=rate)) == [pc.encode(b"a", 16, rate)]   # a refusal leaves the handle usable


# ---- 2. decoder, hard input --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C_", COLS)
@pytest.mark.parametrize("rate", pc.RATES)
def test_decode_clean(eng, rate, C_):
    got = as_model(eng.fec_decode(list(blocks(C_, rate)), cfg_of(C_, rate)))
    assert got == [(1, p, 0) for p in payloads()]
    assert got == [model_decode(b, C_, rate) for b in blocks(C_, rate)]
    assert eng.fec_decode([], dict(rate=rate)) == []


@pytest.mark.parametrize("flips", [0.01, 0.30])
@pytest.mark.parametrize("C_", (1, 16))
@pytest.mark.parametrize("rate", pc.RATES)
def test_decode_with_flips_equals_the_model_in_every_field(eng, rate, C_, flips):
    """30 % is hopeless: the garbage, ok = 0 and corrected still equal the model's."""
    blks = damaged(C_, rate, flips)
    got = as_model(eng.fec_decode(blks, cfg_of(C_, rate)))
    want = [pc.decode(b, C_, rate) for b in blks]
    print("rate %s flips %.2f C %d: ok %d of %d, corrected %s" % (rate, flips, C_, sum(w[0] for w in want), len(want), [w[2] for w in want][-4:]))
    assert got == want
    if flips == 0.30:
        assert want[-1][0] == 0 and want[-2][0] == 0
    else:
        assert sum(w[0] for w in want) >= 5                                 # the short blocks mostly take no flip at all


# ---- 3. decoder, soft input --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", pc.RATES)
def test_decode_soft_with_zeros_ties_and_minus_128(eng, rate):
    rng = np.random.default_rng(143 + pc.RATE_ID[rate])
    vals = []
    for n in (0, 1, 2, 3, 4, 11, 12, 100):
        v = rng.integers(-128, 128, 8 * pc.coded_len(n, rate), dtype=np.int16).astype(np.int8)
        v[rng.random(len(v)) < 0.1] = 0
        v[rng.random(len(v)) < 0.05] = -128
        vals.append(v)
    vals.append(np.zeros(8 * pc.coded_len(12, rate), np.int8))               # erasures only: zeros, and the CRC fails
    clean = 100 * fc.hard_values(pc.encode(payloads()[6], 16, rate)).astype(np.int16)
    clean[::7] = 0                                                           # a seventh erased on top of the puncturing
    vals.append(clean.astype(np.int8))
    vals.append(np.full(8 * pc.coded_len(5, rate), -128, np.int8))           # -128 everywhere reads as -127
    for C_ in COLS:
        got = as_model(eng.fec_decode_soft(vals, cfg_of(C_, rate)))
        assert got == [pc.decode_values(v, C_, rate) for v in vals], C_
    assert got[-3] == (0, bytes(12), 0) == fc.decode_values(np.zeros(8 * fc.coded_len(12), np.int8))
    assert pc.decode_values(vals[-2], 16, rate)[:2] == (1, payloads()[6])
    # random bytes as hard input: +-1 metrics tie constantly, so this is the tie-break test; hard == soft of +-1
    noise = [rng.integers(0, 256, pc.coded_len(n, rate), dtype=np.uint8).tobytes() for n in (0, 1, 2, 63, 64, 65, 500)]
    for C_ in (1, 16):
        want = [pc.decode(b, C_, rate) for b in noise]
        assert as_model(eng.fec_decode(noise, cfg_of(C_, rate))) == want
        assert as_model(eng.fec_decode_soft([fc.hard_values(b) for b in noise], cfg_of(C_, rate))) == want


@pytest.mark.parametrize("rate", pc.RATES)
def test_lengths_that_are_no_block_at_this_rate_inside_a_batch(eng, rate):
    """Gap lengths (P skips them), lengths out of range, and lengths that are blocks at ANOTHER rate only."""
    table = pc.length_table(rate)
    gaps = [m for m in range(min(table), 60) if m not in table]
    elsewhere = [m for r in ("1/2",) + pc.RATES if r != rate for m in pc.length_table(r) if m not in table and m < 3070]
    assert len(gaps) >= 3 and len(elsewhere) >= 3
    good = blocks(16, rate)
    rng = np.random.default_rng(9)
    junk = [rng.integers(0, 256, m, dtype=np.uint8).tobytes() for m in (gaps[0], gaps[2], elsewhere[0], elsewhere[-1], 0, 4090, 3, max(table) + 1)]
    batch = [good[4], junk[0], good[8], junk[1], junk[2], good[5], junk[3], junk[4], good[0], junk[5], junk[6], junk[7], good[7]]
    got = as_model(eng.fec_decode(batch, dict(rate=rate)))
    assert got == [pc.decode(b, 16, rate) for b in batch]
    for i, j in ((0, 4), (2, 8), (5, 5), (8, 0), (12, 7)):
        assert got[i] == (1, payloads()[j], 0)
    for i in (1, 3, 4, 6, 7, 9, 10, 11):
        assert got[i] == (0, b"", 0)
    # the same as values; an array whose length is no multiple of 8 is no block either
    vals = [fc.hard_values(b) for b in batch] + [np.ones(8 * len(good[4]) + 1, np.int8)]
    assert as_model(eng.fec_decode_soft(vals, dict(rate=rate))) == got + [(0, b"", 0)]
    assert as_model(eng.fec_decode(junk, dict(rate=rate))) == [(0, b"", 0)] * len(junk)          # not one block: no launch
    # a block of another rate that is a block here too decodes as this rate's block, whatever comes out
    other = [pc.encode(payloads()[5], 16, r) for r in ("1/2",) + pc.RATES if r != rate]
    assert as_model(eng.fec_decode(other, dict(rate=rate))) == [pc.decode(b, 16, rate) for b in other]


# ---- 4. slices, pointers, rate 1/2, timing ---------------------------------------------------------------------------------
@pytest.mark.parametrize("rate,soft", [("2/3", False), ("3/4", True), ("5/6", False)])
def test_a_batch_wider_than_the_workspace_goes_in_slices(eng, rate, soft):
    """One 2040-byte payload makes every block's share of the workspace 128 KiB: 4096 blocks fill its 512 MiB, the rest
    of the batch is a second depuncture + decoder launch over the same workspace and the same mother values."""
    small = [blocks(16, rate)[i] for i in (0, 3, 4, 6)]
    small[1] = fc.flip(small[1], [5])                                        # one flip: within every rate's power
    gap = next(m for m in range(8, 60) if pc.payload_len(m, rate) is None)
    batch = [small[i % 4] for i in range(4200)]
    batch[7], batch[4097] = bytes(gap), bytes(gap)                           # no block in either slice
    batch[4095], batch[4096], batch[4199] = blocks(16, rate)[-1], small[1], blocks(16, rate)[-1]
    if soft:
        got = as_model(eng.fec_decode_soft([fc.hard_values(b) for b in batch], dict(rate=rate)))
    else:
        got = as_model(eng.fec_decode(batch, dict(rate=rate)))
    assert got == [model_decode(b, 16, rate) for b in batch]
    assert got[4199] == (1, payloads()[-1], 0) and got[4096] == (1, payloads()[3], 1) and got[4097] == (0, b"", 0)


@pytest.mark.parametrize("rate", pc.RATES)
def test_device_pointers(rate):
    torch = pytest.importorskip("torch")
    dev = engine.Engine(options.default_options(modulation="qpsk"), device_ptrs=True)
    try:
        idx = (0, 1, 4, 7, 8)
        pay = [payloads()[i] for i in idx]
        blob, offs, lens = engine.pack_payloads(pay)
        d_pay = torch.from_numpy(blob.copy()).cuda()
        d_coded = torch.zeros(8192, dtype=torch.uint8, device="cuda")
        coff = dev.fec_encode_device(d_pay.data_ptr(), offs, lens, d_coded.data_ptr(), d_coded.numel(), dict(rate=rate))
        coded = d_coded.cpu().numpy()
        want = [blocks(16, rate)[i] for i in idx]
        assert [coded[int(coff[i]):int(coff[i + 1])].tobytes() for i in range(len(idx))] == want
        assert not coded[int(coff[len(idx)]):].any()                                   # nothing behind the last block
        with pytest.raises(engine.EngineError):
            dev.fec_encode_device(d_pay.data_ptr(), offs, lens, d_coded.data_ptr(), int(coff[len(idx)]) - 1, dict(rate=rate))
        clen = np.diff(coff).astype(np.uint32)
        d_out = torch.full((4096,), 0xEE, dtype=torch.uint8, device="cuda")
        poff, ok, corr = dev.fec_decode_device(d_coded.data_ptr(), coff[:len(idx)].copy(), clen, d_out.data_ptr(), d_out.numel(),
                                               dict(rate=rate))
        out = d_out.cpu().numpy()
        assert ok.tolist() == [1] * len(idx) and corr.tolist() == [0] * len(idx)
        assert [out[int(poff[i]):int(poff[i + 1])].tobytes() for i in range(len(idx))] == pay
        assert (out[int(poff[len(idx)]):] == 0xEE).all()                               # nothing written past the payloads
        with pytest.raises(engine.EngineError):
            dev.fec_decode_device(d_coded.data_ptr(), coff[:len(idx)].copy(), clen, d_out.data_ptr(), int(poff[len(idx)]) - 1,
                                  dict(rate=rate))
        rng = np.random.default_rng(3)
        soft = np.concatenate([(fc.hard_values(b).astype(np.int16) * rng.integers(1, 128, 8 * len(b))).astype(np.int8) for b in want])
        d_soft = torch.from_numpy(soft.copy()).cuda()
        d_out.fill_(0xEE)
        poff2, ok2, corr2 = dev.fec_decode_device(d_soft.data_ptr(), (8 * coff[:len(idx)]).astype(np.uint64), clen, d_out.data_ptr(),
                                                  d_out.numel(), dict(rate=rate), soft=True)
        assert poff2.tolist() == poff.tolist() and ok2.tolist() == [1] * len(idx) and corr2.tolist() == [0] * len(idx)
        assert np.array_equal(d_out.cpu().numpy(), out)
    finally:
        dev.close()


def test_rate_one_half_through_the_new_field_is_the_call_without_it(eng):
    pay = list(payloads())
    for C_ in (1, 16):
        a = eng.fec_encode(pay, C_)
        assert a == eng.fec_encode(pay, cfg_of(C_, "1/2")) == [fc.encode(p, C_) for p in pay]
        cfg = fec.fec_cfg(C_)
        cfg.rate = _abi.OFDM_FEC_RATE_1_2
        assert eng.fec_encode(pay, cfg) == a
        dam = [fc.flip(b, [3, 40, 41]) for b in a] + [bytes(11)]
        assert eng.fec_decode(dam, C_) == eng.fec_decode(dam, cfg_of(C_, "1/2")) == [
            (bool(ok), p, c) for ok, p, c in (fc.decode(b, C_) for b in dam)]
        vals = [(37 * fc.hard_values(b).astype(np.int16)).astype(np.int8) for b in dam[:-1]]
        assert eng.fec_decode_soft(vals, C_) == eng.fec_decode_soft(vals, cfg_of(C_, "1/2"))


def test_punct_last_ms():
    e = engine.Engine(options.default_options(modulation="qpsk"))
    try:
        e.prof_enable(True)
        with pytest.raises(ValueError):
            e.fec_punct_last_ms()                      # no fec call yet
        e.fec_encode([b"abc"])
        assert e.fec_last_ms() > 0.0
        with pytest.raises(ValueError):
            e.fec_punct_last_ms()                      # a rate-1/2 call runs none of the new kernels
        blk = e.fec_encode([b"abc"], dict(rate="3/4"))
        assert e.fec_punct_last_ms() > 0.0
        e.fec_decode(blk, dict(rate="3/4"))
        assert e.fec_punct_last_ms() > 0.0 and e.fec_last_ms() > 0.0     # depuncture alone | the decoder
        e.fec_decode_soft([fc.hard_values(blk[0])], dict(rate="3/4"))
        assert e.fec_punct_last_ms() > 0.0
        e.fec_decode([bytes(10)], dict(rate="3/4"))    # 10 is no block at 3/4: nothing launched, no time to report
        for refused in (e.fec_punct_last_ms, e.fec_last_ms):
            with pytest.raises(ValueError):
                refused()
        e.fec_decode(blk, dict(rate="3/4"))
        e.fec_decode([bytes(10)])                      # rate 1/2 again: the punctured kernels' time is of that call no more
        assert e.fec_last_ms() > 0.0
        with pytest.raises(ValueError):
            e.fec_punct_last_ms()
        e.prof_enable(False)
        e.fec_decode(blk, dict(rate="3/4"))
        with pytest.raises(ValueError):
            e.fec_punct_last_ms()                      # the last call ran without profiling
        assert len(e.prof()) == _abi.K_COUNT           # the kernel table is what it was
    finally:
        e.close()


# ---- 5. on a link ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("modulation", ["qpsk", "8psk"])
@pytest.mark.parametrize("rate", pc.RATES)
def test_clean_loopback_and_the_bytes_on_the_air(rate, modulation):
    """N = 64; 8-PSK's three bits per carrier straddle the bytes.  Hard and soft.  (The payload lengths and their order
    were chosen on the CPU with the oracle's receiver: at this geometry it, and so this one, loses or fails some packets
    of a clean 8-PSK burst, depending on the lengths around them; with these it delivers all five at every rate.)"""
    N, CP = 64, 16
    opt = options.default_options(modulation=modulation, fft_length=N, occupied_tones=48, cp_length=CP)
    rng = np.random.default_rng(147)
    pay = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (59, 180, 1, 148, 0)]
    mod = ofdm.ofdm_mod(opt, pad_for_usrp=False, fec=dict(rate=rate))
    hard = ofdm.ofdm_demod(opt, fec=dict(rate=rate))
    soft = ofdm.ofdm_demod(opt, fec=dict(interleave=16, rate=rate), soft=True)
    plain = ofdm.ofdm_demod(opt)
    try:
        for p in pay[:2]:
            mod.send_pkt(p)
        with pytest.raises(ValueError):
            mod.send_pkt(bytes(2041))                                     # the offending packet only
        for p in pay[2:]:
            mod.send_pkt(p)
        x = np.concatenate([np.zeros(2 * N, np.complex64), mod.flush(), np.zeros(N + CP, np.complex64)])
        assert plain.work(x) == [(True, pc.encode(p, 16, rate)) for p in pay]      # exactly the model's punctured blocks
        for dem in (hard, soft):
            assert dem.work(x) == [(True, p) for p in pay]
            assert dem.last_fec == [(True, 0)] * len(pay) and (dem.n_packets, dem.n_ok) == (len(pay), len(pay))
        assert [len(v) for v in soft.last_soft] == [8 * fec.coded_len(len(p), rate) for p in pay]
        half = len(x) // 2                                                  # the chunked path decodes what it delivers, too
        assert soft.feed(x[:half]) + soft.feed(x[half:]) + soft.flush() == [(True, p) for p in pay]
    finally:
        for o in (mod, hard, soft, plain):
            o.engine().close()


def test_the_command_line_takes_the_rate(tmp_path):
    """benchmark_ofdm_tx --fec-rate -> file -> benchmark_ofdm_rx --fec-rate, hard and with --fec-soft: the file comes back."""
    from ofdm_uhd_amd import benchmark_ofdm_rx, benchmark_ofdm_tx, iqio
    src = tmp_path / "tx.bin"
    data = np.random.default_rng(0).integers(0, 256, 20000, dtype=np.uint8).tobytes()
    src.write_bytes(data)
    iqf, plain_iqf = str(tmp_path / "tx.dat"), str(tmp_path / "tx_half.dat")
    npk = benchmark_ofdm_tx.main(["--from-file", str(src), "--to-file", iqf, "-M", "1.0", "-s", "1024", "--fec-rate", "5/6"])
    assert npk == benchmark_ofdm_tx.main(["--from-file", str(src), "--to-file", plain_iqf, "-M", "1.0", "-s", "1024", "--fec"])
    iq = iqio.read_complex_binary(iqf)
    assert 0 < len(iq) < 0.65 * len(iqio.read_complex_binary(plain_iqf))         # 5/6 against 1/2: 0.6 of the air time
    rng = np.random.default_rng(1)                                               # a noise floor and a tail, as the receiver needs
    x = np.concatenate([np.zeros(1024, np.complex64), iq, np.zeros(2048, np.complex64)])
    x += ((rng.standard_normal(len(x)) + 1j * rng.standard_normal(len(x))) * 1e-3).astype(np.complex64)
    iqio.file_sink(iqf).write(x)
    for extra in ([], ["--fec-soft"]):
        out = str(tmp_path / ("rx%d.bin" % len(extra)))
        acct = benchmark_ofdm_rx.main(["--from-file", iqf, "--to-file", out, "--fec-rate", "5/6"] + extra)
        assert acct.n_rcvd == npk and acct.n_right == npk
        assert open(out, "rb").read() == data


def link_case(snr_db, rate, seed=sc.LINK_SEED):
    return _link_case(snr_db, rate, seed)


@functools.lru_cache(maxsize=None)
def _link_case(snr_db, rate, seed):
    """The link of soft_cases at one level, rate and noise seed: one receive call with everything the soft model needs,
    the model's values and both model decoders on them, and what ofdm_demod(fec=) returns hard and soft."""
    opt = options.default_options(modulation=sc.LINK_MOD, fft_length=sc.LINK_N, occupied_tones=sc.LINK_OCC, cp_length=sc.LINK_CP)
    pay = list(sc.link_payloads())
    fcfg = dict(rate=rate)
    mod = ofdm.ofdm_mod(opt, pad_for_usrp=False, fec=fcfg)
    hard = ofdm.ofdm_demod(opt, fec=fcfg)
    soft = ofdm.ofdm_demod(opt, fec=fcfg, soft=True)
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
        want = sc.call_values(eng.cfg, pk, eng.rx_quality(), eng.rx_csi()["eq"], eng.tap(_abi.TAP_RX_SINK), eng.tap(_abi.TAP_RX_DEMAPPED))
        got_vals = eng.rx_soft()
        got_dec = as_model(eng.rx_fec_decode_soft(fcfg))
        got_h, got_s = hard.work(y), soft.work(y)
        return dict(pay=pay, nsamp=len(iq), pk=pk, want=want, got_vals=got_vals, got_dec=got_dec, got_h=got_h, got_s=got_s,
                    fec_h=list(hard.last_fec), fec_s=list(soft.last_fec), n_ok=(hard.n_ok, soft.n_ok))
    finally:
        for o in (mod, hard, soft):
            o.engine().close()
        eng.close()


def _ok_count(r, key):
    return sum(1 for ok, _ in r[key] if ok)


LINK_CASES = [(13.0, "1/2", sc.LINK_SEED), (13.0, "2/3", sc.LINK_SEED), (13.0, "3/4", sc.LINK_SEED), (17.0, "3/4", sc.LINK_SEED),
              (17.0, "5/6", 12)]


@pytest.mark.parametrize("snr_db,rate,seed", LINK_CASES, ids=["%.1f-%s" % c[:2] for c in LINK_CASES])
def test_impaired_link_equals_the_model(snr_db, rate, seed):
    """Exact part, per level and rate: the soft values equal the soft model fed with the same call's taps, records and
    eq rows; rx_fec_decode_soft, ofdm_demod(fec=, soft=) and ofdm_demod(fec=) equal the model decoders at the rate in every
    field.  Every ok payload is one that was sent."""
    r = link_case(snr_db, rate, seed)
    pk, want = r["pk"], r["want"]
    assert len(r["got_vals"]) == len(want) == len(pk) == len(r["pay"])
    for i, (a, b) in enumerate(zip(r["got_vals"], want)):
        assert a.dtype == np.int8 and np.array_equal(a, b), i
    wsoft = [pc.decode_values(v, 16, rate) for v in want]
    whard = [pc.decode(p, 16, rate) for _, p in pk]
    print("link at %.0f dB rate %s: %d samples, outer ok %s, hard ok %s, soft ok %s, corrected hard %s soft %s" % (
        snr_db, rate, r["nsamp"], [int(ok) for ok, _ in pk], [w[0] for w in whard], [w[0] for w in wsoft],
        [w[2] for w in whard], [w[2] for w in wsoft]))
    assert r["got_dec"] == wsoft
    assert r["got_s"] == [(bool(w[0]), w[1]) for w in wsoft]
    assert r["got_h"] == [(bool(w[0]), w[1]) for w in whard]
    assert r["fec_s"] == [(bool(ok), w[2]) for (ok, _), w in zip(pk, wsoft)]
    assert r["fec_h"] == [(bool(ok), w[2]) for (ok, _), w in zip(pk, whard)]
    assert r["n_ok"] == (sum(w[0] for w in whard), sum(w[0] for w in wsoft))
    for got in (r["got_h"], r["got_s"]):
        for (ok, p), sent in zip(got, r["pay"]):
            assert not ok or p == sent
    if rate != "1/2":
        assert r["nsamp"] < link_case(13.0, "1/2")["nsamp"]                # less air time than the mother code


def test_impaired_link_the_rates_separate():
    """Physical part, weak on purpose.  13 dB: the soft ok-count does not rise with the rate and 1/2 returns strictly more
    than 3/4 (CPU: 6 / 5 / 0).  17 dB at 3/4: soft returns strictly more than hard (CPU: 6 against 1)."""
    s12, s23, s34 = (_ok_count(link_case(13.0, r), "got_s") for r in ("1/2", "2/3", "3/4"))
    print("13 dB soft ok at 1/2, 2/3, 3/4: %d %d %d" % (s12, s23, s34))
    assert s12 >= s23 >= s34 and s12 > s34
    r = link_case(17.0, "3/4")
    print("17 dB rate 3/4: soft ok %d, hard ok %d" % (_ok_count(r, "got_s"), _ok_count(r, "got_h")))
    assert _ok_count(r, "got_s") > _ok_count(r, "got_h")
    n12, n23, n34 = (link_case(13.0, x)["nsamp"] for x in ("1/2", "2/3", "3/4"))
    assert (n12, n23, n34) == (31360, 24960, 23040)
