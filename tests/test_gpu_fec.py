"""Coded links on the GPU (csrc/fec.h, ofdm_fec_encode / ofdm_fec_decode / ofdm_fec_decode_soft): everything is integer
arithmetic, so every result is compared with the NumPy model of tests/fec_cases.py by equality -- the encoder's blocks,
the decoder's payloads, verdicts and corrected counts on clean, damaged and hopeless input, soft input with its ties,
lengths that are no block, a batch wider than one workspace slice, the device-pointer forms, and the layer on a link:
ofdm_mod(fec=) -> ofdm_demod(fec=) clean and through a noisy channel.

CPU pre-check of the impaired link (the float64 channel model of multipath_cases fed to the oracle's receiver, the
model decoder behind it): 16-QAM, N 512 / occ 200 / CP 128, six packets of 300, 301, 257, 400, 333 and 300 bytes,
noise only at 15 dB below the signal, noise seed 7: the oracle's raw bytes show 0.16, 0.18, 0.17, 0.14, 0.94 and 0.14 %
bit errors, no packet passes the packet CRC, and the model corrects 8, 9, 7, 9, 51 and 7 coded bits to the payloads
sent.  (At 16 dB one packet of the six already passes the CRC undamaged; at 18 dB five do.)"""
import ctypes as C
import functools

import numpy as np
import pytest

import fec_cases as fc
from ofdm_uhd_amd import _abi, engine, multipath, ofdm, options

pytestmark = pytest.mark.gpu

# T = 8 (n + 4) + 6: n = 3 / 4 and 11 / 12 put it at 62 / 70 and 126 / 134, either side of the 64-step decision chunk
SIZES = list(range(17)) + [63, 64, 65, 2040]
COLS = (1, 16)
IMPAIRED_SNR_DB, IMPAIRED_SEED = 15.0, 7


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
def blocks(C_):
    return tuple(fc.encode(p, C_) for p in payloads())


@functools.lru_cache(maxsize=None)
def model_decode(block, C_):
    """The model's answer, computed once per distinct block."""
    return fc.decode(block, C_)


def as_model(res):
    return [(int(ok), p, c) for ok, p, c in res]


def damaged(C_, rate):
    rng = np.random.default_rng(int(rate * 1000) + C_)
    out = []
    for b in blocks(C_):
        bits = np.unpackbits(np.frombuffer(b, np.uint8))
        out.append(np.packbits(bits ^ (rng.random(len(bits)) < rate)).tobytes())
    return out


# ---- 1. encoder --------------------------------------------------------------------------------------------------------
def test_encode_one_mixed_batch(eng):
    for C_ in COLS:
        assert eng.fec_encode(list(payloads()), C_) == list(blocks(C_))
    assert eng.fec_encode(list(payloads())) == list(blocks(16))          # the default is 16 columns
    assert eng.fec_encode([]) == []
    for C_ in (2, 4, 8):
        assert eng.fec_encode([payloads()[13]], dict(interleave=C_)) == [fc.encode(payloads()[13], C_)]


def test_encode_refusals(eng):
    with pytest.raises(ValueError):
        eng.fec_encode([b"a", bytes(2041)])
    bad = _abi.ofdm_fec_cfg(struct_size=C.sizeof(_abi.ofdm_fec_cfg), interleave_cols=3)
    with pytest.raises(ValueError):
        eng.fec_encode([b"a"], bad)
    with pytest.raises(ValueError):
        eng.fec_decode([bytes(10)], bad)
    bad = _abi.ofdm_fec_cfg(struct_size=8, interleave_cols=16)
    with pytest.raises(ValueError):
        eng.fec_encode([b"a"], bad)
    assert eng.fec_encode([b"a"]) == [fc.encode(b"a")]                   # a refusal leaves the handle usable


# ---- 2. decoder --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C_", COLS)
def test_decode_clean(eng, C_):
    got = as_model(eng.fec_decode(list(blocks(C_)), C_))
    assert got == [(1, p, 0) for p in payloads()]
    assert got == [model_decode(b, C_) for b in blocks(C_)]
    assert eng.fec_decode([]) == []


@pytest.mark.parametrize("rate", [0.01, 0.05, 0.12])
@pytest.mark.parametrize("C_", COLS)
def test_decode_with_flips_equals_the_model_in_every_field(eng, C_, rate):
    """5 % and 12 % are beyond the code's power: the garbage, ok = 0 and corrected still equal the model's."""
    blks = damaged(C_, rate)
    got = as_model(eng.fec_decode(blks, C_))
    want = [fc.decode(b, C_) for b in blks]
    print("rate %.2f C %d: ok %d of %d, corrected %s" % (rate, C_, sum(w[0] for w in want), len(want), [w[2] for w in want][-4:]))
    assert got == want
    if rate == 0.01:
        assert want[-1][:2] == (1, payloads()[-1]) and want[-1][2] > 200   # the 2040-byte block: about 327 flips
    if rate == 0.12:
        assert want[-1][0] == 0


def test_decode_soft_with_ties_erasures_and_minus_128(eng):
    rng = np.random.default_rng(43)
    vals = []
    for n in (0, 3, 4, 11, 12, 100):
        v = rng.integers(-128, 128, 8 * fc.coded_len(n), dtype=np.int16).astype(np.int8)
        v[rng.random(len(v)) < 0.1] = 0
        v[rng.random(len(v)) < 0.05] = -128
        vals.append(v)
    vals.append(np.zeros(8 * fc.coded_len(12), np.int8))                    # erasures only: zeros, and the CRC fails
    clean = 100 * fc.hard_values(blocks(16)[12]).astype(np.int16)
    clean[::3] = 0                                                          # a third punctured away: still exact
    vals.append(clean.astype(np.int8))
    for C_ in COLS:
        got = as_model(eng.fec_decode_soft(vals, C_))
        assert got == [fc.decode_values(v, C_) for v in vals]
    assert got[-2] == (0, bytes(12), 0)
    assert got[-1][:2] == (1, payloads()[12])
    # random bytes as hard input: +-1 metrics tie constantly, so this is the tie-break test
    noise = [rng.integers(0, 256, m, dtype=np.uint8).tobytes() for m in (10, 12, 136, 138, 266, 1000)]
    for C_ in COLS:
        want = [fc.decode(b, C_) for b in noise]
        assert as_model(eng.fec_decode(noise, C_)) == want
        assert as_model(eng.fec_decode_soft([fc.hard_values(b) for b in noise], C_)) == want
    # a length that is no multiple of 8 values is no block
    assert as_model(eng.fec_decode_soft([np.ones(81, np.int8), vals[1]])) == [(0, b"", 0), fc.decode_values(vals[1])]


def test_lengths_that_are_no_block_inside_a_batch(eng):
    good = blocks(16)
    batch = [good[5], b"", good[16], bytes(9), bytes(range(11)), good[17], bytes(4091), good[1]]
    got = as_model(eng.fec_decode(batch))
    for i in (1, 3, 4, 6):
        assert got[i] == (0, b"", 0)
    for i, j in ((0, 5), (2, 16), (5, 17), (7, 1)):
        assert got[i] == (1, payloads()[j], 0)
    assert got == [fc.decode(b) for b in batch]
    assert as_model(eng.fec_decode([b"", bytes(9), bytes(4091)])) == [(0, b"", 0)] * 3     # not one block: no launch


def test_a_batch_wider_than_the_workspace_goes_in_slices(eng):
    """One 2040-byte block makes every block's share of the workspace 128 KiB: 4096 blocks fill its 512 MiB, the rest
    of the batch is a second launch over the same memory."""
    small = [blocks(16)[i] for i in (0, 3, 4, 12)]
    small[1] = fc.flip(small[1], [5, 77])
    batch = [small[i % 4] for i in range(4200)]
    batch[4095], batch[4096], batch[4199] = blocks(16)[-1], small[1], blocks(16)[-1]
    got = as_model(eng.fec_decode(batch))
    assert got == [model_decode(b, 16) for b in batch]
    assert got[4199] == (1, payloads()[-1], 0) and got[4096] == (1, payloads()[3], 2)


def test_last_ms(eng):
    eng.prof_enable(False)
    eng.fec_encode([b"abc"])
    with pytest.raises(ValueError):
        eng.fec_last_ms()                       # the last call ran without profiling
    eng.prof_enable(True)
    try:
        eng.fec_encode([b"abc"])
        assert eng.fec_last_ms() > 0.0
        eng.fec_decode([blocks(16)[3]])
        assert eng.fec_last_ms() > 0.0
        eng.fec_decode([b""])                   # nothing launched: no time to report
        with pytest.raises(ValueError):
            eng.fec_last_ms()
        assert len(eng.prof()) == _abi.K_COUNT  # the kernel table is what it was
    finally:
        eng.prof_enable(False)


def test_device_pointers():
    torch = pytest.importorskip("torch")
    dev = engine.Engine(options.default_options(modulation="qpsk"), device_ptrs=True)
    try:
        pay = [payloads()[i] for i in (0, 1, 12, 18)]
        blob, offs, lens = engine.pack_payloads(pay)
        d_pay = torch.from_numpy(blob.copy()).cuda()
        d_coded = torch.zeros(8192, dtype=torch.uint8, device="cuda")
        coff = dev.fec_encode_device(d_pay.data_ptr(), offs, lens, d_coded.data_ptr(), d_coded.numel())
        coded = d_coded.cpu().numpy()
        want = [blocks(16)[i] for i in (0, 1, 12, 18)]
        assert [coded[int(coff[i]):int(coff[i + 1])].tobytes() for i in range(4)] == want
        assert not coded[int(coff[4]):].any()                                   # nothing behind the last block
        with pytest.raises(engine.EngineError):
            dev.fec_encode_device(d_pay.data_ptr(), offs, lens, d_coded.data_ptr(), int(coff[4]) - 1)
        clen = np.diff(coff).astype(np.uint32)
        d_out = torch.full((4096,), 0xEE, dtype=torch.uint8, device="cuda")
        poff, ok, corr = dev.fec_decode_device(d_coded.data_ptr(), coff[:4].copy(), clen, d_out.data_ptr(), d_out.numel())
        out = d_out.cpu().numpy()
        assert ok.tolist() == [1] * 4 and corr.tolist() == [0] * 4
        assert [out[int(poff[i]):int(poff[i + 1])].tobytes() for i in range(4)] == pay
        assert (out[int(poff[4]):] == 0xEE).all()                               # nothing written past the payloads
        soft = np.concatenate([fc.hard_values(b) for b in want])
        d_soft = torch.from_numpy(soft.copy()).cuda()
        poff2, ok2, corr2 = dev.fec_decode_device(d_soft.data_ptr(), (8 * coff[:4]).astype(np.uint64), clen, d_out.data_ptr(),
                                                  d_out.numel(), soft=True)
        assert poff2.tolist() == poff.tolist() and ok2.tolist() == [1] * 4 and corr2.tolist() == [0] * 4
    finally:
        dev.close()


# ---- 3. on a link ------------------------------------------------------------------------------------------------------
def _air(iq, tail=512 + 128 + 2 * 512, N=512):
    """The burst with silence around it, as the receiver's tests embed one."""
    return np.concatenate([np.zeros(2 * N, np.complex64), iq, np.zeros(tail, np.complex64)])


def test_clean_loopback_and_the_bytes_on_the_air():
    opt = options.default_options(modulation="qpsk")                  # N 512 / occ 200 / CP 128
    rng = np.random.default_rng(47)
    pay = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (0, 1, 100, 2040)]
    mod = ofdm.ofdm_mod(opt, pad_for_usrp=False, fec=True)
    seen = []
    coded = ofdm.ofdm_demod(opt, callback=lambda ok, payload: seen.append((ok, payload)), fec=dict(interleave=16))
    plain = ofdm.ofdm_demod(opt)
    try:
        for p in pay[:2]:
            mod.send_pkt(p)
        with pytest.raises(ValueError):
            mod.send_pkt(bytes(2041))                                   # the offending packet only
        for p in pay[2:]:
            mod.send_pkt(p)
        # (one symbol of silence behind the burst: on more EXACT silence than that the reference's receiver, and so
        # this one, delivers one more, empty, CRC-failed packet; any noise removes it -- the oracle on the CPU shows both)
        x = _air(mod.flush(), tail=512 + 128)
        got = coded.work(x)
        assert got == [(True, p) for p in pay] == seen
        assert coded.last_fec == [(True, 0)] * 4 and (coded.n_packets, coded.n_ok) == (4, 4)
        assert plain.work(x) == [(True, fc.encode(p)) for p in pay]   # exactly the model's coded blocks
        assert plain.last_fec == []
        # the chunked path decodes what it delivers, too
        half = len(x) // 2
        assert coded.feed(x[:half]) + coded.feed(x[half:]) + coded.flush() == [(True, p) for p in pay]
    finally:
        for o in (mod, coded, plain):
            o.engine().close()


def test_impaired_link_equals_the_model_and_recovers_failed_packets():
    """16-QAM through noise at the level the file's docstring derives on the CPU.  Exact part: what ofdm_demod(fec=)
    returns is the model applied to what ofdm_demod without fec returns, in every field.  Physical part: packets the
    packet CRC gave up on come back whole."""
    opt = options.default_options(modulation="qam16")
    rng = np.random.default_rng(2024)
    pay = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (300, 301, 257, 400, 333, 300)]
    mod = ofdm.ofdm_mod(opt, pad_for_usrp=False, fec=True)
    coded = ofdm.ofdm_demod(opt, fec=True)
    plain = ofdm.ofdm_demod(opt)
    try:
        for p in pay:
            mod.send_pkt(p)
        iq = mod.flush()
        psig = float(np.mean(np.abs(iq.astype(np.complex128)) ** 2))
        ch = mod.engine()
        ch.set_multipath(multipath.multipath_cfg(sigma=multipath.sigma_for_snr(IMPAIRED_SNR_DB, psig), seed=IMPAIRED_SEED))
        y = ch.multipath(_air(iq))
        raw = plain.work(y)
        got = coded.work(y)
        want = [fc.decode(p) for _, p in raw]
        print("impaired link: outer ok %s, decoded ok %s, corrected %s" % ([int(ok) for ok, _ in raw], [w[0] for w in want],
                                                                         [w[2] for w in want]))
        assert len(raw) == len(pay)
        assert got == [(bool(w[0]), w[1]) for w in want]
        assert coded.last_fec == [(bool(ok), w[2]) for (ok, _), w in zip(raw, want)]
        assert coded.n_ok == sum(w[0] for w in want)
        assert any(not outer and ok for (outer, _), (ok, _) in zip(raw, got))
        for (ok, p), sent in zip(got, pay):
            assert not ok or p == sent
    finally:
        for o in (mod, coded, plain):
            o.engine().close()
