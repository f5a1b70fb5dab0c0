"""The signal field on the GPU (csrc/sig.h, ofdm_sig_encode / ofdm_sig_decode / ofdm_sig_decode_soft /
ofdm_rx_sig_decode_soft) and the self-describing link above it.  Everything is integer arithmetic, so every result is
compared with the NumPy model of tests/sig_cases.py by equality: the encoder's blocks over one wave, a partly filled
workgroup, two workgroups and many, with bodies of 0 .. 4080 bytes at odd offsets; the decoder's word and margin on
clean fields, all-zero values, 15 and 17 flipped bits, erased copies, values of -128, a constructed tie, packets of 0,
11 and 12 bytes, packets at unaligned offsets (every load path of k_sig_decode: 16-byte, 4-byte and byte loads) and the
seeded AWGN set of 2048 words at Es/N0 = -3 dB; the device-pointer forms and the error codes.

On a link: one ofdm_mod(sig=True) batch of eight packets with eight codings into one ofdm_demod(sig=True), hard and
soft; a batch of one coding through a signalled link and through a link whose ends are both set, with identical
results in every field; the mixed batch through feed() in three cuts, one inside a field and one inside a body, against
work(); and the mixed batch through noise (Engine.multipath, 12 dB, QPSK), where rx_sig_decode_soft must equal the
model on the rx_soft() values of the same call and every decoded packet must equal what the codec calls give on the
values behind the field."""
import functools
import itertools

import numpy as np
import pytest

import sig_cases as sc
from ofdm_uhd_amd import engine, multipath, ofdm, options, sig

pytestmark = pytest.mark.gpu

BODY_LENS = (0, 1, 7, 8, 255, 4080)
# the link's eight codings, as send_pkt(coding=) takes them
LINK_CODINGS = (dict(), dict(rs=True), dict(fec=dict(interleave=16, rate="1/2")), dict(fec=dict(interleave=1, rate="3/4"), rs=True),
                dict(ldpc=dict(rate="1/2")), dict(ldpc=dict(rate="5/6")), dict(ldpc=dict(rate="2/3"), rs=True),
                dict(fec=dict(interleave=4, rate="5/6")))
LINK_SIZES = (40, 93, 100, 150, 92, 300, 188, 61)
N, CP = 512, 128
L = N + CP


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(options.default_options(modulation="qpsk"))
    yield e
    e.close()


def _opt():
    return options.default_options(modulation="qpsk")                 # N 512 / occ 200 / CP 128


def _close(*objs):
    for o in objs:
        o.engine().close()


# ---- 1. encoder --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def encode_case(nblk):
    rng = np.random.default_rng(100 + nblk)
    valid = sc.valid_words()
    words = [valid[(7 * k + nblk) % len(valid)] for k in range(nblk)]
    bodies = [rng.integers(0, 256, BODY_LENS[(k + nblk) % len(BODY_LENS)], dtype=np.uint8).tobytes() for k in range(nblk)]
    return words, bodies, sc.encode(words, bodies)


@pytest.mark.parametrize("nblk", [1, 3, 5, 257])
def test_encode_equals_the_model(eng, nblk):
    words, bodies, want = encode_case(nblk)
    got = eng.sig_encode(words, bodies)
    assert len(got) == nblk
    for k in range(nblk):
        assert np.array_equal(np.frombuffer(got[k], np.uint8), np.frombuffer(want[k], np.uint8)), k
    if nblk >= 5:
        offs = np.cumsum([0] + [len(b) for b in want])
        assert (offs[:-1] % 2).any() and (offs[:-1] % 4 == 0).sum() >= 1       # odd block offsets, and aligned ones
    assert eng.sig_encode([sig.coding(w) for w in words], bodies) == want       # Codings in the words' place


def test_encode_every_body_length_alone_and_the_empty_batch(eng):
    rng = np.random.default_rng(9)
    for n in BODY_LENS:
        body = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        assert eng.sig_encode([0x480], [body]) == sc.encode([0x480], [body]), n
    assert eng.sig_encode([], []) == []


# ---- 2. decoder --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def value_cases():
    """(tag, int8 values) per packet: the field's 96 values and, behind them, some body values."""
    rng = np.random.default_rng(77)

    def body(nbytes):
        return rng.integers(-128, 128, 8 * nbytes).astype(np.int8)

    out = []
    for w in (0, 0x480, 0xB80, 0xFFF, 0x123):
        out.append(("clean %x" % w, np.concatenate([sc.clean_values(w), body(w % 5)])))
    out.append(("zeros", np.zeros(96 + 16, np.int8)))
    for seed, w in enumerate((0x440, 0x980, 0x7FF, 0x001)):
        out.append(("15 flips", np.concatenate([sc.flipped(w, 15, seed), body(3)])))
        out.append(("17 flips", np.concatenate([sc.flipped(w, 17, 50 + seed, amp=1 + 40 * seed), body(1)])))
    for n in (1, 2, 3):
        for copies in itertools.combinations(range(4), n):
            out.append(("erased %s" % (copies,), sc.erased_copies(0xA50, copies, amp=3 + n)))
    out.append(("-128", np.full(96, -128, np.int8)))
    v = sc.clean_values(0x6D0, amp=127).copy()
    v[v < 0] = -128
    out.append(("-128 mixed", v))
    out.append(("tie", sc.tie_values()))
    out.append(("0 bytes", np.zeros(0, np.int8)))
    out.append(("11 bytes", sc.clean_values(0x480)[:88]))
    out.append(("12 bytes", sc.clean_values(0x480)))
    return tuple(out)


def _model(vals):
    return [sc.decode_values(v) for v in vals]


def test_decode_soft_equals_the_model(eng):
    vals = [v for _, v in value_cases()]
    want = _model(vals)
    got = eng.sig_decode_soft(vals)
    for (tag, _), g, w in zip(value_cases(), got, want):
        assert g == w, (tag, g, w)
    tags = [t for t, _ in value_cases()]
    assert want[tags.index("zeros")] == (0, 0) and want[tags.index("tie")] == (0xFF0, 0)
    assert want[tags.index("0 bytes")] == want[tags.index("11 bytes")] == (sc.NO_WORD, 0)
    assert want[tags.index("12 bytes")] == (0x480, 2 * 4 * 8 * 64) and want[tags.index("-128")] == (0, 2 * 4 * 8 * 127)
    assert all(w[1] > 0 for t, w in zip(tags, want) if t == "15 flips" or t.startswith("erased"))
    assert eng.sig_decode_soft([]) == []
    for i in (0, 5, len(vals) - 1):
        assert eng.sig_decode_soft([vals[i]]) == [want[i]]
    assert eng.sig_decode_soft([vals[-3], vals[-2]]) == [(sc.NO_WORD, 0)] * 2      # not one field in the batch


@pytest.mark.parametrize("shift", [1, 2, 3, 4, 5, 8, 12])
def test_decode_soft_at_unaligned_offsets(eng, shift):
    """A stub of ``shift`` values in front moves every packet behind it: offsets that are 0 mod 16, 0 mod 4 and odd."""
    vals = [v for t, v in value_cases() if len(v) >= 96][:12]
    stub = np.ones(shift, np.int8)
    batch = [stub] + vals + [np.ones(3, np.int8)] + vals[::-1]
    want = [(sc.NO_WORD, 0)] + _model(vals) + [(sc.NO_WORD, 0)] + _model(vals[::-1])
    assert eng.sig_decode_soft(batch) == want


def test_decode_hard_equals_the_model(eng):
    rng = np.random.default_rng(78)
    blocks = []
    for _, v in value_cases():
        if len(v) % 8 == 0:
            blocks.append(np.packbits(v > 0).tobytes())
    for k, w in enumerate(sc.valid_words()):                       # odd body lengths: every alignment of the next field
        blocks.append(sc.field_bytes(w) + rng.integers(0, 256, k % 7, dtype=np.uint8).tobytes())
    for seed in range(8):
        for nflip in (15, 17):
            blocks.append(np.packbits(sc.flipped(0x480 + 16 * seed, nflip, 200 + seed) > 0).tobytes() + bytes(seed))
    blocks += [b"", bytes(11), bytes(12)]
    want = [sc.decode_bytes(b) for b in blocks]
    got = eng.sig_decode(blocks)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, len(blocks[i]), g, w)
    assert want[-3:] == [(sc.NO_WORD, 0), (sc.NO_WORD, 0), (0, 2 * 4 * 8)]
    offs = np.cumsum([0] + [len(b) for b in blocks[:-1]])
    assert {int(o) % 4 for o, b in zip(offs, blocks) if len(b) >= 12} == {0, 1, 2, 3}
    assert eng.sig_decode([]) == [] and eng.sig_decode([bytes(5)]) == [(sc.NO_WORD, 0)]
    # hard input is the soft rule on +-1
    some = [b for b in blocks if len(b) >= 12][:20]
    assert eng.sig_decode_soft([sc.values_of_bytes(b) for b in some]) == eng.sig_decode(some)


def test_decode_the_awgn_set(eng):
    words, vals = sc.awgn_set()
    best, margin = sc.decode_many(vals)
    assert np.array_equal(best, words)                                  # the condition test_sig_host.py establishes
    got = eng.sig_decode_soft(list(vals))
    assert [g[0] for g in got] == best.tolist()
    assert [g[1] for g in got] == margin.tolist()
    # the same fields sliced to hard bits: wrong words occur, and the GPU decodes as the model does
    hard = [np.packbits(v > 0).tobytes() for v in vals[:512]]
    want = [sc.decode_bytes(b) for b in hard]
    assert eng.sig_decode(hard) == want
    print("awgn: hard decisions give %d of 512 words wrong" % sum(w[0] != t for w, t in zip(want, words[:512])))


def test_errors(eng):
    with pytest.raises(ValueError):
        eng.sig_encode([0x001], [b"abc"])                               # reserved bits set
    with pytest.raises(ValueError):
        eng.sig_encode([0x480, 0xC00], [b"abc", b""])                   # codec 3
    with pytest.raises(ValueError):
        eng.sig_encode([0x480], [b"abc", b""])
    with pytest.raises(ValueError):
        eng.rx_sig_decode_soft()                                        # no rx() with soft values before it
    assert eng.sig_encode([0x480], [b"abc"]) == sc.encode([0x480], [b"abc"])


def test_device_pointers():
    torch = pytest.importorskip("torch")
    dev = engine.Engine(_opt(), device_ptrs=True)
    try:
        words, bodies, want = encode_case(5)
        blob, offs, lens = engine.pack_payloads(bodies)
        d_body = torch.from_numpy(blob.copy()).cuda()
        total = sum(len(b) for b in want)
        d_out = torch.full((total + 64,), 0xEE, dtype=torch.uint8, device="cuda")
        for base in (0, 1, 3):                                          # the block buffer itself at odd addresses
            d_out.fill_(0xEE)
            coff = dev.sig_encode_device(words, d_body.data_ptr(), offs, lens, d_out.data_ptr() + base, total)
            out = d_out.cpu().numpy()
            assert [out[base + int(coff[i]):base + int(coff[i + 1])].tobytes() for i in range(5)] == want
            assert (out[:base] == 0xEE).all() and (out[base + total:] == 0xEE).all()      # nothing outside the blocks
        with pytest.raises(engine.EngineError):
            dev.sig_encode_device(words, d_body.data_ptr(), offs, lens, d_out.data_ptr(), total - 1)
        clen = np.diff(coff).astype(np.uint32)
        word, margin = dev.sig_decode_device(d_out.data_ptr() + 3, coff[:5].copy(), clen)
        assert word.tolist() == words and margin.tolist() == [64] * 5
        vals = [v for t, v in value_cases() if len(v) >= 96][:10]
        for base in (0, 1, 4, 7):
            flat = np.concatenate([np.zeros(base, np.int8)] + vals)
            d_soft = torch.from_numpy(flat).cuda()
            voff = (base + np.cumsum([0] + [len(v) for v in vals[:-1]])).astype(np.uint64)
            vlen = np.array([len(v) // 8 for v in vals], np.uint32)
            word, margin = dev.sig_decode_device(d_soft.data_ptr(), voff, vlen, soft=True)
            assert list(zip(word.tolist(), margin.tolist())) == _model(vals), base
    finally:
        dev.close()


def test_max_payload_is_what_framed_len_takes(eng):
    for cod in sig.all_codings():
        n = sig.max_payload(cod)
        assert eng.framed_len(sig.coded_len(n, cod)) > 0
        try:
            block = sig.coded_len(n + 1, cod)
        except ValueError:
            continue                                                    # the code itself takes no more
        with pytest.raises(ValueError):
            eng.framed_len(block)


# ---- 3. on a link ------------------------------------------------------------------------------------------------------
def _air(iq, tail=L, floor=0.0):
    """The burst with silence around it, as the receiver's tests embed one.  ``floor``: a seeded noise floor of that
    standard deviation over the whole capture -- long stretches of exact zeros are 0 / 0 to the receiver's metric."""
    x = np.concatenate([np.zeros(2 * N, np.complex64), iq, np.zeros(tail, np.complex64)])
    if floor:
        rng = np.random.default_rng(1)
        x += ((rng.standard_normal(len(x)) + 1j * rng.standard_normal(len(x))) * floor).astype(np.complex64)
    return x


@functools.lru_cache(maxsize=None)
def mixed_batch():
    """(payloads, codings, IQ of the burst, first sample of every packet in the burst): the eight codings in one batch."""
    rng = np.random.default_rng(2026)
    pay = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in LINK_SIZES]
    cods = [sig.coding(**kw) for kw in LINK_CODINGS]
    mod = ofdm.ofdm_mod(_opt(), pad_for_usrp=False, sig=True)
    try:
        with pytest.raises(ValueError):
            mod.send_pkt(bytes(2036), coding=dict(fec=True))            # 12 bytes less than without the field
        for p, kw in zip(pay, LINK_CODINGS):
            mod.send_pkt(p, coding=kw)
        iq = mod.flush()
        nsym = [mod.engine().tx_frame_count([sig.coded_len(len(p), c)])[0] for p, c in zip(pay, cods)]
        assert mod.packets_sent == 8 and mod.flush() is None
    finally:
        _close(mod)
    assert len(iq) == sum(nsym) * L and len(set(cods)) == 8
    starts = np.concatenate([[0], np.cumsum(nsym)[:-1]]) * L
    iq.setflags(write=False)
    return tuple(pay), tuple(cods), iq, tuple(int(s) for s in starts)


def _sig_fields(dem):
    return dict(last_sig=list(dem.last_sig), last_fec=list(dem.last_fec), last_ldpc=list(dem.last_ldpc), last_rs=list(dem.last_rs))


@pytest.mark.parametrize("soft", [False, True])
def test_clean_loopback_of_eight_codings_in_one_batch(soft):
    pay, cods, iq, _ = mixed_batch()
    x = _air(iq)
    seen, snrs = [], []
    dem = ofdm.ofdm_demod(_opt(), callback=lambda ok, p: seen.append((ok, p)), sig=True, soft=True if soft else None,
                          quality_callback=lambda ok, p, q: snrs.append(float(q["snr_preamble_db"])))
    plain = ofdm.ofdm_demod(_opt())
    try:
        got = dem.work(x)
        assert got == [(True, p) for p in pay] == seen                  # every payload, ok, in the order sent
        assert [c for _, _, c in dem.last_sig] == list(cods)
        assert [w for w, _, _ in dem.last_sig] == [c.word for c in cods]
        raw = plain.work(x)
        assert [ok for ok, _ in raw] == [True] * 8
        assert [p[:12] for _, p in raw] == [sc.field_bytes(c.word) for c in cods]          # the model's field on the air
        if soft:
            assert [(w, m) for w, m, _ in dem.last_sig] == [sc.decode_values(v) for v in dem.last_soft]
            assert all(m > 64 for _, m, _ in dem.last_sig)
        else:
            assert [m for _, m, _ in dem.last_sig] == [64] * 8
        assert (dem.n_packets, dem.n_ok) == (8, 8)
        # neutral entries where a coding lacks the stage, the decoders' own where it has it
        assert dem.last_fec == [(True, 0)] * 8 and dem.last_rs == [(True, 0, 0)] * 8
        assert dem.last_ldpc == [(1, 0) if c.codec == sig.CODEC_LDPC else (0, 0) for c in cods]
        # the receiver's own measurements choose the next coding
        assert len(snrs) == 8 and dem.suggest_coding() == sig.coding()                  # a clean capture carries uncoded packets
        assert dem.suggest_coding(margin_db=1e9) == sig.default_table()[0][1]
        dem.reset_coding_history()
        assert dem.suggest_coding() is None
        with pytest.raises(ValueError):
            plain.suggest_coding()                                      # no link quality
    finally:
        _close(dem, plain)


def test_a_packet_with_an_invalid_word_comes_back_as_received(eng):
    """Two blocks made by hand: one whose field holds the codeword of a word that is not valid, one of 5 bytes."""
    opt = _opt()
    good = eng.sig_encode([0], [b"hello"])[0]
    bad = sc.field_bytes(0xC00) + b"body bytes"                         # codec 3
    mod, dem = ofdm.ofdm_mod(opt, pad_for_usrp=False), ofdm.ofdm_demod(opt, sig=True)
    try:
        for b in (good, bad, b"short"):
            mod.send_pkt(b)
        got = dem.work(_air(mod.flush()))
        assert got == [(True, b"hello"), (False, b"body bytes"), (False, b"")]
        assert dem.last_sig == [(0, 64, sig.coding()), (0xC00, 64, None), (sc.NO_WORD, 0, None)]
        assert (dem.n_packets, dem.n_ok) == (3, 1)
    finally:
        _close(mod, dem)


@pytest.mark.parametrize("soft", [False, True])
@pytest.mark.parametrize("kw", [dict(fec=dict(interleave=8, rate="3/4")), dict(ldpc=dict(rate="2/3")),
                                dict(ldpc=dict(rate="1/2"), rs=True)], ids=["conv", "ldpc", "rs-over-ldpc"])
def test_signalled_link_equals_the_link_whose_ends_are_both_set(kw, soft):
    opt = _opt()
    rng = np.random.default_rng(31)
    pay = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (0, 92, 93, 300)]
    s = dict(soft=True) if soft else {}
    mod_s, dem_s = ofdm.ofdm_mod(opt, pad_for_usrp=False, sig=True, **kw), ofdm.ofdm_demod(opt, sig=True, **s)
    mod_b, dem_b = ofdm.ofdm_mod(opt, pad_for_usrp=False, **kw), ofdm.ofdm_demod(opt, **dict(kw, **s))
    try:
        for p in pay:
            mod_s.send_pkt(p)                                           # the link's default coding
            mod_b.send_pkt(p)
        got_s, got_b = dem_s.work(_air(mod_s.flush())), dem_b.work(_air(mod_b.flush()))
        assert got_s == got_b == [(True, p) for p in pay]
        assert [c for _, _, c in dem_s.last_sig] == [sig.coding(**kw)] * 4
        assert dem_s.last_fec == dem_b.last_fec and len(dem_s.last_fec) == 4
        if "ldpc" in kw:
            assert dem_s.last_ldpc == dem_b.last_ldpc and len(dem_s.last_ldpc) == 4
        if kw.get("rs"):
            assert dem_s.last_rs == dem_b.last_rs and len(dem_s.last_rs) == 4
        assert (dem_s.n_packets, dem_s.n_ok) == (dem_b.n_packets, dem_b.n_ok)
    finally:
        _close(mod_s, dem_s, mod_b, dem_b)


@pytest.mark.parametrize("soft", [False, True])
def test_feed_in_three_cuts_equals_work(soft):
    pay, cods, iq, starts = mixed_batch()
    s = dict(soft=True) if soft else {}
    one, fed = ofdm.ofdm_demod(_opt(), sig=True, **s), ofdm.ofdm_demod(_opt(), sig=True, **s)
    try:
        span = fed._stream_geometry()[1]
        x = _air(iq, tail=span + 4096, floor=1e-3)
        # inside packet 3's field (its first data symbol holds header and field), inside packet 5's body (its fourth data
        # symbol), and late enough that the call before the last delivers the first packets and holds the others back
        cuts = [2 * N + starts[3] + L + L // 2, 2 * N + starts[5] + 4 * L + L // 3, 2 * N + starts[4] + span + 100]
        assert cuts == sorted(cuts) and cuts[-1] < len(x) and starts[6] - starts[5] > 6 * L
        want = one.work(x)
        assert want == [(True, p) for p in pay]
        want_f = _sig_fields(one)
        got, got_f, sizes = [], {k: [] for k in want_f}, []
        for a, b in zip([0] + cuts, cuts + [len(x)]):
            out = fed.feed(x[a:b])
            assert len(fed.last_sig) == len(fed.last_fec) == len(fed.last_ldpc) == len(fed.last_rs) == len(out)
            sizes.append(len(out))
            got += out
            for k, v in _sig_fields(fed).items():
                got_f[k] += v
        out = fed.flush()
        sizes.append(len(out))
        got += out
        for k, v in _sig_fields(fed).items():
            got_f[k] += v
        assert got == want and got_f == want_f                          # every field of last_sig included
        assert sizes[:3] == [0, 0, 4] and sum(sizes) == 8                # a strict subset delivered in mid-stream
        assert (fed.n_packets, fed.n_ok) == (one.n_packets, one.n_ok) == (8, 8)
    finally:
        _close(one, fed)


def test_command_lines(tmp_path):
    """benchmark_ofdm_tx --sig announces the coding its flags choose; benchmark_ofdm_rx --sig / --sig-soft need none."""
    from ofdm_uhd_amd import benchmark_ofdm_rx, benchmark_ofdm_tx, iqio
    src = tmp_path / "data.bin"
    src.write_bytes(np.random.default_rng(0).integers(0, 256, 3000, dtype=np.uint8).tobytes())
    for flags in (["--ldpc-rate", "3/4", "--rs"], ["--fec-rate", "2/3"], []):
        iqf = str(tmp_path / "tx.dat")
        npk = benchmark_ofdm_tx.main(["-m", "qpsk", "--from-file", str(src), "--to-file", iqf, "-s", "1024", "--sig"] + flags)
        iq = iqio.read_complex_binary(iqf)
        rng = np.random.default_rng(1)
        x = np.concatenate([np.zeros(1024, np.complex64), iq, np.zeros(2048, np.complex64)])
        x += ((rng.standard_normal(len(x)) + 1j * rng.standard_normal(len(x))) * 1e-3).astype(np.complex64)
        iqio.file_sink(iqf).write(x)
        for extra in (["--sig"], ["--sig-soft"]):
            acct = benchmark_ofdm_rx.main(["-m", "qpsk", "--from-file", iqf, "--to-file", str(tmp_path / "rx.bin")] + extra)
            assert (acct.n_rcvd, acct.n_right) == (npk, npk) and npk == 23, (flags, extra)
    with pytest.raises(SystemExit):
        benchmark_ofdm_rx.main(["--from-file", iqf, "--to-file", str(tmp_path / "rx.bin"), "--sig", "--ldpc"])


def test_noise_the_field_decodes_as_the_model_and_the_bodies_as_the_codec_calls(eng):
    """Engine.multipath, noise only, 12 dB below the burst's mean power, seed 5: the packet CRC fails on two of the eight
    packets and the decoders behind the field have errors to correct, while the field's margins stay above 1500."""
    snr_db = 12.0
    pay, cods, iq, _ = mixed_batch()
    psig = float(np.mean(np.abs(iq.astype(np.complex128)) ** 2))
    dem = ofdm.ofdm_demod(_opt(), sig=True, soft=True)
    try:
        ch = dem.engine()
        ch.set_multipath(multipath.multipath_cfg(sigma=multipath.sigma_for_snr(snr_db, psig), seed=5))
        y = ch.multipath(_air(iq))
        # the engine's call on the handle's own values against the model on the values of the same call
        eng.set_rx_soft(True)
        try:
            raw = eng.rx(y)
            vals = eng.rx_soft()
            got = eng.rx_sig_decode_soft()
        finally:
            eng.set_rx_soft(None)
        assert len(raw) == len(vals) == len(got)
        assert got == [sc.decode_values(v) for v in vals]
        assert got == eng.sig_decode_soft(vals)
        print("noise %.0f dB: %d packets, packet CRC %s, words %s, margins %s" % (
            snr_db, len(raw), [int(ok) for ok, _ in raw], ["%03x" % w for w, _ in got], [m for _, m in got]))
        assert len(vals) and len({int(abs(int(v))) for v in vals[0][:96]}) > 4        # the values are noisy
        assert [w for w, _ in got] == [c.word for c in cods]            # this level does not trouble the field
        assert not all(ok for ok, _ in raw)                             # though it does trouble the packets
        # the link: every packet equals what the codec calls give on the values behind the field
        out = dem.work(y)
        assert [(w, m) for w, m, _ in dem.last_sig] == got and [len(v) for v in dem.last_soft] == [len(v) for v in vals]
        for i, (_, _, cod) in enumerate(dem.last_sig):
            below, body = bool(raw[i][0]), dem.last_soft[i][96:]
            cur = (False if cod is None else below, raw[i][1][12:])
            if cod is not None and cod.codec == sig.CODEC_FEC:
                d = eng.fec_decode_soft([body], cod.fec)[0]
                assert dem.last_fec[i] == (below, d[2])
                cur = (d[0], d[1])
            elif cod is not None and cod.codec == sig.CODEC_LDPC:
                d = eng.ldpc_decode_soft([body], cod.ldpc())[0]
                assert dem.last_fec[i] == (below, d[2]) and dem.last_ldpc[i] == (d[3], d[4])
                cur = (d[0], d[1])
            if cod is not None and cod.rs:
                d = eng.rs_decode([cur[1]])[0]
                assert dem.last_rs[i] == (bool(cur[0]), d[2], d[3])
                cur = (d[0], d[1])
            assert out[i] == (bool(cur[0]), cur[1]), i
        print("noise %.0f dB: verdicts %s, corrected %s" % (snr_db, [int(ok) for ok, _ in out], [c for _, c in dem.last_fec]))
        assert out == [(True, p) for p in pay]
        assert sum(c for _, c in dem.last_fec) + sum(c for _, c, _ in dem.last_rs) > 0      # the decoders had work to do
    finally:
        _close(dem)
