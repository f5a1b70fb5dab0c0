"""The LDPC decoder's byte reliabilities without a GPU: the model of tests/ldpc_rel_cases.py against ldpc_rate_cases's
decoder (the five fields it shares), the definition's consequences on small cases, the worth of the definition on the
seeded RS-over-LDPC chain (BPSK over AWGN, the counts DESIGN.md section 7 records), the ctypes
declarations of the three entry points, and ofdm_demod's argument checks (they run before the constructor opens an
engine)."""
import numpy as np
import pytest

import ldpc_rate_cases as lr
import ldpc_rel_cases as lc
from ofdm_uhd_amd import _abi, ofdm, options


def _values(c, seed):
    """A few blocks of one rate as values: clean, noisy near the threshold, erased in places; and their hard forms."""
    rng = np.random.default_rng(seed)
    out = []
    for n in (0, 1, c.CW_INFO - 4, 2 * c.CW_INFO + 7):
        blk = c.encode(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
        noisy = c.awgn_values(blk, 1.0 + 4.0 * c.fraction, rng)
        erased = noisy.copy()
        erased[rng.integers(0, 100, len(erased)) < 10] = 0
        out += [lr.hard_values(blk), noisy, erased,
                lr.hard_values(lr.flip(blk, rng.choice(8 * len(blk), 3 + len(blk) // 12, replace=False)))]
    out.insert(3, np.zeros(8 * 193, np.int8))            # no block at any rate: (193 - 1) mod 192 = 0 < PB
    return out


@pytest.mark.parametrize("rate", lc.RATES)
def test_the_model_returns_what_the_plain_decoder_returns(rate):
    c = lc.code(rate)
    vals = _values(c, 3)
    assert not c.is_block(193)
    for iters in (1, 3, lc.DEFAULT_ITERS):
        plain = lr.code(rate).decode_many(vals, iters)
        withrel = c.decode_many_rel(vals, iters)
        assert [tuple(d[:5]) for d in withrel] == [tuple(p) for p in plain], (rate, iters)
        for d in withrel:
            assert d[5].dtype == np.uint8 and len(d[5]) == len(d[1])
        assert len(withrel[3][5]) == 0 and withrel[3][:5] == lr.NO_BLOCK
    # some codeword failed and some converged among them, so both halves of the range are visited
    q = np.concatenate([d[5] for d in c.decode_many_rel(vals, 1)])
    assert (q < 128).any() and (q >= 128).any()


@pytest.mark.parametrize("rate", lc.RATES)
def test_consequences_of_the_definition(rate):
    c = lc.code(rate)
    KI = c.CW_INFO
    pay = bytes(range(256)) * 2
    pay = pay[:2 * KI - 4]                                 # two full codewords
    blk = c.encode(pay)
    # clean +-127: every |P| grows past 127, the codeword converges: 255 everywhere
    strong = (127 * (2 * np.unpackbits(np.frombuffer(blk, np.uint8)).astype(np.int16) - 1)).astype(np.int8)
    d = c.decode_values_rel(strong)
    assert d[:5] == (1, pay, 0, 1, 0) and (d[5] == 255).all() and len(d[5]) == len(pay)
    # hard input: the same rule on +-16
    d = c.decode_rel(blk)
    assert d[0] == 1 and d[1] == pay and (d[5] >= 128).all() and (d[5] < 255).any()
    # all values 0 in the first codeword: the all-zero word meets every check with P = 0 everywhere: q = 128 + 0
    v = lr.hard_values(blk).copy()
    v[:8 * lr.CW_SENT] = 0
    d = c.decode_values_rel(v)
    assert d[4] == 0 and (d[5][:KI] == 128).all() and (d[5][KI:] > 128).all()
    # a failed codeword next to a converged one: every byte of the first ranks below every byte of the second
    bad = lc.spoil(blk, [0])
    d = c.decode_rel(bad, 1)
    assert d[4] == 1 and d[5][:KI].max() < 128 <= d[5][KI:].min()
    d = c.decode_rel(bad)                                  # the same flips with iterations to spare: it converges
    assert d[:2] == (1, pay) and d[4] == 0 and d[3] > 1 and d[5].min() >= 128
    # straight from P, one integer at a time, on a noisy block
    rng = np.random.default_rng(9)
    vals = c.awgn_values(blk, 0.5, rng)
    V, sent, k = c.block_values(vals)
    bits, iters, failed, P = c.decode_codewords_rel(V, 2)
    q = c.rel(P, failed, k)
    for g in (0, 1, KI - 1, KI, len(pay) - 1):
        w, m = divmod(g, KI)
        assert int(q[g]) == min([127] + [abs(int(x)) for x in P[w, 8 * m:8 * m + 8]]) + (0 if failed[w] else 128)
    assert len(q) == k - 4


@pytest.mark.parametrize("point", sorted(lc.CHAIN_POINTS))
def test_the_chain_gains_the_recorded_seeds(point):
    """RS above LDPC on seeds 0 .. 119: blocks returned by RS alone and with the reliabilities, the seeds gained, none
    lost, no wrong payload accepted, every gained seed through the second pass."""
    rate, db = point
    gained, alone, withrel = lc.CHAIN_POINTS[point]
    ch = lc.chain(tuple(range(120)), rate, db)
    plain = [s for s, (p, _, _, o, _) in enumerate(ch) if o[0] and o[1] == p]
    rel = [s for s, (p, _, _, _, o) in enumerate(ch) if o[0] and o[1] == p]
    print(rate, db, "RS alone", len(plain), "with reliabilities", len(rel), "gained", sorted(set(rel) - set(plain)))
    assert len(plain) == alone and len(rel) == withrel
    assert set(plain) <= set(rel)                                              # nothing is lost
    assert tuple(sorted(set(rel) - set(plain))) == gained
    for p, _, _, o1, o2 in ch:
        assert not (o1[0] and o1[1] != p) and not (o2[0] and o2[1] != p)       # no wrong payload accepted
    for s in gained:
        assert ch[s][4][4] == 1, s                                             # second == 1
    # the inner fields are the plain decoder's on the same values
    assert [tuple(d[:5]) for _, _, d, _, _ in ch] == [tuple(r) for r in lr.code(rate).decode_many([v for _, v, _, _, _ in ch])]


def test_the_entry_points_are_declared():
    for name in ("ofdm_ldpc_decode_rel", "ofdm_ldpc_decode_soft_rel", "ofdm_rx_ldpc_decode_soft_rel"):
        assert name in _abi.EXPORTS
    assert _abi.OFDM_ABI_VERSION == 6


def test_value_errors_of_the_receiver_object():
    opt = options.default_options(modulation="qpsk")
    # as before, with the messages they had
    with pytest.raises(ValueError, match="this decoder produces no byte reliabilities"):
        ofdm.ofdm_demod(opt, ldpc=True, soft=True, rs=dict(erasures=True))
    with pytest.raises(ValueError, match="this decoder produces no byte reliabilities"):
        ofdm.ofdm_demod(opt, ldpc=True, rs=dict(erasures=True))
    with pytest.raises(ValueError, match="this decoder produces no byte reliabilities"):
        ofdm.ofdm_demod(opt, ldpc=True, rs=dict(erasures=True, source="fec"))
    with pytest.raises(ValueError, match="source must be \"fec\""):
        ofdm.ofdm_demod(opt, soft=True, rs=dict(erasures=True, source="soft"))
    with pytest.raises(ValueError, match="source must be \"fec\""):
        ofdm.ofdm_demod(opt, fec=True, rs=dict(erasures=True, source="soft"))
    with pytest.raises(ValueError, match="two inner codes"):
        ofdm.ofdm_demod(opt, ldpc=True, fec=True, rs=dict(erasures=True, source="ldpc"))
    with pytest.raises(ValueError, match='source="fec"\\) needs fec='):
        ofdm.ofdm_demod(opt, rs=dict(erasures=True, source="fec"))
    # new
    with pytest.raises(ValueError, match='source="ldpc"\\) needs ldpc='):
        ofdm.ofdm_demod(opt, rs=dict(erasures=True, source="ldpc"))
    with pytest.raises(ValueError, match='source="ldpc"\\) needs ldpc='):
        ofdm.ofdm_demod(opt, soft=True, rs=dict(erasures=True, source="ldpc", max_erasures=20))
    with pytest.raises(ValueError, match='source="ldpc"\\) does not combine with fec='):
        ofdm.ofdm_demod(opt, fec=True, rs=dict(erasures=True, source="ldpc"))
    with pytest.raises(ValueError, match="max_erasures"):
        ofdm.ofdm_demod(opt, ldpc=True, rs=dict(erasures=True, source="ldpc", max_erasures=33))
    with pytest.raises(ValueError):
        ofdm.ofdm_demod(opt, ldpc=True, rs=dict(source="ldpc"))                # source without erasures=True
