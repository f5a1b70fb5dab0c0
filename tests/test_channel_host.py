"""The oracle's synthetic channel (orc_channel) against the float64 model of chan_cases.py: no GPU needed.

The GPU tests compare the engine with orc_channel; this file is what makes orc_channel worth comparing with.  The
model draws the same Philox counters in NumPy integers and evaluates Box-Muller and the rotation in float64; the oracle
evaluates them in float32.  The bound below is derived from the oracle's roundings, nothing in it is measured.

eps = 2^-24 (float32 unit roundoff; one ulp is at most 2 eps relative).  libm's logf, cosf and sinf are taken to be
within one ulp (glibc documents less).  First order in eps throughout; the count is then rounded up to absorb the
second-order terms.

  u1, u2     (float)(16 bits) + 0.5 has 17 significant bits and 2^-16 is a power of two: exact.
  rad        logf within 1 ulp: relative 2 eps; -2.0f * l is exact; the square root halves a relative error (eps) and
             sqrtf rounds once (eps): relative 2 eps.
  th         the float32 constant for 2 pi is 0.47 eps off, the product 2 pi * u2 rounds once: th is relative 1.5 eps,
             at most 1.5 eps * 2 pi = 3 pi eps radians, off the angle; cos and sin move by no more than the angle does.
  cosf/sinf  within 1 ulp of a value of modulus <= 1: 2 eps absolute.
             Together |c - cos(2 pi u2)| <= (3 pi + 2) eps = 11.43 eps.
  s          the float32 constant for 1/sqrt 2 is 0.29 eps off, sigma * constant rounds once: relative 1.3 eps, taken
             as 1.5.
  products   rad * c and s * (...) round once each: 2 eps relative.
  noise term s rad c is therefore within  s rad [(1.5 + 2 + 2) |cos| + 11.43] eps <= 16.93 eps s rad  of the model's;
             taken as 18 eps (sigma / sqrt 2) rad, rad being the model's own radius of that sample.
  rotation   (cfo != 0) the phase is float64 in both; cos and sin of it are rounded to float32 (eps each, absolute),
             and the complex product is two rounded products and one rounded sum per part:
             eps (|x.re| + |x.im|) [rounded factors] + eps (|x.re| + |x.im|) [products] + eps |x| [sum]
             <= (2 sqrt 2 + 1) eps |x| = 3.83 eps |x|, taken as 4 eps |x| per part.
  final add  x + noise rounds once: eps |y_part|.

Per part:  |oracle - model| <= 18 eps (sigma / sqrt 2) rad + [cfo != 0] 4 eps |x| + eps |y_part|.

The last two tests show that the comparison has teeth: a model with the words of a pair exchanged, and one whose cyclic
prefix reuses the noise word of the body sample it copies, miss the oracle by more than 1000 times that bound."""
import ctypes as C

import numpy as np
import pytest

import chan_cases as cc


def _orc_philox(orc, seed, stream, counter, rounds=None):
    out = (C.c_uint32 * 2)()
    if rounds is None:
        orc.lib().orc_philox(C.c_uint64(seed), C.c_uint64(stream), C.c_uint64(counter), out)
    else:
        orc.lib().orc_philox_r(C.c_uint64(seed), C.c_uint64(stream), C.c_uint64(counter), rounds, out)
    return (out[0], out[1])


def _model_philox(key, counter, rounds=7):
    w0, w1 = cc.philox(key, np.array([counter], np.uint64), rounds)
    return (int(w0[0]), int(w1[0]))


def test_model_philox_known_answers():
    """The Random123 known-answer vectors of test_oracle.py (key = seed with stream 0), seven and ten rounds."""
    assert cc.chan_key(0x13198a2e, 0) == 0x13198a2e and cc.chan_key(0xffffffff, 0) == 0xffffffff

    def ph(c0, c1, k, rounds=7):
        return _model_philox(cc.chan_key(k, 0), (c1 << 32) | c0, rounds)
    assert ph(0, 0, 0) == (0x257a3673, 0xcd26be2a)
    assert ph(0xffffffff, 0xffffffff, 0xffffffff) == (0xab302c4d, 0x3dc9d239)
    assert ph(0x243f6a88, 0x85a308d3, 0x13198a2e) == (0xbedbbe6b, 0xe4c770b3)
    assert ph(0, 0, 0, 10) == (0xff1dae59, 0x6cd10df2)
    assert ph(0xffffffff, 0xffffffff, 0xffffffff, 10) == (0x2c3f628b, 0xab4fd7ad)
    assert ph(0x243f6a88, 0x85a308d3, 0x13198a2e, 10) == (0xdd7ce038, 0xf62a4c12)


def test_model_philox_equals_oracle_on_large_indices(orc):
    """Counters whose high word is non-zero (2^33 and beyond), keys that take both halves of seed and stream id."""
    counters = [2 ** 33, 2 ** 33 + 1, 2 ** 33 + 5, 2 ** 40 + 12345, 2 ** 63 + 7, 2 ** 64 - 1, 0, 1, 2 ** 32 - 1, 2 ** 32]
    keys = [(0xC0FFEE, 0), (cc.BIG_SEED, 3), (0xC0FFEE, (9 << 32) | 1), (2 ** 64 - 1, 2 ** 64 - 1), (1 << 32, 1 << 32)]
    for seed, stream in keys:
        key = cc.chan_key(seed, stream)
        w0, w1 = cc.philox(key, np.array(counters, np.uint64))
        for i, ctr in enumerate(counters):
            assert (int(w0[i]), int(w1[i])) == _orc_philox(orc, seed, stream, ctr), (seed, stream, ctr)
    # the halves do enter the key
    assert len({cc.chan_key(s, t) for s, t in keys}) == len(keys)
    assert cc.chan_key(cc.BIG_SEED, 3) != cc.chan_key(77, 3) != cc.chan_key(cc.BIG_SEED, 0)
    # words(): one call per pair of stream indices, word 0 to the even one
    idx = np.array([2 ** 33 + 4, 2 ** 33 + 5, 2 ** 34 + 1], np.uint64)
    w = cc.words(cc.BIG_SEED, 3, idx)
    assert int(w[0]) == _orc_philox(orc, cc.BIG_SEED, 3, 2 ** 32 + 2)[0]
    assert int(w[1]) == _orc_philox(orc, cc.BIG_SEED, 3, 2 ** 32 + 2)[1]
    assert int(w[2]) == _orc_philox(orc, cc.BIG_SEED, 3, 2 ** 33)[1]


def _check(x, got, sigma, cfo, seed, stream_id, index0):
    y, rad = cc.model(x, sigma, cfo, seed, stream_id, index0)
    err = np.abs(cc.parts(got) - cc.parts(y))
    b = cc.oracle_bound(x, y, rad, sigma, cfo)
    bad = err > b
    assert not bad.any(), "%d parts beyond the bound, worst %.3g of it" % (int(bad.sum()), float(np.max(err[bad] / b[bad])))
    return y, rad, b


@pytest.mark.parametrize("case", cc.CASES, ids=cc.IDS)
def test_oracle_channel_equals_model_on_transmit_buffers(orc, case):
    clean, ref = cc.reference(orc, case)
    nsym = (len(clean) - case.lead - cc.tail_of(case)) // (case.N + case.CP)
    assert nsym >= 3 and len(ref) == len(clean)
    _, rad, _ = _check(clean, ref, index0=0, **cc.chan_args(case))
    if case.sigma > 0:
        # (Box-Muller on 16 bits: the radius lies between sqrt(-2 ln(1 - 2^-17)) and sqrt(-2 ln 2^-17) = 4.855)
        assert 0.0039 < rad.min() and rad.max() < 4.86 and 1.2 < np.mean(rad) < 1.3
    else:
        assert not rad.any()


def test_oracle_channel_equals_model_standalone(orc):
    """The stand-alone call's edge case: an odd first index beyond 2^33, rotation and noise; and n = 1, n = 0."""
    s = cc.STANDALONE
    x = cc.ramp(s["n"])
    kw = dict(sigma=s["sigma"], cfo=s["cfo"], seed=s["seed"], stream_id=s["stream_id"], index0=s["index0"])
    _check(x, orc.channel(x.copy(), **kw), **kw)
    _check(x[-1:], orc.channel(x[-1:].copy(), **kw), **kw)
    assert len(orc.channel(x[:0].copy(), **kw)) == 0 and len(cc.model(x[:0], **kw)[0]) == 0
    # noise alone and rotation alone
    for kw2 in (dict(kw, cfo=0.0), dict(kw, sigma=0.0)):
        _check(x[:4099], orc.channel(x[:4099].copy(), **kw2), **kw2)


# ---- teeth -----------------------------------------------------------------------------------------------------------
TEETH = [c for c in cc.CASES if c.sigma > 0 and c.name in ("n64_paired_lean", "n512_paired_cfo", "n512_odd_cp")]


def _missed(case, clean, ref, word_index):
    """which samples of the oracle's buffer a model using word_index misses by more than 1000 times the bound"""
    y, rad = cc.model(clean, index0=0, word_index=word_index, **cc.chan_args(case))
    b = cc.oracle_bound(clean, y, rad, case.sigma, cc.cfo_of(case))
    return (np.abs(cc.parts(ref) - cc.parts(y)) > 1000.0 * b).any(axis=1)


@pytest.mark.parametrize("case", TEETH, ids=[c.name for c in TEETH])
def test_exchanged_words_are_caught(orc, case):
    """Word 1 to the even sample and word 0 to the odd one: still Gaussian at the right power, and far outside."""
    clean, ref = cc.reference(orc, case)
    idx = cc.indices(len(clean), 0)
    assert not _missed(case, clean, ref, idx).any()                        # (the unmutated model, same yardstick)
    miss = _missed(case, clean, ref, idx ^ np.uint64(1))
    assert miss.mean() >= 1.0 / 3.0, miss.mean()


@pytest.mark.parametrize("case", TEETH, ids=[c.name for c in TEETH])
def test_prefix_reusing_the_body_word_is_caught(orc, case):
    """A cyclic-prefix copy that carries the noise of the body sample it copies (stream index + N) instead of its own.
    The mutation touches the prefix samples only -- CP of every N + CP, fewer than a third of the buffer -- so the third
    is asked of those; every other sample must still agree."""
    clean, ref = cc.reference(orc, case)
    idx = cc.indices(len(clean), 0)
    pre = cc.prefix_mask(len(clean), case.lead, cc.tail_of(case), case.N, case.CP)
    assert pre.sum() * (case.N + case.CP) == case.CP * (len(clean) - case.lead - cc.tail_of(case))
    miss = _missed(case, clean, ref, np.where(pre, idx + np.uint64(case.N), idx))
    assert not miss[~pre].any()
    assert miss[pre].mean() >= 1.0 / 3.0, miss[pre].mean()
