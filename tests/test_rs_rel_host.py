"""Decoding with reliabilities without a GPU: the NumPy model of tests/rs_rel_cases.py against the definition (uniqueness
on constructed cases, the threshold at ties, M = 0 and all-255 reliabilities equal to rs_cases.decode, the rule that
makes reliabilities from values), the Python helpers of rs.py against it, the header, the exports and the struct, and the
host arithmetic of csrc/rs_plan.h through the stand-alone checker tools/rs_rel_check.cpp; and the impaired link on the CPU
over its whole grid (the grid, its counts and the points the GPU test takes are listed in tests/test_gpu_rs_rel.py)."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import rs_cases as rc
import rs_rel_cases as rr
import stage_harness as sh
from ofdm_uhd_amd import _abi, rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rand_payload(n, seed=0):
    return np.random.default_rng(5000 * seed + n).integers(0, 256, n, dtype=np.uint8).tobytes()


# ---- 1. the threshold --------------------------------------------------------------------------------------------------
def test_threshold_at_ties():
    q = np.full(255, 200, np.int64)
    q[:29] = 0
    assert rr.threshold(q, 28) is None and len(rr.erased(q, 28)) == 0              # 29 at 0: c(0) > M, no second pass
    assert rr.threshold(q, 29) == 199 and rr.erased(q, 29).tolist() == list(range(29))
    q[28] = 1
    q[29:33] = 1                                                                    # 28 at 0 and 5 at 1
    assert rr.threshold(q, 28) == 0 and rr.erased(q, 28).tolist() == list(range(28))
    assert rr.threshold(q, 32) == 0 and rr.threshold(q, 33) == 199 and len(rr.erased(q, 33)) == 33
    assert rr.threshold(np.full(40, 255), 32) is None                               # 255: never erased, c(tau*) = 0
    q = np.full(40, 255, np.int64)
    q[7] = 254
    assert rr.threshold(q, 32) == 254 and rr.erased(q, 32).tolist() == [7]
    assert rr.threshold(np.zeros(36, np.int64), 32) is None and rr.threshold(np.zeros(32, np.int64), 32) == 254
    assert rr.threshold(np.arange(36), 0) is None                                   # M = 0: c(0) = 1 > 0
    q = np.array([3, 3, 3, 9, 9, 200], np.int64)                                    # ties across the cap at every M
    assert [rr.threshold(q, M) for M in range(7)] == [None, None, None, 8, 8, 199, 254]
    assert [len(rr.erased(q, M)) for M in range(7)] == [0, 0, 0, 3, 3, 5, 6]


# ---- 2. the second pass against the definition ----------------------------------------------------------------------------
def test_second_pass_returns_the_codeword_and_only_within_the_count():
    rng = np.random.default_rng(1)
    for n, (f, e) in itertools.product((36, 60, 255), ((32, 0), (30, 1), (16, 8), (2, 15), (31, 0), (20, 0), (1, 0), (17, 8), (26, 4), (33, 0))):
        sent = np.frombuffer(rc.encode(rand_payload(n - 36, 1)), np.uint8)
        perm = rng.permutation(n)
        J, E = np.sort(perm[:f]), perm[f:f + e]
        r = sent.copy()
        r[np.concatenate([J[::2], E])] ^= rng.integers(1, 256, len(J[::2]) + e).astype(np.uint8)      # half of J stays correct
        out = rr.second_pass(r, J)
        if 2 * e + f <= 32:
            assert out is not None and np.array_equal(out, sent), (n, f, e)
        elif f <= 32:
            # past the line: nothing, or ANOTHER codeword inside the count (then the sent one is outside it: unique)
            assert out is None or (not rc.syndromes(out).any() and 2 * int((out != r)[np.setdiff1d(np.arange(n), J)].sum()) + f <= 32)
            assert out is None or not np.array_equal(out, sent)
        else:
            assert out is None                                                      # more than 32 erasures: never
    assert rr.second_pass(sent, np.zeros(0, np.int64)) is None                      # nothing erased: no second pass


def test_uniqueness_by_search_on_a_small_case():
    """The definition searched directly: a 36-symbol word, J of 30 positions, one error outside: among ALL words that
    differ from r in at most one position outside J (6 positions x 255 values, and none), exactly one completes to a
    codeword, and it is what second_pass returns."""
    rng = np.random.default_rng(2)
    sent = np.frombuffer(rc.encode(b""), np.uint8)
    perm = rng.permutation(36)
    J, out_pos = np.sort(perm[:30]), np.sort(perm[30:])
    r = sent.copy()
    r[J[:25]] ^= rng.integers(1, 256, 25).astype(np.uint8)
    r[out_pos[2]] ^= 0x41
    X = rc.EXP[np.arange(35, -1, -1) % 255]
    A = [[int(rc.EXP[(rc.LOG[int(X[p])] * i) % 255]) for p in J] for i in range(32)]   # 32 equations, 30 unknowns
    # every candidate's syndromes as one more column of the same elimination: a column is consistent where nothing of it
    # is left below the rank of A
    cands = [(None, 0)] + [(int(p), v) for p in out_pos for v in range(1, 256)]
    words = np.repeat(r[None, :], len(cands), axis=0)
    for i, (p, v) in enumerate(cands):
        if p is not None:
            words[i, p] ^= v
    aug = np.concatenate([np.array(A, np.int64), np.array([rc.syndromes(w) for w in words], np.int64).T], axis=1)
    row = 0
    for col in range(len(J)):
        nz = np.flatnonzero(aug[row:, col])
        assert len(nz)                                                              # (A has full column rank: distinct locators)
        aug[[row, row + int(nz[0])]] = aug[[row + int(nz[0]), row]]
        aug[row] = rc.gmul_v(aug[row], rc.ginv(int(aug[row, col])))
        for other in range(32):
            if other != row and aug[other, col]:
                aug[other] ^= rc.gmul_v(aug[row], int(aug[other, col]))
        row += 1
    consistent = np.flatnonzero(~aug[row:, len(J):].any(axis=0))
    found = []
    for i in consistent:
        cand = words[i].copy()
        Y = rr.solve(A, [int(x) for x in rc.syndromes(cand)])
        cand[J] ^= Y.astype(np.uint8)
        assert not rc.syndromes(cand).any()
        found.append(cand)
    assert len(found) == 1 and np.array_equal(found[0], sent)
    assert np.array_equal(rr.second_pass(r, J), sent)


def test_solve():
    rng = np.random.default_rng(3)
    for m, n in ((4, 4), (8, 5), (32, 32), (32, 17)):
        A = rng.integers(0, 256, (m, n))
        x = rng.integers(0, 256, n)
        b = [int(np.bitwise_xor.reduce(rc.gmul_v(A[i], x))) for i in range(m)]
        got = rr.solve(A, b)
        assert got is not None and [int(np.bitwise_xor.reduce(rc.gmul_v(A[i], got))) for i in range(m)] == b
    assert rr.solve([[1, 1], [1, 1]], [1, 2]) is None and rr.solve([[0, 0]], [0]).tolist() == [0, 0]


# ---- 3. blocks ------------------------------------------------------------------------------------------------------------
def test_no_erasures_and_all_255_equal_errors_only():
    rng = np.random.default_rng(4)
    for n in (0, 3, 219, 220, 443):
        b = rc.encode(rand_payload(n, 2))
        for d in (b, rc.errors_per_codeword(b, 16, rng), rc.errors_per_codeword(b, 17, rng), rc.damage(b, rng.choice(len(b), 30, False), rng)):
            want = rc.decode(d) + (0,)
            assert rr.decode(d, None) == want and rr.decode(d, np.zeros(len(d), np.uint8), 0) == want
            assert rr.decode(d, np.full(len(d), 255, np.uint8), 28) == want and rr.decode(d, np.full(len(d), 255, np.uint8), 32) == want
    for m in (0, 35, 256, 4081):
        assert rr.decode(bytes(m), np.zeros(m, np.uint8)) == (0, b"", 0, 0, 0)


def test_blocks_with_reliabilities():
    rng = np.random.default_rng(5)
    p = rand_payload(220, 3)
    b = rc.encode(p)                                                                # W = 2
    d, rel, J = rr.spoil(b, 1, 20, 0, rng)
    assert rc.decode(d) == (0, d[:220], 0, 1) and rr.decode(d, rel) == (1, p, 20, 0, 1)
    assert rr.decode(d, rel, 19) == (0, d[:220], 0, 1, 0)                           # c(0) = 20 > 19
    d, rel, J = rr.spoil(b, 0, 24, 4, rng, erase_good=5, pin=(0, -1))
    assert {0, 143}.issubset(J.tolist()) and rr.decode(d, rel) == (1, p, 23, 0, 1)  # 19 erased and wrong, 4 errors
    d, rel, J = rr.spoil(b, 0, 24, 5, rng)
    assert rr.decode(d, rel)[2:] == (0, 1, 0)                                       # 2 * 5 + 24 = 34
    d16 = rc.errors_per_codeword(b, 16, rng)                                        # the first pass decodes: reliabilities play no part
    assert rr.decode(d16, np.zeros(len(b), np.uint8), 32) == (1, p, 32, 0, 0)


# ---- 4. reliabilities from values ------------------------------------------------------------------------------------------
def test_rel_from_values():
    v = np.array([-128, 127, -128, 127, -127, 127, -128, -128,   5, -4, 3, -128, 9, 100, -100, 7,   90, 90, 90, 0, 90, 90, 90, 90,
                  1, -1, 1, -1, 1, -1, 1, -1,   -128] + [-128] * 7, np.int8)
    assert rr.rel_from_values(v).tolist() == rs.rel_from_values(v).tolist() == [127, 3, 0, 1, 127]
    rng = np.random.default_rng(6)
    v = rng.integers(-128, 128, 8 * 500).astype(np.int8)
    assert np.array_equal(rr.rel_from_values(v), rs.rel_from_values(v)) and rs.rel_from_values(v).dtype == np.uint8
    assert len(rs.rel_from_values(np.zeros(0, np.int8))) == 0
    with pytest.raises(ValueError):
        rs.rel_from_values(np.zeros(9, np.int8))


# ---- 5. Python configuration, header, exports, the checker ------------------------------------------------------------------
def test_rs_cfg():
    c = rs.rs_cfg()
    assert (c.struct_size, c.max_erasures, list(c.reserved)) == (32, 28, [0] * 6) and rs.DEFAULT_MAX_ERASURES == rr.DEFAULT_M == 28
    assert rs.rs_cfg(0).max_erasures == 0 and rs.rs_cfg(32).max_erasures == 32
    for bad in (-1, 33, 2.5, True):
        with pytest.raises(ValueError):
            rs.rs_cfg(bad)
    assert rs.as_cfg(None).max_erasures == 28 and rs.as_cfg(dict(max_erasures=5)).max_erasures == 5 and rs.as_cfg(c) is c
    with pytest.raises(ValueError):
        rs.as_cfg(7)


def test_header_exports_and_struct_layout(tmp_path):
    hdr, code = sh.check_header_declares_and_library_exports(["ofdm_rs_decode_rel", "ofdm_rs_rel_from_soft", "ofdm_rs_rel_last_ms"])
    assert "decoding with reliabilities" in hdr
    sh.check_cfg_layout_matches_header(tmp_path, _abi.ofdm_rs_rel_cfg, 32)
    assert re.search(r"int\s+ofdm_rs_decode_rel\(ofdm_handle \*h, const ofdm_rs_rel_cfg \*cfg, const uint8_t \*coded,", code)
    lib = _abi.load()
    assert len(lib.ofdm_rs_decode_rel.argtypes) == 15 and len(lib.ofdm_rs_rel_from_soft.argtypes) == 8
    assert len(lib.ofdm_rs_decode.argtypes) == 11                                   # ofdm_rs_decode is what it was
    assert lib.ofdm_rs_rel_last_ms(None, C.byref(C.c_double(0))) == _abi.OFDM_E_INVAL


def test_rel_checker(tmp_path):
    """The host arithmetic as a program of its own (the build a sanitizer run uses adds -fsanitize=address,undefined)."""
    exe = str(tmp_path / "rs_rel_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tools", "rs_rel_check.cpp")])
    out = subprocess.check_output([exe]).decode()
    assert out.strip().endswith("rs_rel_check ok")


# ---- 6. the impaired link on the CPU, over the grid -------------------------------------------------------------------------
LINK_SEEDS, LINK_DB = range(7, 13), range(16, 23)


def test_link_grid_conditions(orc):
    """Noise seeds 7 .. 12, 16 .. 22 dB, M = 28.  At every point where the six packets are delivered: decoding with
    reliabilities returns every packet that errors-only decoding returns, and no decoder reports ok for a wrong payload.
    The counts are those of test_gpu_rs_rel.py's table."""
    import soft_cases as sc
    from ofdm_uhd_amd import config, options
    opt = options.default_options(modulation=sc.LINK_MOD, fft_length=sc.LINK_N, occupied_tones=sc.LINK_OCC, cp_length=sc.LINK_CP)
    cfg = config.make_cfg(opt)
    pay = sc.link_payloads()
    per_level = {}
    points = better = 0
    for seed in LINK_SEEDS:
        for snr in LINK_DB:
            plain, wrel = rr.link_on_the_cpu(orc, cfg, float(snr), seed)
            if plain is None:
                continue
            points += 1
            a, b = rr.link_summary(plain, pay), rr.link_summary(wrel, pay)
            for side in (plain, wrel):
                for o, p in zip(side, pay):
                    assert not o[0] or o[1] == p, (seed, snr)                    # no ok for a wrong payload
            assert all(y >= x for x, y in zip(a, b)), (seed, snr, a, b)           # never fewer
            n = per_level.setdefault(snr, [0, 0])
            n[0] += a.count("1")
            n[1] += b.count("1")
            better += a.count("1") <= 4 and b.count("1") > a.count("1")
    print("link grid: %d points, errors only > with reliabilities per level %s, %d points lose two and gain" % (points, per_level, better))
    assert points == 42 and better == 21
    assert [tuple(per_level[s]) for s in LINK_DB] == [(3, 15), (9, 24), (19, 31), (28, 32), (31, 32), (34, 34), (34, 35)]
