"""The LDPC coded-link layer at its four rates without a GPU: the NumPy model of tests/ldpc_rate_cases.py against
ldpc_cases.py at rate 1/2 and against its own consequences at every rate (entry counts and row degrees, no 4-cycles over
all 24 columns, zero syndromes, the parity bits as the unique solution, known lengths, round trips clean and with
flips), the library's ofdm_ldpc_coded_len_rate / ofdm_ldpc_payload_len_rate against the model over every length, the
configuration helpers, the header, and the host arithmetic of csrc/ldpc_plan.h at every rate through the stand-alone
checker tools/ldpc_rate_plan_check.cpp, built plain and with -fsanitize=address,undefined."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ldpc_cases as lc
import ldpc_rate_cases as rc
from ofdm_uhd_amd import _abi, ldpc, rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_RATES = ("2/3", "3/4", "5/6")
# hard-decision damage the round trips must survive: a quarter of the binary symmetric channel's limit for the rate
# (1 - H(p) = R at p = 6.1, 4.2 and 2.5 %); twice that for the block that has to take several iterations
FLIPS = {"2/3": 0.015, "3/4": 0.010, "5/6": 0.006}
# rate -> (mb, kb, mid, info entries, parity entries, row degrees, KI, PB, largest payload)
FACTS = {
    "1/2": (12, 12, 6, 58, 25, [7] * 6 + [6] + [7] * 5, 96, 96, 2012),
    "2/3": (8, 16, 4, 54, 17, [8] + [9] * 7, 128, 64, 2684),
    "3/4": (6, 18, 3, 60, 13, [12, 12, 12, 12, 13, 12], 144, 48, 3020),
    "5/6": (4, 20, 2, 64, 9, [18, 18, 19, 18], 160, 32, 3356),
}


def rand_payload(n, seed=0):
    return np.random.default_rng(1000 * seed + n).integers(0, 256, n, dtype=np.uint8).tobytes()


def sizes(c):
    KI = c.CW_INFO
    return (0, 1, KI - 5, KI - 4, KI - 3, 2 * KI - 4, 2 * KI - 3, c.MAX_PAYLOAD)


# ---- 1. rate 1/2 is ldpc_cases ---------------------------------------------------------------------------------------------
def test_rate_half_equals_ldpc_cases():
    c = rc.code("1/2")
    assert np.array_equal(c.H, lc.H) and c.ROW_ENTRIES == lc.ROW_ENTRIES and c.N_ENTRIES == lc.N_ENTRIES
    assert (c.CW_INFO, c.CW_PARITY, c.MAX_PAYLOAD, rc.MAX_CODED, rc.HARD) == (lc.CW_INFO, lc.CW_PARITY, lc.MAX_PAYLOAD, lc.MAX_CODED, lc.HARD)
    rng = np.random.default_rng(5)
    info = rng.integers(0, 2, (30, lc.K_BITS), dtype=np.uint8)
    assert np.array_equal(c.encode_codeword(info), lc.encode_codeword(info))
    for n in (0, 1, 91, 92, 93, 189, 2012):
        p = rand_payload(n)
        b = lc.encode(p)
        assert c.encode(p) == b and c.coded_len(n) == lc.coded_len(n)
        bad = lc.flip(b, np.flatnonzero(rng.random(8 * len(b)) < 0.05))
        assert c.decode(bad) == lc.decode(bad)
        assert c.decode(bad, 2) == lc.decode(bad, 2)
        v = lc.awgn_values(b, 1.5, 0.5, rng)
        assert c.decode_values(v) == lc.decode_values(v)
    vals = [lc.awgn_values(lc.encode(rand_payload(n, 6)), 1.5, 0.5, rng) for n in (0, 93, 500)] + [np.zeros(8 * 99, np.int8)]
    assert c.decode_many(vals) == lc.decode_many(vals)
    for m in range(4201):
        assert c.payload_len(m) == lc.payload_len(m)


# ---- 2. the tables -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", rc.RATES)
def test_table_shape_degrees_and_no_4_cycles(rate):
    c = rc.code(rate)
    mb, kb, mid, n_info, n_par, degs, KI, PB, maxp = FACTS[rate]
    H = c.H
    assert H.shape == (mb, 24) and (c.ROWS, c.KB, c.MID) == (mb, kb, mid) and (c.CW_INFO, c.CW_PARITY, c.MAX_PAYLOAD) == (KI, PB, maxp)
    assert int((H[:, :kb] >= 0).sum()) == n_info and int((H[:, kb:] >= 0).sum()) == n_par and c.N_ENTRIES == n_info + n_par
    assert [len(r) for r in c.ROW_ENTRIES] == degs and max(degs) <= 19
    assert ((H >= -1) & (H < 64)).all()
    assert (H[:, kb:] >= 0).sum(axis=0).tolist() == [3] + [2] * (mb - 1)         # the staircase and its first column
    assert (H[0, kb], H[mid, kb], H[mb - 1, kb]) == (1, 0, 1)
    n = 0
    for r in range(mb):
        for r2 in range(r + 1, mb):
            both = np.flatnonzero((H[r] >= 0) & (H[r2] >= 0))
            for a in range(len(both)):
                for b in range(a + 1, len(both)):
                    c1, c2 = both[a], both[b]
                    assert (H[r, c1] - H[r2, c1] - H[r, c2] + H[r2, c2]) % 64 != 0, (r, r2, c1, c2)
                    n += 1
    assert n > 0                                                                 # (there are rectangles to look at)


# ---- 3. the encoder ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", rc.RATES)
def test_zero_syndrome_and_the_parity_bits_are_the_unique_solution(rate):
    c = rc.code(rate)
    rng = np.random.default_rng(3)
    info = rng.integers(0, 2, (100, c.K_BITS), dtype=np.uint8)
    info[0] = 0
    info[1] = 1
    info[2:2 + c.KB] = 0
    for j in range(c.KB):
        info[2 + j, 64 * j] = 1                                                  # one bit per info column
    cw = c.encode_codeword(info)
    assert cw.shape == (100, rc.N_BITS) and np.array_equal(cw[:, :c.K_BITS], info)     # systematic
    assert not c.syndrome(cw).any()
    assert not cw[0].any()
    # any single flipped bit breaks as many checks as its column has entries; so for the parity bits: with the info bits
    # fixed no word at distance 1 meets the checks, and since the parity part of H is square the solution is the only one
    for b in range(rc.N_BITS):
        flipped = cw[:3].copy()
        flipped[:, b] ^= 1
        assert c.syndrome(flipped).reshape(3, -1).sum(axis=1).tolist() == [int((c.H[:, b // 64] >= 0).sum())] * 3
    # the parity part alone is invertible over GF(2): its 64 mb x 64 mb matrix has full rank
    mb = c.ROWS
    M = np.zeros((64 * mb, 64 * mb), np.uint8)
    for i in range(mb):
        for j in range(c.KB, 24):
            if c.H[i, j] >= 0:
                for z in range(64):
                    M[64 * i + z, 64 * (j - c.KB) + (z + int(c.H[i, j])) % 64] = 1
    assert gf2_rank(M) == 64 * mb


def gf2_rank(M):
    M = M.copy()
    rank = 0
    for col in range(M.shape[1]):
        piv = np.flatnonzero(M[rank:, col])
        if len(piv) == 0:
            continue
        p = rank + piv[0]
        M[[rank, p]] = M[[p, rank]]
        rows = np.flatnonzero(M[:, col])
        rows = rows[rows != rank]
        M[rows] ^= M[rank]
        rank += 1
        if rank == M.shape[0]:
            break
    return rank


@pytest.mark.parametrize("rate", NEW_RATES)
def test_blocks_of_the_model(rate):
    c = rc.code(rate)
    KI, PB = c.CW_INFO, c.CW_PARITY
    for n in sizes(c):
        p = rand_payload(n)
        b = c.encode(p)
        assert len(b) == c.coded_len(n)
        k = n + 4
        kws = c.cw_info_lens(k)
        assert sum(kws) == k and all(kw == KI for kw in kws[:-1]) and 1 <= kws[-1] <= KI
        info = b"".join(b[192 * w:192 * w + kw] for w, kw in enumerate(kws))    # systematic: the info bytes are on the air
        assert info[:n] == p and len(info) == k
    assert {n: c.coded_len(n) for n in (0, KI - 4, KI - 3, 2 * KI - 4, c.MAX_PAYLOAD)} == {
        0: PB + 4, KI - 4: 192, KI - 3: 193 + PB, 2 * KI - 4: 384, c.MAX_PAYLOAD: 4032}
    assert c.coded_len(c.MAX_PAYLOAD + 1) is None
    with pytest.raises(AssertionError):
        c.encode(bytes(c.MAX_PAYLOAD + 1))


# ---- 4. lengths: the library against the model ---------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", rc.RATES)
def test_length_functions_equal_the_model_for_every_length(rate):
    c = rc.code(rate)
    KI, PB, maxp = c.CW_INFO, c.CW_PARITY, c.MAX_PAYLOAD
    assert ldpc.max_payload(rate) == maxp == 21 * KI - 4 and ldpc.cw_info(rate) == KI and ldpc.MAX_CODED == rc.MAX_CODED == 4032
    prev = -1
    for n in range(maxp + 90):
        want = c.coded_len(n)
        if want is None:
            assert n > maxp
            with pytest.raises(ValueError):
                ldpc.coded_len(n, rate)
        else:
            assert ldpc.coded_len(n, rate) == want > prev                       # strictly increasing in n
            prev = want
    blocks = 0
    for m in range(4101):
        assert ldpc.payload_len(m, rate) == c.payload_len(m), m
        assert (c.payload_len(m) is not None) == (PB + 4 <= m <= 4032 and (m - 1) % 192 >= PB)
        blocks += c.payload_len(m) is not None
    assert blocks == maxp + 1
    for m in (PB + 3, 192 + PB, 4033):
        assert ldpc.payload_len(m, rate) is None
    assert ldpc.payload_len(192 + PB + 1, rate) == KI - 3 and ldpc.payload_len(PB + 4, rate) == 0
    with pytest.raises(ValueError):
        ldpc.coded_len(-1, rate)
    assert ldpc.payload_len(-1, rate) is None and ldpc.payload_len(1 << 33, rate) is None
    lib = _abi.load()
    v = C.c_uint32(77)
    r = rc.RATE_IDS[rate]
    assert lib.ofdm_ldpc_coded_len_rate(r, 5, None) == _abi.OFDM_E_INVAL and lib.ofdm_ldpc_payload_len_rate(r, 192, None) == _abi.OFDM_E_INVAL
    assert lib.ofdm_ldpc_payload_len_rate(r, PB + 3, C.byref(v)) == _abi.OFDM_E_INVAL and v.value == 77
    assert lib.ofdm_ldpc_coded_len_rate(4, 5, C.byref(v)) == _abi.OFDM_E_INVAL and v.value == 77       # no such rate
    assert lib.ofdm_ldpc_payload_len_rate(4, 192, C.byref(v)) == _abi.OFDM_E_INVAL and v.value == 77
    # the two names without a rate mean rate 1/2; a config names the rate as well as a string does
    assert ldpc.coded_len(92) == ldpc.coded_len(92, "1/2") == ldpc.coded_len(92, None) == 192
    assert ldpc.coded_len(300, ldpc.ldpc_cfg(rate=rate)) == c.coded_len(300)
    # a length that is a block at one rate need not be one at another
    assert [ldpc.payload_len(100, q) is not None for q in rc.RATES] == [True, True, True, True]
    assert [ldpc.payload_len(192 + 40, q) is not None for q in rc.RATES] == [False, False, False, True]


# ---- 5. round trips of the model -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", NEW_RATES)
def test_model_round_trips_clean_and_with_flips(rate):
    c = rc.code(rate)
    PB = c.CW_PARITY
    rng = np.random.default_rng(11)
    for n in sizes(c):
        p = rand_payload(n, 1)
        b = c.encode(p)
        assert c.decode(b) == (1, p, 0, 1, 0)
        pos = np.flatnonzero(rng.random(8 * len(b)) < FLIPS[rate])
        ok, got, corrected, iters, failed = c.decode(rc.flip(b, pos))
        assert (ok, got, failed) == (1, p, 0) and corrected == len(pos) and 1 <= iters <= 20
    assert iters > 1                                                             # (the longest block needed more than one)
    for m in (0, PB + 3, 192 + PB, 4033):
        assert c.decode(bytes(m)) == rc.NO_BLOCK
    assert c.decode_values(np.ones(8 * 192 + 1, np.int8)) == rc.NO_BLOCK
    # nothing but erasures: every check holds for the all-zero word, whose CRC field does not match
    n = c.CW_INFO - 4
    assert c.decode_values(np.zeros(8 * c.coded_len(n), np.int8)) == (0, bytes(n), 0, 1, 0)
    # max_iters bounds the decoder
    p = rand_payload(2 * c.CW_INFO - 4, 5)
    b = c.encode(p)
    bad = rc.flip(b, np.flatnonzero(rng.random(8 * len(b)) < 2 * FLIPS[rate]))
    full = c.decode(bad)
    assert full[0] == 1 and full[3] > 2
    one = c.decode(bad, 1)
    assert one[3] == 1 and one[4] >= 1
    assert c.decode(bad, full[3])[:2] == (1, p) and c.decode(bad, full[3] - 1)[4] >= 1


# ---- 6. configuration --------------------------------------------------------------------------------------------------------------
def test_cfg_helpers():
    c = ldpc.ldpc_cfg()
    assert (c.struct_size, c.max_iters, list(c.reserved)) == (32, 20, [0] * 6) and c.rate == _abi.OFDM_LDPC_RATE_1_2 == 0
    assert C.sizeof(_abi.ofdm_ldpc_cfg) == 32 and _abi.ofdm_ldpc_cfg.rate.offset == 8 == _abi.ofdm_ldpc_cfg.reserved.offset
    for i, rate in enumerate(rc.RATES):
        c = ldpc.ldpc_cfg(rate=rate)
        assert (c.struct_size, c.max_iters, c.rate, list(c.reserved)) == (32, 20, i, [i, 0, 0, 0, 0, 0])
        assert ldpc.ldpc_cfg(7, i).rate == i and ldpc.rate_id(c) == i and ldpc.rate_id(rate) == i
        assert ldpc.as_cfg(dict(rate=rate, max_iters=3)).rate == i and ldpc.as_cfg(dict(rate=rate)).max_iters == 20
    assert (_abi.OFDM_LDPC_RATE_2_3, _abi.OFDM_LDPC_RATE_3_4, _abi.OFDM_LDPC_RATE_5_6) == (1, 2, 3)
    assert ldpc.rate_id(None) == 0 and ldpc.as_cfg(True).rate == 0 and ldpc.as_cfg(7).rate == 0
    for bad in ("4/5", "", 4, -1, True, False, 0.5, 1.0, b"1/2"):
        with pytest.raises(ValueError):
            ldpc.ldpc_cfg(rate=bad)
        with pytest.raises(ValueError):
            ldpc.as_cfg(dict(rate=bad))
    for bad in ("4/5", 4, True):
        with pytest.raises(ValueError):
            ldpc.coded_len(10, bad)
    with pytest.raises(ValueError):
        ldpc.as_cfg(dict(rate="3/4", iters=3))
    assert [ldpc.max_payload(r) for r in rc.RATES] == [2012, 2684, 3020, 3356] and ldpc.MAX_PAYLOAD == 2012
    # the largest RS block that fits the inner code at each rate
    want = [1752, 2328, 2632, 2904]
    assert [rs.max_payload_under(ldpc.max_payload(r)) for r in rc.RATES] == want and want[0] == rs.MAX_PAYLOAD_UNDER_LDPC
    for r, n in zip(rc.RATES, want):
        assert rs.coded_len(n) <= ldpc.max_payload(r) < rs.coded_len(n + 1)


def test_header_and_exports():
    with open(os.path.join(ROOT, "include", "ofdm_hip.h")) as f:
        hdr = f.read()
    lib = _abi.load()
    for name in ("ofdm_ldpc_coded_len_rate", "ofdm_ldpc_payload_len_rate"):
        assert name + "(" in hdr and name in _abi.EXPORTS and hasattr(lib, name)
    for i, r in enumerate(("1_2", "2_3", "3_4", "5_6")):
        assert re.search(r"#define\s+OFDM_LDPC_RATE_%s\s+%d\b" % (r, i), hdr)
    assert "#define OFDM_ABI_VERSION 6" in hdr and _abi.OFDM_ABI_VERSION == 6
    # the tables in the header's comment are the model's
    for rate in NEW_RATES:
        kb = rc.code(rate).KB
        rows = re.findall(r"^ \* +%s (\d+):((?: +(?:-|\d+)){%d})$" % (re.escape(rate), kb), hdr, re.M)
        assert [int(r[0]) for r in rows] == list(range(rc.code(rate).ROWS))
        for i, (_, cells) in enumerate(rows):
            assert [(-1 if c == "-" else int(c)) for c in cells.split()] == list(rc.INFO_SHIFTS[rate][i])


# ---- 7. the host arithmetic as a program of its own -------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [["-O1"], ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitizers"])
def test_rate_plan_checker(tmp_path, flags):
    exe = str(tmp_path / "ldpc_rate_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-I", os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tools", "ldpc_rate_plan_check.cpp")])
    out = subprocess.check_output([exe]).decode()
    assert out.strip().endswith("ldpc_rate_plan_check ok")
