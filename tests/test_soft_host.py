"""Soft-decision receive without a GPU: the NumPy model of tests/soft_cases.py against the definition's own consequences
(every constellation point gives its own bits at full confidence, the placement map is a bijection, zero and non-finite
equaliser entries), the exports and NULL-handle refusals of the loaded library, the ctypes mirror of ofdm_soft_cfg, and
the host arithmetic of csrc/soft_plan.h through the stand-alone checker tools/soft_plan_check.cpp."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import soft_cases as sc
import stage_harness as sh
from helpers import make_cfg
from ofdm_uhd_amd import _abi, config, ofdm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODS = ("bpsk", "qpsk", "8psk", "qam8", "qam16", "qam64", "qam256")
SOFT_FUNCS = ["ofdm_set_rx_soft", "ofdm_rx_soft", "ofdm_rx_fec_decode_soft", "ofdm_rx_soft_last_ms"]


def test_every_modulation_is_covered():
    """MODS is every constellation options.modulation accepts (config.MODS): 1, 2, 3, 4, 6 and 8 bits per carrier."""
    assert sorted(MODS) == sorted(config.MODS)
    bits = []
    for mod in MODS:
        cfg = make_cfg(mod, 64, 48, 16)
        bits.append(int(cfg.arity).bit_length() - 1)
        assert 1 << bits[-1] == cfg.arity
    assert bits == [1, 2, 3, 3, 4, 6, 8]


@pytest.mark.parametrize("mod", MODS)
def test_every_point_gives_its_own_bits(mod):
    """A noiseless sink row at every constellation point, a flat equaliser: value (carrier, bit) has the sign of the
    point's bit, and |v| >= scale, since |D0 - D1| >= dmin2 there and w = wbar makes the factor scale / dmin2."""
    cfg = make_cfg(mod, 64, 48, 16)
    cst, smap = sc.cst_of(cfg), sc.smap_of(cfg)
    arity, nmap = len(cst), len(smap)
    nbits = arity.bit_length() - 1
    plen = 2 * (-(-arity * nbits // 8)) + 7
    ncar = sc.carriers_needed(plen, nbits)
    pts = np.arange(ncar) % arity
    nsym = -(-ncar // nmap)
    x = np.zeros(nsym * nmap, np.complex64)
    x[:ncar] = cst[pts]
    eq = np.full(cfg.occupied_tones, 0.25 - 0.5j, np.complex64)
    for scale in (32.0, 5.0):
        v = sc.packet_values(x, eq, smap, cst, plen, np.zeros(4096, np.uint8), scale)
        car, bit, idx, mb, e = sc.placement(plen, nbits, ncar)
        want = (pts[car] >> bit) & 1
        assert np.array_equal(v[idx] > 0, want.astype(bool))
        assert (np.abs(v[idx].astype(int)) >= min(int(scale), 127)).all()
        # the whitening mask negates exactly the values of its set bits
        mask = sc.mask_of(cfg)
        vm = sc.packet_values(x, eq, smap, cst, plen, mask, scale)
        flip = ((mask[mb] >> e) & 1).astype(bool)
        assert np.array_equal(vm[idx], np.where(flip, -v[idx].astype(int), v[idx]).astype(np.int8))
    assert v.min() >= -127


@pytest.mark.parametrize("nbits", [1, 2, 3, 4, 6, 8])
def test_placement_is_a_bijection(nbits):
    for nmap in (8, 43, 48, 187):                       # nmap * nbits a multiple of 8, and not
        for plen in (1, 2, 29, 301):
            ncar = sc.carriers_needed(plen, nbits)
            car, bit, idx, mb, e = sc.placement(plen, nbits, ncar + nmap)
            assert sorted(idx.tolist()) == list(range(8 * plen))
            assert car.max() == ncar - 1                  # the carriers counted, and not one more
            beta = car * nbits + bit
            assert np.array_equal(beta >> 3, mb + 4) and np.array_equal(beta & 7, e)
            assert np.array_equal(idx, 8 * mb + 7 - e)
    assert (nmap * nbits) % 8 != 0 or nbits == 8
    assert sc.carriers_needed(0, nbits) == 0


def _noisy_row(cfg, plen, seed):
    cst, smap = sc.cst_of(cfg), sc.smap_of(cfg)
    nbits = len(cst).bit_length() - 1
    ncar = sc.carriers_needed(plen, nbits)
    n = -(-ncar // len(smap)) * len(smap)
    rng = np.random.default_rng(seed)
    x = cst[rng.integers(0, len(cst), n)] + (0.05 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)
    eq = (1.0 + 0.3 * rng.standard_normal(cfg.occupied_tones) + 0.3j * rng.standard_normal(cfg.occupied_tones)).astype(np.complex64)
    return x.astype(np.complex64), eq, smap, cst, ncar, nbits


def test_zero_and_non_finite_eq_entries_silence_their_carrier_only():
    cfg = make_cfg("qam16", 64, 48, 16)
    plen = 40
    x, eq, smap, cst, ncar, nbits = _noisy_row(cfg, plen, 5)
    mask = sc.mask_of(cfg)
    base = sc.packet_values(x, eq, smap, cst, plen, mask)
    assert np.count_nonzero(base) > 0.9 * len(base)
    car, bit, idx, mb, e = sc.placement(plen, nbits, ncar)
    for bad in (0, np.nan, np.inf, complex(np.nan, 1.0), complex(0.0, -np.inf)):
        c0 = 7
        eq2 = eq.copy()
        eq2[smap[c0]] = bad
        v = sc.packet_values(x, eq2, smap, cst, plen, mask)
        hit = (car % len(smap)) == c0
        assert hit.any() and not v[idx[hit]].any()
        assert np.count_nonzero(v[idx[~hit]]) > 0.9 * np.count_nonzero(~hit)
        assert sc.weights(eq2)[smap[c0]] == 0
    # an entry outside the sink's map changes nothing
    off = np.setdiff1d(np.arange(cfg.occupied_tones), smap)
    eq3 = eq.copy()
    eq3[off] = np.nan
    assert np.array_equal(sc.packet_values(x, eq3, smap, cst, plen, mask), base)


def test_an_all_zero_eq_row_gives_an_all_zero_packet():
    cfg = make_cfg("qpsk", 64, 48, 16)
    plen = 33
    x, eq, smap, cst, ncar, nbits = _noisy_row(cfg, plen, 6)
    mask = sc.mask_of(cfg)
    for row in (np.zeros_like(eq), np.full_like(eq, np.nan), np.full_like(eq, 1e-30)):   # wbar 0, 0, +inf
        v = sc.packet_values(x, row, smap, cst, plen, mask)
        assert v.shape == (8 * plen,) and not v.any()
    assert len(sc.packet_values(x, eq, smap, cst, 0, mask)) == 0


def test_a_hard_decision_in_values_decodes_as_the_bytes():
    """Values that are all +-1 or larger with the signs of a block decode exactly as the block's bytes do."""
    import fec_cases as fc
    rng = np.random.default_rng(8)
    p = rng.integers(0, 256, 21, dtype=np.uint8).tobytes()
    blk = fc.flip(fc.encode(p), [3, 90, 200])
    v = fc.hard_values(blk).astype(np.int32) * rng.integers(1, 128, 8 * len(blk))
    assert fc.decode_values(v.astype(np.int8))[:2] == fc.decode(blk)[:2] == (1, p)


def test_header_exports_and_layout(tmp_path):
    sh.check_header_declares_and_library_exports(SOFT_FUNCS)
    sh.check_cfg_layout_matches_header(tmp_path, _abi.ofdm_soft_cfg, 8, ())


def test_null_handle_refusals():
    lib = _abi.load()
    n = C.c_int(0)
    ms = C.c_double(0)
    cfg = _abi.ofdm_soft_cfg(struct_size=C.sizeof(_abi.ofdm_soft_cfg), scale=32.0)
    assert lib.ofdm_set_rx_soft(None, C.byref(cfg)) == _abi.OFDM_E_INVAL
    assert lib.ofdm_set_rx_soft(None, None) == _abi.OFDM_E_INVAL
    assert lib.ofdm_rx_soft(None, None, 0, None, C.byref(n)) == _abi.OFDM_E_INVAL
    assert lib.ofdm_rx_fec_decode_soft(None, None, None, 0, None, None, None, 0, C.byref(n)) == _abi.OFDM_E_INVAL
    assert lib.ofdm_rx_soft_last_ms(None, C.byref(ms)) == _abi.OFDM_E_INVAL


def test_ofdm_demod_takes_soft():
    import inspect
    assert "soft" in inspect.signature(ofdm.ofdm_demod.__init__).parameters


def test_plan_checker(tmp_path):
    """The host arithmetic as a program of its own (the build a sanitizer run uses adds -fsanitize=address,undefined)."""
    exe = str(tmp_path / "soft_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tools", "soft_plan_check.cpp")])
    out = subprocess.check_output([exe]).decode()
    assert out.strip().endswith("soft_plan_check ok")
