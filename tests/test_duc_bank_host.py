"""Host side of the DUC bank (duc.bank_cfg, the float64 model and the float32 emulation of duc_bank_cases, the
ofdm_duc_bank_* part of the C ABI, ofdm_mod_bank's argument checks): no GPU needed."""
import ctypes
import re

import numpy as np
import pytest

import duc_bank_cases as bc
import duc_cases
import stage_harness as sh
from ofdm_uhd_amd import _abi, ddc, duc, ofdm

BANK_FUNCS = ("ofdm_set_duc_bank", "ofdm_duc_bank_reset", "ofdm_duc_bank", "ofdm_duc_bank_taps", "ofdm_duc_bank_last_ms")


def test_header_declares_the_bank_and_the_library_exports_it():
    _, code = sh.check_header_declares_and_library_exports(BANK_FUNCS)
    assert re.search(r"#define\s+OFDM_DUC_BANK_MAX_LINKS\s+8\b", code) and _abi.OFDM_DUC_BANK_MAX_LINKS == 8 == bc.MAX_LINKS


def test_struct_layout_matches_the_header(tmp_path):
    """sizeof / offsetof as the C compiler sees include/ofdm_hip.h == the ctypes mirror."""
    st = _abi.ofdm_duc_bank_cfg
    assert [f for f, _ in st._fields_] == ["struct_size", "interpolation", "ntaps", "nlinks", "out_format", "out_scale",
                                          "center_freq", "taps"]
    sh.check_cfg_layout_matches_header(tmp_path, st, 24 + 8 * 8 + 4 * 1024)


def test_bank_cfg_builder_and_its_refusals():
    c = duc.bank_cfg(4, [0.25, -0.125], occupied_fraction=200 / 512.0)
    assert (c.struct_size, c.interpolation, c.nlinks, c.out_format, c.out_scale) == (ctypes.sizeof(_abi.ofdm_duc_bank_cfg), 4, 2, 0, 0.0)
    assert list(c.center_freq) == [0.25, -0.125] + [0.0] * 6
    assert np.array_equal(np.ctypeslib.as_array(c.taps)[:c.ntaps], duc.design(4, 200 / 512.0))
    c = duc.bank_cfg(64, [0.5] * 8, taps=np.ones(1024, np.float32), out_format="sc16", out_scale=1000.0)
    assert (c.nlinks, c.ntaps, c.out_format, c.out_scale) == (8, 1024, _abi.OFDM_IQ_SC16, 1000.0)    # equal frequencies are allowed
    assert duc.bank_cfg(8, 0.1, taps=[1.0]).nlinks == 1                                              # ntaps < L, one link
    for bad in (dict(center_freqs=[]), dict(center_freqs=[0.0] * 9), dict(center_freqs=[0.1, 0.5000001]),
                dict(center_freqs=[-0.6]), dict(center_freqs=[0.1, float("nan")]), dict(center_freqs=[float("inf")]),
                dict(taps=[]), dict(taps=np.zeros(1025, np.float32)), dict(taps=[1.0, float("nan")]),
                dict(taps=[float("inf")]), dict(interpolation=0), dict(interpolation=65), dict(out_format="u8"),
                dict(out_scale=-1.0), dict(out_scale=float("nan"))):
        kw = dict(interpolation=4, center_freqs=[0.1, -0.2], taps=np.ones(3, np.float32))
        kw.update(bad)
        with pytest.raises(ValueError):
            duc.bank_cfg(**kw)
    with pytest.raises(ValueError):
        duc.bank_cfg(4, [0.1])                          # neither taps nor occupied_fraction


def _rows(rng, K, n, amp=0.25):
    return (amp * (rng.standard_normal((K, n)) + 1j * rng.standard_normal((K, n)))).astype(np.complex64)


def test_model_is_the_sum_of_the_duc_models():
    rng = np.random.default_rng(3)
    K, L, ntaps, first = 3, 4, 31, 1000003
    x, h, fcs = _rows(rng, K, 200), bc.taps_for(rng, ntaps), bc.freqs(K)
    y, s = bc.model(x, h, L, fcs, first)
    want = sum(duc_cases.model(x[i], h, L, duc_cases.phase_step(fcs[i]), first)[0] for i in range(K))
    assert len(y) == 200 * L and np.array_equal(y, want) and np.all(s >= 0)
    assert len(bc.model(x[:, :0], h, L, fcs)[0]) == 0
    # the identity the bank rests on: the shift on the input side with the band-pass table is the same signal
    m = first + np.arange(200)
    n = first * L + np.arange(200 * L)
    alt = np.zeros(200 * L, np.complex128)
    for i, fc in enumerate(fcs):
        up = np.zeros(200 * L, np.complex128)
        up[::L] = x[i] * np.exp(2j * np.pi * ((fc * L * m) % 1.0))
        c = h.astype(np.float64) * np.exp(2j * np.pi * fc * np.arange(ntaps))
        alt += np.convolve(up, c)[:200 * L]
    # (the zeros before the stream's first index stand where the model has them; the phase reference is n = 0)
    assert np.max(np.abs(alt - y)) <= 1e-6 * np.max(np.abs(y)), float(np.max(np.abs(alt - y)))
    assert n[0] == first * L


@pytest.mark.parametrize("K,L,ntaps", bc.HOST_SHAPES)
def test_float32_emulation_of_the_definition_stays_within_the_bound(K, L, ntaps):
    rng = np.random.default_rng(1000 * K + 10 * L + ntaps)
    nin = max(3 * bc.history(ntaps, L) + 50, 600 // L + 7)
    x, h, fcs = _rows(rng, K, nin), bc.taps_for(rng, ntaps), bc.freqs(K)
    add = _rows(rng, 1, nin * L)[0]
    worst = 0.0
    for first in (0, 1000003, (1 << 40) - 5):
        y64, s = bc.model(x, h, L, fcs, first)
        for a in (None, add):
            got = bc.emulate(x, h, L, fcs, first, a).astype(np.complex128)
            want = y64 + (a.astype(np.complex128) if a is not None else 0.0)
            err, bound = np.abs(got - want), bc.bound(K, ntaps, L, s, a)
            assert np.all(err <= bound), (K, L, ntaps, first)
            assert np.all(got[bound == 0] == 0)                       # no tap, or nothing under the taps yet: exactly 0
            worst = max(worst, float(np.max(err / np.maximum(bound, 1e-300))))
    print("K=%d L=%d ntaps=%d: worst error / bound = %.3g" % (K, L, ntaps, worst))


def test_emulation_anchors():
    """What the GPU tests pin bit for bit holds in the emulation of the definition: one link at fc = 0 is the plain
    real-tap chain; a zero link in front or behind changes nothing; the table is ddc.bandpass_taps."""
    rng = np.random.default_rng(9)
    L, ntaps = 4, 31
    x, h = _rows(rng, 2, 120), bc.taps_for(rng, ntaps)
    one = bc.emulate(x[:1], h, L, [0.0])
    up = np.zeros(120 * L)
    chain = np.zeros(120 * L, np.complex128)
    for part in ("real", "imag"):
        up[::L] = getattr(x[0], part)
        acc = np.zeros(120 * L, np.float32)
        for k in range(ntaps):                       # ascending q inside each phase is ascending k
            sh = np.concatenate([np.zeros(k), up[:len(up) - k]]).astype(np.float32)
            sel = (np.arange(120 * L) % L) == (k % L)
            acc[sel] = bc._fma32(np.float32(h[k]) * np.ones(sel.sum(), np.float32), sh[sel], acc[sel])
        chain = chain + (acc if part == "real" else 1j * acc)
    assert np.array_equal(one, chain.astype(np.complex64))
    z = np.zeros((1, 120), np.complex64)
    two = bc.emulate(x, h, L, [0.2, -0.3])
    assert np.array_equal(bc.emulate(np.concatenate([z, x]), h, L, [0.1, 0.2, -0.3]), two)
    assert np.array_equal(bc.emulate(np.concatenate([x, z]), h, L, [0.2, -0.3, 0.1]), two)
    assert np.array_equal(ddc.bandpass_taps(h, 0.0), h.astype(np.complex64))


def test_shapes_of_the_gpu_tests():
    for L in (1, 2, 3, 4, 8, 64):
        n, T = bc.stream_inputs(L), bc.tile_outputs(L)
        assert 2 * T < n * L < 3 * T and (n * L) % T != 0 and (L == 1 or n % L != 0)
        for ntaps in (1, 31, 1024):
            Q, Ti = bc.history(ntaps, L), max(T // L, 1)
            total = 3 * Ti + 100 + 3 * Q
            sizes = bc.chunk_inputs(np.random.default_rng(L), total, L, ntaps)
            assert sum(sizes) == total and sizes[0] == 0
            assert {1, Q + 1, Ti + 1} | ({Ti - 1} if Ti > 1 else set()) | ({Q} if Q else set()) | ({Q - 1} if Q > 1 else set()) <= set(sizes)
    assert all(abs(f) <= 0.5 for f in bc.freqs(8)) and len(set(bc.freqs(8))) == 8


def test_entry_points_refuse_a_null_handle_without_a_gpu():
    lib = _abi.load()
    n, k, ms = ctypes.c_uint64(7), ctypes.c_int(7), ctypes.c_double(7.0)
    good = duc.bank_cfg(2, [0.1], taps=[1.0])
    assert lib.ofdm_set_duc_bank(None, None) == _abi.OFDM_E_INVAL
    assert lib.ofdm_set_duc_bank(None, ctypes.byref(good)) == _abi.OFDM_E_INVAL
    assert lib.ofdm_duc_bank_reset(None, 0) == _abi.OFDM_E_INVAL
    assert lib.ofdm_duc_bank(None, None, 0, 0, None, None, 0, ctypes.byref(n)) == _abi.OFDM_E_INVAL
    assert lib.ofdm_duc_bank_taps(None, 0, None, 0, ctypes.byref(k)) == _abi.OFDM_E_INVAL
    assert lib.ofdm_duc_bank_last_ms(None, ctypes.byref(ms)) == _abi.OFDM_E_INVAL
    assert (n.value, k.value, ms.value) == (7, 7, 7.0)            # nothing was written


@pytest.mark.parametrize("kw", [
    dict(center_freqs=[]), dict(center_freqs=[0.0] * 9), dict(center_freqs=[0.1, 0.6]), dict(center_freqs=[float("nan")]),
    dict(interpolation=0), dict(interpolation=65), dict(taps=[]), dict(taps=[float("nan")]), dict(iq_format="u8"),
    dict(iq_scale=-1.0), dict(options=3),
])
def test_mod_bank_checks_its_arguments_before_any_engine_exists(kw, monkeypatch):
    sh.check_arguments_are_checked_before_any_engine_exists(
        monkeypatch, ofdm.ofdm_mod_bank, ("options", "center_freqs", "interpolation"),
        dict(center_freqs=[0.2, -0.1], interpolation=4), kw)


def test_mod_bank_drops_a_failing_batch_on_every_link():
    sh.check_mod_links_drops_a_failing_batch_on_every_link(ofdm.ofdm_mod_bank, "duc_bank",
                                                           duc.bank_cfg(4, [0.0, 0.1, 0.2], taps=[1.0]))


def test_the_two_multi_link_modulators_share_one_flush():
    assert ofdm.ofdm_mod_bank.flush is ofdm.ofdm_mod_channelizer.flush
    assert ofdm.ofdm_mod_bank._stage == "duc_bank" and ofdm.ofdm_mod_channelizer._stage == "pfb_synth"
