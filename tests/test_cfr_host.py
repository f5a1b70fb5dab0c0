"""CPU tests of the crest-factor reduction stage (ofdm_uhd_amd/cfr.py, include/ofdm_hip.h): the model the GPU tests
compare with bit for bit keeps the definition's promises before any GPU sees it, and the host-side helpers do what they
say.

Peak bound, max |y| <= A (1 + 2^-22) + 2^-24 max |x| (four float32 roundings on the path m, A / m, 1 - c, b x; the
subtraction's error is absolute, hence the term in max |x|).  Worst max |y| / A - 1 measured here: 7.8e-8 over the
cases, 1.2e-7 over Gaussian streams of 20000 samples at 3, 4.5, 6, 7.5 and 9 dB with H = 16; 2^-22 is 2.4e-7."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cfr_cases as cc
import stage_harness as sh
from ofdm_uhd_amd import _abi, cfr, options


@pytest.mark.parametrize("name", cc.NAMES)
def test_the_models_output_stays_under_the_threshold(name):
    c = cc.CASES[name]
    x = cc.input_of(name)
    t = cc.model_of(name)
    top = float(np.abs(t.y.astype(np.complex128)).max())
    print("%s: max |y| / A - 1 = %.3g" % (name, top / float(np.float32(c.threshold)) - 1.0))
    assert top <= cc.peak_bound(c.threshold, x)
    assert np.array_equal(t.xd[c.H:], x[:len(x) - c.H]) and not t.xd[:c.H].any()      # the delay is H


def test_the_peak_bound_on_gaussian_streams_at_3_to_9_db():
    worst = 0.0
    for seed, db in enumerate((3.0, 4.5, 6.0, 7.5, 9.0)):
        x = cc.stream(20000, seed=200 + seed)
        A = cfr.threshold_for(db, cc.rms(x))
        t = cc.model(x, A, cfr.design(16))
        top = float(np.abs(t.y.astype(np.complex128)).max())
        worst = max(worst, top / float(np.float32(A)) - 1.0)
        assert top <= cc.peak_bound(A, x)
    print("worst max |y| / A - 1 = %.3g" % worst)


def test_the_cases_are_what_the_tests_say_they_are():
    assert [n for n in cc.NAMES if n.startswith("under")] == ["under_h16"]
    assert len(cc.NAMES) == 4 * 3 + 1
    for name in cc.NAMES:
        c, t = cc.CASES[name], cc.model_of(name)
        st = cc.statistics(t, c.threshold)
        assert st["n"] == cc.length(c.H) >= 2 * cc.TILE + 2 * c.H + 301
        share = st["n_over"] / float(st["n"])
        if name.startswith("none"):
            assert st["n_over"] == st["n_touched"] == 0 and np.all(t.b == 1.0)
        elif name.startswith("papr7"):
            assert 0.002 <= share <= 0.02 and st["n_touched"] >= st["n_over"]
            # tiles (and stretches of 64 + 2 H samples) without a peak exist next to ones with
            if c.H <= 16:
                assert np.any(t.b[:cc.TILE] < 1.0) and np.any(np.all(t.b.reshape(-1)[:2 * cc.TILE].reshape(-1, 64) == 1.0, axis=1))
        elif name.startswith("under"):
            assert share > 0.5
            assert np.any(t.b == 0.0) and np.any((t.b > 0.0) & (t.b < 1.0)) and np.any(t.s > 1.0)
        else:
            assert st["n_over"] == st["n"]


def test_half_width_0_is_the_polar_clip():
    for name in ("none_h0", "papr7_h0", "all_h0"):
        c = cc.CASES[name]
        x = cc.input_of(name)
        assert np.array_equal(cc.model_of(name).y, cc.polar_clip(x, c.threshold))
    x = cc.input_of("papr7_h0")
    A = cc.CASES["papr7_h0"].threshold
    y = cc.polar_clip(x, A).astype(np.complex128)
    over = np.abs(x.astype(np.complex128)) > A * (1 + 1e-6)
    assert over.any() and np.allclose(np.abs(y[over]), A, rtol=1e-6) and np.allclose(np.angle(y[over]), np.angle(x[over]), atol=1e-6)


@pytest.mark.parametrize("name", cc.NAMES)
def test_skipping_zero_terms_leaves_s_unchanged_in_bits(name):
    c = cc.CASES[name]
    x = cc.input_of(name)
    a = cc.model(x, c.threshold, cfr.design(c.H))
    b = cc.model(x, c.threshold, cfr.design(c.H), skip_zero_terms=True)
    assert np.array_equal(a.s.view(np.uint32), b.s.view(np.uint32)) and np.array_equal(a.y.view(np.uint32), b.y.view(np.uint32))


def test_design_invariants():
    for H in (0, 1, 2, 16, 100, 511):
        for kind in ("hann", "triangular", "rect"):
            w = cfr.design(H, kind)
            assert w.dtype == np.float32 and len(w) == 2 * H + 1 and w[H] == 1.0
            assert np.all(w > 0.0) and np.all(w <= 1.0) and np.array_equal(w, w[::-1])
            if kind != "rect":
                assert np.all(np.diff(w[:H + 1]) > 0)
            cfr.cfr_cfg(1.0, w)
    assert np.array_equal(cfr.design(0), [1.0])
    for bad in (-1, 512, 1.5):
        with pytest.raises(ValueError):
            cfr.design(bad)
    with pytest.raises(ValueError):
        cfr.design(4, "kaiser")


def test_cfr_cfg_round_trips_and_refuses_what_the_library_refuses():
    w = cfr.design(16)
    cfg = cfr.cfr_cfg(0.75, w, out_format="sc16", out_scale=30000)
    assert cfg.struct_size == C.sizeof(_abi.ofdm_cfr_cfg) and cfg.ntaps == 33 and cfr.half_width(cfg) == 16
    assert cfg.threshold == 0.75 and np.array_equal(cfr.window_of(cfg), w)
    assert (cfg.out_format, cfg.out_scale) == (_abi.OFDM_IQ_SC16, 30000.0)
    d = cfr.cfr_cfg(1.0)
    assert d.ntaps == 33 and d.out_format == _abi.OFDM_IQ_FC32 and d.out_scale == 0.0
    nan, inf = float("nan"), float("inf")
    half = w.copy()
    half[16] = 0.5
    bad = [dict(threshold=0.0), dict(threshold=-1.0), dict(threshold=nan), dict(threshold=inf),
           dict(threshold=1.0, window=np.ones(2)), dict(threshold=1.0, window=np.ones(1025)), dict(threshold=1.0, window=[]),
           dict(threshold=1.0, window=half), dict(threshold=1.0, window=[0.5, 1.0, 1.5]),
           dict(threshold=1.0, window=[-0.1, 1.0, 0.5]), dict(threshold=1.0, window=[nan, 1.0, 0.5]),
           dict(threshold=1.0, out_format="sc8"), dict(threshold=1.0, out_format="sc16", out_scale=0.0)]
    for kw in bad:
        with pytest.raises(ValueError):
            cfr.cfr_cfg(**kw)
    cfr.cfr_cfg(1e-30, np.ones(1023))          # the edges


def test_threshold_modem_rms_and_report():
    assert cfr.threshold_for(6.0, 0.5) == pytest.approx(0.5 * 10 ** 0.3, rel=1e-15) and cfr.threshold_for(0.0, 2.0) == 2.0
    for bad in ((float("nan"), 1.0), (6.0, 0.0), (6.0, -1.0), (6.0, float("inf"))):
        with pytest.raises(ValueError):
            cfr.threshold_for(*bad)
    opt = options.default_options(modulation="qpsk")
    opt.fft_length, opt.occupied_tones, opt.tx_amplitude = 512, 200, 0.25
    assert cfr.modem_rms(opt) == pytest.approx(0.25 * np.sqrt(200 / 512.0), rel=1e-15)
    st = dict(n=1000, n_over=10, n_touched=50, peak_in=16.0, peak_out=4.0, sum_in=2000.0, sum_out=1000.0, sum_err=20.0)
    r = cfr.report(st)
    assert r["papr_in_db"] == pytest.approx(10 * np.log10(8.0)) and r["papr_out_db"] == pytest.approx(10 * np.log10(4.0))
    assert r["evm_db"] == pytest.approx(-20.0) and (r["share_over"], r["share_touched"]) == (0.01, 0.05)
    r = cfr.report(st, rms=1.0)
    assert r["papr_in_db"] == pytest.approx(10 * np.log10(16.0)) and r["papr_out_db"] == pytest.approx(10 * np.log10(4.0))
    assert r["mean_in_db"] == pytest.approx(10 * np.log10(2.0)) and r["mean_out_db"] == pytest.approx(0.0)
    with pytest.raises(ValueError):
        cfr.report(dict(st, n=0))
    # on a case: the figures of the model's statistics
    c = cc.CASES["papr7_h16"]
    r = cfr.report(cc.statistics(cc.model_of("papr7_h16"), c.threshold))
    assert 7.0 < r["papr_in_db"] < 13.0 and r["papr_out_db"] < r["papr_in_db"] and -40.0 < r["evm_db"] < -10.0


def test_abi_declares_exports_and_lays_out_the_two_structs(tmp_path):
    funcs = ("ofdm_set_cfr", "ofdm_cfr_reset", "ofdm_cfr", "ofdm_cfr_stats", "ofdm_cfr_last_ms")
    hdr, code = sh.check_header_declares_and_library_exports(funcs)
    assert "ofdm_cfr_cfg" in code and "struct ofdm_cfr_stats" in code
    got = sh.check_cfg_layout_matches_header(tmp_path, _abi.ofdm_cfr_cfg, 4112, macros=(("maxtaps", "OFDM_CFR_MAX_TAPS"),))
    assert int(got["maxtaps"]) == _abi.OFDM_CFR_MAX_TAPS == 1023
    assert [f for f, _ in _abi.ofdm_cfr_cfg._fields_] == ["struct_size", "threshold", "ntaps", "out_format", "out_scale", "taps"]
    # the statistics are a struct tag (the name is the function's): sizeof / offsetof as gcc sees the header
    st = _abi.ofdm_cfr_stats
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ofdm_hip.h"', 'int main(void){',
             'printf("size %zu\\n", sizeof(struct ofdm_cfr_stats));']
    for f, _ in st._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(struct ofdm_cfr_stats, %s));' % (f, f))
    lines.append('return 0;}')
    src = tmp_path / "stats_layout.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "stats_layout")
    subprocess.check_call(["gcc", "-I", os.path.join(sh.ROOT, "include"), "-o", exe, str(src)])
    out = dict(l.split() for l in subprocess.check_output([exe]).decode().splitlines())
    assert int(out["size"]) == C.sizeof(st) == 56
    for f, _ in st._fields_:
        assert int(out[f]) == getattr(st, f).offset, f
    assert [f for f, _ in st._fields_] == ["n", "n_over", "n_touched", "peak_in", "peak_out", "sum_in", "sum_out", "sum_err"]
