"""The spectrum stage without a GPU: the float64 model of psd_cases on signals whose spectrum is known, the host-side
figures of ofdm_uhd_amd/spectrum.py on hand-made densities and on a trapezoid with closed-form answers, the refusals of
psd_cfg, the layout of ofdm_psd_cfg as the C compiler sees it, the host arithmetic of csrc/psd_plan.h through the
stand-alone checker tools/psd_plan_check.cpp, and the float64 amplifier chain in ACLR.

The amplifier chain (psd_cases.pa_probe: band-limited noise, rms 0.2, polar-clipped at 7 dB; 127 segments of 1024 at hop
512; adjacent bands 0.2 wide, 0.02 away), lower / upper ACLR in dB as this test measured them here:
    the amplifier's input                                 40.89 / 40.53
    behind dpd.example_pa()                               39.00 / 37.74
    behind it after two rounds of indirect learning, 3x3  40.80 / 40.55
The differences are 1.8 to 2.8 dB; the test asserts each in order with a margin of 1 dB."""
import math
import os
import subprocess

import numpy as np
import pytest

import psd_cases as pc
import stage_harness as sh
from ofdm_uhd_amd import _abi, dpd, spectrum

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the model on known signals -------------------------------------------------------------------------------------
def test_white_noise_reads_its_power_in_every_bin():
    """Independent segments (hop = F) of complex white noise of power sigma^2: a bin's density is sigma^2 times a mean
    of nseg unit exponentials, standard deviation sigma^2 / sqrt(nseg); the mean over the bins is the stream's power
    under the window, standard deviation at most sigma^2 / sqrt(nseg) / sqrt(F / 4) (a Blackman-Harris window correlates
    about four neighbouring bins)."""
    F, nseg, sigma2 = 256, 400, 0.37
    rng = np.random.default_rng(2)
    x = math.sqrt(sigma2 / 2) * (rng.standard_normal(F * nseg) + 1j * rng.standard_normal(F * nseg))
    w = pc.taps(F)
    r = pc.welch64(x, F, F, w)
    assert r["nseg"] == nseg
    d = spectrum.density(r["sum"], r["nseg"], w)
    sd = sigma2 / math.sqrt(nseg)
    assert np.all(np.abs(d - sigma2) < 6 * sd)
    assert abs(np.mean(d) - sigma2) < 6 * sd / math.sqrt(F / 4)
    assert spectrum.band_power(d, -0.5, 0.5) == pytest.approx(float(np.mean(d)), rel=1e-12)


@pytest.mark.parametrize("name", spectrum.WINDOWS)
def test_an_on_bin_tone_under_each_window(name):
    """A tone of amplitude A on bin k0: the row's peak is A^2 (sum w)^2, the power over the whole band A^2."""
    F, k0, A = 128, 37, 0.3
    w = spectrum.window_taps(name, F)
    x = A * np.exp(2j * np.pi * k0 * np.arange(5 * F) / F)
    r = pc.welch64(x, F, F // 2, w)
    assert r["nseg"] == 9
    assert r["peak"][k0] == pytest.approx(A * A * float(np.sum(w.astype(np.float64))) ** 2, rel=1e-9)
    assert int(np.argmax(r["sum"])) == k0
    d = spectrum.density(r["sum"], r["nseg"], w)
    assert spectrum.band_power(d, -0.5, 0.5) == pytest.approx(A * A, rel=1e-9)
    # the host estimator of the package is the same definition
    h = spectrum.welch(x, F, F // 2, name)
    assert h["nseg"] == 9 and np.allclose(h["sum"], r["sum"], rtol=1e-12, atol=1e-18) and np.allclose(h["peak"], r["peak"], rtol=1e-12)


# ---- 2. band_power -----------------------------------------------------------------------------------------------------
def test_band_power_takes_bins_by_their_overlapped_fraction_and_wraps():
    d = np.arange(1.0, 9.0)                       # F = 8: bin k covers [(k - 1/2) / 8, (k + 1/2) / 8)
    bp = spectrum.band_power
    assert bp(d, -1 / 16, 1 / 16) == pytest.approx(d[0] / 8)
    assert bp(d, 0.0, 1 / 8) == pytest.approx((d[0] / 2 + d[1] / 2) / 8)
    assert bp(d, 1 / 32, 1 / 16 + 1 / 64) == pytest.approx((d[0] / 4 + d[1] / 8) / 8)
    assert bp(d, -3 / 16, -1 / 16) == pytest.approx(d[7] / 8)                       # a negative frequency is bin F - 1
    assert bp(d, 0.45, 0.55) == pytest.approx(0.8 * d[4] / 8)                       # across 1/2: one bin, 0.8 of it
    assert bp(d, 0.45 - 3, 0.55 - 3) == pytest.approx(0.8 * d[4] / 8)               # frequencies are cyclic
    assert bp(d, 7 / 16 - 1 / 32, 9 / 16 + 1 / 32) == pytest.approx((d[3] / 4 + d[4] + d[5] / 4) / 8)
    assert bp(d, -0.5, 0.5) == pytest.approx(np.mean(d)) and bp(d, 0.3, 1.3) == pytest.approx(np.mean(d))
    assert bp(d, 0.2, 0.2) == 0.0
    for lo, hi in ((0.0, 1.01), (0.2, 0.1), (float("nan"), 0.1)):
        with pytest.raises(ValueError):
            bp(d, lo, hi)
    assert np.array_equal(spectrum.ascending(np.arange(8)), [4, 5, 6, 7, 0, 1, 2, 3])
    assert np.array_equal(spectrum.freqs(8, "ascending"), np.arange(-4, 4) / 8.0)
    assert np.array_equal(spectrum.freqs(8), np.fft.fftfreq(8))


# ---- 3. a trapezoid with closed-form figures ---------------------------------------------------------------------------
F_T, K1, K2, GAP, EPS = 1024, 100, 150, 10, 0.01
F1, F2 = (K1 + 0.5) / F_T, (K2 + 0.5) / F_T          # the kinks lie on bin edges: a midpoint sum is exact for every piece


def _g(f):
    f = abs(f)
    return 1.0 if f <= F1 else (EPS if f >= F2 else 1.0 - (1.0 - EPS) * (f - F1) / (F2 - F1))


def _trapezoid(shift=0):
    d = np.array([_g(f) for f in np.fft.fftfreq(F_T)])
    return np.roll(d, shift)


def test_aclr_of_a_trapezoid():
    bw, sp = 2 * F1, 2 * F1 + GAP / F_T
    a = F1 + GAP / F_T                                                     # where the upper adjacent band begins
    adj = 0.5 * (_g(a) + EPS) * (F2 - a) + EPS * (a + bw - F2)             # the skirt's trapezium, then the floor
    want = 10 * math.log10(bw / adj)
    lo, hi = spectrum.aclr_db(_trapezoid(), 0.0, bw, sp)
    assert lo == pytest.approx(want, abs=1e-9) and hi == pytest.approx(want, abs=1e-9)
    # anywhere on the axis, and across 1/2
    for shift in (77, 512, 1000):
        lo, hi = spectrum.aclr_db(_trapezoid(shift), shift / F_T, bw, sp)
        assert lo == pytest.approx(want, abs=1e-9) and hi == pytest.approx(want, abs=1e-9)
    # an adjacent band that reaches the channel is refused
    for b, s in ((0.2, 0.19), (0.4, 0.61), (0.0, 0.1), (-0.1, 0.2)):
        with pytest.raises(ValueError):
            spectrum.aclr_db(_trapezoid(), 0.0, b, s)
    spectrum.aclr_db(_trapezoid(), 0.0, 0.4, 0.6)                          # (the bands just touch around the axis)


def test_occupied_bandwidth_of_a_trapezoid():
    side = EPS * (0.5 - F2) + 0.5 * (1.0 + EPS) * (F2 - F1)                # floor and skirt on one side
    total = 2 * F1 + 2 * side
    d = _trapezoid()
    assert spectrum.band_power(d, -0.5, 0.5) == pytest.approx(total, rel=1e-12)
    # 99 %: half a percent lies in the floor on either side
    tail = 0.005 * total
    assert tail < EPS * (0.5 - F2)
    assert spectrum.occupied_bandwidth(d, 0.99) == pytest.approx(1.0 - 2 * tail / EPS, abs=1e-9)
    lo, hi = spectrum.occupied_band(d, 0.99)
    assert lo == pytest.approx(-0.5 + tail / EPS, abs=1e-9) and hi == pytest.approx(0.5 - tail / EPS, abs=1e-9)
    # 50 %: a quarter lies beyond either edge, which is inside the flat top
    tail = 0.25 * total
    assert tail > side
    assert spectrum.occupied_bandwidth(d, 0.5) == pytest.approx(2 * (F1 - (tail - side)), abs=1e-9)
    # the same around a centre anywhere on the axis
    for shift in (300, 512, 900):
        assert spectrum.occupied_bandwidth(_trapezoid(shift), 0.99, center=shift / F_T) == pytest.approx(1.0 - 2 * 0.005 * total / EPS, abs=1e-9)
        lo, hi = spectrum.occupied_band(_trapezoid(shift), 0.5, center=shift / F_T)
        assert 0.5 * (lo + hi) == pytest.approx(shift / F_T, abs=1e-9)
    for share in (0.0, 1.0, 1.5):
        with pytest.raises(ValueError):
            spectrum.occupied_bandwidth(d, share)


def test_mask_margin_of_a_trapezoid():
    bw = 2 * F1
    a = F1 + GAP / F_T
    mask = [(a, F2, -3.0), (F2, 0.4, -25.0), (-F2, -a, -3.0), (-0.4, -F2, -18.0)]
    margin, at = spectrum.mask_margin_db(_trapezoid(), mask, 0.0, bw)
    # the channel's mean density is 1; the floor reads -20 dBc against a limit of -25: 5 dB outside the mask
    assert margin == pytest.approx(-5.0, abs=1e-9) and at["segment"] == 1 and at["level_dbc"] == pytest.approx(-20.0, abs=1e-9)
    assert F2 <= at["freq"] < 0.4 and at["limit_dbc"] == -25.0
    # without that segment the skirt's first bin decides: its centre lies half a bin inside the segment
    level = 10 * math.log10(_g(a + 0.5 / F_T))
    margin, at = spectrum.mask_margin_db(_trapezoid(), [mask[0], mask[2], mask[3]], 0.0, bw)
    assert margin == pytest.approx(-3.0 - level, abs=1e-9) and at["segment"] in (0, 1)
    assert abs(at["freq"]) == pytest.approx(a + 0.5 / F_T, abs=1e-12)
    # shifted along the axis the figures stay
    m2, at2 = spectrum.mask_margin_db(_trapezoid(700), mask, 700 / F_T, bw)
    assert m2 == pytest.approx(-5.0, abs=1e-9) and at2["segment"] == 1
    with pytest.raises(ValueError):
        spectrum.mask_margin_db(_trapezoid(), [(0.2, 0.1, -10.0)], 0.0, bw)
    with pytest.raises(ValueError):
        spectrum.mask_margin_db(_trapezoid(), [], 0.0, bw)


def test_report_ties_the_figures_together():
    w = pc.taps(F_T)
    w2 = float(np.sum(w.astype(np.float64) ** 2))
    d = _trapezoid()
    read = {"sum": d * 7 * w2, "peak": (2 * d * w2).astype(np.float32), "nseg": 7}
    bw, sp = 2 * F1, 2 * F1 + GAP / F_T
    r = spectrum.report(read, spectrum.psd_cfg(F_T), center=0.0, bandwidth=bw, spacing=sp, mask=[(F2, 0.4, -25.0)])
    assert np.allclose(r["density"], d, rtol=1e-12) and np.allclose(r["peak"], 2 * d, rtol=1e-6) and r["nseg"] == 7
    assert r["aclr_db"] == spectrum.aclr_db(r["density"], 0.0, bw, sp) and r["obw"] == spectrum.occupied_bandwidth(r["density"], 0.99, 0.0)
    assert r["mask_margin_db"] == pytest.approx(-5.0, abs=1e-6) and r["channel_power"] == pytest.approx(bw, rel=1e-9)
    plain = spectrum.report(read, w)
    assert "aclr_db" not in plain and plain["obw"] == pytest.approx(r["obw"], abs=1e-12)
    with pytest.raises(ValueError):
        spectrum.report({"sum": d, "peak": d, "nseg": 0}, w)


# ---- 4. the configuration ----------------------------------------------------------------------------------------------
def test_psd_cfg_and_its_refusals():
    cfg = spectrum.psd_cfg(1024)
    assert (cfg.nfft, cfg.hop, cfg.in_format, cfg.in_scale) == (1024, 512, _abi.OFDM_IQ_FC32, 0.0)
    assert np.array_equal(spectrum.taps_of(cfg), pc.taps(1024))
    cfg = spectrum.psd_cfg(64, 1, np.arange(1, 65), "sc16", 1.0 / 2048)
    assert (cfg.nfft, cfg.hop, cfg.in_format) == (64, 1, _abi.OFDM_IQ_SC16) and cfg.in_scale == np.float32(1.0 / 2048)
    assert np.array_equal(spectrum.taps_of(cfg), np.arange(1, 65, dtype=np.float32))
    for bad in (dict(nfft=32), dict(nfft=8192), dict(nfft=96), dict(nfft=100.5), dict(nfft=256, hop=0), dict(nfft=256, hop=257),
                dict(nfft=256, hop=1.5), dict(nfft=256, window="kaiser"), dict(nfft=256, window=np.ones(255)),
                dict(nfft=256, window=np.zeros(256)), dict(nfft=256, window=np.r_[np.ones(255), np.nan]),
                dict(nfft=256, window=np.r_[np.ones(255), np.inf]), dict(nfft=256, in_format="fc64"),
                dict(nfft=256, in_format="sc16", in_scale=-1.0), dict(nfft=256, in_format="sc16", in_scale=float("inf"))):
        with pytest.raises(ValueError):
            spectrum.psd_cfg(**bad)
    assert [spectrum.segments(n, 64, 16) for n in (0, 63, 64, 79, 80, 96)] == [0, 0, 1, 1, 2, 3]


def test_cfg_layout_matches_the_header(tmp_path):
    got = sh.check_cfg_layout_matches_header(tmp_path, _abi.ofdm_psd_cfg, 20 + 4 * 4096, macros=(("maxfft", "OFDM_PSD_MAX_FFT"),))
    assert int(got["maxfft"]) == _abi.OFDM_PSD_MAX_FFT == spectrum.MAX_FFT == 4096
    for name in ("ofdm_set_psd", "ofdm_psd_reset", "ofdm_psd_count", "ofdm_psd", "ofdm_psd_read", "ofdm_psd_last_ms"):
        assert name in _abi.EXPORTS


def test_the_case_list_covers_what_the_kernel_distinguishes():
    Fs = {c[0] for c in pc.CASES}
    assert Fs == {64, 512, 1024, 2048, 4096}
    for F in Fs:
        G = pc.groups(F)
        mine = [c for c in pc.CASES if c[0] == F]
        assert {F, F // 2, F // 4 + 3} <= {c[1] for c in mine}
        assert {0, 1, G - 1, G, G + 1} <= {c[2] for c in mine}
        assert any(pc.plan(c[2], F)[1] > G for c in mine)          # a workgroup with more than one round
        assert any((c[2] - 1) % G == 0 and c[2] > G + 1 for c in mine)   # one more than a whole number of shares
    assert (64, 1, 0) in pc.CASES and pc.groups(64) == 32 and pc.groups(4096) == 1
    assert pc.samples_for(0, 64, 1) == 63 and pc.samples_for(3, 64, 16) == 96


def test_plan_checker(tmp_path):
    """The host arithmetic as a program of its own (the build a sanitizer run uses adds -fsanitize=address,undefined)."""
    exe = str(tmp_path / "psd_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tools", "psd_plan_check.cpp")])
    out = subprocess.check_output([exe]).decode()
    assert out.strip().endswith("psd_plan_check ok")


# ---- 5. what the transmit chain is for ---------------------------------------------------------------------------------
def test_the_amplifier_costs_aclr_and_the_fitted_table_gives_it_back():
    x = pc.pa_probe()
    pa = dpd.example_pa()
    a_in = pc.aclr_of(x)
    a_pa = pc.aclr_of(dpd.apply64(x, pa))
    coef = pc.fit64(x, pa)
    a_dpd = pc.aclr_of(dpd.apply64(dpd.apply64(x, coef), pa))
    print("ACLR lower / upper: input %.2f / %.2f, amplifier %.2f / %.2f, predistorted %.2f / %.2f dB" % (a_in + a_pa + a_dpd))
    for side in (0, 1):
        assert a_pa[side] < a_in[side] - 1.0          # the amplifier's figures are worse than its input's
        assert a_dpd[side] > a_pa[side] + 1.0         # behind the fitted table they are better than the amplifier's alone
