"""CPU tests of the propagation channel stage (ofdm_uhd_amd/multipath.py, include/ofdm_hip.h): the bound the GPU tests
hold the kernel to is attainable and sharp before any GPU sees it, and the host-side helpers do what they say.

The float32 emulation (multipath_cases.emulate: the kernel's operations in NumPy float32, libm in the hardware
transcendentals' place) lies within (P + J + 16) 2^-24 S + 1e-4 sigma of the float64 model for every profile, every
start and with `add`; worst error / bound measured here: 0.108 ("doppler4", first index 0, with `add`; "late_only" 0.098,
"everything" 0.026).  Each mutated emulation misses the same bound by far more than 10x (the smallest: the noise word
of n xor 1 on "everything", 2.3e4 times the bound)."""
import numpy as np
import pytest

import multipath_cases as mc
import stage_harness as sh
from ofdm_uhd_amd import _abi, multipath

N = 2 * mc.TILE + 1023 + 301          # longer than two tiles plus the longest history
STARTS = (0, sh.START, sh.FAR)


@pytest.mark.parametrize("name", mc.NAMES)
def test_float32_emulation_lies_within_the_bound(name):
    cfg = mc.cfg_of(name)
    x = mc.stream(N, seed=3)
    w = mc.stream(N, seed=4)
    for first in STARTS:
        for add in (None, w):
            y64, S = mc.model(x, cfg, first, add)
            r = mc.ratio(mc.emulate(x, cfg, first, add), y64, mc.bound(cfg, S))
            print("%s first %d add %s: worst error / bound = %.3g" % (name, first, add is not None, r))
            assert r <= 1.0


MUTATIONS = [
    # (profile, keywords of multipath_cases.emulate)
    ("unit", dict(delay_off=(0, 1))),
    ("two_ray", dict(delay_off=(1, -1))),
    ("late_only", dict(delay_off=(0, -1))),
    ("everything", dict(delay_off=(7, 1))),
    ("doppler4", dict(doppler_at=1)),
    ("everything", dict(doppler_at=1)),
    ("everything", dict(word_xor=1)),
    ("two_ray", dict(conj_gain=True)),
    ("twins", dict(conj_gain=True)),
    ("everything", dict(conj_gain=True)),
    ("tones4", dict(tone_phase=False)),
    ("everything", dict(tone_phase=False)),
    ("two_ray", dict(drop_history_at=mc.TILE)),
    ("late_only", dict(drop_history_at=997)),
    ("everything", dict(drop_history_at=2 * mc.TILE + 1)),
]


@pytest.mark.parametrize("name,mutation", MUTATIONS, ids=["%s-%s" % (n, "-".join(m)) for n, m in MUTATIONS])
def test_a_mutated_emulation_misses_the_bound_tenfold(name, mutation):
    cfg = mc.cfg_of(name)
    x = mc.stream(N, seed=3)
    y64, S = mc.model(x, cfg, sh.START)
    r = mc.ratio(mc.emulate(x, cfg, sh.START, **mutation), y64, mc.bound(cfg, S))
    print("%s %s: worst error / bound = %.3g" % (name, mutation, r))
    assert r >= 10.0


def test_model_of_the_unit_profile_is_the_input_and_of_noise_the_flat_channel():
    import chan_cases
    x = mc.stream(500)
    y64, S = mc.model(x, mc.cfg_of("unit"), 77)
    assert np.array_equal(y64, x.astype(np.complex128)) and np.array_equal(S, np.abs(x.astype(np.complex128)))
    kw = dict(sigma=0.01, cfo=0.002, seed=chan_cases.BIG_SEED, stream_id=3)
    y64, _ = mc.model(x, mc.cfg_of("unit", **kw), 77)
    assert np.array_equal(y64, chan_cases.model(x, index0=77, **kw)[0])


def test_turns_is_the_librarys_phase_convention():
    assert mc.turns(0.0) == 0 and mc.turns(0.5) == 1 << 63 and mc.turns(-0.5) == 1 << 63
    assert mc.turns(0.25) == 1 << 62 and mc.turns(-0.25) == 3 << 62 and mc.turns(1.25) == 1 << 62
    assert mc.turns(-1e-30) == 0            # frac rounds up to a whole turn: phase 0


def test_frequency_response_is_the_fft_of_the_impulse_response():
    for name in ("unit", "two_ray", "dense16", "twins", "late_only"):
        cfg = mc.cfg_of(name)
        for n in (1024, 2048):
            h = np.zeros(n, np.complex128)
            for d, g, _ in multipath.paths_of(cfg):
                h[d] += g
            assert np.allclose(multipath.frequency_response(cfg, n), np.fft.fft(h), rtol=0, atol=1e-12)
    # shorter than the longest delay: the delays wrap, as the circular convolution of an OFDM symbol does
    cfg = mc.cfg_of("late_only")
    h = np.zeros(512, np.complex128)
    h[1023 % 512] = multipath.paths_of(cfg)[0][1]
    assert np.allclose(multipath.frequency_response(cfg, 512), np.fft.fft(h), rtol=0, atol=1e-12)
    with pytest.raises(ValueError):
        multipath.frequency_response(mc.cfg_of("doppler4"), 512)


def test_multipath_cfg_round_trips_and_refuses_what_the_library_refuses():
    cfg = multipath.multipath_cfg(paths=[(0, 1), (4, 0.5j, 1e-4)], tones=[(0.01, 0.125), (0.02, -0.3, 0.25)], sigma=0.01,
                                  cfo=0.002, seed=5, stream_id=(9 << 32) | 1, out_format="sc16", out_scale=32767)
    assert cfg.struct_size == _abi.C.sizeof(_abi.ofdm_multipath_cfg) and (cfg.npaths, cfg.ntones) == (2, 2)
    assert multipath.paths_of(cfg) == [(0, 1 + 0j, 0.0), (4, 0.5j, 1e-4)]
    assert multipath.tones_of(cfg) == [(float(np.float32(0.01)), 0.125, 0.0), (float(np.float32(0.02)), -0.3, 0.25)]
    assert (cfg.sigma, cfg.cfo) == (float(np.float32(0.01)), float(np.float32(0.002)))
    assert (cfg.seed, cfg.stream_id, cfg.out_format, cfg.out_scale) == (5, (9 << 32) | 1, _abi.OFDM_IQ_SC16, 32767.0)
    assert multipath.max_delay(cfg) == 4
    d = multipath.multipath_cfg()
    assert multipath.paths_of(d) == [(0, 1 + 0j, 0.0)] and d.ntones == 0 and d.out_scale == 0.0 and d.seed == 0xC0FFEE
    nan, inf = float("nan"), float("inf")
    bad = [dict(paths=[]), dict(paths=[(0, 1)] * 17), dict(tones=[(0.1, 0.1)] * 5), dict(paths=[(1024, 1)]),
           dict(paths=[(-1, 1)]), dict(paths=[(1.5, 1)]), dict(paths=[(0, inf)]), dict(paths=[(0, complex(0, nan))]),
           dict(paths=[(0, 1, 0.5000001)]), dict(paths=[(0, 1, nan)]), dict(paths=[(0,)]), dict(tones=[(-0.1, 0.1)]),
           dict(tones=[(nan, 0.1)]), dict(tones=[(0.1, 0.51)]), dict(tones=[(0.1, nan)]), dict(tones=[(0.1, 0.1, inf)]),
           dict(tones=[(0.1,)]), dict(sigma=-1e-3), dict(sigma=inf), dict(sigma=nan), dict(cfo=nan), dict(cfo=inf),
           dict(out_format="sc8"), dict(out_format="sc16", out_scale=0.0), dict(out_format="sc16", out_scale=inf)]
    for kw in bad:
        with pytest.raises(ValueError):
            multipath.multipath_cfg(**kw)
    multipath.multipath_cfg(paths=[(1023, 1, 0.5), (1023, 1, -0.5)], tones=[(0.0, 0.5, -7.25)] * 4)   # the edges


def test_parse_reads_the_command_lines_specifications():
    assert multipath.parse("0:1;4:0.35+0.35j;9:0.1@1e-4") == [(0, 1 + 0j), (4, 0.35 + 0.35j), (9, 0.1 + 0j, 1e-4)]
    assert multipath.parse(" 3:-0.5j ; ") == [(3, -0.5j)]
    assert multipath.parse_tones("0.01:0.125;0.02:-0.3@0.25") == [(0.01, 0.125), (0.02, -0.3, 0.25)]
    assert multipath.parse_tones("") == []
    for name in mc.NAMES:
        paths = mc.PROFILES[name].paths
        back = multipath.parse(multipath.format_paths(paths))
        assert multipath.paths_of(multipath.multipath_cfg(paths=back)) == multipath.paths_of(mc.cfg_of(name))
    for bad in ("", "1", "x:1", "0:1@", "0:one", "0:1;4", "0:1@zero", "-1:1"):
        with pytest.raises(ValueError):
            multipath.parse(bad)
    for bad in ("0.1", "a:0.1", "0.1:0.2@x"):
        with pytest.raises(ValueError):
            multipath.parse_tones(bad)


def test_sigma_for_snr():
    assert multipath.sigma_for_snr(30.0, 1.0) == pytest.approx(10.0 ** -1.5, rel=1e-15)
    assert multipath.sigma_for_snr(0.0, 0.25) == 0.5 and multipath.sigma_for_snr(20.0, 0.0) == 0.0
    x = mc.stream(4000)
    p = float(np.mean(np.abs(x.astype(np.complex128)) ** 2))
    s = multipath.sigma_for_snr(17.0, p)
    assert 10.0 * np.log10(p / s ** 2) == pytest.approx(17.0, abs=1e-12)
    for bad in ((float("nan"), 1.0), (10.0, -1.0), (10.0, float("inf"))):
        with pytest.raises(ValueError):
            multipath.sigma_for_snr(*bad)


def test_exponential_profile():
    paths = multipath.exponential_profile(np.random.default_rng(5), 8, 12.0)
    delays = [d for d, _ in paths]
    assert len(paths) == 8 and delays[0] == 0 and delays == sorted(set(delays)) and delays[-1] <= 72
    assert sum(abs(g) ** 2 for _, g in paths) == pytest.approx(1.0, rel=1e-12)
    multipath.multipath_cfg(paths=paths)
    assert [d for d, _ in multipath.exponential_profile(np.random.default_rng(5), 16, 1000.0)][-1] <= 1023
    (d0, g0), = multipath.exponential_profile(np.random.default_rng(5), 1, 3.0)
    assert d0 == 0 and abs(g0) == pytest.approx(1.0, rel=1e-12)
    for bad in ((0, 3.0), (17, 3.0), (4, 0.0), (4, float("nan"))):
        with pytest.raises(ValueError):
            multipath.exponential_profile(np.random.default_rng(5), *bad)


def test_profiles_are_what_the_tests_say_they_are():
    d16 = [d for d, _, _ in multipath.paths_of(mc.cfg_of("dense16"))]
    assert len(set(d16)) == 16 and min(d16) == 0 and max(d16) == 1023 and d16[-1] != 1023
    assert [mc.dmax_of(n) for n in mc.NAMES] == [0, 4, 1023, 7, 1023, 40, 0, 1023]
    ev = mc.cfg_of("everything")
    assert sum(1 for _, _, f in multipath.paths_of(ev) if f != 0.0) == 4 and ev.ntones == 4 and ev.sigma > 0 and ev.cfo != 0
    assert [f for _, _, f in multipath.paths_of(mc.cfg_of("doppler4"))] == [0.0, 1e-4, -3e-3, 0.5]
    tones = multipath.tones_of(mc.cfg_of("tones4"))
    assert sorted(f for _, f, _ in tones)[:1] == [-0.5] and 0.0 in [f for _, f, _ in tones] and 0.5 in [f for _, f, _ in tones]
    assert sum(1 for _, _, ph in tones if ph != 0.0) == 1


def test_abi_declares_exports_and_lays_out_the_configuration(tmp_path):
    funcs = ("ofdm_set_multipath", "ofdm_multipath_reset", "ofdm_multipath", "ofdm_multipath_last_ms")
    hdr, code = sh.check_header_declares_and_library_exports(funcs)
    assert "ofdm_multipath_cfg" in code
    got = sh.check_cfg_layout_matches_header(tmp_path, _abi.ofdm_multipath_cfg, 448, macros=(
        ("paths", "OFDM_MULTIPATH_MAX_PATHS"), ("tones", "OFDM_MULTIPATH_MAX_TONES"), ("maxdelay", "OFDM_MULTIPATH_MAX_DELAY")))
    assert (int(got["paths"]), int(got["tones"]), int(got["maxdelay"])) == (
        _abi.OFDM_MULTIPATH_MAX_PATHS, _abi.OFDM_MULTIPATH_MAX_TONES, _abi.OFDM_MULTIPATH_MAX_DELAY) == (16, 4, 1023)
    order = [f for f, _ in _abi.ofdm_multipath_cfg._fields_]
    assert order == ["struct_size", "npaths", "ntones", "out_format", "out_scale", "sigma", "cfo", "seed", "stream_id",
                     "delay", "gain", "doppler", "tone_amp", "tone_freq", "tone_phase"]
