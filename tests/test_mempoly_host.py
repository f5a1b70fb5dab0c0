"""CPU tests of the memory-polynomial stage's host side (ofdm_uhd_amd/dpd.py, include/ofdm_hip.h): the float32 model the
GPU tests compare with bit for bit lies within its derived bound of the float64 model, the least-squares fit recovers a
known post-inverse, the training loop's arithmetic runs on the float64 model standing in for the engine, the ctypes
structs are laid out as gcc lays out the header's, and mempoly_cfg refuses what the library refuses.

Float32 against float64 (mempoly_cases.bound): the worst error / bound over the cases is 0.03 to 0.10; at (3, 3) the
worst error is 5e-8 absolute, 1.0e-7 of the output's peak."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mempoly_cases as mc
import stage_harness as sh
from ofdm_uhd_amd import _abi, dpd


@pytest.mark.parametrize("name", mc.NAMES)
def test_the_float32_model_lies_within_its_bound_of_the_float64_model(name):
    c = mc.CASES[name]
    x = mc.input_of(name)
    assert len(x) == mc.length(c.M) == 2 * mc.TILE + c.M - 1 + 301 and mc.CASES[name].coef.shape == (c.M, c.K)
    assert name == "example_pa" or np.abs(c.coef).max() <= 1.0
    assert mc.RMS * 0.97 < np.sqrt(np.mean(np.abs(x.astype(np.complex128)) ** 2)) < mc.RMS * 1.03
    t = mc.model(x, c.coef)
    y64 = mc.model64(x, c.coef)
    err = np.abs(t.y.astype(np.complex128) - y64)
    b = mc.bound(x, c.coef)
    worst = float(np.max(err / np.maximum(b, 1e-300)))
    print("%s: worst error / bound = %.3g, worst error %.3g, %.3g of the output's peak" % (
        name, worst, err.max(), err.max() / np.abs(y64).max()))
    assert np.all(np.isfinite(t.y.real) & np.isfinite(t.y.imag)) and np.all(err <= b)
    assert worst > 1e-3                              # the bound is not idle: float32 does differ


def test_the_model_at_its_anchors():
    x = mc.stream(3000, seed=5)
    assert np.array_equal(mc.model(x, dpd.identity(3, 3)).y, x)
    g = np.complex64(0.75 - 0.5j)
    want = np.empty(len(x), np.complex64)           # the gr_complex product, part by part
    want.real = g.real * x.real - g.imag * x.imag
    want.imag = g.real * x.imag + g.imag * x.real
    assert np.array_equal(mc.model(x, [[g]]).y.view(np.uint32), want.view(np.uint32))
    for m in (1, 7):
        a = np.zeros((8, 2), np.complex64)
        a[m, 0] = 1.0
        y = mc.model(x, a).y
        assert np.array_equal(y[m:], x[:len(x) - m]) and not y[:m].any()
    st = mc.statistics(mc.model(x, dpd.identity(1, 1)), limit=0.3)
    mag2 = x.real.astype(np.float32) ** 2 + x.imag.astype(np.float32) ** 2
    assert st["n"] == 3000 and st["peak_in"] == st["peak_out"] == float(mag2.max()) and st["sum_in"] == st["sum_out"]
    assert 0 < st["n_over"] == int(np.sum(mag2 > np.float32(0.3) * np.float32(0.3))) < 3000
    assert mc.statistics(mc.model(x, dpd.identity(1, 1)))["n_over"] == 0


def test_basis_is_the_definitions_regressors():
    x = mc.stream(50, seed=2).astype(np.complex128)
    B = dpd.basis(x, 3, 2)
    assert B.shape == (50, 6) and B.dtype == np.complex128
    for m in range(3):
        for k in range(2):
            want = np.concatenate([np.zeros(m), x[:50 - m] * np.abs(x[:50 - m]) ** (2 * k)])
            assert np.allclose(B[:, m * 2 + k], want, rtol=1e-15, atol=0.0)
    assert dpd.basis(x[:2], 3, 2).shape == (2, 6) and not dpd.basis(x[:2], 3, 2)[:, 4:].any()


def test_fit_recovers_a_known_post_inverse():
    """pa_in = (float64 model with table c0)(pa_out / gain): the least-squares solution is c0."""
    c0 = mc.table(3, 3, seed=11)
    g = 1.05 + 0.09j
    v = mc.stream(6000, seed=12).astype(np.complex128)
    u = dpd.apply64(v / g, c0)
    c = dpd.fit(u, v, 3, 3, gain=g)
    assert c.dtype == np.complex64 and c.shape == (3, 3)
    # orders 3 and 5 at rms 0.2 are scaled by p ~ 0.04 and p^2 ~ 0.0016: the columns' conditioning costs digits
    assert np.allclose(c, c0, rtol=0.0, atol=1e-4)
    # the default gain is the least-squares complex gain; an amplifier's table stands for its a[0][0]
    pa = dpd.example_pa()
    x = mc.polar_clip(mc.stream(6000, seed=13), 0.2 * 10 ** (7.0 / 20))
    y = dpd.apply64(x, pa)
    ls = np.vdot(x, y) / np.vdot(x, x)
    assert np.array_equal(dpd.fit(x, y, 3, 3), dpd.fit(x, y, 3, 3, gain=ls))
    assert np.array_equal(dpd.fit(x, y, 3, 3, gain=pa), dpd.fit(x, y, 3, 3, gain=complex(pa[0, 0])))
    for bad in (dict(memory=0), dict(memory=9), dict(orders=0), dict(orders=6)):
        with pytest.raises(ValueError):
            dpd.fit(x, y, **dict(dict(memory=3, orders=3), **bad))
    with pytest.raises(ValueError):
        dpd.fit(x, y[:-1], 3, 3)


def test_train_on_the_float64_model_linearises_the_example_amplifier():
    """A Gaussian stream at rms 0.2, peaks clipped at 7 dB: two iterations take the error against a[0][0] x down by far
    more than 20 dB (measured here: -23.1 dB without, -46.8 / -47.1 dB after one / two iterations)."""
    pa = dpd.example_pa()
    probe = mc.polar_clip(mc.stream(20000, seed=21), mc.RMS * 10 ** (7.0 / 20)).astype(np.complex64)
    eng = mc.Model64Engine(pa)
    coef, nmse = dpd.train(eng, probe, memory=3, orders=3, iterations=2)
    g = complex(pa[0, 0])
    before = dpd.nmse_db(mc.model64(probe, pa), g * probe.astype(np.complex128))
    print("NMSE without %.2f dB, per iteration %s" % (before, ", ".join("%.2f" % v for v in nmse)))
    assert coef.shape == (3, 3) and coef.dtype == np.complex64 and len(nmse) == 2
    assert nmse[-1] <= before - 20.0 and nmse[0] <= before - 20.0
    assert np.array_equal(dpd.coef_of(eng.dpd_cfg), coef)          # the last table is left loaded
    # the loop's arithmetic, written out
    u = probe
    v = eng.pa(u)
    for it in range(2):
        c = dpd.fit(u, v, 3, 3, g)
        u = mc.model64(probe, c).astype(np.complex64)
        v = eng.pa(u)
        assert dpd.nmse_db(v, g * probe.astype(np.complex128)) == nmse[it]
    assert np.array_equal(c, coef)
    # a test stream of another seed at the same level and clip is linearised as well
    other = mc.polar_clip(mc.stream(20000, seed=22), mc.RMS * 10 ** (7.0 / 20)).astype(np.complex64)
    lin = mc.model64(mc.model64(other, coef), pa)
    assert dpd.nmse_db(lin, g * other.astype(np.complex128)) <= before - 20.0
    with pytest.raises(ValueError):
        none = mc.Model64Engine(pa)
        none.pa_cfg = None
        dpd.train(none, probe)


def test_nmse_report_identity_and_example():
    assert dpd.nmse_db([1.1, 1.0], [1.0, 1.0]) == pytest.approx(10 * np.log10(0.01 / 2.0))
    assert dpd.nmse_db([1.0], [1.0]) == float("-inf")
    with pytest.raises(ValueError):
        dpd.nmse_db([1.0], [0.0])
    r = dpd.report(dict(n=1000, n_over=25, peak_in=0.2, peak_out=0.25, sum_in=40.0, sum_out=44.0))
    assert r["gain_db"] == pytest.approx(10 * np.log10(1.1)) and r["peak_expansion_db"] == pytest.approx(10 * np.log10(1.25))
    assert r["share_over"] == 0.025
    with pytest.raises(ValueError):
        dpd.report(dict(n=0, n_over=0, peak_in=0.0, peak_out=0.0, sum_in=0.0, sum_out=0.0))
    a = dpd.identity(8, 5)
    assert a.shape == (8, 5) and a[0, 0] == 1.0 and np.count_nonzero(a) == 1
    pa = dpd.example_pa()
    assert pa.shape == (3, 3) and pa.dtype == np.complex64 and pa[0, 0] == np.complex64(1.0513 + 0.0904j)
    assert pa[2, 2] == np.complex64(0.1229 + 0.1508j) and pa[1, 0] == np.complex64(-0.0680 - 0.0023j)


def test_mempoly_cfg_round_trips_and_refuses_what_the_library_refuses(tmp_path):
    a = mc.table(3, 4, seed=3)
    cfg = dpd.mempoly_cfg(a, out_format="sc16", out_scale=30000, limit=0.5)
    assert cfg.struct_size == C.sizeof(_abi.ofdm_mempoly_cfg) and (cfg.memory, cfg.orders) == (3, 4)
    assert np.array_equal(dpd.coef_of(cfg), a) and cfg.coef[1 * 5 + 2].re == float(a[1, 2].real)
    assert (cfg.out_format, cfg.out_scale, cfg.limit) == (_abi.OFDM_IQ_SC16, 30000.0, 0.5)
    d = dpd.mempoly_cfg(dpd.identity(1, 1))
    assert d.out_format == _abi.OFDM_IQ_FC32 and d.out_scale == 0.0 and d.limit == float("inf")
    nan, inf = float("nan"), float("inf")
    one = dpd.identity(2, 2)
    bad_table = one.copy()
    bad_table[1, 1] = nan
    inf_table = one.copy()
    inf_table[0, 1] = complex(0.0, inf)
    bad = [dict(coef=np.zeros((0, 3))), dict(coef=np.zeros((9, 1))), dict(coef=np.zeros((1, 0))), dict(coef=np.zeros((1, 6))),
           dict(coef=np.zeros(3)), dict(coef=bad_table), dict(coef=inf_table),
           dict(coef=one, limit=0.0), dict(coef=one, limit=-1.0), dict(coef=one, limit=nan), dict(coef=one, limit=-inf),
           dict(coef=one, out_format="sc8"), dict(coef=one, out_format="sc16", out_scale=0.0)]
    for kw in bad:
        with pytest.raises(ValueError):
            dpd.mempoly_cfg(**kw)
    dpd.mempoly_cfg(np.ones((8, 5)), limit=inf)     # the edges
    path = str(tmp_path / "coef.npy")
    np.save(path, a)
    assert np.array_equal(dpd.load_coef(path), a)
    np.save(path, np.zeros((9, 9)))
    with pytest.raises(ValueError):
        dpd.load_coef(path)


def test_abi_declares_exports_and_lays_out_the_two_structs(tmp_path):
    funcs = ("ofdm_set_mempoly", "ofdm_mempoly_reset", "ofdm_mempoly", "ofdm_mempoly_stats", "ofdm_mempoly_last_ms")
    hdr, code = sh.check_header_declares_and_library_exports(funcs)
    assert "ofdm_mempoly_cfg" in code and "struct ofdm_mempoly_stats" in code
    got = sh.check_cfg_layout_matches_header(tmp_path, _abi.ofdm_mempoly_cfg, 24 + 8 * 8 * 5, macros=(
        ("maxm", "OFDM_MEMPOLY_MAX_MEMORY"), ("maxk", "OFDM_MEMPOLY_MAX_ORDERS"), ("dpd", "(int)OFDM_MEMPOLY_DPD"),
        ("pa", "(int)OFDM_MEMPOLY_PA"), ("slots", "OFDM_MEMPOLY_SLOTS")))
    assert int(got["maxm"]) == _abi.OFDM_MEMPOLY_MAX_MEMORY == 8 and int(got["maxk"]) == _abi.OFDM_MEMPOLY_MAX_ORDERS == 5
    assert (int(got["dpd"]), int(got["pa"]), int(got["slots"])) == (_abi.OFDM_MEMPOLY_DPD, _abi.OFDM_MEMPOLY_PA, 2) == (0, 1, 2)
    assert [f for f, _ in _abi.ofdm_mempoly_cfg._fields_] == ["struct_size", "memory", "orders", "out_format", "out_scale",
                                                              "limit", "coef"]
    # the statistics are a struct tag (the name is the function's): sizeof / offsetof as gcc sees the header
    st = _abi.ofdm_mempoly_stats
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ofdm_hip.h"', 'int main(void){',
             'printf("size %zu\\n", sizeof(struct ofdm_mempoly_stats));']
    for f, _ in st._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(struct ofdm_mempoly_stats, %s));' % (f, f))
    lines.append('return 0;}')
    src = tmp_path / "stats_layout.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "stats_layout")
    subprocess.check_call(["gcc", "-I", os.path.join(sh.ROOT, "include"), "-o", exe, str(src)])
    out = dict(l.split() for l in subprocess.check_output([exe]).decode().splitlines())
    assert int(out["size"]) == C.sizeof(st) == 40
    for f, _ in st._fields_:
        assert int(out[f]) == getattr(st, f).offset, f
    assert [f for f, _ in st._fields_] == ["n", "n_over", "peak_in", "peak_out", "sum_in", "sum_out"]
