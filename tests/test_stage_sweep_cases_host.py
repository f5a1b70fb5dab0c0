"""stage_sweep_cases.py without a GPU: the lists are seeded, every case is accepted by its stage's cfg builder, every
listed class has a case, the float64 model runs on every case and, for the transmit stages, stays below half of the
16-bit full scale on its own."""
import ctypes as C

import numpy as np
import pytest

import pfb_cases
import stage_harness as sh
import stage_sweep_cases as sw


@pytest.mark.parametrize("stage", sw.STAGE_NAMES)
def test_the_lists_are_seeded(stage):
    a, b = sw.cases.__wrapped__(stage), sw.cases.__wrapped__(stage)
    assert a == b == sw.cases(stage) and len(a) >= sw.RANDOM_CASES + len(sw.BOUNDARY_SHAPES[stage])
    assert [c.idx for c in a] == list(range(len(a)))
    assert sum(c.why == "random" for c in a) == sw.RANDOM_CASES
    assert len(set(sw.SEEDS.values())) == len(sw.STAGE_NAMES) == len(sh.STAGES)


@pytest.mark.parametrize("stage", sw.STAGE_NAMES)
def test_every_listed_class_and_boundary_has_a_case(stage):
    cs = sw.cases(stage)
    have = set().union(*(sw.classes_of(stage, c.shape, c.ntaps, c.sel) for c in cs))
    assert have == set(sw.CLASSES[stage])
    assert set(sw.BOUNDARY_SHAPES[stage]) <= {c.shape for c in cs}
    P = {c.ntaps - c.shape[0] for c in cs}
    assert {-1, 0, 1} <= P and {1, 1024} <= {c.ntaps for c in cs}          # P - 1, P, P + 1; the ends
    assert any(c.ntaps % c.shape[0] == 0 and c.ntaps > c.shape[0] > 1 for c in cs)
    st = sh.STAGES[stage]
    firsts = {c.first for c in cs}
    assert 0 in firsts and (st.phase_free or {sh.START, sh.FAR} <= firsts)
    assert st.phase_free or any(c.first == st.index_limit(*c.shape) - c.n - 1 for c in cs)
    assert any(0 < c.first < 1000 and (max(c.shape) == 1 or c.first % max(c.shape)) for c in cs)
    if st.rows and st.sel_field == "center_freq":
        assert {1, 3, 8} <= {len(c.sel) for c in cs} <= set(range(1, 9))
        fcs = {f for c in cs for f in c.sel}
        assert {0.0, 0.5, -0.5} <= fcs and any(len(set(c.sel)) < len(c.sel) for c in cs)
    if st.sel_field == "channel":
        for ch in (lambda M: 0, lambda M: M // 2, lambda M: M - 1):
            assert any(ch(c.shape[0]) in c.sel for c in cs)


@pytest.mark.parametrize("stage", sw.STAGE_NAMES)
def test_every_case_is_accepted_and_shaped_as_the_sweep_needs(stage):
    st = sh.STAGES[stage]
    for c in sw.cases(stage):
        for fmt in (("fc32", "sc16") if st.side == "tx" else (None,)):
            cfg = sw.cfg_of(c, fmt)
            assert cfg.struct_size == C.sizeof(type(cfg)) and cfg.ntaps == c.ntaps
        tile = st.tile_inputs(*c.shape)
        assert 2 * tile < c.n <= 5 * tile // 2 + c.ntaps + 2 * max(c.shape) + 4                       # three tiles, no more
        assert c.n < 12000 and sum(c.chunks) == c.n and 0 in c.chunks and 1 in c.chunks
        assert 0 <= c.first and c.first + c.n <= st.index_limit(*c.shape)
        at = [sum(c.chunks[:k]) for k in range(len(c.chunks))]
        empty = [s for a, s in zip(at, c.chunks) if s and st.count(c.first + a, s, *c.shape) == 0]
        can = any(st.count(c.first + j, 1, *c.shape) == 0 for j in range(c.n))
        assert bool(empty) == can, c


@pytest.mark.parametrize("stage", sw.STAGE_NAMES)
def test_the_model_runs_and_the_16_bit_reference_stays_unclamped(stage):
    st = sh.STAGES[stage]
    for c in sw.cases(stage):
        no = st.count(c.first, c.n, *c.shape)
        assert no > 0
        if st.side == "rx":
            for fmt in ("fc32", "sc16"):
                raw, x = sw.rx_input(c, fmt)
                assert len(raw) == len(x) == c.n and x.dtype == np.complex64
            if stage == "pfb":
                y64, s = pfb_cases.model(x, sw.taps_of(c), c.shape[0], c.sel[0], c.first)
            else:
                D = (sh.ddc_cases.phase_step(c.sel if not st.rows else c.sel[0], *c.shape) if len(c.shape) == 1 else
                     sh.resamp_cases.phase_step(c.sel if not st.rows else c.sel[0], *c.shape))
                cases = sh.ddc_cases if len(c.shape) == 1 else sh.resamp_cases
                y64, s = cases.model(x, sw.rx_table(c, 0 if st.rows else None), *c.shape, D, c.first)
            assert len(y64) == len(s) == no and np.all(np.isfinite(y64)) and np.all(s >= 0)
            continue
        x = sw.tx_input(c)
        assert x.shape == ((len(c.sel), c.n) if st.rows else (c.n,)) and x.dtype == np.complex64
        y64, s = sw.tx_model(stage, c.shape, sw.taps_of(c), c.sel, c.first, x)
        assert len(y64) == no and np.all(np.isfinite(y64))
        # the condition of check_tx_model on the reference alone: nothing clamps, the peak is below half of full scale
        peak = max(np.max(np.abs(y64.real)), np.max(np.abs(y64.imag)))
        assert 0.2 * sw.HALF_SCALE < peak < sw.HALF_SCALE, (c, peak)
        free = (np.abs(y64.real) * sh.SCALE < 32767 - 1) & (np.abs(y64.imag) * sh.SCALE < 32767 - 1)
        assert np.count_nonzero(free) > 0.9 * no and np.log2(c.amp) == np.floor(np.log2(c.amp))
