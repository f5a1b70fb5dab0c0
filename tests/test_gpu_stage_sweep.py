"""The ten wideband stream stages over the seeded, stratified sweep of stage_sweep_cases.py, one parameter per (stage,
sample format).  Every case: (a) the whole stream in one call against the stage's float64 model within its derived bound
(DESIGN.md section 7), every link or channel; (b) the case's chunking gives the same stored bits and every count is the
model's; (c) every link of a receive bank is the single stage bit for bit (a transmit bank has no per-link output to
compare: its anchors are in its own file); (d) a transmit stage run once more onto a band: one float32 addition per part
on the plain output, then the library's 16-bit store; (e) through device pointers, with 13 samples of SENTINEL behind
every row of the output: the host-mode bits, and the sentinel survives; (f) wherever the input is complex64 that device
run is made twice, the input pointer on an even and on an odd sample of its buffer (the 16-byte interior load)."""
import time

import numpy as np
import pytest

import pfb_cases
import stage_harness as sh
import stage_sweep_cases as sw
from helpers import make_cfg
from ofdm_uhd_amd import engine, iqio
from stage_harness import eng   # noqa: F401 (one handle per file)

pytestmark = pytest.mark.gpu

PAD = 13
FILL16 = -7777
PARAMS = [(s, f) for s in sw.STAGE_NAMES for f in ("fc32", "sc16")]


@pytest.fixture(scope="module")
def dev():
    e = engine.Engine(cfg=make_cfg(device_ptrs=True))
    yield e
    e.close()


def _what(case, fmt, more=""):
    return "%s #%d (%s) %s ntaps=%d first=%d n=%d %s%s" % (case.stage, case.idx, case.why, case.shape, case.ntaps,
                                                        case.first, case.n, fmt, more)


def _device_input(torch, flat, off):
    """The complex64 samples ``flat`` on the device, beginning ``off`` samples into a buffer on the 16-byte grid."""
    buf = torch.zeros(len(flat) + 2, dtype=torch.complex64, device="cuda")
    assert buf.data_ptr() % 16 == 0
    buf[off:off + len(flat)] = torch.from_numpy(np.ascontiguousarray(flat))
    return buf, buf.data_ptr() + 8 * off


def _rx_case(torch, eng, dev, st, case, fmt):
    shape, first, n, K = case.shape, case.first, case.n, (len(case.sel) if st.rows else 1)
    raw, x = sw.rx_input(case, fmt)
    taps, cfg = sw.taps_of(case), sw.cfg_of(case)
    no = st.count(first, n, *shape)
    st.set(eng, cfg)
    st.reset(eng, first)
    assert st.count_of(eng, n) == no
    whole = st.run(eng, raw).copy()
    rows = whole if st.rows else whole[None]
    assert rows.shape == (K, no) and rows.dtype == np.complex64, _what(case, fmt)
    # (a) every link or channel against the float64 model
    for i in range(K):
        what = _what(case, fmt, " row %d" % i)
        if st.name == "pfb":
            y64, s = pfb_cases.model(x, taps, shape[0], case.sel[i], first)
            assert len(y64) == no
            sh._within(rows[i], y64, pfb_cases.bound(case.ntaps, shape[0], s), what)
        else:
            c = st.taps(eng, i) if st.rows else st.taps(eng)
            st.check_model(rows[i], x, c, shape, case.sel[i] if st.rows else case.sel, first, what)
    # (b) the case's chunking: the same bits, every count the model's
    st.reset(eng, first)
    parts, a = [], 0
    for s in case.chunks:
        want = st.count(first + a, s, *shape)
        assert st.count_of(eng, s) == want, _what(case, fmt)
        y = st.run(eng, raw[a:a + s])
        assert y.shape == ((K, want) if st.rows else (want,)), _what(case, fmt)
        parts.append(y.copy())
        a += s
    assert np.array_equal(sh.bits(np.concatenate(parts, axis=-1)), sh.bits(whole)), _what(case, fmt, " chunked")
    # (c) every link of a bank is the single stage on the same handle
    if st.single:
        one = sh.STAGES[st.single]
        for fc in sorted(set(case.sel)):
            one.set(eng, one.cfg(*shape, fc, taps=taps))
            one.reset(eng, first)
            y1 = one.run(eng, raw)
            for i in [i for i, f in enumerate(case.sel) if f == fc]:
                assert np.array_equal(sh.bits(rows[i]), sh.bits(y1)), _what(case, fmt, " link %d against the single stage" % i)
        one.set(eng, None)
    # (e), (f) device pointers: the host-mode bits and nothing behind a row's outputs
    st.set(dev, cfg)
    for off in ((0, 1) if fmt == "fc32" else (0,)):
        if fmt == "fc32":
            buf, ptr = _device_input(torch, raw, off)
        else:
            buf = torch.from_numpy(np.ascontiguousarray(raw)).cuda()
            ptr = buf.data_ptr()
        y = torch.full((K, no + PAD), complex(sh.SENTINEL), dtype=torch.complex64, device="cuda")
        torch.cuda.synchronize()
        st.reset(dev, first)
        got = st.device(dev, ptr, n, y.data_ptr(), no + PAD, no) if st.rows else st.device(dev, ptr, n, y.data_ptr(), no)
        torch.cuda.synchronize()
        out = y.cpu().numpy()
        assert got == no and np.array_equal(sh.bits(out[:, :no]), sh.bits(rows)), _what(case, fmt, " device, offset %d" % off)
        assert np.all(out[:, no:] == sh.SENTINEL), _what(case, fmt, " device, offset %d: wrote behind the outputs" % off)
        sh.zero(torch, buf, y)


def _tx_case(torch, eng, dev, st, case, fmt):
    shape, first, n, K = case.shape, case.first, case.n, (len(case.sel) if st.rows else 1)
    x, taps = sw.tx_input(case), sw.taps_of(case)
    no = st.count(first, n, *shape)
    st.set(eng, sw.cfg_of(case, "fc32"))
    st.reset(eng, first)
    plain = st.run(eng, x).copy()
    assert plain.shape == (no,) and plain.dtype == np.complex64, _what(case, fmt)
    cfg = sw.cfg_of(case, fmt)
    if fmt == "sc16":
        st.set(eng, cfg)
        st.reset(eng, first)
        whole = st.run(eng, x).copy()
        assert np.array_equal(whole, iqio.to_sc16(plain)), _what(case, fmt, " the 16-bit store")
    else:
        whole = plain
    # (a) against the float64 model
    if st.rows:
        sh.check_tx_bank_model(whole, x, taps, st, shape, list(case.sel), first, fmt, _what(case, fmt))
    else:
        sh.check_tx_model(whole, x, taps, st, shape, case.sel, first, fmt, _what(case, fmt))
    # (b) the case's chunking: the same bits, every count the model's
    st.reset(eng, first)
    parts, a = [], 0
    for s in case.chunks:
        want = st.count(first + a, s, *shape)
        if st.has_count:
            assert st.count_of(eng, s) == want, _what(case, fmt)
        y = st.run(eng, x[..., a:a + s])
        assert len(y) == want, _what(case, fmt)
        parts.append(y.copy())
        a += s
    got = np.concatenate(parts)
    assert got.dtype == whole.dtype and np.array_equal(sh.bits(got), sh.bits(whole)), _what(case, fmt, " chunked")
    # (d) onto a band: one float32 addition per part, then the store
    add = sw.tx_add(case, no)
    st.reset(eng, first)
    got = st.run(eng, x, add=add)
    want = sh.part_sum(add, plain)
    assert np.array_equal(sh.bits(got), sh.bits(iqio.to_sc16(want) if fmt == "sc16" else want)), _what(case, fmt, " add")
    # (e), (f) device pointers, the rows one behind the other from an even and from an odd sample of the buffer
    st.set(dev, cfg)
    for off in (0, 1):
        buf, ptr = _device_input(torch, x.reshape(-1), off)
        if fmt == "sc16":
            y = torch.full((no + PAD, 2), FILL16, dtype=torch.int16, device="cuda")
        else:
            y = torch.full((no + PAD,), complex(sh.SENTINEL), dtype=torch.complex64, device="cuda")
        torch.cuda.synchronize()
        st.reset(dev, first)
        got = st.device(dev, ptr, n, n, y.data_ptr(), no) if st.rows else st.device(dev, ptr, n, y.data_ptr(), no)
        torch.cuda.synchronize()
        out = y.cpu().numpy()
        assert got == no and np.array_equal(sh.bits(out[:no]), sh.bits(whole)), _what(case, fmt, " device, offset %d" % off)
        assert np.all(out[no:] == (FILL16 if fmt == "sc16" else sh.SENTINEL)), \
            _what(case, fmt, " device, offset %d: wrote behind the outputs" % off)
        sh.zero(torch, buf, y)


@pytest.mark.parametrize("stage,fmt", PARAMS)
def test_sweep(eng, dev, stage, fmt):
    import torch
    st = sh.STAGES[stage]
    t0 = time.time()
    rx = st.side == "rx"
    try:
        if rx:
            eng.set_rx_iq_format(fmt)
            dev.set_rx_iq_format(fmt)
        for case in sw.cases(stage):
            (_rx_case if rx else _tx_case)(torch, eng, dev, st, case, fmt)
    finally:
        for e in (eng, dev):
            e.set_rx_iq_format("fc32")
            st.set(e, None)
        torch.cuda.empty_cache()
    print("%s %s: %d cases in %.2f s" % (stage, fmt, len(sw.cases(stage)), time.time() - t0))
