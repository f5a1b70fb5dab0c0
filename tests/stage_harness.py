"""What the tests of the ten wideband stream stages share: one descriptor per stage (STAGES) and the checks that the
per-stage files (test_gpu_<stage>.py, test_<stage>_host.py) call with their own seeds, shapes and expectations.  A
descriptor holds what differs between sibling stages as data -- the method prefix, the side, the row layout, the cfg
builder, the restated arithmetic of the *_cases modules, the C argument order, the index limit, the refusal data.
Each stage's float64 model, emulation and error bound stay in its own *_cases module."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ddc_bank_cases
import ddc_cases
import duc_bank_cases
import duc_cases
import pfb_cases
import pfb_synth_cases
import resamp_bank_cases
import resamp_cases
import tx_resamp_bank_cases
import tx_resamp_cases
from helpers import make_cfg, make_payloads
from ofdm_uhd_amd import (_abi, benchmark_ofdm_rx, benchmark_ofdm_tx, ddc, duc, engine, iqio, ofdm, options, pfb,
                          receive_path, resample, transmit_path, tx_resample)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -24
SCALE = 32768.0
AMP = 1.0 / 16.0            # keeps every band of the transmit banks' tests inside the 16-bit range
START = 1000003             # a first input index that is a multiple of no tile
FAR = (1 << 40) - 5         # ... and one near 2^40
FCS = (0.0, 0.25, -1.0 / 3.0 + 0.013, 0.5)
SENTINEL = np.complex64(-7.5 + 3.25j)


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(cfg=make_cfg())
    yield e
    e.close()


class Stage(object):
    """One stream stage.  ``name`` is the method prefix (set_<name>, <name>, <name>_reset, <name>_count, <name>_taps,
    <name>_last_ms, <name>_device, <name>_cfg); a shape is (R,), (L,), (M,) or (L, M); ``sel`` is what follows it in the
    cfg builder: a centre frequency, a list of them or a list of channels."""
    has_count = has_taps = True         # whether the engine has <name>_count and <name>_taps
    rows = single = cases = None        # "in" / "out" for a bank; the bank's single stage; its *_cases module
    phase_free = False                  # the output does not depend on the stream's first index
    refusal_messages = None             # distinct refusal messages its test counts
    sel_field = beyond = None           # the cfg's array of frequencies or channels; a value refused inside the count
    refused_fields = refused_sel = ()   # refused field settings; refused values of sel_field

    def __getattr__(self, field):       # (only reached for a field that neither the stage nor the class has)
        raise AttributeError("stage %r has no %r: this check is not for it" % (self.__dict__.get("name"), field))

    def __init__(self, name, **fields):
        self.name = name
        self.__dict__.update(fields)

    def set(self, e, cfg):
        getattr(e, "set_" + self.name)(cfg)

    def run(self, e, x, **kw):
        return getattr(e, self.name)(x, **kw)

    def reset(self, e, first):
        getattr(e, self.name + "_reset")(first)

    def count_of(self, e, n):
        return getattr(e, self.name + "_count")(n)

    def taps(self, e, *link):
        return getattr(e, self.name + "_taps")(*link)

    def last_ms(self, e):
        return getattr(e, self.name + "_last_ms")()

    def device(self, e, *args, **kw):
        return getattr(e, self.name + "_device")(*args, **kw)

    def cfg_of(self, e):
        return getattr(e, self.name + "_cfg")

    def c_fn(self, suffix=""):
        return getattr(_abi.load(), "ofdm_" + ("set_" + self.name if suffix == "set" else self.name + suffix))

    def raw(self, h, x, out, stride, cap, nin=None, add=None):
        """The stage's call itself through ctypes, (return code, *nout).  Receive banks take (h, in, nin, out, stride,
        cap, &nout), transmit banks (h, in, stride, nin, add, out, cap, &nout)."""
        nn = C.c_uint64(0)
        xp, op = x.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
        if self.side == "rx":
            rc = self.c_fn()(h, xp, len(x) if nin is None else nin, op, stride, cap, C.byref(nn))
        else:
            rc = self.c_fn()(h, xp, stride, nin, None if add is None else add.ctypes.data_as(C.c_void_p), op, cap, C.byref(nn))
        return rc, nn.value


def _ddc_chunk_sizes(rng, n, ntaps, R):
    tile = ddc_cases.tile_outputs(R) * R
    sizes = [s for s in (1, R - 1, R, ntaps - 2, ntaps, 997, tile - 1, tile + 1) if s >= 1]
    out, left = [], n
    seq = list(sizes)                       # every size once, then random draws (small ones weighted down)
    while left > 0:
        s = seq.pop(0) if seq else int(rng.choice(sizes, p=np.array([1.0 if v < 16 else 4.0 for v in sizes]) /
                                                  sum(1.0 if v < 16 else 4.0 for v in sizes)))
        s = min(s, left)
        out.append(s)
        left -= s
    assert any(s < ntaps - 1 for s in out) or ntaps <= 2
    return out


def _resamp_chunk_sizes(rng, n, ntaps, L, M):
    tile, Q = resamp_cases.tile_inputs(L, M), (ntaps - 1) // L
    sizes = [s for s in (1, M - 1, M, Q - 1, Q + 1, 997, tile - 1, tile + 1) if s >= 1]
    weights = np.array([1.0 if v < 16 else 4.0 for v in sizes])
    out, left = [], n
    seq = list(sizes)                       # every size once, then random draws (small ones weighted down)
    while left > 0:
        s = min(seq.pop(0) if seq else int(rng.choice(sizes, p=weights / weights.sum())), left)
        out.append(s)
        left -= s
    if M > L:
        # one call that produces nothing for certain: cut the first longer chunk where a single sample completes no
        # output (between two outputs the input index advances by M / L > 1)
        k = next(i for i, s in enumerate(out) if s > 2 * M)
        at = sum(out[:k])
        lone = next(j for j in range(1, M + 1) if resamp_cases.count(at + j, 1, L, M) == 0)
        out[k:k + 1] = [lone, 1, out[k] - lone - 1]
    assert sum(out) == n and min(out) >= 1
    return out


def check_ddc_model(y, x, c, shape, fc, first, what):
    """The derived bound: |y - y64| <= (ntaps + 16) 2^-24 sum_k |c[k]| |x[mR - k]| per output -- a
    float32 sum of ntaps products in any order, 16 more roundings for the complex products and the rotation."""
    R, = shape
    y64, s = ddc_cases.model(x, c, R, ddc_cases.phase_step(fc, R), first)
    assert len(y) == len(y64) == ddc_cases.count(first, len(x), R), what
    _within(y, y64, (len(c) + 16) * EPS * s, what)


def check_resamp_model(y, x, c, shape, fc, first, what):
    """The derived bound: |y - y64| <= (ceil(ntaps / L) + 16) 2^-24 sum |c| |x| per output -- a
    float32 sum of at most ceil(ntaps / L) products in any order, 16 more roundings for the complex products and the
    rotation."""
    L, M = shape
    y64, s = resamp_cases.model(x, c, L, M, resamp_cases.phase_step(fc, L, M), first)
    assert len(y) == len(y64) == resamp_cases.count(first, len(x), L, M), what
    _within(y, y64, (-(-len(c) // L) + 16) * EPS * s, what)


def _within(y, y64, bound, what):
    err = np.abs(y.astype(np.complex128) - y64)
    worst = float(np.max(err / np.maximum(bound, 1e-300))) if len(y) else 0.0
    print("%s: %d outputs, worst error / bound = %.3g" % (what, len(y), worst))
    assert np.all(err <= bound), what


# refused field settings of a transmit stage's 16-bit output, and what every bank refuses
_OUT_BAD = (dict(out_format=2), dict(out_format=1, out_scale=-1.0), dict(out_format=1, out_scale=float("inf")))
_LINKS_BAD = (dict(ntaps=0), dict(ntaps=1025), dict(nlinks=0), dict(nlinks=9))
_CHAN_BAD = (dict(struct_size=12), dict(nchannels=0), dict(nchannels=1), dict(nchannels=3), dict(nchannels=128), dict(ntaps=0),
             dict(ntaps=1025), dict(nsel=0), dict(nsel=5))
_R_BAD = (dict(struct_size=12), dict(decimation=0), dict(decimation=65))
_L_BAD = (dict(struct_size=12), dict(interpolation=0), dict(interpolation=65))
_LM_BAD = _L_BAD + (dict(decimation=0), dict(decimation=65))

STAGES = {s.name: s for s in (
    Stage("ddc", side="rx", rows=None, cfg=ddc.ddc_cfg, count=ddc_cases.count,
          tile_inputs=lambda R, K=1: ddc_cases.tile_outputs(R) * R, chunk_sizes=_ddc_chunk_sizes, check_model=check_ddc_model,
          index_limit=lambda R: 1 << 62, every_call_has_outputs=lambda R: R == 1, kernel_word="ddc"),
    Stage("ddc_bank", side="rx", rows="out", cfg=ddc.bank_cfg, count=ddc_cases.count, single="ddc", cases=ddc_bank_cases,
          tile_inputs=lambda R, K=1: ddc_bank_cases.tile_outputs(R, K) * R, chunk_sizes=_ddc_chunk_sizes,
          check_model=check_ddc_model, index_limit=lambda R: 1 << 62, every_call_has_outputs=lambda R: R == 1,
          sel_field="center_freq", beyond=3.0, refused_fields=_R_BAD + _LINKS_BAD, refused_sel=(0.5000001, -0.51, float("nan")),
          kernel_word="ddc"),
    Stage("resamp", side="rx", rows=None, cfg=resample.resamp_cfg, count=resamp_cases.count,
          tile_inputs=lambda L, M, K=1: resamp_cases.tile_inputs(L, M), chunk_sizes=_resamp_chunk_sizes,
          check_model=check_resamp_model, index_limit=lambda L, M: 1 << 56, every_call_has_outputs=lambda L, M: M <= L,
          kernel_word="resamp"),
    Stage("resamp_bank", side="rx", rows="out", cfg=resample.bank_cfg, count=resamp_cases.count, single="resamp",
          cases=resamp_bank_cases, tile_inputs=resamp_bank_cases.tile_inputs, chunk_sizes=_resamp_chunk_sizes,
          check_model=check_resamp_model, index_limit=lambda L, M: 1 << 56, every_call_has_outputs=lambda L, M: M <= L,
          sel_field="center_freq", beyond=3.0, refused_fields=_LM_BAD + _LINKS_BAD,
          refused_sel=(0.5000001, -0.51, float("nan")), kernel_word="resamp"),
    Stage("pfb", side="rx", rows="out", cfg=pfb.pfb_cfg, count=pfb_cases.count, cases=pfb_cases,
          tile_inputs=lambda M: pfb_cases.tile_outputs(M) * M, index_limit=lambda M: 1 << 62, has_taps=False,
          sel_field="channel", beyond=200, refused_fields=_CHAN_BAD, refused_sel=(4,), kernel_word="pfb"),
    Stage("pfb_synth", side="tx", rows="in", cfg=pfb.synth_cfg, count=lambda first, n, M: n * M, single="duc",
          cases=pfb_synth_cases, tile_inputs=pfb_synth_cases.tile_inputs, history=pfb_synth_cases.history,
          index_limit=lambda M: (1 << 63) // M, has_count=False, has_taps=False, phase_free=True, sel_field="channel",
          beyond=200, refused_fields=_CHAN_BAD + _OUT_BAD, refused_sel=(4, 1), refusal_messages=None, kernel_word="pfb"),
    Stage("duc", side="tx", rows=None, cfg=duc.duc_cfg, count=lambda first, n, L: n * L, cases=duc_cases,
          tile_inputs=lambda L: duc_cases.tile_outputs(L) // L, history=duc_cases.history,
          index_limit=lambda L: (1 << 63) // L, has_count=False, kernel_word="duc"),
    Stage("duc_bank", side="tx", rows="in", cfg=duc.bank_cfg, count=lambda first, n, L: n * L, single="duc",
          cases=duc_bank_cases, tile_inputs=lambda L: max(duc_bank_cases.tile_outputs(L) // L, 1),
          history=duc_bank_cases.history, index_limit=lambda L: (1 << 63) // L, has_count=False, has_taps=True,
          phase_free=False, sel_field="center_freq", beyond=7.0, refused_fields=_L_BAD + _LINKS_BAD + _OUT_BAD,
          refused_sel=(0.5000001, -0.51, float("nan"), float("inf")), refusal_messages=None, kernel_word="duc"),
    Stage("tx_resamp", side="tx", rows=None, cfg=tx_resample.tx_resamp_cfg, count=tx_resamp_cases.count,
          cases=tx_resamp_cases, tile_inputs=tx_resamp_cases.tile_inputs, history=lambda ntaps, L, M: (ntaps - 1) // L,
          index_limit=lambda L, M: 1 << 56, has_count=True, kernel_word="resamp"),
    Stage("tx_resamp_bank", side="tx", rows="in", cfg=tx_resample.bank_cfg, count=tx_resamp_cases.count,
          single="tx_resamp", cases=tx_resamp_bank_cases, tile_inputs=tx_resamp_bank_cases.tile_inputs,
          history=lambda ntaps, L, M: (ntaps - 1) // L, index_limit=lambda L, M: 1 << 56, has_count=True, has_taps=True,
          phase_free=False, sel_field="center_freq", beyond=7.0, refused_fields=_LM_BAD + _LINKS_BAD + _OUT_BAD,
          refused_sel=(0.5000001, -0.51, float("nan"), float("inf")),
          refusal_messages=9,     # struct_size, L, M, ntaps, nlinks, format, scale, frequency, taps: one each
          kernel_word="resamp"),
)}


# ---- small helpers ----------------------------------------------------------------------------------------------------

def rx_stream(rng, n, fmt):
    """(samples in the receive format, the same samples converted to complex64)"""
    if fmt == "sc16":
        q = rng.integers(-32768, 32768, (n, 2)).astype(np.int16)
        return q, iqio.from_sc16(q)
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    return x, x


def tx_stream(rng, n, amp=1.0):
    return (amp * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)


def rows(rng, K, n, amp=AMP):
    return (amp * (rng.standard_normal((K, n)) + 1j * rng.standard_normal((K, n)))).astype(np.complex64)


def bits(a):
    """The stored bits: -0 and +0 differ (int16 samples compare as they are)."""
    return a.view(np.uint32) if a.dtype == np.complex64 else a


def c64(out, fmt):
    """The stage's output as complex128 samples."""
    return (iqio.from_sc16(out) if fmt == "sc16" else out).astype(np.complex128)


def as_complex(y, fmt):
    """The stored samples as float64 complex numbers, in units of the float output (int16 / full scale)."""
    if fmt == "sc16":
        assert y.dtype == np.int16 and y.ndim == 2 and y.shape[1] == 2
        return (y[:, 0].astype(np.float64) + 1j * y[:, 1].astype(np.float64)) / SCALE
    assert y.dtype == np.complex64
    return y.astype(np.complex128)


def part_sum(a, b):
    """a + b formed in float32 part by part."""
    a, b = np.asarray(a, np.complex64), np.asarray(b, np.complex64)
    out = np.empty(len(a), np.complex64)
    out.real = a.real + b.real
    out.imag = a.imag + b.imag
    return out


def zero(torch, *tensors):
    """Zero the test's device buffers before they are released: a later test's torch.empty() must not inherit this
    file's bytes."""
    for t in tensors:
        t.zero_()
    torch.cuda.synchronize()


def release(torch, *tensors):
    """Hand the test's device buffers back zeroed and drop torch's cache."""
    zero(torch, *tensors)
    del tensors
    torch.cuda.empty_cache()


def options_of(k):
    return options.default_options(modulation=k["mod"], fft_length=k["N"], occupied_tones=k["occ"], cp_length=k["CP"])


def engine_tx(e):
    def tx(cfg, payloads, lead, tail):
        e.set_channel(sigma=0.0, lead=lead, tail=tail)
        try:
            return e.tx(payloads)
        finally:
            e.set_channel(enable=False)
    return tx


def wide_sc16(wide):
    """The capture as 16-bit IQ with its peak at half scale; nothing may saturate."""
    peak = float(max(np.max(np.abs(wide.real)), np.max(np.abs(wide.imag))))
    q = iqio.to_sc16(wide * np.float32(0.5 / peak))
    assert int(np.max(np.abs(q.astype(np.int32)))) < 32767, "a sample saturated"
    return q


def with_noise_floor(wide, ratio, lead, tail, seed=5):
    """Silence around the stream and a noise floor 30 dB below the link inside its band, which is 1 / ratio of the
    wideband one (the receiver's metric is 0/0 on exact zeros)."""
    rng = np.random.default_rng(seed)
    x = np.concatenate([np.zeros(lead, np.complex64), wide, np.zeros(tail, np.complex64)])
    sigma = np.sqrt(float(np.mean(np.abs(wide) ** 2)) * ratio / 1e3)
    return (x + sigma * np.sqrt(0.5) * (rng.standard_normal(len(x)) + 1j * rng.standard_normal(len(x)))).astype(np.complex64)


def raw_cfg(base, **kw):
    """A fresh configuration from ``base()`` with fields overwritten as they are (no builder checks them)."""
    c = base()
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def record(d, name):
    """Keeps what the demodulator's front end (Engine.<name>) hands to the receiver."""
    e, rec = d.engine(), []
    orig = getattr(e, name)

    def run_and_keep(iq):
        y = orig(iq)
        rec.append(y.copy())
        return y
    setattr(e, name, run_and_keep)
    return rec


def launches(e):
    return {k: v[1] for k, v in e.prof().items()}


def write_capture(path, wide):
    sink = iqio.file_sink(path)
    sink.write(wide)
    sink.close()


# ---- every stage ------------------------------------------------------------------------------------------------------

def check_interleaved(stages, off):
    """``stages``: name -> (configure, run(a, b), total, step).  Each stage alone, then all configured on the one handle
    with their calls interleaved, each in its own chunking: every stage gives the bits of its uninterrupted run.
    Returns the uninterrupted outputs; every stage is left configured."""
    alone = {}
    for name, (cfg, run, total, _) in stages.items():
        cfg()
        alone[name] = run(0, total).copy()
        off[name](None)
    for cfg, _, _, _ in stages.values():
        cfg()
    parts = {name: [] for name in stages}
    pos = {name: 0 for name in stages}
    while any(pos[name] < stages[name][2] for name in stages):
        for name, (_, run, total, step) in stages.items():
            if pos[name] < total:
                parts[name].append(run(pos[name], min(pos[name] + step, total)).copy())
                pos[name] += step
    for name in stages:
        assert np.array_equal(np.concatenate(parts[name], axis=-1), alone[name]), name
    return alone


# ---- receive stages ---------------------------------------------------------------------------------------------------

def check_rx_segmentation(eng, st, shape, ntaps, K, fmt, seed, n):
    """The stream in one call (checked against the float64 model) and in chunks of every critical size: the same bits,
    calls without outputs included; and again from a start that is no multiple of the period."""
    rng = np.random.default_rng(seed)
    fc = -1.0 / 3.0 + 0.013
    if st.rows:
        sel = [float(f) for f in rng.uniform(-0.5, 0.5, K)]
        sel[0] = fc
        link, row_shape, axis = (K - 1,), lambda no: (K, no), 1
    else:
        sel, link, row_shape, axis = fc, (), lambda no: (no,), 0
    eng.set_rx_iq_format(fmt)
    try:
        raw, x = rx_stream(rng, n, fmt)
        taps = ddc_bank_cases.taps_for(rng, ntaps)
        st.set(eng, st.cfg(*shape, sel, taps=taps))
        c = st.taps(eng, *link)
        assert c.dtype == np.complex64 and len(c) == len(taps)
        whole = st.run(eng, raw).copy()
        assert whole.shape == row_shape(st.count(0, n, *shape))
        st.check_model(whole[link], x, c, shape, sel[K - 1] if st.rows else fc, 0,
                       "whole %s ntaps=%d K=%s %s" % (shape, ntaps, K, fmt))
        st.reset(eng, 0)
        sizes = st.chunk_sizes(rng, n, ntaps, *shape)
        parts, a, empty = [], 0, 0
        for s in sizes:
            want = st.count(a, s, *shape)
            assert st.count_of(eng, s) == want
            y = st.run(eng, raw[a:a + s])
            assert y.shape == row_shape(want)
            empty += want == 0
            parts.append(y.copy())
            a += s
        assert empty >= 1 or st.every_call_has_outputs(*shape)        # calls that produce nothing are part of the stream
        assert np.array_equal(np.concatenate(parts, axis=axis), whole)
        # ... and from a start that is no multiple of the period (R or M)
        first = 7 * shape[-1] + 1
        st.reset(eng, first)
        w2 = st.run(eng, raw).copy()
        assert w2.shape == row_shape(st.count(first, n, *shape))
        st.reset(eng, first)
        p2 = [st.run(eng, raw[i:i + 997]).copy() for i in range(0, n, 997)]
        assert np.array_equal(np.concatenate(p2, axis=axis), w2)
    finally:
        eng.set_rx_iq_format("fc32")
        st.set(eng, None)


def check_capacity_error_leaves_the_stream_state(eng, st, shape, fc, taps, x):
    """A single stage's call with room for one output too few: OFDM_E_CAPACITY with *nout set, and the retried call
    continues the stream bit for bit."""
    st.set(eng, st.cfg(*shape, fc, taps=taps))
    try:
        want = st.run(eng, x).copy()
        st.reset(eng, 0)
        first = st.run(eng, x[:1001])
        need = st.count(1001, 3999, *shape)
        if st.has_count:
            assert st.count_of(eng, 3999) == need
        out = np.zeros(need, np.complex64)
        n = C.c_uint64(0)
        xp, op = x[1001:].ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
        if st.side == "rx":
            rc = st.c_fn()(eng._h, xp, 3999, op, need - 1, C.byref(n))
        else:
            rc = st.c_fn()(eng._h, xp, 3999, None, op, need - 1, C.byref(n))
        assert rc == _abi.OFDM_E_CAPACITY and n.value == need
        if st.has_count:
            assert st.count_of(eng, 3999) == need
        rest = st.run(eng, x[1001:])
        assert np.array_equal(np.concatenate([first, rest]), want)
    finally:
        st.set(eng, None)


def check_phase_step_zero_and_index_limit(eng, st, sel, link):
    """The DDC family at R = 4: fc R a hair below a whole turn from the negative side (frac rounds up to 1 and the phase
    step is 0, not 2^64) in ``sel``, read at ``link`` (() for the single stage); stream indices are refused before 64-bit
    arithmetic could wrap."""
    rng = np.random.default_rng(9)
    raw, x = rx_stream(rng, 700, "fc32")
    taps = (rng.standard_normal(9) / 3).astype(np.float32)
    lim = st.index_limit(4)
    try:
        st.set(eng, st.cfg(4, sel, taps=taps))
        c = st.taps(eng, *link)
        assert c.dtype == np.complex64 and len(c) == len(taps)
        assert ddc_cases.phase_step(-1e-20, 4) == 0
        st.reset(eng, 1000003)
        check_ddc_model(st.run(eng, raw)[link], x, c, (4,), -1e-20, 1000003, "fc=-1e-20")
        st.reset(eng, lim)
        assert st.count_of(eng, 8) == 2
        with pytest.raises(ValueError):
            st.reset(eng, lim + 1)
        assert st.count_of(eng, 8) == 2                   # the refused reset left the stream where it was
    finally:
        st.set(eng, None)


def check_rx_layout_and_capacity(eng, st, shape, sel, taps, one_sel):
    """A receive bank's output layout: a stride beyond nout leaves the gaps alone, a capacity one short or a stride
    below nout is refused and moves nothing, one row ignores the stride.  ``one_sel`` selects what row 1 of ``sel``
    holds."""
    rng = np.random.default_rng(5)
    raw, _ = rx_stream(rng, 5000, "fc32")
    st.set(eng, st.cfg(*shape, sel, taps=taps))
    try:
        want = st.run(eng, raw).copy()
        no = want.shape[1]
        assert no == st.count(0, 5000, *shape)
        # stride > nout: the gaps keep what they held
        st.reset(eng, 0)
        out = np.full((3, no + 13), SENTINEL, np.complex64)
        assert st.raw(eng._h, raw, out, no + 13, no) == (_abi.OFDM_OK, no)
        assert np.array_equal(out[:, :no], want) and np.all(out[:, no:] == SENTINEL)
        # out_cap one short: refused with *nout set, and the stream does not move
        st.reset(eng, 0)
        first = st.run(eng, raw[:1001]).copy()
        need = st.count_of(eng, 3999)
        out = np.full((3, need), SENTINEL, np.complex64)
        rest_in = np.ascontiguousarray(raw[1001:])
        assert st.raw(eng._h, rest_in, out, need, need - 1) == (_abi.OFDM_E_CAPACITY, need)
        assert np.all(out == SENTINEL) and st.count_of(eng, 3999) == need
        # stride < nout with more than one row
        assert st.raw(eng._h, rest_in, out, need - 1, need) == (_abi.OFDM_E_INVAL, need)
        assert st.count_of(eng, 3999) == need
        # the retried call gives the bits of an uninterrupted run
        rest = st.run(eng, rest_in)
        assert np.array_equal(np.concatenate([first, rest], axis=1), want)
        # one row: the stride does not matter
        st.set(eng, st.cfg(*shape, one_sel, taps=taps))
        out = np.zeros(no, np.complex64)
        assert st.raw(eng._h, raw, out, 0, no) == (_abi.OFDM_OK, no)
        assert np.array_equal(out, want[1])
    finally:
        st.set(eng, None)


def _misaligned_sc16_input_is_refused(eng, st, out, at, count64, more_args):
    """A 16-bit input pointer that is not 4-byte aligned, with the stream ``at`` samples in: refused, nothing moves
    (64 more inputs still give ``count64`` outputs); the configuration is dropped afterwards."""
    eng.set_rx_iq_format("sc16")
    try:
        q = np.zeros(2 * 64 + 2, np.int16)
        nn = C.c_uint64(0)
        if at:
            st.run(eng, q[:2 * at].reshape(at, 2))
        rc = st.c_fn()(eng._h, C.c_void_p(q.ctypes.data + 2), 64, out.ctypes.data_as(C.c_void_p), 64, *(more_args + (C.byref(nn),)))
        assert rc == _abi.OFDM_E_INVAL
        assert st.count_of(eng, 64) == count64                           # ... and the stream did not move
    finally:
        eng.set_rx_iq_format("fc32")
        st.set(eng, None)


def check_rx_single_invalid_arguments(eng, st, shape, base, bads, fed_sc16, count64):
    """A single receive stage: no configuration; every refused configuration (``bads``, a NaN and an infinite tap) with
    none in force and with one in force, which stays in force, stream state included; the ends of the frequency range;
    a misaligned 16-bit pointer ``fed_sc16`` samples into the stream, where 64 inputs give ``count64`` outputs."""
    st.set(eng, None)
    x = np.zeros(64, np.complex64)
    out = np.zeros(64, np.complex64)

    def raw():
        """the stage's call itself (Engine.<stage> asks the count first, which refuses on its own)"""
        n = C.c_uint64(0)
        return st.c_fn()(eng._h, x.ctypes.data_as(C.c_void_p), 64, out.ctypes.data_as(C.c_void_p), 64, C.byref(n))

    assert raw() == _abi.OFDM_E_INVAL                # no configuration
    for call in (lambda: st.run(eng, x), lambda: st.reset(eng, 0), lambda: st.count_of(eng, 8), lambda: st.taps(eng)):
        with pytest.raises(ValueError):
            call()
    st.set(eng, raw_cfg(base))
    assert raw() == _abi.OFDM_OK
    st.set(eng, None)
    assert raw() == _abi.OFDM_E_INVAL                # ... and after a configuration was dropped
    for bad in bads:
        with pytest.raises(ValueError):
            st.set(eng, raw_cfg(base, **bad))
    for v in (float("nan"), float("inf")):
        c = raw_cfg(base)
        c.taps[3] = v
        with pytest.raises(ValueError):
            st.set(eng, c)
    assert raw() == _abi.OFDM_E_INVAL                # a refused configuration changes nothing: still none in force
    # ... and with one in force it stays in force, stream state included
    st.set(eng, raw_cfg(base))
    st.run(eng, x[:7])
    table = st.taps(eng)
    for bad in bads:
        with pytest.raises(ValueError):
            st.set(eng, raw_cfg(base, **bad))
    assert np.array_equal(st.taps(eng), table) and st.count_of(eng, 64) == st.count(7, 64, *shape)
    st.set(eng, raw_cfg(base, center_freq=0.5))      # the ends of the range are inside it
    st.set(eng, raw_cfg(base, center_freq=-0.5))
    _misaligned_sc16_input_is_refused(eng, st, out, fed_sc16, count64, ())


def check_rx_bank_invalid_arguments(eng, st, shape, base, x, nout, after62, still_refused, edge_sel, middle=None):
    """A receive bank fed ``x`` (64 inputs give ``nout`` outputs per row; 62 inputs in, 2 and 3 more give ``after62``):
    no configuration; every refused configuration (the descriptor's refused_fields,
    refused_sel in slot 1 of its sel_field, a NaN and an infinite tap) through Engine and through the raw ABI, none
    touching the one in force (``still_refused`` indexes the one tried again in mid-stream); rows that do not exist;
    ``middle(lib, x, out)`` for what only this stage has; ``edge_sel`` (or None), a selection at the ends of its range;
    a misaligned 16-bit pointer."""
    lib = _abi.load()
    st.set(eng, None)
    out = np.zeros((2, 64), np.complex64)
    k = C.c_int(0)
    no = nout
    assert no == st.count(0, 64, *shape)
    assert st.raw(eng._h, x, out, 64, 64)[0] == _abi.OFDM_E_INVAL          # no configuration
    calls = [lambda: st.run(eng, x), lambda: st.reset(eng, 0), lambda: st.count_of(eng, 4), lambda: st.last_ms(eng)]
    if st.has_taps:
        calls.append(lambda: st.taps(eng, 0))
    for call in calls:
        with pytest.raises(ValueError):
            call()
    good = raw_cfg(base)
    st.set(eng, good)
    table = st.taps(eng, 1) if st.has_taps else None
    assert st.raw(eng._h, x, out, 64, 64) == (_abi.OFDM_OK, no)
    y = out[:, :no].copy()
    bad_sel = []
    for v in st.refused_sel:
        c = raw_cfg(base)
        getattr(c, st.sel_field)[1] = v
        bad_sel.append(c)
    bad_tap = []
    for v in (float("nan"), float("inf")):
        c = raw_cfg(base)
        c.taps[3] = v
        bad_tap.append(c)
    refused = [raw_cfg(base, **b) for b in st.refused_fields] + bad_sel + bad_tap
    for c in refused:
        with pytest.raises(ValueError):
            st.set(eng, c)
        assert st.cfg_of(eng) is good
    # the same through the raw ABI, and an entry beyond the count of rows is not looked at
    for c in refused:
        assert st.c_fn("set")(eng._h, C.byref(c)) == _abi.OFDM_E_INVAL
    c = raw_cfg(base)
    getattr(c, st.sel_field)[2] = st.beyond
    st.set(eng, c)
    st.set(eng, good)
    for c in refused[:3]:
        with pytest.raises(ValueError):
            st.set(eng, c)
    # ... a refused configuration left the one in force untouched: same table, same stream position, same outputs
    if st.has_taps:
        assert np.array_equal(st.taps(eng, 1), table)
    st.run(eng, x[:62])
    with pytest.raises(ValueError):
        st.set(eng, refused[still_refused])
    assert st.count_of(eng, 2) == after62[0] == st.count(62, 2, *shape)     # still 62 samples into the stream
    assert st.count_of(eng, 3) == after62[1] == st.count(62, 3, *shape) == 1
    st.reset(eng, 0)
    assert np.array_equal(st.run(eng, x), y)
    if st.has_taps:
        # link >= nlinks
        for link in (2, 8, -1):
            assert st.c_fn("_taps")(eng._h, link, None, 0, C.byref(k)) == _abi.OFDM_E_INVAL
        assert st.c_fn("_taps")(eng._h, 1, None, 0, C.byref(k)) == _abi.OFDM_OK and k.value == 5
    if middle is not None:
        middle(lib, x, out)
    if edge_sel is not None:
        # the ends of the range are inside it
        st.set(eng, st.cfg(*shape, edge_sel, taps=np.ones(5, np.float32)))
    _misaligned_sc16_input_is_refused(eng, st, out, 0, no, (64,))
    assert st.raw(eng._h, x, out, 64, 64)[0] == _abi.OFDM_E_INVAL          # ... and after it was dropped


def singles(eng, st, shape, taps, fcs, raw, first):
    """What the single stage gives for each frequency on the same handle: (outputs, tables)."""
    ys, cs = [], []
    for fc in fcs:
        st.set(eng, st.cfg(*shape, fc, taps=taps))
        if first:
            st.reset(eng, first)
        ys.append(st.run(eng, raw).copy())
        cs.append(st.taps(eng))
    st.set(eng, None)
    return ys, cs


def check_every_link_is_the_single_stage(eng, st, shape, fmt, seed, n, start):
    """Over the bank's tap grid, link counts and both starts: every link's output and table are the single stage's bit
    for bit; one link of the largest bank also against the float64 model."""
    one, bc = STAGES[st.single], st.cases
    rng = np.random.default_rng(seed)
    freqs = bc.frequencies(rng, FCS)
    assert 0.5 in freqs and 0.0 in freqs
    eng.set_rx_iq_format(fmt)
    try:
        raw, x = rx_stream(rng, n, fmt)
        for ntaps in bc.TAP_GRID[shape[0] if len(shape) == 1 else shape]:
            taps = bc.taps_for(rng, ntaps)
            for first in (0, start):
                no = st.count(first, n, *shape)
                want, tabs = singles(eng, one, shape, taps, freqs, raw, first)
                by_fc = dict(zip(freqs, zip(want, tabs)))
                for K in bc.LINK_COUNTS:
                    fcs = bc.pick(freqs, K)
                    st.set(eng, st.cfg(*shape, fcs, taps=taps))
                    if first:
                        st.reset(eng, first)
                    assert st.count_of(eng, n) == no
                    y = st.run(eng, raw)
                    assert y.shape == (K, no) and y.dtype == np.complex64
                    for i, fc in enumerate(fcs):
                        what = "%s ntaps=%d K=%d link %d fc=%g first=%d %s" % (shape, ntaps, K, i, fc, first, fmt)
                        assert np.array_equal(y[i], by_fc[fc][0]), what
                        assert np.array_equal(st.taps(eng, i), by_fc[fc][1]), what
                # one link of the largest bank against the float64 model: the file stands on its own
                i = 2 + (ntaps + (first > 0)) % 5
                st.check_model(y[i], x, st.taps(eng, i), shape, freqs[i], first,
                               "%s ntaps=%d K=8 link %d first=%d %s" % (shape, ntaps, i, first, fmt))
    finally:
        eng.set_rx_iq_format("fc32")
        st.set(eng, None)
        one.set(eng, None)


def check_link_order_and_count_do_not_matter(eng, st, shape, ntaps, seed):
    rng = np.random.default_rng(seed)
    n = st.tile_inputs(*shape, 8) + 1001
    raw, _ = rx_stream(rng, n, "fc32")
    taps = st.cases.taps_for(rng, ntaps)
    fcs = [float(f) for f in rng.uniform(-0.5, 0.5, 7)]
    try:
        st.set(eng, st.cfg(*shape, fcs, taps=taps))
        ref = st.run(eng, raw).copy()
        perm = [int(i) for i in rng.permutation(7)]
        assert perm != list(range(7))
        st.set(eng, st.cfg(*shape, [fcs[i] for i in perm], taps=taps))
        y = st.run(eng, raw)
        for j, i in enumerate(perm):
            assert np.array_equal(y[j], ref[i]), (j, i)
        for i in (0, 3, 6):                               # first of a group, last of a group, the odd one out
            st.set(eng, st.cfg(*shape, [fcs[i]], taps=taps))
            assert np.array_equal(st.run(eng, raw)[0], ref[i]), i
        # equal frequencies give equal outputs
        st.set(eng, st.cfg(*shape, [fcs[1]] * 5, taps=taps))
        y = st.run(eng, raw)
        for j in range(5):
            assert np.array_equal(y[j], ref[1])
    finally:
        st.set(eng, None)


def check_receiver_launches_what_it_launched(st, shape, cap, sel):
    """Two handles demodulate the same narrowband stream: one never saw the stage, the other used it on another stream
    and dropped it.  Same packets, same per-kernel launch counts; the kernel table has no entry for the stage.  With
    the stage configured again the receiver's own launches stay what they are, and the stage reports its time."""
    cfg = cap["cfg"]
    row = (lambda y: y[0]) if st.rows else (lambda y: y)
    a, b = engine.Engine(cfg=cfg), engine.Engine(cfg=cfg)
    try:
        st.set(b, st.cfg(*shape, sel, taps=cap["taps"]))
        y = row(st.run(b, cap["wide"])).copy()
        st.set(b, None)
        for e in (a, b):
            e.prof_enable(True)
            e.prof_reset()
        pa, pb = a.rx(y), b.rx(y)
        assert pa == pb and len(pa) == 4
        ca, cb = launches(a), launches(b)
        assert ca == cb and sum(ca.values()) > 0
        assert len(ca) == _abi.K_COUNT == 11 and not any(st.kernel_word in k for k in ca)
        st.set(b, st.cfg(*shape, sel, taps=cap["taps"]))
        b.prof_reset()
        with pytest.raises(ValueError):
            st.last_ms(b)                                 # no profiled call yet
        y2 = st.run(b, cap["wide"])
        assert np.array_equal(row(y2), y) and st.last_ms(b) > 0.0
        assert b.rx(row(y2)) == pa
        assert launches(b) == ca
    finally:
        a.close()
        b.close()


def check_a_stream_fed_after_work_starts_afresh(st, shape, cap, kw):
    """work() on a capture whose length is no multiple of the period and whose tail is loud, then feed() of another
    stream on the same demodulator: the front end's output and the packets are those of a fresh demodulator (no index,
    phase or filter history carried over).  ``kw`` is ofdm_demod's keyword for the front end."""
    wide = cap["wide"]
    rng = np.random.default_rng(3)
    loud = (30.0 * (rng.standard_normal(1000) + 1j * rng.standard_normal(1000))).astype(np.complex64)
    first = np.concatenate([wide[:len(wide) // 2], loud])
    while len(first) % shape[-1] == 0:
        first = first[:-1]

    def stream(d):
        rec = record(d, st.name)
        out = []
        for a in range(0, len(wide), 5000):
            out += d.feed(wide[a:a + 5000])
        out += d.flush()
        return np.concatenate(rec), out

    used, fresh = ofdm.ofdm_demod(options_of(cap), **kw), ofdm.ofdm_demod(options_of(cap), **kw)
    try:
        used.work(first)
        y_used, p_used = stream(used)
        y_fresh, p_fresh = stream(fresh)
        assert len(y_used) == len(y_fresh) == st.count(0, len(wide), *shape)
        assert np.array_equal(y_used, y_fresh)
        assert p_used == p_fresh and [p for ok, p in p_fresh if ok] == cap["payloads"][1]
        # and a second stream after a flush, and a work() after a stream
        y_again, p_again = stream(used)
        assert np.array_equal(y_again, y_fresh) and p_again == p_fresh
        used.feed(first[:7001])
        assert used.work(wide) == p_fresh
    finally:
        used.engine().close()
        fresh.engine().close()


def check_receive_path_and_command_line(cap, tmp_path, kw, set_options, flags, check_designed=None):
    """receive_path with the front end's keyword ``kw``; with the options' attributes as the command line sets them
    (``set_options(opt)``, tuned to the second link; ``check_designed(engine)`` looks at the designed taps);
    benchmark_ofdm_rx with ``flags`` on a wideband capture file, whole and in chunks, and without them."""
    sent = cap["payloads"][0]
    got = []
    rp = receive_path.receive_path(lambda ok, p: got.append((ok, p)), options_of(cap), **kw)
    try:
        assert rp.work(cap["wide"]) == got and [p for ok, p in got if ok] == sent
    finally:
        rp.ofdm_rx.engine().close()
    opt = options_of(cap)
    set_options(opt)
    rp = receive_path.receive_path(None, opt)
    try:
        if check_designed is not None:
            check_designed(rp.ofdm_rx.engine())
        assert [p for ok, p in rp.work(cap["wide"]) if ok] == cap["payloads"][1]
    finally:
        rp.ofdm_rx.engine().close()
    # benchmark_ofdm_rx on a wideband capture file, whole and in chunks
    f = str(tmp_path / "wide.dat")
    write_capture(f, cap["wide"])
    for extra in ([], ["--chunk-samples", "5000"]):
        acct = benchmark_ofdm_rx.main(["-m", "qpsk", "--from-file", f, "--to-file", str(tmp_path / "rx.txt")] + flags + extra)
        assert (acct.n_rcvd, acct.n_right) == (4, 4)
    # without the flags the wideband file is not a capture of this modem
    acct = benchmark_ofdm_rx.main(["-m", "qpsk", "--from-file", f, "--to-file", str(tmp_path / "rx.txt")])
    assert acct.n_right == 0


def check_links_that_differ_in_modulation_and_the_command_line(cap, tmp_path, make_bank, base, freq_flag, freqs_flag):
    """``make_bank(options)`` with a list of option sets, one per link: the second link demodulated as BPSK finds no
    good packet.  benchmark_ofdm_rx with ``base`` flags and the list flag gives one account and one file per link; list
    and single flag together are refused; the single flag alone gives one account, as before."""
    o_ok, o_other = options_of(cap), options_of(cap)
    o_other.modulation = "bpsk"
    bank = make_bank([o_ok, o_other])
    try:
        out = bank.work(cap["wide"])
        assert [p for ok, p in out[0] if ok] == cap["payloads"][0] and not any(ok for ok, _ in out[1])
    finally:
        bank.close()
    f = str(tmp_path / "wide.dat")
    write_capture(f, cap["wide"])
    to = str(tmp_path / "rx.txt")
    base = ["-m", "qpsk", "--from-file", f, "--to-file", to] + base
    for extra in ([], ["--chunk-samples", "5000"]):
        accts = benchmark_ofdm_rx.main(base + freqs_flag + extra)
        assert [(a.n_rcvd, a.n_right) for a in accts] == [(4, 4), (4, 4)]
        assert (tmp_path / "rx.txt.link0").exists() and (tmp_path / "rx.txt.link1").exists()
    with pytest.raises(SystemExit):
        benchmark_ofdm_rx.main(base + freq_flag[0] + freqs_flag)
    # without the new flag: one account, as before
    acct = benchmark_ofdm_rx.main(base + freq_flag[1])
    assert (acct.n_rcvd, acct.n_right) == (4, 4)


def check_rx_device_pointers(torch, st, host, devE, cfg, raw, K, fmt, clear_between=False):
    """A receive bank driven through device pointers: torch buffers, raw pointers, a row stride beyond nout; then the
    stream in two halves.  Returns (x, y, want, no, stride): the device input and output and the host's reference."""
    dev = torch.device("cuda", 0)
    n = len(raw)
    for e in (host, devE):
        e.set_rx_iq_format(fmt)
        st.set(e, cfg)
        e.prof_enable(True)
    with pytest.raises(ValueError):
        st.last_ms(devE)                                  # no profiled call yet
    want = st.run(host, raw)
    no = want.shape[1]
    stride = no + 3
    x = torch.from_numpy(np.array(raw)).to(dev)           # (a writable, contiguous copy)
    y = torch.full((K, stride), -2.0 + 1.0j, dtype=torch.complex64, device=dev)
    got = st.device(devE, x.data_ptr(), n, y.data_ptr(), stride, no)
    torch.cuda.synchronize()
    assert got == no
    out = y.cpu().numpy()
    assert np.array_equal(out[:, :no], want) and np.all(out[:, no:] == np.complex64(-2.0 + 1.0j))
    assert st.last_ms(devE) > 0.0 and st.last_ms(host) > 0.0
    # two halves through device pointers continue the stream
    st.reset(devE, 0)
    if clear_between:
        y.fill_(0)
    h1 = n // 2 + 1
    n1 = st.device(devE, x.data_ptr(), h1, y.data_ptr(), stride, stride)
    off = h1 * (4 if fmt == "sc16" else 8)                # bytes per wideband sample
    n2 = st.device(devE, x.data_ptr() + off, n - h1, y.data_ptr() + 8 * n1, stride, stride - n1)
    torch.cuda.synchronize()
    assert n1 + n2 == no and np.array_equal(y.cpu().numpy()[:, :no], want)
    return x, y, want, no, stride


# ---- transmit stages --------------------------------------------------------------------------------------------------

def check_tx_model(y, x, taps, st, shape, fc, first, fmt, what, add=None):
    """A single transmit stage against its float64 model within its derived bound (<stage>_cases.bound, DESIGN.md
    section 7); 16-bit output: |q - scale y64| <= 0.5 + scale bound per part wherever nothing clamps.  Returns the
    worst error / bound."""
    y64, s = st.cases.model(x, taps, *shape, st.cases.phase_step(fc), first)
    if add is not None:
        y64 = y64 + np.asarray(add).astype(np.complex128)
    assert len(y) == len(y64) == st.count(first, len(x), *shape), what
    bound = st.cases.bound(len(taps), shape[0], s, add)
    d = as_complex(y, fmt) - y64
    if fmt == "sc16":
        free = (np.abs(y64.real) * SCALE < 32767 - 1) & (np.abs(y64.imag) * SCALE < 32767 - 1)
        assert np.count_nonzero(free) > 0.9 * len(y), what
        err = np.maximum(np.abs(d.real), np.abs(d.imag))[free]
        bound = (0.5 / SCALE + bound)[free]
    else:
        err = np.abs(d)
    worst = float(np.max(err / np.maximum(bound, 1e-300))) if len(err) else 0.0
    print("%s: %d outputs, worst error / bound = %.3g" % (what, len(y), worst))
    assert np.all(err <= bound), "%s: worst error / bound = %.3g" % (what, worst)
    return worst


def check_tx_bank_model(y, x, taps, st, shape, sel, first, fmt, what):
    """check_tx_model for a transmit bank: the band of the rows ``x`` on the frequencies or channels ``sel`` against the
    bank's float64 model within its derived bound (<stage>_cases.bound); 16-bit output as check_tx_model has it."""
    bc = st.cases
    if st.phase_free:
        y64, s = bc.model(x, taps, *shape, sel)
        bound = bc.bound(len(taps), shape[0], s)
    else:
        y64, s = bc.model(x, taps, *shape, sel, first)
        bound = bc.bound(len(sel), len(taps), shape[0], s)
    assert len(y) == len(y64) == st.count(first, np.asarray(x).shape[-1], *shape), what
    d = as_complex(y, fmt) - y64
    if fmt == "sc16":
        free = (np.abs(y64.real) * SCALE < 32767 - 1) & (np.abs(y64.imag) * SCALE < 32767 - 1)
        assert np.count_nonzero(free) > 0.9 * len(y), what
        err = np.maximum(np.abs(d.real), np.abs(d.imag))[free]
        bound = (0.5 / SCALE + bound)[free]
    else:
        err = np.abs(d)
    worst = float(np.max(err / np.maximum(bound, 1e-300))) if len(err) else 0.0
    print("%s: %d outputs, worst error / bound = %.3g" % (what, len(y), worst))
    assert np.all(err <= bound), "%s: worst error / bound = %.3g" % (what, worst)
    return worst


def check_unit_stage_returns_its_input(eng, st, shape):
    x = tx_stream(np.random.default_rng(1), 5000)
    try:
        st.set(eng, st.cfg(*shape, 0.0, taps=[1.0], out_format="fc32"))
        assert np.array_equal(st.run(eng, x), x)
    finally:
        st.set(eng, None)


def check_single_add_is_one_float32_addition_per_part(eng, st, shape, taps, x, w):
    """``add`` is one float32 addition per part onto the plain output, the 16-bit store is the library's rule on that
    sum, and an ``add`` of any other length is refused without moving the stream."""
    fc = FCS[2]
    try:
        st.set(eng, st.cfg(*shape, fc, taps=taps, out_format="fc32"))
        plain = st.run(eng, x).copy()
        st.reset(eng, 0)
        want = part_sum(w, plain)
        assert np.array_equal(st.run(eng, x, add=w), want)
        check_tx_model(want, x, taps, st, shape, fc, 0, "fc32", "add %s" % (shape,), add=w)
        # 16-bit output: the library's quantisation rule applied to that float32 sum
        st.set(eng, st.cfg(*shape, fc, taps=taps, out_format="sc16"))
        q = st.run(eng, x, add=w)
        assert q.dtype == np.int16 and np.array_equal(q, iqio.to_sc16(want))
        st.reset(eng, 0)
        assert np.array_equal(st.run(eng, x), iqio.to_sc16(plain))
        # `add` must hold exactly what the call produces from where the stream stands (hence the reset: the count of
        # a call depends on its first index)
        st.reset(eng, 0)
        for bad in (w[:-1], np.concatenate([w, w[:1]])):
            with pytest.raises(ValueError):
                st.run(eng, x, add=bad)
        assert np.array_equal(st.run(eng, x, add=w), q)
    finally:
        st.set(eng, None)


def check_tx_single_invalid_arguments(eng, st, base, nin, shape, bads, still_refused, sc16_shape):
    """A single transmit stage: no configuration, every refused configuration (``bads``; one of them again,
    ``still_refused``, with a 16-bit one in force), misaligned pointers and the index limit.  ``base`` builds the
    4-outputs-per-... configuration the file uses, ``nin`` inputs fit the buffers."""
    lib = _abi.load()
    st.set(eng, None)
    x = np.zeros(nin, np.complex64)
    out = np.zeros(4 * nin + 1, np.complex64)
    lim = st.index_limit(*shape)

    def raw(inp=None, outp=None, add=None, nin=nin):
        n = C.c_uint64(0)
        return st.c_fn()(eng._h, C.c_void_p(inp or x.ctypes.data), nin, C.c_void_p(add) if add else None,
                         C.c_void_p(outp or out.ctypes.data), 4 * len(x), C.byref(n))

    def raw_count(n_in):
        n = C.c_uint64(0)
        return st.c_fn("_count")(eng._h, n_in, C.byref(n))

    assert raw() == _abi.OFDM_E_INVAL                # no configuration
    calls = [lambda: st.run(eng, x), lambda: st.reset(eng, 0), lambda: st.last_ms(eng)]
    if st.has_count:
        assert raw_count(10) == _abi.OFDM_E_INVAL
        calls.append(lambda: st.count_of(eng, 10))
    for call in calls:
        with pytest.raises(ValueError):
            call()
    st.set(eng, raw_cfg(base))
    assert raw() == _abi.OFDM_OK
    st.set(eng, None)
    assert raw() == _abi.OFDM_E_INVAL                # ... and after a configuration was dropped
    for bad in bads:
        with pytest.raises(ValueError):
            st.set(eng, raw_cfg(base, **bad))
    for v in (float("nan"), float("inf")):
        c = raw_cfg(base)
        c.taps[3] = v
        with pytest.raises(ValueError):
            st.set(eng, c)
    assert raw() == _abi.OFDM_E_INVAL                # a refused configuration changes nothing: still none in force
    try:
        st.set(eng, raw_cfg(base, center_freq=0.5))  # the ends of the range are inside it
        st.set(eng, raw_cfg(base, center_freq=-0.5, out_format=1, out_scale=0.0))
        # ... and a refused one leaves the old one in force: 16-bit output at the configured ratio
        with pytest.raises(ValueError):
            st.set(eng, raw_cfg(base, **still_refused))
        y = st.run(eng, x)
        assert y.dtype == np.int16 and y.shape == sc16_shape
        st.reset(eng, 0)
        # misaligned pointers: 4-byte for the 16-bit output, 8-byte for every float32 buffer
        assert raw(outp=out.ctypes.data + 2) == _abi.OFDM_E_INVAL
        assert raw(outp=out.ctypes.data + 4) == _abi.OFDM_OK
        assert raw(inp=x.ctypes.data + 4, nin=60) == _abi.OFDM_E_INVAL
        assert raw(add=out.ctypes.data + 4) == _abi.OFDM_E_INVAL
        st.set(eng, raw_cfg(base))
        assert raw(outp=out.ctypes.data + 4) == _abi.OFDM_E_INVAL
        # indices: the stream may stand on the limit and never pass it
        st.reset(eng, lim)
        with pytest.raises(ValueError):
            st.reset(eng, lim + 1)
        assert raw(nin=1) == _abi.OFDM_E_INVAL       # the stream stands at the limit: not one more sample
        if st.has_count:
            assert raw_count(1) == _abi.OFDM_E_INVAL
        assert raw(nin=0) == _abi.OFDM_OK
        st.reset(eng, lim - nin)
        assert raw(nin=nin) == _abi.OFDM_OK and raw(nin=1) == _abi.OFDM_E_INVAL
    finally:
        st.set(eng, None)


def check_modulator_with_the_stage_feeds_the_demodulator(st, shape, fmt, mod_kw, demod_kw, ntaps, ratio, unconfigured):
    """ofdm_mod with the stage (``mod_kw``) in one batch and in three: the stream continues across flush() calls and
    starts afresh after the end; ofdm_demod with the mirror front end (``demod_kw``) returns every payload.  The stages
    named in ``unconfigured`` have no configuration on the modulator's engine."""
    opt = options.default_options(modulation="qpsk", fft_length=512, occupied_tones=200, cp_length=128)
    opt.tx_amplitude = 0.25
    # 90-byte payloads fill their last symbol exactly at this geometry: no seeded fill symbols, whose values depend on a
    # packet's place in its batch, so three batches modulate to the samples of one
    sent = make_payloads(6, 90, seed=3)
    one = ofdm.ofdm_mod(opt, pad_for_usrp=False, iq_format=fmt, **mod_kw)
    three = ofdm.ofdm_mod(opt, pad_for_usrp=False, iq_format=fmt, **mod_kw)
    d = ofdm.ofdm_demod(opt, **demod_kw)
    try:
        for m in (one, three):
            m.engine().set_tx_amplitude(0.1)                    # (the modulator alone has unit gain: keep off the 16-bit rails)
        assert st.cfg_of(one.engine()).ntaps == ntaps and one.engine().tx_iq_format == "fc32"
        assert all(getattr(one.engine(), s + "_cfg") is None for s in unconfigured)
        assert one.flush(end=True) is None                      # nothing queued, nothing in flight
        for p in sent:
            one.send_pkt(p)
        whole = one.flush(end=True)
        _, nsamp = one.engine().tx_frame_count([len(p) for p in sent])
        Q = (ntaps - 1) // shape[0]
        assert len(whole) == st.count(0, nsamp + Q, *shape)
        assert whole.dtype == (np.int16 if fmt == "sc16" else np.complex64)
        # three batches and the end: the stream continues across flush() calls
        sink = iqio.vector_sink()
        three.connect(sink)
        parts = []
        for batch in (sent[:2], sent[2:3], sent[3:]):
            for p in batch:
                three.send_pkt(p)
            parts.append(three.flush())
        assert sum(len(p) for p in parts) == st.count(0, nsamp, *shape)
        three.send_pkt(eof=True)                                # delivers the tail
        assert len(sink.data()) == len(whole) and np.array_equal(sink.data(), whole)
        # ... and a second stream on the same modulator starts afresh
        for p in sent:
            three.send_pkt(p)
        assert np.array_equal(three.flush(end=True), whole)
        wide = iqio.from_sc16(whole) if fmt == "sc16" else whole
        got = d.work(with_noise_floor(wide, ratio, 4096, 8192))
        assert [p for ok, p in got if ok] == sent
    finally:
        for o in (one, three, d):
            o.engine().close()


def check_transmit_path_and_command_line(st, tmp_path, set_options, want_cfg, tx_flags, rx_flags, rx_flags_other, ratio,
                                         period):
    """transmit_path with the options' attributes as the command line sets them; benchmark_ofdm_tx with ``tx_flags``
    writes a band that benchmark_ofdm_rx with ``rx_flags`` reads back, and tuned to the other side finds nothing."""
    opt = options.default_options(modulation="qpsk", fft_length=512, occupied_tones=200, cp_length=128)
    opt.tx_amplitude = 0.25
    set_options(opt)
    tp = transmit_path.transmit_path(opt)
    try:
        cfg = st.cfg_of(tp.ofdm_tx.engine())
        assert tuple(getattr(cfg, k) for k in want_cfg) == tuple(want_cfg.values())
        tp.send_pkt(b"\x00\x01\x00\x00 one packet")
        y = tp.flush(end=True)
        assert y.dtype == np.complex64 and len(y) > 0 and len(y) % period == 0
    finally:
        tp.ofdm_tx.engine().close()
    f = str(tmp_path / "wide.dat")
    npk = benchmark_ofdm_tx.main(["-m", "qpsk", "--to-file", f, "-M", "9e-6"] + tx_flags)
    assert npk == 4
    wide = iqio.read_complex_binary(f)
    assert len(wide) % period == 0
    iqio.file_sink(f).write(with_noise_floor(wide, ratio, 4096, 8192))
    acct = benchmark_ofdm_rx.main(["-m", "qpsk", "--from-file", f, "--to-file", str(tmp_path / "rx.txt")] + rx_flags)
    assert (acct.n_rcvd, acct.n_right) == (4, 4)
    # tuned to the other side of the band there is nothing
    acct = benchmark_ofdm_rx.main(["-m", "qpsk", "--from-file", f, "--to-file", str(tmp_path / "rx.txt")] + rx_flags_other)
    assert acct.n_right == 0


def check_single_device_pointer_path_behind_an_asynchronous_transmit(torch, st, shape, fc, taps, more=None):
    """The stage's input is what tx_device(wait=False) is still producing on the same handle; then ``add`` aliasing the
    output.  ``more(dev, d_iq, nsamp)`` goes on with the device handle."""
    cfg = make_cfg()
    pays = make_payloads(4, 100, seed=7)
    host = engine.Engine(cfg=cfg)
    dev = engine.Engine(cfg=make_cfg(device_ptrs=True))
    try:
        x = host.tx(pays)
        nw = st.count(0, len(x), *shape)
        st.set(host, st.cfg(*shape, fc, taps=taps))
        want = st.run(host, x)
        w = tx_stream(np.random.default_rng(2), nw, 0.1)
        st.reset(host, 0)
        want_add = st.run(host, x, add=w)

        blob, offs, lens = engine.pack_payloads(pays)
        _, nsamp = dev.tx_frame_count(lens)
        assert nsamp == len(x)
        d_pay = torch.from_numpy(blob.copy()).cuda()
        d_iq = torch.zeros(nsamp, dtype=torch.complex64, device="cuda")
        d_out = torch.zeros(nw, dtype=torch.complex64, device="cuda")
        st.set(dev, st.cfg(*shape, fc, taps=taps))
        torch.cuda.synchronize()
        if st.has_count:
            assert st.count_of(dev, nsamp) == nw
        assert dev.tx_device(d_pay.data_ptr(), offs, lens, d_iq.data_ptr(), nsamp, wait=False) == nsamp
        assert st.device(dev, d_iq.data_ptr(), nsamp, d_out.data_ptr(), nw) == nw
        assert np.array_equal(d_iq.cpu().numpy(), x)
        assert np.array_equal(d_out.cpu().numpy(), want)
        # `add` aliasing the output: each sample is read before it is written
        d_out.copy_(torch.from_numpy(w))
        torch.cuda.synchronize()
        st.reset(dev, 0)
        assert st.device(dev, d_iq.data_ptr(), nsamp, d_out.data_ptr(), nw, add_ptr=d_out.data_ptr()) == nw
        assert np.array_equal(d_out.cpu().numpy(), want_add)
        assert np.array_equal(want_add, part_sum(w, want))
        if more is not None:
            more(dev, d_iq, nsamp)
    finally:
        host.close()
        dev.close()


def check_transmitter_and_receiver_launch_what_they_launched(st, shape, fc, taps, nout):
    """Two handles run the same TX + RX: one never saw the stage, the other used it and dropped it.  Same IQ bits,
    same packets, same per-kernel launch counts; the kernel table has no entry for the stage."""
    cfg = make_cfg()
    pays = make_payloads(4, 100, seed=11)
    a, b = engine.Engine(cfg=cfg), engine.Engine(cfg=cfg)
    try:
        st.set(b, st.cfg(*shape, fc, taps=taps))
        b.prof_enable(True)
        assert len(st.run(b, tx_stream(np.random.default_rng(1), 3000, 0.1))) == nout == st.count(0, 3000, *shape)
        assert st.last_ms(b) > 0.0
        st.set(b, None)
        with pytest.raises(ValueError):
            st.last_ms(b)
        for e in (a, b):
            e.set_channel(sigma=0.01, lead=1024, tail=1536)
            e.prof_enable(True)
            e.prof_reset()
        xa, xb = a.tx(pays), b.tx(pays)
        assert np.array_equal(xa, xb)
        pa, pb = a.rx(xa), b.rx(xb)
        assert pa == pb and [p for ok, p in pa if ok] == pays
        ca, cb = launches(a), launches(b)
        assert ca == cb and sum(ca.values()) > 0
        assert len(ca) == _abi.K_COUNT == 11 and not any(st.kernel_word in k for k in ca)
        # with the stage configured and used, the kernel table still counts only what it counted
        st.set(b, st.cfg(*shape, fc, taps=taps))
        b.prof_reset()
        st.run(b, xb)
        assert np.array_equal(b.tx(pays), xa) and b.rx(xa) == pa
        assert launches(b) == ca
    finally:
        a.close()
        b.close()


# ---- transmit banks (rows in, one band out) ---------------------------------------------------------------------------

def check_tx_bank_segmentation(eng, st, shape, ntaps, sel, fmt, seed, far, band_spare=0):
    """The band in one call and in chunks of every critical size (0, 1, around the history, around the tile), plain from
    index 0 and added onto a band from ``far``: the same stored bits.  The band to add onto is ``band_spare`` samples
    longer than a call from index 0 produces."""
    bc = st.cases
    rng = np.random.default_rng(seed)
    Ti, Q = st.tile_inputs(*shape), st.history(ntaps, *shape)
    nin = 3 * Ti + 100 + 3 * Q
    x, h = rows(rng, len(sel), nin), bc.taps_for(rng, ntaps)
    band = rows(rng, 1, st.count(0, nin, *shape) + band_spare)[0]
    try:
        st.set(eng, st.cfg(*shape, sel, taps=h, out_format=fmt))
        for first, add in ((0, None), (far, band)):
            no = st.count(first, nin, *shape)
            st.reset(eng, first)
            whole = st.run(eng, x, add=None if add is None else add[:no]).copy()
            assert len(whole) == no and np.any(whole != 0)
            st.reset(eng, first)
            sizes = bc.chunk_inputs(rng, nin, *shape, ntaps)
            assert sum(sizes) == nin and {0, 1, Q + 1, Ti + 1, Ti - 1} <= set(sizes)
            assert (Q in sizes or Q == 0) and (Q - 1 in sizes or Q <= 1)
            parts, a, o = [], 0, 0
            for n in sizes:
                cnt = st.count(first + a, n, *shape)
                if st.has_count:
                    assert st.count_of(eng, n) == cnt
                y = st.run(eng, x[:, a:a + n], add=None if add is None else add[o:o + cnt])
                assert len(y) == cnt                            # the count is what the call returns
                parts.append(y.copy())
                a += n
                o += cnt
            got = np.concatenate(parts)
            assert got.dtype == whole.dtype and np.array_equal(bits(got), bits(whole)), (shape, ntaps, first, fmt)
    finally:
        st.set(eng, None)


def check_one_row_at_zero_frequency_is_the_single_stage(eng, st, shape, ntaps, fmt, seed, sel):
    """``sel`` (one link at fc = 0, or channel 0 alone) against the single stage at fc = 0: equal as numbers (the sign
    of a zero may differ), from both starts."""
    one, bc = STAGES[st.single], st.cases
    rng = np.random.default_rng(seed)
    x = rows(rng, 1, bc.stream_inputs(*shape))
    h = bc.taps_for(rng, ntaps)
    try:
        st.set(eng, st.cfg(*shape, sel, taps=h, out_format=fmt))
        one.set(eng, one.cfg(*shape, 0.0, taps=h, out_format=fmt))
        for first in (0, START):
            st.reset(eng, first)
            one.reset(eng, first)
            a, b = st.run(eng, x), one.run(eng, x[0])
            assert a.shape == b.shape and a.dtype == b.dtype
            assert np.array_equal(a, b), (shape, ntaps, fmt, first)
        assert np.any(a != 0)
    finally:
        st.set(eng, None)
        one.set(eng, None)


def check_one_link_with_the_unit_tap_is_the_single_stage(eng, st, shape, seed, fcs):
    """h = {1.0}: the table is (1, 0), the chain is one exact product, and what is left is r, the phase convention and
    the gr_complex product -- the single stage's, bit for bit, at every fc of ``fcs`` and wherever the stream starts."""
    one = STAGES[st.single]
    rng = np.random.default_rng(seed)
    x = rows(rng, 1, st.cases.stream_inputs(*shape), amp=1.0)
    try:
        for fc in fcs:
            st.set(eng, st.cfg(*shape, [fc], taps=[1.0]))
            one.set(eng, one.cfg(*shape, fc, taps=[1.0]))
            for first in (0, START, FAR):
                st.reset(eng, first)
                one.reset(eng, first)
                a, b = st.run(eng, x), one.run(eng, x[0])
                assert len(a) == len(b) and np.array_equal(a, b) and np.any(a != 0), (shape, fc, first)
    finally:
        st.set(eng, None)
        one.set(eng, None)


def check_a_link_of_zeros_changes_no_value(eng, st, shape, ntaps, seed):
    bc = st.cases
    rng = np.random.default_rng(seed)
    nin = bc.stream_inputs(*shape)
    x, h = rows(rng, 3, nin), bc.taps_for(rng, ntaps)
    z = np.zeros((1, nin), np.complex64)
    fcs = bc.freqs(3)
    try:
        st.set(eng, st.cfg(*shape, fcs, taps=h))
        ref = st.run(eng, x).copy()
        assert np.any(ref != 0)
        st.set(eng, st.cfg(*shape, fcs + [0.37], taps=h))
        assert np.array_equal(st.run(eng, np.concatenate([x, z])), ref)
        st.set(eng, st.cfg(*shape, [0.37] + fcs, taps=h))
        assert np.array_equal(st.run(eng, np.concatenate([z, x])), ref)
        # the order of the list is part of the configuration: the same links in another order are the same signal
        st.set(eng, st.cfg(*shape, fcs[::-1], taps=h))
        other = st.run(eng, x[::-1])
        _, s = bc.model(x, h, *shape, fcs)
        assert np.all(np.abs(other.astype(np.complex128) - ref.astype(np.complex128)) <= 2 * bc.bound(3, ntaps, shape[0], s))
    finally:
        st.set(eng, None)


def check_bank_add_and_sc16_store(eng, st, shape, ntaps, seed):
    """``add`` is one float32 addition per part; an ``add`` of another length is refused; the 16-bit store is the
    transmit rule on the same float32 value, and on the sum where there is an add."""
    bc = st.cases
    rng = np.random.default_rng(seed)
    nin = bc.stream_inputs(*shape)
    no = st.count(0, nin, *shape)
    x, h, fcs = rows(rng, 3, nin), bc.taps_for(rng, ntaps), bc.freqs(3)
    band = rows(rng, 1, no, amp=3.0)[0]
    try:
        st.set(eng, st.cfg(*shape, fcs, taps=h))
        v = st.run(eng, x).copy()
        assert len(v) == no
        st.reset(eng, 0)
        got = st.run(eng, x, add=band)
        want = (v.real + band.real).astype(np.float32) + 1j * (v.imag + band.imag).astype(np.float32)
        assert np.array_equal(got, want.astype(np.complex64))
        st.reset(eng, 0)                                  # (the count is the stream's: from the same start)
        for wrong in (band[:-1], np.concatenate([band, band[:1]])):
            with pytest.raises(ValueError):
                st.run(eng, x, add=wrong)
        # 16-bit output: the transmit rule on the same float32 value, and on the sum where there is an add
        for scale in (None, 1000.0):
            st.set(eng, st.cfg(*shape, fcs, taps=h, out_format="sc16", out_scale=scale))
            assert np.array_equal(st.run(eng, x), iqio.to_sc16(v, scale or SCALE))
            small = (band * np.float32(0.01)).astype(np.complex64)
            st.reset(eng, 0)
            sum32 = (v.real + small.real).astype(np.float32) + 1j * (v.imag + small.imag).astype(np.float32)
            assert np.array_equal(st.run(eng, x, add=small), iqio.to_sc16(sum32.astype(np.complex64), scale or SCALE))
    finally:
        st.set(eng, None)


def check_against_k_single_stage_passes(eng, st, shape, ntaps, K, seed, fcs):
    """Same taps and frequencies, one pass of the single stage per link with add=band: the two ways differ by no more
    than the bank's bound plus the sum of the passes' bounds (a pass's `add` being the band so far)."""
    one, bc = STAGES[st.single], st.cases
    rng = np.random.default_rng(seed)
    nin = bc.stream_inputs(*shape)
    x, h = rows(rng, K, nin), bc.taps_for(rng, ntaps)
    try:
        for first in (0, START):
            st.set(eng, st.cfg(*shape, fcs, taps=h))
            st.reset(eng, first)
            y = st.run(eng, x).copy()
            _, s_terms = bc.model_terms(x, h, *shape, fcs, first)
            bound = bc.bound(K, ntaps, shape[0], s_terms.sum(axis=0))
            band = None
            for i, fc in enumerate(fcs):
                one.set(eng, one.cfg(*shape, fc, taps=h))
                one.reset(eng, first)
                bound = bound + one.cases.bound(ntaps, shape[0], s_terms[i], band)
                band = one.run(eng, x[i], add=band).copy()
            err = np.abs(y.astype(np.complex128) - band.astype(np.complex128))
            print("%s ntaps=%d K=%d first=%d: worst |bank - passes| / (sum of the bounds) = %.3g"
                  % (shape, ntaps, K, first, float(np.max(err / np.maximum(bound, 1e-300)))))
            assert len(y) == len(band) and np.all(err <= bound) and np.any(y != 0)
    finally:
        st.set(eng, None)
        one.set(eng, None)


def check_in_device_mode_add_may_be_the_output_buffer(torch, st, shape, sel, ntaps, nin):
    bc = st.cases
    rng = np.random.default_rng(31)
    no = st.count(0, nin, *shape)
    stride = nin + 5
    x = np.zeros((3, stride), np.complex64)
    x[:, :nin] = rows(rng, 3, nin)
    band = rows(rng, 1, no)[0]
    h = bc.taps_for(rng, ntaps)
    host = engine.Engine(cfg=make_cfg())
    dev = engine.Engine(cfg=make_cfg(device_ptrs=True))
    try:
        for e in (host, dev):
            st.set(e, st.cfg(*shape, sel, taps=h))
            e.prof_enable(True)
        with pytest.raises(ValueError):
            st.last_ms(dev)                               # no profiled call yet
        want = st.run(host, x[:, :nin], add=band)
        d_x = torch.from_numpy(x).cuda()
        d_out = torch.from_numpy(band.copy()).cuda()
        torch.cuda.synchronize()
        assert st.device(dev, d_x.data_ptr(), stride, nin, d_out.data_ptr(), no, add_ptr=d_out.data_ptr()) == no
        assert np.array_equal(d_out.cpu().numpy(), want)
        assert st.last_ms(dev) > 0.0 and st.last_ms(host) > 0.0
        # two halves through device pointers continue the stream
        st.reset(dev, 0)
        d_out.copy_(torch.from_numpy(band))
        torch.cuda.synchronize()
        n1 = nin // 2 + 1
        a = st.device(dev, d_x.data_ptr(), stride, n1, d_out.data_ptr(), no, add_ptr=d_out.data_ptr())
        b = st.device(dev, d_x.data_ptr() + 8 * n1, stride, nin - n1, d_out.data_ptr() + 8 * a, no - a,
                      add_ptr=d_out.data_ptr() + 8 * a)
        assert a == st.count(0, n1, *shape) and a + b == no and np.array_equal(d_out.cpu().numpy(), want)
        zero(torch, d_x, d_out)
        del d_x, d_out
        torch.cuda.empty_cache()
    finally:
        host.close()
        dev.close()


def check_mod_bank_continues_and_drops_a_failing_batch(tx, plain, sent, st, shape, Q):
    """Two batches continue the band; the tail comes with end=True, which also starts the bank afresh.  A failing batch
    is dropped on every link and the band has not moved.  ``plain`` are single-link modulators fed the same packets."""
    e = tx.engine()
    halves = []
    for part in (slice(0, 1), slice(1, None)):
        for i, pays in enumerate(sent):
            for p in pays[part]:
                tx.send_pkt(i, p)
                plain[i].send_pkt(p)
        halves.append((tx.flush(end=part.start == 1), [m.flush() for m in plain]))
    assert tx.flush() is None and tx.flush(end=True) is None       # nothing queued, nothing in flight
    pos = 0
    for j, (got, nbj) in enumerate(halves):
        nj = max(len(v) for v in nbj)
        assert j == 0 or min(len(v) for v in nbj) < nj
        xj = np.zeros((3, nj + (Q if j == 1 else 0)), np.complex64)
        for i, v in enumerate(nbj):
            xj[i, :len(v)] = v
        want = st.run(e, xj)                                          # (the bank had reset: the same stream again)
        assert len(got) == st.count(pos, xj.shape[1], *shape) and np.array_equal(bits(got), bits(want)), j
        pos += xj.shape[1]
    st.reset(e, 0)
    # a failing batch (link 1 holds something the engine cannot frame) is dropped on ALL links, link 0's that was
    # already modulated and link 2's that was not yet; the band has not moved
    tx.send_pkt(0, sent[0][0])
    tx.links()[1]._pending.append(object())
    tx.send_pkt(2, sent[2][0])
    with pytest.raises(Exception):
        tx.flush()
    assert all(not m._pending for m in tx.links()) and tx.flush() is None and tx.flush(end=True) is None
    tx.send_pkt(0, sent[0][0])
    plain[0].send_pkt(sent[0][0])
    one = plain[0].flush()
    x1 = np.zeros((3, len(one)), np.complex64)
    x1[0] = one
    got = tx.flush().copy()
    st.reset(e, 0)
    assert np.array_equal(bits(got), bits(st.run(e, x1))) and np.any(got != 0)


def check_tx_bank_layout_and_capacity(eng, st, shape, sel, taps, nin, one_sel):
    """A transmit bank's input layout: a row stride beyond nin is not read, a capacity one short or a stride below nin
    is refused and moves nothing, calls of 0 and shorter than the history are part of the stream, one row ignores the
    stride."""
    rng = np.random.default_rng(5)
    x = rows(rng, 3, nin)
    Q = st.history(len(taps), *shape)
    no = st.count(0, nin, *shape)
    st.set(eng, st.cfg(*shape, sel, taps=taps))
    try:
        want = st.run(eng, x).copy()
        assert len(want) == no
        # stride > nin: the gaps are not read
        st.reset(eng, 0)
        wide = np.full((3, nin + 13), np.complex64(np.nan), np.complex64)
        wide[:, :nin] = x
        out = np.zeros(no, np.complex64)
        assert st.raw(eng._h, wide, out, nin + 13, no, nin) == (_abi.OFDM_OK, no)
        assert np.array_equal(out, want)
        # out_cap one short: refused with *nout set, and the stream does not move
        st.reset(eng, 0)
        n1 = 401
        first = st.run(eng, x[:, :n1]).copy()
        rest_in = np.ascontiguousarray(x[:, n1:])
        n2 = nin - n1
        no2 = st.count(n1, n2, *shape)
        assert len(first) + no2 == no
        if st.has_count:
            assert st.count_of(eng, n2) == no2
        out = np.full(no2, SENTINEL, np.complex64)
        assert st.raw(eng._h, rest_in, out, n2, no2 - 1, n2) == (_abi.OFDM_E_CAPACITY, no2)
        assert np.all(out == SENTINEL)
        if st.has_count:
            assert st.count_of(eng, n2) == no2
        # stride < nin with more than one row
        assert st.raw(eng._h, rest_in, out, n2 - 1, no2, n2)[0] == _abi.OFDM_E_INVAL
        assert np.all(out == SENTINEL)
        rest = st.run(eng, rest_in)
        assert np.array_equal(np.concatenate([first, rest]), want)        # the stream continues bit for bit
        # calls of 0 and calls shorter than Q are part of the stream
        st.reset(eng, 0)
        assert Q >= 2
        parts = [st.run(eng, x[:, a:b]).copy() for a, b in ((0, 0), (0, 1), (1, Q), (Q, Q), (Q, nin))]
        assert [len(p) for p in parts[:4]] == [0, st.count(0, 1, *shape), st.count(1, Q - 1, *shape), 0]
        assert np.array_equal(np.concatenate(parts), want)
        # one row: the stride does not matter
        st.set(eng, st.cfg(*shape, one_sel, taps=taps))
        one = st.run(eng, x[1]).copy()
        st.reset(eng, 0)
        out = np.zeros(no, np.complex64)
        assert st.raw(eng._h, np.ascontiguousarray(x[1]), out, 0, no, nin) == (_abi.OFDM_OK, no)
        assert np.array_equal(out, one)
    finally:
        st.set(eng, None)


def check_tx_bank_invalid_arguments(eng, st, shape, base, nout, still_refused, edge_sel):
    """A transmit bank: no configuration; every refused configuration (the descriptor's refused_fields, refused_sel in
    slot 1 of its sel_field, a NaN and an infinite tap), each with its message and through the raw ABI, none touching
    the configuration in force; the index limit; a call too long for one grid; misaligned and null pointers.
    ``still_refused`` indexes the entry of refused_sel that is tried again in mid-stream, ``edge_sel`` (or None) is a
    selection at the ends of its range."""
    lib = _abi.load()
    st.set(eng, None)
    x = np.zeros((2, 16), np.complex64)
    x[:, ::3] = 1.0
    out = np.zeros(64, np.complex64)
    nn = C.c_uint64(0)
    no = nout                                           # outputs of 16 inputs per row
    assert no == st.count(0, 16, *shape)
    raw = lambda stride, nin, cap=64: st.raw(eng._h, x, out, stride, cap, nin)
    assert raw(16, 16)[0] == _abi.OFDM_E_INVAL            # no configuration
    calls = [lambda: st.run(eng, x), lambda: st.reset(eng, 0), lambda: st.last_ms(eng)]
    if st.has_taps:
        calls.append(lambda: st.taps(eng, 0))
    if st.has_count:
        assert st.c_fn("_count")(eng._h, 16, C.byref(nn)) == _abi.OFDM_E_INVAL
        calls.append(lambda: st.count_of(eng, 4))
    for call in calls:
        with pytest.raises(ValueError):
            call()
    good = raw_cfg(base)
    st.set(eng, good)
    table = st.taps(eng, 1) if st.has_taps else None
    assert raw(16, 16) == (_abi.OFDM_OK, no)
    y = out[:no].copy()
    bad_sel = []
    for v in st.refused_sel:
        c = raw_cfg(base)
        getattr(c, st.sel_field)[1] = v
        bad_sel.append(c)
    bad_tap = []
    for v in (float("nan"), float("inf")):
        c = raw_cfg(base)
        c.taps[3] = v
        bad_tap.append(c)
    refused = [raw_cfg(base, **b) for b in st.refused_fields] + bad_sel + bad_tap
    messages = set()
    for c in refused:
        with pytest.raises(ValueError) as info:
            st.set(eng, c)
        assert str(info.value)                            # each refusal has its message
        messages.add(str(info.value))
        assert st.cfg_of(eng) is good
    if st.refusal_messages is not None:
        assert len(messages) == st.refusal_messages
    for c in refused:
        assert st.c_fn("set")(eng._h, C.byref(c)) == _abi.OFDM_E_INVAL
    c = raw_cfg(base)
    getattr(c, st.sel_field)[2] = st.beyond               # an entry beyond the count of rows is not looked at
    st.set(eng, c)
    st.set(eng, good)
    # a refused configuration leaves the one in force untouched: same table, same stream position, same outputs
    a = st.run(eng, x[:, :7]).copy()
    with pytest.raises(ValueError):
        st.set(eng, bad_sel[still_refused])
    if st.has_taps:
        assert np.array_equal(st.taps(eng, 1), table)
    b = st.run(eng, x[:, 7:])
    assert np.array_equal(np.concatenate([a, b]), y)
    if edge_sel is not None:
        # the ends of the range are inside it
        st.set(eng, st.cfg(*shape, edge_sel, taps=np.ones(good.ntaps, np.float32)))
        st.set(eng, good)
    # the index limit is the single stage's
    lim = st.index_limit(*shape)
    st.reset(eng, lim)
    with pytest.raises(ValueError):
        st.reset(eng, lim + 1)
    assert raw(16, 1)[0] == _abi.OFDM_E_INVAL             # one input more would pass it
    if st.has_count:
        assert st.c_fn("_count")(eng._h, 1, C.byref(nn)) == _abi.OFDM_E_INVAL
    assert raw(16, 0) == (_abi.OFDM_OK, 0)
    if st.phase_free:
        # a call may end on the limit, and gives the bits of any other start
        st.reset(eng, lim - 16)
        assert raw(16, 16) == (_abi.OFDM_OK, no) and np.array_equal(out[:no], y)
    st.reset(eng, 0)
    assert raw(2 * lim, 2 * lim)[0] == _abi.OFDM_E_INVAL
    # a call too long for one grid (more than 2^31 - 1 tiles): refused before anything is read or written, the stream
    # stays where it was
    long_n = (1 << 31) * st.tile_inputs(*shape) + 1
    assert raw(long_n, long_n, 1 << 62) == (_abi.OFDM_E_INVAL, st.count(0, long_n, *shape))
    assert b"too long" in lib.ofdm_last_error(eng._h)
    assert raw(16, 16) == (_abi.OFDM_OK, no) and np.array_equal(out[:no], y)
    st.reset(eng, 0)
    # misaligned buffers: complex64 in, add and out on 8 bytes, 16-bit out on 4
    f = np.zeros(2 * 64 + 2, np.float32)
    fn = st.c_fn()
    xp, op, odd = x.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), C.c_void_p(f.ctypes.data + 4)
    assert fn(eng._h, odd, 0, 16, None, op, 64, C.byref(nn)) == _abi.OFDM_E_INVAL
    assert fn(eng._h, xp, 16, 16, odd, op, 64, C.byref(nn)) == _abi.OFDM_E_INVAL
    assert fn(eng._h, xp, 16, 16, None, odd, 64, C.byref(nn)) == _abi.OFDM_E_INVAL
    assert fn(eng._h, xp, 16, 16, None, None, 64, C.byref(nn)) == _abi.OFDM_E_INVAL       # null iq_out
    assert fn(eng._h, None, 16, 16, None, op, 64, C.byref(nn)) == _abi.OFDM_E_INVAL       # null iq_in
    assert fn(eng._h, xp, 16, 16, None, op, 64, None) == _abi.OFDM_E_INVAL
    st.set(eng, raw_cfg(base, out_format=1))
    try:
        q = np.zeros(2 * 64 + 2, np.int16)
        assert fn(eng._h, xp, 16, 16, None, C.c_void_p(q.ctypes.data + 2), 64, C.byref(nn)) == _abi.OFDM_E_INVAL
        assert fn(eng._h, xp, 16, 16, None, C.c_void_p(q.ctypes.data + 4), 64, C.byref(nn)) == _abi.OFDM_OK
        assert np.array_equal(q[2:2 + 2 * no].reshape(-1, 2), iqio.to_sc16(y))             # ... and the stream had not moved
    finally:
        st.set(eng, None)
    assert raw(16, 16)[0] == _abi.OFDM_E_INVAL            # ... and after it was dropped


def check_bank_device_pointer_path_behind_an_asynchronous_transmit(torch, st, shape, fcs, taps):
    """The bank's input is what tx_device(wait=False) is still producing on the same handle."""
    pays = make_payloads(4, 100, seed=7)
    host = engine.Engine(cfg=make_cfg())
    dev = engine.Engine(cfg=make_cfg(device_ptrs=True))
    try:
        x = host.tx(pays)
        st.set(host, st.cfg(*shape, fcs, taps=taps))
        # the two links are the two halves of the buffer the transmitter fills
        nin = len(x) // 2
        wide = st.run(host, np.stack([x[:nin], x[nin:2 * nin]]))
        no = len(wide)
        assert no == st.count(0, nin, *shape)
        blob, offs, lens = engine.pack_payloads(pays)
        _, nsamp = dev.tx_frame_count(lens)
        assert nsamp == len(x)
        d_pay = torch.from_numpy(blob.copy()).cuda()
        d_iq = torch.zeros(nsamp, dtype=torch.complex64, device="cuda")
        d_wide = torch.zeros(no, dtype=torch.complex64, device="cuda")
        st.set(dev, st.cfg(*shape, fcs, taps=taps))
        torch.cuda.synchronize()
        assert dev.tx_device(d_pay.data_ptr(), offs, lens, d_iq.data_ptr(), nsamp, wait=False) == nsamp
        assert st.device(dev, d_iq.data_ptr(), nin, nin, d_wide.data_ptr(), no) == no
        assert np.array_equal(d_wide.cpu().numpy(), wide) and np.any(wide != 0)
        zero(torch, d_pay, d_iq, d_wide)
        del d_pay, d_iq, d_wide
        torch.cuda.empty_cache()
    finally:
        host.close()
        dev.close()


def check_a_handle_that_dropped_the_bank_launches_what_it_launched(st, shape, fcs, nout):
    """Two handles transmit the same packets: one never saw the bank, the other used it and dropped it.  Same IQ bits,
    same per-kernel launch counts; the kernel table has no entry for the stage."""
    pays = make_payloads(3, 100, seed=3)
    a, b = engine.Engine(cfg=make_cfg()), engine.Engine(cfg=make_cfg())
    try:
        st.set(b, st.cfg(*shape, fcs, occupied_fraction=200 / 512.0))
        assert len(st.run(b, rows(np.random.default_rng(2), 2, 3000))) == nout == st.count(0, 3000, *shape)
        st.set(b, None)
        for e in (a, b):
            e.prof_enable(True)
            e.prof_reset()
        ia, ib = a.tx(pays), b.tx(pays)
        assert np.array_equal(ia, ib)
        ca, cb = launches(a), launches(b)
        assert ca == cb and sum(ca.values()) > 0
        assert len(ca) == _abi.K_COUNT == 11 and not any(st.kernel_word in k for k in ca)
    finally:
        a.close()
        b.close()


# ---- host side (no GPU) -----------------------------------------------------------------------------------------------

def check_header_declares_and_library_exports(funcs):
    """Every name of ``funcs`` is declared in include/ofdm_hip.h, listed in _abi.EXPORTS and exported; the ABI version
    and the kernel table are what they were.  Returns the header, and the header without its comments."""
    hdr = open(os.path.join(ROOT, "include", "ofdm_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(ofdm_[a-z_0-9]+)\s*\(", code))
    lib = _abi.load()
    for name in funcs:
        assert name in declared, name
        assert name in _abi.EXPORTS, name
        assert hasattr(lib, name), name
    # additions only: the version and the kernel table are what they were
    assert re.search(r"#define\s+OFDM_ABI_VERSION\s+6\b", code) and lib.ofdm_abi_version() == 6
    assert _abi.OFDM_ABI_VERSION == 6
    assert _abi.K_COUNT == 11 and re.search(r"OFDM_K_COUNT\s*=\s*11\b", code)
    return hdr, code


def check_cfg_layout_matches_header(tmp_path, st, size, macros=()):
    """sizeof / offsetof as the C compiler sees include/ofdm_hip.h == the ctypes mirror ``st`` (of ``size`` bytes).
    Returns what the C program printed, the values of ``macros`` (name -> C macro) among it."""
    name = st.__name__
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ofdm_hip.h"', 'int main(void){',
             'printf("size %%zu\\n", sizeof(%s));' % name]
    for key, macro in macros:
        lines.append('printf("%s %%d\\n", %s);' % (key, macro))
    for f, _ in st._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(%s, %s));' % (f, name, f))
    lines.append('return 0;}')
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)])
    got = dict(l.split() for l in subprocess.check_output([exe]).decode().splitlines())
    assert int(got["size"]) == C.sizeof(st) == size
    for f, _ in st._fields_:
        assert int(got[f]) == getattr(st, f).offset, f
    return got


def qpsk_options():
    return options.default_options(modulation="qpsk")


def check_arguments_are_checked_before_any_engine_exists(monkeypatch, ctor, positional, defaults, kw):
    """``ctor`` with ``defaults`` overridden by ``kw`` (the names in ``positional`` passed in that order) raises
    ValueError before it creates an engine.  options=3 stands for three option sets, one more than the links."""
    def no_engine(*a, **k):
        raise AssertionError("an engine was created before the arguments were checked")
    monkeypatch.setattr(engine, "Engine", no_engine)
    args = dict(defaults, options=qpsk_options())
    args.update(kw)
    if args["options"] == 3:
        args["options"] = [qpsk_options()] * 3
    with pytest.raises(ValueError):
        ctor(*[args.pop(k) for k in positional], **args)


def check_mod_links_drops_a_failing_batch_on_every_link(cls, stage, cfg):
    """flush() of the multi-link modulator ``cls`` modulates every link before the band moves; a link that fails takes
    the whole batch with it, and Engine.<stage> is never called."""
    class Link(object):
        def __init__(self, fail):
            self._pending, self.fail = [b"p"], fail

        def flush(self):
            self._pending = []
            if self.fail:
                raise RuntimeError("link failed")
            return np.ones(4, np.complex64)

    class Bank(object):
        calls = 0

    def run(self, x):
        Bank.calls += 1
    setattr(Bank, stage, run)
    tx = cls.__new__(cls)
    tx._links, tx._engine, tx._live = [Link(False), Link(True), Link(False)], Bank(), False
    setattr(tx._engine, stage + "_cfg", cfg)
    with pytest.raises(RuntimeError):
        tx.flush()
    assert Bank.calls == 0 and not tx._live and all(not m._pending for m in tx._links)
    assert tx.flush() is None


def check_command_line_refuses(monkeypatch, capsys, tmp_path, main, argv, names):
    """``main(argv)`` exits with status 2 and names ``names`` on stderr, before an engine or a file in tmp_path exists."""
    def no_engine(*a, **k):
        raise AssertionError("an engine was created for a refused command line")
    monkeypatch.setattr(engine, "Engine", no_engine)
    with pytest.raises(SystemExit) as e:
        main(argv)
    assert e.value.code == 2 and names in capsys.readouterr().err
    assert not list(tmp_path.iterdir())           # refused before a file was opened
