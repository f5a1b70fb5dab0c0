"""The synthetic channel on the GPU against the oracle, sample for sample.

ofdm_tx with a channel set writes a whole buffer through three kernels: k_tx_mod's fused store (the paired route, one
Philox call per two samples with the halves swapped between neighbouring lanes, or the per-sample route when the
lead-in or the cyclic prefix is odd or sigma is 0; each in the LEAN instantiation and in the full one, for float and
for 16-bit output) and the noise-only fills of lead-in and tail (k_channel, k_noise_sc16).  The reference is the
oracle's transmit buffer put through orc_channel as ONE stream from index 0, so lead-in, body samples, prefix copies
and tail are each checked at their own stream index; orc_channel itself is held to a float64 model by
test_channel_host.py, which also shows that exchanged or reused noise words miss by orders of magnitude.

The bound (chan_cases.engine_bound) is the issue's: 1e-4 sigma + 4 * 2^-24 (|clean| + |ref|) per sample."""
import collections

import numpy as np
import pytest

import chan_cases as cc
from ofdm_uhd_amd import _abi, engine, iqio
from ofdm_uhd_amd.engine import pack_payloads

pytestmark = pytest.mark.gpu

Run = collections.namedtuple("Run", "case eng pay iq")


def _arm(eng, case, fmt="fc32", taps=()):
    """channel on with the case's parameters, output format, taps: everything the launch rule looks at"""
    eng.set_channel(lead=case.lead, tail=cc.tail_of(case), **cc.chan_args(case))
    eng.set_tx_iq_format(fmt)
    eng.set_taps(*taps)


@pytest.fixture(scope="module", params=cc.CASES, ids=cc.IDS)
def run(request):
    """One engine per case and its float run without taps (LEAN when the case has no carrier offset), computed once."""
    case = request.param
    eng = engine.Engine(cfg=cc.cfg_of(case))
    pay = cc.payloads_of(case)
    _arm(eng, case)
    eng.prof_enable(True)
    eng.prof_reset()
    iq = eng.tx(pay)
    launches = {k: v[1] for k, v in eng.prof().items()}
    eng.prof_enable(False)
    assert launches["k_tx_mod"] == 1 and launches["k_channel"] == 2, launches      # modulator, lead-in fill, tail fill
    iq.setflags(write=False)
    yield Run(case, eng, pay, iq)
    eng.close()


def _ratio(err, bound):
    """error over bound; where the bound is 0 (silence in, no noise) the error has to be 0 too"""
    pos = bound > 0
    return np.where(pos, err / np.where(pos, bound, 1.0), np.where(err == 0, 0.0, np.inf))


def _regions(case, n):
    pre = cc.prefix_mask(n, case.lead, cc.tail_of(case), case.N, case.CP)
    k = np.arange(n)
    lead, tail = k < case.lead, k >= n - cc.tail_of(case)
    return (("lead-in", lead), ("body", ~(lead | tail | pre)), ("prefix", pre), ("tail", tail))


def test_fused_channel_equals_oracle(orc, run):
    case, iq = run.case, run.iq
    clean, ref = cc.reference(orc, case)
    assert iq.dtype == np.complex64 and iq.shape == ref.shape
    err = np.abs(iq.astype(np.complex128) - ref.astype(np.complex128))
    ratio = _ratio(err, cc.engine_bound(case.sigma, clean, ref))
    print("fused channel %s: worst error / bound %.4f (%s)" % (
        case.name, float(ratio.max()), ", ".join("%s %.4f" % (nm, float(ratio[m].max())) for nm, m in _regions(case, len(iq)))))
    bad = np.flatnonzero(ratio > 1.0)
    assert bad.size == 0, "%d samples beyond the bound, first at %d, worst %.3g of it" % (bad.size, bad[0], ratio.max())
    if case.sigma > 0:
        # lead-in and tail are noise of the right power, not silence
        for part in (iq[:case.lead], iq[len(iq) - cc.tail_of(case):]):
            assert 0.7 * case.sigma < np.sqrt(np.mean(np.abs(part) ** 2)) < 1.3 * case.sigma


def test_channel_off_equals_oracle_tx(orc, run):
    case, eng = run.case, run.eng
    try:
        eng.set_channel(enable=False)
        x = eng.tx(run.pay)
    finally:
        _arm(eng, case)
    assert np.array_equal(x, orc.tx(cc.cfg_of(case), run.pay))


def test_sc16_within_one_lsb_of_float_run(run):
    """The 16-bit kernels (k_tx_mod<N, *, sc16>, k_noise_sc16) store to_sc16 of what the float ones store, within the
    1 LSB of test_tx_sc16_channel_on, lead-in and tail included: with the float run pinned to the oracle, so are they."""
    case, eng = run.case, run.eng
    try:
        _arm(eng, case, fmt="sc16")
        q = eng.tx(run.pay)
    finally:
        _arm(eng, case)
    want = iqio.to_sc16(run.iq)
    assert q.dtype == np.int16 and q.shape == want.shape
    d = np.abs(q.astype(np.int32) - want.astype(np.int32))
    print("fused channel %s, sc16: %d of %d parts differ from to_sc16(float run), max %d LSB" % (
        case.name, int(np.count_nonzero(d)), d.size, int(d.max())))
    assert int(d.max()) <= 1
    if case.sigma > 0:
        assert np.any(q[:case.lead] != 0) and np.any(q[len(q) - cc.tail_of(case):] != 0)


LEAN_VS_FULL = [c for c in cc.CASES if c.cfo_bins == 0.0]              # (the N = 512 rows, and 64 and 4096 as well)


@pytest.mark.parametrize("case", LEAN_VS_FULL, ids=[c.name for c in LEAN_VS_FULL])
def test_lean_and_full_kernel_give_the_same_bits(case):
    """Without a carrier offset the launch rule picks LEAN; a transmit-side tap forces the full kernel.  The two
    instantiations share the noise path: same bits, float and 16-bit."""
    eng = engine.Engine(cfg=cc.cfg_of(case))
    pay = cc.payloads_of(case)
    out = {}
    for fmt in ("fc32", "sc16"):
        for taps in ((), (_abi.TAP_TX_FREQ,)):
            _arm(eng, case, fmt=fmt, taps=taps)
            out[fmt, len(taps)] = eng.tx(pay)
    eng.close()
    assert np.array_equal(out["fc32", 1], out["fc32", 0]) and np.any(out["fc32", 0][:case.lead] != 0)
    assert np.array_equal(out["sc16", 1], out["sc16", 0])


def test_device_mode_equals_host_mode():
    """tx_device(wait=False) then wait(): the bytes of the host-mode run, float and 16-bit."""
    import torch
    dev = torch.device("cuda:0")
    case = cc.CASES[cc.IDS.index("n512_paired_cfo")]
    pay = cc.payloads_of(case)
    blob, offs, lens = pack_payloads(pay)
    eh = engine.Engine(cfg=cc.cfg_of(case))
    ed = engine.Engine(cfg=cc.cfg_of(case, device_ptrs=True))
    d_blob = torch.from_numpy(blob.copy()).to(dev)
    for fmt in ("fc32", "sc16"):
        _arm(eh, case, fmt=fmt)
        _arm(ed, case, fmt=fmt)
        host = eh.tx(pay)
        _, nsamp = ed.tx_frame_count(lens)
        assert nsamp == len(host)
        d_out = torch.zeros(nsamp * (4 if fmt == "sc16" else 8), dtype=torch.uint8, device=dev)
        n = ed.tx_device(d_blob.data_ptr(), offs, lens, d_out.data_ptr(), nsamp, wait=False)
        ed.wait()
        assert n == nsamp
        assert d_out.cpu().numpy().tobytes() == host.tobytes(), fmt
    eh.close()
    ed.close()


# ---- the stand-alone call ----------------------------------------------------------------------------------------------
def test_standalone_channel_edges(orc):
    """ofdm_channel on more samples than k_channel has threads (the grid-stride loop wraps) from an odd stream index
    beyond 2^33 (the pair counter's high word is non-zero), rotation and noise; then one sample, then none."""
    s = cc.STANDALONE
    kw = dict(sigma=s["sigma"], cfo=s["cfo"], seed=s["seed"], stream_id=s["stream_id"], index0=s["index0"])
    x = cc.ramp(s["n"])
    assert len(x) > 2048 * 256 and s["index0"] & 1 and (s["index0"] >> 1) >> 32
    eng = engine.Engine(cfg=cc.cfg_of(cc.CASES[1]))
    for n in (len(x), 1, 0):
        xin = x[:n]
        got = eng.channel(xin, **kw)
        ref = orc.channel(xin.copy(), **kw)
        assert got.dtype == np.complex64 and got.shape == ref.shape == (n,)
        if n == 0:
            continue
        ratio = _ratio(np.abs(got.astype(np.complex128) - ref.astype(np.complex128)), cc.engine_bound(s["sigma"], xin, ref))
        print("stand-alone channel, n = %d from index %d: worst error / bound %.4f" % (n, s["index0"], float(ratio.max())))
        bad = np.flatnonzero(ratio > 1.0)
        assert bad.size == 0, "%d samples beyond the bound, first at %d, worst %.3g of it" % (bad.size, bad[0], ratio.max())
        assert not np.array_equal(got, xin)
    eng.close()
