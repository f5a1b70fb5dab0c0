"""16-bit IQ (sc16) on the host side: the normative conversions of iqio, the sc16 file source / sink, the C ABI's
setters without a handle, the three command lines -- and the oracle on quantised captures: quantising a capture to
16 bits does not change what the reference receiver delivers, which is what keeps the GPU tests of
test_gpu_iq_format.py (engine and oracle on the SAME quantised array) about the link and not about the rounding."""
import numpy as np
import pytest

from helpers import loopback_stream, make_cfg, make_payloads
from ofdm_uhd_amd import _abi, iqio

# (copied from test_gpu_parity.CASES) mod, N, occ, CP, payload, packets, snr, cfo(bins)
CASES = [
    ("qpsk", 512, 200, 128, 1026, 6, 30.0, 0.0),
    ("bpsk", 512, 200, 128, 300, 5, 30.0, 0.05),
    ("qpsk", 512, 200, 128, 1026, 6, 30.0, 0.3),
    ("8psk", 256, 120, 64, 500, 4, 30.0, 0.0),
    ("qam16", 2048, 1200, 512, 4091, 3, 30.0, 0.0),
    ("qam64", 1024, 600, 256, 2000, 3, 36.0, 0.1),
    ("qam64", 4096, 2400, 1024, 4091, 3, 36.0, 0.0),
    ("qam256", 64, 48, 16, 100, 4, 55.0, 0.0),
    ("bpsk", 128, 64, 32, 64, 4, 30.0, 0.0),
    ("qpsk", 512, 200, 128, 1026, 4, 30.0, 1.3),
    ("qpsk", 512, 200, 128, 1026, 4, 30.0, -2.4),
]


def _c(re, im=0.0):
    return np.array([complex(re, im)], np.complex64)


def test_to_sc16_rounds_half_to_even():
    # in LSBs (scale 1): 0.5 -> 0, 1.5 -> 2, -2.5 -> -2, and the ordinary cases around them
    x = np.array([0.5 + 1.5j, -2.5 + 2.5j, -0.5 - 1.5j, 0.49 + 0.51j, 3.5 - 3.5j], np.complex64)
    assert iqio.to_sc16(x, 1.0).tolist() == [[0, 2], [-2, 2], [0, -2], [0, 1], [4, -4]]
    # the same ties through the default scale 2^15 (the products are exact)
    assert iqio.to_sc16(x / np.float32(32768.0)).tolist() == [[0, 2], [-2, 2], [0, -2], [0, 1], [4, -4]]


def test_to_sc16_saturates_and_drops_nan():
    x = np.array([1.0 - 1.0j, 0.99999 - 0.99999j, 7.0 - 7.0j, complex(np.inf, -np.inf), complex(np.nan, 0.25),
                  complex(0.25, np.nan)], np.complex64)
    q = iqio.to_sc16(x)
    assert q.dtype == np.int16 and q.shape == (6, 2)
    assert q.tolist() == [[32767, -32768], [32767, -32768], [32767, -32768], [32767, -32768], [0, 8192], [8192, 0]]
    assert iqio.to_sc16(_c(32767.4, -32768.4), 1.0).tolist() == [[32767, -32768]]
    assert iqio.to_sc16(_c(32767.6, -32768.6), 1.0).tolist() == [[32767, -32768]]


def test_non_power_of_two_scale_is_one_float32_multiply():
    rng = np.random.default_rng(5)
    x = (rng.uniform(-1, 1, 4096) + 1j * rng.uniform(-1, 1, 4096)).astype(np.complex64)
    s = 32767.0
    q = iqio.to_sc16(x, s)
    parts = x.view(np.float32)
    want = np.clip(np.rint(parts * np.float32(s)), -32768, 32767).astype(np.int16).reshape(-1, 2)   # float32 product
    assert np.array_equal(q, want)
    back = iqio.from_sc16(q, 1.0 / s)
    assert back.dtype == np.complex64
    assert np.array_equal(back.view(np.float32), q.reshape(-1).astype(np.float32) * np.float32(1.0 / s))
    for bad in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError):
            iqio.to_sc16(x, bad)
        with pytest.raises(ValueError):
            iqio.from_sc16(q, bad)


@pytest.mark.parametrize("s", [2.0 ** 15, 32767.0, 1000.0])
def test_round_trip_within_half_an_lsb(s):
    rng = np.random.default_rng(6)
    lim = 32767.0 / s * 0.999                       # inside full scale
    x = (rng.uniform(-lim, lim, 20000) + 1j * rng.uniform(-lim, lim, 20000)).astype(np.complex64)
    y = iqio.from_sc16(iqio.to_sc16(x, s), 1.0 / s)
    err = np.abs((y.view(np.float32).astype(np.float64) - x.view(np.float32).astype(np.float64)) * s)
    if s == 2.0 ** 15:
        # the default scales are powers of two: both products are exact, the only error is the rounding to the grid
        assert err.max() <= 0.5
    else:
        # half an LSB, plus the float32 roundings of the two products and of 1/s (each below 2^-23 relative, of values
        # up to 2^15 LSB: 2^-7 LSB with margin)
        assert err.max() <= 0.5 + 2.0 ** -7
    # the defaults are exact powers of two: the quantised grid comes back exactly
    q = iqio.to_sc16(x / np.float32(lim * s / 32767.0))
    assert np.array_equal(iqio.to_sc16(iqio.from_sc16(q)), q)


def test_sc16_arrays_are_never_reinterpreted():
    q = np.arange(12, dtype=np.int16)
    assert iqio.as_sc16(q).shape == (6, 2) and iqio.as_sc16(q.reshape(6, 2)).shape == (6, 2)
    for bad in (np.zeros(4, np.complex64), np.zeros(4, np.float32), np.zeros(4, np.int32), np.zeros(5, np.int16),
                np.zeros((2, 3), np.int16)):
        with pytest.raises(ValueError):
            iqio.as_sc16(bad)
    assert np.array_equal(iqio.from_sc16(q, 1.0), np.array([0 + 1j, 2 + 3j, 4 + 5j, 6 + 7j, 8 + 9j, 10 + 11j], np.complex64))


def test_file_sink_source_round_trip(tmp_path):
    rng = np.random.default_rng(7)
    q = rng.integers(-32768, 32768, (10007, 2)).astype(np.int16)
    fn = str(tmp_path / "cap.sc16")
    sink = iqio.file_sink(fn, fmt="sc16")
    sink.write(q[:4000])
    sink.write(q[4000:].reshape(-1))                 # flat 2n accepted
    sink.close()
    raw = open(fn, "rb").read()
    assert len(raw) == 4 * len(q)
    # byte layout: little-endian I, Q int16
    assert raw[:8] == b"".join(int(v).to_bytes(2, "little", signed=True) for v in q[:2].reshape(-1))
    src = iqio.file_source(fn, fmt="sc16")
    a = src.read_all()
    assert a.dtype == np.int16 and a.shape == q.shape and np.array_equal(a, q)
    assert np.array_equal(iqio.read_short_binary(fn, count=10, offset_samples=3), q[3:13])
    pieces = list(src.read_chunks(3000))            # 3000 does not divide 10007: chunks count SAMPLES
    assert [len(p) for p in pieces] == [3000, 3000, 3000, 1007]
    assert all(p.dtype == np.int16 and p.shape[1] == 2 for p in pieces)
    assert np.array_equal(np.concatenate(pieces), q)
    # append mode, and the float format is what it was
    s2 = iqio.file_sink(fn, append=True, fmt="sc16")
    s2.write(q[:5])
    s2.close()
    assert np.array_equal(iqio.file_source(fn, fmt="sc16").read_all(), np.concatenate([q, q[:5]]))
    x = (rng.standard_normal(1001) + 1j * rng.standard_normal(1001)).astype(np.complex64)
    fn2 = str(tmp_path / "cap.fc32")
    s3 = iqio.file_sink(fn2)
    s3.write(x)
    s3.close()
    assert np.array_equal(iqio.file_source(fn2).read_all(), x)
    assert [len(p) for p in iqio.file_source(fn2).read_chunks(400)] == [400, 400, 201]
    with pytest.raises(ValueError):
        iqio.file_sink(fn2, fmt="sc8")
    with pytest.raises(ValueError):
        iqio.file_source(fn2, fmt="sc12")
    s4 = iqio.file_sink(fn2)
    with pytest.raises(ValueError):
        s4.write(q)                                   # int16 into a float file: refused, not converted silently
    s4.close()
    s5 = iqio.file_sink(fn, fmt="sc16")
    with pytest.raises(ValueError):
        s5.write(x)
    s5.close()


def test_vector_source_and_sink_keep_their_dtype():
    q = np.arange(40, dtype=np.int16).reshape(20, 2)
    vs = iqio.vector_source(q)
    assert vs.read_all().dtype == np.int16
    assert [p.shape for p in vs.read_chunks(8)] == [(8, 2), (8, 2), (4, 2)]
    sink = iqio.vector_sink()
    for p in vs.read_chunks(8):
        sink.write(p)
    assert sink.data().dtype == np.int16 and np.array_equal(sink.data(), q)
    x = np.arange(10).astype(np.complex64)
    fs = iqio.vector_sink()
    fs.write(x)
    assert fs.data().dtype == np.complex64 and np.array_equal(iqio.vector_source(x).read_all(), x)


def test_setters_without_a_handle():
    lib = _abi.load()
    assert lib.ofdm_abi_version() == _abi.OFDM_ABI_VERSION
    assert hasattr(lib, "ofdm_set_rx_iq_format") and hasattr(lib, "ofdm_set_tx_iq_format")
    assert lib.ofdm_set_rx_iq_format(None, _abi.OFDM_IQ_SC16, 2.0 ** -15) == _abi.OFDM_E_INVAL
    assert lib.ofdm_set_tx_iq_format(None, _abi.OFDM_IQ_SC16, 2.0 ** 15) == _abi.OFDM_E_INVAL
    assert lib.ofdm_set_rx_iq_format(None, _abi.OFDM_IQ_FC32, 0.0) == _abi.OFDM_E_INVAL
    assert "ofdm_set_rx_iq_format" in _abi.EXPORTS and "ofdm_set_tx_iq_format" in _abi.EXPORTS
    import ctypes as C
    assert C.sizeof(_abi.ofdm_sc16) == 4 and (_abi.OFDM_IQ_FC32, _abi.OFDM_IQ_SC16) == (0, 1)


def test_command_line_options():
    from ofdm_uhd_amd import benchmark_ofdm_rx, benchmark_ofdm_tx, predictive_sense
    for mod in (benchmark_ofdm_rx, benchmark_ofdm_tx):
        o, _ = mod.make_parser().parse_args([])
        assert o.iq_format == "fc32" and o.iq_scale is None
        o, _ = mod.make_parser().parse_args(["--iq-format", "sc16", "--iq-scale", "32767"])
        assert o.iq_format == "sc16" and o.iq_scale == 32767.0
        with pytest.raises(SystemExit):
            mod.make_parser().parse_args(["--iq-format", "sc8"])
    s = predictive_sense.sensor([])
    assert s.options.iq_format == "fc32"
    s = predictive_sense.sensor(["--iq-format", "sc16", "--iq-scale", "1e-4"])
    assert s.options.iq_format == "sc16" and s.options.iq_scale == 1e-4


def test_predictive_sense_reads_an_sc16_file(tmp_path):
    from ofdm_uhd_amd import predictive_sense
    q = np.arange(2000, dtype=np.int16).reshape(-1, 2)
    fn = str(tmp_path / "s.sc16")
    k = iqio.file_sink(fn, fmt="sc16")
    k.write(q)
    k.close()
    s = predictive_sense.sensor(["-i", fn, "--iq-format", "sc16"])
    got = s._samples(None)
    assert got.dtype == np.int16 and np.array_equal(got, q)


@pytest.mark.parametrize("s", [2.0 ** 15, 32767.0])
@pytest.mark.parametrize("mod,N,occ,CP,plen,npkt,snr,cfo", CASES)
def test_oracle_on_quantised_capture(orc, mod, N, occ, CP, plen, npkt, snr, cfo, s):
    """The reference receiver on x and on x quantised to 16 bits at full scale s: no sample saturates, and it raises
    the same number of flags and delivers the same number of packets and CRC passes, every CRC-ok payload identical.
    (CRC-failed packets may carry other bytes: a packet already lost may differ.)"""
    cfg = make_cfg(mod, N, occ, CP)
    x = loopback_stream(orc, cfg, make_payloads(npkt, plen), snr_db=snr, cfo_bins=cfo)
    parts = x.view(np.float32)
    assert float(np.max(np.abs(parts))) * s < 32767.0          # to_sc16 saturates no sample
    q = iqio.to_sc16(x, s)
    assert int(np.max(q)) < 32767 and int(np.min(q)) > -32768
    xq = iqio.from_sc16(q, 1.0 / s)
    ra, rb = orc.rx(cfg, x), orc.rx(cfg, xq)
    for k in ("peaks", "packets", "crc_ok"):
        assert ra.stats[k] == rb.stats[k], k
    assert len(ra.packets) == len(rb.packets)
    assert [ok for ok, _ in ra.packets] == [ok for ok, _ in rb.packets]
    assert [p for ok, p in ra.packets if ok] == [p for ok, p in rb.packets if ok]
    assert ra.stats["crc_ok"] >= 1
