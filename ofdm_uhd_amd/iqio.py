"""IQ sample sources and sinks that stand in for the reference's UHD radio I/O
(usrp_transmit_path.py:66-72, usrp_receive_path.py:67-73).

File format = ``gr.file_sink(gr.sizeof_gr_complex, ...)`` / ``gr.file_source``:
raw little-endian interleaved float32 I,Q (ofdm.py:124-131;
utils/read_complex_binary.m:40-45), so captures move freely between this engine
and a real GNU Radio flow graph.

The second format is the one radios and most capture tools produce: ``sc16``, raw little-endian
interleaved int16 I,Q (UHD's rx_samples_to_file, utils/read_short_binary.m).  In Python an sc16
stream is an ``int16`` array of shape ``(n, 2)``; ``to_sc16`` / ``from_sc16`` are the normative
conversions, which the engine's kernels match bit for bit (include/ofdm_hip.h).
"""
import numpy as np

FORMATS = ("fc32", "sc16")
RX_SCALE = 2.0 ** -15   # default scale of from_sc16 / the engine's receive side
TX_SCALE = 2.0 ** 15    # default scale of to_sc16 / the engine's transmit side


def check_format(fmt):
    if fmt not in FORMATS:
        raise ValueError("IQ format must be one of %s, not %r" % (", ".join(FORMATS), fmt))
    return fmt


def check_scale(scale, default):
    scale = default if scale is None else float(scale)
    if not (np.isfinite(scale) and scale > 0):
        raise ValueError("IQ scale must be finite and positive")
    return scale


def as_sc16(a):
    """An int16 array of 2n entries (flat or (n, 2)) as a contiguous (n, 2) array; anything else is refused."""
    a = np.asarray(a)
    if a.dtype != np.int16:
        raise ValueError("sc16 samples must be an int16 array, not %s" % a.dtype)
    if a.ndim == 2 and a.shape[1] == 2:
        return np.ascontiguousarray(a)
    if a.ndim == 1 and a.size % 2 == 0:
        return np.ascontiguousarray(a).reshape(-1, 2)
    raise ValueError("sc16 samples must have shape (n, 2) or (2n,)")


def from_sc16(a, scale=None):
    """int16 I,Q pairs -> complex64: ``(float32)i * float32(scale)`` per part (one float32 multiply)."""
    a = as_sc16(a)
    scale = np.float32(check_scale(scale, RX_SCALE))
    return np.ascontiguousarray(a.astype(np.float32) * scale).view(np.complex64).reshape(-1)


def to_sc16(iq, scale=None):
    """complex64 -> int16 (n, 2): ``clamp(rint(x * float32(scale)), -32768, 32767)`` per part, one float32
    multiply, round half to even, NaN -> 0, clamped in float before the integer conversion."""
    iq = np.ascontiguousarray(iq, np.complex64).reshape(-1)
    scale = np.float32(check_scale(scale, TX_SCALE))
    with np.errstate(over="ignore", invalid="ignore"):
        x = iq.view(np.float32) * scale
    x = np.nan_to_num(x, nan=0.0, posinf=np.inf, neginf=-np.inf)
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16).reshape(-1, 2)


def _keep(iq):
    """The array in its own sample format: int16 stays sc16 (n, 2), everything else becomes complex64."""
    if np.asarray(iq).dtype == np.int16:
        return as_sc16(iq)
    return np.ascontiguousarray(iq, np.complex64)


class vector_sink(object):
    """Collects everything written to it (gr.vector_sink_c)."""

    def __init__(self):
        self._chunks = []

    def write(self, iq):
        self._chunks.append(_keep(iq))

    def data(self):
        if not self._chunks:
            return np.zeros(0, np.complex64)
        return np.concatenate(self._chunks)

    def close(self):
        pass


class file_sink(object):
    """gr.file_sink(gr.sizeof_gr_complex, filename); fmt="sc16": int16 samples as little-endian I,Q shorts."""

    def __init__(self, filename, append=False, fmt="fc32"):
        self.fmt = check_format(fmt)
        self._f = open(filename, "ab" if append else "wb")

    def write(self, iq):
        if self.fmt == "sc16":
            as_sc16(iq).astype("<i2", copy=False).tofile(self._f)
        else:
            if np.asarray(iq).dtype == np.int16:
                raise ValueError("int16 samples handed to an fc32 file_sink (convert with from_sc16, or open it with fmt=\"sc16\")")
            np.ascontiguousarray(iq, np.complex64).astype("<c8", copy=False).tofile(self._f)

    def close(self):
        if self._f:
            self._f.close()
            self._f = None


class null_sink(object):
    def write(self, iq):
        pass

    def close(self):
        pass


def read_complex_binary(filename, count=-1, offset_samples=0):
    """utils/read_complex_binary.m: interleaved float32 -> complex64."""
    return np.fromfile(filename, dtype="<c8", count=count, offset=8 * offset_samples).astype(np.complex64, copy=False)


def read_short_binary(filename, count=-1, offset_samples=0):
    """utils/read_short_binary.m for an IQ capture: interleaved int16 -> int16 (n, 2); count and offset in samples.
    A trailing half sample is dropped."""
    a = np.fromfile(filename, dtype="<i2", count=-1 if count < 0 else 2 * count, offset=4 * offset_samples)
    return a[:len(a) // 2 * 2].astype(np.int16, copy=False).reshape(-1, 2)


class file_source(object):
    """gr.file_source(gr.sizeof_gr_complex, filename, repeat) (predictive_sense.py:92); fmt="sc16": a file of
    little-endian I,Q shorts, read as int16 (n, 2)."""

    def __init__(self, filename, repeat=False, fmt="fc32"):
        self.filename = filename
        self.repeat = repeat
        self.fmt = check_format(fmt)
        self._read = read_short_binary if self.fmt == "sc16" else read_complex_binary

    def read_all(self):
        return self._read(self.filename)

    def read_chunks(self, chunk_samples):
        """The file in pieces of chunk_samples SAMPLES (the last one shorter), without loading it whole."""
        off = 0
        while True:
            a = self._read(self.filename, count=chunk_samples, offset_samples=off)
            if len(a) == 0:
                return
            yield a
            off += len(a)
            if len(a) < chunk_samples:
                return


class vector_source(object):
    def __init__(self, iq):
        self._iq = _keep(iq)

    def read_all(self):
        return self._iq

    def read_chunks(self, chunk_samples):
        for a in range(0, len(self._iq), chunk_samples):
            yield self._iq[a:a + chunk_samples]
