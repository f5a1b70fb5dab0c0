"""Per-packet link quality (ofdm_set_rx_quality / ofdm_rx_quality): the entry points exist and the record layout the C
compiler sees is the one ctypes and NumPy read.  No compute calls here (no GPU needed)."""
import ctypes
import os
import subprocess

import numpy as np

from ofdm_uhd_amd import _abi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_quality_entry_points_exported():
    lib = _abi.load()
    for name in ("ofdm_set_rx_quality", "ofdm_rx_quality"):
        assert name in _abi.EXPORTS
        assert hasattr(lib, name), name
    assert lib.ofdm_abi_version() == _abi.OFDM_ABI_VERSION == 6


def test_quality_calls_refuse_a_null_handle():
    lib = _abi.load()
    n = ctypes.c_int(-1)
    assert lib.ofdm_set_rx_quality(None, 1) == _abi.OFDM_E_INVAL
    assert lib.ofdm_rx_quality(None, None, 0, ctypes.byref(n)) == _abi.OFDM_E_INVAL


def test_quality_record_layout_matches_header(tmp_path):
    """sizeof / offsetof of ofdm_pkt_quality as gcc compiles include/ofdm_hip.h == the ctypes mirror == the NumPy dtype
    Engine.rx_quality returns."""
    st = _abi.ofdm_pkt_quality
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ofdm_hip.h"', 'int main(void){',
             'printf("size %zu\\n", sizeof(ofdm_pkt_quality));']
    for f, _ in st._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(ofdm_pkt_quality, %s));' % (f, f))
    lines.append('return 0;}')
    src = tmp_path / "q.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "q")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)])
    got = dict(l.split() for l in subprocess.check_output([exe]).decode().splitlines())
    assert int(got["size"]) == ctypes.sizeof(st) == 56
    dt = engine.QUALITY_DTYPE
    assert dt.itemsize == ctypes.sizeof(st)
    assert list(dt.names) == [f for f, _ in st._fields_]
    for f, ct in st._fields_:
        assert int(got[f]) == getattr(st, f).offset == dt.fields[f][1], f
        assert dt.fields[f][0].itemsize == ctypes.sizeof(ct), f
    assert dt.fields["flag"][0] == np.uint64 and dt.fields["coarse"][0] == np.int32
    assert dt.fields["cfo_bins"][0] == np.float32
