"""The captures of soft_tile_cases.py on the oracle alone: each delivers the packets it was built for, the store shapes
counted from their lengths are every shape the kernel's store skeleton has, and the model of soft_cases.py on the
oracle's own taps gives decisions with the sign of the delivered bits.  These are conditions on the captures, kept here
so that test_gpu_soft_tiles.py can rely on them; no GPU and no engine.

The restated tile arithmetic is held against csrc/soft_plan.h itself through a small program built from the header."""
import functools
import os
import subprocess

import numpy as np
import pytest

import soft_cases as sc
import soft_tile_cases as tc
from ofdm_uhd_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASK = (1 << _abi.TAP_RX_FFT) | (1 << _abi.TAP_RX_SINK) | (1 << _abi.TAP_RX_FRAMES)


@functools.lru_cache(maxsize=None)
def oracle_run(name):
    c = tc.case(name)
    from oracle import oracle
    return c, oracle.rx(c.cfg, c.x, MASK)


def oracle_values(c, ro):
    """The model on the oracle's taps.  Every flag of these captures is a sent packet's (the capture's tail may raise one
    more); delivered packet k is the k-th frame, the swallowed packet's frame left out.  Its preamble is row
    sum(1 + symbols emitted by the frames before) of TAP_RX_FFT, hinv formed from it as soft_cases.hinv_from_preamble
    does; its sink rows follow those of the packet before, ceil(8 (4 + len + 4) / (nmap nbits)) of them."""
    frames, fft, sink = ro.tap(_abi.TAP_RX_FRAMES), ro.tap(_abi.TAP_RX_FFT), ro.tap(_abi.TAP_RX_SINK)
    assert len(c.sent) <= len(frames) <= len(c.sent) + 1
    pre = np.concatenate([[0], np.cumsum(frames[:, 1].astype(np.int64) + 1)])
    assert pre[-1] == len(fft)
    idx = [j for j in range(len(c.sent)) if c.cut is None or j != c.cut + 1]
    smap, cst, mask = sc.smap_of(c.cfg), sc.cst_of(c.cfg), sc.mask_of(c.cfg)
    row, out = 0, []
    for j, (ok, p) in zip(idx, ro.packets):
        ns = -(-8 * (sc.HEADER + len(p) + 4) // (c.nmap * c.nbits))
        eq = sc.hinv_from_preamble(c.cfg, fft[pre[j]])
        out.append(sc.packet_values(sink[row:row + ns, :c.nmap], eq, smap, cst, len(p), mask))
        row += ns
    assert row <= len(sink) <= row + 2          # (the tail's flag, where there is one, demaps a symbol or two of noise)
    return out


@pytest.mark.parametrize("name", tc.ALL_CASES)
def test_the_oracle_delivers_every_packet(name):
    c, ro = oracle_run(name)
    pk = list(ro.packets)
    assert [len(p) for _, p in pk] == list(c.lens)
    assert c.nmap == len(sc.smap_of(c.cfg))
    ok = [o for o, _ in pk]
    want = list(c.sent)
    if c.cut is not None:
        # the cut packet came back CRC-failed, its chain took the next packet's preamble, and that packet is gone
        assert not ok[c.cut] and ro.stats["chained_frames"] == 1
        assert tc.ntiles(c.lens[c.cut], c.nbits) >= 3
        del want[c.cut + 1]
        del ok[c.cut], want[c.cut], pk[c.cut]
    assert len(want) == len(pk)
    assert all(p == w for (o, p), w in zip(pk, want) if o)
    if name == "qam256":
        # 256-QAM at N = 64 fails CRCs of a back-to-back burst at any noise level: delivery and length only
        assert sum(ok) >= 4
    else:
        assert all(ok)


def test_the_longest_packet_walks_128_tiles():
    c = tc.case("bpsk")
    assert max(c.lens) == tc.MAX_PAYLOAD and tc.ntiles(tc.MAX_PAYLOAD, 1) == 128
    with pytest.raises(ValueError):
        from oracle import oracle
        oracle.tx(c.cfg, [bytes(tc.MAX_PAYLOAD + 1)])


def test_map_widths():
    """dc = 2 with ds = 1, dc = 0, and ds = 0 (a tile is part of one symbol; nmap 598: the column wraps on every second
    or third tile, 2398: on every ninth or tenth)."""
    got = {name: (tc.case(name).nmap, tc.TILE_CARRIERS // tc.case(name).nmap, tc.TILE_CARRIERS % tc.case(name).nmap)
           for name in tc.WIDTH_GRID}
    assert got == {"qam16-254": (254, 1, 2), "8psk-256": (256, 1, 0), "qam256-258": (258, 0, 256), "qam64-598": (598, 0, 256),
                   "qpsk-2398": (2398, 0, 256)}
    for name in tc.WIDTH_GRID:
        c = tc.case(name)
        assert max(tc.ntiles(n, c.nbits) for n in c.lens) >= 3
        # the longest packet spans several symbols, so the column wraps inside it
        assert sc.carriers_needed(max(c.lens), c.nbits) > c.nmap


def test_every_store_shape_is_reached():
    union = set()
    for name in tc.TILE_GRID:
        c = tc.case(name)
        union |= tc.shape_set(c.lens, c.nbits)
    assert len(tc.ALL_SHAPES) == 14 and union == tc.ALL_SHAPES
    assert not union & tc.IMPOSSIBLE_SHAPES


@pytest.mark.parametrize("name", ["8psk", "qam8", "qam64", "qam256"])
def test_the_straddling_constellations_reach_the_edges(name):
    """3, 6 and 8 bits per carrier, each on its own: both head values behind the first tile, a packet that ends exactly on
    a tile's end (first tile and a later one), a later tile of one group at both parities, a packet one byte short of a
    tile's end, and every shape."""
    c = tc.case(name)
    st = tc.call_stores(c.lens, c.nbits)
    later = [s for s in st if not s.first]
    assert {s.head for s in later} == {0, 1}
    assert any(s.full and s.first for s in st) and any(s.full and not s.first for s in st)
    assert {s.head for s in later if s.n8 == 1} == {0, 1}
    B = 32 * c.nbits
    assert B - 5 in c.lens and B - 4 in c.lens and B - 3 in c.lens
    assert tc.shape_set(c.lens, c.nbits) == tc.ALL_SHAPES
    assert max(tc.ntiles(n, c.nbits) for n in c.lens) == 4
    # multi-tile packets begin at both offset parities
    off = np.concatenate([[0], np.cumsum(c.lens)])[:-1]
    assert {int(o) & 1 for o, n in zip(off, c.lens) if tc.ntiles(n, c.nbits) >= 3} == {0, 1}


@pytest.mark.parametrize("name", tc.ALL_CASES)
def test_the_model_on_the_oracles_taps_gives_the_delivered_bits(name):
    """v != 0 implies (v > 0) == bit on every CRC-ok packet, and none of its values is 0."""
    c, ro = oracle_run(name)
    vals = oracle_values(c, ro)
    assert len(vals) == len(ro.packets)
    nok = 0
    for (ok, p), v in zip(ro.packets, vals):
        assert len(v) == 8 * len(p)
        if not ok:
            continue
        nok += 1
        assert np.all(v != 0)
        assert np.array_equal(v > 0, sc.hard_bits(p).astype(bool))
    assert nok >= 3


def test_tiles_cover_each_packet_once_and_agree_with_the_placement():
    for nbits in (1, 2, 3, 4, 6, 8):
        for plen in (1, 2, 32 * nbits - 5, 32 * nbits - 4, 32 * nbits - 3, 64 * nbits - 4, 96 * nbits - 3, 1000):
            nxt = 0
            for t in tc.tiles_of(plen, nbits):
                if t.hi > t.lo:
                    assert t.out0 == nxt and t.lo % 8 == 0 and t.hi % 8 == 0
                    nxt += t.hi - t.lo
            assert nxt == 8 * plen
            for boff in (0, 1):
                for s in tc.packet_stores(boff, plen, nbits):
                    assert s.n8 == s.head + 2 * s.n16 + s.tail and s.head <= 1 and s.tail <= 1


PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include "soft_plan.h"
int main(int argc, char** argv) {
  for (int i = 1; i + 1 < argc; i += 2) {
    const uint32_t nbits = (uint32_t)atoi(argv[i]), plen = (uint32_t)atoi(argv[i + 1]);
    for (uint64_t t0 = 0; t0 < soft_carriers(plen, nbits); t0 += SOFT_TILE_CARRIERS) {
      const SoftTile t = soft_tile(t0, nbits, plen);
      printf("%u %u %llu %u %u %u %llu\n", nbits, plen, (unsigned long long)t.byte0, t.nbytes, t.lo, t.hi, (unsigned long long)t.out0);
    }
  }
  return 0;
}
"""


def test_the_restated_tiles_are_those_of_the_header(tmp_path):
    src, exe = tmp_path / "tiles.cpp", str(tmp_path / "tiles")
    src.write_text(PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "ofdm_uhd_amd", "csrc"), "-o", exe, str(src)])
    pairs = sorted({(tc.case(name).nbits, n) for name in tc.ALL_CASES for n in tc.case(name).lens})
    out = subprocess.check_output([exe] + [str(v) for p in pairs for v in p]).decode().split("\n")
    got = [tuple(int(v) for v in line.split()) for line in out if line]
    want = [(nbits, plen) + tuple(t) for nbits, plen in pairs for t in tc.tiles_of(plen, nbits)]
    assert got == want and len(want) > 300
