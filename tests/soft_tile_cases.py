"""Captures that take k_soft_demap (csrc/rx_soft.h) where the captures of test_gpu_soft.py do not go, shared by
test_soft_tile_cases_host.py (the oracle alone: every capture delivers what it is for, and the store shapes counted
here are all reached) and test_gpu_soft_tiles.py (the kernel against the model of soft_cases.py).

The kernel walks a packet's carriers in tiles of 256 (SOFT_TILE_CARRIERS), B = 32 * nbits frame bytes each, and stores
the packet's part of a tile as 8-byte groups: an 8-byte head where the destination is not 16-byte aligned, 16-byte
pairs, an 8-byte tail.  The values buffer is 16-byte aligned at its base and packet k's values begin at 8 * (payload
offset of k), so the head is decided by the parity of (payload offset + first message byte of the tile) and is known
on the CPU.  soft_tile() and store_split() restate csrc/soft_plan.h and the tail of the kernel's tile loop.

    tile grid   N 64 / occ 48 / CP 16 (nmap 46), one capture per constellation of 1, 3, 3, 6 and 8 bits: packets that
                end on, one byte past and one byte short of a tile end, packets of two, three and more tiles at both
                offset parities, a chained packet of more than three tiles, and for BPSK the longest packet the framing
                takes (128 tiles)
    map widths  nmap 254, 256, 258, 598, 2398: dc = 2 and ds = 1, dc = 0, ds = 0 with a wrap on nearly every step

No GPU and no engine here.  Captures are computed once and are read-only."""
import collections
import functools

import numpy as np

import fec_cases as fc
import soft_cases as sc
from helpers import make_cfg

TILE_CARRIERS = 256          # csrc/soft_plan.h SOFT_TILE_CARRIERS
HEADER = sc.HEADER
MAX_PAYLOAD = 4091           # the framing's longest payload: the header carries len + 4 in 12 bits

Tile = collections.namedtuple("Tile", "byte0 nbytes lo hi out0")
Store = collections.namedtuple("Store", "first head n16 tail n8 full")


# ---- the tile arithmetic, restated -------------------------------------------------------------------------------------
def soft_tile(first, nbits, plen):
    """csrc/soft_plan.h soft_tile: the tile that begins at carrier ``first`` (a multiple of 256) of the chain."""
    byte0 = (first * nbits) >> 3
    nbytes = (TILE_CARRIERS // 8) * nbits
    m0, m1 = HEADER, HEADER + plen
    a, e = max(byte0, m0), min(byte0 + nbytes, m1)
    if a >= e:
        return Tile(byte0, nbytes, 0, 0, 0)
    return Tile(byte0, nbytes, 8 * (a - byte0), 8 * (e - byte0), 8 * (a - m0))


def tiles_of(plen, nbits):
    """The tiles the kernel's loop walks for a packet of plen payload bytes, in order."""
    return [soft_tile(t0, nbits, plen) for t0 in range(0, sc.carriers_needed(plen, nbits), TILE_CARRIERS)]


def store_split(boff, tile):
    """(head, n16, tail) of the tile's store: 8-byte groups n8 = head + 2 * n16 + tail, or None where the tile holds
    nothing of the packet.  ``boff``: the packet's payload offset in bytes."""
    if tile.hi <= tile.lo:
        return None
    n8 = (tile.hi - tile.lo) >> 3
    head = min((boff + tile.out0 // 8) & 1, n8)
    n16 = (n8 - head) >> 1
    return head, n16, n8 - head - 2 * n16


def packet_stores(boff, plen, nbits):
    """One Store per tile of the packet that stores something.  ``full``: the packet ends exactly on this tile's end."""
    out = []
    for k, t in enumerate(tiles_of(plen, nbits)):
        s = store_split(boff, t)
        if s is not None:
            out.append(Store(k == 0, s[0], s[1], s[2], (t.hi - t.lo) >> 3, t.hi == 8 * t.nbytes and t.byte0 + t.nbytes == HEADER + plen))
    return out


def call_stores(lens, nbits):
    """The Stores of a call's delivered packets (payload lengths in delivery order: the payloads lie back to back)."""
    out, boff = [], 0
    for n in lens:
        out += packet_stores(boff, n, nbits)
        boff += n
    return out


def shape_set(lens, nbits):
    """{(first_tile, head, n16 > 0, tail)} over the tiles of a call's delivered packets."""
    return {(s.first, s.head, s.n16 > 0, s.tail) for s in call_stores(lens, nbits)}


def ntiles(plen, nbits):
    return len(tiles_of(plen, nbits))


# Every (first_tile, head, n16 > 0, tail) but two: a tile that stores anything has n8 >= 1, so head = 0, n16 = 0, tail = 0
# does not exist, on the first tile or behind it.
IMPOSSIBLE_SHAPES = {(True, 0, False, 0), (False, 0, False, 0)}
ALL_SHAPES = {(f, h, p, t) for f in (True, False) for h in (0, 1) for p in (False, True) for t in (0, 1)} - IMPOSSIBLE_SHAPES


# ---- captures ----------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "name cfg nmap nbits sent lens cut x")


def _orc():
    from oracle import oracle
    oracle.lib()
    return oracle


def body(n, rng):
    """n bytes: a coded block where n is a block's length (test_gpu_soft._body), so that the decoder has work"""
    if fc.is_block(n):
        return fc.encode(rng.integers(0, 256, (n - 10) // 2, dtype=np.uint8).tobytes())
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def nbits_of(cfg):
    return int(cfg.arity).bit_length() - 1


# name -> (mod, noise SNR in dB of test_gpu_soft.GEOMS for the constellation, payload seed, noise seed, longest packet too).
# At N = 64 the oracle's receiver loses or fails single packets of a back-to-back burst depending on the bytes around them
# (test_gpu_punct.py has the same remark); the seeds are the first of a search (payload seed + 10 k, noise seed 950 .. 961)
# at which it delivers every packet -- test_soft_tile_cases_host.py keeps that true.
TILE_GRID = collections.OrderedDict([
    ("bpsk", ("bpsk", 30.0, 300, 950, True)),
    ("8psk", ("8psk", 30.0, 301, 950, False)),
    ("qam8", ("qam8", 30.0, 302, 953, False)),
    ("qam64", ("qam64", 36.0, 523, 961, False)),
    ("qam256", ("qam256", 55.0, 304, 950, False)),
])
TILE_N, TILE_OCC, TILE_CP, TILE_NMAP = 64, 48, 16, 46


def tile_lens(nbits, longest=False):
    """(sent payload lengths, index of the cut packet).  B = 32 * nbits frame bytes per tile, the first four of the first
    tile the header; B is even, so every tile of a packet has the parity of the packet's payload offset.  (o) / (e): the
    packet begins at an odd / even offset.
        1 (e), 0         the offset shift in front
        B - 4 (o)        ends on the first tile's end
        B - 5 (o)        one byte short of it: an odd number of groups behind a head
        B - 3 (e)        one byte past it: a second tile of one group, stored as a tail
        2B - 4 (o)       ends on the second tile's end: a full tile behind a head
        3B - 3 (o)       a third tile of one group, stored as a head
        3B + 11 (e)      more than three tiles, odd length: full tiles and an odd last one without a head
        3B + 40 (o)      more than three tiles, even length
        2 (o), 2B - 2 (o)   head + tail and nothing between, on the first tile and on a later one
        1 (o)            a first tile that is a head only
        B - 5 (e)        an odd number of groups without a head
        2B + 1 (o)       an odd last tile behind a head
    The cut packet (3B + 6, more than three tiles) loses its last two symbols, chains into the next packet's preamble
    and swallows that packet; one more packet behind it."""
    B = 32 * nbits
    front = [1, 0, B - 4, B - 5, B - 3, 2 * B - 4, 3 * B - 3, 3 * B + 11, 3 * B + 40, 2, 2 * B - 2, 1, B - 5, 2 * B + 1]
    if longest:
        front.append(MAX_PAYLOAD)
    cut = 3 * B + 6
    return front + [cut, 20, 30], len(front)


@functools.lru_cache(maxsize=None)
def tile_case(name):
    mod, snr, pseed, nseed, longest = TILE_GRID[name]
    cfg = make_cfg(mod, TILE_N, TILE_OCC, TILE_CP)
    orc = _orc()
    N, L = cfg.fft_length, cfg.fft_length + cfg.cp_length
    nbits, nmap = nbits_of(cfg), len(sc.smap_of(cfg))
    assert nmap == TILE_NMAP
    sent, k = tile_lens(nbits, longest)
    rng = np.random.default_rng(pseed)
    pay = [body(n, rng) for n in sent]
    a, b, c = orc.tx(cfg, pay[:k]), orc.tx(cfg, pay[k:k + 1]), orc.tx(cfg, pay[k + 1:])
    x = np.concatenate([np.zeros(2 * N, np.complex64), a, b[:len(b) - 2 * L], c, np.zeros(L + 2 * N, np.complex64)])
    psig = float(np.mean(np.abs(a) ** 2))
    orc.channel(x, sigma=float(np.sqrt(psig / 10 ** (snr / 10.0))), seed=nseed)
    x.setflags(write=False)
    lens = tuple(sent[:k + 1] + sent[k + 2:])                 # delivered: all but the swallowed one
    return Case(name, cfg, nmap, nbits, tuple(pay), lens, k, x)


# name -> (mod, N, occ, CP, carriers, nmap, payload lengths, noise SNR in dB, payload seed, noise seed).  The default map
# (FE7F) drops two carriers and the sink's map exists only where occ is a multiple of four, so nmap = 256 is not to be had
# from it: F66F drops four of occ = 260.  (qam256-258: the first noise seed from 960 up at which the oracle returns the
# empty packet with its length; the others took their first.)
_WIDE_LENS = (0, 1, 37, 301, 700, 1000)
WIDTH_GRID = collections.OrderedDict([
    ("qam16-254", ("qam16", 512, 256, 32, None, 254, _WIDE_LENS, 30.0, 310, 960)),
    ("8psk-256", ("8psk", 512, 260, 32, "F66F", 256, _WIDE_LENS, 30.0, 311, 961)),
    ("qam256-258", ("qam256", 512, 260, 32, None, 258, _WIDE_LENS, 55.0, 312, 966)),
    ("qam64-598", ("qam64", 1024, 600, 64, None, 598, _WIDE_LENS, 36.0, 313, 963)),
    ("qpsk-2398", ("qpsk", 4096, 2400, 1024, None, 2398, (0, 37, 700), 30.0, 314, 964)),
])


@functools.lru_cache(maxsize=None)
def width_case(name):
    mod, N, occ, CP, carriers, nmap, sent, snr, pseed, nseed = WIDTH_GRID[name]
    cfg = make_cfg(mod, N, occ, CP, **({"carriers": carriers} if carriers else {}))
    orc = _orc()
    assert len(sc.smap_of(cfg)) == nmap, (len(sc.smap_of(cfg)), nmap)
    rng = np.random.default_rng(pseed)
    pay = [body(n, rng) for n in sent]
    a = orc.tx(cfg, pay)
    x = np.concatenate([np.zeros(2 * N, np.complex64), a, np.zeros(N + CP + 2 * N, np.complex64)])
    psig = float(np.mean(np.abs(a) ** 2))
    orc.channel(x, sigma=float(np.sqrt(psig / 10 ** (snr / 10.0))), seed=nseed)
    x.setflags(write=False)
    return Case(name, cfg, nmap, nbits_of(cfg), tuple(pay), tuple(sent), None, x)


def case(name):
    return tile_case(name) if name in TILE_GRID else width_case(name)


ALL_CASES = tuple(TILE_GRID) + tuple(WIDTH_GRID)


def longest_cut(c):
    """A sample in the middle of the capture's longest packet (where the stream test cuts)."""
    orc = _orc()
    pos = 2 * c.cfg.fft_length
    best = (0, 0)
    for i, p in enumerate(c.sent):
        n = len(orc.tx(c.cfg, [p]))
        if c.cut is not None and i == c.cut:
            n -= 2 * (c.cfg.fft_length + c.cfg.cp_length)
        if n > best[0]:
            best = (n, pos + n // 2)
        pos += n
    assert pos + 3 * c.cfg.fft_length + c.cfg.cp_length == len(c.x)
    return best[1]
