"""Outer code: the length arithmetic of the Reed-Solomon layer over the payload.

RS over GF(2^8) with 32 parity bytes per codeword (t = 16), byte-interleaved to the depth a payload needs, decoded on
the GPU (include/ofdm_hip.h, "outer code").  It sits above the coded links (``fec``) and corrects
the short bursts of wrong bytes a Viterbi decoder leaves; it also works on an uncoded link.  The code has no
parameters.  The work is ``Engine.rs_encode`` / ``Engine.rs_decode``; ``ofdm_mod(rs=True)`` and ``ofdm_demod(rs=True)``
put it on a link, both ends alike.

Decoding with reliabilities (``Engine.rs_decode_rel``, ``ofdm_demod(rs=dict(erasures=True))``): one byte per received
byte says how far to trust it, and a codeword that bounded-distance decoding fails is tried once more with its weakest
symbols, ``max_erasures`` at the most, erased.  ``rs_cfg`` makes the call's configuration, ``rel_from_values`` restates
on the host what ``Engine.rs_rel_from_soft`` computes on the GPU.  That is the source of reliabilities on an RS link
without an inner code.  On a concatenated link the source is the inner decoder itself
(``ofdm_demod(fec=..., rs=dict(erasures=True, source="fec"))``): the soft-output Viterbi decoder
(``Engine.fec_decode_rel`` / ``fec_decode_soft_rel`` / ``rx_fec_decode_soft_rel``) returns one reliability per decoded
byte, 0 .. 255, in the format ``Engine.rs_decode_rel`` takes, at the payloads' own offsets.
"""
import ctypes as C

import numpy as np

from . import _abi

PARITY = _abi.OFDM_RS_PARITY
MAX_PAYLOAD = _abi.OFDM_RS_MAX_PAYLOAD
MAX_CODED = _abi.OFDM_RS_MAX_CODED
MAX_PAYLOAD_UNDER_FEC = 1780          # the RS block must fit fec.MAX_PAYLOAD: W = 8, block 2040
MAX_PAYLOAD_UNDER_LDPC = 1752         # the RS block must fit ldpc.MAX_PAYLOAD: W = 8, block 2012
DEFAULT_MAX_ERASURES = 28             # leaves four parity symbols as a check on what the erasures fill in


def coded_len(payload_len):
    """Bytes of the RS block of a ``payload_len``-byte payload: k + 32 ceil(k / 223), k = n + 4.  ValueError above
    MAX_PAYLOAD."""
    n = C.c_uint32(0)
    if payload_len < 0 or payload_len > 0xffffffff or _abi.load().ofdm_rs_coded_len(int(payload_len), C.byref(n)) != _abi.OFDM_OK:
        raise ValueError("rs: len(payload) must be in [0, %d]" % MAX_PAYLOAD)
    return n.value


def max_payload_under(limit):
    """The largest payload whose RS block fits an inner code that takes ``limit`` bytes (1752 under 2012, 2328, 2632 and
    2904 under the LDPC code's 2684, 3020 and 3356)."""
    def block(n):
        return n + 4 + PARITY * ((n + 4 + 222) // 223)
    n = min(int(limit), MAX_PAYLOAD)
    while n >= 0 and block(n) > limit:
        n -= 1
    if n < 0:
        raise ValueError("rs: no block fits %d bytes" % limit)
    return n


def payload_len(coded_len):
    """Payload bytes of an RS block of ``coded_len`` bytes, None for a length that is no block (one the block length
    never reaches, under 36, over MAX_CODED)."""
    n = C.c_uint32(0)
    if coded_len < 0 or coded_len > 0xffffffff or _abi.load().ofdm_rs_payload_len(int(coded_len), C.byref(n)) != _abi.OFDM_OK:
        return None
    return n.value


def rs_cfg(max_erasures=DEFAULT_MAX_ERASURES):
    """``ofdm_rs_rel_cfg`` of a decode with reliabilities: at most ``max_erasures`` (0 .. 32) symbols of a codeword are
    erased; 0 turns the second pass off."""
    if isinstance(max_erasures, bool) or int(max_erasures) != max_erasures or not 0 <= max_erasures <= PARITY:
        raise ValueError("rs: max_erasures must be an integer in [0, %d]" % PARITY)
    return _abi.ofdm_rs_rel_cfg(struct_size=C.sizeof(_abi.ofdm_rs_rel_cfg), max_erasures=int(max_erasures))


def as_cfg(rs):
    """None / True, a dict of rs_cfg's keywords or an ``ofdm_rs_rel_cfg`` -> ``ofdm_rs_rel_cfg``."""
    if isinstance(rs, _abi.ofdm_rs_rel_cfg):
        return rs
    if rs is None or rs is True:
        return rs_cfg()
    if isinstance(rs, dict):
        return rs_cfg(**rs)
    raise ValueError("rs: expected None, True, a dict of rs_cfg's keywords or an ofdm_rs_rel_cfg")


def rel_from_values(values):
    """One reliability byte per byte from its eight int8 values: the smallest |v|, -128 read as 127 (0 .. 127; a byte
    with an erased bit gets 0).  ``len(values)`` must be a multiple of 8."""
    v = np.ascontiguousarray(values, np.int8).reshape(-1)
    if len(v) % 8:
        raise ValueError("rs: 8 values per byte")
    a = np.minimum(np.abs(v.astype(np.int16)), 127).reshape(-1, 8)
    return a.min(axis=1).astype(np.uint8)
