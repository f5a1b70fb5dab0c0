"""Outer code: the length arithmetic of the Reed-Solomon layer over the payload.

RS over GF(2^8) with 32 parity bytes per codeword (t = 16), byte-interleaved to the depth a payload needs, decoded on
the GPU (include/ofdm_hip.h, "outer code").  It sits above the coded links (``fec``) and corrects
the short bursts of wrong bytes a Viterbi decoder leaves; it also works on an uncoded link.  The code has no
parameters.  The work is ``Engine.rs_encode`` / ``Engine.rs_decode``; ``ofdm_mod(rs=True)`` and ``ofdm_demod(rs=True)``
put it on a link, both ends alike.
"""
import ctypes as C

from . import _abi

PARITY = _abi.OFDM_RS_PARITY
MAX_PAYLOAD = _abi.OFDM_RS_MAX_PAYLOAD
MAX_CODED = _abi.OFDM_RS_MAX_CODED
MAX_PAYLOAD_UNDER_FEC = 1780          # the RS block must fit fec.MAX_PAYLOAD: W = 8, block 2040


def coded_len(payload_len):
    """Bytes of the RS block of a ``payload_len``-byte payload: k + 32 ceil(k / 223), k = n + 4.  ValueError above
    MAX_PAYLOAD."""
    n = C.c_uint32(0)
    if payload_len < 0 or payload_len > 0xffffffff or _abi.load().ofdm_rs_coded_len(int(payload_len), C.byref(n)) != _abi.OFDM_OK:
        raise ValueError("rs: len(payload) must be in [0, %d]" % MAX_PAYLOAD)
    return n.value


def payload_len(coded_len):
    """Payload bytes of an RS block of ``coded_len`` bytes, None for a length that is no block (one the block length
    never reaches, under 36, over MAX_CODED)."""
    n = C.c_uint32(0)
    if coded_len < 0 or coded_len > 0xffffffff or _abi.load().ofdm_rs_payload_len(int(coded_len), C.byref(n)) != _abi.OFDM_OK:
        return None
    return n.value
