"""Coded links, the second inner code: the configuration and length arithmetic of the LDPC layer over the payload.

A rate-1/2 quasi-cyclic LDPC code (circulant size 64, 12 x 24 base matrix, 1536-bit codewords) decoded by a layered
normalised min-sum decoder on the GPU, one wave per codeword (include/ofdm_hip.h, "coded links: LDPC"; DESIGN.md
section 7).  The work is ``Engine.ldpc_encode`` / ``Engine.ldpc_decode`` / ``Engine.ldpc_decode_soft``;
``ofdm_mod(ldpc=...)`` and ``ofdm_demod(ldpc=...)`` put it on a link in the place of ``fec=``.
"""
import ctypes as C

from . import _abi

MAX_PAYLOAD = _abi.OFDM_LDPC_MAX_PAYLOAD
MAX_CODED = _abi.OFDM_LDPC_MAX_CODED
MAX_ITERS = 64


def ldpc_cfg(max_iters=20):
    """An ``ofdm_ldpc_cfg``: ``max_iters`` is the most iterations a codeword gets, 1 .. 64."""
    if isinstance(max_iters, bool) or not isinstance(max_iters, int) or not 1 <= max_iters <= MAX_ITERS:
        raise ValueError("ldpc max_iters must be an int in [1, %d]" % MAX_ITERS)
    cfg = _abi.ofdm_ldpc_cfg()
    cfg.struct_size = C.sizeof(_abi.ofdm_ldpc_cfg)
    cfg.max_iters = max_iters
    return cfg


def as_cfg(ldpc):
    """What ``ofdm_mod`` / ``ofdm_demod`` / the Engine methods accept as ``ldpc``: None or False (no coding), True
    (defaults), an int (max_iters), a dict of ldpc_cfg's keywords or an ``ofdm_ldpc_cfg``."""
    if ldpc is None or ldpc is False:
        return None
    if ldpc is True:
        return ldpc_cfg()
    if isinstance(ldpc, _abi.ofdm_ldpc_cfg):
        return ldpc
    if isinstance(ldpc, dict):
        unknown = set(ldpc) - {"max_iters"}
        if unknown:
            raise ValueError("unknown ldpc option(s): %s" % ", ".join(sorted(unknown)))
        return ldpc_cfg(**ldpc)
    return ldpc_cfg(ldpc)


def coded_len(payload_len):
    """Bytes of the coded block of a ``payload_len``-byte payload: n + 4 + 96 * ceil((n + 4) / 96).  ValueError above
    MAX_PAYLOAD."""
    n = C.c_uint32(0)
    if payload_len < 0 or payload_len > 0xffffffff or _abi.load().ofdm_ldpc_coded_len(
            int(payload_len), C.byref(n)) != _abi.OFDM_OK:
        raise ValueError("ldpc: len(payload) must be in [0, %d]" % MAX_PAYLOAD)
    return n.value


def payload_len(coded_len):
    """Payload bytes of a coded block of ``coded_len`` bytes, None for a length that is no block."""
    n = C.c_uint32(0)
    if coded_len < 0 or coded_len > 0xffffffff or _abi.load().ofdm_ldpc_payload_len(
            int(coded_len), C.byref(n)) != _abi.OFDM_OK:
        return None
    return n.value
