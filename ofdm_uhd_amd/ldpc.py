"""Coded links, the second inner code: the configuration and length arithmetic of the LDPC layer over the payload.

Quasi-cyclic LDPC codes of rate 1/2, 2/3, 3/4 and 5/6 (circulant size 64, 24 columns and 12, 8, 6 or 4 rows in the base
matrix, 1536-bit codewords at every rate) decoded by a layered normalised min-sum decoder on the GPU, one wave per
codeword (include/ofdm_hip.h, "coded links: LDPC").  The work is ``Engine.ldpc_encode`` /
``Engine.ldpc_decode`` / ``Engine.ldpc_decode_soft``; ``ofdm_mod(ldpc=...)`` and ``ofdm_demod(ldpc=...)`` put it on a
link in the place of ``fec=``, both ends at the same rate.

Reliabilities out (``Engine.ldpc_decode_rel`` / ``ldpc_decode_soft_rel`` / ``rx_ldpc_decode_soft_rel``,
``ofdm_demod(ldpc=..., rs=dict(erasures=True, source="ldpc"))``): the same decoder also returns one byte per payload byte
for ``Engine.rs_decode_rel`` -- min(127, the smallest final |P| of the byte's eight bits), plus 128 where the byte's
codeword met all checks (include/ofdm_hip.h, "coded links: LDPC, reliabilities out").
"""
import ctypes as C

from . import _abi

MAX_PAYLOAD = _abi.OFDM_LDPC_MAX_PAYLOAD      # at rate 1/2; max_payload(rate) for the others
MAX_CODED = _abi.OFDM_LDPC_MAX_CODED
MAX_ITERS = 64
RATES = {"1/2": _abi.OFDM_LDPC_RATE_1_2, "2/3": _abi.OFDM_LDPC_RATE_2_3, "3/4": _abi.OFDM_LDPC_RATE_3_4,
         "5/6": _abi.OFDM_LDPC_RATE_5_6}
_CW_INFO = (96, 128, 144, 160)                # info bytes of a full codeword, by rate id


def rate_id(rate):
    """The OFDM_LDPC_RATE_* value of ``rate``: one of the strings "1/2", "2/3", "3/4", "5/6", None (1/2), such a value
    itself (0 .. 3) or an ``ofdm_ldpc_cfg`` (its rate)."""
    if rate is None:
        return _abi.OFDM_LDPC_RATE_1_2
    if isinstance(rate, _abi.ofdm_ldpc_cfg):
        rate = int(rate.rate)
    if isinstance(rate, str) and rate in RATES:
        return RATES[rate]
    if isinstance(rate, int) and not isinstance(rate, bool) and 0 <= rate < len(_CW_INFO):
        return rate
    raise ValueError('ldpc rate must be "1/2", "2/3", "3/4" or "5/6"')


def cw_info(rate=None):
    """Info bytes of a full codeword at ``rate``: 96, 128, 144 or 160 of its 192."""
    return _CW_INFO[rate_id(rate)]


def max_payload(rate=None):
    """The largest payload at ``rate``, 21 full codewords less the CRC: 2012, 2684, 3020 or 3356 bytes."""
    return 21 * cw_info(rate) - 4


def ldpc_cfg(max_iters=20, rate="1/2"):
    """An ``ofdm_ldpc_cfg``: ``max_iters`` is the most iterations a codeword gets, 1 .. 64; ``rate`` the code rate,
    "1/2", "2/3", "3/4" or "5/6"."""
    if isinstance(max_iters, bool) or not isinstance(max_iters, int) or not 1 <= max_iters <= MAX_ITERS:
        raise ValueError("ldpc max_iters must be an int in [1, %d]" % MAX_ITERS)
    cfg = _abi.ofdm_ldpc_cfg()
    cfg.struct_size = C.sizeof(_abi.ofdm_ldpc_cfg)
    cfg.max_iters = max_iters
    cfg.rate = rate_id(rate)
    return cfg


def as_cfg(ldpc):
    """What ``ofdm_mod`` / ``ofdm_demod`` / the Engine methods accept as ``ldpc``: None or False (no coding), True
    (defaults), an int (max_iters), a dict of ldpc_cfg's keywords (``max_iters``, ``rate``) or an ``ofdm_ldpc_cfg``."""
    if ldpc is None or ldpc is False:
        return None
    if ldpc is True:
        return ldpc_cfg()
    if isinstance(ldpc, _abi.ofdm_ldpc_cfg):
        return ldpc
    if isinstance(ldpc, dict):
        unknown = set(ldpc) - {"max_iters", "rate"}
        if unknown:
            raise ValueError("unknown ldpc option(s): %s" % ", ".join(sorted(unknown)))
        return ldpc_cfg(**ldpc)
    return ldpc_cfg(ldpc)


def coded_len(payload_len, rate="1/2"):
    """Bytes of the coded block of a ``payload_len``-byte payload at ``rate`` (a rate string or an ``ofdm_ldpc_cfg``):
    n + 4 + PB * ceil((n + 4) / KI) with KI / PB = 96 / 96, 128 / 64, 144 / 48, 160 / 32.  ValueError above
    max_payload(rate)."""
    n = C.c_uint32(0)
    r = rate_id(rate)
    if payload_len < 0 or payload_len > 0xffffffff or _abi.load().ofdm_ldpc_coded_len_rate(
            r, int(payload_len), C.byref(n)) != _abi.OFDM_OK:
        raise ValueError("ldpc: len(payload) must be in [0, %d]" % max_payload(r))
    return n.value


def payload_len(coded_len, rate="1/2"):
    """Payload bytes of a coded block of ``coded_len`` bytes at ``rate``, None for a length that is no block there."""
    n = C.c_uint32(0)
    if coded_len < 0 or coded_len > 0xffffffff or _abi.load().ofdm_ldpc_payload_len_rate(
            rate_id(rate), int(coded_len), C.byref(n)) != _abi.OFDM_OK:
        return None
    return n.value
