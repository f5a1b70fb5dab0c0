"""Coded links: the configuration and length arithmetic of the forward-error-correcting layer over the payload.

A rate-1/2, K = 7 convolutional code (133 / 171 octal) with a block interleaver, decoded by a full-sequence Viterbi
decoder on the GPU, and its punctured rates 2/3, 3/4 and 5/6 (the 802.11 patterns) for links that can afford less
redundancy (include/ofdm_hip.h, "coded links").  The work is ``Engine.fec_encode`` /
``Engine.fec_decode`` / ``Engine.fec_decode_soft``; ``ofdm_mod(fec=...)`` and ``ofdm_demod(fec=...)`` put it on a
link, both ends with the same setting.

Reliabilities out (include/ofdm_hip.h, "coded links, reliabilities out"): ``Engine.fec_decode_rel`` /
``Engine.fec_decode_soft_rel`` / ``Engine.rx_fec_decode_soft_rel`` run a second decoder that returns the same payloads,
verdicts and corrected counts, and one uint8 per decoded payload byte: half the metric gap between the decoded path and
the best path that disagrees in one of the byte's bits, clamped to 255 (0: a path as good as the decoded one disagrees
here).  That is what ``Engine.rs_decode_rel`` takes, so a concatenated link can erase the outer code's weakest symbols:
``ofdm_demod(fec=..., rs=dict(erasures=True, source="fec"))``.
"""
import ctypes as C

from . import _abi

MAX_PAYLOAD = _abi.OFDM_FEC_MAX_PAYLOAD
MAX_CODED = _abi.OFDM_FEC_MAX_CODED
INTERLEAVE_COLS = (1, 2, 4, 8, 16)
RATES = {"1/2": _abi.OFDM_FEC_RATE_1_2, "2/3": _abi.OFDM_FEC_RATE_2_3, "3/4": _abi.OFDM_FEC_RATE_3_4,
         "5/6": _abi.OFDM_FEC_RATE_5_6}


def rate_id(rate):
    """The OFDM_FEC_RATE_* value of ``rate``: one of the strings "1/2", "2/3", "3/4", "5/6", None (1/2), or an
    ``ofdm_fec_cfg`` (its rate)."""
    if rate is None:
        return _abi.OFDM_FEC_RATE_1_2
    if isinstance(rate, _abi.ofdm_fec_cfg):
        return int(rate.rate)
    if not isinstance(rate, str) or rate not in RATES:
        raise ValueError('fec rate must be "1/2", "2/3", "3/4" or "5/6"')
    return RATES[rate]


def fec_cfg(interleave=16, rate="1/2"):
    """An ``ofdm_fec_cfg``: ``interleave`` is the interleaver's column count, one of 1 (none), 2, 4, 8, 16; ``rate``
    the code rate, "1/2" (the mother code) or one of the punctured "2/3", "3/4", "5/6"."""
    if isinstance(interleave, bool) or int(interleave) != interleave or int(interleave) not in INTERLEAVE_COLS:
        raise ValueError("fec interleave must be 1, 2, 4, 8 or 16")
    cfg = _abi.ofdm_fec_cfg()
    cfg.struct_size = C.sizeof(_abi.ofdm_fec_cfg)
    cfg.interleave_cols = int(interleave)
    cfg.rate = rate_id(rate)
    return cfg


def as_cfg(fec):
    """What ``ofdm_mod`` / ``ofdm_demod`` / the Engine methods accept as ``fec``: None or False (no coding), True
    (defaults), a dict of fec_cfg's keywords (``interleave``, ``rate``), an int (the column count) or an ``ofdm_fec_cfg``."""
    if fec is None or fec is False:
        return None
    if fec is True:
        return fec_cfg()
    if isinstance(fec, _abi.ofdm_fec_cfg):
        return fec
    if isinstance(fec, dict):
        return fec_cfg(**fec)
    return fec_cfg(fec)


def coded_len(payload_len, rate=None):
    """Bytes of the coded block of a ``payload_len``-byte payload: 2 n + 10 at rate 1/2, P(n) of the punctured block
    at ``rate`` (a rate string or an ``ofdm_fec_cfg``).  ValueError above MAX_PAYLOAD."""
    n = C.c_uint32(0)
    if payload_len < 0 or payload_len > 0xffffffff or _abi.load().ofdm_fec_coded_len_rate(
            rate_id(rate), int(payload_len), C.byref(n)) != _abi.OFDM_OK:
        raise ValueError("fec: len(payload) must be in [0, %d]" % MAX_PAYLOAD)
    return n.value


def payload_len(coded_len, rate=None):
    """Payload bytes of a coded block of ``coded_len`` bytes at ``rate``, None for a length that is no block (rate 1/2:
    odd, under 10, over MAX_CODED; punctured: a length no payload length gives)."""
    n = C.c_uint32(0)
    if coded_len < 0 or coded_len > 0xffffffff or _abi.load().ofdm_fec_payload_len_rate(
            rate_id(rate), int(coded_len), C.byref(n)) != _abi.OFDM_OK:
        return None
    return n.value
