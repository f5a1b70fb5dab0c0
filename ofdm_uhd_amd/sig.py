"""Coded links: the signal field -- a 12-byte field in front of every coded block that names the block's coding.

A 12-bit coding word (codec, rate id, outer code present, the convolutional interleaver's columns) is sent as four
copies of its extended Golay (24,12,8) codeword, inside the packet's payload, and decoded on the GPU by exhaustive
maximum likelihood over the sum of the copies (include/ofdm_hip.h, "coded links: the signal field"; DESIGN.md section
7).  With it a receiver needs no coding setting of its own, one batch can hold packets of different codings, and the
receiver's own SNR measurements can choose the next coding (``suggest_coding``).  The work is ``Engine.sig_encode`` /
``Engine.sig_decode`` / ``Engine.sig_decode_soft`` / ``Engine.rx_sig_decode_soft``; ``ofdm_mod(sig=True)`` and
``ofdm_demod(sig=True)`` put it on a link.

A coding is a ``Coding``: ``coding(fec=..., ldpc=..., rs=...)`` makes one from what ``ofdm_mod`` takes for those
keywords, ``coding(word)`` from a decoded word; ``Coding.word`` is the way back.
"""
import collections
import ctypes as C

import numpy as np

from . import _abi, fec as _fec, ldpc as _ldpc, ofdm_packet_utils, rs as _rs

FIELD_BYTES = _abi.OFDM_SIG_FIELD_BYTES
NO_WORD = _abi.OFDM_SIG_NO_WORD
CODEC_NONE, CODEC_FEC, CODEC_LDPC = _abi.OFDM_SIG_CODEC_NONE, _abi.OFDM_SIG_CODEC_FEC, _abi.OFDM_SIG_CODEC_LDPC
_RATE_NAMES = ("1/2", "2/3", "3/4", "5/6")        # by OFDM_FEC_RATE_* / OFDM_LDPC_RATE_*


class Coding(collections.namedtuple("Coding", "codec rate rs interleave")):
    """What a signal field says: ``codec`` (CODEC_NONE / CODEC_FEC / CODEC_LDPC), ``rate`` (the rate id 0 .. 3), ``rs``
    (the outer code is present) and ``interleave`` (the convolutional interleaver's columns; 0 for the other codecs)."""
    __slots__ = ()

    @property
    def word(self):
        """The 12-bit coding word."""
        w = C.c_uint16(0)
        if _abi.load().ofdm_sig_word(self.codec, self.rate, int(self.rs), self.interleave, C.byref(w)) != _abi.OFDM_OK:
            raise ValueError("sig: %r is no coding" % (tuple(self),))
        return w.value

    @property
    def fec(self):
        """``ofdm_mod`` / ``Engine.fec_*``'s ``fec`` argument of this coding, None where it has no convolutional code."""
        return dict(interleave=self.interleave, rate=_RATE_NAMES[self.rate]) if self.codec == CODEC_FEC else None

    def ldpc(self, max_iters=None):
        """``Engine.ldpc_*``'s ``ldpc`` argument of this coding, None where it has no LDPC code."""
        if self.codec != CODEC_LDPC:
            return None
        d = dict(rate=_RATE_NAMES[self.rate])
        if max_iters is not None:
            d["max_iters"] = max_iters
        return d

    def __str__(self):
        inner = {CODEC_NONE: "uncoded", CODEC_FEC: "fec %s C=%d" % (_RATE_NAMES[self.rate], self.interleave),
                 CODEC_LDPC: "ldpc %s" % _RATE_NAMES[self.rate]}[self.codec]
        return inner + ("+rs" if self.rs else "")


def word_valid(word):
    """Whether ``word`` is one of the 50 valid coding words."""
    return isinstance(word, (int, np.integer)) and 0 <= int(word) <= 0xffffffff and bool(_abi.load().ofdm_sig_word_valid(int(word)))


def coding(word=None, fec=None, ldpc=None, rs=False):
    """``coding(fec=, ldpc=, rs=)``: the Coding of what ``ofdm_mod`` takes for these keywords (an LDPC code's
    ``max_iters`` is the receiver's business and not part of it).  ``coding(word)``: the Coding of a 12-bit word,
    ValueError for a word that is not valid.  A Coding passes through."""
    if word is not None:
        if fec is not None or ldpc is not None or rs:
            raise ValueError("sig.coding takes a word or keywords, not both")
        if isinstance(word, Coding):
            word.word       # (ValueError for fields that name no coding)
            return word
        if isinstance(word, bool) or not isinstance(word, (int, np.integer)):
            raise ValueError("sig.coding: a word is an int")
        f = [C.c_uint32(0) for _ in range(4)]
        if not 0 <= int(word) <= 0xffffffff or _abi.load().ofdm_sig_word_fields(int(word), *[C.byref(x) for x in f]) != _abi.OFDM_OK:
            raise ValueError("sig: 0x%x is no valid coding word" % int(word))
        return Coding(f[0].value, f[1].value, bool(f[2].value), f[3].value)
    fc, lc = _fec.as_cfg(fec), _ldpc.as_cfg(ldpc)
    if fc is not None and lc is not None:
        raise ValueError("fec= and ldpc= are two inner codes: a link has one of them")
    if isinstance(rs, dict):
        raise ValueError("sig: rs is True or False here (rs=dict(erasures=...) is a receiver's setting)")
    if fc is not None:
        c = Coding(CODEC_FEC, int(fc.rate), bool(rs), int(fc.interleave_cols))
    elif lc is not None:
        c = Coding(CODEC_LDPC, int(lc.rate), bool(rs), 0)
    else:
        c = Coding(CODEC_NONE, 0, bool(rs), 0)
    c.word
    return c


def all_codings():
    """The 50 valid codings, by word."""
    return [coding(w) for w in range(0, 1 << 12, 16) if word_valid(w)]


def body_len(n, cod):
    """Bytes of the coded body of an ``n``-byte payload under ``cod``: the outer code's block, if any, inside the inner
    code's, if any.  ValueError above what the codes take."""
    cod = coding(cod)
    if cod.rs:
        n = _rs.coded_len(n)
    if cod.codec == CODEC_FEC:
        n = _fec.coded_len(n, _RATE_NAMES[cod.rate])
    elif cod.codec == CODEC_LDPC:
        n = _ldpc.coded_len(n, _RATE_NAMES[cod.rate])
    return n


def coded_len(n, cod):
    """Bytes of the block (field | body) of an ``n``-byte payload under ``cod``: what gets framed."""
    return FIELD_BYTES + body_len(n, cod)


def max_payload(cod, block_limit=None):
    """The largest payload under ``cod`` whose block, field included, is at most ``block_limit`` bytes -- None: what
    ofdm_packet_utils' whitening mask leaves a packet next to its CRC and the trailing 0x55, 4091, Engine.framed_len's
    limit without padding.  Found from the codes' own length functions: the largest n they take whose coded_len
    fits."""
    cod = coding(cod)
    if block_limit is None:
        block_limit = len(ofdm_packet_utils.random_mask_tuple) - 5

    def fits(n):
        try:
            return coded_len(n, cod) <= block_limit
        except ValueError:
            return False
    if not fits(0):
        raise ValueError("sig: no block of %s fits %d bytes" % (cod, block_limit))
    lo, hi = 0, int(block_limit)            # coded_len grows with n: fits(lo), not fits(hi + 1)
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if fits(mid):
            lo = mid
        else:
            hi = mid - 1
    return lo


def default_table():
    """An ordered list of (min_snr_db, Coding) for ``suggest_coding``: uncoded and the four LDPC rates, most redundant
    first.  The thresholds are the lowest grid points at which tools/ldpc_gain.py's CPU models (BPSK over AWGN, one full
    codeword per block, 400 blocks, one seed) failed no block -- Eb/N0 2.0, 3.0, 3.5 and 4.0 dB at rates 1/2, 2/3, 3/4 and
    5/6, moved to Es/N0 by 10 log10(rate) -- and, for the uncoded link, the 10.5 dB at which
    BPSK's bit error rate is 1e-6.  They are NOT measured on a GPU or on a real channel, and they read the receiver's
    per-carrier SNR as BPSK's Es/N0: a starting point for a link's own table, nothing more."""
    return [(-1.0, coding(ldpc=dict(rate="1/2"))), (1.2, coding(ldpc=dict(rate="2/3"))), (2.3, coding(ldpc=dict(rate="3/4"))),
            (3.2, coding(ldpc=dict(rate="5/6"))), (10.5, coding())]


def suggest_coding(snr_db, table=None, margin_db=1.0):
    """The least redundant coding of ``table`` -- an ordered list of (min_snr_db, coding), thresholds ascending, the
    most redundant coding first -- whose threshold plus ``margin_db`` the median of ``snr_db`` (numbers in dB, or
    quality records, whose ``snr_preamble_db`` is taken) clears.  The first entry where the median clears none, None
    for an empty ``snr_db``."""
    table = default_table() if table is None else [(float(t), coding(c)) for t, c in table]
    if not table:
        raise ValueError("suggest_coding: an empty table")
    if any(b[0] < a[0] for a, b in zip(table, table[1:])):
        raise ValueError("suggest_coding: the table's thresholds must ascend")
    snr = np.asarray(snr_db)
    if snr.dtype.names:                 # quality records (engine.QUALITY_DTYPE): their preamble SNR
        snr = snr["snr_preamble_db"]
    snr = snr.astype(np.float64).reshape(-1)
    snr = snr[~np.isnan(snr)]           # (a noiseless capture's +inf clears every threshold)
    if snr.size == 0:
        return None
    med = float(np.median(snr))
    best = table[0][1]
    for thr, cod in table:
        if med >= thr + margin_db:
            best = cod
    return best
