"""The punctured rates of the coded-link layer as NumPy, on top of fec_cases.py (imported, not edited), shared by
test_punct_host.py and test_gpu_punct.py.  Restates include/ofdm_hip.h ("punctured rates"): the 802.11 patterns over
the mother coded bits, the kept stream and its block length, the C' interleaver of the punctured block, and decoding
as the mother decoder on values with zeros at every position that was not sent.  Everything is integer arithmetic, so
a GPU result is compared with array_equal."""
import numpy as np

import fec_cases as fc

RATES = ("2/3", "3/4", "5/6")
RATE_ID = {"1/2": 0, "2/3": 1, "3/4": 2, "5/6": 3}
PERIOD = {"2/3": 4, "3/4": 6, "5/6": 10}
KEEP = {"2/3": (0, 1, 2), "3/4": (0, 1, 2, 5), "5/6": (0, 1, 2, 5, 6, 9)}


def mother_bits(n):
    return 16 * n + 76                     # 2T, T = 8 (n + 4) + 6: the pad is not among them


def kept_index(rate, n):
    """i_q: the mother indices of the kept bits of an n-byte payload's block, ascending."""
    i = np.arange(mother_bits(n))
    return i[np.isin(i % PERIOD[rate], KEEP[rate])]


def kept_bits(rate, n):
    return len(kept_index(rate, n))


def coded_len(n, rate):
    if rate == "1/2":
        return fc.coded_len(n)
    return -(-kept_bits(rate, n) // 8)


def length_table(rate):
    """{P: n} over every payload length."""
    if rate == "1/2":
        return {fc.coded_len(n): n for n in range(fc.MAX_PAYLOAD + 1)}
    # (K by the closed form the definition implies, checked against the counted one in test_punct_host.py)
    per, keep = PERIOD[rate], KEEP[rate]
    out = {}
    for n in range(fc.MAX_PAYLOAD + 1):
        full, rem = divmod(mother_bits(n), per)
        K = full * len(keep) + sum(1 for k in keep if k < rem)
        out[-(-K // 8)] = n
    return out


_TABLES = {}


def payload_len(P, rate):
    """n of a block of P bytes, None for a length that is no block at this rate."""
    if rate not in _TABLES:
        _TABLES[rate] = length_table(rate)
    return _TABLES[rate].get(P)


def cols(C, P):
    """C': the largest power of two <= C that divides 8 P."""
    c = C
    while (8 * P) % c:
        c //= 2
    return c


def encode(payload, C=16, rate="3/4"):
    payload = bytes(payload)
    if rate == "1/2":
        return fc.encode(payload, C)
    assert len(payload) <= fc.MAX_PAYLOAD and C in fc.COLS
    c = fc.conv(fc.info_bits(payload))
    assert len(c) == mother_bits(len(payload))
    kept = c[kept_index(rate, len(payload))]
    P = -(-len(kept) // 8)
    p = np.concatenate([kept, np.zeros(8 * P - len(kept), np.uint8)])
    return np.packbits(p[fc.perm(8 * P, cols(C, P))]).tobytes()


def mother_values(v, C=16, rate="3/4"):
    """One signed value per sent bit of a punctured block -> the mother block's values in SENT order for C columns (what
    fc.decode_values(., C) takes), or None for a length that is no block."""
    v = np.asarray(v, np.int8)
    if len(v) % 8 or payload_len(len(v) // 8, rate) is None:
        return None
    P = len(v) // 8
    n = payload_len(P, rate)
    p = np.empty(8 * P, np.int8)
    p[fc.perm(8 * P, cols(C, P))] = v      # undo the C' interleaver: p[q] belongs to kept bit q
    idx = kept_index(rate, n)
    d = np.zeros(16 * n + 80, np.int8)
    d[idx] = p[:len(idx)]                  # the pad values p[K:] are ignored; punctured and pad positions stay 0
    return d[fc.perm(len(d), C)]


def decode_values(v, C=16, rate="3/4"):
    """One punctured block from one signed value per sent bit -> (ok, payload, corrected)."""
    if rate == "1/2":
        return fc.decode_values(v, C)
    m = mother_values(v, C, rate)
    if m is None:
        return (0, b"", 0)
    return fc.decode_values(m, C)


def decode(block, C=16, rate="3/4"):
    """One hard punctured block (bytes of any length) -> (ok, payload, corrected)."""
    if rate == "1/2":
        return fc.decode(block, C)
    block = bytes(block)
    if payload_len(len(block), rate) is None:
        return (0, b"", 0)
    return decode_values(fc.hard_values(block), C, rate)


def link_on_the_cpu(orc, cfg, snr_db, rate, seed=None, scale=32.0):
    """soft_cases.link_on_the_cpu at a rate: the punctured blocks of soft_cases.link_payloads() -> oracle transmitter ->
    float64 channel model -> oracle receiver with its taps -> the soft model -> both model decoders at that rate.
    Returns (hard, soft): per packet (ok, payload == sent); (None, None) where the receiver's packet list is not the
    six packets."""
    import multipath_cases as mpc
    import soft_cases as sc
    from ofdm_uhd_amd import _abi
    seed = sc.LINK_SEED if seed is None else seed
    pay = sc.link_payloads()
    iq = orc.tx(cfg, [encode(p, 16, rate) for p in pay])
    psig = float(np.mean(np.abs(iq.astype(np.complex128)) ** 2))
    y, _ = mpc.model(sc.link_air(iq), sc.link_channel_cfg(snr_db, psig, seed), 0)
    res = orc.rx(cfg, y.astype(np.complex64), (1 << _abi.TAP_RX_FFT) | (1 << _abi.TAP_RX_SINK) | (1 << _abi.TAP_RX_FRAMES))
    pk = res.packets
    fft, sink, frames = res.tap(_abi.TAP_RX_FFT), res.tap(_abi.TAP_RX_SINK), res.tap(_abi.TAP_RX_FRAMES)
    smap, cst, mask = sc.smap_of(cfg), sc.cst_of(cfg), sc.mask_of(cfg)
    nbits = int(cfg.arity).bit_length() - 1
    if len(pk) != len(pay) or len(frames) != len(pay):
        return None, None
    pre = np.concatenate([[0], np.cumsum(frames[:, 1].astype(np.int64) + 1)])[:-1]
    row, hard, soft = 0, [], []
    for k, ((ok, blk), sent) in enumerate(zip(pk, pay)):
        ns = -(-8 * (sc.HEADER + len(blk) + 4) // (len(smap) * nbits))
        x = sink[row:row + ns, :len(smap)]
        row += ns
        eq = sc.hinv_from_preamble(cfg, fft[pre[k]])
        v = sc.packet_values(x, eq, smap, cst, len(blk), mask, scale)
        h, s = decode(blk, 16, rate), decode_values(v, 16, rate)
        hard.append((h[0], h[1] == sent))
        soft.append((s[0], s[1] == sent))
    if row != len(sink):
        return None, None
    return hard, soft
