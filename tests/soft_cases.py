"""Shared by test_soft_host.py and test_gpu_soft.py: the definition of the soft-decision receive option
(include/ofdm_hip.h, "soft-decision receive") restated in NumPy, float32 operation by float32 operation, so that a GPU
result is compared with array_equal; the model fed from a receiver's taps; and the link both files run.

    carrier weight  m_i = eq[i].re^2 + eq[i].im^2;  w_i = 1 / m_i if m_i is finite and > 0, else 0
    mean weight     wbar = (sequential float32 sum of w_smap[c], c ascending) / nmap
    gain            g = scale / (wbar * dmin2);  wbar 0 or not finite: the packet's values are all 0
    bit b           l = (D0 - D1) * (w_smap[c] * g), D0 / D1 the nearest squared distance among the points with bit b
                    clear / set;  v = rint(l) clamped to [-127, 127], NaN -> 0
    placement       stream bit beta = (s nmap + c) nbits + b -> frame byte beta >> 3, weight e = beta & 7; message byte
                    mb = (beta >> 3) - 4 in [0, plen) -> index 8 mb + 7 - e, negated where bit e of mask[mb] is set"""
import functools

import numpy as np

import fec_cases as fc
from ofdm_uhd_amd import _abi, config, multipath

F32 = np.float32
HEADER = 4


def cst_of(cfg):
    return np.array([complex(v.re, v.im) for v in cfg.constellation[:cfg.arity]], np.complex64)


def smap_of(cfg):
    return np.asarray(config.carrier_map(cfg.occupied_tones, cfg.occupied_tones, cfg.carrier_map.decode("ascii") or "FE7F"))


def mask_of(cfg):
    return np.frombuffer(bytes(bytearray(cfg.whitening_mask)), np.uint8)


def dmin2(cst):
    """Smallest cnorm(csub(cst[a], cst[b])) over a != b, float32."""
    cst = np.asarray(cst, np.complex64)
    dr = cst.real[:, None] - cst.real[None, :]
    di = cst.imag[:, None] - cst.imag[None, :]
    d = dr * dr + di * di
    assert d.dtype == F32
    return d[~np.eye(len(cst), dtype=bool)].min()


def weights(eq):
    """w_i of an equaliser row (complex64 [occ])."""
    eq = np.asarray(eq, np.complex64)
    with np.errstate(all="ignore"):
        m = eq.real * eq.real + eq.imag * eq.imag
        good = np.isfinite(m) & (m > 0)
        return np.where(good, F32(1) / np.where(good, m, F32(1)), F32(0)).astype(F32)


def mean_weight(w, smap):
    """One sequential float32 chain in carrier order, divided by (float)nmap."""
    acc = F32(0)
    with np.errstate(all="ignore"):
        for v in np.asarray(w, F32)[np.asarray(smap)]:
            acc = F32(acc + v)
        return F32(acc / F32(len(smap)))


def gain(wbar, cst, scale=32.0):
    """g, or None where the packet's values are all 0."""
    if not (np.isfinite(wbar) and wbar > 0):
        return None
    with np.errstate(all="ignore"):
        return F32(F32(scale) / F32(wbar * dmin2(cst)))


def placement(plen, nbits, ncarriers):
    """(carrier, bit, index) of every stream bit of ``ncarriers`` carriers (stream order) that lands in the packet."""
    k = np.arange(ncarriers * nbits, dtype=np.int64)
    byte, e = k >> 3, k & 7
    mb = byte - HEADER
    ok = (mb >= 0) & (mb < plen)
    return (k // nbits)[ok], (k % nbits)[ok], (8 * mb + 7 - e)[ok], mb[ok], e[ok]


def carriers_needed(plen, nbits):
    return 0 if plen == 0 else -(-8 * (HEADER + plen) // nbits)


def packet_values(x, eq, smap, cst, plen, mask, scale=32.0):
    """The packet's 8 * plen int8 values.  ``x``: the slicer's inputs of the packet's demapped symbols in stream order
    (complex64, symbol after symbol, nmap carriers each; at least carriers_needed of them), ``eq``: its hinv row."""
    cst = np.asarray(cst, np.complex64)
    arity, nmap = len(cst), len(smap)
    nbits = int(arity).bit_length() - 1
    out = np.zeros(8 * plen, np.int8)
    if plen == 0:
        return out
    w = weights(eq)
    g = gain(mean_weight(w, smap), cst, scale)
    if g is None:
        return out
    ncar = carriers_needed(plen, nbits)
    x = np.asarray(x, np.complex64).reshape(-1)[:ncar]
    assert len(x) == ncar, (len(x), ncar)
    with np.errstate(all="ignore"):
        dr = x.real[:, None] - cst.real[None, :]
        di = x.imag[:, None] - cst.imag[None, :]
        d = dr * dr + di * di                                     # cnorm(csub(x, cst[j])), separately rounded
        assert d.dtype == F32
        wg = (w[np.asarray(smap)][np.arange(ncar) % nmap] * g).astype(F32)
        car, bit, idx, mb, e = placement(plen, nbits, ncar)
        j = np.arange(arity)
        v = np.zeros((ncar, nbits), F32)
        inf = F32(np.inf)
        for b in range(nbits):
            one = ((j >> b) & 1).astype(bool)
            D0 = np.fmin.reduce(np.where(~one[None, :], d, inf), axis=1, initial=inf)
            D1 = np.fmin.reduce(np.where(one[None, :], d, inf), axis=1, initial=inf)
            l = ((D0 - D1).astype(F32) * wg).astype(F32)
            r = np.rint(l)
            r = np.where(np.isnan(r), F32(0), r)
            v[:, b] = np.clip(r, -127, 127)
    val = v[car, bit].astype(np.int32)
    neg = ((np.asarray(mask, np.uint8)[mb] >> e) & 1).astype(bool)
    out[idx] = np.where(neg, -val, val).astype(np.int8)
    return out


def hard_bits(payload):
    return np.unpackbits(np.frombuffer(bytes(payload), np.uint8))


def call_values(cfg, pk, recs, eq_rows, sink, dem, scale=32.0):
    """The model over one receive call: the packets ``pk`` [(ok, payload)], their link-quality records, their CSI ``eq``
    rows, and the TAP_RX_SINK / TAP_RX_DEMAPPED taps of the same call."""
    smap, cst, mask = smap_of(cfg), cst_of(cfg), mask_of(cfg)
    dem = np.asarray(dem).astype(bool)
    sink_row = np.cumsum(dem) - 1
    out = []
    for (ok, payload), r, eq in zip(pk, recs, eq_rows):
        fs, ns = int(r["first_symbol"]), int(r["nsym"])
        x = sink[sink_row[fs + 1:fs + 1 + ns], :len(smap)]
        out.append(packet_values(x, eq, smap, cst, len(payload), mask, scale))
    return out


def hinv_from_preamble(cfg, fft_row, coarse=0):
    """The equaliser row as test_gpu_csi._model_check forms it from the preamble's TAP_RX_FFT row."""
    N, occ, CP = cfg.fft_length, cfg.occupied_tones, cfg.cp_length
    zl = (N - occ + 1) // 2
    ks = np.array([complex(v.re, v.im) for v in cfg.known_symbol[:occ]], np.complex64)
    idx = np.arange(occ) + zl + coarse
    Y = np.where((idx >= 0) & (idx < N), fft_row[np.clip(idx, 0, N - 1)], 0).astype(np.complex64)
    a = np.float32(-2 * np.pi * coarse * CP / N)
    comp = np.complex64(np.cos(a) + 1j * np.sin(a))
    h = np.zeros(occ, np.complex64)
    with np.errstate(all="ignore"):
        h[0::2] = ks[0::2] / (comp * Y[0::2])
        h[1:occ - 1:2] = (h[0:occ - 2:2] + h[2::2][:len(h[1:occ - 1:2])]) / np.float32(2)
    if occ % 2 == 0:
        h[occ - 1] = h[occ - 2]
    return h


# ---- the link of the link test: N 512 / occ 200 / CP 128, 16-QAM, the six packets of test_gpu_fec.py, two paths + noise ----
LINK_MOD, LINK_N, LINK_OCC, LINK_CP = "qam16", 512, 200, 128
LINK_SIZES = (300, 301, 257, 400, 333, 300)
LINK_PATHS = [(0, 1.0), (9, 0.8 * np.exp(2.1j))]     # a second ray 1.9 dB down, nine samples late: notches across the band
LINK_SNR_DB, LINK_SEED = 13.0, 7                      # chosen on the CPU: test_gpu_soft.py's docstring has the grid
LINK_GRID_DB = tuple(range(10, 25))


@functools.lru_cache(maxsize=None)
def link_payloads():
    rng = np.random.default_rng(2024)
    return tuple(rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in LINK_SIZES)


def link_air(iq, N=LINK_N, CP=LINK_CP):
    return np.concatenate([np.zeros(2 * N, np.complex64), iq, np.zeros(N + CP + 2 * N, np.complex64)])


def link_channel_cfg(snr_db, psig, seed=LINK_SEED):
    return multipath.multipath_cfg(paths=LINK_PATHS, sigma=multipath.sigma_for_snr(snr_db, psig), seed=seed)


def link_on_the_cpu(orc, cfg, snr_db, seed=LINK_SEED, scale=32.0):
    """The CPU chain at one noise level: coded blocks -> oracle transmitter -> float64 channel model -> oracle receiver
    with its taps -> the soft model -> both model decoders.  Returns (hard, soft): per packet (ok, payload == sent)."""
    import multipath_cases as mpc
    pay = link_payloads()
    iq = orc.tx(cfg, [fc.encode(p) for p in pay])
    psig = float(np.mean(np.abs(iq.astype(np.complex128)) ** 2))
    y, _ = mpc.model(link_air(iq), link_channel_cfg(snr_db, psig, seed), 0)
    res = orc.rx(cfg, y.astype(np.complex64), (1 << _abi.TAP_RX_FFT) | (1 << _abi.TAP_RX_SINK) | (1 << _abi.TAP_RX_FRAMES))
    pk = res.packets
    fft, sink, frames = res.tap(_abi.TAP_RX_FFT), res.tap(_abi.TAP_RX_SINK), res.tap(_abi.TAP_RX_FRAMES)
    smap, cst, mask = smap_of(cfg), cst_of(cfg), mask_of(cfg)
    nbits = int(cfg.arity).bit_length() - 1
    hard, soft = [], []
    if len(pk) != len(pay) or len(frames) != len(pay):
        return None, None                                  # a flag lost or gained: the level is no candidate
    # no chain on this link: frame k is packet k, its preamble row K_0 + 1 + ... rows down, its demapped rows in order
    pre = np.concatenate([[0], np.cumsum(frames[:, 1].astype(np.int64) + 1)])[:-1]
    row = 0
    for k, ((ok, blk), sent) in enumerate(zip(pk, pay)):
        ns = -(-8 * (HEADER + len(blk) + 4) // (len(smap) * nbits))
        x = sink[row:row + ns, :len(smap)]
        row += ns
        eq = hinv_from_preamble(cfg, fft[pre[k]])
        v = packet_values(x, eq, smap, cst, len(blk), mask, scale)
        h, s = fc.decode(blk), fc.decode_values(v)
        hard.append((h[0], h[1] == sent))
        soft.append((s[0], s[1] == sent))
    if row != len(sink):
        return None, None
    return hard, soft
