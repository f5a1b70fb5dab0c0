"""Shared by test_gpu_coded_stream.py, test_gpu_soft.py and the CPU pre-check below: ONE capture builder for coded links
that are long enough for ofdm_demod.feed() to deliver packets before flush(), the ten link configurations, the model
chain behind each of them, and the chunkings.

A capture (N 512 / occ 200 / CP 128, 16-QAM): 1500 silent samples, then bursts of 1 .. 5 packets, one ofdm_mod.flush()
each, joined by seeded silences of 200 .. 30000 samples, one symbol of silence behind the last burst.  28 .. 34 packets of
0 .. 300 payload bytes in benchmark_ofdm_tx's layout (!H packet number | !H 0 | data); 0, 91, 92, 93 (either side of one
LDPC codeword), 219, 220 (either side of one RS codeword) and 300 are always among them.  The layout seed is searched
upward from the one asked for until the capture is at least 4 spans (ofdm_demod._stream_geometry()) and at most 300000
samples long.  Impairments, in this order: the oracle's channel() (seeded AWGN at ``snr_db`` below the bursts' mean
power), then seeded complex-Gaussian impulse bursts added in NumPy onto chosen packets' sample ranges -- (packet, data
symbol, sample offset in it, samples, dB above the bursts' mean power).  Packet -1 is the longest packet: every
configuration loses it to a two-symbol burst, so that failure records are compared too.

capture_on_the_cpu() is the same capture from the model encoders and the oracle's transmitter (ofdm_mod is pinned to
both elsewhere); precheck() sends it through the oracle's receiver, restates the frame sink over the oracle's taps to
find each packet's symbols and equaliser row, forms the soft values with soft_cases and runs the model decoders.

CPU pre-check (PYTHONPATH=. python tests/coded_stream_cases.py; test_coded_stream_cases_host.py repeats it), layout seed 1
throughout.  Per configuration: noise level and seed, the burst levels, packets sent, samples, packets the receiver
returned, of them: packet CRC ok, decoded ok at the end, decoded to a payload that was sent ("right"), corrected > 0 in
the code that faces the channel, packet CRC failed and decoded ok ("recovered"), LDPC iterations >= 2, RS corrected > 0,
RS second pass > 0:
    id              dB    seed bursts dB    sent samples returned crc_ok ok right corrected recovered iters2 rs_corrected second
    fec-hard        15.0  7    -              31  219040       29      5 28    28        24        23      0            0      0
    fec34-soft      14.0  7    -              31  197920       27      3 25    25        21        22      0            0      0
    fec-soft-rs     15.0  7    2,3,4          31  237600       28      1 22    22        27        21      0           16      0
    fec-hard-rsrel  16.0  9    2,3,4          31  237600       28      4 23    23        24        19      0           11      1
    fec-soft-rsrel  16.0  7    4,5,6          31  237600       27      2 16    16        25        14      0           14      4
    soft-rsrel      14.0  9    -              31  195360       27      2 23    23        22        21      0           22      1
    rs-hard         14.0  9    -              31  195360       27      2 23    23        21        21      0           21      0
    ldpc-hard       13.0  7    -              31  228640       26      0 25    25        26        25     17            0      0
    ldpc-soft       13.0  7    -              31  228640       26      0 25    25        26        25      8            0      0
    ldpc-soft-rs    13.0  9    -              31  248480       26      0 23    23        26        23     15            4      0
How they were found: starting from test_gpu_fec.py's 15 dB / seed 7 and test_gpu_ldpc.py's 12 dB / seed 7, noise seeds
7 .. 11 and levels in 0.5 .. 1 dB steps around them.  Noise alone leaves the outer code above the K = 7 code one packet
to correct and no second pass at 15 and 16 dB, hence the bursts there: (2, 3, 4) dB gives the hard chain one second-pass
success at 16 dB / seed 9 (none at seed 7, one at seed 8 with (0, 1, 2, 3)), (4, 5, 6) dB gives the soft chain four at
16 dB / seed 7 (two at seed 9, three at seed 8).  The RS link without an inner code has second-pass successes from noise
alone at 13.5 .. 15 dB (one each at 14 dB / seed 9, 13.5 dB / seed 11, 15 dB / seed 9); a one-symbol burst there costs a
one-codeword packet outright.  At 12 dB the receiver returns 18 .. 24 of the 31 LDPC packets (headers lost), at 13 dB 23 .. 26.
The receiver loses two to five packets of every capture: a header it cannot read, or the first packet of a burst.
No decoder reported ok for a payload that was not sent."""
import functools
import struct

import numpy as np

import fec_cases as fc
import fec_rel_cases as fr
import ldpc_cases as lc
import punct_cases as pc
import rs_cases as rc
import rs_rel_cases as rr
import soft_cases as sc
from helpers import make_cfg

# the table of the docstring, as test_coded_stream_cases_host.py and the GPU reference compare it
_KEYS = ("sent", "samples", "returned", "crc_ok", "ok", "right", "corrected", "recovered", "iters2", "rs_corrected", "second")
PRECHECK = {name: dict(zip(_KEYS, row)) for name, row in (
    ("fec-hard", (31, 219040, 29, 5, 28, 28, 24, 23, 0, 0, 0)),
    ("fec34-soft", (31, 197920, 27, 3, 25, 25, 21, 22, 0, 0, 0)),
    ("fec-soft-rs", (31, 237600, 28, 1, 22, 22, 27, 21, 0, 16, 0)),
    ("fec-hard-rsrel", (31, 237600, 28, 4, 23, 23, 24, 19, 0, 11, 1)),
    ("fec-soft-rsrel", (31, 237600, 27, 2, 16, 16, 25, 14, 0, 14, 4)),
    ("soft-rsrel", (31, 195360, 27, 2, 23, 23, 22, 21, 0, 22, 1)),
    ("rs-hard", (31, 195360, 27, 2, 23, 23, 21, 21, 0, 21, 0)),
    ("ldpc-hard", (31, 228640, 26, 0, 25, 25, 26, 25, 17, 0, 0)),
    ("ldpc-soft", (31, 228640, 26, 0, 25, 25, 26, 25, 8, 0, 0)),
    ("ldpc-soft-rs", (31, 248480, 26, 0, 23, 23, 26, 23, 15, 4, 0)),
)}

MOD, N, OCC, CP = "qam16", 512, 200, 128
L = N + CP
LEAD = 1500
ALWAYS = (0, 91, 92, 93, 219, 220, 300)
MAX_SAMPLES = 300000
CHUNKINGS = ("40000", "7000", "random", "one")
LOST = (-1, 1, 0, 2 * L, 3.0)            # the longest packet: its second and third data symbol under noise 3 dB above the signal

# id -> what ofdm_mod takes, what ofdm_demod takes, (SNR dB, noise seed), layout seed, and the impulse bursts besides LOST:
# levels in dB above the bursts' mean power, taken in turn by the packets of three or more data symbols (the longest
# excepted) in the order sent, each for one symbol of noise over its second data symbol; () for none
def _config(tx, rx, level, impulses=(), seed=1):
    return dict(tx=tx, rx=rx, level=level, impulses=impulses, seed=seed)


_RSREL = dict(erasures=True, source="fec")
CONFIGS = {
    "fec-hard": _config(dict(fec=True), dict(fec=True), (15.0, 7)),
    "fec34-soft": _config(dict(fec=dict(rate="3/4")), dict(fec=dict(rate="3/4"), soft=True), (14.0, 7)),
    "fec-soft-rs": _config(dict(fec=True, rs=True), dict(fec=True, soft=True, rs=True), (15.0, 7), (2.0, 3.0, 4.0)),
    "fec-hard-rsrel": _config(dict(fec=True, rs=True), dict(fec=True, rs=_RSREL), (16.0, 9), (2.0, 3.0, 4.0)),
    "fec-soft-rsrel": _config(dict(fec=True, rs=True), dict(fec=True, soft=True, rs=_RSREL), (16.0, 7), (4.0, 5.0, 6.0)),
    "soft-rsrel": _config(dict(rs=True), dict(soft=True, rs=dict(erasures=True)), (14.0, 9)),
    "rs-hard": _config(dict(rs=True), dict(rs=True), (14.0, 9)),
    "ldpc-hard": _config(dict(ldpc=True), dict(ldpc=True), (13.0, 7)),
    "ldpc-soft": _config(dict(ldpc=True), dict(ldpc=True, soft=True), (13.0, 7)),
    "ldpc-soft-rs": _config(dict(ldpc=True, rs=True), dict(ldpc=True, soft=True, rs=True), (13.0, 9)),
}
IDS = tuple(CONFIGS)


def _orc():
    from oracle import oracle
    oracle.lib()
    return oracle


def options_of():
    from ofdm_uhd_amd import options
    return options.default_options(modulation=MOD, fft_length=N, occupied_tones=OCC, cp_length=CP)


def span_of():
    """One maximum-length packet plus two sync tiles, as feed() computes it for this geometry (no GPU needed)."""
    from ofdm_uhd_amd import ofdm

    class _Geometry(object):
        _stream_geometry = ofdm.ofdm_demod._stream_geometry

        class _engine(object):
            cfg = make_cfg(MOD, N, OCC, CP)
    return _Geometry()._stream_geometry()[1]


# ---- the codes of a configuration, in the models ---------------------------------------------------------------------------
def coded_block(tx, payload):
    """What ofdm_mod(**tx) frames for one payload: outer, then inner code."""
    b = bytes(payload)
    if tx.get("rs"):
        b = rc.encode(b)
    fec = tx.get("fec")
    if fec:
        rate = fec.get("rate", "1/2") if isinstance(fec, dict) else "1/2"
        b = fc.encode(b) if rate == "1/2" else pc.encode(b, 16, rate)
    if tx.get("ldpc"):
        b = lc.encode(b)
    return b


def packet_symbols(nbytes, cfg=None):
    """Preamble plus data symbols of a packet whose framed body holds ``nbytes`` bytes."""
    import ctypes as C
    cfg = cfg or make_cfg(MOD, N, OCC, CP)
    lib = _orc().lib()
    fl = C.c_uint32(0)
    assert lib.orc_framed_len(C.byref(cfg), int(nbytes), C.byref(fl)) == 0
    return 1 + int(lib.orc_tx_data_symbols(C.byref(cfg), fl.value, len(sc.smap_of(cfg))))


def model_chain(rx, raw, vals):
    """The receiving end of ofdm_demod(**rx) in the models: ``raw`` the packets an uncoded receiver returns, ``vals`` their
    soft values (None on a hard path).  Returns the fields of ofdm_demod after work(): pkts, last_fec, last_ldpc,
    last_rs, last_rs_second, last_fec_rel."""
    soft = bool(rx.get("soft"))
    fec, ldpc, rs = rx.get("fec"), rx.get("ldpc"), rx.get("rs")
    rate = fec.get("rate", "1/2") if isinstance(fec, dict) else "1/2"
    rel_fec = isinstance(rs, dict) and rs.get("source") == "fec"
    rel_soft = isinstance(rs, dict) and not rel_fec
    out = dict(pkts=[(bool(ok), p) for ok, p in raw], last_fec=[], last_ldpc=[], last_rs=[], last_rs_second=[], last_fec_rel=[])
    if fec:
        if rel_fec:
            dec = [fr.decode_values_rate(v, 16, rate) for v in vals] if soft else [fr.decode_rate(p, 16, rate) for _, p in raw]
            out["last_fec_rel"] = [d[3] for d in dec]
        elif soft:
            dec = [fc.decode_values(v) if rate == "1/2" else pc.decode_values(v, 16, rate) for v in vals]
        else:
            dec = [fc.decode(p) if rate == "1/2" else pc.decode(p, 16, rate) for _, p in raw]
        out["last_fec"] = [(bool(ok), d[2]) for (ok, _), d in zip(raw, dec)]
        out["pkts"] = [(bool(d[0]), d[1]) for d in dec]
    elif ldpc:
        dec = lc.decode_many(list(vals)) if soft else [lc.decode(p) for _, p in raw]
        out["last_fec"] = [(bool(ok), d[2]) for (ok, _), d in zip(raw, dec)]
        out["last_ldpc"] = [(d[3], d[4]) for d in dec]
        out["pkts"] = [(bool(d[0]), d[1]) for d in dec]
    if rs:
        below = out["pkts"]
        if rel_fec:
            dec = [rr.decode(p, q, rr.DEFAULT_M) for (_, p), q in zip(below, out["last_fec_rel"])]
        elif rel_soft:
            dec = [rr.decode(p, rr.rel_from_values(v), rr.DEFAULT_M) for (_, p), v in zip(below, vals)]
        else:
            dec = [rc.decode(p) + (0,) for _, p in below]
        if isinstance(rs, dict):
            out["last_rs_second"] = [d[4] for d in dec]
        out["last_rs"] = [(bool(ok), d[2], d[3]) for (ok, _), d in zip(below, dec)]
        out["pkts"] = [(bool(d[0]), d[1]) for d in dec]
    return out


def counts(rx, raw, want):
    """What the non-triviality conditions look at, of one model_chain() (or of a demodulator's fields in the same dict)."""
    first = want["last_fec"] if (rx.get("fec") or rx.get("ldpc")) else want["last_rs"]        # the code that faces the channel
    return dict(returned=len(raw), crc_ok=sum(bool(ok) for ok, _ in raw), ok=sum(ok for ok, _ in want["pkts"]),
                corrected=sum(f[1] > 0 for f in first),
                recovered=sum(ok and not rok for (ok, _), (rok, _) in zip(want["pkts"], raw)),
                iters2=sum(it >= 2 for it, _ in want["last_ldpc"]), rs_corrected=sum(r[1] > 0 for r in want["last_rs"]),
                second=sum(s > 0 for s in want["last_rs_second"]))


def nontrivial(name, c):
    """The conditions every configuration's reference must meet before a streamed comparison means anything."""
    rx = CONFIGS[name]["rx"]
    assert c["returned"] >= 20, c
    assert 2 * c["corrected"] >= c["returned"], c
    assert c["recovered"] >= 1 and c["ok"] < c["returned"], c
    if rx.get("ldpc"):
        assert c["iters2"] >= 1, c
    if rx.get("rs"):
        assert c["rs_corrected"] >= 1, c
    if isinstance(rx.get("rs"), dict):
        assert c["second"] >= 1, c


# ---- the capture ---------------------------------------------------------------------------------------------------------
def payloads_of(seed):
    rng = np.random.default_rng(seed)
    npkt = int(rng.integers(28, 35))
    sizes = list(ALWAYS) + [int(n) for n in rng.integers(0, 301, npkt - len(ALWAYS))]
    sizes = [sizes[i] for i in rng.permutation(npkt)]
    pay = []
    for i, n in enumerate(sizes):
        pay.append((struct.pack("!HH", i, 0) + rng.integers(0, 256, max(n - 4, 0), dtype=np.uint8).tobytes())[:n])
    return pay, rng


def _layout(name, seed, tx_burst):
    """(payloads, clean iq, first sample of every packet, symbols of every packet) of the first layout seed >= ``seed``
    whose capture has a legal length; ``tx_burst`` modulates one burst of payloads."""
    tx = CONFIGS[name]["tx"]
    span = span_of()
    for s in range(seed, seed + 200):
        pay, rng = payloads_of(s)
        parts, start, k, pos = [np.zeros(LEAD, np.complex64)], [], 0, LEAD
        nsym = [packet_symbols(len(coded_block(tx, p))) for p in pay]
        while k < len(pay):
            n = int(rng.integers(1, 6))
            gap = int(rng.integers(200, 30001))
            burst = pay[k:k + n]
            for j in range(len(burst)):
                start.append(pos + L * sum(nsym[k:k + j]))
            blen = L * sum(nsym[k:k + len(burst)])
            k += n
            last = k >= len(pay)
            parts.append(burst)
            parts.append(np.zeros(L if last else gap, np.complex64))
            pos += blen + (L if last else gap)
        if not 4 * span <= pos <= MAX_SAMPLES:
            continue
        iq = []
        for part in parts:
            if isinstance(part, list):
                b = tx_burst(part)
                iq.append(np.asarray(b, np.complex64))
            else:
                iq.append(part)
        x = np.concatenate(iq)
        assert len(x) == pos, (len(x), pos)                 # every packet is where packet_symbols() puts it
        return pay, x, start, nsym
    raise AssertionError("no layout seed gives %s a capture of 4 spans .. %d samples" % (name, MAX_SAMPLES))


def _impair(name, x, start, nsym):
    """channel(), then the impulse bursts: in place."""
    c = CONFIGS[name]
    snr_db, noise_seed = c["level"]
    psig = float(np.mean(np.abs(x[x != 0].astype(np.complex128)) ** 2))
    _orc().channel(x, sigma=float(np.sqrt(psig / 10 ** (snr_db / 10.0))), seed=noise_seed)
    rng = np.random.default_rng(1000 + noise_seed)
    longest = int(np.argmax(nsym))
    hit = [i for i, ns in enumerate(nsym) if i != longest and ns >= 4]
    bursts = [(i, 1, 0, L, c["impulses"][k % len(c["impulses"])]) for k, i in enumerate(hit)] if c["impulses"] else []
    for pkt, sym, off, n, db in [LOST] + bursts:
        pkt = longest if pkt < 0 else pkt
        assert 1 + sym < nsym[pkt] and off + n <= (nsym[pkt] - 1 - sym) * L, (pkt, sym, off, n)
        a = start[pkt] + (1 + sym) * L + off
        g = np.sqrt(psig * 10 ** (db / 10.0) / 2.0)
        x[a:a + n] += (g * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)
    return x


@functools.lru_cache(maxsize=None)
def capture(name, seed=None):
    """(payloads sent, IQ) of configuration ``name``: ofdm_mod(**tx), one flush() per burst (needs the GPU).  The array is
    shared: read-only."""
    from ofdm_uhd_amd import ofdm
    c = CONFIGS[name]
    mod = ofdm.ofdm_mod(options_of(), pad_for_usrp=False, **c["tx"])

    def tx_burst(burst):
        for p in burst:
            mod.send_pkt(p)
        return mod.flush()

    try:
        pay, x, start, nsym = _layout(name, c["seed"] if seed is None else seed, tx_burst)
    finally:
        mod.engine().close()
    x = _impair(name, x, start, nsym)
    x.setflags(write=False)
    return pay, x


@functools.lru_cache(maxsize=None)
def capture_on_the_cpu(name, seed=None):
    """The same capture from the model encoders and the oracle's transmitter."""
    c = CONFIGS[name]
    cfg = make_cfg(MOD, N, OCC, CP)
    cfg.tx_amplitude = 1.0                        # ofdm_mod on its own has unit gain
    orc = _orc()
    pay, x, start, nsym = _layout(name, c["seed"] if seed is None else seed,
                                  lambda burst: orc.tx(cfg, [coded_block(c["tx"], p) for p in burst]))
    x = _impair(name, x, start, nsym)
    x.setflags(write=False)
    return pay, x


def chunks(chunking, n):
    """The cuts of a capture of n samples: [(a, b)]."""
    if chunking == "one":
        return [(0, n)]
    rng = np.random.default_rng(1)
    cuts, pos = [], 0
    while pos < n:
        step = int(rng.integers(1, 90001)) if chunking == "random" else int(chunking)
        cuts.append((pos, min(n, pos + step)))
        pos += step
    return cuts


# ---- the CPU pre-check -----------------------------------------------------------------------------------------------------
def receive_on_the_cpu(x):
    """The oracle's receiver on a capture, and the frame sink restated over its taps: returns (packets, soft values) --
    the values by soft_cases from each packet's demapped symbols and the equaliser row of the preamble that opened it."""
    from ofdm_uhd_amd import _abi
    cfg = make_cfg(MOD, N, OCC, CP)
    res = _orc().rx(cfg, np.ascontiguousarray(x), (1 << _abi.TAP_RX_FFT) | (1 << _abi.TAP_RX_SINK) | (1 << _abi.TAP_RX_FRAMES))
    pk = res.packets
    fft, sink, frames = res.tap(_abi.TAP_RX_FFT), res.tap(_abi.TAP_RX_SINK), res.tap(_abi.TAP_RX_FRAMES)
    smap, cst, mask = sc.smap_of(cfg), sc.cst_of(cfg), sc.mask_of(cfg)
    nbits = int(cfg.arity).bit_length() - 1
    flag = np.zeros(int((frames[:, 1].astype(np.int64) + 1).sum()), bool)
    flag[np.concatenate([[0], np.cumsum(frames[:, 1].astype(np.int64) + 1)])[:-1]] = True
    assert len(flag) == len(fft)
    # digital_ofdm_frame_sink over the sampled symbols: a flag in state 0 opens a packet, the next symbol holds the header
    vals, state, row, k, need, rows, eq = [], 0, 0, 0, 0, [], None
    for s in range(len(flag)):
        if state == 0:
            if flag[s]:
                state, eq, rows = 1, sc.hinv_from_preamble(cfg, fft[s]), []
            continue
        rows.append(sink[row, :len(smap)])
        row += 1
        if state == 1:
            hdr = _header(rows[0], cst, nbits)
            if (hdr >> 16) != (hdr & 0xFFFF):
                state = 0
                continue
            need = -(-8 * (sc.HEADER + ((hdr >> 16) & 0x0FFF)) // (len(smap) * nbits))
            state = 2
        if len(rows) == need:
            plen = len(pk[k][1])
            vals.append(sc.packet_values(np.concatenate(rows), eq, smap, cst, plen, mask))
            k += 1
            state = 0
    assert row == len(sink) and k == len(pk), (row, len(sink), k, len(pk))
    return pk, vals[:len(pk)]


def _header(x, cst, nbits):
    """The four header bytes the slicer reads off the first carriers of a symbol (nearest point, lowest index first)."""
    ncar = -(-32 // nbits)
    d = np.abs(x[:ncar, None] - cst[None, :]) ** 2
    j = np.argmin(d, axis=1)
    hdr = [0, 0, 0, 0]
    for beta in range(32):
        if (j[beta // nbits] >> (beta % nbits)) & 1:
            hdr[beta >> 3] |= 1 << (beta & 7)
    return (hdr[0] << 24) | (hdr[1] << 16) | (hdr[2] << 8) | hdr[3]


def precheck(name):
    """counts() of the model chain on the CPU capture, and the capture's length."""
    pay, x = capture_on_the_cpu(name)
    pk, vals = receive_on_the_cpu(x)
    rx = CONFIGS[name]["rx"]
    want = model_chain(rx, pk, vals if rx.get("soft") else None)
    c = counts(rx, pk, want)
    c.update(sent=len(pay), samples=len(x), right=sum(ok and p in pay for ok, p in want["pkts"]))
    return c


if __name__ == "__main__":
    import sys
    print("span %d" % span_of())
    for name in (sys.argv[1:] or IDS):
        c = precheck(name)
        print("  %-15s %s" % (name, " ".join("%s %d" % kv for kv in c.items())))
        try:
            nontrivial(name, c)
        except AssertionError:
            print("    ^ trivial")
