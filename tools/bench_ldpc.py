"""The LDPC kernels (k_ldpc_encode, k_ldpc_decode) on one MI355X, next to k_fec_encode / k_fec_decode at rate 1/2 from
the same run:
python tools/bench_ldpc.py

Device pointers; bench_fec.py's payload set (65 536 blocks of 1 026 payload bytes, the C2 packet, PCG64 seed 0x0FEC), the
K = 7 code with 16 interleaver columns, the LDPC decoder at max_iters 20.  Inputs: the clean coded blocks as hard bytes
and as +-16 / +-1 values (every LDPC codeword stops after one iteration), and input near the LDPC decoder's threshold:
hard bytes with 5 % of the bits flipped, and BPSK / AWGN values rint(4 LLR) at --ebn0 dB (2.0), both made on the device
from a seed.  After two warm-ups per variant: ROUNDS alternations of CALLS calls of every variant; the kernels' HIP-event
times from ofdm_ldpc_last_ms / ofdm_fec_last_ms (the Viterbi decoder's covers all its slices).  Prints one JSON line:
median / min / max ms per variant, ns per payload byte, the LDPC decoder's block verdicts and mean iteration counts, and
every LDPC time as a ratio to k_fec_decode / k_fec_encode on the same kind of input.

--rate R (2/3, 3/4 or 5/6): the same job also runs the LDPC code of rate R and the K = 7 code punctured to R, on blocks of
as many LDPC codewords as the rate-1/2 ones (11, the last one filled to the same fraction: 1 369, 1 541 or 1 712 payload
bytes), the noisy inputs at --rate-ebn0 dB (2.5 / 3.0 / 3.75, at the nominal rate R) and --rate-flip-rate (3 / 2 / 1 %).
The K = 7 times at R are the decode call's k_fec_decode time (the depuncture kernel's, ofdm_fec_punct_last_ms, is listed
next to it).  "rate_over_half" holds every rate-R LDPC time as a ratio to the rate-1/2 LDPC kernel on the same kind of
input in this job, "ldpc_over_fec_at_rate" as a ratio to the K = 7 code at R.

--rel: k_ldpc_decode_rel next to k_ldpc_decode of the same build instead, nothing of the K = 7 code: for each of the four
rates the batch above at that rate (clean and near the threshold, hard and soft), both kernels on the same buffers in
alternation, the two calls' payloads and per-block arrays compared once.  Prints one JSON line per rate: median / min /
max ms of either kernel per kind of input and "rel_over_plain", the ratio of the medians."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from ofdm_uhd_amd import config, engine, fec, ldpc, options  # noqa: E402


def _stats(v):
    return [round(float(np.median(v)), 4), round(float(np.min(v)), 4), round(float(np.max(v)), 4)]


def _bits(d_coded, lo, hi):
    """Bits of coded bytes [lo, hi), MSB first, as a float tensor of +-1."""
    sh = torch.arange(7, -1, -1, dtype=torch.uint8, device=d_coded.device)
    b = (d_coded[lo:hi].unsqueeze(1) >> sh) & 1
    return b.reshape(-1).to(torch.float32) * 2.0 - 1.0


def hard_values(d_coded, amp, chunk=1 << 24):
    out = torch.empty(d_coded.numel() * 8, dtype=torch.int8, device=d_coded.device)
    for lo in range(0, d_coded.numel(), chunk):
        hi = min(lo + chunk, d_coded.numel())
        out[8 * lo:8 * hi] = (_bits(d_coded, lo, hi) * amp).to(torch.int8)
    return out


def awgn_values(d_coded, ebn0_db, gen, chunk=1 << 24, rate=0.5):
    """BPSK over AWGN at Eb/N0 for a code of nominal ``rate`` (1/2): int8 values rint(4 LLR) clamped to +-127."""
    sigma2 = 1.0 / (2.0 * rate * 10.0 ** (ebn0_db / 10.0))
    out = torch.empty(d_coded.numel() * 8, dtype=torch.int8, device=d_coded.device)
    for lo in range(0, d_coded.numel(), chunk):
        hi = min(lo + chunk, d_coded.numel())
        y = _bits(d_coded, lo, hi)
        y += torch.randn(y.numel(), generator=gen, device=y.device) * sigma2 ** 0.5
        out[8 * lo:8 * hi] = torch.clamp(torch.round(y * (8.0 / sigma2)), -127, 127).to(torch.int8)
    return out


def flipped(d_coded, rate, gen, chunk=1 << 24):
    out = d_coded.clone()
    w = (1 << torch.arange(8, device=d_coded.device)).to(torch.int32)
    for lo in range(0, d_coded.numel(), chunk):
        hi = min(lo + chunk, d_coded.numel())
        m = (torch.rand((hi - lo, 8), generator=gen, device=d_coded.device) < rate).to(torch.int32)
        out[lo:hi] ^= (m * w).sum(dim=1).to(torch.uint8)
    return out


RATE_NOMINAL = {"1/2": 0.5, "2/3": 2.0 / 3.0, "3/4": 0.75, "5/6": 5.0 / 6.0}
RATE_EBN0 = {"2/3": 2.5, "3/4": 3.0, "5/6": 3.75}
RATE_FLIP = {"2/3": 0.03, "3/4": 0.02, "5/6": 0.01}


def rate_size(size, R):
    """Payload bytes of a rate-R block of as many codewords as the rate-1/2 block of ``size``, the last one as full."""
    KI = ldpc.cw_info(R)
    W = (size + 4 + 95) // 96
    return (W - 1) * KI + ((size + 4 - 96 * (W - 1)) * KI) // 96 - 4


def main_rel(a):
    dev = torch.device("cuda", 0)
    P = a.blocks
    opt = options.default_options(modulation="qpsk", fft_length=512, occupied_tones=200, cp_length=128, tx_amplitude=0.25)
    e = engine.Engine(cfg=config.make_cfg(opt, device_ptrs=True))
    e.prof_enable(True)
    rng = np.random.Generator(np.random.PCG64(0x0FEC))
    gen = torch.Generator(device=dev)
    gen.manual_seed(0x1D9C)
    for R in ("1/2", "2/3", "3/4", "5/6"):
        size = a.size if R == "1/2" else rate_size(a.size, R)
        ebn0 = a.ebn0 if R == "1/2" else (RATE_EBN0[R] if a.rate_ebn0 is None else a.rate_ebn0)
        flip = a.flip_rate if R == "1/2" else (RATE_FLIP[R] if a.rate_flip_rate is None else a.rate_flip_rate)
        cfg = ldpc.ldpc_cfg(a.max_iters, R)
        csize = ldpc.coded_len(size, R)
        d_pay = torch.from_numpy(rng.integers(0, 256, P * size, dtype=np.uint8)).to(dev)
        offs, lens = np.arange(P, dtype=np.uint64) * np.uint64(size), np.full(P, size, np.uint32)
        coffs, clens = np.arange(P, dtype=np.uint64) * np.uint64(csize), np.full(P, csize, np.uint32)
        d_coded = torch.empty(P * csize, dtype=torch.uint8, device=dev)
        e.ldpc_encode_device(d_pay.data_ptr(), offs, lens, d_coded.data_ptr(), d_coded.numel(), cfg)
        bufs = {("clean", False): d_coded, ("clean", True): hard_values(d_coded, 16), ("noisy", False): flipped(d_coded, flip, gen),
                ("noisy", True): awgn_values(d_coded, ebn0, gen, rate=RATE_NOMINAL[R])}
        d_dec = torch.empty(P * size, dtype=torch.uint8, device=dev)
        d_dec_rel = torch.empty(P * size, dtype=torch.uint8, device=dev)
        d_rel = torch.empty(P * size, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        state = {}

        def run(what, soft, rel):
            buf = bufs[(what, soft)]
            o = coffs * np.uint64(8) if soft else coffs
            if rel:
                res = e.ldpc_decode_rel_device(buf.data_ptr(), o, clens, d_dec_rel.data_ptr(), d_dec_rel.numel(), d_rel.data_ptr(),
                                               d_rel.numel(), cfg, soft=soft)
            else:
                res = e.ldpc_decode_device(buf.data_ptr(), o, clens, d_dec.data_ptr(), d_dec.numel(), cfg, soft=soft)
            state[(what, soft, rel)] = res
            return e.ldpc_last_ms()

        kinds = [(w, s) for w in ("clean", "noisy") for s in (False, True)]
        name = lambda w, s, rel: "k_ldpc_decode%s %s %s" % ("_rel" if rel else "", w, "soft" if s else "hard")
        verdicts = {}
        for w, s in kinds:
            for rel in (False, True):
                for _ in range(2):
                    run(w, s, rel)
            plain, withrel = state[(w, s, False)], state[(w, s, True)]
            assert all(np.array_equal(x, y) for x, y in zip(plain, withrel)) and bool((d_dec == d_dec_rel).all())
            failed = withrel[4] > 0
            q = d_rel.reshape(P, size)
            verdicts["%s %s" % (w, "soft" if s else "hard")] = dict(
                ok=int(withrel[1].sum()), cw_failed=int(withrel[4].sum()), mean_block_iters=round(float(withrel[3].mean()), 2),
                rel_min=int(q.min()), rel_max=int(q.max()),
                rel_below_128_in_ok_blocks=int((q[torch.from_numpy(~failed).to(dev)] < 128).sum()))
        ms = {name(w, s, rel): [] for w, s in kinds for rel in (False, True)}
        for _ in range(a.rounds):
            for w, s in kinds:
                for rel in (False, True):
                    ms[name(w, s, rel)] += [run(w, s, rel) for _ in range(a.calls)]
        med = {v: float(np.median(t)) for v, t in ms.items()}
        print(json.dumps({"rate": R, "blocks": P, "payload_bytes": size, "ldpc_coded_bytes": csize,
                          "ldpc_codewords": P * ((size + 4 + ldpc.cw_info(R) - 1) // ldpc.cw_info(R)), "max_iters": a.max_iters,
                          "ebn0_db": ebn0, "flip_rate": flip, "calls": a.calls * a.rounds,
                          "ms_median_min_max": {v: _stats(t) for v, t in ms.items()}, "verdicts": verdicts,
                          "rel_over_plain": {"%s %s" % (w, "soft" if s else "hard"): round(med[name(w, s, True)] / med[name(w, s, False)], 4)
                                             for w, s in kinds}}), flush=True)
        del bufs, d_coded, d_pay, d_dec, d_dec_rel, d_rel
        torch.cuda.empty_cache()
    e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=65536)
    ap.add_argument("--size", type=int, default=1026)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--ebn0", type=float, default=2.0)
    ap.add_argument("--flip-rate", type=float, default=0.05)
    ap.add_argument("--max-iters", type=int, default=20)
    ap.add_argument("--rate", choices=("1/2", "2/3", "3/4", "5/6"), default="1/2")
    ap.add_argument("--rate-ebn0", type=float, default=None)
    ap.add_argument("--rate-flip-rate", type=float, default=None)
    ap.add_argument("--rel", action="store_true", help="k_ldpc_decode_rel next to k_ldpc_decode, every rate (see above)")
    a = ap.parse_args()
    if a.rel:
        return main_rel(a)
    R = a.rate if a.rate != "1/2" else None
    if R:
        nominal = RATE_NOMINAL[R]
        r_ebn0 = RATE_EBN0[R] if a.rate_ebn0 is None else a.rate_ebn0
        r_flip = RATE_FLIP[R] if a.rate_flip_rate is None else a.rate_flip_rate
        KI = ldpc.cw_info(R)
        rsize = rate_size(a.size, R)                                             # as many codewords, the last as full
    dev = torch.device("cuda", 0)
    P, size = a.blocks, a.size
    fsize, lsize = fec.coded_len(size), ldpc.coded_len(size)
    opt = options.default_options(modulation="qpsk", fft_length=512, occupied_tones=200, cp_length=128, tx_amplitude=0.25)
    e = engine.Engine(cfg=config.make_cfg(opt, device_ptrs=True))
    e.prof_enable(True)
    rng = np.random.Generator(np.random.PCG64(0x0FEC))
    d_pay = torch.from_numpy(rng.integers(0, 256, P * size, dtype=np.uint8)).to(dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(0x1D9C)
    offs = np.arange(P, dtype=np.uint64) * np.uint64(size)
    lens = np.full(P, size, np.uint32)
    d_dec = torch.empty(P * (max(size, rsize) if R else size), dtype=torch.uint8, device=dev)
    code = {}
    for name, csize, enc in (("fec", fsize, e.fec_encode_device), ("ldpc", lsize, e.ldpc_encode_device)):
        d_coded = torch.empty(P * csize, dtype=torch.uint8, device=dev)
        enc(d_pay.data_ptr(), offs, lens, d_coded.data_ptr(), d_coded.numel())
        code[name] = dict(csize=csize, coffs=np.arange(P, dtype=np.uint64) * np.uint64(csize), clens=np.full(P, csize, np.uint32),
                          clean=d_coded, clean_soft=hard_values(d_coded, 16 if name == "ldpc" else 1),
                          noisy=flipped(d_coded, a.flip_rate, gen), noisy_soft=awgn_values(d_coded, a.ebn0, gen),
                          pay=d_pay, offs=offs, lens=lens, size=size, kw={})
    state = {}
    lcfg = ldpc.ldpc_cfg(a.max_iters)
    names = ["fec", "ldpc"]
    if R:           # the same at rate R: payloads of their own, the K = 7 code punctured to R and the LDPC code of rate R
        d_rpay = torch.from_numpy(rng.integers(0, 256, P * rsize, dtype=np.uint8)).to(dev)
        roffs, rlens = np.arange(P, dtype=np.uint64) * np.uint64(rsize), np.full(P, rsize, np.uint32)
        rcfg = ldpc.ldpc_cfg(a.max_iters, R)
        for name, csize, enc, kw in (("fec " + R, fec.coded_len(rsize, R), e.fec_encode_device, dict(fec=dict(rate=R))),
                                     ("ldpc " + R, ldpc.coded_len(rsize, R), e.ldpc_encode_device, dict(ldpc=rcfg))):
            d_coded = torch.empty(P * csize, dtype=torch.uint8, device=dev)
            enc(d_rpay.data_ptr(), roffs, rlens, d_coded.data_ptr(), d_coded.numel(), **kw)
            code[name] = dict(csize=csize, coffs=np.arange(P, dtype=np.uint64) * np.uint64(csize), clens=np.full(P, csize, np.uint32),
                              clean=d_coded, clean_soft=hard_values(d_coded, 16 if name.startswith("ldpc") else 1),
                              noisy=flipped(d_coded, r_flip, gen), noisy_soft=awgn_values(d_coded, r_ebn0, gen, rate=nominal),
                              pay=d_rpay, offs=roffs, lens=rlens, size=rsize, kw=kw)
            names.append(name)

    def encode(name):
        c = code[name]
        fn = e.fec_encode_device if name.startswith("fec") else e.ldpc_encode_device
        fn(c["pay"].data_ptr(), c["offs"], c["lens"], c["clean"].data_ptr(), c["clean"].numel(), **c["kw"])
        return e.fec_last_ms() if name.startswith("fec") else e.ldpc_last_ms()

    def right(c):
        n = P * c["size"]
        return int((d_dec[:n] == c["pay"]).reshape(P, c["size"]).all(dim=1).sum())

    def decode(name, what, soft):
        c = code[name]
        buf = c[what + ("_soft" if soft else "")]
        o = c["coffs"] * np.uint64(8) if soft else c["coffs"]
        if name.startswith("fec"):
            _, ok, corr = e.fec_decode_device(buf.data_ptr(), o, c["clens"], d_dec.data_ptr(), d_dec.numel(), soft=soft, **c["kw"])
            state[(name, what, soft)] = dict(ok=int(ok.sum()), right=right(c))
            if c["kw"]:
                state[(name, what, soft)]["k_fec_depuncture_ms"] = round(e.fec_punct_last_ms(), 4)
            return e.fec_last_ms()
        _, ok, corr, it, failed = e.ldpc_decode_device(buf.data_ptr(), o, c["clens"], d_dec.data_ptr(), d_dec.numel(),
                                                       c["kw"].get("ldpc", lcfg), soft=soft)
        state[(name, what, soft)] = dict(ok=int(ok.sum()), right=right(c),
                                         mean_block_iters=round(float(it.mean()), 2), cw_failed=int(failed.sum()))
        return e.ldpc_last_ms()

    torch.cuda.synchronize()            # the inputs are torch's work; the engine reads them on streams of its own
    variants = [("k_%s_encode" % n, (lambda n=n: encode(n))) for n in names]
    for what in ("clean", "noisy"):
        for soft in (False, True):
            for n in names:
                variants.append(("k_%s_decode %s %s" % (n, what, "soft" if soft else "hard"),
                                 (lambda n=n, what=what, soft=soft: decode(n, what, soft))))
    for _, f in variants:
        for _ in range(2):
            f()
    for soft in (False, True):
        for n in names:
            assert state[(n, "clean", soft)]["right"] == P and state[(n, "clean", soft)]["ok"] == P
    assert all(state[(n, "clean", True)]["mean_block_iters"] == 1.0 for n in names if n.startswith("ldpc"))
    ms = {v: [] for v, _ in variants}
    for _ in range(a.rounds):
        for v, f in variants:
            ms[v] += [f() for _ in range(a.calls)]
    med = {v: float(np.median(t)) for v, t in ms.items()}
    out = {"blocks": P, "payload_bytes": size, "fec_coded_bytes": fsize, "ldpc_coded_bytes": lsize,
           "ldpc_codewords": P * ((size + 4 + 95) // 96), "max_iters": a.max_iters, "ebn0_db": a.ebn0, "flip_rate": a.flip_rate,
           "calls": a.calls * a.rounds, "ms_median_min_max": {v: _stats(t) for v, t in ms.items()},
           "ns_per_payload_byte": {v: round(med[v] * 1e6 / (P * (rsize if R and (" " + R + "_") in v else size)), 4) for v in med},
           "verdicts": {"%s %s %s" % (n, w, "soft" if s else "hard"): st for (n, w, s), st in state.items()},
           "ldpc_over_fec": {"encode": round(med["k_ldpc_encode"] / med["k_fec_encode"], 4)}}
    for what in ("clean", "noisy"):
        for soft in ("hard", "soft"):
            out["ldpc_over_fec"]["decode %s %s" % (what, soft)] = round(
                med["k_ldpc_decode %s %s" % (what, soft)] / med["k_fec_decode %s %s" % (what, soft)], 4)
    if R:
        out.update({"rate": R, "rate_payload_bytes": rsize, "rate_fec_coded_bytes": code["fec " + R]["csize"],
                    "rate_ldpc_coded_bytes": code["ldpc " + R]["csize"], "rate_ldpc_codewords": P * ((rsize + 4 + KI - 1) // KI),
                    "rate_ebn0_db": r_ebn0, "rate_flip_rate": r_flip})
        kinds = ["encode"] + ["decode %s %s" % (w, s) for w in ("clean", "noisy") for s in ("hard", "soft")]
        key = lambda n, k: "k_%s_%s" % (n, k)
        out["rate_over_half"] = {k: round(med[key("ldpc " + R, k)] / med[key("ldpc", k)], 4) for k in kinds}
        out["ldpc_over_fec_at_rate"] = {k: round(med[key("ldpc " + R, k)] / med[key("fec " + R, k)], 4) for k in kinds}
    print(json.dumps(out), flush=True)
    e.close()


if __name__ == "__main__":
    main()
