"""The outer code's kernels (k_rs_encode, k_rs_decode) on one MI355X, next to a device copy of the bytes each reads and
writes and next to the inner decoder on the same payloads:
python tools/bench_rs.py [--grid]

Device pointers; 65 536 blocks of 1 026 payload bytes (the batch of bench_punct.py): W = 5 codewords, 1 190-byte RS
blocks.  After two warm-ups per variant, ROUNDS * CALLS = 9 calls per variant, the variants alternating; median and
min - max per variant:
  - k_rs_encode (HIP-event time from ofdm_rs_last_ms);
  - k_rs_decode on clean input, with 8 and with 16 wrong bytes in every codeword, and on random bytes, with the whole
    decode call by the host's clock around it (table upload, kernel, verdict read-back);
  - a torch device copy of as many bytes as each kernel reads plus writes (half of them copied: a copy reads and writes
    each byte);
  - k_fec_decode, rate 1/2 and hard decisions, on the same payloads (ofdm_fec_last_ms): the yardstick.
--grid: the link of tests/test_gpu_soft.py (16-QAM, two paths) over 8 .. 20 dB at rates 1/2 and 3/4, --grid-packets per
level: packets that come back as sent, inner code alone against the concatenation, hard and soft, and the samples on the
air of both.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from ofdm_uhd_amd import config, engine, fec, ofdm, options, rs  # noqa: E402


def _stats(v):
    return [round(float(np.median(v)), 4), round(float(np.min(v)), 4), round(float(np.max(v)), 4)]


def kernels(a):
    dev = torch.device("cuda", 0)
    P, size = a.blocks, a.size
    rsize, k = rs.coded_len(size), size + 4
    W = (rsize - k) // rs.PARITY
    csize = fec.coded_len(size)
    opt = options.default_options(modulation="qpsk", fft_length=512, occupied_tones=200, cp_length=128, tx_amplitude=0.25)
    e = engine.Engine(cfg=config.make_cfg(opt, device_ptrs=True))
    e.prof_enable(True)
    rng = np.random.Generator(np.random.PCG64(0x0255))
    d_pay = torch.from_numpy(rng.integers(0, 256, P * size, dtype=np.uint8)).to(dev)
    offs, lens = np.arange(P, dtype=np.uint64) * np.uint64(size), np.full(P, size, np.uint32)
    roffs, rlens = np.arange(P, dtype=np.uint64) * np.uint64(rsize), np.full(P, rsize, np.uint32)
    coffs, clens = np.arange(P, dtype=np.uint64) * np.uint64(csize), np.full(P, csize, np.uint32)
    d_rs = torch.empty(P * rsize, dtype=torch.uint8, device=dev)
    d_dec = torch.empty(P * size, dtype=torch.uint8, device=dev)
    d_coded = torch.empty(P * csize, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()   # (the engine works on streams of its own)
    e.rs_encode_device(d_pay.data_ptr(), offs, lens, d_rs.data_ptr(), d_rs.numel())
    e.fec_encode_device(d_pay.data_ptr(), offs, lens, d_coded.data_ptr(), d_coded.numel())

    def damaged(per_cw):
        """`per_cw` wrong bytes in every codeword: info symbols 0, 12, 24, ... of each, i.e. W bytes in a row at each."""
        d = d_rs.clone().view(P, rsize)
        for j in range(per_cw):
            d[:, 12 * j * W:12 * j * W + W] ^= 0xA5
        return d.view(-1).contiguous()

    inputs = {"clean": (d_rs, P, 0, 0), "8 per codeword": (damaged(8), P, 8 * W * P, 0), "16 per codeword": (damaged(16), P, 16 * W * P, 0),
              "garbage": (torch.from_numpy(rng.integers(0, 256, P * rsize, dtype=np.uint8)).to(dev), None, None, None)}
    torch.cuda.synchronize()
    state = {}

    def enc():
        e.rs_encode_device(d_pay.data_ptr(), offs, lens, d_rs.data_ptr(), d_rs.numel())
        return {"k_ms": e.rs_last_ms()}

    def dec(name):
        d_in, want_ok, want_corr, want_fail = inputs[name]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, ok, corr, fail = e.rs_decode_device(d_in.data_ptr(), roffs, rlens, d_dec.data_ptr(), d_dec.numel())
        ms = (time.perf_counter() - t0) * 1e3
        got = (int(ok.sum()), int(corr.sum()), int(fail.sum()))
        if want_ok is not None:
            assert got == (want_ok, want_corr, want_fail), (name, got)
        state[name] = {"ok": got[0], "corrected": got[1], "failed": got[2]}
        return {"call_ms": ms, "k_ms": e.rs_last_ms()}

    def inner():
        _, ok, _ = e.fec_decode_device(d_coded.data_ptr(), coffs, clens, d_dec.data_ptr(), d_dec.numel())
        assert int(ok.sum()) == P
        return {"k_ms": e.fec_last_ms()}

    variants = [("k_rs_encode", enc)] + [("k_rs_decode " + n, lambda n=n: dec(n)) for n in inputs] + [("k_fec_decode hard 1/2", inner)]
    for v, f in variants:
        for _ in range(2):
            f()
        if v != "k_rs_decode garbage" and v != "k_rs_encode":
            assert torch.equal(d_dec, d_pay), v
    got = {v: [] for v, _ in variants}
    for _ in range(a.rounds):
        for v, f in variants:
            got[v] += [f() for _ in range(a.calls)]

    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def copy_ms(nbytes):
        half = max(nbytes // 2, 1)
        src = torch.empty(half, dtype=torch.uint8, device=dev)
        dst = torch.empty(half, dtype=torch.uint8, device=dev)
        out = []
        torch.cuda.synchronize()
        for i in range(5):
            ev[0].record()
            dst.copy_(src)
            ev[1].record()
            torch.cuda.synchronize()
            if i >= 2:
                out.append(ev[0].elapsed_time(ev[1]))
        return out

    res = {"blocks": P, "payload_bytes": size, "rs_block_bytes": rsize, "codewords_per_block": W, "calls": a.calls * a.rounds,
           "inner_block_bytes": csize, "outcome": state}
    yard = float(np.median([x["k_ms"] for x in got["k_fec_decode hard 1/2"]]))
    moved = P * (size + rsize)          # both kernels: the payload on one side, the block on the other
    cp = copy_ms(moved)
    res["copy_same_bytes_ms"] = _stats(cp)
    res["bytes_moved"] = moved
    for v, _ in variants:
        kms = [x["k_ms"] for x in got[v]]
        out = {"kernel_ms": _stats(kms)}
        if v.startswith("k_rs"):
            out["over_copy"] = round(float(np.median(kms) / np.median(cp)), 2)
            out["over_k_fec_decode"] = round(float(np.median(kms)) / yard, 4)
            out["GBps_moved"] = round(moved / float(np.median(kms)) * 1e-6, 1)
        if "call_ms" in got[v][0]:
            out["call_ms"] = _stats([x["call_ms"] for x in got[v]])
        res[v] = out
    e.close()
    return res


def grid(a):
    """The link test's channel over a 1 dB grid: packets that come back as sent, inner code alone against concatenated."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import soft_cases as sc
    opt = options.default_options(modulation=sc.LINK_MOD, fft_length=sc.LINK_N, occupied_tones=sc.LINK_OCC, cp_length=sc.LINK_CP)
    rng = np.random.default_rng(2024)
    pay = [rng.integers(0, 256, sc.LINK_SIZES[i % 6], dtype=np.uint8).tobytes() for i in range(a.grid_packets)]
    sent = set(pay)
    out = {"sent": len(pay), "paths": [[d, [round(g.real, 4), round(g.imag, 4)]] for d, g in sc.LINK_PATHS], "rates": {}}
    for rate in ("1/2", "3/4"):
        fcfg = dict(rate=rate)
        rows, nsamp = [], {}
        for outer in (False, True):
            mod = ofdm.ofdm_mod(opt, pad_for_usrp=False, fec=fcfg, rs=outer)
            hard = ofdm.ofdm_demod(opt, fec=fcfg, rs=outer)
            soft = ofdm.ofdm_demod(opt, fec=fcfg, soft=True, rs=outer)
            for p in pay:
                mod.send_pkt(p)
            iq = mod.flush()
            nsamp["concatenated" if outer else "inner"] = len(iq)
            psig = float(np.mean(np.abs(iq.astype(np.complex128)) ** 2))
            for i, snr in enumerate(range(a.grid_lo, a.grid_hi + 1)):
                ch = mod.engine()
                ch.set_multipath(sc.link_channel_cfg(float(snr), psig))
                ch.multipath_reset(0)
                y = ch.multipath(sc.link_air(iq))
                h = sum(1 for ok, p in hard.work(y) if ok and p in sent)
                s = sum(1 for ok, p in soft.work(y) if ok and p in sent)
                if not outer:
                    rows.append({"snr_db": snr, "inner_hard_ok": h, "inner_soft_ok": s})
                else:
                    rows[i].update({"concatenated_hard_ok": h, "concatenated_soft_ok": s,
                                    "rs_corrected_hard": sum(c for _, c, _ in hard.last_rs), "rs_failed_hard": sum(f for _, _, f in hard.last_rs)})
            for o in (mod, hard, soft):
                o.engine().close()
        out["rates"][rate] = {"samples_on_the_air": nsamp, "levels": rows}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=65536)
    ap.add_argument("--size", type=int, default=1026)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--grid", action="store_true")
    ap.add_argument("--grid-packets", type=int, default=24)
    ap.add_argument("--grid-lo", type=int, default=8)
    ap.add_argument("--grid-hi", type=int, default=20)
    a = ap.parse_args()
    out = {"kernels": kernels(a)}
    if a.grid:
        out["grid"] = grid(a)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
