"""Decoding with reliabilities (k_rs_decode_rel, k_rs_rel_soft) on one MI355X, next to k_rs_decode on the same blocks:
python tools/bench_rs_rel.py [--grid]

The method of tools/bench_rs.py: device pointers; 65 536 blocks of 1 026 payload bytes (W = 5 codewords, 1 190-byte RS
blocks); after two warm-ups per variant, ROUNDS * CALLS = 9 calls per variant, the variants alternating in one job;
median and min - max of the HIP-event time per variant (ofdm_rs_last_ms, ofdm_rs_rel_last_ms):
  - k_rs_decode on clean input: the yardstick;
  - k_rs_decode_rel on clean input (reliabilities all 200): what staging one more byte per symbol costs;
  - both with 16 wrong bytes in every codeword: the first pass suffices;
  - k_rs_decode_rel with 24 wrong bytes of reliability 0 in every codeword: every codeword takes the second pass;
  - k_rs_rel_soft (8 values in, 1 byte out) next to a torch device copy of as many bytes as it reads plus writes (half of
    them copied: a copy reads and writes each byte).
--grid: the link of tests/test_gpu_rs_rel.py (16-QAM, two paths, RS blocks without an inner code) over --grid-lo ..
--grid-hi dB, --grid-packets per level: packets that come back as sent, errors only against with reliabilities.
Prints one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from ofdm_uhd_amd import config, engine, ofdm, options, rs  # noqa: E402


def _stats(v):
    return [round(float(np.median(v)), 4), round(float(np.min(v)), 4), round(float(np.max(v)), 4)]


def kernels(a):
    dev = torch.device("cuda", 0)
    P, size = a.blocks, a.size
    rsize, k = rs.coded_len(size), size + 4
    W = (rsize - k) // rs.PARITY
    opt = options.default_options(modulation="qpsk", fft_length=512, occupied_tones=200, cp_length=128, tx_amplitude=0.25)
    e = engine.Engine(cfg=config.make_cfg(opt, device_ptrs=True))
    e.prof_enable(True)
    rng = np.random.Generator(np.random.PCG64(0x0255))
    d_pay = torch.from_numpy(rng.integers(0, 256, P * size, dtype=np.uint8)).to(dev)
    offs, lens = np.arange(P, dtype=np.uint64) * np.uint64(size), np.full(P, size, np.uint32)
    roffs, rlens = np.arange(P, dtype=np.uint64) * np.uint64(rsize), np.full(P, rsize, np.uint32)
    d_rs = torch.empty(P * rsize, dtype=torch.uint8, device=dev)
    d_dec = torch.empty(P * size, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()   # (the engine works on streams of its own)
    e.rs_encode_device(d_pay.data_ptr(), offs, lens, d_rs.data_ptr(), d_rs.numel())

    def damaged(per_cw):
        """`per_cw` wrong bytes in every codeword (info symbols 0, 8, 16, ...: W bytes in a row at each), and the
        reliabilities that mark exactly those."""
        d = d_rs.clone().view(P, rsize)
        q = torch.full((P, rsize), 200, dtype=torch.uint8, device=dev)
        for j in range(per_cw):
            d[:, 8 * j * W:8 * j * W + W] ^= 0xA5
            q[:, 8 * j * W:8 * j * W + W] = 0
        return d.view(-1).contiguous(), q.view(-1).contiguous()

    d16, q16 = damaged(16)
    d24, q24 = damaged(24)
    q_clean = torch.full((P * rsize,), 200, dtype=torch.uint8, device=dev)
    d_vals = torch.randint(-128, 128, (8 * P * rsize,), dtype=torch.int8, device=dev)
    d_rel = torch.empty(P * rsize, dtype=torch.uint8, device=dev)
    voffs = roffs * np.uint64(8)
    torch.cuda.synchronize()
    state = {}

    def dec(name, d_in, d_q, want):
        if d_q is None:
            _, ok, corr, fail = e.rs_decode_device(d_in.data_ptr(), roffs, rlens, d_dec.data_ptr(), d_dec.numel())
            sec = np.zeros(1)
        else:
            _, ok, corr, fail, sec = e.rs_decode_rel_device(d_in.data_ptr(), roffs, rlens, d_q.data_ptr(), None, d_dec.data_ptr(), d_dec.numel())
        got = (int(ok.sum()), int(corr.sum()), int(fail.sum()), int(sec.sum()))
        assert got == want, (name, got, want)
        state[name] = dict(zip(("ok", "corrected", "failed", "second"), got))
        return e.rs_last_ms()

    def rel_soft():
        e.rs_rel_from_soft_device(d_vals.data_ptr(), voffs, rlens, d_rel.data_ptr(), d_rel.numel())
        return e.rs_rel_last_ms()

    variants = [
        ("k_rs_decode clean", lambda: dec("k_rs_decode clean", d_rs, None, (P, 0, 0, 0))),
        ("k_rs_decode_rel clean", lambda: dec("k_rs_decode_rel clean", d_rs, q_clean, (P, 0, 0, 0))),
        ("k_rs_decode 16 per codeword", lambda: dec("k_rs_decode 16 per codeword", d16, None, (P, 16 * W * P, 0, 0))),
        ("k_rs_decode_rel 16 per codeword", lambda: dec("k_rs_decode_rel 16 per codeword", d16, q16, (P, 16 * W * P, 0, 0))),
        ("k_rs_decode_rel 24 erased per codeword", lambda: dec("k_rs_decode_rel 24 erased per codeword", d24, q24, (P, 24 * W * P, 0, W * P))),
        ("k_rs_rel_soft", rel_soft),
    ]
    for v, f in variants:
        for _ in range(2):
            f()
        if v != "k_rs_rel_soft":
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

    res = {"blocks": P, "payload_bytes": size, "rs_block_bytes": rsize, "codewords_per_block": W, "calls": a.calls * a.rounds, "outcome": state}
    yard = float(np.median(got["k_rs_decode clean"]))
    cp = copy_ms(9 * P * rsize)
    res["copy_of_k_rs_rel_soft_bytes_ms"] = _stats(cp)
    for v, _ in variants:
        out = {"kernel_ms": _stats(got[v]), "over_k_rs_decode_clean": [round(float(x) / yard, 3) for x in _stats(got[v])]}
        if v == "k_rs_rel_soft":
            out["over_copy"] = round(float(np.median(got[v]) / np.median(cp)), 2)
            out["GBps_moved"] = round(9 * P * rsize / float(np.median(got[v])) * 1e-6, 1)
        res[v] = out
    res["k_rs_decode_rel 16 per codeword"]["over_k_rs_decode_16"] = round(
        float(np.median(got["k_rs_decode_rel 16 per codeword"]) / np.median(got["k_rs_decode 16 per codeword"])), 3)
    e.close()
    return res


def grid(a):
    """The link test's channel over a 1 dB grid: packets that come back as sent, errors only against with reliabilities."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import soft_cases as sc
    opt = options.default_options(modulation=sc.LINK_MOD, fft_length=sc.LINK_N, occupied_tones=sc.LINK_OCC, cp_length=sc.LINK_CP)
    rng = np.random.default_rng(2024)
    pay = [rng.integers(0, 256, sc.LINK_SIZES[i % 6], dtype=np.uint8).tobytes() for i in range(a.grid_packets)]
    sent = set(pay)
    mod = ofdm.ofdm_mod(opt, pad_for_usrp=False, rs=True)
    plain = ofdm.ofdm_demod(opt, rs=True)
    wrel = ofdm.ofdm_demod(opt, soft=True, rs=dict(erasures=True, max_erasures=a.max_erasures))
    for p in pay:
        mod.send_pkt(p)
    iq = mod.flush()
    psig = float(np.mean(np.abs(iq.astype(np.complex128)) ** 2))
    rows = []
    for snr in range(a.grid_lo, a.grid_hi + 1):
        ch = mod.engine()
        ch.set_multipath(sc.link_channel_cfg(float(snr), psig))
        ch.multipath_reset(0)
        y = ch.multipath(sc.link_air(iq))
        h = sum(1 for ok, p in plain.work(y) if ok and p in sent)
        s = sum(1 for ok, p in wrel.work(y) if ok and p in sent)
        rows.append({"snr_db": snr, "errors_only_ok": h, "with_reliabilities_ok": s, "second_pass_codewords": sum(wrel.last_rs_second),
                     "failed_errors_only": sum(f for _, _, f in plain.last_rs), "failed_with_reliabilities": sum(f for _, _, f in wrel.last_rs)})
    for o in (mod, plain, wrel):
        o.engine().close()
    return {"sent": len(pay), "max_erasures": a.max_erasures, "samples_on_the_air": len(iq), "levels": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=65536)
    ap.add_argument("--size", type=int, default=1026)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--grid", action="store_true")
    ap.add_argument("--grid-packets", type=int, default=24)
    ap.add_argument("--grid-lo", type=int, default=14)
    ap.add_argument("--grid-hi", type=int, default=24)
    ap.add_argument("--max-erasures", type=int, default=28)
    a = ap.parse_args()
    out = {"kernels": kernels(a)}
    if a.grid:
        out["grid"] = grid(a)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
