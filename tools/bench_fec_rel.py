#!/usr/bin/env python
"""k_fec_decode_rel<true> next to k_fec_decode<true> on the same batches, and one point of the link-gain grid on the GPU.

Kernel time is ofdm_fec_last_ms with profiling on (HIP events around the decoder's slices), host mode, C = 16; the two
decoders alternate in one job, median of --reps after --warmup.  The batches are DESIGN.md section 7's: 256 blocks of
n = 2040 and 4096 blocks of n = 219, int8 values of +-1 plus Gaussian noise (sigma 0.7) at scale 32.

--link runs the concatenated chain of tests/fec_rel_cases.py (RS block, rate 1/2, BPSK over AWGN, M = 28) on the GPU over
the seeds 0 .. --blocks - 1 at --ebn0 dB and counts the blocks returned as sent without and with the reliabilities: the
same count as fec_rel_cases.chain_outcome gives on the CPU.

    python tools/bench_fec_rel.py [--reps 10] [--warmup 2] [--link] [--blocks 200] [--ebn0 2.0]

Prints one JSON line per measurement."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import fec_cases as fc  # noqa: E402
import fec_rel_cases as fr  # noqa: E402
from ofdm_uhd_amd import engine, options  # noqa: E402


def kernel_times(eng, nblk, n, reps, warmup, rng):
    pays = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for _ in range(nblk)]
    coded = eng.fec_encode(pays, 16)
    vals = [np.clip(np.rint(32.0 * (fc.hard_values(c) + 0.7 * rng.standard_normal(8 * len(c)))), -127, 127).astype(np.int8) for c in coded]
    plain, rel = [], []
    for rep in range(warmup + reps):
        a = eng.fec_decode_soft(vals, 16)
        t = eng.fec_last_ms()
        b = eng.fec_decode_soft_rel(vals, 16)
        u = eng.fec_last_ms()
        if rep >= warmup:
            plain.append(t)
            rel.append(u)
    assert [(x[0], x[1], x[2]) for x in b] == a        # the same payloads, verdicts and counts
    return dict(blocks=nblk, payload_bytes=n, k_fec_decode_ms=float(np.median(plain)), k_fec_decode_range=[min(plain), max(plain)],
                k_fec_decode_rel_ms=float(np.median(rel)), k_fec_decode_rel_range=[min(rel), max(rel)],
                ratio=float(np.median(rel) / np.median(plain)), inner_ok=sum(1 for x in a if x[0]))


def link_point(eng, n, blocks, ebn0):
    seeds = list(range(blocks))
    pay = [fr.chain_payload(n, s) for s in seeds]
    coded = eng.fec_encode(eng.rs_encode(pay), 16)
    vals = [fr.chain_channel(c, n, s, ebn0) for c, s in zip(coded, seeds)]
    inner = eng.fec_decode_soft_rel(vals, 16)
    blk, rel = [d[1] for d in inner], [d[3] for d in inner]
    with_rel, without = eng.rs_decode_rel(blk, rel), eng.rs_decode(blk)
    sent = lambda r, p: bool(r[0]) and r[1] == p
    return dict(payload_bytes=n, ebn0_db=ebn0, blocks=blocks, rs_alone=sum(sent(a, p) for a, p in zip(without, pay)),
                rs_with_reliabilities=sum(sent(b, p) for b, p in zip(with_rel, pay)),
                gained=[s for s, a, b, p in zip(seeds, without, with_rel, pay) if not sent(a, p) and sent(b, p)],
                lost=[s for s, a, b, p in zip(seeds, without, with_rel, pay) if sent(a, p) and not sent(b, p)],
                ok_but_wrong=sum(int(bool(b[0]) and b[1] != p) for b, p in zip(with_rel, pay)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--link", action="store_true")
    ap.add_argument("--blocks", type=int, default=200)
    ap.add_argument("--ebn0", type=float, default=2.0)
    args = ap.parse_args()
    if engine.device_count() < 1:
        raise SystemExit("bench_fec_rel needs a GPU")
    eng = engine.Engine(options.default_options(modulation="qpsk"))
    try:
        eng.prof_enable(True)
        rng = np.random.default_rng(1)
        for nblk, n in ((256, 2040), (4096, 219)):
            print(json.dumps(kernel_times(eng, nblk, n, args.reps, args.warmup, rng)), flush=True)
        if args.link:
            print(json.dumps(link_point(eng, 219, args.blocks, args.ebn0)), flush=True)
    finally:
        eng.close()


if __name__ == "__main__":
    main()
