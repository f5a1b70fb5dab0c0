"""The signal field next to the strongest body it announces, from the NumPy models of tests/ (no GPU): BPSK over AWGN
at the same Es/N0 for both.
python tools/sig_gain.py [--words 20000] [--blocks 400] [--seed 1] [--grid -6,-5,...]
The field: random 12-bit words, values clip(rint(32 y), +-127), the exhaustive decoder of sig_cases; a word is wrong
when the decoded word is not the one sent.  The body: rate-1/2 LDPC blocks of 92-byte payloads (one codeword, 192 sent
bytes), values rint(4 LLR) clamped to +-127, max_iters 20 (ldpc_cases, as tools/ldpc_gain.py runs it); a block fails when
its CRC does or the payload is not the one sent.  Es/N0 is per sent bit: Eb/N0 of the rate-1/2 body is 3.01 dB above it.
Prints one JSON line per Es/N0."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import ldpc_cases as lc  # noqa: E402
import sig_cases as sc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--words", type=int, default=20000)
    ap.add_argument("--blocks", type=int, default=400)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--grid", default="-6,-5,-4,-3,-2,-1.5,-1,0")
    a = ap.parse_args()
    for db in (float(x) for x in a.grid.split(",")):
        rng = np.random.default_rng([a.seed, int(round(10 * db)) + 1000])
        words = rng.integers(0, 4096, a.words)
        wrong = 0
        sigma = np.sqrt(0.5 / 10.0 ** (db / 10.0))
        for lo in range(0, a.words, 4096):
            w = words[lo:lo + 4096]
            bits = np.tile(sc.codebook()[w], (1, 4)).astype(np.float64)
            y = (2.0 * bits - 1.0) + sigma * rng.standard_normal(bits.shape)
            best, _ = sc.decode_many(np.clip(np.rint(32.0 * y), -127, 127).astype(np.int8))
            wrong += int((best != w).sum())
        pay = [rng.integers(0, 256, 92, dtype=np.uint8).tobytes() for _ in range(a.blocks)]
        res = lc.decode_many([lc.awgn_values(lc.encode(p), db, 1.0, rng) for p in pay])      # (rate 1: db is per sent bit)
        failed = sum(not (r[0] and r[1] == p) for r, p in zip(res, pay))
        print(json.dumps({"esn0_db": db, "words": a.words, "words_wrong": wrong, "word_error_rate": wrong / a.words,
                          "ldpc_blocks": a.blocks, "ldpc_failed": int(failed), "ldpc_failure_rate": failed / a.blocks,
                          "ldpc_mean_iters": round(float(np.mean([r[3] for r in res])), 2)}), flush=True)


if __name__ == "__main__":
    main()
