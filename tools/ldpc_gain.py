"""Block failure rates of the two inner codes from the NumPy models of tests/ (no GPU): BPSK over AWGN, decoder values
rint(4 LLR) clamped to +-127, 92-byte payloads (one LDPC codeword; a 194-byte K = 7 block with 16 interleaver columns),
Eb/N0 at the nominal rate 1/2 for both codes, LDPC max_iters 20.
python tools/ldpc_gain.py [--blocks 400] [--seed 1]
Prints one JSON line per Eb/N0: blocks, failures of either code (a block fails when its inner CRC does or the payload is
not the one sent), and the LDPC model's mean iteration count."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import fec_cases as fc  # noqa: E402
import ldpc_cases as lc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=400)
    ap.add_argument("--size", type=int, default=92)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--grid", default="1.5,2.0,2.5,3.0,3.5,4.0")
    a = ap.parse_args()
    for db in (float(x) for x in a.grid.split(",")):
        rng = np.random.default_rng([a.seed, int(round(10 * db))])
        pay = [rng.integers(0, 256, a.size, dtype=np.uint8).tobytes() for _ in range(a.blocks)]
        lv = [lc.awgn_values(lc.encode(p), db, 0.5, rng) for p in pay]
        fv = [lc.awgn_values(fc.encode(p), db, 0.5, rng) for p in pay]
        lres = lc.decode_many(lv)
        lfail = sum(not (r[0] and r[1] == p) for r, p in zip(lres, pay))
        ffail = 0
        for v, p in zip(fv, pay):
            r = fc.decode_values(v)
            ffail += not (r[0] and r[1] == p)
        print(json.dumps({"ebn0_db": db, "blocks": a.blocks, "ldpc_failed": int(lfail), "fec_failed": int(ffail),
                          "ldpc_mean_iters": round(float(np.mean([r[3] for r in lres])), 2)}), flush=True)


if __name__ == "__main__":
    main()
