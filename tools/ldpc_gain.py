"""Block failure rates of the two inner codes from the NumPy models of tests/ (no GPU): BPSK over AWGN, decoder values
rint(4 LLR) clamped to +-127, one full LDPC codeword per block, LDPC max_iters 20, the K = 7 code with 16 interleaver
columns on the same payloads.
python tools/ldpc_gain.py [--rate 1/2] [--blocks 400] [--seed 1] [--grid 1.5,2.0,...] [--size N]
--rate 1/2: 92-byte payloads (a 194-byte K = 7 block), Eb/N0 at the nominal rate 1/2 for both codes.
--rate 2/3, 3/4, 5/6: the LDPC code of that rate (ldpc_rate_cases.py) next to the K = 7 code punctured to the same rate
(punct_cases.py), payloads of KI - 4 = 124, 140 or 156 bytes, Eb/N0 at the nominal rate R for both codes.
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
import ldpc_rate_cases as rc  # noqa: E402
import punct_cases as pc  # noqa: E402

GRIDS = {"1/2": "1.5,2.0,2.5,3.0,3.5,4.0", "2/3": "2.0,2.5,3.0,3.5,4.0", "3/4": "2.5,3.0,3.5,4.0,4.5",
         "5/6": "3.0,3.5,4.0,4.5,5.5"}
NOMINAL = {"1/2": 0.5, "2/3": 2.0 / 3.0, "3/4": 0.75, "5/6": 5.0 / 6.0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rate", choices=rc.RATES, default="1/2")
    ap.add_argument("--blocks", type=int, default=400)
    ap.add_argument("--size", type=int, default=None, help="payload bytes [KI - 4: one full LDPC codeword]")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--grid", default=None)
    a = ap.parse_args()
    code, R = rc.code(a.rate), NOMINAL[a.rate]
    size = code.CW_INFO - 4 if a.size is None else a.size
    if a.rate == "1/2":       # the models the rate-1/2 figures of DESIGN.md come from
        l_enc, l_dec, f_enc, f_dec = lc.encode, lc.decode_many, fc.encode, fc.decode_values
    else:
        l_enc, l_dec = code.encode, code.decode_many
        f_enc, f_dec = (lambda p: pc.encode(p, 16, a.rate)), (lambda v: pc.decode_values(v, 16, a.rate))
    for db in (float(x) for x in (a.grid or GRIDS[a.rate]).split(",")):
        rng = np.random.default_rng([a.seed, int(round(10 * db))])
        pay = [rng.integers(0, 256, size, dtype=np.uint8).tobytes() for _ in range(a.blocks)]
        lv = [lc.awgn_values(l_enc(p), db, R, rng) for p in pay]
        fv = [lc.awgn_values(f_enc(p), db, R, rng) for p in pay]
        lres = l_dec(lv)
        lfail = sum(not (r[0] and r[1] == p) for r, p in zip(lres, pay))
        ffail = 0
        for v, p in zip(fv, pay):
            r = f_dec(v)
            ffail += not (r[0] and r[1] == p)
        print(json.dumps({"rate": a.rate, "payload_bytes": size, "ebn0_db": db, "blocks": a.blocks, "ldpc_failed": int(lfail),
                          "fec_failed": int(ffail), "ldpc_mean_iters": round(float(np.mean([r[3] for r in lres])), 2)}), flush=True)


if __name__ == "__main__":
    main()
