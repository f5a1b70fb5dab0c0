"""What the LDPC decoder's byte reliabilities are worth to the outer code, from the NumPy models of tests/ (no GPU): BPSK
over AWGN, decoder values rint(4 LLR) clamped to +-127, payload -> RS -> LDPC at the rate -> values at Eb/N0 (at the
code's nominal rate) -> the min-sum model with reliabilities (ldpc_rel_cases.py) -> the RS model alone (rs_cases.decode) and
with the reliabilities (rs_rel_cases.decode, at most M erasures per codeword).
python tools/ldpc_rel_gain.py [--rate 1/2] [--grid 1.25,1.5] [--size 880] [--M 28] [--seeds 0:120 | --stream 11 --blocks 150]
--seeds A:B   one default_rng(seed) per block, seeds A .. B - 1: the construction tests/test_ldpc_rel_host.py pins
--stream S    --blocks blocks drawn one after the other from one default_rng(S): payload, then its noise
Prints one JSON line per Eb/N0: blocks, LDPC blocks with a failed codeword, blocks returned correct by RS alone and with
reliabilities, the seeds (or block numbers) gained and lost, wrong payloads accepted by either, and the RS codewords the
second pass decoded."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import ldpc_rel_cases as lc  # noqa: E402
import rs_cases as rc  # noqa: E402

GRIDS = {"1/2": "1.25,1.5,1.75", "2/3": "2.0,2.25,2.5", "3/4": "2.5,2.75,3.0", "5/6": "3.25,3.5,3.75"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rate", choices=lc.RATES, default="1/2")
    ap.add_argument("--grid", default=None)
    ap.add_argument("--size", type=int, default=lc.CHAIN_PAYLOAD)
    ap.add_argument("--M", type=int, default=lc.CHAIN_M)
    ap.add_argument("--seeds", default="0:120")
    ap.add_argument("--stream", type=int, default=None)
    ap.add_argument("--blocks", type=int, default=150)
    a = ap.parse_args()
    c = lc.code(a.rate)
    lo, hi = (int(x) for x in a.seeds.split(":"))
    for db in (float(x) for x in (a.grid or GRIDS[a.rate]).split(",")):
        if a.stream is None:
            ids = list(range(lo, hi))
            blocks = [lc.chain_block(s, a.rate, db, a.size) for s in ids]
        else:
            rng = np.random.default_rng(a.stream)
            ids, blocks = list(range(a.blocks)), []
            for _ in ids:
                payload = rng.integers(0, 256, a.size, dtype=np.uint8).tobytes()
                blocks.append((payload, c.awgn_values(c.encode(rc.encode(payload)), db, rng)))
        inner = c.decode_many_rel([v for _, v in blocks])
        alone, withrel, wrong, second = [], [], 0, 0
        for i, (p, _), d in zip(ids, blocks, inner):
            o1, o2 = lc.chain_outer(d[1], d[5], a.M)
            wrong += int(bool(o1[0]) and o1[1] != p) + int(bool(o2[0]) and o2[1] != p)
            second += o2[4]
            if o1[0] and o1[1] == p:
                alone.append(i)
            if o2[0] and o2[1] == p:
                withrel.append(i)
        print(json.dumps({"rate": a.rate, "payload_bytes": a.size, "ebn0_db": db, "M": a.M, "blocks": len(ids),
                          "draw": "seeds %d:%d" % (lo, hi) if a.stream is None else "stream %d" % a.stream,
                          "ldpc_blocks_with_failed_cw": sum(d[4] > 0 for d in inner), "ldpc_ok": sum(d[0] for d in inner),
                          "rs_alone": len(alone), "rs_with_rel": len(withrel), "gained": sorted(set(withrel) - set(alone)),
                          "lost": sorted(set(alone) - set(withrel)), "wrong_accepted": wrong, "second_pass_codewords": int(second)}), flush=True)


if __name__ == "__main__":
    main()
