"""The punctured-rate kernels (k_fec_puncture, k_fec_depuncture) on one MI355X, next to a device copy of the bytes each
reads and writes, and the whole decode call per rate next to the rate-1/2 call of equal payload:
python tools/bench_punct.py [--parent-tree DIR]

Device pointers; 65 536 blocks of 1 026 payload bytes (the C2 packet), 16 interleaver columns.  After two warm-ups per
variant: ROUNDS alternations over the variants, CALLS calls each.  Per rate: the encode call (k_fec_puncture's HIP-event
time from ofdm_fec_punct_last_ms), the hard and the soft decode call (k_fec_depuncture's time from ofdm_fec_punct_last_ms,
k_fec_decode's from ofdm_fec_last_ms, the whole call by the host's clock around it: table upload, kernels, verdict
read-back), and torch device copies of as many bytes as the kernel reads plus writes (half of them copied: a copy
reads and writes each byte).  Rate 1/2 runs the same calls without the new kernels.

--parent-tree DIR: the rate-1/2 decode calls are also run from another checkout of the project (the parent commit's,
built), in a child process of its own before and after this tree's measurements, by this file's --half-only mode, which
uses nothing the parent lacks.  Prints one JSON line: median / min / max ms per variant, the kernels' ratio to their
copy, and the decode calls' excess over the rate-1/2 call next to the depuncture kernel's time."""
import argparse
import json
import os
import subprocess
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--blocks", type=int, default=65536)
ap.add_argument("--size", type=int, default=1026)
ap.add_argument("--calls", type=int, default=3)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--parent-tree", default=None)
ap.add_argument("--half-only", action="store_true", help="rate 1/2 decode calls only, from the tree in --tree")
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ARGS = ap.parse_args()
sys.path.insert(0, os.path.abspath(ARGS.tree))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from ofdm_uhd_amd import config, engine, options  # noqa: E402


def _stats(v):
    return [round(float(np.median(v)), 4), round(float(np.min(v)), 4), round(float(np.max(v)), 4)]


class Bench:
    def __init__(self, a):
        self.P, self.size = a.blocks, a.size
        self.dev = torch.device("cuda", 0)
        opt = options.default_options(modulation="qpsk", fft_length=512, occupied_tones=200, cp_length=128, tx_amplitude=0.25)
        self.e = engine.Engine(cfg=config.make_cfg(opt, device_ptrs=True))
        self.e.prof_enable(True)
        rng = np.random.Generator(np.random.PCG64(0x0FEC))
        self.d_pay = torch.from_numpy(rng.integers(0, 256, self.P * self.size, dtype=np.uint8)).to(self.dev)
        self.d_dec = torch.empty(self.P * self.size, dtype=torch.uint8, device=self.dev)
        self.offs = np.arange(self.P, dtype=np.uint64) * np.uint64(self.size)
        self.lens = np.full(self.P, self.size, np.uint32)
        self.ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def coded(self, csize, fec=None):
        """The batch encoded at ``fec``: (device blocks, offsets, lengths, device +-64 values)."""
        d_coded = torch.empty(self.P * csize, dtype=torch.uint8, device=self.dev)
        kw = {} if fec is None else {"fec": fec}
        # (the engine works on streams of its own: torch may hand out memory that work still queued on its stream uses)
        torch.cuda.synchronize()
        self.e.fec_encode_device(self.d_pay.data_ptr(), self.offs, self.lens, d_coded.data_ptr(), d_coded.numel(), **kw)
        coffs = np.arange(self.P, dtype=np.uint64) * np.uint64(csize)
        clens = np.full(self.P, csize, np.uint32)
        shifts = torch.arange(7, -1, -1, dtype=torch.uint8, device=self.dev)
        bits = (d_coded[:, None] >> shifts) & 1                     # MSB first
        d_soft = ((bits.to(torch.int8) * 2 - 1) * 64).reshape(-1).contiguous()
        torch.cuda.synchronize()
        return d_coded, coffs, clens, d_soft

    def decode_call(self, d_in, coffs, clens, soft, fec=None):
        """-> (whole call ms by the host's clock, k_fec_decode ms)"""
        kw = {} if fec is None else {"fec": fec}
        offs = (8 * coffs).astype(np.uint64) if soft else coffs
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, ok, corr = self.e.fec_decode_device(d_in.data_ptr(), offs, clens, self.d_dec.data_ptr(), self.d_dec.numel(), soft=soft, **kw)
        ms = (time.perf_counter() - t0) * 1e3
        assert int(ok.sum()) == self.P and int(corr.sum()) == 0, (fec, soft, int(ok.sum()), int(corr.sum()), np.flatnonzero(ok == 0)[:8].tolist())
        return ms, self.e.fec_last_ms()

    def copy_ms(self, nbytes):
        """A device copy that moves ``nbytes`` in all (reads half, writes half)."""
        half = max(nbytes // 2, 1)
        src = torch.empty(half, dtype=torch.uint8, device=self.dev)
        dst = torch.empty(half, dtype=torch.uint8, device=self.dev)
        out = []
        torch.cuda.synchronize()
        for i in range(5):
            self.ev[0].record()
            dst.copy_(src)
            self.ev[1].record()
            torch.cuda.synchronize()
            if i >= 2:
                out.append(self.ev[0].elapsed_time(self.ev[1]))
        del src, dst
        return out


def half_only(a):
    """Rate 1/2 decode calls, hard and soft, with nothing but what the coded-link layer had from the start."""
    from ofdm_uhd_amd import fec
    b = Bench(a)
    d_coded, coffs, clens, d_soft = b.coded(fec.coded_len(a.size))
    res = {}
    for name, d_in, soft in (("hard", d_coded, False), ("soft", d_soft, True)):
        for _ in range(2):
            b.decode_call(d_in, coffs, clens, soft)
        assert torch.equal(b.d_dec, b.d_pay)
        t = [b.decode_call(d_in, coffs, clens, soft) for _ in range(a.calls * a.rounds)]
        res["decode_%s_call_ms" % name] = _stats([x[0] for x in t])
        res["decode_%s_k_fec_decode_ms" % name] = _stats([x[1] for x in t])
    b.e.close()
    print(json.dumps(res), flush=True)


def parent_run(a):
    out = subprocess.check_output([sys.executable, os.path.abspath(__file__), "--half-only", "--tree", a.parent_tree, "--blocks", str(a.blocks),
                                   "--size", str(a.size), "--calls", str(a.calls), "--rounds", str(a.rounds)], timeout=300)
    return json.loads(out.decode().strip().splitlines()[-1])


def main(a):
    from ofdm_uhd_amd import fec
    parent = [parent_run(a)] if a.parent_tree else []
    b = Bench(a)
    P, size = b.P, b.size
    rates = ("1/2", "2/3", "3/4", "5/6")
    data, variants = {}, []
    for r in rates:
        cfg = dict(rate=r)
        csize = fec.coded_len(size, r)
        data[r] = b.coded(csize, cfg) + (csize,)

        def enc(cfg=cfg, r=r):
            b.e.fec_encode_device(b.d_pay.data_ptr(), b.offs, b.lens, data[r][0].data_ptr(), data[r][0].numel(), fec=cfg)
            return {"k_ms": b.e.fec_last_ms(), "punct_ms": b.e.fec_punct_last_ms() if r != "1/2" else 0.0}

        def dec(soft, cfg=cfg, r=r):
            d_coded, coffs, clens, d_soft, _ = data[r]
            call, k = b.decode_call(d_soft if soft else d_coded, coffs, clens, soft, cfg)
            return {"call_ms": call, "k_ms": k, "punct_ms": b.e.fec_punct_last_ms() if r != "1/2" else 0.0}

        variants += [("encode %s" % r, enc), ("decode hard %s" % r, lambda dec=dec: dec(False)), ("decode soft %s" % r, lambda dec=dec: dec(True))]
    for v, f in variants:
        for _ in range(2):
            f()
        assert v.startswith("encode") or torch.equal(b.d_dec, b.d_pay)
    got = {v: [] for v, _ in variants}
    for _ in range(a.rounds):
        for v, f in variants:
            got[v] += [f() for _ in range(a.calls)]
    res = {"blocks": P, "payload_bytes": size, "interleave_cols": 16, "calls": a.calls * a.rounds, "coded_bytes": {r: data[r][4] for r in rates}}
    msize = 8 * fec.coded_len(size)                     # mother values of one block
    for r in rates:
        csize = data[r][4]
        e, h, s = got["encode %s" % r], got["decode hard %s" % r], got["decode soft %s" % r]
        out = {"encode_kernel_ms": _stats([x["k_ms"] for x in e]),
               "decode_hard_call_ms": _stats([x["call_ms"] for x in h]), "decode_soft_call_ms": _stats([x["call_ms"] for x in s]),
               "decode_hard_k_fec_decode_ms": _stats([x["k_ms"] for x in h]), "decode_soft_k_fec_decode_ms": _stats([x["k_ms"] for x in s])}
        if r != "1/2":
            moved = {"puncture": P * (size + csize), "depuncture_hard": P * (csize + msize), "depuncture_soft": P * (8 * csize + msize)}
            kern = {"puncture": [x["punct_ms"] for x in e], "depuncture_hard": [x["punct_ms"] for x in h],
                    "depuncture_soft": [x["punct_ms"] for x in s]}
            for k in kern:
                cp = b.copy_ms(moved[k])
                out["k_fec_%s_ms" % k] = _stats(kern[k])
                out["copy_%s_ms" % k] = _stats(cp)
                out["%s_over_copy" % k] = round(float(np.median(kern[k]) / np.median(cp)), 2)
                out["%s_GBps_moved" % k] = round(moved[k] / float(np.median(kern[k])) * 1e-6, 1)
            for k, v, base in (("hard", h, got["decode hard 1/2"]), ("soft", s, got["decode soft 1/2"])):
                out["decode_%s_call_minus_half_rate_call_ms" % k] = round(
                    float(np.median([x["call_ms"] for x in v]) - np.median([x["call_ms"] for x in base])), 4)
        res[r] = out
    b.e.close()
    del b
    torch.cuda.empty_cache()
    if a.parent_tree:
        parent.append(parent_run(a))
        res["parent_tree_half_rate_before_after"] = parent
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    half_only(ARGS) if ARGS.half_only else main(ARGS)
