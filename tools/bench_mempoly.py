"""The memory-polynomial stage (k_mempoly and the reduction of its partials) against a device copy of the same bytes on
one MI355X, one size per step, each step under a time limit of its own and the next only after it ended well:

    timeout -k 10 240 python tools/bench_mempoly.py --samples 134217728 && \\
    timeout -k 10 120 python tools/bench_mempoly.py --samples 16777216

Device pointers; a stream of complex Gaussian samples at rms 0.2; (memory, orders) = (1, 1), (3, 3), (4, 4) and (8, 5)
with seeded coefficients of magnitude at most 1 (the values do not change the work); complex64 out and 16-bit IQ out.
Per configuration, after two warm-ups per variant: ROUNDS alternations of [CALLS calls of the stage, CALLS device
copies]; the stage's HIP-event time from ofdm_mempoly_last_ms (k_mempoly and k_stat_reduce), the copy's from torch
events.  The yardstick is a torch copy that moves the bytes the stage must move (8 in per sample, 8 or 4 out: half of
them read, half written).  Prints one JSON line per configuration: median / min / max ms, TB/s, ps per sample, float32
operations per second by the definition's count (4 K + 7 per term, M terms, less the 2 additions t_0 does not have),
and the ratio to the copy by medians and for the least favourable pairing of single runs (slowest stage call, fastest
copy)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from ofdm_uhd_amd import config, dpd, engine, options  # noqa: E402

RMS = 0.2
SHAPES = ((1, 1), (3, 3), (4, 4), (8, 5))


def _stats(v):
    return [round(float(np.median(v)), 4), round(float(np.min(v)), 4), round(float(np.max(v)), 4)]


def _table(M, K):
    rng = np.random.default_rng(10 * M + K)
    return (rng.uniform(0.0, 1.0, (M, K)) * np.exp(2j * np.pi * rng.uniform(0.0, 1.0, (M, K)))).astype(np.complex64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, nargs="+", default=[1 << 24])
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    opt = options.default_options(modulation="qpsk")
    for n in a.samples:
        g = torch.Generator(device=dev)
        g.manual_seed(7)
        x = torch.randn(2 * n, dtype=torch.float32, device=dev, generator=g).mul_(RMS / np.sqrt(2.0))
        for M, K in SHAPES:
            for fmt in ("fc32", "sc16"):
                e = engine.Engine(cfg=config.make_cfg(opt, device_ptrs=True))
                e.prof_enable(True)
                oss = 8 if fmt == "fc32" else 4
                out = torch.empty(n * oss, dtype=torch.uint8, device=dev)
                moved = (8 + oss) * n
                src = torch.zeros(moved // 2, dtype=torch.uint8, device=dev)
                dst = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                e.set_dpd(dpd.mempoly_cfg(_table(M, K), out_format=fmt, limit=1.0))
                torch.cuda.synchronize()

                def stage():
                    e.dpd_reset()
                    assert e.dpd_device(x.data_ptr(), n, out.data_ptr(), n) == n
                    return e.dpd_last_ms()

                def copy():
                    ev[0].record()
                    dst.copy_(src)
                    ev[1].record()
                    torch.cuda.synchronize()
                    return ev[0].elapsed_time(ev[1])

                variants = (("k_mempoly", stage), ("copy", copy))
                for _, f in variants:
                    for _ in range(2):
                        f()
                ms = {v: [] for v, _ in variants}
                for _ in range(a.rounds):
                    for v, f in variants:
                        ms[v] += [f() for _ in range(a.calls)]
                st = e.dpd_stats()
                assert st["n"] == n
                med = {v: float(np.median(t)) for v, t in ms.items()}
                res = {v + "_ms": _stats(t) for v, t in ms.items()}
                flops = (M * (4 * K + 7) - 2) * n
                res["k_mempoly_TBps"] = round(moved / med["k_mempoly"] * 1e-9, 3)
                res["k_mempoly_ps_per_sample"] = round(med["k_mempoly"] * 1e9 / n, 3)
                res["k_mempoly_Tflops"] = round(flops / med["k_mempoly"] * 1e-9, 3)
                res["copy_TBps"] = round(moved / med["copy"] * 1e-9, 3)
                res["stage_over_copy_median"] = round(med["k_mempoly"] / med["copy"], 4)
                res["stage_over_copy_worst"] = round(float(np.max(ms["k_mempoly"])) / float(np.min(ms["copy"])), 4)
                print(json.dumps({"memory": M, "orders": K, "format": fmt, "samples": n, "bytes_moved": moved,
                                  "float32_ops_per_sample": M * (4 * K + 7) - 2, "calls": a.calls * a.rounds,
                                  "ms_median_min_max": res}), flush=True)
                e.close()
                for t in (out, src, dst):        # handed back zeroed
                    t.zero_()
                torch.cuda.synchronize()
                del out, src, dst
                torch.cuda.empty_cache()
        x.zero_()
        torch.cuda.synchronize()
        del x
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
