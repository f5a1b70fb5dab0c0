"""The crest-factor reduction stage (k_cfr and the reduction of its partials) against a device copy of the same bytes on
one MI355X:  python tools/bench_cfr.py

Device pointers; streams of 2^24 and 2^27 complex Gaussian samples; half-widths 0, 16 and 128 (Hann windows); thresholds
at "nothing over" (far above the peak), 7 dB and 4 dB over the rms (0.7 % and 8 % of the samples over); complex64 out,
and 16-bit IQ out for H = 16.  Per configuration, after two warm-ups per variant: ROUNDS alternations of [CALLS calls of
the stage, CALLS device copies]; the stage's HIP-event time from ofdm_cfr_last_ms (k_cfr and k_cfr_reduce), the copy's
from torch events.  The yardstick is a torch copy that moves the bytes the stage must move (8 in per sample, 8 or 4 out:
half of them read, half written).  Prints one JSON line per configuration: median / min / max ms, TB/s, ps per sample,
the share of samples over the threshold and of 1024-sample tiles that hold a peak (from the input, on the host side of
the device: a tile stages 1024 + 2 H samples, so the kernel's share is a little larger), and the ratio to the copy by
medians and for the least favourable pairing of single runs (slowest stage call, fastest copy)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from ofdm_uhd_amd import cfr, config, engine, options  # noqa: E402

SIGMA = 0.05                       # per part: rms 0.05 sqrt(2)
THRESHOLDS = (("none", None), ("7dB", 7.0), ("4dB", 4.0))


def _stats(v):
    return [round(float(np.median(v)), 4), round(float(np.min(v)), 4), round(float(np.max(v)), 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, nargs="+", default=[1 << 24, 1 << 27])
    ap.add_argument("--half-widths", type=int, nargs="+", default=[0, 16, 128])
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    opt = options.default_options(modulation="qpsk")
    rms = SIGMA * np.sqrt(2.0)
    for n in a.samples:
        g = torch.Generator(device=dev)
        g.manual_seed(7)
        x = torch.randn(2 * n, dtype=torch.float32, device=dev, generator=g).mul_(SIGMA)
        mag2 = x.view(n, 2).square().sum(dim=1)
        for H in a.half_widths:
            for fmt in ("fc32", "sc16") if H == 16 else ("fc32",):
                for tname, db in THRESHOLDS:
                    thr = 1e3 if db is None else cfr.threshold_for(db, rms)
                    over = mag2 > float(np.float32(thr)) ** 2
                    pad = (-n) % 1024
                    tiles = torch.nn.functional.pad(over, (0, pad)).view(-1, 1024).any(dim=1)
                    share_over, share_tiles = float(over.float().mean().item()), float(tiles.float().mean().item())
                    del over, tiles
                    e = engine.Engine(cfg=config.make_cfg(opt, device_ptrs=True))
                    e.prof_enable(True)
                    oss = 8 if fmt == "fc32" else 4
                    out = torch.empty(n * oss, dtype=torch.uint8, device=dev)
                    moved = (8 + oss) * n
                    src = torch.zeros(moved // 2, dtype=torch.uint8, device=dev)
                    dst = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
                    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                    e.set_cfr(cfr.cfr_cfg(thr, cfr.design(H), out_format=fmt))
                    torch.cuda.synchronize()

                    def stage():
                        e.cfr_reset()
                        assert e.cfr_device(x.data_ptr(), n, out.data_ptr(), n) == n
                        return e.cfr_last_ms()

                    def copy():
                        ev[0].record()
                        dst.copy_(src)
                        ev[1].record()
                        torch.cuda.synchronize()
                        return ev[0].elapsed_time(ev[1])

                    variants = (("k_cfr", stage), ("copy", copy))
                    for _, f in variants:
                        for _ in range(2):
                            f()
                    ms = {v: [] for v, _ in variants}
                    for _ in range(a.rounds):
                        for v, f in variants:
                            ms[v] += [f() for _ in range(a.calls)]
                    st = e.cfr_stats()
                    med = {v: float(np.median(t)) for v, t in ms.items()}
                    res = {v + "_ms": _stats(t) for v, t in ms.items()}
                    res["k_cfr_TBps"] = round(moved / med["k_cfr"] * 1e-9, 3)
                    res["k_cfr_ps_per_sample"] = round(med["k_cfr"] * 1e9 / n, 3)
                    res["copy_TBps"] = round(moved / med["copy"] * 1e-9, 3)
                    res["stage_over_copy_median"] = round(med["k_cfr"] / med["copy"], 4)
                    res["stage_over_copy_worst"] = round(float(np.max(ms["k_cfr"])) / float(np.min(ms["copy"])), 4)
                    print(json.dumps({"threshold": tname, "half_width": H, "taps": 2 * H + 1, "format": fmt, "samples": n,
                                      "share_over": round(share_over, 5), "share_tiles_with_a_peak": round(share_tiles, 4),
                                      "share_touched": round(st["n_touched"] / float(n), 5), "bytes_moved": moved,
                                      "calls": a.calls * a.rounds, "ms_median_min_max": res}), flush=True)
                    e.close()
                    for t in (out, src, dst):        # handed back zeroed
                        t.zero_()
                    torch.cuda.synchronize()
                    del out, src, dst
                    torch.cuda.empty_cache()
        x.zero_()
        torch.cuda.synchronize()
        del x, mag2
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
