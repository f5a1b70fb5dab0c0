"""The propagation channel stage (k_multipath) against a device copy of the same bytes on one MI355X:
python tools/bench_multipath.py

Device pointers; a stream of 2^24 random complex64 samples; float32 and 16-bit IQ out.  Configurations: three static
profiles (one path; two paths; sixteen paths with delays up to 1023), four paths of which three carry a Doppler shift,
and sixteen paths with four Doppler shifts, four tones, a carrier offset and noise.  Per configuration and format, after
two warm-ups per variant: ROUNDS alternations of [CALLS calls of k_multipath, CALLS device copies]; k_multipath's
HIP-event time from ofdm_multipath_last_ms, the copy's from torch events.  The yardstick is a torch copy that moves the
bytes k_multipath must move (8 in per sample, 8 or 4 out: half of them read, half written).  Prints one JSON line per
configuration and format: median / min / max ms, TB/s, ps per sample, float64 phasors per sample, and the ratio to the
copy by medians and for the least favourable pairing of single runs (slowest stage call, fastest copy)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from ofdm_uhd_amd import config, engine, multipath, options  # noqa: E402


def _dense16():
    rng = np.random.default_rng(1601)
    delays = np.concatenate([[0, 1023], 1 + rng.choice(1022, 14, replace=False)])
    g = (rng.standard_normal(16) + 1j * rng.standard_normal(16)) * 0.25
    return [(int(d), complex(c)) for d, c in zip(delays, g)]


def _everything():
    f = {1: 1e-4, 5: -3e-3, 9: 0.5, 14: 0.0371}
    return [(d, g, f[p]) if p in f else (d, g) for p, (d, g) in enumerate(_dense16())]


TONES4 = [(0.05, 0.0), (0.03, 0.5), (0.04, -0.5, 0.3), (0.02, 0.1234)]
CONFIGS = (
    ("unit", dict(paths=[(0, 1.0)])),
    ("two_ray", dict(paths=[(0, 1.0), (4, 0.5 * np.exp(0.7j))])),
    ("dense16", dict(paths=_dense16())),
    ("doppler4", dict(paths=[(0, 1.0, 0.0), (3, 0.5j, 1e-4), (11, -0.4 + 0.1j, -3e-3), (40, 0.3, 0.5)])),
    ("everything", dict(paths=_everything(), tones=TONES4, sigma=0.01, cfo=0.003)),
)


def _stats(v):
    return [round(float(np.median(v)), 4), round(float(np.min(v)), 4), round(float(np.max(v)), 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1 << 24)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    n = a.samples
    opt = options.default_options(modulation="qpsk")
    for name, kw in CONFIGS:
        for fmt in ("fc32", "sc16"):
            e = engine.Engine(cfg=config.make_cfg(opt, device_ptrs=True))
            e.prof_enable(True)
            cfg = multipath.multipath_cfg(out_format=fmt, **kw)
            phasors = sum(1 for _, _, f in multipath.paths_of(cfg) if f != 0.0) + cfg.ntones + (1 if cfg.cfo != 0.0 else 0)
            oss = 8 if fmt == "fc32" else 4
            g = torch.Generator(device=dev)
            g.manual_seed(7)
            x = torch.randn(2 * n, dtype=torch.float32, device=dev, generator=g).mul_(0.05)
            out = torch.empty(n * oss, dtype=torch.uint8, device=dev)
            moved = (8 + oss) * n
            src = torch.zeros(moved // 2, dtype=torch.uint8, device=dev)
            dst = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            e.set_multipath(cfg)
            torch.cuda.synchronize()

            def stage():
                e.multipath_reset(0)
                assert e.multipath_device(x.data_ptr(), n, out.data_ptr(), n) == n
                return e.multipath_last_ms()

            def copy():
                ev[0].record()
                dst.copy_(src)
                ev[1].record()
                torch.cuda.synchronize()
                return ev[0].elapsed_time(ev[1])

            variants = (("k_multipath", stage), ("copy", copy))
            for _, f in variants:
                for _ in range(2):
                    f()
            ms = {v: [] for v, _ in variants}
            for _ in range(a.rounds):
                for v, f in variants:
                    ms[v] += [f() for _ in range(a.calls)]
            med = {v: float(np.median(t)) for v, t in ms.items()}
            res = {v + "_ms": _stats(t) for v, t in ms.items()}
            res["k_multipath_TBps"] = round(moved / med["k_multipath"] * 1e-9, 3)
            res["k_multipath_ps_per_sample"] = round(med["k_multipath"] * 1e9 / n, 3)
            res["copy_TBps"] = round(moved / med["copy"] * 1e-9, 3)
            res["stage_over_copy_median"] = round(med["k_multipath"] / med["copy"], 4)
            res["stage_over_copy_worst"] = round(float(np.max(ms["k_multipath"])) / float(np.min(ms["copy"])), 4)
            print(json.dumps({"config": name, "npaths": cfg.npaths, "ntones": cfg.ntones, "phasors_per_sample": phasors,
                              "noise": cfg.sigma > 0, "format": fmt, "samples": n, "bytes_moved": moved,
                              "calls": a.calls * a.rounds, "ms_median_min_max": res}), flush=True)
            e.close()
            for t in (x, out, src, dst):        # handed back zeroed
                t.zero_()
            torch.cuda.synchronize()
            del x, out, src, dst
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
