"""The transmit resampler bank (k_tx_resamp_bank) against K passes of the single stage (k_tx_resamp, the later ones with
`add`) and a device copy on one MI355X:
python tools/bench_tx_resamp_bank.py

Device pointers; every link's narrowband stream has the sample count of bench.py's C2 stream of --packets packets
(tools/bench_tx_resamp.py's stream), random samples; the band is L / M times as long, float32 and 16-bit IQ.  Shapes:
5/2 with 39 taps and 25/8 with 481 taps (what tx_resample.design gives for 200/512 and 48/64 occupancy), K = 2 and K = 8
links at frequencies off every grid.  Per shape and format, after two warm-ups per variant: ROUNDS alternations of [CALLS
calls of k_tx_resamp_bank, CALLS times the K passes of k_tx_resamp -- the first without `add`, every later one added onto
the band so far --, CALLS device copies]; k_tx_resamp_bank's HIP-event time from ofdm_tx_resamp_bank_last_ms, a run of
passes as the sum of ofdm_tx_resamp_last_ms over its K passes (with 16-bit output the last pass stores the 16-bit band,
the others float32), the copy's from torch events.  The yardsticks are the single stage -- existing code this tool does
not touch -- and a torch copy that moves the bytes k_tx_resamp_bank must move (8 K in per input index, 8 or 4 out per
output: half of them read, half written).  Prints one JSON line per shape and format: median / min / max ms, TB/s, and
the ratios to each yardstick, by medians and for the least favourable pairing of single runs (slowest bank call, fastest
yardstick run)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench as B  # noqa: E402
from ofdm_uhd_amd import config, engine, options, tx_resample  # noqa: E402

SHAPES = ((5, 2, 200 / 512.0, 39), (25, 8, 48 / 64.0, 481))
LINKS = (2, 8)
FREQS = (0.1875 + 1e-3 / 3.0, -0.3141592653589793, 0.0612, 0.4331, -0.0625 + 1e-4, 0.2871, -0.4503, -0.1999)


def _stats(v):
    return [round(float(np.median(v)), 4), round(float(np.min(v)), 4), round(float(np.max(v)), 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=16384)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    c = B.CONFIGS["c2"]
    opt = options.default_options(modulation=c["mod"], fft_length=c["N"], occupied_tones=c["occ"], cp_length=c["CP"])
    for L, M, occ_frac, want_taps in SHAPES:
        taps = tx_resample.design(L, M, occ_frac)
        assert len(taps) == want_taps
        for K in LINKS:
            fcs = list(FREQS[:K])
            for fmt in ("fc32", "sc16"):
                e = engine.Engine(cfg=config.make_cfg(opt, device_ptrs=True))
                e.prof_enable(True)
                _, nsamp = e.tx_frame_count(np.full(a.packets, c["size"], np.uint32))
                nsamp = int(nsamp)
                nout = tx_resample.count(0, nsamp, L, M)
                oss = 8 if fmt == "fc32" else 4
                stride = nsamp + 2
                g = torch.Generator(device=dev)
                g.manual_seed(L)
                x = torch.randn(2 * K * stride, dtype=torch.float32, device=dev, generator=g).mul_(0.05)
                band = torch.zeros(2 * nout, dtype=torch.float32, device=dev)      # the passes' float32 band
                out = torch.empty(nout * oss, dtype=torch.uint8, device=dev)       # the bank's band; the 16-bit last pass's
                moved = 8 * K * nsamp + oss * nout
                src = torch.zeros(moved // 2, dtype=torch.uint8, device=dev)
                dst = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                e.set_tx_resamp_bank(tx_resample.bank_cfg(L, M, fcs, taps=taps, out_format=fmt))
                cfgs = [tx_resample.tx_resamp_cfg(L, M, fc, taps=taps) for fc in fcs]
                if fmt == "sc16":
                    cfgs[-1] = tx_resample.tx_resamp_cfg(L, M, fcs[-1], taps=taps, out_format="sc16")
                torch.cuda.synchronize()

                def bank():
                    e.tx_resamp_bank_reset(0)
                    assert e.tx_resamp_bank_device(x.data_ptr(), stride, nsamp, out.data_ptr(), nout) == nout
                    return e.tx_resamp_bank_last_ms()

                def passes():
                    total = 0.0
                    for i, cfg in enumerate(cfgs):
                        e.set_tx_resamp(cfg)
                        to = out if (fmt == "sc16" and i == K - 1) else band
                        assert e.tx_resamp_device(x.data_ptr() + 8 * i * stride, nsamp, to.data_ptr(), nout,
                                                  add_ptr=band.data_ptr() if i else None) == nout
                        total += e.tx_resamp_last_ms()
                    return total

                def copy():
                    ev[0].record()
                    dst.copy_(src)
                    ev[1].record()
                    torch.cuda.synchronize()
                    return ev[0].elapsed_time(ev[1])

                variants = (("k_tx_resamp_bank", bank), ("k_tx_resamp_passes", passes), ("copy", copy))
                for _, f in variants:
                    for _ in range(2):
                        f()
                ms = {name: [] for name, _ in variants}
                for _ in range(a.rounds):
                    for name, f in variants:
                        ms[name] += [f() for _ in range(a.calls)]
                med = {name: float(np.median(v)) for name, v in ms.items()}
                res = {name + "_ms": _stats(v) for name, v in ms.items()}
                # the passes: 8 in per input and pass, 8 out per output and pass (the last 8 or 4), 8 more per added pass
                pass_bytes = K * (8 * nsamp + 8 * nout) + (K - 1) * 8 * nout - (8 - oss) * nout
                res["k_tx_resamp_bank_TBps"] = round(moved / med["k_tx_resamp_bank"] * 1e-9, 3)
                res["k_tx_resamp_bank_ps_per_output"] = round(med["k_tx_resamp_bank"] * 1e9 / nout, 3)
                res["k_tx_resamp_passes_TBps"] = round(pass_bytes / med["k_tx_resamp_passes"] * 1e-9, 3)
                res["k_tx_resamp_passes_ps_per_output"] = round(med["k_tx_resamp_passes"] * 1e9 / nout, 3)
                res["copy_TBps"] = round(moved / med["copy"] * 1e-9, 3)
                for name in ("k_tx_resamp_passes", "copy"):
                    res["bank_over_%s_median" % name] = round(med["k_tx_resamp_bank"] / med[name], 4)
                    res["bank_over_%s_worst" % name] = round(float(np.max(ms["k_tx_resamp_bank"])) / float(np.min(ms[name])), 4)
                print(json.dumps({"L": L, "M": M, "ntaps": len(taps), "nlinks": K, "format": fmt, "inputs_per_link": nsamp,
                                  "outputs": nout, "bytes_moved": moved, "calls": a.calls * a.rounds,
                                  "ms_median_min_max": res}), flush=True)
                e.close()
                for t in (x, band, out, src, dst):        # handed back zeroed
                    t.zero_()
                torch.cuda.synchronize()
                del x, band, out, src, dst
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
