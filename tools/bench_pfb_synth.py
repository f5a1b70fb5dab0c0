"""The polyphase-FFT synthesis bank (k_pfb_synth) against K passes of the DUC (k_duc with `add`) and a device copy on one
MI355X:
python tools/bench_pfb_synth.py

Device pointers; every link's narrowband stream has the sample count of bench.py's C2 stream of --packets packets, random
samples; the band is M times as long, float32 and 16-bit IQ.  Shapes: M=4 / 31 taps / 4 channels, M=8 / 155 taps / 8
channels, M=8 / 155 taps / 2 channels and M=32 / 155 taps / 32 channels.  Per shape and format, after two warm-ups per
variant: ROUNDS alternations of [CALLS calls of k_pfb_synth, CALLS times the K passes of k_duc at L = M, fc = c / M, each
added onto the band so far, CALLS device copies]; k_pfb_synth's HIP-event time from ofdm_pfb_synth_last_ms, a DUC run's
as the sum of ofdm_duc_last_ms over its K passes (with 16-bit output the last pass stores the 16-bit band, the others
float32), the copy's from torch events.  The yardsticks are the DUC -- existing code this tool does not touch -- and a
torch copy that moves the bytes k_pfb_synth must move (8 K in per input index, 8 or 4 out per output: half of them read,
half written).  Prints one JSON line per shape and format: median / min / max ms, TB/s, and the ratios to each yardstick,
by medians and for the least favourable pairing of single runs (slowest k_pfb_synth call, fastest yardstick run)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench as B  # noqa: E402
from ofdm_uhd_amd import config, duc, engine, options, pfb  # noqa: E402

# M, (occupied fraction, transition) the prototype is designed for, channels that carry a link (None: all).  M = 32
# takes the 155 taps of M = 8: the shape is timed, not the filter
SHAPES = ((4, (200 / 512.0, None), None), (8, (48 / 64.0, None), None), (8, (48 / 64.0, None), (1, 6)),
          (32, (48 / 64.0, 1 / 64.0), None))


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
    for M, proto, sel in SHAPES:
        taps = pfb.synth_design(M, *proto)
        chans = list(range(M)) if sel is None else list(sel)
        K = len(chans)
        for fmt in ("fc32", "sc16"):
            e = engine.Engine(cfg=config.make_cfg(opt, device_ptrs=True))
            e.prof_enable(True)
            _, nsamp = e.tx_frame_count(np.full(a.packets, c["size"], np.uint32))
            nsamp = int(nsamp)
            nout = nsamp * M
            oss = 8 if fmt == "fc32" else 4
            stride = nsamp + 2
            g = torch.Generator(device=dev)
            g.manual_seed(M)
            x = torch.randn(2 * K * stride, dtype=torch.float32, device=dev, generator=g).mul_(0.05)
            band = torch.zeros(2 * nout, dtype=torch.float32, device=dev)      # the DUC passes' float32 band
            out = torch.empty(nout * oss, dtype=torch.uint8, device=dev)       # the bank's band; the 16-bit last pass's
            moved = 8 * K * nsamp + oss * nout
            # the copy reads moved / 2 bytes and writes as many, between two of this shape's own buffers that are large
            # enough (M = 32 leaves no room for two more of that size)
            big = [t.view(torch.uint8) for t in (x, band, out) if t.numel() * t.element_size() >= moved // 2]
            if len(big) >= 2:
                src, dst = big[0][:moved // 2], big[1][:moved // 2]
            else:
                src = torch.zeros(moved // 2, dtype=torch.uint8, device=dev)
                dst = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            e.set_pfb_synth(pfb.synth_cfg(M, chans, taps=taps, out_format=fmt))
            fcs = [ch / float(M) if ch <= M // 2 else (ch - M) / float(M) for ch in chans]
            cfgs = [duc.duc_cfg(M, fc, taps=taps) for fc in fcs]
            if fmt == "sc16":
                cfgs[-1] = duc.duc_cfg(M, fcs[-1], taps=taps, out_format="sc16")

            def bank():
                e.pfb_synth_reset(0)
                assert e.pfb_synth_device(x.data_ptr(), stride, nsamp, out.data_ptr(), nout) == nout
                return e.pfb_synth_last_ms()

            def passes():
                total = 0.0
                for i, cfg in enumerate(cfgs):
                    e.set_duc(cfg)
                    to = out if (fmt == "sc16" and i == K - 1) else band
                    assert e.duc_device(x.data_ptr() + 8 * i * stride, nsamp, to.data_ptr(), nout, add_ptr=band.data_ptr()) == nout
                    total += e.duc_last_ms()
                return total

            def copy():
                ev[0].record()
                dst.copy_(src)
                ev[1].record()
                torch.cuda.synchronize()
                return ev[0].elapsed_time(ev[1])

            variants = (("k_pfb_synth", bank), ("k_duc_passes", passes), ("copy", copy))
            for _, f in variants:
                for _ in range(2):
                    f()
            ms = {name: [] for name, _ in variants}
            for _ in range(a.rounds):
                for name, f in variants:
                    ms[name] += [f() for _ in range(a.calls)]
            med = {name: float(np.median(v)) for name, v in ms.items()}
            res = {name + "_ms": _stats(v) for name, v in ms.items()}
            duc_bytes = K * (8 * nsamp + 16 * nout) - (8 - oss) * nout
            res["k_pfb_synth_TBps"] = round(moved / med["k_pfb_synth"] * 1e-9, 3)
            res["k_duc_passes_TBps"] = round(duc_bytes / med["k_duc_passes"] * 1e-9, 3)
            res["copy_TBps"] = round(moved / med["copy"] * 1e-9, 3)
            for name in ("k_duc_passes", "copy"):
                res["synth_over_%s_median" % name] = round(med["k_pfb_synth"] / med[name], 4)
                res["synth_over_%s_worst" % name] = round(float(np.max(ms["k_pfb_synth"])) / float(np.min(ms[name])), 4)
            print(json.dumps({"M": M, "ntaps": len(taps), "nsel": K, "format": fmt, "inputs_per_channel": nsamp,
                              "outputs": nout, "bytes_moved": moved, "calls": a.calls * a.rounds,
                              "ms_median_min_max": res}), flush=True)
            e.close()
            for t in (x, band, out, dst):             # handed back zeroed
                t.zero_()
            torch.cuda.synchronize()
            del x, band, out, src, dst, big
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
