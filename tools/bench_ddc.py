"""The wideband front end (k_ddc) on one MI355X: python tools/bench_ddc.py

Device pointers.  The wideband stream is R times the sample count of bench.py's C2 stream of --packets packets (random
samples: the kernel's time does not depend on their values).  Shapes: R=4 / 31 taps and R=8 / 155 taps (what ddc.design
gives for C2's 200/512 and for 48/64 occupancy), float32 and 16-bit IQ alternating on one box, ROUNDS alternations of
CALLS calls after a warm-up; k_ddc's HIP-event time from ofdm_ddc_last_ms.  Beside it the device-to-device torch copy
of the same input buffer (HIP events).  Prints one JSON line per shape: median / min / max ms, bytes moved (8 or 4 B in
per input sample, 8 / R out), TB/s, and the FMA rate (4 ntaps / R scalar FMAs per input sample)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench as B  # noqa: E402
from ofdm_uhd_amd import config, ddc, engine, options  # noqa: E402

SHAPES = ((4, 200 / 512.0), (8, 48 / 64.0))


def _stats(v):
    return [round(float(np.median(v)), 4), round(float(np.min(v)), 4), round(float(np.max(v)), 4)]


def _copy_ms(src, calls):
    dst = torch.empty_like(src)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for i in range(calls + 2):
        a.record()
        dst.copy_(src)
        b.record()
        torch.cuda.synchronize()
        if i >= 2:
            out.append(a.elapsed_time(b))
    del dst
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=16384)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    c = B.CONFIGS["c2"]
    opt = options.default_options(modulation=c["mod"], fft_length=c["N"], occupied_tones=c["occ"], cp_length=c["CP"])
    engs = {}
    for fmt in ("fc32", "sc16"):
        e = engine.Engine(cfg=config.make_cfg(opt, device_ptrs=True))
        e.set_rx_iq_format(fmt)
        e.prof_enable(True)
        engs[fmt] = e
    _, nsamp = engs["fc32"].tx_frame_count(np.full(a.packets, c["size"], np.uint32))
    for R, occ_frac in SHAPES:
        taps = ddc.design(R, occ_frac)
        nin = int(nsamp) * R
        g = torch.Generator(device=dev)
        g.manual_seed(R)
        x = {"fc32": torch.randn(2 * nin, dtype=torch.float32, device=dev, generator=g),
             "sc16": torch.randint(-32768, 32768, (2 * nin,), dtype=torch.int16, device=dev, generator=g)}
        y = torch.empty(2 * (int(nsamp) + 1), dtype=torch.float32, device=dev)
        ms = {f: [] for f in engs}
        for f, e in engs.items():
            e.set_ddc(ddc.ddc_cfg(R, 0.25, taps=taps))
            for _ in range(2):
                e.ddc_reset(0)
                e.ddc_device(x[f].data_ptr(), nin, y.data_ptr(), int(nsamp) + 1)
        for _ in range(a.rounds):
            for f in ("fc32", "sc16"):
                e = engs[f]
                for _ in range(a.calls):
                    e.ddc_reset(0)
                    n = e.ddc_device(x[f].data_ptr(), nin, y.data_ptr(), int(nsamp) + 1)
                    assert n == (nin + R - 1) // R
                    ms[f].append(e.ddc_last_ms())
        copy = {f: _copy_ms(x[f], a.calls) for f in engs}
        res = {}
        for f in engs:
            bytes_moved = nin * (8 if f == "fc32" else 4) + n * 8
            med = float(np.median(ms[f]))
            res[f] = {"k_ddc_ms": _stats(ms[f]), "bytes": bytes_moved, "TBps": round(bytes_moved / med * 1e-9, 3),
                      "TFMAps": round(4.0 * len(taps) / R * nin / med * 1e-9, 3),
                      "torch_copy_ms": _stats(copy[f]),
                      "torch_copy_TBps": round(2 * x[f].numel() * x[f].element_size() / float(np.median(copy[f])) * 1e-9, 3)}
        print(json.dumps({"R": R, "ntaps": len(taps), "input_samples": nin, "outputs": int(n), "calls": a.calls * a.rounds,
                          "ms_median_min_max": res}), flush=True)
        del x, y
    for e in engs.values():
        e.close()


if __name__ == "__main__":
    main()
