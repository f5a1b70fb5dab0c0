"""The rational-rate transmit stage (k_tx_resamp) on one MI355X: python tools/bench_tx_resamp.py

Device pointers.  The narrowband stream has the sample count of bench.py's C2 stream of --packets packets (random
samples: the kernel's time does not depend on their values).  Shapes: 5/2 at 39 taps and 25/8 at 481 taps (what
tx_resample.design gives for 200/512 and 48/64 occupancy) and, for comparison in the same job, k_duc at L = 4 / 31
taps; variants: complex64 and 16-bit output, with and without `add` (a second buffer, not the output itself),
alternating on one box, ROUNDS alternations of CALLS calls after two warm-up calls; the kernel's HIP-event time from
ofdm_tx_resamp_last_ms / ofdm_duc_last_ms.  The yardstick, in the same job: a device-to-device torch copy that moves the
same number of bytes (HIP events).  Prints one JSON line per shape: median / min / max ms, bytes moved (8 M / L in, 8 or
4 out, 8 more with add, per output), TB/s, the share of the copy's rate, and the FMA rate (2 ceil(ntaps / L) scalar FMAs
per output)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench as B  # noqa: E402
from ofdm_uhd_amd import config, duc, engine, options, tx_resample  # noqa: E402

# stage, L, M, occupied fraction, the tap count the design must give
SHAPES = (("tx_resamp", 5, 2, 200 / 512.0, 39), ("tx_resamp", 25, 8, 48 / 64.0, 481), ("duc", 4, 1, 200 / 512.0, 31))
VARIANTS = (("fc32", False), ("fc32", True), ("sc16", False), ("sc16", True))


def _stats(v):
    return [round(float(np.median(v)), 4), round(float(np.min(v)), 4), round(float(np.max(v)), 4)]


def _copy_ms(nbytes, calls, dev):
    """A copy that reads and writes nbytes in all (half of it each way)."""
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
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
    del src, dst
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
    e = engine.Engine(cfg=config.make_cfg(opt, device_ptrs=True))
    e.prof_enable(True)
    _, nsamp = e.tx_frame_count(np.full(a.packets, c["size"], np.uint32))
    nin = int(nsamp)
    for stage, L, M, occ_frac, want_taps in SHAPES:
        taps = tx_resample.design(L, M, occ_frac)
        assert len(taps) == want_taps
        no = tx_resample.count(0, nin, L, M)
        g = torch.Generator(device=dev)
        g.manual_seed(L)
        x = torch.randn(2 * nin, dtype=torch.float32, device=dev, generator=g)
        w = torch.randn(2 * no, dtype=torch.float32, device=dev, generator=g)
        y = torch.empty(2 * no, dtype=torch.float32, device=dev)     # (the 16-bit variants fill half of it)
        torch.cuda.synchronize()

        def run(fmt, add):
            add_ptr = w.data_ptr() if add else None
            if stage == "duc":
                e.set_duc(duc.duc_cfg(L, 0.25, taps=taps, out_format=fmt))
                n, last_ms = e.duc_device(x.data_ptr(), nin, y.data_ptr(), no, add_ptr=add_ptr), e.duc_last_ms
            else:
                e.set_tx_resamp(tx_resample.tx_resamp_cfg(L, M, 0.25, taps=taps, out_format=fmt))
                n, last_ms = e.tx_resamp_device(x.data_ptr(), nin, y.data_ptr(), no, add_ptr=add_ptr), e.tx_resamp_last_ms
            assert n == no
            return last_ms()

        ms = {v: [] for v in VARIANTS}
        for v in VARIANTS:
            for _ in range(2):
                run(*v)
        for _ in range(a.rounds):
            for v in VARIANTS:
                for _ in range(a.calls):
                    ms[v].append(run(*v))
        res = {}
        for fmt, add in VARIANTS:
            nbytes = nin * 8 + no * (8 if fmt == "fc32" else 4) + (no * 8 if add else 0)
            med = float(np.median(ms[(fmt, add)]))
            copy = _copy_ms(nbytes, a.calls, dev)
            cmed = float(np.median(copy))
            res[fmt + ("+add" if add else "")] = {
                "kernel_ms": _stats(ms[(fmt, add)]), "bytes": nbytes, "TBps": round(nbytes / med * 1e-9, 3),
                "TFMAps": round(2.0 * -(-len(taps) // L) * no / med * 1e-9, 3),
                "torch_copy_ms": _stats(copy), "torch_copy_TBps": round(nbytes / cmed * 1e-9, 3),
                "share_of_copy": round(cmed / med, 3)}
        print(json.dumps({"kernel": "k_" + stage, "L": L, "M": M, "ntaps": len(taps), "input_samples": nin, "outputs": no,
                          "calls": a.calls * a.rounds, "ms_median_min_max": res}), flush=True)
        del x, w, y
        e.set_duc(None)
        e.set_tx_resamp(None)
    e.close()


if __name__ == "__main__":
    main()
