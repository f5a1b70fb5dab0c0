"""The wideband transmit stage (k_duc) on one MI355X: python tools/bench_duc.py

Device pointers.  The narrowband stream has the sample count of bench.py's C2 stream of --packets packets (random
samples: the kernel's time does not depend on their values).  Shapes: L=4 / 31 taps, L=8 / 155 taps and L=2 / 25 taps
(what duc.design gives for 200/512, 48/64 and 0.61 occupancy); variants: complex64 and 16-bit output, with and without
`add` (a second buffer, not the output itself), alternating on one box, ROUNDS alternations of CALLS calls after a
warm-up; k_duc's HIP-event time from ofdm_duc_last_ms.  The yardstick, in the same job: a device-to-device torch copy
that moves the same number of bytes (HIP events).  Prints one JSON line per shape: median / min / max ms, bytes moved
(8 / L in, 8 or 4 out, 8 more with add, per output), TB/s, the share of the copy's rate, and the FMA rate
(2 ceil(ntaps / L) scalar FMAs per output)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench as B  # noqa: E402
from ofdm_uhd_amd import config, duc, engine, options  # noqa: E402

SHAPES = ((4, 200 / 512.0, 31), (8, 48 / 64.0, 155), (2, 0.61, 25))
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
    for L, occ_frac, want_taps in SHAPES:
        taps = duc.design(L, occ_frac)
        assert len(taps) == want_taps
        no = nin * L
        g = torch.Generator(device=dev)
        g.manual_seed(L)
        x = torch.randn(2 * nin, dtype=torch.float32, device=dev, generator=g)
        w = torch.randn(2 * no, dtype=torch.float32, device=dev, generator=g)
        y = torch.empty(2 * no, dtype=torch.float32, device=dev)     # (the 16-bit variants fill half of it)
        torch.cuda.synchronize()

        def run(fmt, add):
            e.set_duc(duc.duc_cfg(L, 0.25, taps=taps, out_format=fmt))
            n = e.duc_device(x.data_ptr(), nin, y.data_ptr(), no, add_ptr=w.data_ptr() if add else None)
            assert n == no
            return e.duc_last_ms()

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
                "k_duc_ms": _stats(ms[(fmt, add)]), "bytes": nbytes, "TBps": round(nbytes / med * 1e-9, 3),
                "TFMAps": round(2.0 * -(-len(taps) // L) * no / med * 1e-9, 3),
                "torch_copy_ms": _stats(copy), "torch_copy_TBps": round(nbytes / cmed * 1e-9, 3),
                "share_of_copy": round(cmed / med, 3)}
        print(json.dumps({"L": L, "ntaps": len(taps), "input_samples": nin, "outputs": no, "calls": a.calls * a.rounds,
                          "ms_median_min_max": res}), flush=True)
        del x, w, y
    e.close()


if __name__ == "__main__":
    main()
