"""The rational-rate front end (k_resamp) on one MI355X: python tools/bench_resamp.py

Device pointers, 2^24 float32 IQ input samples (random: the kernel's time does not depend on their values).  Shapes:
(L, M, ntaps) = (2, 5, 39) and (8, 25, 481) -- what resample.design gives for 200/512 and 48/64 occupancy -- and beside
them k_ddc at R = 3 / 31 taps (a 0.0775 transition) on the same buffer, the existing stage nearest in work per sample.  The three alternate on
one box: ROUNDS alternations of CALLS calls after a warm-up of every shape; HIP-event kernel times from
ofdm_resamp_last_ms / ofdm_ddc_last_ms.  Prints one JSON line per shape: median / min / max ms, bytes moved (8 B per
input sample plus 8 B per output) and the implied TB/s."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from ofdm_uhd_amd import config, ddc, engine, options, resample  # noqa: E402

SHAPES = ((2, 5, 200 / 512.0), (8, 25, 48 / 64.0))
DDC_R, DDC_OCC, DDC_TRANSITION = 3, 200 / 512.0, 0.0775      # firdes.low_pass gives 31 taps at this transition


def _stats(v):
    return [round(float(np.median(v)), 4), round(float(np.min(v)), 4), round(float(np.max(v)), 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-samples", type=int, default=24)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    nin = 1 << a.log2_samples
    opt = options.default_options(modulation="qpsk")
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    x = torch.randn(2 * nin, dtype=torch.float32, device=dev, generator=g)
    y = torch.empty(2 * (nin + 1), dtype=torch.float32, device=dev)      # L / M <= 1 in every shape here
    runs = []
    for L, M, occ in SHAPES:
        e = engine.Engine(cfg=config.make_cfg(opt, device_ptrs=True))
        e.prof_enable(True)
        taps = resample.design(L, M, occ)
        e.set_resamp(resample.resamp_cfg(L, M, 0.21, taps=taps))
        runs.append((dict(stage="k_resamp", L=L, M=M, ntaps=len(taps)), e, e.resamp_reset, e.resamp_device, e.resamp_last_ms))
    e = engine.Engine(cfg=config.make_cfg(opt, device_ptrs=True))
    e.prof_enable(True)
    taps = ddc.design(DDC_R, DDC_OCC, DDC_TRANSITION)
    assert len(taps) == 31
    e.set_ddc(ddc.ddc_cfg(DDC_R, 0.21, taps=taps))
    runs.append((dict(stage="k_ddc", R=DDC_R, ntaps=len(taps)), e, e.ddc_reset, e.ddc_device, e.ddc_last_ms))
    ms, nout = [[] for _ in runs], [0] * len(runs)
    for _, _, reset, run, _ in runs:                 # warm-up: code objects, buffers
        for _ in range(2):
            reset(0)
            run(x.data_ptr(), nin, y.data_ptr(), nin + 1)
    for _ in range(a.rounds):
        for i, (_, _, reset, run, last_ms) in enumerate(runs):
            for _ in range(a.calls):
                reset(0)
                nout[i] = run(x.data_ptr(), nin, y.data_ptr(), nin + 1)
                ms[i].append(last_ms())
    for i, (what, e, _, _, _) in enumerate(runs):
        moved = 8 * nin + 8 * nout[i]
        med = float(np.median(ms[i]))
        print(json.dumps(dict(what, input_samples=nin, outputs=int(nout[i]), calls=len(ms[i]), ms_median_min_max=_stats(ms[i]),
                              bytes=moved, TBps=round(moved / med * 1e-9, 3))), flush=True)
        e.close()


if __name__ == "__main__":
    main()
