"""The DDC bank (k_ddc_bank) against K calls of the single DDC (k_ddc) on one MI355X: python tools/bench_ddc_bank.py

Device pointers, the stream of tools/bench_ddc.py: R times the sample count of bench.py's C2 stream of --packets
packets, random samples.  Shapes: R=4 / 31 taps and R=8 / 155 taps, float32 and 16-bit IQ.  Per shape and format, after
two warm-up calls per variant: ROUNDS alternations of [CALLS calls of the single DDC, then CALLS calls of the bank at
K = 2, 4 and 8]; k_ddc's HIP-event time from ofdm_ddc_last_ms, k_ddc_bank's from ofdm_ddc_bank_last_ms.  The yardstick
for the bank at K links is K times the median of k_ddc in the same job, never the bank itself.  Prints one JSON line
per shape and format: median / min / max ms, the ratio bank / (K x single), bytes moved (8 or 4 B in per input sample,
8 K / R out), TB/s, and the FMA rate (4 K ntaps / R scalar FMAs per input sample)."""
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
LINKS = (2, 4, 8)


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
    rng = np.random.default_rng(7)
    freqs = [0.25] + [float(f) for f in rng.uniform(-0.5, 0.5, max(LINKS) - 1)]
    for R, occ_frac in SHAPES:
        taps = ddc.design(R, occ_frac)
        for fmt in ("fc32", "sc16"):
            e = engine.Engine(cfg=config.make_cfg(opt, device_ptrs=True))
            e.set_rx_iq_format(fmt)
            e.prof_enable(True)
            _, nsamp = e.tx_frame_count(np.full(a.packets, c["size"], np.uint32))
            nsamp = int(nsamp)
            nin = nsamp * R
            g = torch.Generator(device=dev)
            g.manual_seed(R)
            if fmt == "fc32":
                x = torch.randn(2 * nin, dtype=torch.float32, device=dev, generator=g)
            else:
                x = torch.randint(-32768, 32768, (2 * nin,), dtype=torch.int16, device=dev, generator=g)
            stride = nsamp + 2
            y = torch.empty(2 * max(LINKS) * stride, dtype=torch.float32, device=dev)
            e.set_ddc(ddc.ddc_cfg(R, freqs[0], taps=taps))

            def single():
                e.ddc_reset(0)
                n = e.ddc_device(x.data_ptr(), nin, y.data_ptr(), stride)
                assert n == (nin + R - 1) // R
                return e.ddc_last_ms()

            def bank():
                e.ddc_bank_reset(0)
                n = e.ddc_bank_device(x.data_ptr(), nin, y.data_ptr(), stride, stride)
                assert n == (nin + R - 1) // R
                return e.ddc_bank_last_ms()

            for _ in range(2):
                single()
            for K in LINKS:
                e.set_ddc_bank(ddc.bank_cfg(R, freqs[:K], taps=taps))
                for _ in range(2):
                    bank()
            ms1, msK = [], {K: [] for K in LINKS}
            for _ in range(a.rounds):
                ms1 += [single() for _ in range(a.calls)]
                for K in LINKS:
                    e.set_ddc_bank(ddc.bank_cfg(R, freqs[:K], taps=taps))
                    msK[K] += [bank() for _ in range(a.calls)]
            nout = (nin + R - 1) // R
            in_bytes = nin * (8 if fmt == "fc32" else 4)
            med1 = float(np.median(ms1))
            res = {"k_ddc_ms": _stats(ms1), "k_ddc_TBps": round((in_bytes + 8 * nout) / med1 * 1e-9, 3),
                   "k_ddc_TFMAps": round(4.0 * len(taps) / R * nin / med1 * 1e-9, 3), "bank": {}}
            for K in LINKS:
                med = float(np.median(msK[K]))
                res["bank"][str(K)] = {
                    "k_ddc_bank_ms": _stats(msK[K]), "K_x_single_ms": round(K * med1, 4),
                    "ratio_median": round(med / (K * med1), 4),
                    # the least favourable pairing of the runs: slowest bank call over K times the fastest single call
                    "ratio_worst": round(float(np.max(msK[K])) / (K * float(np.min(ms1))), 4),
                    "TBps": round((in_bytes + 8 * K * nout) / med * 1e-9, 3),
                    "TFMAps": round(4.0 * K * len(taps) / R * nin / med * 1e-9, 3)}
            print(json.dumps({"R": R, "ntaps": len(taps), "format": fmt, "input_samples": nin, "outputs_per_link": nout,
                              "calls": a.calls * a.rounds, "ms_median_min_max": res}), flush=True)
            e.close()
            del x, y
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
