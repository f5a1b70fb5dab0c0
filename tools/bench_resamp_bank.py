"""The resampler bank (k_resamp_bank) against K calls of the single resampler (k_resamp) on one MI355X:
python tools/bench_resamp_bank.py

Device pointers, 2^--log2-samples random wideband samples.  Shapes: tools/bench_resamp.py's two, (L, M, ntaps) =
(2, 5, 39) and (8, 25, 481), float32 and 16-bit IQ.  Per shape and format, after two warm-up calls per variant: ROUNDS
alternations of [CALLS calls of the single resampler, then CALLS calls of the bank at K = 2, 4 and 8]; k_resamp's
HIP-event time from ofdm_resamp_last_ms, k_resamp_bank's from ofdm_resamp_bank_last_ms.  The yardstick for the bank at
K links is K times the median of k_resamp in the same job, never the bank itself.  Prints one JSON line per shape and
format: median / min / max ms, the ratio bank / (K x single), bytes moved (8 or 4 B in per input sample, 8 K L / M out),
TB/s, and the FMA rate (4 K ntaps / M scalar FMAs per input sample)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from ofdm_uhd_amd import config, engine, options, resample  # noqa: E402

SHAPES = ((2, 5, 200 / 512.0), (8, 25, 48 / 64.0))
LINKS = (2, 4, 8)


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
    rng = np.random.default_rng(7)
    freqs = [0.21] + [float(f) for f in rng.uniform(-0.5, 0.5, max(LINKS) - 1)]
    for L, M, occ_frac in SHAPES:
        taps = resample.design(L, M, occ_frac)
        nout = resample.count(0, nin, L, M)
        stride = nout + 2
        for fmt in ("fc32", "sc16"):
            e = engine.Engine(cfg=config.make_cfg(opt, device_ptrs=True))
            e.set_rx_iq_format(fmt)
            e.prof_enable(True)
            g = torch.Generator(device=dev)
            g.manual_seed(L)
            if fmt == "fc32":
                x = torch.randn(2 * nin, dtype=torch.float32, device=dev, generator=g)
            else:
                x = torch.randint(-32768, 32768, (2 * nin,), dtype=torch.int16, device=dev, generator=g)
            y = torch.empty(2 * max(LINKS) * stride, dtype=torch.float32, device=dev)
            e.set_resamp(resample.resamp_cfg(L, M, freqs[0], taps=taps))

            def single():
                e.resamp_reset(0)
                assert e.resamp_device(x.data_ptr(), nin, y.data_ptr(), stride) == nout
                return e.resamp_last_ms()

            def bank():
                e.resamp_bank_reset(0)
                assert e.resamp_bank_device(x.data_ptr(), nin, y.data_ptr(), stride, stride) == nout
                return e.resamp_bank_last_ms()

            for _ in range(2):
                single()
            for K in LINKS:
                e.set_resamp_bank(resample.bank_cfg(L, M, freqs[:K], taps=taps))
                for _ in range(2):
                    bank()
            ms1, msK = [], {K: [] for K in LINKS}
            for _ in range(a.rounds):
                ms1 += [single() for _ in range(a.calls)]
                for K in LINKS:
                    e.set_resamp_bank(resample.bank_cfg(L, M, freqs[:K], taps=taps))
                    msK[K] += [bank() for _ in range(a.calls)]
            in_bytes = nin * (8 if fmt == "fc32" else 4)
            med1 = float(np.median(ms1))
            fma = 4.0 * len(taps) / M * nin           # scalar FMAs per link: 4 per tap, ntaps / L taps per output
            res = {"k_resamp_ms": _stats(ms1), "k_resamp_TBps": round((in_bytes + 8 * nout) / med1 * 1e-9, 3),
                   "k_resamp_TFMAps": round(fma / med1 * 1e-9, 3), "bank": {}}
            for K in LINKS:
                med = float(np.median(msK[K]))
                res["bank"][str(K)] = {
                    "k_resamp_bank_ms": _stats(msK[K]), "K_x_single_ms": round(K * med1, 4),
                    "ratio_median": round(med / (K * med1), 4),
                    # the least favourable pairing of the runs: slowest bank call over K times the fastest single call
                    "ratio_worst": round(float(np.max(msK[K])) / (K * float(np.min(ms1))), 4),
                    "TBps": round((in_bytes + 8 * K * nout) / med * 1e-9, 3),
                    "TFMAps": round(K * fma / med * 1e-9, 3)}
            print(json.dumps({"L": L, "M": M, "ntaps": len(taps), "format": fmt, "input_samples": nin,
                              "outputs_per_link": nout, "calls": a.calls * a.rounds, "ms_median_min_max": res}), flush=True)
            e.close()
            del x, y
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
