"""The spectrum stage (k_psd and k_psd_reduce) against a device copy of the same input bytes and against k_sense on one
MI355X:  python tools/bench_psd.py

One job of several steps, one step per stream length and input format; each step is a process of its own under its own
time limit, and the job ends with the first step that fails or runs out of time (nothing more is started on the GPU
then).  A step holds a stream of 2^24 or 2^27 seeded Gaussian samples on the device (complex64, or 16-bit IQ at a
quarter of full scale) and walks F in {512, 1024, 4096} x hop in {F, F/2, F/4} x {no rows, rows}.  Per configuration,
after two warm-ups per variant: ROUNDS alternations of [CALLS calls of the stage, CALLS device copies]; the stage's
HIP-event time from ofdm_psd_last_ms (k_psd and k_psd_reduce), the copy's from torch events.  The yardstick is a torch
copy whose source is the stage's input, byte for byte (it reads them and writes as many; the stage without rows writes
next to nothing).  At hop = F the sensor runs on the same bytes as one dwell (tune_delay 0, dwell_delay = all vectors):
k_sense's time from the profiler's table.  Prints one JSON line per configuration: median / min / max ms, input TB/s,
ps per sample, transforms per second, and the ratio to the copy by medians."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = [(n, fmt) for n in (1 << 24, 1 << 27) for fmt in ("fc32", "sc16")]
STEP_SECONDS = 240


def _stats(v):
    import numpy as np
    return [round(float(np.median(v)), 4), round(float(np.min(v)), 4), round(float(np.max(v)), 4)]


def step(n, fmt, ffts, calls, rounds):
    import numpy as np
    import torch

    from ofdm_uhd_amd import config, engine, options, spectrum
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    if fmt == "sc16":
        x = torch.randn(2 * n, dtype=torch.float32, device=dev, generator=g).mul_(8192.0).clamp_(-32768, 32767).to(torch.int16)
    else:
        x = torch.randn(2 * n, dtype=torch.float32, device=dev, generator=g).mul_(0.25)
    nbytes = x.numel() * x.element_size()
    dst = torch.empty_like(x)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    e = engine.Engine(cfg=config.make_cfg(options.default_options(modulation="qpsk"), device_ptrs=True))
    e.prof_enable(True)
    e.set_rx_iq_format(fmt)

    def copy():
        ev[0].record()
        dst.copy_(x)
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1])

    for F in ffts:
        for hop in (F, F // 2, F // 4):
            nseg = spectrum.segments(n, F, hop)
            for with_rows in (False, True):
                e.set_psd(spectrum.psd_cfg(F, hop, in_format=fmt))
                rows = torch.empty(nseg * F, dtype=torch.float32, device=dev) if with_rows else None

                def stage():
                    e.psd_reset()
                    got = e.psd_device(x.data_ptr(), n, rows.data_ptr() if with_rows else None, nseg if with_rows else 0)
                    assert got == nseg
                    return e.psd_last_ms()

                variants = [("k_psd", stage), ("copy", copy)]
                if hop == F and not with_rows:
                    sc = config.make_sense_cfg(F, 0, n // F, 1, 0)

                    def sense():
                        e.prof_reset()
                        e.sense(sc, x.data_ptr(), n)
                        t = [v[0] for k, v in e.prof().items() if "sense" in k and v[1]]
                        assert len(t) == 1
                        return t[0]
                    variants.append(("k_sense", sense))
                for _, f in variants:
                    for _ in range(2):
                        f()
                ms = {v: [] for v, _ in variants}
                for _ in range(rounds):
                    for v, f in variants:
                        ms[v] += [f() for _ in range(calls)]
                med = {v: float(np.median(t)) for v, t in ms.items()}
                res = {v + "_ms": _stats(t) for v, t in ms.items()}
                res["k_psd_input_TBps"] = round(nbytes / med["k_psd"] * 1e-9, 3)
                res["k_psd_ps_per_sample"] = round(med["k_psd"] * 1e9 / n, 3)
                res["k_psd_Mtransforms_per_s"] = round(nseg / med["k_psd"] * 1e-3, 2)
                res["copy_TBps_read_plus_written"] = round(2 * nbytes / med["copy"] * 1e-9, 3)
                res["stage_over_copy_median"] = round(med["k_psd"] / med["copy"], 4)
                if "k_sense" in med:
                    res["stage_over_sense_median"] = round(med["k_psd"] / med["k_sense"], 4)
                print(json.dumps({"nfft": F, "hop": hop, "format": fmt, "samples": n, "segments": nseg, "rows": with_rows,
                                  "input_bytes": nbytes, "rows_bytes": 4 * nseg * F if with_rows else 0,
                                  "calls": calls * rounds, "ms_median_min_max": res}), flush=True)
                if rows is not None:
                    rows.zero_()
                    torch.cuda.synchronize()
                    del rows
                    torch.cuda.empty_cache()
    e.close()
    for t in (x, dst):           # handed back zeroed
        t.zero_()
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default=None, metavar="SAMPLES,FORMAT", help="run this one step in this process")
    ap.add_argument("--ffts", type=int, nargs="+", default=[512, 1024, 4096])
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--step-seconds", type=int, default=STEP_SECONDS)
    a = ap.parse_args()
    if a.step is not None:
        n, fmt = a.step.split(",")
        step(int(n), fmt, a.ffts, a.calls, a.rounds)
        return 0
    for n, fmt in STEPS:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", "%d,%s" % (n, fmt), "--calls", str(a.calls), "--rounds", str(a.rounds),
               "--ffts"] + [str(f) for f in a.ffts]
        try:
            rc = subprocess.run(cmd, timeout=a.step_seconds).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            sys.stderr.write("bench_psd: step %d,%s ended with status %d; nothing more is started\n" % (n, fmt, rc))
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
