"""Float32 against 16-bit IQ at the engine boundary, per kernel and per call: python tools/bench_iq_format.py

Device pointers: one TX + RX step per call at BASELINE configs c2 / c3 / c5 (bench.py's shapes), the two formats
alternating on one box (ROUNDS alternations of CALLS calls each), per-kernel HIP-event times from ofdm_prof_get and the
wall time of the step.  Host pointers (--host): wall time of one ofdm_tx and one ofdm_rx at c2 with 4 096 packets, where
the 16-bit format halves the bytes that cross PCIe.  Prints one JSON line per configuration."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench as B  # noqa: E402
from ofdm_uhd_amd import config, engine, options  # noqa: E402

KERNELS = ("k_chan_filter", "k_tx_mod", "k_sense", "k_sync", "k_rx_demod")


def _setup(name, packets, device_ptrs):
    c = B.CONFIGS[name]
    N, occ, CP, size = c["N"], c["occ"], c["CP"], c["size"]
    P = packets or c["packets"]
    opt = options.default_options(modulation=c["mod"], fft_length=N, occupied_tones=occ, cp_length=CP, tx_amplitude=0.25)
    ncar = len(config.carrier_map(occ, N))
    cpow = float(np.mean(np.abs(np.array(config.rotated_constellation(c["mod"]))) ** 2))
    sigma = float(np.sqrt(ncar * cpow / float(N) * 0.25 ** 2 / 10 ** (c["snr"] / 10.0)))
    engs = {}
    for fmt in ("fc32", "sc16"):
        e = engine.Engine(cfg=config.make_cfg(opt, device_ptrs=device_ptrs))
        e.set_channel(sigma=sigma, seed=0xC0FFEE, stream_id=0, lead=2 * N, tail=(N + CP) + 2 * N)
        e.set_tx_iq_format(fmt)
        e.set_rx_iq_format(fmt)
        if name == "c5":   # the sensor of predictive_sense.py fused into the receiver (bench.py's sizing)
            e.set_rx_sense(config.make_sense_cfg(N, max(0, int(round(1e-3 * 6.25e6 / N))), max(1, int(round(10e-3 * 6.25e6 / N))),
                                                 10, 1, threshold=1e-4))
        e.prof_enable(True)
        engs[fmt] = e
    return c, P, size, engs


def device_mode(name, packets, calls, rounds):
    dev = torch.device("cuda", 0)
    c, P, size, engs = _setup(name, packets, True)
    blob = torch.from_numpy(B.make_payload_blob(P, size, 0).copy()).to(dev)
    offs = np.arange(P, dtype=np.uint64) * np.uint64(size)
    lens = np.full(P, size, np.uint32)
    _, nsamp = engs["fc32"].tx_frame_count(lens)
    iq = {"fc32": torch.empty(nsamp * 2, dtype=torch.float32, device=dev),
          "sc16": torch.empty(nsamp * 2, dtype=torch.int16, device=dev)}
    out = torch.empty(P * size + 4096, dtype=torch.uint8, device=dev)
    res = {f: {"step_ms": [], "crc_ok": None, **{k: [] for k in KERNELS}} for f in engs}

    def step(f):
        e = engs[f]
        n = e.tx_device(blob.data_ptr(), offs, lens, iq[f].data_ptr(), nsamp, wait=False)
        _, _, _, ok = e.rx_device(iq[f].data_ptr(), n, out.data_ptr(), out.numel(), P + 1024)
        return int(ok.sum())

    for f in engs:
        step(f)
        step(f)
    for _ in range(rounds):
        for f in ("fc32", "sc16"):
            e = engs[f]
            for _ in range(calls):
                e.prof_reset()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res[f]["crc_ok"] = step(f)
                res[f]["step_ms"].append(1e3 * (time.perf_counter() - t0))
                pr = e.prof()
                for k in KERNELS:
                    res[f][k].append(pr[k][0])
    for e in engs.values():
        e.close()
    summ = {f: {k: (round(float(np.median(v)), 4), round(float(np.min(v)), 4), round(float(np.max(v)), 4))
                for k, v in r.items() if k != "crc_ok"} for f, r in res.items()}
    print(json.dumps({"mode": "device", "config": name, "packets": P, "samples": int(nsamp), "calls": calls * rounds,
                      "crc_ok": {f: res[f]["crc_ok"] for f in res}, "ms_median_min_max": summ}), flush=True)


def host_mode(packets, calls, rounds):
    c, P, size, engs = _setup("c2", packets, False)
    pay = [bytes(r) for r in B.make_payload_blob(P, size, 0).reshape(P, size)]
    res = {f: {"tx_ms": [], "rx_ms": [], "crc_ok": None} for f in engs}
    for f, e in engs.items():
        e.rx(e.tx(pay[:64]))
    for _ in range(rounds):
        for f in ("fc32", "sc16"):
            e = engs[f]
            for _ in range(calls):
                t0 = time.perf_counter()
                x = e.tx(pay)
                t1 = time.perf_counter()
                pk = e.rx(x)
                t2 = time.perf_counter()
                res[f]["tx_ms"].append(1e3 * (t1 - t0))
                res[f]["rx_ms"].append(1e3 * (t2 - t1))
                res[f]["crc_ok"] = sum(ok for ok, _ in pk)
    for e in engs.values():
        e.close()
    summ = {f: {k: (round(float(np.median(v)), 3), round(float(np.min(v)), 3), round(float(np.max(v)), 3))
                for k, v in r.items() if k != "crc_ok"} for f, r in res.items()}
    print(json.dumps({"mode": "host (Engine.tx / Engine.rx wall time, NumPy packing included)", "config": "c2", "packets": P,
                      "calls": calls * rounds, "crc_ok": {f: res[f]["crc_ok"] for f in res}, "ms_median_min_max": summ}),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c2,c3,c5")
    ap.add_argument("--packets", type=int, default=None, help="packets per step (default: bench.py's per config)")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--host", action="store_true", help="also the host-pointer measurement (c2, --host-packets)")
    ap.add_argument("--host-packets", type=int, default=4096)
    a = ap.parse_args()
    for name in [s for s in a.configs.split(",") if s]:
        device_mode(name, a.packets, a.calls, a.rounds)
    if a.host:
        host_mode(a.host_packets, a.calls, a.rounds)


if __name__ == "__main__":
    main()
