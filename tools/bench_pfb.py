"""The polyphase-FFT channeliser (k_pfb) against the DDC bank (k_ddc_bank) and a device copy on one MI355X:
python tools/bench_pfb.py

Device pointers, the stream of tools/bench_ddc_bank.py: M times the sample count of bench.py's C2 stream of --packets
packets, random samples, float32 and 16-bit IQ.  Shapes: M=4 / 31 taps, M=8 / 155 taps and M=32 / 155 taps with all M
channels kept, and M=8 / 155 taps with two channels kept (what unselected rows save).  Per shape and format, after two
warm-up calls per variant: ROUNDS alternations of [CALLS calls of k_pfb, CALLS calls of k_ddc_bank at K = 8 with
fc = c / M, CALLS device copies]; k_pfb's HIP-event time from ofdm_pfb_last_ms, k_ddc_bank's from
ofdm_ddc_bank_last_ms, the copy's from torch events.  The yardsticks are the bank -- existing code this tool does not
touch -- and a torch copy that moves the bytes k_pfb must move (8 or 4 B in per input sample, 8 nsel / M out: half of
them read, half written).  Prints one JSON line per shape and format: median / min / max ms, TB/s, and the ratios to each
yardstick, by medians and for the least favourable pairing of single runs (slowest k_pfb call, fastest yardstick call)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench as B  # noqa: E402
from ofdm_uhd_amd import config, ddc, engine, options, pfb  # noqa: E402

# M, (occupied fraction, transition) the prototype is designed for, channels kept (None: all).  M = 32 takes the 155 taps
# of M = 8: the shape is timed, not the filter
SHAPES = ((4, (200 / 512.0, None), None), (8, (48 / 64.0, None), None), (32, (48 / 64.0, 1 / 64.0), None),
          (8, (48 / 64.0, None), (1, 6)))
BANK_LINKS = 8


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
        taps = pfb.design(M, *proto)
        chans = list(range(M)) if sel is None else list(sel)
        K = len(chans)
        for fmt in ("fc32", "sc16"):
            e = engine.Engine(cfg=config.make_cfg(opt, device_ptrs=True))
            e.set_rx_iq_format(fmt)
            e.prof_enable(True)
            _, nsamp = e.tx_frame_count(np.full(a.packets, c["size"], np.uint32))
            nsamp = int(nsamp)
            nin = nsamp * M
            nout = (nin + M - 1) // M
            g = torch.Generator(device=dev)
            g.manual_seed(M)
            if fmt == "fc32":
                x = torch.randn(2 * nin, dtype=torch.float32, device=dev, generator=g)
            else:
                x = torch.randint(-32768, 32768, (2 * nin,), dtype=torch.int16, device=dev, generator=g)
            stride = nsamp + 2
            y = torch.empty(2 * max(K, BANK_LINKS) * stride, dtype=torch.float32, device=dev)
            in_bytes = nin * (8 if fmt == "fc32" else 4)
            moved = in_bytes + 8 * K * nout
            # the copy reads moved / 2 bytes and writes as many; where the input and the output have that size they serve
            if in_bytes == moved // 2:
                src, dst = x.view(torch.uint8)[:moved // 2], y.view(torch.uint8)[:moved // 2]
            else:
                src = torch.zeros(moved // 2, dtype=torch.uint8, device=dev)
                dst = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            e.set_pfb(pfb.pfb_cfg(M, chans, taps=taps))
            e.set_ddc_bank(ddc.bank_cfg(M, [((i % M) / float(M) + 0.5) % 1.0 - 0.5 for i in range(BANK_LINKS)], taps=taps))

            def chan():
                e.pfb_reset(0)
                assert e.pfb_device(x.data_ptr(), nin, y.data_ptr(), stride, stride) == nout
                return e.pfb_last_ms()

            def bank():
                e.ddc_bank_reset(0)
                assert e.ddc_bank_device(x.data_ptr(), nin, y.data_ptr(), stride, stride) == nout
                return e.ddc_bank_last_ms()

            def copy():
                ev[0].record()
                dst.copy_(src)
                ev[1].record()
                torch.cuda.synchronize()
                return ev[0].elapsed_time(ev[1])

            variants = (("k_pfb", chan), ("k_ddc_bank", bank), ("copy", copy))
            for _, f in variants:
                for _ in range(2):
                    f()
            ms = {name: [] for name, _ in variants}
            for _ in range(a.rounds):
                for name, f in variants:
                    ms[name] += [f() for _ in range(a.calls)]
            med = {name: float(np.median(v)) for name, v in ms.items()}
            res = {name + "_ms": _stats(v) for name, v in ms.items()}
            res["k_pfb_TBps"] = round(moved / med["k_pfb"] * 1e-9, 3)
            res["k_ddc_bank_TBps"] = round((in_bytes + 8 * BANK_LINKS * nout) / med["k_ddc_bank"] * 1e-9, 3)
            res["copy_TBps"] = round(moved / med["copy"] * 1e-9, 3)
            for name in ("k_ddc_bank", "copy"):
                res["pfb_over_%s_median" % name] = round(med["k_pfb"] / med[name], 4)
                res["pfb_over_%s_worst" % name] = round(float(np.max(ms["k_pfb"])) / float(np.min(ms[name])), 4)
            print(json.dumps({"M": M, "ntaps": len(taps), "nsel": K, "bank_links": BANK_LINKS, "format": fmt,
                              "input_samples": nin, "outputs_per_channel": nout, "bytes_moved": moved,
                              "calls": a.calls * a.rounds, "ms_median_min_max": res}), flush=True)
            e.close()
            del x, y, src, dst
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
