"""The coded-link kernels (k_fec_encode, k_fec_decode) on one MI355X, next to the demodulator they follow and to a device
copy of the decoder's input:
python tools/bench_fec.py

Device pointers; 65 536 blocks of 1 026 payload bytes (the C2 packet), 16 interleaver columns.  After two warm-ups per
variant: ROUNDS alternations of [CALLS encodes, CALLS hard decodes, CALLS device copies of the coded bytes]; the
kernels' HIP-event times from ofdm_fec_last_ms (the decoder's covers all its slices), the copy's from torch events.
Then the receiver at the C2 configuration (N 512 / occ 200 / CP 128, QPSK, 30 dB) on the same number of 1 026-byte
packets, and on the 2 062-byte coded blocks as packets (what a coded link really demodulates): k_rx_demod's mean time per
call from ofdm_prof_get.  Prints one JSON line: median / min / max ms per variant, payload GB/s of both kernels, ns per
trellis step and block, and the decoder's ratio to k_rx_demod and to the copy."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from ofdm_uhd_amd import config, engine, fec, options  # noqa: E402


def _stats(v):
    return [round(float(np.median(v)), 4), round(float(np.min(v)), 4), round(float(np.max(v)), 4)]


def _demod_ms(eng, dev, d_blob, P, size, steps):
    """Mean k_rx_demod time per ofdm_rx over ``steps`` TX -> RX loopbacks of P packets of ``size`` bytes."""
    offs = np.arange(P, dtype=np.uint64) * np.uint64(size)
    lens = np.full(P, size, np.uint32)
    _, nsamp = eng.tx_frame_count(lens)
    d_iq = torch.empty(nsamp * 2, dtype=torch.float32, device=dev)
    d_out = torch.empty(P * size + 4096, dtype=torch.uint8, device=dev)
    okc = 0
    for i in range(steps + 1):
        if i == 1:
            eng.prof_reset()                     # the first pass warms up
        n = eng.tx_device(d_blob.data_ptr(), offs, lens, d_iq.data_ptr(), nsamp)
        npk, _, _, ok = eng.rx_device(d_iq.data_ptr(), n, d_out.data_ptr(), d_out.numel(), P + 1024)
        okc = int(ok.sum())
    ms, calls = eng.prof()["k_rx_demod"]
    del d_iq, d_out
    torch.cuda.empty_cache()
    return ms / max(calls, 1), okc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=65536)
    ap.add_argument("--size", type=int, default=1026)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--demod-steps", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    P, size = a.blocks, a.size
    csize = fec.coded_len(size)
    opt = options.default_options(modulation="qpsk", fft_length=512, occupied_tones=200, cp_length=128, tx_amplitude=0.25)
    cfg = config.make_cfg(opt, device_ptrs=True)
    e = engine.Engine(cfg=cfg)
    e.prof_enable(True)
    rng = np.random.Generator(np.random.PCG64(0x0FEC))
    d_pay = torch.from_numpy(rng.integers(0, 256, P * size, dtype=np.uint8)).to(dev)
    d_coded = torch.empty(P * csize, dtype=torch.uint8, device=dev)
    d_dec = torch.empty(P * size, dtype=torch.uint8, device=dev)
    d_copy = torch.empty(P * csize, dtype=torch.uint8, device=dev)
    offs = np.arange(P, dtype=np.uint64) * np.uint64(size)
    lens = np.full(P, size, np.uint32)
    coffs = np.arange(P, dtype=np.uint64) * np.uint64(csize)
    clens = np.full(P, csize, np.uint32)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    state = {}

    def encode():
        e.fec_encode_device(d_pay.data_ptr(), offs, lens, d_coded.data_ptr(), d_coded.numel())
        return e.fec_last_ms()

    def decode():
        _, ok, corr = e.fec_decode_device(d_coded.data_ptr(), coffs, clens, d_dec.data_ptr(), d_dec.numel())
        state["ok"], state["corrected"] = int(ok.sum()), int(corr.sum())
        return e.fec_last_ms()

    def copy():
        ev[0].record()
        d_copy.copy_(d_coded)
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1])

    variants = (("k_fec_encode", encode), ("k_fec_decode", decode), ("copy", copy))
    for _, f in variants:
        for _ in range(2):
            f()
    assert state["ok"] == P and state["corrected"] == 0 and torch.equal(d_dec, d_pay)
    ms = {v: [] for v, _ in variants}
    for _ in range(a.rounds):
        for v, f in variants:
            ms[v] += [f() for _ in range(a.calls)]
    med = {v: float(np.median(t)) for v, t in ms.items()}

    # the demodulator at C2 on the same number of packets, and on the coded blocks as packets
    psig = len(config.carrier_map(200, 512)) / 512.0 * 0.25 ** 2
    lead, tail = 2 * 512, 640 + 2 * 512
    e.set_channel(sigma=float(np.sqrt(psig / 10 ** 3.0)), cfo=0.0, seed=0xC0FFEE, stream_id=0, lead=lead, tail=tail)
    demod_ms, ok_plain = _demod_ms(e, dev, d_pay, P, size, a.demod_steps)
    demod_coded_ms, ok_coded = _demod_ms(e, dev, d_coded, P, csize, a.demod_steps)
    steps = 8 * (size + 4) + 6
    res = {v + "_ms": _stats(t) for v, t in ms.items()}
    print(json.dumps({
        "blocks": P, "payload_bytes": size, "coded_bytes": csize, "trellis_steps": steps, "interleave_cols": 16,
        "calls": a.calls * a.rounds, "ms_median_min_max": res,
        "encode_payload_GBps": round(P * size / med["k_fec_encode"] * 1e-6, 2),
        "decode_payload_GBps": round(P * size / med["k_fec_decode"] * 1e-6, 2),
        "decode_ns_per_block": round(med["k_fec_decode"] * 1e6 / P, 1),
        "decode_ps_per_step_and_block": round(med["k_fec_decode"] * 1e9 / P / steps, 2),
        "k_rx_demod_ms_same_packets": round(demod_ms, 4), "crc_ok_same_packets": ok_plain,
        "k_rx_demod_ms_coded_packets": round(demod_coded_ms, 4), "crc_ok_coded_packets": ok_coded,
        "decode_over_demod_same_packets": round(med["k_fec_decode"] / demod_ms, 3),
        "decode_over_demod_coded_packets": round(med["k_fec_decode"] / demod_coded_ms, 3),
        "encode_over_demod_same_packets": round(med["k_fec_encode"] / demod_ms, 3),
        "decode_over_copy": round(med["k_fec_decode"] / med["copy"], 2),
        "copy_TBps": round(2 * P * csize / med["copy"] * 1e-9, 3)}), flush=True)
    e.close()


if __name__ == "__main__":
    main()
