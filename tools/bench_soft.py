"""Soft-decision receive (k_soft_demap, ofdm_rx_fec_decode_soft) on one MI355X, next to what it follows and feeds:
python tools/bench_soft.py

Device pointers, the C2 configuration (N 512 / occ 200 / CP 128, QPSK, 30 dB), --packets coded blocks of 1 026 payload
bytes (2 062 bytes on the air each).  After one warm-up per variant, ROUNDS alternations of [hard call, soft call]:
  - wall time of ofdm_rx with the option off and on (the soft call adds the tap pass, the CSI instantiation and
    k_soft_demap), device synchronised around each call;
  - k_soft_demap's HIP-event time (ofdm_rx_soft_last_ms) and k_rx_demod's (ofdm_prof_get) in the same soft calls;
  - a device copy of the bytes k_soft_demap reads and writes (8 per carrier and 8 per equaliser entry in, 1 per value
    out), torch events;
  - k_fec_decode<false> on the delivered bytes against k_fec_decode<true> on the handle's values (ofdm_fec_last_ms).
Then, with --grid, the link of tests/test_gpu_soft.py (16-QAM, two paths) over a 1 dB grid: packets decoded to the
payload sent, hard against soft, --grid-packets per level, and the share of values that are clipped (|v| = 127) or
erased (v = 0).  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from ofdm_uhd_amd import config, engine, fec, multipath, ofdm, options  # noqa: E402


def _stats(v):
    return [round(float(np.median(v)), 4), round(float(np.min(v)), 4), round(float(np.max(v)), 4)]


def kernels(a):
    dev = torch.device("cuda", 0)
    P, size = a.packets, a.size
    csize = fec.coded_len(size)
    opt = options.default_options(modulation="qpsk", fft_length=512, occupied_tones=200, cp_length=128, tx_amplitude=0.25)
    e = engine.Engine(cfg=config.make_cfg(opt, device_ptrs=True))
    e.prof_enable(True)
    rng = np.random.Generator(np.random.PCG64(0x50F7))
    d_pay = torch.from_numpy(rng.integers(0, 256, P * size, dtype=np.uint8)).to(dev)
    d_coded = torch.empty(P * csize, dtype=torch.uint8, device=dev)
    offs, lens = np.arange(P, dtype=np.uint64) * np.uint64(size), np.full(P, size, np.uint32)
    coffs, clens = np.arange(P, dtype=np.uint64) * np.uint64(csize), np.full(P, csize, np.uint32)
    e.fec_encode_device(d_pay.data_ptr(), offs, lens, d_coded.data_ptr(), d_coded.numel())
    nmap = len(config.carrier_map(200, 512))
    psig = nmap / 512.0 * 0.25 ** 2
    e.set_channel(sigma=float(np.sqrt(psig / 10 ** 3.0)), cfo=0.0, seed=0xC0FFEE, stream_id=0, lead=1024, tail=640 + 1024)
    _, nsamp = e.tx_frame_count(clens)
    d_iq = torch.empty(nsamp * 2, dtype=torch.float32, device=dev)
    n = e.tx_device(d_coded.data_ptr(), coffs, clens, d_iq.data_ptr(), nsamp)
    d_out = torch.empty(P * csize + 4096, dtype=torch.uint8, device=dev)
    d_dec = torch.empty(P * size + 4096, dtype=torch.uint8, device=dev)
    # what k_soft_demap moves: per packet its carriers' slicer inputs and one equaliser row in, its values out
    ncar = -(-8 * (4 + csize) // 2)
    moved = P * (8 * ncar + 8 * nmap + 8 * csize)
    d_a = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
    d_b = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = {k: [] for k in ("rx_hard_wall", "rx_soft_wall", "k_soft_demap", "k_rx_demod_in_soft_call", "k_rx_demod_in_hard_call",
                          "copy_same_bytes", "k_fec_decode_hard", "k_fec_decode_soft")}
    state = {}

    def call(soft, keep):
        e.set_rx_soft(True if soft else None)
        e.prof_reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        npk, off, ln, ok = e.rx_device(d_iq.data_ptr(), n, d_out.data_ptr(), d_out.numel(), P + 1024)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        demod = e.prof()["k_rx_demod"][0]
        assert npk == P, (npk, P)
        if soft:
            sd = e.rx_soft_last_ms()
            _, dok, corr = e.rx_fec_decode_soft_device(d_dec.data_ptr(), d_dec.numel())
            fs = e.fec_last_ms()
            state["soft_ok"], state["soft_corrected"] = int(dok.sum()), int(corr.sum())
        else:
            _, dok, corr = e.fec_decode_device(d_out.data_ptr(), off[:npk].copy(), ln, d_dec.data_ptr(), d_dec.numel())
            fh = e.fec_last_ms()
            state["hard_ok"], state["hard_corrected"], state["crc_ok"] = int(dok.sum()), int(corr.sum()), int(ok.sum())
        if keep:
            ms["rx_soft_wall" if soft else "rx_hard_wall"].append(wall)
            ms["k_rx_demod_in_soft_call" if soft else "k_rx_demod_in_hard_call"].append(demod)
            if soft:
                ms["k_soft_demap"].append(sd)
                ms["k_fec_decode_soft"].append(fs)
            else:
                ms["k_fec_decode_hard"].append(fh)

    def copy(keep):
        ev[0].record()
        d_b.copy_(d_a)
        ev[1].record()
        torch.cuda.synchronize()
        if keep:
            ms["copy_same_bytes"].append(ev[0].elapsed_time(ev[1]))

    for keep in [False] + [True] * a.rounds:
        call(False, keep)
        call(True, keep)
        copy(keep)
    e.close()
    med = {k: float(np.median(v)) for k, v in ms.items()}
    return {"packets": P, "payload_bytes": size, "coded_bytes": csize, "rounds": a.rounds, "values": P * 8 * csize,
            "bytes_moved_by_k_soft_demap": moved, "ms_median_min_max": {k: _stats(v) for k, v in ms.items()},
            "soft_demap_over_copy": round(med["k_soft_demap"] / med["copy_same_bytes"], 2),
            "soft_demap_over_demod": round(med["k_soft_demap"] / med["k_rx_demod_in_soft_call"], 3),
            "soft_call_over_hard_call": round(med["rx_soft_wall"] / med["rx_hard_wall"], 3),
            "decode_soft_over_hard": round(med["k_fec_decode_soft"] / med["k_fec_decode_hard"], 3), **state}


def grid(a):
    """The link test's channel over a 1 dB grid: packets that come back as sent, hard against soft."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import soft_cases as sc
    opt = options.default_options(modulation=sc.LINK_MOD, fft_length=sc.LINK_N, occupied_tones=sc.LINK_OCC, cp_length=sc.LINK_CP)
    rng = np.random.default_rng(2024)
    pay = [rng.integers(0, 256, sc.LINK_SIZES[i % 6], dtype=np.uint8).tobytes() for i in range(a.grid_packets)]
    mod = ofdm.ofdm_mod(opt, pad_for_usrp=False, fec=True)
    hard, soft = ofdm.ofdm_demod(opt, fec=True), ofdm.ofdm_demod(opt, fec=True, soft=True)
    for p in pay:
        mod.send_pkt(p)
    iq = mod.flush()
    psig = float(np.mean(np.abs(iq.astype(np.complex128)) ** 2))
    rows = []
    for snr in range(a.grid_lo, a.grid_hi + 1):
        ch = mod.engine()
        ch.set_multipath(sc.link_channel_cfg(float(snr), psig))
        ch.multipath_reset(0)
        y = ch.multipath(sc.link_air(iq))
        sent = set(pay)
        h = sum(1 for ok, p in hard.work(y) if ok and p in sent)
        s = sum(1 for ok, p in soft.work(y) if ok and p in sent)
        v = np.concatenate(soft.last_soft + [np.zeros(0, np.int8)]).astype(np.int32)
        rows.append({"snr_db": snr, "delivered": len(soft.last_soft), "hard_ok": h, "soft_ok": s,
                     "clipped": round(float(np.mean(np.abs(v) == 127)), 4) if len(v) else None,
                     "erased": round(float(np.mean(v == 0)), 4) if len(v) else None})
    for o in (mod, hard, soft):
        o.engine().close()
    return {"sent": len(pay), "paths": [[d, [round(g.real, 4), round(g.imag, 4)]] for d, g in sc.LINK_PATHS], "levels": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=8192)
    ap.add_argument("--size", type=int, default=1026)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--grid", action="store_true")
    ap.add_argument("--grid-packets", type=int, default=24)
    ap.add_argument("--grid-lo", type=int, default=8)
    ap.add_argument("--grid-hi", type=int, default=20)
    a = ap.parse_args()
    out = {"kernels": kernels(a)}
    if a.grid:
        out["grid"] = grid(a)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
