"""The signal field's kernels (k_sig_encode, k_sig_decode hard and soft) on one MI355X, next to a device copy of the
same bytes and next to k_soft_demap for the same packets, one job:
python tools/bench_sig.py

Device pointers; --packets (16 384) blocks of --size (192) random body bytes behind the fields of the 50 valid words
in turn (PCG64 seed 0x0516).  k_sig_encode makes the blocks; they go through ofdm_tx with its channel at 30 dB and
through ofdm_rx with soft values on, which gives k_soft_demap's time for these packets (ofdm_rx_soft_last_ms); then
k_sig_decode<soft> runs on the handle's own values (ofdm_rx_sig_decode_soft) and k_sig_decode<hard> on the bytes ofdm_rx
delivered.  Every decoded word must be the word sent.  After two warm-ups: ROUNDS alternations of CALLS calls of every
variant, the kernels' HIP-event times from ofdm_sig_last_ms; the copies are torch device-to-device copies between two
buffers of the bytes the kernel touches (encode: the blocks, read and written; decode: the fields, 12 or 96 bytes per
packet), timed with events.  Prints one JSON line: median / min / max ms per variant, ns per packet, and every sig time
as a ratio to k_soft_demap and to its copy."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from ofdm_uhd_amd import config, engine, options, sig  # noqa: E402


def _stats(v):
    return [round(float(np.median(v)), 4), round(float(np.min(v)), 4), round(float(np.max(v)), 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=16384)
    ap.add_argument("--size", type=int, default=192)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    P, size = a.packets, a.size
    bsize = sig.FIELD_BYTES + size
    opt = options.default_options(modulation="qpsk", fft_length=512, occupied_tones=200, cp_length=128, tx_amplitude=0.25)
    e = engine.Engine(cfg=config.make_cfg(opt, device_ptrs=True))
    e.prof_enable(True)
    rng = np.random.Generator(np.random.PCG64(0x0516))
    valid = [c.word for c in sig.all_codings()]
    words = np.array([valid[k % len(valid)] for k in range(P)], np.uint16)
    d_body = torch.from_numpy(rng.integers(0, 256, P * size, dtype=np.uint8)).to(dev)
    offs, lens = np.arange(P, dtype=np.uint64) * np.uint64(size), np.full(P, size, np.uint32)
    boffs, blens = np.arange(P, dtype=np.uint64) * np.uint64(bsize), np.full(P, bsize, np.uint32)
    d_blk = torch.empty(P * bsize, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()            # the inputs are torch's work; the engine reads them on streams of its own

    def encode():
        e.sig_encode_device(words, d_body.data_ptr(), offs, lens, d_blk.data_ptr(), d_blk.numel())
        return e.sig_last_ms()

    encode()
    nmap = len(config.carrier_map(200, 512))
    psig = nmap / 512.0 * 0.25 ** 2
    e.set_channel(sigma=float(np.sqrt(psig / 10 ** 3.0)), cfo=0.0, seed=0xC0FFEE, stream_id=0, lead=1024, tail=640 + 1024)
    _, nsamp = e.tx_frame_count(blens)
    d_iq = torch.empty(nsamp * 2, dtype=torch.float32, device=dev)
    n = e.tx_device(d_blk.data_ptr(), boffs, blens, d_iq.data_ptr(), nsamp)
    d_out = torch.empty(P * bsize + 4096, dtype=torch.uint8, device=dev)
    e.set_rx_soft(True)
    state = {}

    def rx():
        npk, off, ln, ok = e.rx_device(d_iq.data_ptr(), n, d_out.data_ptr(), d_out.numel(), P + 1024)
        assert npk == P, (npk, P)
        state["off"], state["ln"], state["crc_ok"] = off[:npk].copy(), ln[:npk].copy(), int(ok.sum())
        return e.rx_soft_last_ms()

    def decode_soft():
        word, margin = e.rx_sig_decode_soft_device()
        state["soft"] = (word, margin)
        return e.sig_last_ms()

    def decode_hard():
        word, margin = e.sig_decode_device(d_out.data_ptr(), state["off"], state["ln"])
        state["hard"] = (word, margin)
        return e.sig_last_ms()

    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    copies = {}

    def copy_of(nbytes):
        if nbytes not in copies:
            copies[nbytes] = (torch.empty(nbytes, dtype=torch.uint8, device=dev), torch.empty(nbytes, dtype=torch.uint8, device=dev))
        src, dst = copies[nbytes]
        ev[0].record()
        dst.copy_(src)
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1])

    variants = [("k_soft_demap", rx), ("k_sig_decode soft", decode_soft), ("k_sig_decode hard", decode_hard), ("k_sig_encode", encode),
                ("copy of the fields' values (96 B per packet)", lambda: copy_of(96 * P)),
                ("copy of the fields' bytes (12 B per packet)", lambda: copy_of(12 * P)),
                ("copy of the blocks' bytes", lambda: copy_of(P * bsize))]
    for _, f in variants:
        for _ in range(2):
            f()
    for k in ("soft", "hard"):
        assert np.array_equal(state[k][0], words), k                   # every field decodes to the word sent
    ms = {v: [] for v, _ in variants}
    for _ in range(a.rounds):
        for v, f in variants:
            ms[v] += [f() for _ in range(a.calls)]
    med = {v: float(np.median(t)) for v, t in ms.items()}
    sigs = ("k_sig_decode soft", "k_sig_decode hard", "k_sig_encode")
    copy_for = dict(zip(sigs, [v for v, _ in variants[4:]]))
    print(json.dumps({"packets": P, "body_bytes": size, "block_bytes": bsize, "calls": a.calls * a.rounds, "crc_ok": state["crc_ok"],
                      "min_margin": {k: int(state[k][1].min()) for k in ("soft", "hard")},
                      "ms_median_min_max": {v: _stats(t) for v, t in ms.items()},
                      "ns_per_packet": {v: round(med[v] * 1e6 / P, 3) for v in med},
                      "over_k_soft_demap": {v: round(med[v] / med["k_soft_demap"], 4) for v in sigs},
                      "over_its_copy": {v: round(med[v] / med[copy_for[v]], 3) for v in sigs}}), flush=True)
    e.close()


if __name__ == "__main__":
    main()
