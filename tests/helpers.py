"""Shared builders for the parity tests."""
import struct

import numpy as np

from ofdm_uhd_amd import config, options


def make_cfg(mod="qpsk", N=512, occ=200, CP=128, **kw):
    opt = options.default_options(modulation=mod, fft_length=N, occupied_tones=occ, cp_length=CP)
    return config.make_cfg(opt, **kw)


def make_payloads(npkt, plen, seed=1, variant="random"):
    """benchmark_ofdm_tx payload layout: !H pktno | !H 0 | data (benchmark_ofdm_tx.py:117)."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(npkt):
        n = plen if np.isscalar(plen) else int(plen[i])
        head = struct.pack('!HH', i & 0xffff, 0)[:n]
        if variant == "random":
            body = rng.integers(0, 256, max(n - 4, 0), dtype=np.uint8).tobytes()
        else:  # reference style: chr(pktno & 0xff) * n (sensing_and_tramsmitting.py:419)
            body = bytes([i & 0xff]) * max(n - 4, 0)
        out.append((head + body)[:n])
    return out


def loopback_stream(orc, cfg, payloads, snr_db=30.0, cfo_bins=0.0, lead=None, tail=None, seed=0xC0FFEE, stream_id=0):
    """Oracle TX + channel: the ONE input array both receivers are fed."""
    N, CP = cfg.fft_length, cfg.cp_length
    lead = 2 * N if lead is None else lead
    tail = (N + CP) + 2 * N if tail is None else tail
    iq = orc.tx(cfg, payloads, lead=lead, tail=tail)
    core = iq[lead:len(iq) - tail] if tail else iq[lead:]
    psig = float(np.mean(np.abs(core) ** 2)) if len(core) else 1.0
    sigma = float(np.sqrt(psig / (10 ** (snr_db / 10.0))))
    orc.channel(iq, sigma=sigma, cfo=cfo_bins * 2 * np.pi / N, seed=seed, stream_id=stream_id)
    return iq


# The four captures of the round-2 soaks (profiles/r02_soak.txt runs C, D, F: fuzz_parity seeds 3, 7, 13) in which the
# engine's timing flags differed from the then oracle's; regenerated from those seeds by tests/soak/find_marginal.py.
# flags = what the normative evaluation of the peak detector raises, literal = gr_peak_detector_fb as a float32
# recurrence from the first sample, at = the flag one of them lacks.
MARGINAL = [
    dict(N=512, occ=296, CP=119, mod="qam64", sizes=[2328, 3699, 2717, 3663, 1986, 3229, 1811, 640, 3867], pseed=758827,
         lead=297, tail=941, cfo=0.03, rise=0.3, fall=0.1, alpha=0.0003, timeout=1000, gap_at=76648, gap_len=2877,
         sigma=0.00544704170897603, cseed=540733740, flags=315, literal=316, at=19953),
    dict(N=512, occ=468, CP=96, mod="qam16", sizes=[2611, 1662, 2261, 2020, 292, 464, 1456, 1189, 1274, 765],
         pseed=664253954, lead=1017, tail=1971, cfo=-0.2, rise=0.5, fall=0.2, alpha=0.001, timeout=2,
         sigma=0.024237971752882004, cseed=184582414, flags=402, literal=403, at=27882),
    dict(N=4096, occ=2456, CP=1440, mod="8psk", sizes=[3498, 3225, 338, 3005, 1586, 3538], pseed=925816359, lead=4937,
         tail=15477, cfo=1.3, rise=0.5, fall=0.4, alpha=0.0003, timeout=1000, gap_at=60297, gap_len=5017,
         sigma=0.001816017203964293, cseed=713355863, flags=551, literal=550, at=11306),
    dict(N=512, occ=144, CP=107, mod="bpsk", sizes=[2486, 3973, 2317, 3674, 83, 2476, 259, 1870], pseed=906997878,
         lead=397, tail=1303, cfo=0.0, rise=0.5, fall=0.2, alpha=0.0003, timeout=1000,
         sigma=0.0013143199030309916, cseed=248467222, flags=300, literal=301, at=542841),
]


def marginal_capture(orc, d):
    cfg = make_cfg(d["mod"], d["N"], d["occ"], d["CP"])
    cfg.sampler_timeout = d["timeout"]
    cfg.peak_rise, cfg.peak_fall, cfg.peak_alpha = d["rise"], d["fall"], d["alpha"]
    pay = make_payloads(len(d["sizes"]), d["sizes"], seed=d["pseed"])
    iq = orc.tx(cfg, pay)
    x = np.concatenate([np.zeros(d["lead"], np.complex64), iq, np.zeros(d["tail"], np.complex64)])
    if "gap_at" in d:
        x = np.concatenate([x[:d["gap_at"]], np.zeros(d["gap_len"], np.complex64), x[d["gap_at"]:]])
    orc.channel(x, sigma=d["sigma"], cfo=d["cfo"] * 2 * np.pi / d["N"], seed=d["cseed"])
    return cfg, x


# The peak detector's average at run starts (OFDM_TAP_RX_RUN_AVG): the grid of tests/test_detector_average.py, a subset
# of which tests/test_gpu_detector.py runs on the engine.
DETECTOR_ALPHAS = (0.0003, 0.001, 0.002, 0.005)
DETECTOR_RISE_FALL = ((0.2, 0.2), (0.5, 0.2), (0.8, 0.6), (0.3, 0.1))
DETECTOR_GEOMS = ((512, 200, 128), (2048, 1200, 512))
# float32 roundings one value of the closed form goes through outside the exact ranges, with margin: a lane's chain of 8
# fmaf, its table weight, the 64-lane scan (6), the four groups (3), the final conversion -- each relative to sums
# of |alpha * decay^j * u32| <= 1 (u32 lies in [-1, theta - 1e-3] there), the earlier tiles' summaries included
F32_ULPS = 24


def q40_bound(alpha, tile=2048):
    """Largest error the Q40 rounding of X(s) can put into the average at a run start: s - amin products, each rounded
    to 2^-40 (error <= 2^-41), carried back by 1 / decay^(Tl - s); the worst s for amin = 0, Tl = 2048.  About
    decay^-2048 * 2^-41 / (e * alpha): 1e-6 at alpha = 0.005, 1.4e-2 at 0.01."""
    d = float(np.float32(1.0) - np.float32(alpha))
    dp = np.ones(tile + 1)
    for j in range(1, tile + 1):
        dp[j] = dp[j - 1] * d
    x = np.arange(tile + 1)
    return float(np.max(x * 2.0 ** -41 / dp[tile - x]))


def run_avg_tolerance(alpha):
    """|tap - float64| <= tol * (1 + |ref|) at every run start: the Q40 bound plus the float32 roundings (F32_ULPS)."""
    return q40_bound(alpha) + F32_ULPS * 2.0 ** -24


def detector_capture(orc, N, occ, CP, snr, lead=None, npkt=4, seed=3):
    """QPSK bursts of 1026-byte packets at 0.05 bins carrier offset (the shape the issue's table was measured on)."""
    cfg = make_cfg("qpsk", N, occ, CP)
    pay = make_payloads(npkt, 1026, seed=seed)
    return loopback_stream(orc, cfg, pay, snr_db=snr, cfo_bins=0.05, lead=lead)


def noise_capture(orc, ntiles=16, seed=11):
    """Several tiles of complex white noise for N = 64: M = |P|^2 / R^2 fluctuates around 1/D there, so with
    rise / fall 0.8 / 0.6 (theta = -0.8) runs of u > theta come from the noise alone."""
    x = np.zeros(ntiles * 2048 + 333, np.complex64)
    orc.channel(x, sigma=0.05, seed=seed)
    return x
